"""
Joint NeRF + camera-pose training step — drop-in for ShawnnnLiu/Robust-NeRF
``noisy_src/train_pose_opt.py`` (the pieces on the hot path).

* ``CameraPoseParameters`` keeps the reference's parameterisation (axis-angle
  rotation deltas and translation deltas, both (N,3), zero-initialised;
  ``R = R_delta(w) R_init``, ``t = t_init + dt``) and its ``theta < 1e-6 -> I``
  quirk that blocks dL/dw at w = 0 (train_pose_opt.py:143-161; Appendix A.1).
  ``get_poses`` is one HIP kernel (``nr_se3_poses_fwd``/``_bwd``).  The two deltas
  are views of one flat 16-B-aligned buffer, so the pose Adam is one fused launch.
* ``train_step_with_poses`` follows train_pose_opt.py:290-411 step for step: poses ->
  rays (one gather kernel) -> render -> MSE coarse+fine -> L2 pose regularisers ->
  backward -> separate clips (coarse 1.0, fine 1.0, poses 0.1) -> the two optimizers.
* ``train_with_pose_optimization(config, noise_config, init_mode, ...)`` is the
  reference loop (train_pose_opt.py:613-1054): noisy or clean initial poses, the pose
  Adam and its LambdaLR only after ``pose_opt_delay``, one CSV row per iteration,
  validation + pose errors + checkpoint every ``val_every``, checkpoints every
  ``save_every``, the final evaluation and checkpoint, ``final_poses.pt`` and
  ``summary.json``.  The step is ``engine.PoseTrainer`` (HIP, no host syncs); what the
  loop shares with ``train.train`` around the step is ``run``'s.  Under
  ``torchrun`` it is data parallel exactly like ``train.train``: identical global draws
  on every rank, contiguous slices, network and pose gradients averaged over RCCL.
  ``graph=True`` (``--graph``) replays the step from hipGraphs after iteration 0
  (``engine.GraphedPoseTrainer``: one graph for frozen poses, one for optimising, the
  pixel batch gathered straight into their static inputs), bit-identical to eager; it
  pays below 1,024 rays per GPU.
* ``c2f=(start, end)`` (``--c2f START END``) anneals both positional encodings coarse to
  fine as BARF does (Lin et al., ICCV 2021): ``pe_window_weights(c2f_alpha(...))`` per
  iteration, folded into the MLP's weight images (``NeRF.set_pe_window``).  The reference
  lists it as future work; it is meant for ``fixed_small_angle=True``
  (``--fixed_small_angle``), where the rotation gradients are live.
* ``learn_focal="shared" | "xy"`` (``--learn_focal``, with ``--focal_init_scale``) learns the
  focal length with the poses as NeRF-- does (Wang et al. 2021; the reference's other
  future-work item): ``CameraIntrinsics`` holds a log scale on the dataset's focal length,
  the ray kernels read (fx, fy) from device memory (``nr_rays_from_pixels_intr_fwd/bwd``), so
  the graphs follow it, and it shares the pose Adam, schedule and delay.
* ``learn_principal`` / ``learn_distortion`` / ``lens_init`` (``--learn_principal``,
  ``--learn_distortion``, ``--lens_init K1 K2``) learn the rest of the lens the same way: the
  principal point and two radial terms of the NeRF-- / SCNeRF ray-side model, six numbers
  that the ray kernels read from device memory (``nr_rays_from_pixels_lens_fwd/bwd``), each
  parameter a clip group of its own; ``lens_init`` alone holds a known calibration
  (DESIGN.md §4c-2).
"""

from __future__ import annotations

import math
from datetime import datetime
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .config import RenderConfig
from .config import NeRFConfig
from .data import BlenderData, load_blender_data
from .data_pose_opt import PixelBatch, PixelSampler, create_pixel_dataset
from .engine import GraphedPoseTrainer, PoseTrainer
from .logger import ExperimentLogger, ValidationMetrics
from .metrics import compute_psnr
from .model import NeRF
from .noise import NoiseConfig, add_noise_to_poses, compute_pose_error
from .optim import FusedAdam, clip_grad_norm_
from .rendering import NeRFRenderer, render_rays
from .run import (LENS_COLUMNS, IterationLog, add_common_args, base_checkpoint, create_nerf_for, draw_randoms, due,  # noqa: F401
                  evaluate_views, loss_line, open_run, run_cli, set_seed, slice_for_rank, write_checkpoint,
                  write_experiment_config)
from .train import render_image


def pe_window_weights(alpha: float, num_freqs: int) -> List[float]:
    """BARF's coarse-to-fine window (Lin et al., ICCV 2021, eq. 14): the weight of
    frequency k at progress ``alpha`` in [0, num_freqs],
    ``w_k = (1 - cos(pi * clamp(alpha - k, 0, 1))) / 2``, in fp64."""
    return [(1.0 - math.cos(math.pi * min(max(alpha - k, 0.0), 1.0))) / 2.0 for k in range(num_freqs)]


def c2f_alpha(iteration: int, num_iterations: int, start: float, end: float, num_freqs: int) -> float:
    """``alpha = L * clamp((p - start) / (end - start), 0, 1)`` with ``p = iteration /
    num_iterations``: no frequency before ``start``, all of them from ``end`` on."""
    if not end > start:
        raise ValueError(f"c2f: end ({end}) must be greater than start ({start})")
    p = iteration / num_iterations
    return num_freqs * min(max((p - start) / (end - start), 0.0), 1.0)


class CameraPoseParameters(nn.Module):
    """Reference train_pose_opt.py:53-271."""

    def __init__(self, initial_poses: torch.Tensor, learn_rotation: bool = True, learn_translation: bool = True,
                 fixed_small_angle: bool = False):
        super().__init__()
        self.n_poses = initial_poses.shape[0]
        self.learn_rotation = learn_rotation
        self.learn_translation = learn_translation
        # opt-in: exact Rodrigues derivative at w = 0 instead of the reference's blocked gradient
        self.fixed_small_angle = fixed_small_angle
        self.register_buffer("initial_poses", initial_poses.clone().float().contiguous())
        dev = initial_poses.device
        flat = torch.zeros(2 * self.n_poses * 3 + 4, device=dev)  # 16-B aligned halves
        off_t = ((self.n_poses * 3 + 3) // 4) * 4
        rot = flat[:self.n_poses * 3].view(self.n_poses, 3)
        trans = flat[off_t:off_t + self.n_poses * 3].view(self.n_poses, 3)
        if learn_rotation:
            self.rotation_deltas = nn.Parameter(rot)
        else:
            self.register_buffer("rotation_deltas", rot)
        if learn_translation:
            self.translation_deltas = nn.Parameter(trans)
        else:
            self.register_buffer("translation_deltas", trans)

    def _skew_symmetric(self, v: torch.Tensor) -> torch.Tensor:
        """Reference train_pose_opt.py:165-184."""
        z = torch.zeros(v.shape[0], device=v.device)
        return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], -1), torch.stack([v[:, 2], z, -v[:, 0]], -1),
                            torch.stack([-v[:, 1], v[:, 0], z], -1)], dim=1)

    def axis_angle_to_rotation_matrix(self, axis_angle: torch.Tensor) -> torch.Tensor:
        """Reference train_pose_opt.py:122-163, on the HIP SE(3) kernel (identity base pose)."""
        shape = axis_angle.shape[:-1]
        aa = axis_angle.reshape(-1, 3).float()
        eye = torch.eye(4, device=aa.device).expand(aa.shape[0], 4, 4).contiguous()
        R = ops.se3_poses(eye, aa, None, None, fixed_small_angle=self.fixed_small_angle)[:, :3, :3]
        return R.reshape(*shape, 3, 3)

    def get_poses(self, indices: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Reference train_pose_opt.py:186-226 -> (N or len(indices), 4, 4)."""
        return ops.se3_poses(self.initial_poses, self.rotation_deltas if self.learn_rotation else None,
                             self.translation_deltas if self.learn_translation else None, indices,
                             fixed_small_angle=self.fixed_small_angle)

    def get_all_poses(self) -> torch.Tensor:
        return self.get_poses()

    def compute_pose_errors(self, ground_truth_poses: torch.Tensor,
                            indices: Optional[torch.Tensor] = None) -> Dict[str, float]:
        """Reference train_pose_opt.py:232-271."""
        with torch.no_grad():
            cur = self.get_poses(indices).cpu()
        gt = (ground_truth_poses[indices] if indices is not None else ground_truth_poses).cpu()
        errs = [compute_pose_error(gt[i], cur[i]) for i in range(cur.shape[0])]
        r = [e["rotation_error_deg"] for e in errs]
        t = [e["translation_error"] for e in errs]
        return {
            "rotation_error_mean": float(np.mean(r)), "rotation_error_std": float(np.std(r)),
            "rotation_error_max": float(np.max(r)), "translation_error_mean": float(np.mean(t)),
            "translation_error_std": float(np.std(t)), "translation_error_max": float(np.max(t)),
        }


class CameraIntrinsics(nn.Module):
    """A learnable focal length for joint optimisation with the poses (NeRF--, Wang et al.
    2021; the reference's POSE_OPTIMIZATION.md lists it as future work).

    One parameter ``log_scale``, zero-initialised: (1,) in mode "shared" (one factor for both
    axes) or (2,) in mode "xy".  ``fxy()`` = ``focal_init * exp(log_scale)`` as a (2,) device
    tensor (fx, fy) that the ray kernels read from device memory.  At zero it is
    ``focal_init`` exactly, so the first step's rays are those of the fixed focal length.
    The log makes one learning rate mean the same at every focal length: a step of 1e-4
    changes it by 0.01 %.  ``focal_init``: a number, or a pair (fx, fy).

    The lens (keyword options) adds the principal point and two radial terms,
    the NeRF-- / SCNeRF model ``ops.ray_directions_lens`` states.  The module has a lens when
    ``learn_principal`` or ``learn_distortion`` is set or ``lens_init`` is not (0, 0); it then
    needs ``image_size=(W, H)``, and ``lens()`` is the (6,) device tensor
    (fx, fy, cx, cy, k1, k2) the ray kernels read:

    * ``principal`` (2,), zero-initialised, registered with ``learn_principal``:
      ``cx = W/2 + focal_init_x * principal[0]``, ``cy`` alike.  In units of the focal length
      for the reason ``log_scale`` is a log: a step of 1e-4 means the same at 50 and at
      1,100 pixels.  Without it the principal point is (W/2, H/2).
    * ``radial`` (2,) = (k1, k2), initialised to ``lens_init``, registered with
      ``learn_distortion``.  Without it a non-zero ``lens_init`` is HELD: a known calibration.

    What is held is a buffer named ``<name>_held`` in place of the parameter ``<name>``:
    ``learn_focal=False`` keeps the focal length at ``focal_init`` as ``log_scale_held``, and
    a held calibration is ``radial_held``.  A buffer is no parameter, so no optimizer ever
    sees it and a held value cannot move; and the state dict's keys alone say which options
    were on (``from_state_dict``).  A module built without the keyword options is the one
    described in the first paragraph: parameters ``["log_scale"]``, state-dict keys
    ``["focal_init", "log_scale"]``."""

    MODES = ("shared", "xy")

    def __init__(self, focal_init, mode: str = "shared", *, learn_focal: bool = True, learn_principal: bool = False,
                 learn_distortion: bool = False, lens_init=(0.0, 0.0), image_size=None):
        super().__init__()
        if mode not in self.MODES:
            raise ValueError(f"CameraIntrinsics: mode must be one of {self.MODES}, not {mode!r}")
        f = torch.as_tensor(focal_init, dtype=torch.float32).reshape(-1)
        if f.numel() not in (1, 2) or not bool((f > 0).all()):
            raise ValueError(f"CameraIntrinsics: focal_init must be one or two positive numbers, got {focal_init!r}")
        k = torch.as_tensor(lens_init, dtype=torch.float32).reshape(-1)
        if k.numel() != 2 or not bool(torch.isfinite(k).all()):
            raise ValueError(f"CameraIntrinsics: lens_init must be two finite numbers (k1, k2), got {lens_init!r}")
        self.mode = mode
        self.has_lens = bool(learn_principal or learn_distortion or bool((k != 0).any()))
        if not learn_focal and not self.has_lens:
            raise ValueError("CameraIntrinsics: learn_focal=False needs learn_principal, learn_distortion or a "
                             "non-zero lens_init (there would be nothing to learn or to hold)")
        self.register_buffer("focal_init", f.expand(2).clone())
        log_scale = torch.zeros(1 if mode == "shared" else 2)
        if learn_focal:
            self.log_scale = nn.Parameter(log_scale)
        else:
            self.register_buffer("log_scale_held", log_scale)
        if not self.has_lens:
            return
        wh = torch.as_tensor(image_size if image_size is not None else (), dtype=torch.float32).reshape(-1)
        if wh.numel() != 2 or not bool((wh > 0).all()):
            raise ValueError(f"CameraIntrinsics: a lens needs image_size=(W, H), two positive numbers, "
                             f"got {image_size!r}")
        self.register_buffer("image_size", wh.clone())
        if learn_principal:
            self.principal = nn.Parameter(torch.zeros(2))
        if learn_distortion:
            self.radial = nn.Parameter(k.clone())
        elif bool((k != 0).any()):
            self.register_buffer("radial_held", k.clone())

    @classmethod
    def from_state_dict(cls, state) -> "CameraIntrinsics":
        """The module a checkpoint's ``intrinsics`` entry was saved from (on the CPU).  The keys
        say how it was built: ``log_scale`` or ``log_scale_held``, ``principal``, ``radial`` or
        ``radial_held``, and ``image_size`` with any of the lens ones."""
        learn_focal = "log_scale" in state
        scale = state["log_scale" if learn_focal else "log_scale_held"]
        radial = state.get("radial", state.get("radial_held"))
        size = state.get("image_size")
        out = cls(state["focal_init"], "shared" if scale.numel() == 1 else "xy", learn_focal=learn_focal,
                  learn_principal="principal" in state, learn_distortion="radial" in state,
                  lens_init=(0.0, 0.0) if radial is None else radial.tolist(),
                  image_size=None if size is None else size.tolist())
        out.load_state_dict(state)
        return out

    def _log_scale(self) -> torch.Tensor:
        return self.log_scale if hasattr(self, "log_scale") else self.log_scale_held

    def fxy(self) -> torch.Tensor:
        return self.focal_init * torch.exp(self._log_scale())

    def fxy_values(self) -> Tuple[float, float]:
        """(fx, fy) as Python floats (one host read; for renders and reports, not the step)."""
        fx, fy = self.fxy().detach().cpu().tolist()
        return fx, fy

    def lens(self) -> torch.Tensor:
        """(fx, fy, cx, cy, k1, k2) as a (6,) device tensor, from torch ops (a captured graph
        holds them in front of the ray kernel, as it does ``fxy()``'s).  With every lens
        parameter at zero it is {fx, fy, W/2, H/2, 0, 0} exactly."""
        if not self.has_lens:
            raise ValueError("CameraIntrinsics.lens: built without a lens (learn_principal, learn_distortion, "
                             "lens_init); use fxy()")
        centre = self.image_size * 0.5
        if hasattr(self, "principal"):
            centre = centre + self.focal_init * self.principal
        radial = getattr(self, "radial", None)
        if radial is None:
            radial = getattr(self, "radial_held", None)
        if radial is None:
            radial = torch.zeros_like(centre)
        return torch.cat([self.fxy(), centre, radial])

    def lens_values(self) -> Tuple[float, float, float, float, float, float]:
        """(fx, fy, cx, cy, k1, k2) as Python floats (one host read, like ``fxy_values``)."""
        return tuple(self.lens().detach().cpu().tolist())

    def camera(self) -> torch.Tensor:
        """What the ray kernels read: ``lens()`` with a lens, ``fxy()`` without."""
        return self.lens() if self.has_lens else self.fxy()

    def camera_values(self) -> Tuple[float, ...]:
        return self.lens_values() if self.has_lens else self.fxy_values()

    def focal_error_pct(self, reference_focal: float) -> torch.Tensor:
        """mean over the axes of |f / reference - 1| in per cent (a device scalar, no sync)."""
        with torch.no_grad():
            return (self.fxy() / float(reference_focal) - 1.0).abs().mean() * 100.0


def train_step_with_poses(model_coarse: NeRF, model_fine: Optional[NeRF], camera_params: CameraPoseParameters,
                          pixel_sampler: PixelSampler, optimizer_nerf: torch.optim.Optimizer,
                          optimizer_poses: Optional[torch.optim.Optimizer], pixel_batch: PixelBatch,
                          render_config: RenderConfig, optimize_poses: bool = True,
                          rotation_reg_weight: float = 0.0, translation_reg_weight: float = 0.0,
                          t_rand: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """Reference train_pose_opt.py:290-411 (``t_rand``/``u`` optionally inject the draws)."""
    optimizer_nerf.zero_grad()
    if optimizer_poses is not None and optimize_poses:
        optimizer_poses.zero_grad()
    all_poses = camera_params.get_all_poses()
    rays_o, rays_d = pixel_sampler.get_rays_for_batch(pixel_batch, all_poses)
    target = pixel_batch.target_rgb
    out = render_rays(model_coarse, model_fine, rays_o, rays_d, render_config, is_train=True, t_rand=t_rand, u=u)
    loss_c = ops.mse_loss(out["rgb_coarse"], target)
    metrics = {"loss_coarse": loss_c.item(), "psnr_coarse": compute_psnr(out["rgb_coarse"].detach(), target).item()}
    if "rgb_fine" in out:
        loss_f = ops.mse_loss(out["rgb_fine"], target)
        loss = loss_c + loss_f
        metrics["loss_fine"] = loss_f.item()
        metrics["psnr_fine"] = compute_psnr(out["rgb_fine"].detach(), target).item()
        metrics["psnr"] = metrics["psnr_fine"]
    else:
        loss = loss_c
        metrics["loss_fine"] = None
        metrics["psnr"] = metrics["psnr_coarse"]
    if optimize_poses and (rotation_reg_weight > 0 or translation_reg_weight > 0):
        reg = 0.0
        if rotation_reg_weight > 0 and camera_params.learn_rotation:
            r = torch.mean(camera_params.rotation_deltas ** 2)
            reg = reg + rotation_reg_weight * r
            metrics["rotation_reg"] = r.item()
        if translation_reg_weight > 0 and camera_params.learn_translation:
            t = torch.mean(camera_params.translation_deltas ** 2)
            reg = reg + translation_reg_weight * t
            metrics["translation_reg"] = t.item()
        loss = loss + reg
        metrics["pose_reg_loss"] = reg.item() if isinstance(reg, torch.Tensor) else reg
    metrics["loss"] = loss.item()
    loss.backward()
    coarse = list(model_coarse.parameters())
    fine = list(model_fine.parameters()) if model_fine is not None else []
    poses = list(camera_params.parameters()) if (optimize_poses and optimizer_poses is not None) else []
    if isinstance(optimizer_nerf, FusedAdam):
        groups = [(coarse, 1.0)] + ([(fine, 1.0)] if fine else [])
        optimizer_nerf.step(clip_groups=groups)  # the clips fold into the fused update
    else:
        clip_grad_norm_(coarse, 1.0)
        if fine:
            clip_grad_norm_(fine, 1.0)
        optimizer_nerf.step()
    if optimizer_poses is not None and optimize_poses:
        if isinstance(optimizer_poses, FusedAdam):
            optimizer_poses.step(clip_groups=[(poses, 0.1)])
        else:
            clip_grad_norm_(poses, 0.1)
            optimizer_poses.step()
    return metrics


@torch.no_grad()
def render_image_with_pose(model_coarse: NeRF, model_fine: Optional[NeRF], pose: torch.Tensor, H: int, W: int,
                           focal: float, render_config: RenderConfig, chunk_size: int = 1024 * 4,
                           fxy: Optional[Tuple[float, float]] = None) -> Dict[str, torch.Tensor]:
    """Reference train_pose_opt.py:415-470.  ``fxy`` (optional): learned focal lengths
    (fx, fy) in place of ``focal`` (``ops.ray_directions_xy``)."""
    return render_image(NeRFRenderer(model_coarse, model_fine, render_config), pose, H, W, focal, chunk_size, fxy)


def _window_dict(net: NeRF) -> Optional[Dict[str, Optional[List[float]]]]:
    pos, dir_ = net.pe_window()
    return None if pos is None and dir_ is None else {"pos": pos, "dir": dir_}


@torch.no_grad()
def evaluate_with_poses(model_coarse: NeRF, model_fine: Optional[NeRF], camera_params: CameraPoseParameters,
                        val_data: BlenderData, val_indices: torch.Tensor, render_config: RenderConfig,
                        logger: Optional[ExperimentLogger] = None, iteration: int = 0, num_images: int = 5,
                        lpips_metric=None, fxy: Optional[Tuple[float, float]] = None) -> ValidationMetrics:
    """Reference train_pose_opt.py:474-545: renders the first ``num_images`` validation
    views from their GROUND-TRUTH poses (the learnable poses are the training views');
    PNGs of the first three when a logger is given.  The networks render with their
    current positional-encoding windows (``NeRF.set_pe_window``), and with the learned
    focal lengths ``fxy`` when given (the field was fitted to rays of that focal length)."""
    views = [int(idx) for idx in val_indices[:min(num_images, len(val_indices))]]
    return evaluate_views(
        lambda idx: render_image_with_pose(model_coarse, model_fine, val_data.poses[idx], val_data.H, val_data.W,
                                           val_data.focal, render_config, fxy=fxy),
        ((f"val_{idx}", idx, val_data.images[idx]) for idx in views), logger, iteration, lpips_metric)


def save_checkpoint_with_poses(output_dir, iteration: int, model_coarse, model_fine, camera_params,
                               optimizer_nerf, optimizer_poses, config: NeRFConfig, noise_config=None,
                               metrics: Optional[Dict] = None, pose_errors: Optional[Dict] = None,
                               is_best: bool = False, intrinsics: Optional[CameraIntrinsics] = None) -> None:
    """Reference train_pose_opt.py:548-610: the train.py checkpoint plus ``camera_params``,
    ``optimizer_nerf`` / ``optimizer_poses``, ``initial_poses`` and ``pose_errors``; with
    learned ``intrinsics`` also their state dict as ``intrinsics``."""
    ckpt = base_checkpoint(iteration, model_coarse, model_fine, config, noise_config, metrics)
    ckpt.update(camera_params=camera_params.state_dict(), optimizer_nerf=optimizer_nerf.state_dict(),
                initial_poses=camera_params.initial_poses.cpu())
    window = _window_dict(model_coarse)
    if window is not None:
        ckpt["mi355x"]["pe_window"] = window  # both networks share the schedule
    if intrinsics is not None:
        ckpt["intrinsics"] = intrinsics.state_dict()  # CameraIntrinsics.from_state_dict rebuilds it
    if optimizer_poses is not None:
        ckpt["optimizer_poses"] = optimizer_poses.state_dict()
    if pose_errors is not None:
        ckpt["pose_errors"] = pose_errors
    write_checkpoint(output_dir, iteration, ckpt, is_best)


def generate_experiment_name(scene: str, noise_config: Optional[NoiseConfig], init_mode: str = "noisy") -> str:
    """Reference train_pose_opt.py:274-287."""
    ts = datetime.now().strftime("%Y%m%d_%H%M%S")
    noise_desc = str(noise_config) if noise_config is not None and noise_config.has_noise else "clean"
    return f"{scene}_poseopt_{init_mode}init_{noise_desc}_{ts}"


def train_with_pose_optimization(config: NeRFConfig, noise_config: Optional[NoiseConfig] = None,
                                 init_mode: str = "noisy", pose_lr: float = 1e-4, pose_opt_delay: int = 1000,
                                 learn_rotation: bool = True, learn_translation: bool = True,
                                 rotation_reg_weight: float = 0.01, translation_reg_weight: float = 0.001, *,
                                 train_data: Optional[BlenderData] = None, val_data: Optional[BlenderData] = None,
                                 process_group=None, experiment_name: Optional[str] = None,
                                 log=print, graph: bool = False, c2f: Optional[Tuple[float, float]] = None,
                                 fixed_small_angle: bool = False, learn_focal: Optional[str] = None,
                                 focal_init_scale: float = 1.0, distortion_weight: float = 0.0,
                                 loss: str = "mse", loss_scale: float = 0.1, learn_principal: bool = False,
                                 learn_distortion: bool = False,
                                 lens_init: Tuple[float, float] = (0.0, 0.0)) -> Dict[str, object]:
    """Reference train_pose_opt.py:613-1054 (same arguments, outputs and files).
    ``train_data`` / ``val_data`` (optional) replace the on-disk scene; ``process_group``
    makes it data parallel; ``experiment_name`` pins the generated run name (all ranks).
    ``graph`` replays the step from hipGraphs (``engine.GraphedPoseTrainer``; same results
    as eager): iteration 0 runs eagerly, the frozen-pose graph is captured at the next
    iteration; the first iteration that optimises the poses runs eagerly (it creates the
    pose Adam's state) and the optimising graph is captured at the one after it.  With
    data parallelism it needs the nccl backend.
    ``c2f=(start, end)`` windows both positional encodings coarse to fine over that
    fraction of the run (``c2f_alpha``, ``pe_window_weights``); ``fixed_small_angle`` is
    ``CameraPoseParameters``' (live rotation gradients at w = 0).  Neither is in the
    reference; both default to its behaviour.
    ``learn_focal`` ("shared" or "xy"; ``--learn_focal``) learns the focal length with the
    poses (``CameraIntrinsics``, NeRF--), starting from ``focal_init_scale`` times the
    dataset's: same Adam, learning rate, schedule and delay as the poses; validation renders
    use the learned value, the log and train_metrics.csv report its error in per cent
    against the dataset's, checkpoints gain ``intrinsics`` and final_poses.pt the three
    ``*_focal`` entries.  None (the default) is the reference's fixed focal length.
    ``learn_principal`` / ``learn_distortion`` (``--learn_principal``, ``--learn_distortion``)
    learn the principal point and the radial terms (k1, k2) of ``CameraIntrinsics``' lens the
    same way, each a clip group of its own; ``lens_init`` (``--lens_init K1 K2``) is where
    (k1, k2) start, or, without ``learn_distortion``, a known calibration that is held.
    Without ``learn_focal`` the focal length is then held at the dataset's (times
    ``focal_init_scale``).  Validation renders use the lens, train_metrics.csv gains
    ``lens_cx, lens_cy, lens_k1, lens_k2`` and final_poses.pt the three ``*_lens`` entries
    (six numbers each; the ground truth is the dataset's centred pinhole).  With none of the
    three nothing changes.
    ``distortion_weight`` > 0 (``--distortion_weight``) adds that multiple of the distortion
    loss on the rendering network's ray weights (``engine.PoseTrainer``); its value goes to
    the console line only.
    ``loss`` / ``loss_scale`` (``--loss``, ``--loss_scale``): the photometric loss of both
    networks and its scale (``engine.PoseTrainer``); the CSV's ``psnr`` stays the plain
    MSE's and the console line names a robust kind."""
    import torch.distributed as dist

    pe_schedule = None
    if c2f is not None:
        c2f = (float(c2f[0]), float(c2f[1]))
        if not 0.0 <= c2f[0] < c2f[1]:
            raise ValueError(f"c2f=(start, end) needs 0 <= start < end, got {c2f}")
        n_it = config.train.num_iterations

        def pe_schedule(iteration, num_freqs):
            return pe_window_weights(c2f_alpha(iteration, n_it, c2f[0], c2f[1], num_freqs), num_freqs)
    exp_name = experiment_name or generate_experiment_name(config.data.scene_name, noise_config, init_mode)
    rank, world, device, output_dir, logger, lpips_metric = open_run(
        config, exp_name, process_group, graph, "train_with_pose_optimization", train_data, val_data)
    if train_data is None:
        root = config.data.data_root if config.data.data_root is not None else Path("data") / "raw"
        train_data = load_blender_data(root, config.data.scene_name, "train", config.data.img_scale, device)
        val_data = load_blender_data(root, config.data.scene_name, "val", config.data.img_scale, device)
    gt_train_poses = train_data.poses.clone()
    if init_mode == "noisy" and noise_config is not None and noise_config.has_noise:
        initial_poses, _ = add_noise_to_poses(train_data.poses, noise_config)
        if logger is not None:
            errs = [compute_pose_error(gt_train_poses[i].cpu(), initial_poses[i].cpu())
                    for i in range(len(initial_poses))]
            log(f"initial pose errors: rotation {np.mean([e['rotation_error_deg'] for e in errs]):.3f} deg, "
                f"translation {np.mean([e['translation_error'] for e in errs]):.4f}")
    else:
        initial_poses = gt_train_poses.clone()
    camera_params = CameraPoseParameters(initial_poses, learn_rotation, learn_translation,
                                         fixed_small_angle=fixed_small_angle).to(device)
    intrinsics = None
    lens_init = tuple(float(k) for k in lens_init)
    with_lens = bool(learn_principal or learn_distortion or any(k != 0 for k in lens_init))
    if learn_focal is not None or with_lens:
        if not focal_init_scale > 0:
            raise ValueError(f"focal_init_scale must be positive, got {focal_init_scale}")
        if not with_lens:
            intrinsics = CameraIntrinsics(train_data.focal * focal_init_scale, learn_focal).to(device)
        else:
            intrinsics = CameraIntrinsics(train_data.focal * focal_init_scale, learn_focal or "shared",
                                          learn_focal=learn_focal is not None, learn_principal=learn_principal,
                                          learn_distortion=learn_distortion, lens_init=lens_init,
                                          image_size=(train_data.W, train_data.H)).to(device)
    initial_lens = intrinsics.lens().detach().cpu() if with_lens else None
    gt_focal = float(train_data.focal)
    model_coarse, model_fine = create_nerf_for(config, device, logger)
    _, pixel_sampler = create_pixel_dataset(train_data)
    pixel_sampler.batch_size = config.data.batch_size
    trainer = PoseTrainer(model_coarse, model_fine, camera_params, pixel_sampler, config.render, lr=config.train.lr,
                          pose_lr=pose_lr, lr_decay=config.train.lr_decay, rotation_reg_weight=rotation_reg_weight,
                          translation_reg_weight=translation_reg_weight, process_group=process_group,
                          pe_schedule=pe_schedule, intrinsics=intrinsics, distortion_weight=distortion_weight,
                          loss=loss, loss_scale=loss_scale)
    optimizer_nerf, optimizer_poses = trainer.optimizer_nerf, trainer.optimizer_poses
    if rank == 0:
        extra = {}
        if c2f is not None:
            extra["c2f"] = list(c2f)
        if fixed_small_angle:
            extra["fixed_small_angle"] = True
        if intrinsics is not None and learn_focal is not None:
            extra["learn_focal"] = {"mode": learn_focal, "focal_init_scale": focal_init_scale}
        if with_lens:
            extra["lens"] = {"learn_principal": learn_principal, "learn_distortion": learn_distortion,
                             "lens_init": list(lens_init), "focal_init_scale": focal_init_scale}
        extra["distortion_weight"] = distortion_weight
        extra["loss"], extra["loss_scale"] = loss, loss_scale
        write_experiment_config(output_dir, config, exp_name, world, noise_config, extra=extra, after_name={
            "init_mode": init_mode,
            "pose_optimization": {"learn_rotation": learn_rotation, "learn_translation": learn_translation,
                                  "pose_lr": pose_lr, "pose_opt_delay": pose_opt_delay,
                                  "rotation_reg_weight": rotation_reg_weight,
                                  "translation_reg_weight": translation_reg_weight}})
        log(f"joint NeRF + pose optimisation: {exp_name} -> {output_dir} ({world} rank(s))")

    def line(vm, lr, rays_per_sec, optimizing):
        focal = f" | focal err: {vm['focal_error_pct']:.3f}%" if "focal_error_pct" in vm else ""
        if "lens_k1" in vm:
            focal += (f" | lens: c ({vm['lens_cx']:.3f}, {vm['lens_cy']:.3f}) k ({vm['lens_k1']:.5f}, "
                      f"{vm['lens_k2']:.5f})")
        if "loss_distortion" in vm:
            focal += f" | distortion: {vm['loss_distortion']:.5f}"
        return f"{loss_line(loss, loss_scale)}lr: {lr:.2e} | poses: {'optimizing' if optimizing else 'frozen'}{focal}"

    def learned_fxy():  # two numbers, or the six of a lens
        return intrinsics.camera_values() if intrinsics is not None else None

    def extra_scalars():
        """Device scalars for the iteration log: the focal error, and the lens's last four."""
        if intrinsics is None:
            return None
        out = {"focal_error_pct": intrinsics.focal_error_pct(gt_focal)}
        if with_lens:
            with torch.no_grad():
                out.update(zip(LENS_COLUMNS, intrinsics.lens()[2:].unbind()))
        return out

    def checkpoint(iteration, pe, **kw):
        save_checkpoint_with_poses(output_dir, iteration, model_coarse, model_fine, camera_params, optimizer_nerf,
                                   optimizer_poses, config, noise_config, pose_errors=pe, intrinsics=intrinsics, **kw)

    B = config.data.batch_size
    rc = config.render
    val_idx = torch.arange(val_data.images.shape[0], device=device)
    best_psnr = 0.0
    graphed = None
    ilog = IterationLog(logger, config, process_group, line, log)
    for iteration in range(config.train.num_iterations):
        # the global batch, identical on every rank (one process in graph mode: the gather
        # kernel writes it straight into the graphs' static inputs).  The draws stay in the
        # eager order: randint, rand, rand
        batch = pixel_sampler.sample_batch(out=graphed.static if (graphed is not None and world == 1) else None)
        now = iteration >= pose_opt_delay
        sl, (t_rand, u) = slice_for_rank(B, rank, world, *draw_randoms(B, rc, model_fine is not None, device))
        args = (batch.slice(sl) if world > 1 else batch, now, t_rand, u)
        if graph and iteration >= 1:
            if graphed is None:  # after one eager step: the networks' Adam state exists
                graphed = GraphedPoseTrainer(trainer, args[0], args[2], args[3], warmup=0)
            m = graphed.step(*args, iteration=iteration)  # eager once more where the pose Adam's state is new
        else:
            m = trainer.step(*args, iteration=iteration)
        # the focal error is a device scalar like the losses: read one iteration late
        ilog.push(iteration, m, optimizer_nerf.param_groups[0]["lr"], extra_scalars(), now)
        what = due(iteration, config.train.val_every, config.train.save_every) if logger is not None else None
        if what:
            ilog.flush()
            pe = camera_params.compute_pose_errors(gt_train_poses)
            if what == "val":
                vmx = evaluate_with_poses(model_coarse, model_fine, camera_params, val_data, val_idx, rc, logger,
                                          iteration, num_images=5, lpips_metric=lpips_metric, fxy=learned_fxy())
                logger.log_validation(vmx)
                is_best = vmx.psnr > best_psnr
                best_psnr = max(best_psnr, vmx.psnr)
                focal = (f"; focal error {float(intrinsics.focal_error_pct(gt_focal)):.3f} %"
                         if intrinsics is not None else "")
                log(f"  validation @ {iteration}: PSNR {vmx.psnr:.2f} dB; pose error rot "
                    f"{pe['rotation_error_mean']:.3f} deg, trans {pe['translation_error_mean']:.4f}{focal}")
                checkpoint(iteration, pe, metrics={"psnr": vmx.psnr, "ssim": vmx.ssim}, is_best=is_best)
            else:
                checkpoint(iteration, pe)
            ilog.pause()
    ilog.flush()
    if pe_schedule is not None:
        # the final evaluation and checkpoint: the window at the end of the schedule
        trainer.set_pe_windows(config.train.num_iterations)
    result = {"model_coarse": model_coarse, "model_fine": model_fine, "camera_params": camera_params,
              "output_dir": output_dir, "pose_errors": camera_params.compute_pose_errors(gt_train_poses)}
    if intrinsics is not None:
        result["intrinsics"] = intrinsics
        result["focal_error_pct"] = float(intrinsics.focal_error_pct(gt_focal))
    if logger is not None:
        final_pe = result["pose_errors"]
        final = evaluate_with_poses(model_coarse, model_fine, camera_params, val_data, val_idx, rc, logger,
                                    config.train.num_iterations, num_images=val_data.images.shape[0],
                                    lpips_metric=lpips_metric, fxy=learned_fxy())
        # (the reference does not write the final evaluation to val_metrics.csv, :1002-1019)
        checkpoint(config.train.num_iterations, final_pe, metrics={"psnr": final.psnr, "ssim": final.ssim})
        with torch.no_grad():
            final_poses = camera_params.get_all_poses()
        record = {"initial_poses": camera_params.initial_poses.cpu(), "optimized_poses": final_poses.cpu(),
                  "ground_truth_poses": gt_train_poses.cpu(), "pose_errors": final_pe}
        if intrinsics is not None:  # (fx, fy) each, for pose_eval's focal report
            record.update(initial_focal=intrinsics.focal_init.detach().cpu().clone(),
                          optimized_focal=intrinsics.fxy().detach().cpu(),
                          ground_truth_focal=torch.full((2,), gt_focal, dtype=torch.float32))
        if with_lens:  # (fx, fy, cx, cy, k1, k2) each, for pose_eval's lens report
            record.update(initial_lens=initial_lens, optimized_lens=intrinsics.lens().detach().cpu(),
                          ground_truth_lens=torch.tensor([gt_focal, gt_focal, train_data.W / 2.0, train_data.H / 2.0,
                                                          0.0, 0.0], dtype=torch.float32))
        torch.save(record, output_dir / "final_poses.pt")
        logger.save_summary()
        logger.close()
        focal = f", focal error {result['focal_error_pct']:.3f} %" if intrinsics is not None else ""
        log(f"final: PSNR {final.psnr:.2f} dB; pose error rot {final_pe['rotation_error_mean']:.3f} deg, "
            f"trans {final_pe['translation_error_mean']:.4f}{focal}; results in {output_dir}")
        result["val"] = final
    if process_group is not None:
        dist.barrier(process_group)
    return result


# what the measured table shows (profiles/pose_graph_ab.json)
GRAPH_HELP = ("replay the joint step from hipGraphs, one for frozen poses and one for optimising (same results as "
              "eager; with RCCL data parallelism the all-reduces are captured too). Measured on one MI355X, bf16 "
              "64c+128f, ms per step eager -> replayed: 512 rays 1.55 -> 1.04; 1024 rays (the default batch) "
              "1.56 -> 1.55, no gain; 4096 rays 5.20 -> 5.22, 0.4 %% slower. It pays below 1024 rays per GPU")


def build_arg_parser():
    """Reference train_pose_opt.py:1057-1142 flags (same names and defaults) plus ``--precision``,
    ``--graph``, ``--c2f``, ``--fixed_small_angle``, ``--learn_focal``, ``--focal_init_scale`` and
    ``--distortion_weight``."""
    import argparse
    ap = argparse.ArgumentParser(description="Joint NeRF + camera pose optimisation (MI355X HIP path)")
    add_common_args(ap, "scene data_root img_scale batch_size num_iters lr", num_iters=dict(default=50000),
                    batch_size=dict(help="global batch (pixels) over all ranks"))
    ap.add_argument("--init_mode", type=str, default="noisy", choices=["noisy", "clean"])
    ap.add_argument("--pose_lr", type=float, default=1e-4)
    ap.add_argument("--pose_opt_delay", type=int, default=1000)
    ap.add_argument("--no_learn_rotation", action="store_true")
    ap.add_argument("--no_learn_translation", action="store_true")
    ap.add_argument("--rotation_reg_weight", type=float, default=0.01)
    ap.add_argument("--translation_reg_weight", type=float, default=0.001)
    add_common_args(ap, "rotation_noise translation_noise translation_noise_pct noise_seed no_hierarchical num_samples "
                        "num_samples_fine log_every val_every save_every output_dir device seed precision",
                    val_every=dict(default=2500))
    ap.add_argument("--graph", action="store_true", help=GRAPH_HELP)
    ap.add_argument("--c2f", type=float, nargs=2, default=None, metavar=("START", "END"),
                    help="coarse-to-fine positional encoding (BARF): the frequencies of both encoders are "
                         "enabled one after another between the fractions START and END of the run")
    ap.add_argument("--fixed_small_angle", action="store_true",
                    help="exact Rodrigues derivative at zero rotation deltas, so the rotations learn (the "
                         "reference blocks that gradient)")
    ap.add_argument("--learn_focal", type=str, default=None, choices=list(CameraIntrinsics.MODES),
                    help="learn the focal length jointly with the poses (NeRF--): one factor for both axes "
                         "(shared) or one per axis (xy), with the pose learning rate, schedule and delay")
    ap.add_argument("--focal_init_scale", type=float, default=1.0,
                    help="with --learn_focal: start from this multiple of the dataset's focal length (the "
                         "deterministic counterpart of the pose-noise flags)")
    add_common_args(ap, "distortion_weight")
    return ap


def build_cli_parser():
    """The command line's parser: ``build_arg_parser()`` (the reference's flags and this
    project's earlier ones, in the order its callers rely on) plus the photometric loss
    flags ``--loss`` and ``--loss_scale`` and the lens flags ``--learn_principal``,
    ``--learn_distortion`` and ``--lens_init``."""
    ap = build_arg_parser()
    add_common_args(ap, "loss loss_scale")
    ap.add_argument("--learn_principal", action="store_true",
                    help="learn the principal point (cx, cy) jointly with the poses, from the image centre, in "
                         "units of the focal length; with the pose learning rate, schedule and delay")
    ap.add_argument("--learn_distortion", action="store_true",
                    help="learn two radial distortion terms (k1, k2) of the NeRF-- / SCNeRF ray-side model "
                         "jointly with the poses, from --lens_init")
    ap.add_argument("--lens_init", type=float, nargs=2, default=(0.0, 0.0), metavar=("K1", "K2"),
                    help="the radial terms to start from; without --learn_distortion a known calibration that "
                         "is held fixed")
    return ap


def main(argv=None) -> None:
    """``python -m noisy_src.train_pose_opt`` (or under ``torchrun`` for data parallelism)."""
    a = build_cli_parser().parse_args(argv)

    def call(cfg, noise_config, pg, name):
        train_with_pose_optimization(cfg, noise_config, a.init_mode, a.pose_lr, a.pose_opt_delay,
                                     not a.no_learn_rotation, not a.no_learn_translation, a.rotation_reg_weight,
                                     a.translation_reg_weight, process_group=pg, experiment_name=name,
                                     graph=a.graph, c2f=tuple(a.c2f) if a.c2f is not None else None,
                                     fixed_small_angle=a.fixed_small_angle, learn_focal=a.learn_focal,
                                     focal_init_scale=a.focal_init_scale, distortion_weight=a.distortion_weight,
                                     loss=a.loss, loss_scale=a.loss_scale, learn_principal=a.learn_principal,
                                     learn_distortion=a.learn_distortion, lens_init=tuple(a.lens_init))

    run_cli(a, lambda noise_config, world: generate_experiment_name(a.scene, noise_config, a.init_mode), call)


__all__ = ["set_seed", "CameraPoseParameters", "CameraIntrinsics", "train_step_with_poses", "render_image_with_pose",
           "evaluate_with_poses", "save_checkpoint_with_poses", "generate_experiment_name",
           "train_with_pose_optimization", "pe_window_weights", "c2f_alpha", "main"]

if __name__ == "__main__":
    main()
