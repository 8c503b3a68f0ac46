"""
Test-set evaluation and checkpoint loading — drop-in for ShawnnnLiu/Robust-NeRF
``noisy_src/inference.py`` (the eval half of BASELINE.json's metric).

``evaluate_test_set`` keeps the reference's signature, per-image metrics and output
files (inference.py:145-318), with the rendering on the HIP forward-only path
(``render_image`` -> NeRFRenderer, is_train=False) and, given a process group, the
test views sharded across ranks (SURVEY.md §8e "Eval"): rank r renders views
r, r+N, r+2N, ...; the per-image metric records are all-gathered so every rank
returns the same summary, and rank 0 writes the JSON files.  Camera noise is drawn
for every view up front, in view order, from the same seed on every rank (the
reference draws it inside its loop, in the same order; rendering itself draws
nothing), so the noisy poses match the reference's sequential run.

``render_video`` (inference.py:365-443) shards its frames the same way, and ``main``
is the reference's command line (inference.py:446-612: ``python -m noisy_src.inference
ckpt.pt --mode test --rotation_noise 1.0``) with a working ``--mode single``,
``--precision`` and, under ``torch.distributed.run``, the sharding above.  On a GPU the
entry point runs the fused image tail (``fused_tail=True``): ``metrics.image_metrics``
(fp64 SSIM, one read-back per image) and the 8-bit frames of ``frame_u8`` /
``depth_frame_u8`` written on the device (csrc/image.hip).

Pose-optimised checkpoints (no reference counterpart; BARF's evaluation protocol):
``--align_train_poses`` carries the ground-truth test poses into the frame the field was
trained in (``pose_eval.align_sim3`` of the checkpoint's optimised train poses against
the train split's), and ``--refine_poses ITERS`` refines every test pose photometrically
against its own image on the frozen field (``engine.PoseRefiner``) before it is rendered
and scored.  Without either flag the outputs are byte for byte what they were.
"""

from __future__ import annotations

import json
import time
from datetime import datetime
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .config import ModelConfig, RenderConfig
from .logger import depth_to_colormap  # the reference's inference.py:114-125 is its logger.py:290-302
from .metrics import LPIPSMetric, compute_mse, compute_psnr, compute_ssim, image_metrics
from .model import NeRF
from .noise import NoiseConfig, add_noise_to_pose, compute_pose_error, set_noise_seed
from .ops import LOSS_KINDS
from .rendering import NeRFRenderer
from .train import render_image


def load_checkpoint(checkpoint_path: Path, device: str = "cuda", precision: Optional[str] = None) -> tuple:
    """Reference inference.py:33-72 -> (renderer, config dict, iteration).  Loads with
    ``weights_only=True``: a checkpoint is tensors, dicts, lists and scalars only.
    ``precision`` overrides the MLP operand precision stored with the checkpoint; a
    positional-encoding window stored with it (``mi355x.pe_window``) is applied."""
    ckpt = torch.load(checkpoint_path, map_location=device, weights_only=True)
    cfg = ckpt.get("config", {})
    model_cfg = ModelConfig(**cfg.get("model", {}))
    # MI355X-only knob, kept out of config["model"] so reference loaders accept the file
    model_cfg.precision = precision or ckpt.get("mi355x", {}).get("precision", model_cfg.precision)
    render_cfg = RenderConfig(**cfg.get("render", {}))
    coarse = NeRF(model_cfg).to(device)
    coarse.load_state_dict(ckpt["model_coarse"])
    coarse.eval()
    fine = None
    if "model_fine" in ckpt:
        fine = NeRF(model_cfg).to(device)
        fine.load_state_dict(ckpt["model_fine"])
        fine.eval()
    window = ckpt.get("mi355x", {}).get("pe_window")
    if window is not None:
        # saved while a coarse-to-fine window was active (train_pose_opt --c2f): the
        # weights were trained against that encoding, so they render with it
        for net in (coarse, fine):
            if net is not None:
                net.set_pe_window(window.get("pos"), window.get("dir"))
    return NeRFRenderer(coarse, fine, render_cfg), cfg, ckpt.get("iteration", 0)


def intrinsics_fxy(ckpt: dict):
    """(fx, fy) a checkpoint learned (its ``intrinsics`` entry, written by ``train_pose_opt
    --learn_focal``: focal_init * exp(log_scale) in fp32, as the training step computes it),
    or None for a checkpoint without the entry, which renders with the dataset's focal length.
    A checkpoint with a lens (``--learn_principal``, ``--learn_distortion``, ``--lens_init``)
    gives its six numbers (fx, fy, cx, cy, k1, k2) instead; everything here that takes ``fxy``
    takes either."""
    state = ckpt.get("intrinsics")
    if state is None:
        return None
    from .train_pose_opt import CameraIntrinsics
    return CameraIntrinsics.from_state_dict({k: v.detach().cpu() for k, v in state.items()}).camera_values()


def _render(renderer, pose, H, W, focal, chunk_size, fxy):
    """``render_image``; without learned focal lengths exactly the call of before."""
    if fxy is None:
        return render_image(renderer, pose, H, W, focal, chunk_size=chunk_size)
    return render_image(renderer, pose, H, W, focal, chunk_size=chunk_size, fxy=fxy)


def checkpoint_intrinsics(checkpoint_path: Path):
    """``intrinsics_fxy`` of the checkpoint file at ``checkpoint_path``."""
    return intrinsics_fxy(torch.load(checkpoint_path, map_location="cpu", weights_only=True))


def save_image(img: torch.Tensor, path: Path) -> None:
    """Reference inference.py:108-111: [0,1] float (H,W,3) -> 8-bit PNG."""
    from PIL import Image
    arr = (img.detach().cpu().numpy() * 255).clip(0, 255).astype(np.uint8)
    Image.fromarray(arr).save(path)


def frame_u8(img: torch.Tensor, out: Optional[torch.Tensor] = None, x0: int = 0) -> torch.Tensor:
    """``save_image``'s quantisation on the device (``nr_frame_u8``): (H,W,C) fp32 -> a device
    uint8 frame with the same bytes.  With ``out`` (H, W_out, C) uint8 the image lands in
    columns [x0, x0 + W): two calls fill a side-by-side comparison frame."""
    from . import _hip
    src = img.detach().float().contiguous()
    sp = _hip.ptr(src)
    if src.dim() != 3:
        raise ValueError(f"frame_u8: need an (H,W,C) image, got {tuple(src.shape)}")
    H, W, C = src.shape
    if out is None:
        out = torch.empty(H, W, C, device=src.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or out.dim() != 3 or out.shape[0] != H or out.shape[2] != C \
            or not 0 <= x0 <= out.shape[1] - W:
        raise ValueError(f"frame_u8: a {(H, W, C)} image at column {x0} does not fit the frame {tuple(out.shape)}")
    _hip.call("nr_frame_u8", sp, H, W, C, _hip.ptr(out), out.shape[1] * C, x0, _hip.stream_ptr())
    return out


def depth_frame_u8(depth: torch.Tensor) -> torch.Tensor:
    """``depth_to_colormap`` and ``save_image``'s quantisation on the device
    (``nr_depth_frame_u8``): (H,W) depth -> (H,W,3) device uint8, the host path's bytes."""
    from . import _hip
    d = depth.detach().float().contiguous()
    dp = _hip.ptr(d)
    if d.dim() != 2:
        raise ValueError(f"depth_frame_u8: need an (H,W) depth map, got {tuple(d.shape)}")
    out = torch.empty(d.shape[0], d.shape[1], 3, device=d.device, dtype=torch.uint8)
    ws = torch.empty(int(_hip.call("nr_depth_frame_u8_workspace_bytes")), device=d.device, dtype=torch.uint8)
    _hip.call("nr_depth_frame_u8", dp, d.shape[0], d.shape[1], _hip.ptr(out), _hip.ptr(ws), _hip.stream_ptr())
    return out


def save_frame_u8(frame: torch.Tensor, path: Path) -> None:
    """A device uint8 frame -> host bytes -> PNG (the image crosses PCIe as bytes)."""
    from PIL import Image
    Image.fromarray(frame.cpu().numpy()).save(path)


def _save_view(out_dir: Path, i: int, pred: torch.Tensor, target: torch.Tensor, depth: torch.Tensor,
               fused_tail: bool) -> None:
    """The four PNGs of one evaluated view (reference inference.py:232-247)."""
    if not fused_tail:
        save_image(pred, out_dir / f"pred_{i:03d}.png")
        save_image(target, out_dir / f"gt_{i:03d}.png")
        save_image(torch.cat([target, pred], dim=1), out_dir / f"comparison_{i:03d}.png")
        save_image(depth_to_colormap(depth), out_dir / f"depth_{i:03d}.png")
        return
    H, W, C = pred.shape
    both = torch.empty(H, 2 * W, C, device=pred.device, dtype=torch.uint8)
    frame_u8(target, out=both, x0=0)
    frame_u8(pred, out=both, x0=W)
    from PIL import Image
    host = both.cpu().numpy()  # one copy; pred and gt are its halves
    Image.fromarray(np.ascontiguousarray(host[:, W:])).save(out_dir / f"pred_{i:03d}.png")
    Image.fromarray(np.ascontiguousarray(host[:, :W])).save(out_dir / f"gt_{i:03d}.png")
    Image.fromarray(host).save(out_dir / f"comparison_{i:03d}.png")
    save_frame_u8(depth_frame_u8(depth), out_dir / f"depth_{i:03d}.png")


def generate_output_folder_name(mode: str, noise_config: NoiseConfig, scene: str) -> str:
    """Reference inference.py:128-142: ``{mode}_{scene}_{noise}_{timestamp}``."""
    return f"{mode}_{scene}_{noise_config}_{datetime.now().strftime('%Y%m%d_%H%M%S')}"


def create_spiral_poses(n_frames: int = 120, radius: float = 0.5, height: float = 0.0, n_rotations: float = 2.0,
                        device: str = "cuda") -> torch.Tensor:
    """Reference inference.py:321-362: look-at-origin cameras on a circle of radius 4."""
    t = np.arange(n_frames) / n_frames
    theta = 2 * np.pi * n_rotations * t
    pos = np.stack([4.0 * np.cos(theta), 4.0 * np.sin(theta), np.full_like(theta, height)], -1)
    fwd = -pos / np.linalg.norm(pos, axis=-1, keepdims=True)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right, axis=-1, keepdims=True)
    up = np.cross(right, fwd)
    c2w = np.tile(np.eye(4, dtype=np.float32), (n_frames, 1, 1))
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, up, -fwd, pos
    return torch.from_numpy(c2w).to(device)


def _noisy_poses(test_data, noise_config: NoiseConfig, poses: Optional[torch.Tensor] = None):
    """Every view's (pose, noise info) in view order, as the reference's loop draws them.
    ``poses``: the clean poses when they are not ``test_data.poses`` (the learned frame)."""
    if noise_config.seed is not None:
        set_noise_seed(noise_config.seed)
    out = []
    for i in range(test_data.images.shape[0]):
        orig = test_data.poses[i] if poses is None else poses[i]
        if noise_config.has_noise:
            pose, info = add_noise_to_pose(orig, rotation_noise_deg=noise_config.rotation_noise_deg,
                                           translation_noise=noise_config.translation_noise)
            info.update(compute_pose_error(orig, pose))
        else:
            pose, info = orig, {}
        out.append((pose, info))
    return out


def _rank0_draws(views, noise_config: NoiseConfig, process_group):
    """Unseeded noise under a process group: every rank must still render rank 0's draws."""
    if process_group is None or not noise_config.has_noise or noise_config.seed is not None:
        return views
    import torch.distributed as dist
    if dist.get_world_size(process_group) == 1 or not views:
        return views
    device = views[0][0].device
    obj = [[(p.cpu(), info) for p, info in views]]
    dist.broadcast_object_list(obj, src=dist.get_global_rank(process_group, 0), group=process_group)
    return [(p.to(device), info) for p, info in obj[0]]


def checkpoint_train_poses(checkpoint_path: Path) -> torch.Tensor:
    """The optimised train poses (N,4,4) a ``train_pose_opt`` checkpoint carries
    (``camera_params``: initial poses and the learned deltas), composed on the host in fp64
    with the SE(3) map of the training run: R = exp([w]x) R_0, t = t_0 + dt."""
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    cam = ckpt.get("camera_params")
    if cam is None or "initial_poses" not in cam:
        raise SystemExit(f"--align_train_poses: {checkpoint_path} carries no camera_params (it was not written by "
                         "noisy_src.train_pose_opt), so there are no optimised train poses to align")
    init = cam["initial_poses"].to(torch.float64)
    n = init.shape[0]
    w = cam.get("rotation_deltas", torch.zeros(n, 3)).to(torch.float64)
    dt = cam.get("translation_deltas", torch.zeros(n, 3)).to(torch.float64)
    K = torch.zeros(n, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    out = init.clone()
    out[:, :3, :3] = torch.linalg.matrix_exp(K) @ init[:, :3, :3]
    out[:, :3, 3] = init[:, :3, 3] + dt
    return out


def refine_view_poses(renderer: NeRFRenderer, test_data, poses: Dict[int, torch.Tensor], iters: int, lr: float = 1e-3,
                      rays_per_view: int = 256, chunk_size: int = 1024 * 4, seed: int = 0,
                      log=print, fxy=None, loss: str = "mse", loss_scale: float = 0.1) -> Dict[int, torch.Tensor]:
    """Photometric refinement of test poses on the frozen field: ``poses`` (view -> (4,4))
    are refined against their own images in groups of ``chunk_size // rays_per_view`` views,
    ``iters`` steps of ``engine.PoseRefiner`` per group with ``rays_per_view`` random pixels
    of every view of the group.  Sampling jitter follows the render config; the density
    noise of training (``raw_noise_std``) is off.  Every draw comes from a generator seeded
    with ``seed`` and the group's first view, so a view's result does not depend on the
    groups before it.  ``fxy`` (optional): learned focal lengths (fx, fy), used as fixed
    values in place of ``test_data.focal``.  ``loss`` / ``loss_scale``: the refiner's
    photometric loss (``engine.PoseRefiner``)."""
    import dataclasses
    from types import SimpleNamespace

    from . import ops
    from .data_pose_opt import PixelBatch, PixelDataset, PixelSampler
    from .engine import PoseRefiner
    from .train_pose_opt import CameraPoseParameters

    if rays_per_view < 1 or rays_per_view > chunk_size:
        raise ValueError(f"refine_rays_per_view must be in [1, chunk_size = {chunk_size}], got {rays_per_view}")
    views = sorted(poses)
    per_group = max(1, chunk_size // rays_per_view)
    rc = dataclasses.replace(renderer.config, raw_noise_std=0.0)
    H, W = test_data.H, test_data.W
    out: Dict[int, torch.Tensor] = {}
    with torch.enable_grad():
        for g0 in range(0, len(views), per_group):
            group = views[g0:g0 + per_group]
            dev = test_data.images.device
            init = torch.stack([poses[v].to(dev).float() for v in group])
            ds = PixelDataset(SimpleNamespace(H=H, W=W, focal=test_data.focal, images=test_data.images[group]))
            sampler = PixelSampler(ds, batch_size=len(group) * rays_per_view)
            cam = CameraPoseParameters(init, fixed_small_angle=True).to(dev)
            gen = torch.Generator(device=dev).manual_seed(int(seed) + int(group[0]))
            base = (torch.arange(len(group), device=dev) * (H * W)).repeat_interleave(rays_per_view)
            B = base.numel()
            first = last = None
            fxy_dev = torch.tensor(fxy, device=dev, dtype=torch.float32) if fxy is not None else None
            with PoseRefiner(renderer.model_coarse, renderer.model_fine, cam, sampler, rc, pose_lr=lr,
                             fxy=fxy_dev, loss=loss, loss_scale=loss_scale) as refiner:
                for _ in range(iters):
                    idx = base + torch.randint(0, H * W, (B,), device=dev, generator=gen)
                    img, pix, rgb = ops.gather_pixels(idx, ds.images, validate=False)
                    t_rand = torch.rand(B, rc.num_samples, device=dev, generator=gen) if rc.perturb else None
                    u = torch.rand(B, rc.num_samples_fine, device=dev, generator=gen)
                    last = refiner.step(PixelBatch(img, pix, rgb, in_range=True), t_rand=t_rand, u=u)["loss"]
                    first = last if first is None else first
            with torch.no_grad():
                refined = cam.get_all_poses()
            for k, v in enumerate(group):
                out[v] = refined[k].detach()
            if first is not None:
                log(f"  refined views {group[0]}..{group[-1]}: loss {float(first):.5f} -> {float(last):.5f} "
                    f"({iters} steps of {B} rays)")
    return out


@torch.no_grad()
def evaluate_test_set(renderer: NeRFRenderer, test_data, output_dir: Path, noise_config: NoiseConfig,
                      device: str = "cuda", chunk_size: int = 1024 * 4, process_group=None,
                      save_images: bool = True, log=print, fused_tail: bool = False, *,
                      view_indices: Optional[Sequence[int]] = None, mode: str = "test",
                      refine_iters: int = 0, refine_lr: float = 1e-3, refine_rays_per_view: int = 256,
                      refine_seed: int = 0, align_train_poses=None, fxy=None, refine_loss: str = "mse",
                      refine_loss_scale: float = 0.1) -> Dict[str, object]:
    """Reference inference.py:145-318 (same per-image records, summary keys and files),
    sharded over ``process_group``'s ranks when one is given.  ``fused_tail``: the metrics
    of a view come from ``metrics.image_metrics`` (fp64 SSIM, one read-back) and its PNGs
    from the frame kernels (device only, no CPU fallback).  ``view_indices`` restricts the
    evaluation to those test views (the noise of every view is still drawn, so a view sees
    the pose it sees in the full run); ``mode`` is recorded in ``experiment_config.json``.

    ``align_train_poses`` = (optimised train poses, ground-truth train poses): the test
    poses are carried into the learned frame (``pose_eval``) before the noise is drawn.
    ``refine_iters`` > 0: each rank then refines the poses of the views it renders
    (``refine_view_poses``; no collective) under the photometric loss ``refine_loss`` at scale
    ``refine_loss_scale``, which the ``pose_refinement`` block records.  With either, every per-image record gains
    ``pose_rotation_error_deg_before/after`` and ``pose_translation_error_before/after``
    (against the ground truth in the frame the view is rendered in) and
    ``test_metrics.json`` a ``pose_refinement`` block; without, nothing changes.
    ``fxy`` (optional): focal lengths (fx, fy) the checkpoint learned; the views are rendered
    (and refined) with them instead of ``test_data.focal``."""
    rank, world = 0, 1
    if process_group is not None:
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    pose_eval_on = refine_iters > 0 or align_train_poses is not None
    clean, sim3 = None, None
    if align_train_poses is not None:
        from .pose_eval import align_sim3, to_learned_frame
        sim3 = align_sim3(*align_train_poses)
        clean = to_learned_frame(sim3, test_data.poses).to(test_data.poses.device, torch.float32)
    views = _rank0_draws(_noisy_poses(test_data, noise_config, clean), noise_config, process_group)
    lpips_metric = LPIPSMetric(device=device)
    order = list(range(test_data.images.shape[0])) if view_indices is None else [int(i) for i in view_indices]
    n_images = len(order)
    if rank == 0:
        log(f"Evaluating {n_images} test images on {world} rank(s)...")
    mine = []
    refined = {}
    if refine_iters > 0:
        refined = refine_view_poses(renderer, test_data, {i: views[i][0] for i in order[rank::world]}, refine_iters,
                                    lr=refine_lr, rays_per_view=refine_rays_per_view, chunk_size=chunk_size,
                                    seed=refine_seed, log=log, fxy=fxy, loss=refine_loss,
                                    loss_scale=refine_loss_scale)
    for i in order[rank::world]:
        pose, noise_info = views[i]
        pose_rec = {}
        if pose_eval_on:
            from .pose_eval import pose_error
            gt = (test_data.poses[i] if clean is None else clean[i]).detach().cpu().double()
            after = refined.get(i, pose)
            eb, ea = pose_error(gt, pose.detach().cpu().double()), pose_error(gt, after.detach().cpu().double())
            pose_rec = {"pose_rotation_error_deg_before": eb["rotation_error_deg"],
                        "pose_rotation_error_deg_after": ea["rotation_error_deg"],
                        "pose_translation_error_before": eb["translation_error"],
                        "pose_translation_error_after": ea["translation_error"]}
            pose = after
        target = test_data.images[i]
        start = time.time()
        out = _render(renderer, pose, test_data.H, test_data.W, test_data.focal, chunk_size, fxy)
        pred = out["rgb"]
        torch.cuda.synchronize() if pred.is_cuda else None
        if fused_tail:
            m = image_metrics(pred, target)
            rec = {"image": i, "psnr": m["psnr"], "ssim": m["ssim"], "mse": m["mse"],
                   "render_time": time.time() - start}
        else:
            rec = {"image": i, "psnr": compute_psnr(pred, target).item(), "ssim": compute_ssim(pred, target).item(),
                   "mse": compute_mse(pred, target).item(), "render_time": time.time() - start}
        if noise_info:
            rec.update({f"noise_{k}": v for k, v in noise_info.items()})
        rec.update(pose_rec)
        lp = lpips_metric(pred, target) if lpips_metric.available else None
        if lp is not None:
            rec["lpips"] = lp.item()
        mine.append(rec)
        if save_images:
            _save_view(output_dir, i, pred, target, out["depth"], fused_tail)
        log(f"  Image {i + 1}/{n_images}: PSNR={rec['psnr']:.2f}, SSIM={rec['ssim']:.4f}, "
            f"time={rec['render_time']:.2f}s")
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, mine, group=process_group)
        per_image = sorted((r for part in gathered for r in part), key=lambda r: r["image"])
    else:
        per_image = mine
    psnr = [r["psnr"] for r in per_image]
    ssim = [r["ssim"] for r in per_image]
    mse = [r["mse"] for r in per_image]
    avg = {"psnr_mean": float(np.mean(psnr)), "psnr_std": float(np.std(psnr)), "ssim_mean": float(np.mean(ssim)),
           "ssim_std": float(np.std(ssim)), "mse_mean": float(np.mean(mse)), "mse_std": float(np.std(mse)),
           "n_images": n_images}
    lp = [r["lpips"] for r in per_image if "lpips" in r]
    if lp:
        avg["lpips_mean"], avg["lpips_std"] = float(np.mean(lp)), float(np.std(lp))
    if noise_config.has_noise:
        rot = [r.get("noise_rotation_error_deg", 0) for r in per_image]
        tr = [r.get("noise_translation_error", 0) for r in per_image]
        avg["noise_config"] = {"rotation_noise_deg": noise_config.rotation_noise_deg,
                               "translation_noise": noise_config.translation_noise, "seed": noise_config.seed}
        avg["actual_noise"] = {"rotation_error_mean_deg": float(np.mean(rot)),
                               "rotation_error_std_deg": float(np.std(rot)),
                               "translation_error_mean": float(np.mean(tr)),
                               "translation_error_std": float(np.std(tr))}
    if pose_eval_on:
        avg["pose_refinement"] = {
            "iters": refine_iters, "lr": refine_lr, "rays_per_view": refine_rays_per_view, "seed": refine_seed,
            "loss": refine_loss, "loss_scale": refine_loss_scale,
            "views_per_group": max(1, chunk_size // max(1, refine_rays_per_view)),
            "aligned_train_poses": sim3 is not None, "sim3": sim3.to_json() if sim3 is not None else None,
            **{f"{k}_mean": float(np.mean([r[k] for r in per_image])) for k in (
                "pose_rotation_error_deg_before", "pose_rotation_error_deg_after",
                "pose_translation_error_before", "pose_translation_error_after")}}
    if rank == 0:
        (output_dir / "per_image_metrics.json").write_text(json.dumps(per_image, indent=2))
        (output_dir / "test_metrics.json").write_text(json.dumps(avg, indent=2))
        (output_dir / "experiment_config.json").write_text(json.dumps({
            "mode": mode,
            "noise_config": {"rotation_noise_deg": noise_config.rotation_noise_deg,
                             "translation_noise": noise_config.translation_noise, "seed": noise_config.seed},
            "timestamp": datetime.now().isoformat(), "output_dir": str(output_dir), "ranks": world}, indent=2))
    return avg


def _noisy_frame_poses(poses: torch.Tensor, noise_config: NoiseConfig):
    """Every video frame's noisy pose in frame order, as the reference's loop draws them
    (inference.py:383-402), in the (pose, info) form of ``_noisy_poses``."""
    if noise_config.seed is not None:
        set_noise_seed(noise_config.seed)
    out = []
    for i in range(poses.shape[0]):
        pose = poses[i]
        if noise_config.has_noise:
            pose, _ = add_noise_to_pose(pose, rotation_noise_deg=noise_config.rotation_noise_deg,
                                        translation_noise=noise_config.translation_noise)
        out.append((pose, {}))
    return out


@torch.no_grad()
def render_video(renderer: NeRFRenderer, poses: torch.Tensor, H: int, W: int, focal: float, output_dir: Path,
                 noise_config: NoiseConfig, fps: int = 30, chunk_size: int = 1024 * 4, *, process_group=None,
                 fused_tail: bool = False, log=print, fxy=None) -> Path:
    """Reference inference.py:365-443: ``frames/frame_%04d.png``, ``video_config.json`` and,
    where ``ffmpeg`` runs, ``video.mp4`` (otherwise the frames directory is returned).
    Every frame's noise is drawn up front in frame order on every rank, so the poses equal
    the reference's sequential run; with a process group rank r renders frames r, r+N, ...
    and rank 0 alone writes the JSON and runs ``ffmpeg``.  ``fused_tail``: frames are
    quantised on the device (``frame_u8``) and cross to the host as bytes.  ``fxy``
    (optional): learned focal lengths (fx, fy) in place of ``focal``."""
    rank, world = 0, 1
    if process_group is not None:
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    output_dir = Path(output_dir)
    frames_dir = output_dir / "frames"
    frames_dir.mkdir(parents=True, exist_ok=True)
    frames = _rank0_draws(_noisy_frame_poses(poses, noise_config), noise_config, process_group)
    n_frames = len(frames)
    if rank == 0:
        log(f"Rendering {n_frames} frames on {world} rank(s)...")
        if noise_config.has_noise:
            log(f"  With noise: rot={noise_config.rotation_noise_deg}°, trans={noise_config.translation_noise}")
    for i in range(rank, n_frames, world):
        rgb = _render(renderer, frames[i][0], H, W, focal, chunk_size, fxy)["rgb"]
        path = frames_dir / f"frame_{i:04d}.png"
        if fused_tail:
            save_frame_u8(frame_u8(rgb), path)
        else:
            save_image(rgb, path)
        if (i + 1) % 10 == 0:
            log(f"  Rendered {i + 1}/{n_frames} frames")
    if world > 1:
        dist.barrier(process_group)
    result = [frames_dir]
    if rank == 0:
        (output_dir / "video_config.json").write_text(json.dumps({
            "n_frames": n_frames, "fps": fps,
            "noise_config": {"rotation_noise_deg": noise_config.rotation_noise_deg,
                             "translation_noise": noise_config.translation_noise, "seed": noise_config.seed},
            "timestamp": datetime.now().isoformat()}, indent=2))
        video_path = output_dir / "video.mp4"
        try:
            import subprocess
            subprocess.run(["ffmpeg", "-y", "-framerate", str(fps), "-i", str(frames_dir / "frame_%04d.png"),
                            "-c:v", "libx264", "-pix_fmt", "yuv420p", str(video_path)], check=True,
                           capture_output=True)
            log(f"Video saved to {video_path}")
            result = [video_path]
        except Exception as e:  # no ffmpeg, or it failed: the frames are the result (reference :438-441)
            log(f"Could not create video (ffmpeg required): {e}")
            log(f"Frames saved to {frames_dir}")
    if world > 1:
        dist.broadcast_object_list(result, src=dist.get_global_rank(process_group, 0), group=process_group)
    return result[0]


def build_arg_parser():
    """Reference inference.py:448-503 flags (same names and defaults) plus ``--precision``
    and ``--image_index``."""
    import argparse
    ap = argparse.ArgumentParser(
        prog="python -m noisy_src.inference", description="NeRF inference with optional camera noise (MI355X HIP path)",
        formatter_class=argparse.RawDescriptionHelpFormatter,
        epilog="Examples:\n"
               "  python -m noisy_src.inference checkpoint.pt --mode test --rotation_noise 1.0 --noise_seed 42\n"
               "  python -m noisy_src.inference checkpoint.pt --mode video --rotation_noise 0.5\n"
               "  python -m noisy_src.inference checkpoint.pt --mode single --image_index 3\n")
    ap.add_argument("checkpoint", type=Path, help="Path to checkpoint file")
    ap.add_argument("--mode", type=str, default="test", choices=["test", "video", "single"], help="Inference mode")
    ap.add_argument("--scene", type=str, default=None, help="Scene name (auto-detected from config if not provided)")
    ap.add_argument("--data_root", type=Path, default=None, help="Data root directory")
    ap.add_argument("--output_dir", type=Path, default=None, help="Output directory (auto-generated if not provided)")
    ap.add_argument("--device", type=str, default="cuda", help="Device")
    ap.add_argument("--precision", type=str, default=None, choices=["fp32", "bf16", "fp16"],
                    help="MLP operand precision (default: the checkpoint's own; fp32 = the reference's numerics)")
    ap.add_argument("--image_index", type=int, default=0, help="Test view rendered by --mode single")
    noise = ap.add_argument_group("Noise Options")
    noise.add_argument("--rotation_noise", type=float, default=0.0,
                       help="Rotation noise std in degrees (default: 0 = no noise)")
    noise.add_argument("--translation_noise", type=float, default=0.0,
                       help="Translation noise std in scene units (default: 0 = no noise)")
    noise.add_argument("--noise_seed", type=int, default=None, help="Random seed for reproducible noise")
    video = ap.add_argument_group("Video Options")
    video.add_argument("--n_frames", type=int, default=120, help="Number of frames for video")
    video.add_argument("--fps", type=int, default=30, help="Video FPS")
    pose = ap.add_argument_group("Pose Evaluation Options (pose-optimised checkpoints; --mode test / single)")
    pose.add_argument("--align_train_poses", action="store_true",
                      help="Carry the test poses into the learned frame: Sim(3) alignment of the checkpoint's "
                           "optimised train poses with the train split's ground truth")
    pose.add_argument("--refine_poses", type=int, default=0, metavar="ITERS",
                      help="Photometric test-time refinement steps per group of views on the frozen field (0 = off)")
    pose.add_argument("--refine_lr", type=float, default=1e-3, help="Pose learning rate of the refinement")
    pose.add_argument("--refine_rays_per_view", type=int, default=256,
                      help="Random pixels per view and step (views are grouped chunk_size // this at a time)")
    pose.add_argument("--refine_seed", type=int, default=0, help="Seed of the refinement's pixel and sample draws")
    pose.add_argument("--refine_loss", type=str, default="mse", choices=list(LOSS_KINDS),
                      help="Photometric loss of the refinement (robust kernels down-weight misrendered rays)")
    pose.add_argument("--refine_loss_scale", type=float, default=0.1,
                      help="Scale c of a robust --refine_loss in colour units (0.1 is a choice, not a tuned value)")
    perf = ap.add_argument_group("Performance Options")
    perf.add_argument("--chunk_size", type=int, default=1024 * 4, help="Rays per chunk (default: 4096)")
    return ap


def main(argv=None) -> None:
    """``python -m noisy_src.inference`` (reference inference.py:446-612), or under
    ``torchrun``: the test views / video frames are sharded over the ranks."""
    from .data import load_blender_data
    from .engine import init_distributed

    a = build_arg_parser().parse_args(argv)
    noise_config = NoiseConfig(rotation_noise_deg=a.rotation_noise, translation_noise=a.translation_noise,
                               seed=a.noise_seed)
    pg, rank, world, device = init_distributed(a.device)
    log = print if rank == 0 else (lambda *_, **__: None)
    try:
        log(f"Loading checkpoint: {a.checkpoint}")
        renderer, config, iteration = load_checkpoint(a.checkpoint, device, precision=a.precision)
        log(f"Loaded model from iteration {iteration}")
        fxy = checkpoint_intrinsics(a.checkpoint)
        if fxy is not None:
            log(f"Learned focal lengths: fx {fxy[0]:.4f}, fy {fxy[1]:.4f} (used in place of the dataset's)")
            if len(fxy) == 6:
                log(f"Learned lens: cx {fxy[2]:.4f}, cy {fxy[3]:.4f}, k1 {fxy[4]:.6f}, k2 {fxy[5]:.6f}")
        scene = a.scene or config.get("data", {}).get("scene_name", "lego")
        log(f"Scene: {scene}")
        if a.output_dir is None:
            name = [generate_output_folder_name(a.mode, noise_config, scene)]
            if world > 1:  # one shared directory name for all ranks (rank 0's timestamp)
                import torch.distributed as dist
                dist.broadcast_object_list(name, src=0, group=pg)
            output_dir = a.checkpoint.parent / name[0]
        else:
            output_dir = a.output_dir
        log(f"Output directory: {output_dir}")
        data_root = a.data_root if a.data_root is not None else Path(__file__).resolve().parents[1] / "data" / "raw"
        img_scale = config.get("data", {}).get("img_scale", 0.5)
        fused = device.startswith("cuda")
        bar = "=" * 60
        if a.mode in ("test", "single"):
            log("\nLoading test data...")
            test_data = load_blender_data(data_root, scene, "test", img_scale, device)
            only = None
            if a.mode == "single":
                if not 0 <= a.image_index < test_data.images.shape[0]:
                    raise SystemExit(f"--image_index {a.image_index} is outside the {test_data.images.shape[0]} "
                                     "test views")
                only = [a.image_index]
            log(f"\n{bar}\n" + ("Test Set Evaluation" if only is None else f"Test view {a.image_index}"))
            if noise_config.has_noise:
                log(f"  Rotation noise:    {noise_config.rotation_noise_deg}° (std)")
                log(f"  Translation noise: {noise_config.translation_noise} (std)")
                if noise_config.seed is not None:
                    log(f"  Noise seed:        {noise_config.seed}")
            else:
                log("  Mode: Clean (no noise)")
            log(f"{bar}\n")
            align = None
            if a.align_train_poses:
                train_data = load_blender_data(data_root, scene, "train", img_scale, device)
                align = (checkpoint_train_poses(a.checkpoint), train_data.poses)
                log("  Test poses carried into the learned frame (Sim(3) alignment of the train poses)")
            if a.refine_poses > 0:
                log(f"  Test-time pose refinement: {a.refine_poses} steps, lr {a.refine_lr}, "
                    f"{a.refine_rays_per_view} rays per view"
                    + ("" if a.refine_loss == "mse" else f", {a.refine_loss} loss (c = {a.refine_loss_scale:g})"))
            m = evaluate_test_set(renderer, test_data, output_dir, noise_config, device, a.chunk_size,
                                  process_group=pg, log=log, fused_tail=fused, view_indices=only, mode=a.mode,
                                  refine_iters=a.refine_poses, refine_lr=a.refine_lr,
                                  refine_rays_per_view=a.refine_rays_per_view, refine_seed=a.refine_seed,
                                  align_train_poses=align, fxy=fxy, refine_loss=a.refine_loss,
                                  refine_loss_scale=a.refine_loss_scale)
            log(f"\n{bar}\nTest Set Results:")
            log(f"  PSNR:  {m['psnr_mean']:.2f} ± {m['psnr_std']:.2f} dB")
            log(f"  SSIM:  {m['ssim_mean']:.4f} ± {m['ssim_std']:.4f}")
            if "lpips_mean" in m:
                log(f"  LPIPS: {m['lpips_mean']:.4f} ± {m['lpips_std']:.4f}")
            if noise_config.has_noise and "actual_noise" in m:
                act = m["actual_noise"]
                log("\nActual Noise Applied:")
                log(f"  Rotation error:    {act['rotation_error_mean_deg']:.3f} ± {act['rotation_error_std_deg']:.3f}°")
                log(f"  Translation error: {act['translation_error_mean']:.4f} ± {act['translation_error_std']:.4f}")
            if "pose_refinement" in m:
                pr = m["pose_refinement"]
                log("\nTest poses (before -> after refinement):")
                log(f"  Rotation error:    {pr['pose_rotation_error_deg_before_mean']:.3f} -> "
                    f"{pr['pose_rotation_error_deg_after_mean']:.3f}°")
                log(f"  Translation error: {pr['pose_translation_error_before_mean']:.4f} -> "
                    f"{pr['pose_translation_error_after_mean']:.4f}")
            log(f"{bar}\nResults saved to: {output_dir}")
        else:
            log("\nLoading data for camera parameters...")
            data = load_blender_data(data_root, scene, "train", img_scale, device)
            log("\nGenerating spiral poses...")
            poses = create_spiral_poses(n_frames=a.n_frames, device=device)
            log("\nRendering video...")
            video_path = render_video(renderer, poses, data.H, data.W, data.focal, output_dir, noise_config, a.fps,
                                      chunk_size=a.chunk_size, process_group=pg, fused_tail=fused, log=log,
                                      fxy=fxy)
            log(f"Video saved to: {video_path}")
        log("\nDone!")
    finally:
        if pg is not None:
            import torch.distributed as dist
            dist.destroy_process_group()


__all__ = ["load_checkpoint", "render_image", "save_image", "depth_to_colormap", "frame_u8", "depth_frame_u8",
           "save_frame_u8", "generate_output_folder_name", "create_spiral_poses", "evaluate_test_set", "render_video",
           "checkpoint_train_poses", "refine_view_poses", "intrinsics_fxy", "checkpoint_intrinsics", "main"]

if __name__ == "__main__":
    main()
