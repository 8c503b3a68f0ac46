"""
What the two training loops (``train.train``, ``train_pose_opt.train_with_pose_optimization``)
and their command lines share, as plain functions around the step: opening a run
(``open_run``, ``create_nerf_for``, ``write_experiment_config``); per iteration the random
draws (``draw_randoms``, ``slice_for_rank``), the lagged read-back behind the CSV row and the
console line (``IterationLog``) and the validation / checkpoint cadence (``due``);
``evaluate_views``; the checkpoint both start from (``base_checkpoint``, ``write_checkpoint``);
the shared flags and set-up of the CLIs (``add_common_args``, ``run_cli``).  Each loop keeps
its own step (``engine`` / ``graphed``), validation and checkpoint bodies and wording.
"""

from __future__ import annotations

import json
import math
import random
import time
from collections import namedtuple
from datetime import datetime
from pathlib import Path
from typing import Callable, Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from .config import DataConfig, ModelConfig, NeRFConfig, RenderConfig, TrainConfig
from .engine import LaggedScalars, check_run_args, init_distributed, mean_over_ranks, rank_slice
from .logger import ExperimentLogger, TrainingMetrics, ValidationMetrics
from .metrics import LPIPSMetric, compute_mse, compute_psnr, compute_ssim
from .model import create_nerf
from .noise import NoiseConfig
from .ops import LOSS_KINDS


def set_seed(seed: int) -> None:
    """Reference train.py:36-42, train_pose_opt.py:44-50."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


# what ``open_run`` hands a loop; ``logger`` and ``lpips_metric`` are None off rank 0
Run = namedtuple("Run", "rank world device output_dir logger lpips_metric")


def open_run(config: NeRFConfig, exp_name: str, process_group, graph: bool, who: str,
             train_data=None, val_data=None) -> Run:
    """The head of a training run: ``check_run_args``, then the backend check of a
    data-parallel graph run (both raise ValueError before any work), the seed, the device
    check, and on rank 0 the output directory with its logger and ``config.json``."""
    import torch.distributed as dist

    rank, world = 0, 1
    if process_group is not None:
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    check_run_args(config, world, train_data, val_data)
    if graph and world > 1 and dist.get_backend(process_group) != "nccl":
        # the captured step contains the all-reduces: only RCCL collectives are graph-capturable
        raise ValueError(f"{who}(graph=True) with data parallelism needs the nccl (RCCL) backend")
    set_seed(config.train.seed)
    device = config.train.device
    if device.startswith("cuda") and not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a ROCm device (the reference falls back to its CPU path; this framework "
                           "has no CPU path)")
    output_dir = Path(config.train.output_dir) / exp_name
    logger = lpips_metric = None
    if rank == 0:
        logger = ExperimentLogger(output_dir, exp_name, use_tensorboard=True)
        logger.log_config(config)
        lpips_metric = LPIPSMetric(device=device)
        if not lpips_metric.available:
            lpips_metric = None
    return Run(rank, world, device, output_dir, logger, lpips_metric)


def create_nerf_for(config: NeRFConfig, device, logger: Optional[ExperimentLogger] = None):
    """create_nerf + .to(device); no fine network without hierarchical sampling
    (train_pose_opt.py:772-777).  A logger records the parameter counts."""
    mc, mf = create_nerf(config.model)
    mc = mc.to(device)
    mf = mf.to(device) if config.render.use_hierarchical else None
    if logger is not None:
        logger.log_model_info(mc, "model_coarse")
        if mf is not None:
            logger.log_model_info(mf, "model_fine")
    return mc, mf


def noise_dict(noise_config: NoiseConfig) -> dict:
    return {"rotation_noise_deg": noise_config.rotation_noise_deg, "translation_noise": noise_config.translation_noise,
            "translation_noise_pct": noise_config.translation_noise_pct, "seed": noise_config.seed}


NO_NOISE = {"rotation_noise_deg": 0, "translation_noise": 0, "translation_noise_pct": 0, "seed": None,
            "has_noise": False}


def write_experiment_config(output_dir: Path, config: NeRFConfig, exp_name: str, world: int,
                            noise_config: Optional[NoiseConfig], no_noise=None, *, after_name: Optional[dict] = None,
                            after_batch: Optional[dict] = None, extra: Optional[dict] = None) -> None:
    """``experiment_config.json`` in the reference's key order (train.py:380-398,
    train_pose_opt.py:800-823).  ``no_noise`` is what ``noise_config`` reads without noise:
    ``NO_NOISE`` in train.py, null in train_pose_opt.py.  The three dicts are a loop's own
    keys: after ``experiment_name``, after ``batch_size`` and at the end."""
    nc = noise_config
    (Path(output_dir) / "experiment_config.json").write_text(json.dumps({
        "scene": config.data.scene_name, "experiment_name": exp_name, **(after_name or {}),
        "noise_config": {**noise_dict(nc), "has_noise": nc.has_noise} if nc else no_noise,
        "num_iterations": config.train.num_iterations, "batch_size": config.data.batch_size, **(after_batch or {}),
        "timestamp": datetime.now().isoformat(), "data_parallel_ranks": world, **(extra or {})}, indent=2))


def draw_randoms(n: int, render_config: RenderConfig, has_fine: bool, device):
    """The global random draws of one step, in the reference's order (jitter, then
    inverse-CDF uniforms: rendering.py:161 -> rays.py:204, :255), identical on every rank."""
    rc = render_config
    t_rand = torch.rand(n, rc.num_samples, device=device) if rc.perturb else None
    u = torch.rand(n, rc.num_samples_fine, device=device) if (rc.use_hierarchical and has_fine) else None
    return t_rand, u


def slice_for_rank(n: int, rank: int, world: int, *tensors):
    """(this rank's slice of a global batch of n, the tensors cut to it; None stays None)."""
    sl = rank_slice(n, rank, world) if world > 1 else slice(0, n)
    return sl, tuple(None if t is None else t[sl] for t in tensors)


# TrainingMetrics' columns for a lens, pushed as extra scalars by train_pose_opt
LENS_COLUMNS = ("lens_cx", "lens_cy", "lens_k1", "lens_k2")


class IterationLog:
    """One row of train_metrics.csv and, every ``log_every``, one console line per
    iteration, from scalars read back one iteration late (``engine.LaggedScalars``: no
    per-step host sync).  ``line(vm, lr, rays_per_sec, meta)`` is the loop's own middle
    part of the console line, between the PSNR and the elapsed time.  Every rank pushes
    (the mean over the ranks is a collective); only rank 0 has a ``logger`` and writes."""

    def __init__(self, logger: Optional[ExperimentLogger], config: NeRFConfig, process_group, line: Callable,
                 log=print):
        self.logger, self.process_group, self.line, self.log = logger, process_group, line, log
        self.batch_size = config.data.batch_size
        self.num_iterations, self.log_every = config.train.num_iterations, config.train.log_every
        self.lagged = LaggedScalars()
        self.start = self.t_prev = time.time()

    def push(self, iteration: int, metrics: Dict[str, torch.Tensor], lr: float,
             extra_scalars: Optional[Dict[str, torch.Tensor]] = None, meta=None) -> None:
        """Queue this iteration's losses (and ``extra_scalars``, device scalars as well);
        write the previous iteration's row."""
        keys = ["loss", "loss_coarse"] + [k for k in ("loss_fine", "loss_distortion", "mse_coarse", "mse_fine")
                                          if k in metrics]
        vals = [metrics[k] for k in keys]
        if extra_scalars:
            keys += extra_scalars
            vals += extra_scalars.values()
        now = time.time()
        self._write(self.lagged.push(mean_over_ranks(vals, self.process_group),
                                     (iteration, keys, lr, now - self.t_prev, meta)))
        self.t_prev = now

    def flush(self) -> None:
        """Write the pending row now (before a validation or checkpoint, and at the end)."""
        self._write(self.lagged.flush())

    def pause(self) -> None:
        """After a validation or checkpoint: the next iteration's time excludes it."""
        self.t_prev = time.time()

    def minutes(self) -> float:
        return (time.time() - self.start) / 60

    def _write(self, done) -> None:
        if done is None or self.logger is None:
            return
        vals, (it, keys, lr, batch_time, meta) = done
        vm = dict(zip(keys, vals))
        # under a robust photometric loss the plain MSE rides along (mse_*): a PSNR stays a PSNR
        last = vm.get("mse_fine", vm.get("mse_coarse", vm.get("loss_fine", vm["loss_coarse"])))
        psnr = -10.0 * math.log10(last) if last > 0 else float("inf")
        rays_per_sec = self.batch_size / batch_time
        self.logger.log_training(TrainingMetrics(iteration=it, loss=vm["loss"], loss_coarse=vm["loss_coarse"],
                                                 loss_fine=vm.get("loss_fine"), psnr=psnr, learning_rate=lr,
                                                 time_per_iter=batch_time, rays_per_sec=rays_per_sec,
                                                 focal_error_pct=vm.get("focal_error_pct"),
                                                 **{k: vm[k] for k in LENS_COLUMNS if k in vm}))
        if it % self.log_every == 0:
            self.log(f"[{it:7d}/{self.num_iterations}] loss: {vm['loss']:.5f} | psnr: {psnr:.2f} | "
                     f"{self.line(vm, lr, rays_per_sec, meta)} | time: {self.minutes():.1f}min")


def due(iteration: int, val_every: int, save_every: int) -> Optional[str]:
    """"val" on a validation iteration (which also checkpoints), "save" on a plain
    checkpoint iteration, else None; never at iteration 0."""
    if iteration > 0:
        if iteration % val_every == 0:
            return "val"
        if iteration % save_every == 0:
            return "save"
    return None


@torch.no_grad()
def evaluate_views(render_view: Callable, views: Iterable[Tuple[str, object, torch.Tensor]],
                   logger: Optional[ExperimentLogger] = None, iteration: int = 0,
                   lpips_metric: Optional[LPIPSMetric] = None) -> ValidationMetrics:
    """Reference train.py:163-233, train_pose_opt.py:474-545: mean PSNR / SSIM / MSE (+ LPIPS
    when available) over ``views``, each ``(tag, view, target)`` with ``render_view(view)``
    -> {"rgb", "depth"}; PNGs of the first three under their tags when a logger is given."""
    psnr, ssim, mse, lp = [], [], [], []
    for i, (tag, view, target) in enumerate(views):
        out = render_view(view)
        pred = out["rgb"]
        mse.append(compute_mse(pred, target).item())
        psnr.append(compute_psnr(pred, target).item())
        ssim.append(compute_ssim(pred, target).item())
        if lpips_metric is not None:
            v = lpips_metric(pred, target)
            if v is not None:
                lp.append(v.item())
        if logger is not None and i < 3:
            logger.log_images(tag, pred, target, iteration, depth=out["depth"])
    return ValidationMetrics(iteration=iteration, psnr=float(np.mean(psnr)), ssim=float(np.mean(ssim)),
                             mse=float(np.mean(mse)), lpips=float(np.mean(lp)) if lp else None,
                             per_image_psnr=psnr, per_image_ssim=ssim)


def _plain(d: dict) -> dict:
    """Config values made plain (Path -> str, tuple -> list) so that the file reads back
    with ``torch.load(..., weights_only=True)``."""
    return {k: str(v) if isinstance(v, Path) else list(v) if isinstance(v, tuple) else v for k, v in d.items()}


def checkpoint_config(config: NeRFConfig) -> dict:
    """The reference's ``checkpoint["config"]`` (train.py:256-264).  ``ModelConfig.precision``
    (an MI355X-only field) is left out so the reference's ``ModelConfig(**cfg["model"])``
    accepts it; it travels under ``checkpoint["mi355x"]``."""
    model = {k: v for k, v in config.model.__dict__.items() if k != "precision"}
    return {"model": _plain(model), "render": _plain(config.render.__dict__), "data": _plain(config.data.__dict__),
            "train": _plain(config.train.__dict__)}


def base_checkpoint(iteration: int, model_coarse, model_fine, config: NeRFConfig, noise_config=None,
                    metrics: Optional[Dict] = None) -> dict:
    """What both loops' checkpoints hold (reference train.py:236-286): iteration, the
    networks' state dicts in nn.Linear naming, the config as plain dicts, and ``metrics`` /
    ``noise_config`` when given.  The loops add their optimizer (and pose) entries."""
    ckpt = {"iteration": iteration, "model_coarse": model_coarse.state_dict(), "config": checkpoint_config(config),
            "mi355x": {"precision": getattr(config.model, "precision", "fp32")}}
    if model_fine is not None:
        ckpt["model_fine"] = model_fine.state_dict()
    if metrics is not None:
        ckpt["metrics"] = metrics
    if noise_config is not None:
        ckpt["noise_config"] = noise_dict(noise_config)
    return ckpt


def write_checkpoint(output_dir, iteration: int, ckpt: dict, is_best: bool = False) -> None:
    """The reference's file names: the numbered checkpoint, ``checkpoint_latest.pt`` and, on
    a new best validation PSNR, ``checkpoint_best.pt``."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    torch.save(ckpt, output_dir / f"checkpoint_{iteration:07d}.pt")
    torch.save(ckpt, output_dir / "checkpoint_latest.pt")
    if is_best:
        torch.save(ckpt, output_dir / "checkpoint_best.pt")


# the flags both training command lines have, with the reference's names and defaults
# (train.py:580-657, train_pose_opt.py:1057-1142); --num_iters and --val_every default per CLI
COMMON_ARGS = {
    "scene": dict(type=str, default="lego"), "data_root": dict(type=str, default=None),
    "img_scale": dict(type=float, default=0.5), "batch_size": dict(type=int, default=1024),
    "num_iters": dict(type=int), "lr": dict(type=float, default=5e-4),
    "no_hierarchical": dict(action="store_true"), "num_samples": dict(type=int, default=64),
    "num_samples_fine": dict(type=int, default=128),
    "rotation_noise": dict(type=float, default=0.0), "translation_noise": dict(type=float, default=0.0),
    "translation_noise_pct": dict(type=float, default=0.0), "noise_seed": dict(type=int, default=None),
    "log_every": dict(type=int, default=100), "val_every": dict(type=int), "save_every": dict(type=int, default=10000),
    "output_dir": dict(type=str, default="outputs"), "device": dict(type=str, default="cuda"),
    "seed": dict(type=int, default=42),
    "precision": dict(type=str, default="fp32", choices=["fp32", "bf16", "fp16"],
                      help="MLP operand precision (fp32 = the reference's numerics)"),
    "distortion_weight": dict(type=float, default=0.0,
                              help="weight of the distortion regulariser on the rendering network's ray weights "
                                   "(mip-NeRF 360; 0 = off, 0.01 is the paper's)"),
    "loss": dict(type=str, default="mse", choices=list(LOSS_KINDS),
                 help="photometric loss per colour channel (robust kernels down-weight rays that a wrong pose "
                      "lands on the wrong surface; the logged PSNR is always the plain MSE's)"),
    "loss_scale": dict(type=float, default=0.1,
                       help="scale c of a robust --loss in colour units: where it stops being quadratic (0.1 is a "
                            "choice, a tenth of the colour range, not a tuned value)"),
}


def add_common_args(ap, names: str, **overrides) -> None:
    """Add the ``COMMON_ARGS`` flags named in ``names`` (space separated) in that order; the
    two parsers place their own flags between different ones.  ``overrides``: per flag,
    ``add_argument`` keywords that replace the table's (a default, a help text)."""
    for name in names.split():
        ap.add_argument(f"--{name}", **{**COMMON_ARGS[name], **overrides.get(name, {})})


def loss_line(loss: str, loss_scale: float) -> str:
    """The console line's note of a robust photometric loss ("" under the MSE)."""
    return "" if loss == "mse" else f"{loss}(c={loss_scale:g}) | "


def noise_config_from_args(a) -> Optional[NoiseConfig]:
    """The training CLIs' pose noise: None unless one of the three noise flags is set."""
    if a.rotation_noise > 0 or a.translation_noise > 0 or a.translation_noise_pct > 0:
        return NoiseConfig(rotation_noise_deg=a.rotation_noise, translation_noise=a.translation_noise,
                           translation_noise_pct=a.translation_noise_pct, seed=a.noise_seed)
    return None


def nerf_config_from_args(a, device: str) -> NeRFConfig:
    return NeRFConfig(
        model=ModelConfig(precision=a.precision),
        render=RenderConfig(use_hierarchical=not a.no_hierarchical, num_samples=a.num_samples,
                            num_samples_fine=a.num_samples_fine),
        data=DataConfig(scene_name=a.scene, data_root=Path(a.data_root) if a.data_root else None,
                        img_scale=a.img_scale, batch_size=a.batch_size),
        train=TrainConfig(lr=a.lr, num_iterations=a.num_iters, output_dir=Path(a.output_dir), device=device,
                          seed=a.seed, log_every=a.log_every, val_every=a.val_every, save_every=a.save_every))


def run_cli(a, run_name: Callable, call: Callable) -> None:
    """A training command line after parsing, alone or under ``torchrun``: join the ranks,
    build the configs, agree on ``run_name(noise_config, world)`` (rank 0's, for its timestamp),
    ``call(config, noise_config, process_group, name)`` and leave the group."""
    import torch.distributed as dist

    noise_config = noise_config_from_args(a)
    pg, rank, world, device = init_distributed(a.device)
    cfg = nerf_config_from_args(a, device)
    name = [run_name(noise_config, world)]
    if pg is not None:
        dist.broadcast_object_list(name, src=0, group=pg)
    call(cfg, noise_config, pg, name[0])
    if pg is not None:
        dist.destroy_process_group()


__all__ = ["set_seed", "Run", "open_run", "create_nerf_for", "noise_dict", "NO_NOISE", "write_experiment_config",
           "draw_randoms", "slice_for_rank", "IterationLog", "due", "evaluate_views", "checkpoint_config",
           "base_checkpoint", "write_checkpoint", "COMMON_ARGS", "add_common_args", "loss_line",
           "noise_config_from_args", "nerf_config_from_args", "run_cli"]
