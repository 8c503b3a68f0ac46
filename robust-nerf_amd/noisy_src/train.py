"""
NeRF training entry point — drop-in for ShawnnnLiu/Robust-NeRF ``noisy_src/train.py``.

* ``train_step(renderer, optimizer, batch)`` keeps the reference's signature and
  returned metrics (train.py:68-119: host syncs for the logged scalars, joint clip at
  1.0 over both networks).  With the package's ``FusedAdam`` the clip folds into the
  fused update.
* ``train(config, noise_config)`` is the reference loop (train.py:307-577): seed,
  data (optionally with fixed pose noise), both networks, Adam + LambdaLR, one CSV
  row per iteration, validation + checkpoint every ``val_every`` (``checkpoint_best``
  on a new best PSNR), a plain checkpoint every ``save_every``, a final checkpoint,
  the final evaluation on every validation view and ``summary.json``.  The step
  itself is ``engine.Trainer`` (HIP kernels, no host syncs); the logged scalars are
  read once per iteration, one iteration late.  Everything around the step that
  ``train_pose_opt`` needs as well (opening the run, the draws, the iteration log, the
  validation / checkpoint cadence, the validation loop, the checkpoint's base, the
  shared flags) is ``run``'s; this module keeps what is its own.
* Data parallel (``torchrun --nproc-per-node N -m noisy_src.train ...``): every rank
  draws the SAME global batch and random numbers (identical seeds), takes its
  contiguous slice, and the gradients are averaged over RCCL inside
  the backward; ``--batch_size`` stays the global batch.  Rank 0 logs, validates and
  writes the checkpoints.
* ``save_checkpoint`` / ``load_checkpoint`` keep the reference's format; the MI355X
  precision knob is stored under a separate top-level key so the reference's
  ``ModelConfig(**cfg["model"])`` still loads the file.
"""

from __future__ import annotations

from datetime import datetime
from typing import Dict, Optional

import torch

from . import ops
from .config import NeRFConfig
from .data import BlenderData, RayDataset, RaySampler, create_data_loaders
from .engine import GraphedTrainer, Trainer
from .logger import ExperimentLogger, ValidationMetrics
from .metrics import LPIPSMetric, compute_psnr
from .noise import NoiseConfig
from .optim import FusedAdam, clip_grad_norm_
from .rays import get_ray_directions, get_rays
from .rendering import NeRFRenderer
from .run import (NO_NOISE, IterationLog, add_common_args, base_checkpoint, checkpoint_config,  # noqa: F401
                  create_nerf_for, draw_randoms, due, evaluate_views, loss_line, noise_dict, open_run, run_cli,
                  set_seed, slice_for_rank, write_checkpoint, write_experiment_config)


def generate_experiment_name(scene: str, noise_config: Optional[NoiseConfig], base_name: str = "") -> str:
    """Reference train.py:44-66: ``{scene}[_{base}]_{noise|clean}_{timestamp}``."""
    ts = datetime.now().strftime("%Y%m%d_%H%M%S")
    noise_desc = str(noise_config) if noise_config is not None and noise_config.has_noise else "clean"
    return f"{scene}_{base_name}_{noise_desc}_{ts}" if base_name else f"{scene}_{noise_desc}_{ts}"


def train_step(renderer: NeRFRenderer, optimizer: torch.optim.Optimizer, batch: Dict[str, torch.Tensor],
               t_rand: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """Reference train.py:68-119 (``t_rand``/``u`` optionally inject the random draws)."""
    from .rendering import render_rays

    optimizer.zero_grad()
    out = render_rays(renderer.model_coarse, renderer.model_fine, batch["rays_o"], batch["rays_d"], renderer.config,
                      is_train=True, t_rand=t_rand, u=u)
    target = batch["target_rgb"]
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
    metrics["loss"] = loss.item()
    loss.backward()
    params = list(renderer.parameters())
    if isinstance(optimizer, FusedAdam):
        optimizer.step(clip_groups=[(params, 1.0)])
    else:
        clip_grad_norm_(params, 1.0)
        optimizer.step()
    return metrics


@torch.no_grad()
def render_image(renderer: NeRFRenderer, pose: torch.Tensor, H: int, W: int, focal: float,
                 chunk_size: int = 1024 * 4, fxy=None) -> Dict[str, torch.Tensor]:
    """Reference train.py:122-160: every pixel of one view, deterministic (is_train=False).
    ``fxy`` (optional): focal lengths (fx, fy) learned with the poses, in place of ``focal``;
    or six numbers, a learned lens (fx, fy, cx, cy, k1, k2) (``ops.ray_directions_lens``)."""
    if fxy is None:
        dirs = get_ray_directions(H, W, focal, device=pose.device)
    elif len(fxy) == 2:
        dirs = ops.ray_directions_xy(H, W, fxy[0], fxy[1], W / 2.0, H / 2.0, pose.device)
    elif len(fxy) == 6:
        dirs = ops.ray_directions_lens(H, W, *fxy, pose.device)
    else:
        raise ValueError(f"render_image: fxy must be (fx, fy) or (fx, fy, cx, cy, k1, k2), got {fxy!r}")
    rays_o, rays_d = get_rays(dirs, pose.detach().contiguous())
    out = renderer(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), chunk_size=chunk_size, is_train=False)
    key = "fine" if "rgb_fine" in out else "coarse"
    return {"rgb": out[f"rgb_{key}"].reshape(H, W, 3), "depth": out[f"depth_{key}"].reshape(H, W),
            "acc": out[f"acc_{key}"].reshape(H, W)}


@torch.no_grad()
def evaluate(renderer: NeRFRenderer, val_data: BlenderData, logger: Optional[ExperimentLogger] = None,
             iteration: int = 0, num_images: int = 5, lpips_metric: Optional[LPIPSMetric] = None,
             chunk_size: int = 1024 * 4) -> ValidationMetrics:
    """Reference train.py:163-233: mean PSNR / SSIM / MSE (+ LPIPS when available) over
    the first ``num_images`` validation views; PNGs of the first three when a logger is
    given."""
    n = min(num_images, val_data.images.shape[0])
    return evaluate_views(
        lambda i: render_image(renderer, val_data.poses[i], val_data.H, val_data.W, val_data.focal, chunk_size),
        ((f"val_{i}", i, val_data.images[i]) for i in range(n)), logger, iteration, lpips_metric)


def save_checkpoint(output_dir, iteration: int, model_coarse, model_fine, optimizer: torch.optim.Optimizer,
                    config: NeRFConfig, noise_config=None, metrics: Optional[Dict] = None,
                    is_best: bool = False) -> None:
    """Reference train.py:236-286: same keys (iteration, model_coarse/_fine state_dicts in
    nn.Linear naming, optimizer state, config as plain dicts), same file names."""
    ckpt = base_checkpoint(iteration, model_coarse, model_fine, config, noise_config, metrics)
    ckpt["optimizer"] = optimizer.state_dict()
    write_checkpoint(output_dir, iteration, ckpt, is_best)


def load_checkpoint(checkpoint_path, model_coarse, model_fine, optimizer: Optional[torch.optim.Optimizer] = None) -> int:
    """Reference train.py:289-304 -> iteration (``weights_only=True``)."""
    ckpt = torch.load(checkpoint_path, map_location=next(model_coarse.parameters()).device, weights_only=True)
    model_coarse.load_state_dict(ckpt["model_coarse"])
    if model_fine is not None and "model_fine" in ckpt:
        model_fine.load_state_dict(ckpt["model_fine"])
    if optimizer is not None and "optimizer" in ckpt:
        optimizer.load_state_dict(ckpt["optimizer"])
    return ckpt.get("iteration", 0)


def train(config: NeRFConfig, noise_config: Optional[NoiseConfig] = None, *,
          train_data: Optional[BlenderData] = None, val_data: Optional[BlenderData] = None,
          process_group=None, log=print, graph: bool = False,
          distortion_weight: float = 0.0, loss: str = "mse", loss_scale: float = 0.1) -> Dict[str, object]:
    """Reference train.py:307-577.  ``train_data`` / ``val_data`` (optional) replace the
    on-disk scene; ``process_group`` (or a torchrun environment, see ``main``) makes it
    data parallel.  ``graph`` replays the training step from a hipGraph after the first
    iteration (``engine.GraphedTrainer``; same results as eager); with data parallelism
    the RCCL all-reduces are captured into it too (``nccl`` backend only).
    ``distortion_weight`` > 0 adds that multiple of the distortion loss on the rendering
    network's ray weights (``engine.Trainer``); it is logged on the console line only.
    ``loss`` / ``loss_scale`` (``--loss``, ``--loss_scale``): the photometric loss of both
    networks and its scale (``engine.Trainer``).  With a robust kind the CSV's loss columns
    are what is minimised, its ``psnr`` column stays the plain MSE's and the console line
    names the kind.
    Returns the networks, the output directory and the final metrics."""
    import torch.distributed as dist

    exp_name = config.train.experiment_name
    if exp_name in ("auto", ""):
        exp_name = generate_experiment_name(config.data.scene_name, noise_config)
    rank, world, device, output_dir, logger, lpips_metric = open_run(config, exp_name, process_group, graph, "train",
                                                                     train_data, val_data)
    if train_data is None:
        sampler, train_data, val_data = create_data_loaders(config.data, device=device, noise_config=noise_config)
    else:
        sampler = RaySampler(RayDataset(train_data, config.data.batch_size, noise_config=noise_config),
                             config.data.batch_size, shuffle=config.data.shuffle)
    model_coarse, model_fine = create_nerf_for(config, device, logger)
    renderer = NeRFRenderer(model_coarse, model_fine, config.render)
    # coarse_stream="auto": the coarse chain becomes a second graph branch only in a
    # --graph replay of <= 1024 rays (engine.Trainer), where it pays
    trainer = Trainer(model_coarse, model_fine, config.render, lr=config.train.lr, lr_decay=config.train.lr_decay,
                      process_group=process_group, coarse_stream="auto", distortion_weight=distortion_weight,
                      loss=loss, loss_scale=loss_scale)
    optimizer = trainer.optimizer
    if rank == 0:
        write_experiment_config(output_dir, config, exp_name, world, noise_config, NO_NOISE,
                                after_batch={"img_scale": config.data.img_scale},
                                extra={"distortion_weight": distortion_weight, "loss": loss,
                                       "loss_scale": loss_scale})
        log(f"NeRF training: {exp_name} -> {output_dir} ({world} rank(s), {sampler.n_rays:,} rays, "
            f"{train_data.H}x{train_data.W}, focal {train_data.focal:.2f})")

    def line(vm, lr, rays_per_sec, meta):
        dist_part = f"distortion: {vm['loss_distortion']:.5f} | " if "loss_distortion" in vm else ""
        return f"{loss_line(loss, loss_scale)}{dist_part}lr: {lr:.2e} | rays/s: {rays_per_sec:.0f}"

    B = config.data.batch_size
    best_psnr = 0.0
    iteration = 0
    graphed = None
    ilog = IterationLog(logger, config, process_group, line, log)
    while iteration < config.train.num_iterations:
        for batch in sampler:
            if iteration >= config.train.num_iterations:
                break
            n = batch["rays_o"].shape[0]
            if world > 1 and n % world:
                # only an epoch's short final batch (batch_size % world == 0 is checked
                # up front): it cannot be split evenly over the ranks, so it is skipped
                continue
            t_rand, u = draw_randoms(n, config.render, model_fine is not None, device)
            _, args = slice_for_rank(n, rank, world, batch["rays_o"], batch["rays_d"], batch["target_rgb"], t_rand, u)
            if graph and graphed is None and iteration >= 1 and n == B:
                # captured after one eager step (state exists), on a full batch: an epoch's
                # short tail batch would leave every full batch after it eager
                graphed = GraphedTrainer(trainer, *args, warmup=0)
            if graphed is not None and args[0].shape == graphed.static[0].shape:
                m = graphed.step(*args)
            else:  # eager (also an epoch's short final batch in graph mode)
                m = trainer.step(*args)
            ilog.push(iteration, m, optimizer.param_groups[0]["lr"])
            what = due(iteration, config.train.val_every, config.train.save_every) if logger is not None else None
            if what:
                ilog.flush()
                if what == "val":
                    vmx = evaluate(renderer, val_data, logger, iteration, num_images=5, lpips_metric=lpips_metric)
                    logger.log_validation(vmx)
                    is_best = vmx.psnr > best_psnr
                    best_psnr = max(best_psnr, vmx.psnr)
                    log(f"  validation @ {iteration}: PSNR {vmx.psnr:.2f} dB, SSIM {vmx.ssim:.4f}"
                        + (" (best)" if is_best else ""))
                    save_checkpoint(output_dir, iteration, model_coarse, model_fine, optimizer, config, noise_config,
                                    metrics={"psnr": vmx.psnr, "ssim": vmx.ssim}, is_best=is_best)
                else:
                    save_checkpoint(output_dir, iteration, model_coarse, model_fine, optimizer, config, noise_config)
                ilog.pause()
            iteration += 1
    ilog.flush()
    result = {"model_coarse": model_coarse, "model_fine": model_fine, "output_dir": output_dir,
              "best_psnr": best_psnr}
    if logger is not None:
        save_checkpoint(output_dir, iteration, model_coarse, model_fine, optimizer, config, noise_config)
        final = evaluate(renderer, val_data, logger, iteration, num_images=val_data.images.shape[0],
                         lpips_metric=lpips_metric)
        logger.log_validation(final)
        logger.save_summary()
        logger.close()
        log(f"final: PSNR {final.psnr:.2f} dB, SSIM {final.ssim:.4f}; {ilog.minutes():.1f} min; "
            f"results in {output_dir}")
        result["val"] = final
    if process_group is not None:
        dist.barrier(process_group)
    return result


def build_arg_parser():
    """Reference train.py:580-657 flags (same names and defaults) plus ``--precision``, ``--graph`` and
    ``--distortion_weight``."""
    import argparse
    ap = argparse.ArgumentParser(description="Train NeRF with optional pose noise (MI355X HIP path)")
    add_common_args(ap, "scene data_root img_scale batch_size num_iters lr no_hierarchical num_samples num_samples_fine "
                        "rotation_noise translation_noise translation_noise_pct noise_seed log_every val_every "
                        "save_every output_dir", num_iters=dict(default=200000), val_every=dict(default=5000),
                    batch_size=dict(help="global batch (rays) over all ranks"))
    ap.add_argument("--exp_name", type=str, default="auto")
    add_common_args(ap, "device seed precision")
    ap.add_argument("--graph", action="store_true",
                    help="replay the training step from a hipGraph (same results as eager; with RCCL data "
                         "parallelism the all-reduces are captured too)")
    add_common_args(ap, "distortion_weight")
    return ap


def build_cli_parser():
    """The command line's parser: ``build_arg_parser()`` (the reference's flags and this
    project's earlier ones, in the order its callers rely on) plus the photometric loss
    flags ``--loss`` and ``--loss_scale``."""
    ap = build_arg_parser()
    add_common_args(ap, "loss loss_scale")
    return ap


def main(argv=None) -> None:
    """``python -m noisy_src.train`` (or under ``torchrun`` for data parallelism)."""
    a = build_cli_parser().parse_args(argv)

    def run_name(noise_config, world):  # a single process leaves "auto" to train()
        auto = world > 1 and a.exp_name in ("auto", "")
        return generate_experiment_name(a.scene, noise_config) if auto else a.exp_name

    def call(cfg, noise_config, pg, name):
        cfg.train.experiment_name = name
        train(cfg, noise_config, process_group=pg, graph=a.graph, distortion_weight=a.distortion_weight, loss=a.loss,
              loss_scale=a.loss_scale)

    run_cli(a, run_name, call)


__all__ = ["set_seed", "generate_experiment_name", "train_step", "render_image", "evaluate", "save_checkpoint",
           "load_checkpoint", "train", "main"]

if __name__ == "__main__":
    main()
