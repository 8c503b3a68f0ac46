"""
The training step of the hot path, without host synchronisation.

Mirrors ``train_step`` of the reference (noisy_src/train.py:68-119) plus the
``scheduler.step()`` of its loop (train.py:461): render coarse+fine, MSE losses,
backward through the HIP kernels, joint gradient clip at 1.0 fused into Adam,
LambdaLR 0.1^(step/(lr_decay*1000)).  Losses stay on the device; callers that
log them call ``.item()`` themselves (the reference syncs four times a step).
For data parallelism each network's flat gradient is all-reduced (RCCL) as soon
as its backward has produced it (the fine net's overlaps the coarse backward),
and the optimizer step waits for both.  The hipGraph replays of these
steps live in ``graphed`` (GraphedTrainer, GraphedPoseTrainer; re-exported here).
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops
from .graphed import GraphedPoseTrainer, GraphedTrainer  # noqa: F401  (the public names of this module)
from .optim import FusedAdam
from .rendering import render_rays


def init_distributed(device: str = "cuda"):
    """One process per GPU under ``torch.distributed.run``: reads RANK / LOCAL_RANK /
    WORLD_SIZE, binds the local GPU and joins the default group (backend "nccl" = RCCL
    on ROCm; "gloo" for CPU-device runs).  Returns (process_group or None, rank, world,
    device string).  Without the torchrun environment it is a single process."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if device.startswith("cuda") and torch.cuda.is_available():
        # one GPU per rank; ranks beyond the visible GPUs share them (gloo test mode)
        local = local % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        device = f"cuda:{local}"
    if world <= 1:
        return None, 0, 1, device
    import torch.distributed as dist
    if not dist.is_initialized():
        if device.startswith("cuda") and os.environ.get("NR_DIST_BACKEND", "nccl") == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(device))
        else:
            dist.init_process_group("gloo")
    return dist.group.WORLD, rank, world, device


def rank_slice(n_global: int, rank: int, world: int) -> slice:
    """Rank r's contiguous share [r*B/N, (r+1)*B/N) of a global batch."""
    if n_global % world:
        raise ValueError(f"global batch {n_global} is not divisible by world size {world}")
    per = n_global // world
    return slice(rank * per, (rank + 1) * per)


def check_run_args(config, world: int, train_data, val_data) -> None:
    """Fail before any work for arguments the loops cannot honour: a global batch the
    ranks cannot split evenly (every batch would be skipped), or only one of
    train_data / val_data (the loops validate on val_data and train on train_data)."""
    if world > 1 and config.data.batch_size % world:
        raise ValueError(f"batch_size {config.data.batch_size} is not divisible by the {world} data-parallel ranks")
    if (train_data is None) != (val_data is None):
        raise ValueError("train_data and val_data must be given together (or neither: load the scene from disk)")


def mean_over_ranks(values, process_group=None):
    """Average a list of device scalars over the group (the logged global-batch losses)."""
    t = torch.stack([v.detach().float().reshape(()) for v in values])
    if process_group is not None:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
        t = t / dist.get_world_size(process_group)
    return t


class LaggedScalars:
    """Logged device scalars read back one iteration late.  ``push`` queues a pinned copy
    of this iteration's values and returns the previous iteration's (synchronising on its
    event only), so the host queues step i+1 while step i still runs instead of idling on
    a per-step ``.item()``/``.tolist()`` as the reference's loops do (train.py:386-420).
    ``flush`` returns the pending values now (before a validation / checkpoint)."""

    def __init__(self, n_max: int = 8):
        self._buf = [torch.zeros(n_max, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        self._k = 0
        self._pending = None

    def push(self, values: torch.Tensor, meta=None):
        n = values.numel()
        host = self._buf[self._k % 2]  # the slot's previous values were resolved by the last push
        self._k += 1
        host[:n].copy_(values.reshape(-1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        prev, self._pending = self._pending, (host, n, ev, meta)
        return self._resolve(prev)

    def flush(self):
        prev, self._pending = self._pending, None
        return self._resolve(prev)

    @staticmethod
    def _resolve(p):
        if p is None:
            return None
        host, n, ev, meta = p
        ev.synchronize()
        return host[:n].tolist(), meta


def lr_lambda_factory(lr_decay: int):
    decay_steps = lr_decay * 1000

    def lr_lambda(step):
        return 0.1 ** (step / decay_steps)

    return lr_lambda


class GradAllReducer:
    """Bucketed data-parallel gradient averaging: one async all-reduce (SUM) per flat
    gradient buffer, launched when the buffer is ready; ``finish`` waits.  With
    ``average`` it then divides by the world size; the trainers instead pre-scale the
    backward seed by 1/world (``prescale``), so the SUM already is the mean and no
    multiply kernel runs per buffer.  Backend-agnostic (RCCL on the GPU box, gloo in
    the CPU tests)."""

    def __init__(self, process_group=None, average: bool = True):
        import torch.distributed as dist
        self.dist = dist
        self.group = process_group
        self.world = dist.get_world_size(process_group)
        self.average = average
        self.pending = []
        # timing (bench.py): per eager step, HIP events on the compute stream at the first
        # launch, before ``finish`` waits and after it: (launch -> done) is the collective's
        # span beside the rest of the backward, (wait -> done) what the step is exposed to
        self.timing = None
        self._t_launch = None

    @property
    def prescale(self) -> float:
        """The factor the backward seed carries when ``average`` is off."""
        return 1.0 if self.average else 1.0 / self.world

    def launch(self, flat: torch.Tensor) -> None:
        if flat.is_cuda and torch.cuda.is_current_stream_capturing():
            # inside a hipGraph capture (GraphedTrainer): the stream-ordered form, captured
            # as the collective's kernel plus the stream dependencies around it
            self.dist.all_reduce(flat, op=self.dist.ReduceOp.SUM, group=self.group)
            self.pending.append((None, flat))
            return
        if self.timing is not None and flat.is_cuda and not self.pending:
            self._t_launch = torch.cuda.Event(enable_timing=True)
            self._t_launch.record()
        work = self.dist.all_reduce(flat, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
        self.pending.append((work, flat))

    def finish(self) -> None:
        timed = self.timing is not None and self._t_launch is not None
        if timed:
            t_wait = torch.cuda.Event(enable_timing=True)
            t_wait.record()
        for work, flat in self.pending:
            if work is not None:
                work.wait()
            if self.average and self.world > 1:
                flat.mul_(1.0 / self.world)
        if timed:
            t_done = torch.cuda.Event(enable_timing=True)
            t_done.record()
            self.timing.append((self._t_launch, t_wait, t_done))
        self._t_launch = None
        self.pending.clear()

    def timing_summary(self) -> Optional[Dict[str, float]]:
        """Means over the recorded steps (ms): ``span`` = first launch -> all reduced,
        ``exposed`` = the compute stream's wait in ``finish``; None without records."""
        if not self.timing:
            return None
        torch.cuda.synchronize()
        span = [a.elapsed_time(c) for a, _, c in self.timing]
        exposed = [b.elapsed_time(c) for _, b, c in self.timing]
        return {"steps": len(span), "span_ms": sum(span) / len(span), "exposed_ms": sum(exposed) / len(exposed)}


def _hooked_reducer(process_group, nets) -> Optional[GradAllReducer]:
    """The trainers' reducer (None for a single process): each network's backward hands
    it the flat gradient as soon as it exists (``_grad_ready_hook``)."""
    if process_group is None:
        return None
    reducer = GradAllReducer(process_group, average=False)
    for net in nets:
        if net is not None:
            net._grad_ready_hook = reducer.launch
    return reducer


def _finish_and_adopt(reducer: GradAllReducer, nets, flats) -> None:
    """Wait for the pending all-reduces; ``flats``: the networks' flat gradients among them."""
    reducer.finish()
    for net in nets:
        if net is not None:
            _adopt_reduced_grad(net, flats)


def _check_distortion_weight(w) -> float:
    w = float(w)
    if not w >= 0.0:
        raise ValueError(f"distortion_weight must be >= 0, not {w}")
    return w


def _check_photometric(kind, c):
    """(kind, c) of the photometric loss: a name of ops.LOSS_KINDS and its scale in colour
    units, finite and > 0 (checked under "mse" too, which does not use it)."""
    if kind not in ops.LOSS_KINDS:
        raise ValueError(f"loss must be one of {', '.join(ops.LOSS_KINDS)}, not {kind!r}")
    c = float(c)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"loss_scale must be finite and > 0, not {c}")
    return kind, c


def _distortion_term(aux, render_config, weight: float, prescale: float):
    """The distortion loss (ops.distortion_loss) on the RENDERING network's weights, from
    ``render_rays(..., return_aux=True)``'s second result: the fine pair, or the coarse one
    when no fine network renders.  The coarse network of a coarse+fine pair is left alone:
    it is a proposal and has to spread.  The gradient carries ``weight * prescale`` already,
    so the term joins the backward sum unweighted; the logged loss adds ``weight`` times it."""
    which = "fine" if "weights_fine" in aux else "coarse"
    return ops.distortion_loss(aux["weights_" + which], aux["z_" + which], render_config.near, render_config.far,
                               grad_scale=weight * prescale)


def _step_losses(out, aux=None, render_config=None, weight: float = 0.0, prescale: float = 1.0):
    """(backward sum, logged loss, metrics) of ``render_rays``' output and aux: the sum is
    loss_coarse [+ loss_fine], plus with ``weight`` > 0 the distortion term, which the
    logged loss counts ``weight`` times and ``metrics["loss_distortion"]`` holds unweighted."""
    bwd = loss = out["loss_coarse"]
    metrics = {"loss_coarse": loss.detach()}  # metrics hold no autograd graph
    if "loss_fine" in out:
        bwd = loss = loss + out["loss_fine"]
        metrics["loss_fine"] = out["loss_fine"].detach()
    for k in ("mse_coarse", "mse_fine"):  # a robust photometric loss: the plain MSE beside it
        if k in out:
            metrics[k] = out[k]
    if weight > 0:
        dist = _distortion_term(aux, render_config, weight, prescale)
        metrics["loss_distortion"] = dist.detach()
        loss = loss.detach() + weight * dist.detach()
        bwd = bwd + dist
    return bwd, loss, metrics


class Trainer:
    """One reference training iteration (train.py:68-119) on the HIP kernels.
    ``coarse_stream``: run the coarse network's forward, compositing, loss and backward on
    a second stream; the coarse backward starts as soon as the coarse forward ends and
    runs beside the fine sampling, forward and backward (the fine samples depend on the
    coarse weights only through detached z values, rays.py:325, so d(loss_c + loss_f)
    reaches the coarse net as d loss_c alone).  Bit-identical to the one-stream step.  It
    pays where one chain does not fill the GPU and the host is out of the way: inside a
    GraphedTrainer capture (the two chains become two branches of the graph) at up to
    ``AUTO_COARSE_STREAM_RAYS`` rays per step (BASELINE cfg #4's 512 rays per rank: 0.856
    -> 0.802 ms per replay; 1024 rays 1.36 -> 1.34 ms; 2048 and 4096 rays no gain or a
    loss; eager steps lose to the second stream's host cost, profiles/r05_coarse_early_ab.txt).
    ``coarse_stream="auto"`` applies exactly that rule per step; True / False force it.
    ``distortion_weight`` > 0 adds that multiple of the distortion loss of the rendering
    network's weights (``_distortion_term``) to the loss; ``metrics["loss_distortion"]`` is
    its unweighted mean.  At 0 the step launches nothing for it.
    ``loss`` / ``loss_scale``: the photometric loss of both networks, a name of
    ``ops.LOSS_KINDS`` and its scale c in colour units (include/nerf_hip.h).  With a kind
    other than "mse" the ``loss*`` metrics are the robust terms that are minimised and
    ``mse_coarse`` / ``mse_fine`` hold the plain mean squared errors."""

    AUTO_COARSE_STREAM_RAYS = 1024

    def __init__(self, model_coarse, model_fine, render_config, lr: float = 5e-4, lr_decay: int = 250,
                 max_norm: float = 1.0, process_group=None, coarse_stream=False, distortion_weight: float = 0.0,
                 loss: str = "mse", loss_scale: float = 0.1):
        self.distortion_weight = _check_distortion_weight(distortion_weight)
        self.photometric = _check_photometric(loss, loss_scale)
        if coarse_stream not in (True, False, "auto"):
            raise ValueError(f"coarse_stream must be True, False or 'auto', not {coarse_stream!r}")
        self.coarse_stream = coarse_stream if coarse_stream == "auto" else bool(coarse_stream)
        self._cstream = None
        self.last_step_coarse_stream = False  # whether the last step (or capture) used it
        self.model_coarse = model_coarse
        self.model_fine = model_fine
        self.render_config = render_config
        params = list(model_coarse.parameters())
        if model_fine is not None:
            params += list(model_fine.parameters())
        self.params = params
        self.max_norm = max_norm
        self.optimizer = FusedAdam(params, lr=lr)
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lr_lambda_factory(lr_decay))
        self.process_group = process_group
        self.reducer = _hooked_reducer(process_group, (model_coarse, model_fine))

    def step(self, rays_o: torch.Tensor, rays_d: torch.Tensor, target_rgb: torch.Tensor,
             t_rand: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        self.optimizer.zero_grad(set_to_none=True)
        cs = None
        if (self.coarse_stream is not False and self.model_fine is not None and rays_o.is_cuda
                and self.render_config.use_hierarchical):
            # created on the first eager step (a GraphedTrainer warms up eagerly), not
            # inside a capture
            if self._cstream is None or self._cstream.device != rays_o.device:
                self._cstream = torch.cuda.Stream(device=rays_o.device)
            if self.coarse_stream is True or (rays_o.shape[0] <= self.AUTO_COARSE_STREAM_RAYS
                                              and torch.cuda.is_current_stream_capturing()):
                cs = self._cstream
        self.last_step_coarse_stream = cs is not None
        gs = self.reducer.prescale if self.reducer is not None else 1.0  # DP: 1/world in the seed
        early = {}

        def coarse_backward(out_c):
            # on the coarse stream: the coarse loss's backward, beside the fine forward
            # (loss = loss_c + loss_f sends exactly d loss_c to the coarse net)
            early["loss_c"] = out_c["loss"]
            if "mse" in out_c:
                early["mse_c"] = out_c["mse"]
            early["loss_c"].backward(ops.unit_grad(rays_o.device))

        # the MSE losses (train.py:89/98) come out of the compositing (ops.composite_mse)
        dw = self.distortion_weight
        out, aux = render_rays(self.model_coarse, self.model_fine, rays_o, rays_d, self.render_config, is_train=True,
                               t_rand=t_rand, u=u, return_aux=True, coarse_stream=cs,
                               coarse_backward=coarse_backward if cs is not None else None,
                               target_rgb=target_rgb, loss_scale=gs, photometric=self.photometric)
        if cs is not None:
            main = torch.cuda.current_stream(rays_o.device)
            loss_f = out["loss_fine"]
            loss_c = early["loss_c"].detach()
            lf = loss_f.detach()
            term = None
            if dw > 0:  # the fine chain's: on the main stream, before its backward
                dist = _distortion_term(aux, self.render_config, dw, gs)
                loss_f = loss_f + dist
                term = dw * dist.detach()
            fine_done = main.record_event()
            loss_f.backward(ops.unit_grad(rays_o.device))
            # the summed value on the coarse stream, beside the fine backward (the backward
            # already ran for loss_c; d(loss_c + loss_f) = d loss_f for the fine net).
            # Captured after the fine backward, so that a graph replay keeps the fine
            # chain on one hardware queue (a hop between queues costs ~10 us)
            cs.wait_event(fine_done)
            lf.record_stream(cs)
            with torch.cuda.stream(cs):
                loss = loss_c + lf
                if term is not None:  # the one-stream step's association: (loss_c + loss_f) + the term
                    term.record_stream(cs)
                    loss = loss + term
            loss.record_stream(main)
            main.wait_stream(cs)  # join the coarse chain
            metrics = {"loss_coarse": loss_c, "loss_fine": lf}
            if "mse_c" in early:
                metrics["mse_coarse"], metrics["mse_fine"] = early["mse_c"], out["mse_fine"]
            if dw > 0:
                metrics["loss_distortion"] = dist.detach()
        else:
            bwd, loss, metrics = _step_losses(out, aux, self.render_config, dw, gs)
            bwd.backward(ops.unit_grad(loss.device))
        if self.reducer is not None:
            _finish_and_adopt(self.reducer, (self.model_coarse, self.model_fine),
                              [flat for _, flat in self.reducer.pending])
        self.optimizer.step(clip_groups=[(self.params, self.max_norm)])
        self.scheduler.step()
        metrics["loss"] = loss.detach()
        metrics["rgb_fine"] = out.get("rgb_fine", out["rgb_coarse"]).detach()
        return metrics


class PoseTrainer:
    """The joint pose-optimisation step without host synchronisation (BASELINE cfg #3).

    Mirrors ``train_step_with_poses`` of the reference (noisy_src/train_pose_opt.py:290-411)
    plus the two ``scheduler.step()`` of its loop (:876-880): all poses from the SE(3)
    kernel, the batch's rays from (image, pixel) and those poses, render coarse+fine, MSE
    losses plus the pose regulariser (0.01 mean w^2 + 0.001 mean dt^2, :377-389, weights
    :621-622), backward, separate clips (coarse 1.0, fine 1.0, poses 0.1, :398-404) fused
    into the Adams, the pose Adam and its LambdaLR only once ``optimize_poses``.  The
    reference's ``.item()`` metrics are left to the caller (losses stay on the device).
    Data parallel: the network gradients all-reduce as in ``Trainer``; the pose gradient
    (each rank touches its own images) is one more all-reduce of 2 x 3 x n_poses floats.
    Every gradient is AVERAGED over the ranks: each rank's loss is the mean over its
    equal share of the global batch plus the replicated pose regulariser, so the mean
    of the rank gradients is the single-process gradient.  The 1/world
    rides in the backward seed (the MSE kernels' gradient scale and the regulariser's
    factor), so the all-reduced SUM is that mean without a multiply per buffer.
    Before the pose-optimisation delay (``optimize_poses=False``) the poses enter the
    step detached: the reference lets their gradient accumulate unused until the first
    optimising step's ``zero_grad``, so skipping it changes
    nothing and saves the MLP's input-gradient pass.

    ``pe_schedule`` (optional) makes the positional encoding coarse-to-fine (BARF): a
    callable ``(iteration, num_freqs) -> num_freqs weights``; a ``step`` that is given
    its ``iteration`` sets both networks' windows from it first (``NeRF.set_pe_window``,
    the position and the direction encoder each with its own frequency count).

    ``intrinsics`` (optional, ``train_pose_opt.CameraIntrinsics``) learns the focal length
    with the poses (NeRF--, Wang et al. 2021): the rays come from its ``fxy()`` tensor, read
    by the ray kernels from device memory, and its ``log_scale`` joins the pose Adam as a
    clip group of its own (0.1), with the pose learning rate, LambdaLR and delay; its
    gradient is appended to the pose-gradient all-reduce.  At ``log_scale = 0`` the rays,
    and with them the networks' and poses' updates, are those without it, bit for bit.
    With a lens (``intrinsics.has_lens``: principal point, radial distortion) the rays come
    from its ``lens()`` tensor instead, and EACH of its parameters is a clip group of its own
    (0.1), so that switching one option on does not change another parameter's clip factor;
    all share the pose learning rate, LambdaLR, delay and all-reduce buffer.  At a neutral
    lens (centred, k = 0) the first step is again the plain one, bit for bit.

    ``distortion_weight``: as in ``Trainer``; the term's gradient reaches the poses through the
    rendering network like the photometric one.  ``loss`` / ``loss_scale``: as in ``Trainer``."""

    def __init__(self, model_coarse, model_fine, camera_params, pixel_sampler, render_config,
                 lr: float = 5e-4, pose_lr: float = 1e-4, lr_decay: int = 250,
                 rotation_reg_weight: float = 0.01, translation_reg_weight: float = 0.001, process_group=None,
                 pe_schedule=None, intrinsics=None, distortion_weight: float = 0.0, loss: str = "mse",
                 loss_scale: float = 0.1):
        self.distortion_weight = _check_distortion_weight(distortion_weight)
        self.photometric = _check_photometric(loss, loss_scale)
        self.pe_schedule = pe_schedule
        self.model_coarse, self.model_fine = model_coarse, model_fine
        self.camera_params, self.pixel_sampler, self.render_config = camera_params, pixel_sampler, render_config
        self.intrinsics = intrinsics
        self.coarse = list(model_coarse.parameters())
        self.fine = list(model_fine.parameters()) if model_fine is not None else []
        self.poses = list(camera_params.parameters())
        self.focal = list(intrinsics.parameters()) if intrinsics is not None else []
        self.rot_w, self.trans_w = rotation_reg_weight, translation_reg_weight
        self.optimizer_nerf = FusedAdam(self.coarse + self.fine, lr=lr)
        # the focal length rides with the poses: same Adam, learning rate, schedule and delay
        # (its own clip group); with no learnable pose it has the optimizer to itself
        self.optimizer_poses = FusedAdam(self.poses + self.focal, lr=pose_lr) if self.poses + self.focal else None
        lam = lr_lambda_factory(lr_decay)
        self.scheduler_nerf = torch.optim.lr_scheduler.LambdaLR(self.optimizer_nerf, lam)
        self.scheduler_poses = (torch.optim.lr_scheduler.LambdaLR(self.optimizer_poses, lam)
                                if self.optimizer_poses is not None else None)
        self.reducer = _hooked_reducer(process_group, (model_coarse, model_fine))

    def set_pe_windows(self, iteration: int) -> None:
        """Both networks' windows of ``iteration`` under ``pe_schedule`` (no-op without one)."""
        if self.pe_schedule is None:
            return
        for net in (self.model_coarse, self.model_fine):
            if net is not None:
                mc = net.config
                net.set_pe_window(self.pe_schedule(iteration, mc.pos_freqs),
                                  self.pe_schedule(iteration, mc.dir_freqs) if mc.use_view_dirs else None)

    def step(self, pixel_batch, optimize_poses: bool = True, t_rand: Optional[torch.Tensor] = None,
             u: Optional[torch.Tensor] = None, iteration: Optional[int] = None) -> Dict[str, torch.Tensor]:
        cam = self.camera_params
        if iteration is not None:
            self.set_pe_windows(iteration)
        optimize_poses = optimize_poses and self.optimizer_poses is not None
        self.optimizer_nerf.zero_grad(set_to_none=True)
        if optimize_poses:
            self.optimizer_poses.zero_grad(set_to_none=True)
        poses = cam.get_all_poses()
        if not optimize_poses:
            poses = poses.detach()
        if self.intrinsics is None:
            rays_o, rays_d = self.pixel_sampler.get_rays_for_batch(pixel_batch, poses)
        else:
            # (fx, fy), or the six-number lens, as a device tensor the ray kernels read; detached
            # before the delay, like the poses
            fxy = self.intrinsics.lens() if getattr(self.intrinsics, "has_lens", False) else self.intrinsics.fxy()
            rays_o, rays_d = self.pixel_sampler.get_rays_for_batch(pixel_batch, poses,
                                                                   fxy if optimize_poses else fxy.detach())
        target = pixel_batch.target_rgb
        gs = self.reducer.prescale if self.reducer is not None else 1.0  # DP: 1/world in the seed
        # the MSE losses (train_pose_opt.py:355-370) come out of the compositing
        dw = self.distortion_weight
        out, aux = render_rays(self.model_coarse, self.model_fine, rays_o, rays_d, self.render_config, is_train=True,
                               t_rand=t_rand, u=u, return_aux=True, target_rgb=target, loss_scale=gs,
                               photometric=self.photometric)
        bwd, loss, metrics = _step_losses(out, aux, self.render_config, dw, gs)
        if optimize_poses:
            # the regulariser is replicated on every rank: its gradient carries the seed's
            # 1/world too, so the SUM over the ranks counts it once
            reg = []
            if self.rot_w > 0 and cam.learn_rotation:
                reg.append(self.rot_w * torch.mean(cam.rotation_deltas ** 2))
            if self.trans_w > 0 and cam.learn_translation:
                reg.append(self.trans_w * torch.mean(cam.translation_deltas ** 2))
            for r in reg:
                loss = loss + r
                bwd = bwd + (r * gs if gs != 1.0 else r)
        bwd.backward(ops.unit_grad(loss.device))
        if self.reducer is not None:
            flats = [flat for _, flat in self.reducer.pending]
            # the focal gradient rides at the end of the pose-gradient buffer: no collective of its own
            pg = [p.grad for p in self.poses + self.focal if p.grad is not None] if optimize_poses else []
            pflat = torch.cat([g.reshape(-1) for g in pg]) if pg else None
            if pflat is not None:
                self.reducer.launch(pflat)
            _finish_and_adopt(self.reducer, (self.model_coarse, self.model_fine), flats)
            off = 0
            for g in pg:
                g.copy_(pflat[off:off + g.numel()].view(g.shape))
                off += g.numel()
        groups = [(self.coarse, 1.0)] + ([(self.fine, 1.0)] if self.fine else [])
        self.optimizer_nerf.step(clip_groups=groups)
        self.scheduler_nerf.step()
        if optimize_poses:
            groups = [(self.poses, 0.1)] + [([p], 0.1) for p in self.focal]  # one group per camera parameter
            self.optimizer_poses.step(clip_groups=groups)
            self.scheduler_poses.step()
        metrics["loss"] = loss.detach()
        metrics["rgb_fine"] = out.get("rgb_fine", out["rgb_coarse"]).detach()
        return metrics


class PoseRefiner:
    """Photometric pose refinement against a FROZEN field: the pose half of
    ``PoseTrainer.step`` and nothing else (BARF's test-time protocol).  Poses from the
    SE(3) kernel, the batch's rays from them, render coarse+fine with the MSE losses
    (``loss_coarse + loss_fine``), backward, one fused pose Adam with the 0.1 clip.  No
    regulariser, no network optimizer, no host synchronisation (losses stay on the device).

    Both networks' parameters are set to ``requires_grad_(False)`` for the refiner's
    lifetime, so the fused MLP takes its input-gradient-only path (masks-only forward,
    no dW); ``close()`` or leaving the ``with`` block restores them.  ``camera_params``
    must use the small-angle Jacobian (``fixed_small_angle=True``): refinement starts at
    w = 0, where the reference's ``theta < 1e-6`` rule gives a rotation gradient of
    exactly zero.  ``lr_decay`` (optional): the LambdaLR of the training loops.
    ``fxy`` (optional, (2,) or (6,) fp32 device tensor): fixed focal lengths (fx, fy) or a
    fixed lens (fx, fy, cx, cy, k1, k2), e.g. those a checkpoint learned, in place of the
    dataset's; the refiner does not learn intrinsics.
    ``loss`` / ``loss_scale``: the photometric loss, as in ``Trainer``."""

    def __init__(self, model_coarse, model_fine, camera_params, pixel_sampler, render_config,
                 pose_lr: float = 1e-3, max_norm: float = 0.1, lr_decay: Optional[int] = None,
                 fxy: Optional[torch.Tensor] = None, loss: str = "mse", loss_scale: float = 0.1):
        self.photometric = _check_photometric(loss, loss_scale)
        self.fxy = fxy.detach() if fxy is not None else None
        if camera_params.learn_rotation and not camera_params.fixed_small_angle:
            raise ValueError("PoseRefiner needs CameraPoseParameters(fixed_small_angle=True): at w = 0 the "
                             "reference's theta < 1e-6 rule blocks the rotation gradient, so the poses could not turn")
        self.poses = list(camera_params.parameters())
        if not self.poses:
            raise ValueError("PoseRefiner: camera_params has no learnable rotation or translation")
        self.model_coarse, self.model_fine = model_coarse, model_fine
        self.camera_params, self.pixel_sampler, self.render_config = camera_params, pixel_sampler, render_config
        self.max_norm = max_norm
        self._frozen = [(p, p.requires_grad) for net in (model_coarse, model_fine) if net is not None
                        for p in net.parameters()]
        for p, _ in self._frozen:
            p.requires_grad_(False)
        self.optimizer_poses = FusedAdam(self.poses, lr=pose_lr)
        self.scheduler_poses = (torch.optim.lr_scheduler.LambdaLR(self.optimizer_poses, lr_lambda_factory(lr_decay))
                                if lr_decay is not None else None)

    def close(self) -> None:
        """Give the networks' parameters their ``requires_grad`` back."""
        for p, was in self._frozen:
            p.requires_grad_(was)
        self._frozen = []

    def __enter__(self) -> "PoseRefiner":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def step(self, pixel_batch, t_rand: Optional[torch.Tensor] = None,
             u: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        self.optimizer_poses.zero_grad(set_to_none=True)
        poses = self.camera_params.get_all_poses()
        rays_o, rays_d = self.pixel_sampler.get_rays_for_batch(pixel_batch, poses, self.fxy)
        out = render_rays(self.model_coarse, self.model_fine, rays_o, rays_d, self.render_config, is_train=True,
                          t_rand=t_rand, u=u, target_rgb=pixel_batch.target_rgb,
                          photometric=self.photometric)
        bwd, loss, metrics = _step_losses(out)
        bwd.backward(ops.unit_grad(loss.device))
        self.optimizer_poses.step(clip_groups=[(self.poses, self.max_norm)])
        if self.scheduler_poses is not None:
            self.scheduler_poses.step()
        metrics["loss"] = loss.detach()
        return metrics


def _adopt_reduced_grad(net, flats) -> None:
    """The MLP backward hands autograd views of its flat gradient, which AccumulateGrad
    normally adopts as ``.grad``; if it copied them instead, copy the reduced values."""
    from .optim import _contiguous_run
    g = _contiguous_run([p.grad for p in net.parameters()])
    if g is not None and any(g.data_ptr() == f.data_ptr() for f in flats):
        return
    # this net's own flat gradient (the coarse and fine nets have equal sizes, and with a
    # coarse stream the coarse all-reduce may be launched first)
    last = getattr(net, "_last_gflat", None)
    mine = [f for f in flats if last is not None and f.data_ptr() == last.data_ptr()]
    for f in mine or flats:
        if f.numel() == net._param_count:
            off = 0
            for p in net.parameters():
                n = p.numel()
                p.grad.copy_(f[off:off + n].view(p.shape))
                off += n
            del flats[next(i for i, x in enumerate(flats) if x is f)]  # by identity (== is elementwise)
            return
