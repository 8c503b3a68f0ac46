"""
The training steps of ``engine`` captured into hipGraphs (``torch.cuda.graph``) and replayed.

``GraphedTrainer`` replays ``Trainer.step`` and ``GraphedPoseTrainer`` replays
``PoseTrainer.step``, both bit-identical to the eager step.  They share one core: the
static inputs a replay reads (``_StaticInputs``), each optimizer's device schedule pair
(``_AdamSchedule``), the capture with its host bookkeeping rolled back (``_capture``), the
list of device addresses a graph holds (``_bound_buffers`` / ``_check_bound``) and the
replay itself (``_replay``).  What differs is policy: when a class warms up and captures,
how many graphs it keeps, and whether it stages positional-encoding windows.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .optim import FusedAdam


class _StaticInputs:
    """The static tensors a captured step reads: ``static`` (the three batch inputs) and
    ``static_rand`` (t_rand, u; None where the step draws inside the graph).

    Randoms the caller does not inject are drawn into static buffers right before each
    step (eager warm-ups and every replay) rather than inside the graph: the same
    torch.rand calls in the same order as the eager step makes them, so the numbers are
    the eager step's, and a replay skips torch's graph-RNG prologue (two fill launches
    before every replay of a graph that draws).  Only when the step draws nothing else
    (raw_noise_std == 0), which would interleave with them."""

    def __init__(self, who: str, static, t_rand, u, render_config, has_fine: bool):
        self.who, self.static = who, list(static)
        self.static_rand = [None if t is None else t.detach().clone() for t in (t_rand, u)]
        self._predraw = []
        rc = render_config
        if t_rand is None and u is None and rc.perturb and not rc.raw_noise_std:
            B, dev = self.static[0].shape[0], self.static[0].device
            counts = [rc.num_samples] + ([rc.num_samples_fine] if rc.use_hierarchical and has_fine else [])
            for i, n in enumerate(counts):
                self.static_rand[i] = torch.empty(B, n, device=dev)
                self._predraw.append(self.static_rand[i])

    def draw(self) -> None:
        for t in self._predraw:
            t.uniform_()  # torch.rand(shape) of the eager step, into the static buffer

    def stage(self, srcs, t_rand=None, u=None) -> None:
        """Copy the caller's inputs (None, or the static buffer itself: as it is) into the
        static buffers, then draw the randoms that were not injected.  Every input is
        checked before the first copy, so a refused call changes nothing."""
        if len(self._predraw) == 2 and (t_rand is None) != (u is None):
            raise ValueError(f"{self.who}: inject both t_rand and u, or neither")
        dsts, cps, plain = [], [], []
        for dst, src in zip(self.static + self.static_rand, (*srcs, t_rand, u)):
            if src is None or src is dst:
                continue
            if dst is None:
                raise ValueError(f"{self.who}: t_rand / u were drawn in the graph at capture")
            if src.shape != dst.shape:
                raise ValueError(f"{self.who}: input of shape {tuple(src.shape)} for the static buffer "
                                 f"{tuple(dst.shape)}")
            # the int64 image indices keep a copy_ of their own: a list of mixed dtypes
            # would send _foreach_copy_ down its one-launch-per-tensor path
            if src.is_cuda and src.device == dst.device and src.dtype == dst.dtype and dst.is_floating_point():
                dsts.append(dst)
                cps.append(src)
            else:
                plain.append((dst, src))
        for dst, src in plain:
            dst.copy_(src)
        if dsts:
            torch._foreach_copy_(dsts, cps)  # one launch for the floating-point static inputs
        if self._predraw and t_rand is None:
            self.draw()


class _AdamSchedule:
    """One FusedAdam's share of a captured step: the 8-byte device pair its Adam launch
    reads (``FusedAdam.device_sched``), the pinned staging ring the pair is written
    through, and the host bookkeeping (step counters, LambdaLR) a replay advances."""

    RING = 64

    def __init__(self, optimizer: FusedAdam, scheduler, device, what: str):
        if not isinstance(optimizer, FusedAdam) or len(optimizer.param_groups) != 1:
            raise ValueError(f"a graphed step needs a single-group FusedAdam for the {what}")
        self.optimizer, self.scheduler, self.what = optimizer, scheduler, what
        self.pair = torch.zeros(2, device=device, dtype=torch.float32)
        # a slot is rewritten only after the copy that read it has run (its event),
        # however far the host runs ahead
        self._ring = torch.zeros(self.RING, 2, dtype=torch.float32).pin_memory()
        self._ring_ev = [None] * self.RING
        self._k = 0

    def step_states(self):
        opt = self.optimizer
        seen, out = set(), []
        for p in opt.param_groups[0]["params"]:
            st = opt.state.get(p)
            if st and "step" in st and id(st["step"]) not in seen:
                seen.add(id(st["step"]))
                out.append(st)
        return out

    def ready(self) -> bool:
        """An eager step has created the flat m / v buffers and the step counters (a
        capture would otherwise allocate and zero them inside the graph)."""
        opt = self.optimizer
        return bool(opt._flat_state) and all("step" in opt.state.get(p, ()) for p in opt.param_groups[0]["params"])

    def common_step(self) -> int:
        """The one Adam step count every buffer shares (one pair of bias corrections
        drives every span of the captured launch)."""
        vals = {int(st["step"]) for st in self.step_states()}
        if len(vals) != 1:
            raise RuntimeError(f"graphed step: the {self.what} optimizer's buffers are at different steps "
                               f"{sorted(vals)}")
        return vals.pop()

    def snapshot(self):
        return ([(st, st["step"].clone()) for st in self.step_states()], self.scheduler.state_dict(),
                [g["lr"] for g in self.optimizer.param_groups])

    def restore(self, snap) -> None:
        steps, sched_state, lr = snap
        for st, v in steps:
            st["step"].copy_(v)
        self.scheduler.load_state_dict(sched_state)
        for g, v in zip(self.optimizer.param_groups, lr):
            g["lr"] = v

    def write_next(self) -> None:
        """Stage the pair of the step about to be replayed (stream-ordered before it)."""
        group = self.optimizer.param_groups[0]
        b1, b2 = group["betas"]
        a, b = ops.adam_sched_values(group["lr"], b1, b2, self.common_step() + 1)
        slot = self._k % self.RING
        if self._ring_ev[slot] is not None:
            self._ring_ev[slot].synchronize()
        self._ring[slot, 0], self._ring[slot, 1] = a, b  # fp32 rounding, as the host path's
        self.pair.copy_(self._ring[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring_ev[slot] = ev
        self._k += 1

    def advance(self) -> None:
        """What ``optimizer.step(); scheduler.step()`` do on the host."""
        for st in self.step_states():
            st["step"] += 1
        self.scheduler.step()


def _capture(scheds, run_step, distributed: bool):
    """Capture ``run_step()`` with every schedule's optimizer reading its device pair.
    Returns (graph, what run_step returned).  The capture runs the step's host bookkeeping
    (Adam step counters, LR schedulers) once without device work: it is rolled back, and
    eager steps between replays use the host scalars again, also when the capture raises."""
    for s in scheds:
        s.common_step()
    snaps = [s.snapshot() for s in scheds]
    graph = torch.cuda.CUDAGraph()
    # data parallel: the process group's watchdog thread polls the events of the eager
    # warm-up's all-reduces until it has seen them complete.  Under the default "global"
    # capture mode such a query from another thread fails while the capture is open,
    # and the watchdog then ends the process; "thread_local" checks this thread only
    mode = "thread_local" if distributed else "global"
    for s in scheds:
        s.optimizer.device_sched = s.pair
    try:
        with torch.cuda.graph(graph, capture_error_mode=mode):
            out = run_step()
    finally:
        for s, snap in zip(scheds, snaps):
            s.optimizer.device_sched = None
            s.restore(snap)
    return graph, out


def _bound_buffers(nets, scheds, extra=()):
    """(tensor, address) of everything a captured graph reads or writes in place: the
    networks' packed images, pack tables and flat parameters, their window tensors (a
    captured step folds the ones it saw, or none), ``extra`` and the optimizers' m / v."""
    ts = [t for n in nets for t in (n._packed, n._table, n._flat) if t is not None]
    ts += [w for n in nets if n._flat is not None for w in n._pe_window.device_weights(n._flat.device)
           if w is not None]
    ts += extra
    for s in scheds:
        for m, v in s.optimizer._flat_state.values():
            ts += [m, v]
    return [(t, t.data_ptr()) for t in ts]


def _check_bound(who: str, bound, now) -> None:
    if len(now) != len(bound) or any(a is not b or pa != pb for (a, pa), (b, pb) in zip(now, bound)):
        raise RuntimeError(f"{who}: a buffer the captured graph writes was replaced (packed images, pack table, "
                           "parameters, poses or Adam state, e.g. by a checkpoint load), or a "
                           f"positional-encoding window was added or removed; build a new {who}")


def _replay(scheds, graph) -> None:
    for s in scheds:
        s.write_next()
    graph.replay()
    for s in scheds:
        s.advance()


def _nets(trainer):
    return [n for n in (trainer.model_coarse, trainer.model_fine) if n is not None]


class GraphedTrainer:
    """``Trainer.step`` captured once into a hipGraph and replayed: the ~23 kernels of a
    step become one graph launch, so a step costs its GPU time even where the host's
    Python dispatch (autograd, the optimizer's bookkeeping: ~1.3 ms per step) exceeds it
    -- small per-GPU batches such as BASELINE cfg #4's 512 rays per rank.

    Everything the replay needs is on the device: the rays go through static input
    buffers, the jitter / inverse-CDF uniforms are drawn by torch.rand into static
    buffers before each replay (or the caller passes them; torch's graph-safe RNG inside
    the graph when the step also draws noise), the fused Adam launch rewrites the packed
    images, and the two step-dependent Adam scalars come from an 8-byte device pair
    written before each replay (``FusedAdam.device_sched``); the LR schedule and the
    optimizer's step counters advance on the host exactly as in ``Trainer.step``.
    Data parallel: the trainer's RCCL all-reduces (one per network) are captured inside
    the graph in their stream-ordered form, so a replay is the whole DP step.

    The graph holds raw device addresses: every network's packed images and pack table
    and the optimizer's flat m / v buffers.  Those tensors are pinned here, and a replay
    after any of them was replaced (a checkpoint load, ``FusedAdam.load_state_dict``)
    raises instead of writing into freed memory."""

    def __init__(self, trainer, rays_o: torch.Tensor, rays_d: torch.Tensor, target_rgb: torch.Tensor,
                 t_rand: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None, warmup: int = 2):
        self.trainer = trainer
        self._refuse_window()
        dev = rays_o.device
        self._scheds = [_AdamSchedule(trainer.optimizer, trainer.scheduler, dev, "trainer")]
        self._inputs = _StaticInputs("GraphedTrainer", [t.detach().clone() for t in (rays_o, rays_d, target_rgb)],
                                     t_rand, u, trainer.render_config, trainer.model_fine is not None)
        self.static, self.static_rand = self._inputs.static, self._inputs.static_rand

        def run_step():
            return trainer.step(*self.static, *self.static_rand)

        # eager warm-up steps on a side stream (allocator pools, optimizer state, packed
        # images and pack tables exist before the capture); they are real training steps.
        # warmup=0 is accepted once the trainer has stepped eagerly (the state exists):
        # the capture then trains on nothing, so a caller's step sequence is unchanged
        if warmup < 1 and not self._scheds[0].step_states():
            warmup = 1
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._inputs.draw()
                run_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph, self.out = _capture(self._scheds, run_step, trainer.process_group is not None)
        self._bound = _bound_buffers(_nets(trainer), self._scheds)

    def _refuse_window(self) -> None:
        # a replay rewrites the images' encoding columns unfolded behind the host's back,
        # and this class does not stage window weights: only GraphedPoseTrainer does
        for n in _nets(self.trainer):
            if n._pe_window.on:
                raise ValueError("GraphedTrainer does not support a positional-encoding window (NeRF.set_pe_window): "
                                 "use the eager Trainer, or GraphedPoseTrainer")

    def step(self, rays_o: Optional[torch.Tensor] = None, rays_d: Optional[torch.Tensor] = None,
             target_rgb: Optional[torch.Tensor] = None, t_rand: Optional[torch.Tensor] = None,
             u: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Replay one training step on these rays (copied into the static buffers; None:
        the buffers as they are).  Returns the captured metrics (device tensors that every
        replay overwrites).  Eager ``trainer.step`` calls may be interleaved (same state)."""
        self._inputs.stage((rays_o, rays_d, target_rgb), t_rand, u)
        self._refuse_window()
        _check_bound("GraphedTrainer", self._bound, _bound_buffers(_nets(self.trainer), self._scheds))
        _replay(self._scheds, self.graph)
        return self.out


class GraphedPoseTrainer:
    """``PoseTrainer.step`` replayed from hipGraphs: the counterpart of ``GraphedTrainer``
    for the joint pose-optimisation step (BASELINE cfg #3), bit-identical to the eager step.

    The step has two shapes, and each gets its own graph, captured on its first use: with
    frozen poses (``optimize_poses=False``: the poses enter detached, so there is no
    input-gradient pass and no pose Adam) and optimising.  Both read one set of static
    inputs: the pixel batch (``self.static``: image_indices, pixel_coords, target_rgb --
    ``PixelSampler.sample_batch(out=self.static)`` writes a batch straight into them) and
    the jitter / inverse-CDF uniforms (``self.static_rand``).  As in ``GraphedTrainer``,
    randoms the caller does not inject are drawn by torch.rand into the static buffers
    before each step, in the eager step's order (no RNG inside the graph unless the step
    also draws noise).  Each optimizer has its own device schedule pair, written before a
    replay; the Adam step counters and both LambdaLRs advance on the host exactly as in
    ``PoseTrainer.step`` (the pose optimizer's only on optimising steps).

    A coarse-to-fine window (``PoseTrainer.pe_schedule``, or ``NeRF.set_pe_window`` between
    steps) lives in each network's persistent window tensor, which the captured fold and
    gradient-scaling launches read: it is written before a replay, never inside the graph.

    Every call of ``step`` is one training step of the caller's sequence.  The first
    ``warmup`` calls of a shape run eagerly (on the static buffers); so does any call
    while that shape's Adam state does not exist yet -- the optimising graph can only be
    captured after one eager optimising step has created the pose Adam's m / v -- and the
    call after them captures and replays.  The capture is single-stream (``PoseTrainer``
    has no coarse stream).  Data parallel: the network all-reduces and the pose-gradient
    all-reduce are captured (RCCL only).

    The graphs hold raw device addresses: both networks' packed images, pack tables and
    parameters, the pose parameters and both optimizers' flat m / v buffers.  A replay
    after any of them was replaced (a checkpoint load, ``FusedAdam.load_state_dict``)
    raises instead of writing into freed memory."""

    def __init__(self, trainer, pixel_batch, t_rand: Optional[torch.Tensor] = None,
                 u: Optional[torch.Tensor] = None, warmup: int = 2):
        from .data_pose_opt import PixelBatch
        self.trainer = trainer
        self.warmup = int(warmup)
        self._require_in_range(pixel_batch)
        dev = pixel_batch.target_rgb.device
        if trainer.reducer is not None:
            # the captured step contains the all-reduces: only RCCL collectives are capturable
            backend = trainer.reducer.dist.get_backend(trainer.reducer.group)
            if backend != "nccl":
                raise ValueError("GraphedPoseTrainer with data parallelism needs the nccl (RCCL) backend, "
                                 f"not {backend}")
        self._nerf = _AdamSchedule(trainer.optimizer_nerf, trainer.scheduler_nerf, dev, "network")
        self._poses = (_AdamSchedule(trainer.optimizer_poses, trainer.scheduler_poses, dev, "pose")
                       if trainer.optimizer_poses is not None else None)
        self._inputs = _StaticInputs("GraphedPoseTrainer",
                                     [pixel_batch.image_indices.detach().to(torch.int64).clone(),
                                      pixel_batch.pixel_coords.detach().float().clone(),
                                      pixel_batch.target_rgb.detach().float().clone()],
                                     t_rand, u, trainer.render_config, trainer.model_fine is not None)
        self.static, self.static_rand = self._inputs.static, self._inputs.static_rand
        self.batch = PixelBatch(*self.static, in_range=True)
        self._graphs = {}  # optimising (bool) -> (graph, captured metrics, bound buffers)
        self._eager_steps = {False: 0, True: 0}

    @staticmethod
    def _require_in_range(pixel_batch) -> None:
        if not pixel_batch.in_range:
            # the validating ray kernel's flag is read on the host: not capturable
            raise ValueError("GraphedPoseTrainer: the pixel batch must have in_range=True (PixelSampler.sample_batch; "
                             "validate other batches with ops.check_index_range first)")

    def _bound_buffers(self, scheds):
        # learned intrinsics add only their parameter: the ray kernels read (fx, fy) from device
        # memory, recomputed from it inside the graph, so nothing of it is baked into a capture
        intr = getattr(self.trainer, "intrinsics", None)
        return _bound_buffers(_nets(self.trainer), scheds, list(self.trainer.camera_params.parameters())
                              + (list(intr.parameters()) if intr is not None else []))

    def step(self, pixel_batch=None, optimize_poses: bool = True, t_rand: Optional[torch.Tensor] = None,
             u: Optional[torch.Tensor] = None, iteration: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """One training step on this batch (copied into the static buffers; None, or the
        batch ``sample_batch(out=self.static)`` returned: the buffers as they are).
        ``iteration`` sets the windows of ``PoseTrainer.pe_schedule`` first.  Returns
        the metrics of the graph it replayed (device tensors that every replay of that
        graph overwrites).  Eager ``trainer.step`` calls may be interleaved (same state)."""
        optimizing = bool(optimize_poses) and self._poses is not None
        srcs = (None, None, None)
        if pixel_batch is not None:
            self._require_in_range(pixel_batch)
            srcs = (pixel_batch.image_indices, pixel_batch.pixel_coords, pixel_batch.target_rgb)
        self._inputs.stage(srcs, t_rand, u)
        if iteration is not None:
            self.trainer.set_pe_windows(iteration)
        nets = _nets(self.trainer)
        for n in nets:
            if n._flat is not None:
                # the window tensors' pending values go out here, stream-ordered before the
                # replay (as _AdamSchedule.write_next's pair), and never inside a capture
                n._pe_window.device_weights(n._flat.device)
        scheds = [self._nerf] + ([self._poses] if optimizing else [])

        def run_step():
            return self.trainer.step(self.batch, optimize_poses=optimizing, t_rand=self.static_rand[0],
                                     u=self.static_rand[1])

        entry = self._graphs.get(optimizing)
        if entry is None:
            if self._eager_steps[optimizing] < self.warmup or not all(s.ready() for s in scheds):
                self._eager_steps[optimizing] += 1
                return run_step()
            graph, out = _capture(scheds, run_step, self.trainer.reducer is not None)
            entry = self._graphs[optimizing] = (graph, out, self._bound_buffers(scheds))
        graph, out, bound = entry
        _check_bound("GraphedPoseTrainer", bound, self._bound_buffers(scheds))
        _replay(scheds, graph)
        for n in nets:
            # the replayed Adam rewrote the images' encoding columns unfolded, unseen by the host
            n._fold_key = None
        return out
