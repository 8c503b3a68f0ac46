"""CPU: FusedAdam's host logic (noisy_src/optim.py) against torch.optim.Adam.

The HIP kernels are replaced by stand-ins built from adam_ref in fp32 (ops.sumsq_partials,
ops.sumsq_into, ops.adam_multi, ops.adam_step; ops._check a no-op; model.flat_owner None),
which work in place on the same fp32 CPU tensors FusedAdam hands to the kernels and record
every launch: which spans, which step, which clip source.  What is under test is everything
FusedAdam decides on the host: which parameters form a run, which step number and which
clip coefficient a run is launched with, and which moment buffers it updates.

Every scenario runs 6 steps with seeded random gradients at lr 1e-2 next to
``clip_grad_norm_`` + ``torch.optim.Adam`` on twins of the parameters and is compared after
every step:

  step counters  ``int(state[p]["step"])`` equals torch's for every parameter, and no two
                 parameters hold the same step tensor
  parameters     ``|p - p_torch| <= 1e-4 lr k + 4 ulp(p)`` after k steps.  The stand-in
                 repeats torch's fp32 operations, so an honest difference is a few ulps of
                 an update of size <= lr per step, about 1e-6 lr; a run launched with the
                 wrong step number or with stale moments moves a coordinate by 0.1 lr or
                 more at the first wrong step.  The bound is 100 times above the rounding
                 and 1000 times below the failure.

Before FusedAdam kept one step counter per parameter and checked its cached moments
against ``self.state``, the split, missing-gradient and rejoin scenarios failed: a run
[A, B] that split by clip group at step 2 launched A with step 2 and B with step 3 (torch:
2 and 2), a B without a gradient at step 2 was at 3 one step later (torch: 2), and after
[A, B] -> [A] -> [A, B] the third launch updated the first step's moments again."""
import copy
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adam_ref  # noqa: E402

LR = 1e-2
STEPS = 6


@pytest.fixture
def launches(monkeypatch):
    """Install the stand-in kernels; the list of recorded launches."""
    from noisy_src import model, ops
    log = []

    def source(t):
        """The index of the launch that produced the clip source ``t``."""
        hits = [i for i, rec in enumerate(log) if rec.get("out") is t]
        assert hits, "a clip source no sumsq launch produced"
        return hits[-1]

    def sumsq_partials(xs, out=None):
        assert 1 <= len(xs) <= ops.MAX_ADAM_SPANS
        out = torch.zeros(256) if out is None else out.zero_()
        out[0] = sum((x.double() ** 2).sum() for x in xs).float()
        log.append(dict(kind="sumsq_partials", ns=[x.numel() for x in xs], out=out))
        return out

    def sumsq_into(x, acc):
        assert x.data_ptr() % 16 == 0
        acc += (x.double() ** 2).sum().float()
        if not (log and log[-1]["kind"] == "sumsq_into" and log[-1]["out"] is acc):
            log.append(dict(kind="sumsq_into", ns=[], out=acc))
        log[-1]["ns"].append(x.numel())

    def adam_multi(spans, lr, beta1, beta2, eps, step, sched=None):
        assert 1 <= len(spans) <= ops.MAX_ADAM_SPANS and sched is None
        rec = dict(kind="adam_multi", step=step, lr=lr, spans=[])
        for sp in spans:
            assert all(sp[k].numel() == sp["p"].numel() and sp[k].data_ptr() % 16 == 0 for k in "pgmv")
            assert "sumsq" not in sp
            coef = adam_ref.clip_coef(sp["partials"].sum(), sp["max_norm"]) if "partials" in sp else None
            adam_ref.adam_step(sp["p"], sp["g"], sp["m"], sp["v"], step, lr, (beta1, beta2), eps, coef)
            rec["spans"].append(dict(n=sp["p"].numel(), p=sp["p"].data_ptr(), m=sp["m"].data_ptr(),
                                     v=sp["v"].data_ptr(), max_norm=sp.get("max_norm"),
                                     clip=source(sp["partials"]) if "partials" in sp else None))
        log.append(rec)

    def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, sumsq=None, max_norm=1.0):
        coef = adam_ref.clip_coef(sumsq, max_norm) if sumsq is not None else None
        adam_ref.adam_step(p, g, m, v, step, lr, (beta1, beta2), eps, coef)
        log.append(dict(kind="adam_step", step=step, lr=lr, n=p.numel(), p=p.data_ptr(), m=m.data_ptr(),
                        max_norm=max_norm, clip=source(sumsq) if sumsq is not None else None))

    monkeypatch.setattr(ops, "sumsq_partials", sumsq_partials)
    monkeypatch.setattr(ops, "sumsq_into", sumsq_into)
    monkeypatch.setattr(ops, "adam_multi", adam_multi)
    monkeypatch.setattr(ops, "adam_step", adam_step)
    monkeypatch.setattr(ops, "_check", lambda *ts: None)
    monkeypatch.setattr(model, "flat_owner", lambda p: None)
    return log


class Twins:
    """Parameters for FusedAdam (``p``) and their twins for torch's Adam (``t``).
    ``storages``: one list of shapes per storage; the parameters of one storage lie back to
    back in it, and so do their gradients (as a network's flat buffers do)."""

    def __init__(self, storages, seed=0):
        self.gen = torch.Generator().manual_seed(seed)
        self.p, self.t, self.storage_of = [], [], []
        for shapes in storages:
            sizes = [int(torch.Size(s).numel()) for s in shapes]
            flat = torch.randn(sum(sizes), generator=self.gen)
            idxs, off = [], 0
            for s, n in zip(shapes, sizes):
                idxs.append(len(self.p))
                self.p.append(torch.nn.Parameter(flat[off:off + n].view(s)))
                self.t.append(torch.nn.Parameter(flat[off:off + n].clone().view(s)))
                off += n
            self.storage_of.append(idxs)
        self.k = 0

    def clones(self):
        """Separately allocated copies of the current (p, t)."""
        return ([torch.nn.Parameter(p.detach().clone()) for p in self.p],
                [torch.nn.Parameter(t.detach().clone()) for t in self.t])

    def set_grads(self, targets, scale=1.0, nograd=()):
        """One draw of gradients, given to every (p list, t list) pair of ``targets``."""
        for idxs in self.storage_of:
            sizes = [self.p[i].numel() for i in idxs]
            flat = torch.randn(sum(sizes), generator=self.gen) * scale
            for ps, ts in targets:
                mine, off = flat.clone(), 0
                for i, n in zip(idxs, sizes):
                    if i in nograd:
                        ps[i].grad = ts[i].grad = None
                    else:
                        ps[i].grad = mine[off:off + n].view(ps[i].shape)
                        ts[i].grad = flat[off:off + n].clone().view(ts[i].shape)
                    off += n


def _ulp32(x):
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs().clamp_min(2.0 ** -126)).exponent - 24)


def _steps_done(opt, p):
    st = opt.state.get(p)
    return int(st["step"]) if st and "step" in st else 0


def _compare(opt, topt, ps, ts, k, lrs=None):
    """The module docstring's assertions after ``k`` steps (``ps`` may live on a device)."""
    for i, (p, t) in enumerate(zip(ps, ts)):
        assert _steps_done(opt, p) == _steps_done(topt, t), (k, i, [(_steps_done(opt, a), _steps_done(topt, b))
                                                                   for a, b in zip(ps, ts)])
    held = [opt.state[p]["step"] for p in ps if "step" in opt.state.get(p, ())]
    assert len({id(s) for s in held}) == len(held), "two parameters share one step tensor"
    for i, (p, t) in enumerate(zip(ps, ts)):
        lr = LR if lrs is None else lrs[i]
        bound = 1e-4 * lr * k + 4 * _ulp32(t.detach())
        d = (p.detach().cpu() - t.detach()).abs()
        assert bool((d <= bound).all()), (k, i, d.max().item(), lr)


def _step(opt, topt, ps, ts, clip=()):
    opt.step(clip_groups=[([ps[i] for i in idxs], mn) for idxs, mn in clip])
    for idxs, mn in clip:
        torch.nn.utils.clip_grad_norm_([ts[i] for i in idxs if ts[i].grad is not None], mn)
    topt.step()


def _run(tw, opt, topt, clip_at=lambda k: (), nograd_at=lambda k: (), scale_at=lambda k: 1.0, after=None,
         lrs=None, steps=STEPS):
    for _ in range(steps):
        tw.k += 1
        tw.set_grads([(tw.p, tw.t)], scale_at(tw.k), nograd_at(tw.k))
        _step(opt, topt, tw.p, tw.t, clip_at(tw.k))
        _compare(opt, topt, tw.p, tw.t, tw.k, lrs)
        if after is not None:
            after(tw.k)


def _pair(tw, **kw):
    from noisy_src.optim import FusedAdam
    return FusedAdam(tw.p, lr=LR, **kw), torch.optim.Adam(tw.t, lr=LR, **kw)


def _multi(log):
    return [rec for rec in log if rec["kind"] == "adam_multi"]


AB = [[(2, 4), (12,)]]  # A and B back to back in one storage, both 16-byte aligned


def test_split_by_clip_group(launches):
    """[A, B] stepped jointly, then A alone in a clip group for one step (the run splits
    into [A] and [B], both at the same step), then jointly again."""
    tw = Twins(AB)
    opt, topt = _pair(tw)
    marks = {}
    _run(tw, opt, topt, clip_at=lambda k: [([0], 0.5)] if k == 3 else (),
         after=lambda k: marks.__setitem__(k, len(launches)))
    per_step = {k: _multi(launches[marks.get(k - 1, 0):marks[k]]) for k in marks}
    for k, recs in per_step.items():
        assert [r["step"] for r in recs] == [k], (k, recs)  # one launch, with torch's step number
        sizes = [s["n"] for s in recs[0]["spans"]]
        assert sizes == ([8, 12] if k == 3 else [20]), (k, sizes)
    a, b = per_step[3][0]["spans"]
    assert a["clip"] is not None and a["max_norm"] == 0.5 and b["clip"] is None


def test_missing_gradient(launches):
    """B has no gradient for one step: torch leaves B's counter alone, so from then on A
    and B are launched with different step numbers."""
    tw = Twins(AB)
    opt, topt = _pair(tw)
    _run(tw, opt, topt, nograd_at=lambda k: (1,) if k == 3 else ())
    assert _steps_done(opt, tw.p[0]) == STEPS and _steps_done(opt, tw.p[1]) == STEPS - 1
    last = _multi(launches)[-2:]
    assert sorted((r["step"], r["spans"][0]["n"]) for r in last) == [(STEPS - 1, 12), (STEPS, 8)]


def test_split_then_rejoin_keeps_the_moments(launches):
    """[A, B] -> [A] + [B] -> [A, B], twice: the launch after a rejoin runs on moments that
    hold every earlier update (they equal torch's), and the exp_avg / exp_avg_sq in
    ``state_dict()`` are the buffers that launch wrote."""
    tw = Twins(AB)
    opt, topt = _pair(tw)

    def after(k):
        sd = opt.state_dict()["state"]
        assert sorted(sd) == [0, 1] and all(sorted(sd[i]) == ["exp_avg", "exp_avg_sq", "step"] for i in sd)
        written = {}
        for rec in launches:  # the last launch that covered each parameter
            if rec["kind"] == "adam_multi" and rec["step"] == k:
                for sp in rec["spans"]:
                    for i, p in enumerate(tw.p):
                        off = p.data_ptr() - sp["p"]
                        if 0 <= off < 4 * sp["n"]:
                            written[i] = (sp["m"] + off, sp["v"] + off)
        for i, t in enumerate(tw.t):
            assert (sd[i]["exp_avg"].data_ptr(), sd[i]["exp_avg_sq"].data_ptr()) == written[i], (k, i)
            for key in ("exp_avg", "exp_avg_sq"):
                want = topt.state[t][key]
                assert sd[i][key].shape == want.shape
                assert (sd[i][key] - want).abs().max() <= 1e-5 * want.abs().max(), (k, i, key)

    _run(tw, opt, topt, clip_at=lambda k: [([0], 0.5)] if k in (2, 4) else (), after=after)
    assert [[s["n"] for s in r["spans"]] for r in _multi(launches)] == [[20], [8, 12], [20], [8, 12], [20], [20]]


POSE = [[(10, 3)], [(10, 3)], [(1,)], [(2,)]]  # rotation and translation deltas, focal pair


def test_pose_shaped_parameters(launches):
    """Small separately allocated tensors with n % 4 != 0, each a span of its own, in two
    clip groups; the gradient scale moves both groups across their max_norm."""
    tw = Twins(POSE)
    opt, topt = _pair(tw)
    clip = [([0, 1], 0.1), ([2, 3], 0.05)]
    _run(tw, opt, topt, clip_at=lambda k: clip, scale_at=lambda k: (1.0, 1e-3, 3e-2, 1.0, 10.0, 1e-2)[k - 1])
    recs = _multi(launches)
    assert len(recs) == STEPS and not [r for r in launches if r["kind"] in ("adam_step", "sumsq_into")]
    for k, rec in enumerate(recs, start=1):
        assert rec["step"] == k and [s["n"] for s in rec["spans"]] == [30, 30, 1, 2]
        c = [s["clip"] for s in rec["spans"]]
        assert c[0] == c[1] and c[2] == c[3] and c[0] != c[2] and None not in c
        assert [s["max_norm"] for s in rec["spans"]] == [0.1, 0.1, 0.05, 0.05]
        assert launches[c[0]]["ns"] == [30, 30] and launches[c[2]]["ns"] == [1, 2]


NINE = [[(4,)], [(3, 3)], [(1,)], [(8,)], [(2,)], [(5,)], [(4, 2)], [(7,)], [(6,)]]


def test_nine_tensors_in_one_clip_group(launches):
    """More buffers than one nr_sumsq_partials launch takes: the accumulator path, one
    nr_sumsq per buffer into one accumulator and one nr_adam_step per buffer reading it."""
    tw = Twins(NINE)
    opt, topt = _pair(tw)
    _run(tw, opt, topt, clip_at=lambda k: [(list(range(9)), 1.0)])
    assert not _multi(launches) and not [r for r in launches if r["kind"] == "sumsq_partials"]
    sums = [i for i, r in enumerate(launches) if r["kind"] == "sumsq_into"]
    assert len(sums) == STEPS and all(launches[i]["ns"] == [p.numel() for p in tw.p] for i in sums)
    steps = [r for r in launches if r["kind"] == "adam_step"]
    assert len(steps) == 9 * STEPS
    for k in range(STEPS):
        mine = steps[9 * k:9 * k + 9]
        assert [r["n"] for r in mine] == [p.numel() for p in tw.p]
        assert all(r["step"] == k + 1 and r["clip"] == sums[k] and r["max_norm"] == 1.0 for r in mine)


def test_nine_tensors_without_a_clip_group(launches):
    """More runs than one nr_adam_multi launch takes: launches of 8 and 1 spans."""
    tw = Twins(NINE)
    opt, topt = _pair(tw)
    _run(tw, opt, topt)
    assert [r["kind"] for r in launches] == ["adam_multi"] * (2 * STEPS)
    assert [len(r["spans"]) for r in launches] == [8, 1] * STEPS
    assert [r["step"] for r in launches] == [k for k in range(1, STEPS + 1) for _ in range(2)]
    assert all(s["clip"] is None for r in launches for s in r["spans"])


def test_two_param_groups(launches):
    """Two groups with their own lr and betas, in one clip group across both."""
    from noisy_src.optim import FusedAdam
    tw = Twins([[(2, 4), (12,)], [(10, 3)], [(3,)]])
    lrs = [LR, LR, 3e-3, 3e-3]

    def groups(ps):
        return [dict(params=ps[:2], lr=LR), dict(params=ps[2:], lr=3e-3, betas=(0.8, 0.99), eps=1e-6)]

    opt, topt = FusedAdam(groups(tw.p)), torch.optim.Adam(groups(tw.t))
    _run(tw, opt, topt, clip_at=lambda k: [([0, 1, 2, 3], 1.0)], lrs=lrs)
    recs = _multi(launches)
    assert [r["lr"] for r in recs] == [LR, 3e-3] * STEPS
    assert [[s["n"] for s in r["spans"]] for r in recs] == [[20], [30, 3]] * STEPS


def test_checkpoint_round_trip(launches):
    """After three steps the state goes into a torch.optim.Adam and into a fresh FusedAdam
    (both over copies of the parameters), which continue for three steps next to the
    original pair; then torch's state goes into another fresh FusedAdam.  The FusedAdam
    loads take the live dict, not a copy of it: it clones the counters it adopts, so the
    optimizers count independently of each other."""
    from noisy_src.optim import FusedAdam
    tw = Twins(AB + POSE[:1])
    opt, topt = _pair(tw)
    clip = [([0, 1], 0.5)]
    _run(tw, opt, topt, clip_at=lambda k: clip if k == 2 else (), steps=3)
    p2, t2 = tw.clones()
    opt2, topt2 = FusedAdam(p2, lr=LR), torch.optim.Adam(t2, lr=LR)
    opt2.load_state_dict(opt.state_dict())
    topt2.load_state_dict(copy.deepcopy(opt.state_dict()))  # as read back from a file
    for _ in range(3):
        tw.k += 1
        tw.set_grads([(tw.p, tw.t), (p2, t2)])
        _step(opt, topt, tw.p, tw.t)
        _step(opt2, topt2, p2, t2)
        _compare(opt, topt, tw.p, tw.t, tw.k)
        _compare(opt2, topt2, p2, t2, tw.k)
        _compare(opt2, topt, p2, tw.t, tw.k)
    p3, t3 = tw.clones()
    opt3, topt3 = FusedAdam(p3, lr=LR), torch.optim.Adam(t3, lr=LR)
    opt3.load_state_dict(topt.state_dict())
    topt3.load_state_dict(copy.deepcopy(topt.state_dict()))
    for _ in range(3):
        tw.k += 1
        tw.set_grads([(tw.p, tw.t), (p3, t3)], nograd=(2,) if tw.k == 8 else ())
        _step(opt, topt, tw.p, tw.t)
        _step(opt3, topt3, p3, t3)
        _compare(opt, topt, tw.p, tw.t, tw.k)
        _compare(opt3, topt3, p3, t3, tw.k)
    assert [_steps_done(opt3, p) for p in p3] == [9, 9, 8]
