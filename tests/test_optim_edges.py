"""GPU: the optimizer tail at its edges, against adam_ref in fp64.

nr_sumsq, nr_sumsq_partials, nr_adam_step and nr_adam_multi run through the raw C ABI into
buffers the test owns (test_edge_shapes' ``guarded``: sentinel elements after every output,
which must come back bit for bit; the partials and the workspace start ``poisoned``), at the
sizes where their code takes another path:

  kernel                 path                                    reached by
  ---------------------  --------------------------------------  ------------------------------
  sumsq_partial_kernel,  one float4 trip of the 65 536 threads   n = 262144 (exactly), below
  sumsq_spans_kernel       (262 144 floats), a second one, the     it, 262145 / 262147 (scalar
                           scalar tail, nothing at all              tail past a full trip),
                                                                    524289 (a third trip), 0
  sumsq_spans_kernel     the all-scalar form of a span whose     bases 1, 2, 3 floats past an
                           base is not 16-byte aligned              aligned allocation
                         spans of different lengths, one empty   8 spans, the empty one with a
                                                                    valid pointer and with NULL
  adam_kernel            one grid pass (2048 blocks x 256 x 4),  n = 2097152, 2097156,
                           a second float4 trip, float4 + a         2097159; 1 .. 1024
                           wrapped scalar tail
  adam_multi_kernel      the same, and with n % 4 != 0 the       the same sizes; 8 spans of
                           all-scalar form (four trips); a grid     2097159, 1, 0, 30, 4, 1023,
                           sized by the longest span; an empty      3, 262148 in one launch with
                           span; two clip groups and a span         clip groups A (spans 0-3),
                           without one in one launch                B (4-6) and none (7)
  clip_coef              above / below max_norm, a zero norm,    the clip regimes; one NaN
                           a NaN norm                               gradient element

Sum of squares.  A lone 3.0 at every float4 / trip boundary must give exactly 9.0 (and
``acc_before + 9``); randn against the fp64 sum within ``(4 ceil(n / 262144) + 24) 2^-24``
relative: the terms are non-negative, so the relative error is at most the longest chain of
roundings one term passes through -- its square, 4 additions per trip, 6 butterfly and 4 wave
additions in each of the two passes, and the accumulate.

One Adam step.  From a seeded state (p ~ randn, g ~ s randn with s in 1e-6, 1, 1e3,
m ~ 0.1 randn, v ~ s^2 rand, or m = v = 0 at step 1; step in 1, 2, 1000, 250000; lr 5e-4),
a range that keeps every fp32 intermediate normal.  The reference is adam_ref's fp64 step
from the same fp32 inputs.  The yardstick is torch's own fp32 step on the CPU
(clip_grad_norm_ + torch.optim.Adam with the state injected) against the same fp64 result,
per output tensor in the 2-norm: ``err_kernel <= max(F_ADAM err_torch32, 4 2^-24
max|want|)``, F_ADAM the smallest power of two that is at least twice the largest ratio
measured on an MI355X (never above 16).  The clipped gradient left in ``g`` is also held,
per element, to ``(d / 2 + 4) 2^-24`` relative of ``g coef`` in fp64, d the chain length
above: half the relative error of the sum through the square root, then the add, the
divide, the select and the multiply.  Each case prints an ``OPTIM_PARITY`` line; one full
run is kept in profiles/optim_edge_parity.json.

Measured on an MI355X, err_kernel / err_torch32 over the cases above the floor:

  nr_adam_step, nr_adam_multi (identical figures: the two kernels give the same bits)
                        g 4.22, v 3.26, m 2.92 (all three n = 1023, s = 1e-6, step 1, norm
                        above max_norm), p 1.69 (n = 30, s = 1e-6, step 250000, no clip)
  the eight-span launch g 1.70, m 2.44, v 2.97 (span 5, n = 1023, step 1), p 1.00  -> F_ADAM = 16

Twice the largest ratio is 8.44, so the smallest admissible power of two is 16, which is also
the cap.  The median over the cases above the floor is 1.0 for every output; with the clip
inactive the largest ratios are 1.69 (p) and 1.25 (m: ``m + (1 - b1) (g - m)`` against
torch's lerp).  The ratios above 2 all come from an active clip at step 1: the coefficient is one
fp32 number that multiplies every element, so its rounding (half an ulp either way, in the
kernel as in torch) is a *coherent* error of the whole tensor, and the ratio compares two
single roundings -- as for g_rays_d at B = 1 in test_edge_shapes.  At step 1 (m = v = 0) m and
v are that clipped gradient times a constant, so they inherit it.  The sum of squares stays
under 0.05 of its bound (n = 524289: 9.3e-8 against 2.1e-6)."""
import ctypes
import functools
import json
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adam_ref  # noqa: E402
import edge_inputs as ei  # noqa: E402
from test_edge_shapes import DEV, _Guarded, poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64
F_ADAM = 16
LR = 5e-4
B1, B2 = adam_ref.BETAS
EPS = adam_ref.EPS
PAD = 64  # sentinel elements behind every buffer
TRIP = 256 * 256 * 4  # floats one float4 trip of the sum-of-squares grid covers
NR_EARG = -22
U = 2.0 ** -24


def _record(**kw):
    print("OPTIM_PARITY " + json.dumps(kw))


def chain(n):
    """The longest chain of roundings a term of the sum of squares passes through."""
    return 4 * max(1, -(-n // TRIP)) + 24


def gbuf(x):
    """``x`` (1-D, fp32, CPU) on the device with PAD sentinel elements behind it."""
    tail = (torch.arange(PAD) % 7).float() * 0.5 - 60.25
    return _Guarded((x.numel(),), PAD, torch.cat([x.float().reshape(-1), tail]))


def _lib():
    from noisy_src import _hip
    return _hip.load()


def _stream():
    from noisy_src import _hip
    return _hip.stream_ptr()


def _ptr(t):
    """The device address of ``t`` (an empty view has none of its own: its place in its storage)."""
    if t is None:
        return None
    return t.data_ptr() if t.numel() else t.untyped_storage().data_ptr() + 4 * t.storage_offset()


def _raw(name, *args):
    """The entry point's return code (no exception on an error)."""
    return getattr(_lib(), name)(*[_ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _stream())


def _ok(name, *args):
    rc = _raw(name, *args)
    assert rc == 0, (name, rc, _last_error())


def _last_error():
    from noisy_src import _hip
    return _hip.last_error()


def _workspace():
    return poisoned(_lib().nr_sumsq_workspace_bytes())


def _new_partials():
    """The 256 partials, poisoned, with sentinels behind them."""
    return gbuf(torch.full((256,), float("nan")))


def _sumsq(x, n, acc_before):
    """nr_sumsq of the device view ``x`` onto ``acc_before`` -> the accumulator's value."""
    acc = gbuf(torch.tensor([acc_before]))
    ws = _workspace()
    _ok("nr_sumsq", x, n, acc.buf, ws)
    torch.cuda.synchronize()
    acc.check()
    return acc.out.item()


def _partials(spans, out=None):
    """nr_sumsq_partials over ``spans`` [(device view or None, n)] -> the guarded partials."""
    out = _new_partials() if out is None else out
    ptrs = (ctypes.c_void_p * len(spans))(*[_ptr(x) for x, _ in spans])
    ns = (ctypes.c_int64 * len(spans))(*[n for _, n in spans])
    _ok("nr_sumsq_partials", ptrs, ns, len(spans), out.buf)
    torch.cuda.synchronize()
    out.check()
    return out


def _host_sum(part):
    got = part.out.cpu()
    assert torch.isfinite(got).all()
    return got.double().sum().item()


def _offset_view(n, off, fill=None):
    """A device view of n floats that starts ``off`` floats past an aligned allocation."""
    base = torch.zeros(n + off + PAD, device=DEV)
    assert base.data_ptr() % 16 == 0
    v = base[off:off + n]
    if fill is not None:
        v.copy_(fill)
    return v


def _edge_positions(n):
    pos = {0, 4 * (n // 4) - 1, 4 * (n // 4), n - 1}
    for k in range(1, n // TRIP + 1):
        pos |= {TRIP * k - 1, TRIP * k, TRIP * k + 1}
    return sorted(p for p in pos if 0 <= p < n)


SUMSQ_N = [0, 1, 3, 4, 5, 1023, 262144, 262145, 262147, 524289]


@functools.lru_cache(maxsize=None)
def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------- sum of squares --
@pytest.mark.parametrize("off", [0, 1, 2, 3], ids=lambda o: f"base+{o}")
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_vs_fp64(n, off):
    """nr_sumsq (aligned bases only: it refuses others) and nr_sumsq_partials summed on
    the host in fp64, on one buffer of n floats at an aligned base and 1, 2, 3 floats past
    one: a lone 3.0 at every edge position gives exactly 9.0, randn stays within the chain
    bound of the fp64 sum, and n = 0 leaves ``acc`` alone / writes all-zero partials."""
    apis = (["sumsq"] if off == 0 else []) + ["partials"]
    x = _offset_view(n, off)
    if n == 0:
        if off == 0:
            ws = _workspace()
            acc = gbuf(torch.tensor([1.5]))
            _ok("nr_sumsq", x, 0, acc.buf, ws)
            torch.cuda.synchronize()
            acc.check()
            assert acc.out.item() == 1.5 and bool((ws == 0xFF).all())
        part = _partials([(x, 0)])
        assert torch.count_nonzero(part.out) == 0
        return
    for pos in _edge_positions(n):
        x[pos] = 3.0
        if "sumsq" in apis:
            assert _sumsq(x, n, 0.0) == 9.0, pos
            assert _sumsq(x, n, 1.5) == 10.5, pos
        assert _host_sum(_partials([(x, n)])) == 9.0, pos
        x[pos] = 0.0
    r = _randn(n, 100 + n)
    x.copy_(r)
    want = (r.double() ** 2).sum().item()
    bound = chain(n) * U
    for api in apis:
        got = _sumsq(x, n, 0.0) if api == "sumsq" else _host_sum(_partials([(x, n)]))
        rel = abs(got - want) / want
        _record(test="sumsq", api=api, n=n, off=off, rel=rel, bound=bound)
        assert rel <= bound, (api, rel, bound)


SPAN_N = [262147, 1, 0, 30, 4, 1023, 3, 130]


@pytest.mark.parametrize("empty", ["valid", "null"])
def test_sumsq_partials_eight_spans(empty):
    """Eight spans of different lengths in one launch, the empty one with a valid pointer
    or with NULL: a lone 3.0 at the ends of every span (and around the big span's float4 and
    trip boundaries) gives exactly 9.0; randn is within the chain bound over the whole."""
    xs = [_offset_view(n, 0) for n in SPAN_N]
    spans = [(None if (n == 0 and empty == "null") else x, n) for x, n in zip(xs, SPAN_N)]
    for x, n in zip(xs, SPAN_N):
        for pos in ([] if n == 0 else sorted({0, n - 1} | (set(_edge_positions(n)) if n > TRIP else set()))):
            x[pos] = 3.0
            assert _host_sum(_partials(spans)) == 9.0, (n, pos)
            x[pos] = 0.0
    want = 0.0
    for k, (x, n) in enumerate(zip(xs, SPAN_N)):
        r = _randn(n, 200 + k)
        x.copy_(r)
        want += (r.double() ** 2).sum().item()
    rel = abs(_host_sum(_partials(spans)) - want) / want
    bound = chain(sum(SPAN_N)) * U
    _record(test="sumsq_spans", empty=empty, rel=rel, bound=bound)
    assert rel <= bound, (rel, bound)


def test_sumsq_argument_errors():
    """nspan 0 and 9, and an unaligned x given to nr_sumsq: NR_EARG, a message, and the
    outputs untouched."""
    x = _offset_view(64, 0, torch.ones(64))
    ptrs = (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9)
    ns = (ctypes.c_int64 * 9)(*[64] * 9)
    for nspan in (0, 9):
        part = _new_partials()
        before = part.buf.clone()
        assert _raw("nr_sumsq_partials", ptrs, ns, nspan, part.buf) == NR_EARG
        assert "nr_sumsq_partials" in _last_error()
        torch.cuda.synchronize()
        assert torch.equal(part.buf.view(torch.int32), before.view(torch.int32))
    acc = gbuf(torch.tensor([1.5]))
    ws = _workspace()
    assert _raw("nr_sumsq", _offset_view(64, 1, torch.ones(64)), 64, acc.buf, ws) == NR_EARG
    assert "aligned" in _last_error()
    torch.cuda.synchronize()
    acc.check()
    assert acc.out.item() == 1.5 and bool((ws == 0xFF).all())


# -------------------------------------------------------------- one Adam step --
def adam_state(n, s, step, seed, zero_g=False):
    """The seeded fp32 state (p, g, m, v) of the module docstring."""
    p = _randn(n, seed).clone()
    g = torch.zeros(n) if zero_g else _randn(n, seed + 1) * s
    if step == 1:
        return p, g, torch.zeros(n), torch.zeros(n)
    m = 0.1 * _randn(n, seed + 2)
    v = torch.rand(n, generator=torch.Generator().manual_seed(seed + 3)) * s ** 2
    return p, g, m, v


def reference_step(states, step, groups):
    """The fp64 reference and torch's fp32 step for ``states`` [(p, g, m, v)] with clip
    ``groups`` [(indices, max_norm)] -> (want, t32): per state a dict p, g, m, v; and each
    state's fp64 clip coefficient (None outside every group)."""
    coef = [None] * len(states)
    for idxs, max_norm in groups:
        c = adam_ref.clip_coef(sum((states[i][1].double() ** 2).sum() for i in idxs), max_norm)
        for i in idxs:
            coef[i] = c
    want = []
    for (p, g, m, v), c in zip(states, coef):
        w = dict(p=p.double(), g=g.double(), m=m.double(), v=v.double())
        adam_ref.adam_step(w["p"], w["g"], w["m"], w["v"], step, LR, coef=c)
        want.append(w)
    tp = [torch.nn.Parameter(p.clone()) for p, _, _, _ in states]
    opt = torch.optim.Adam(tp, lr=LR, betas=(B1, B2), eps=EPS)
    for t, (_, g, m, v) in zip(tp, states):
        t.grad = g.clone()
        if step > 1:
            opt.state[t] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    for idxs, max_norm in groups:
        torch.nn.utils.clip_grad_norm_([tp[i] for i in idxs], max_norm)
    opt.step()
    t32 = [dict(p=t.detach(), g=t.grad, m=opt.state[t]["exp_avg"], v=opt.state[t]["exp_avg_sq"]) for t in tp]
    return want, t32, coef


def _span_struct(bufs, n, partials, max_norm):
    from noisy_src import _hip
    return _hip.NrAdamSpan(_ptr(bufs["p"].buf), _ptr(bufs["g"].buf), _ptr(bufs["m"].buf), _ptr(bufs["v"].buf), n,
                           _ptr(None if partials is None else partials.buf), float(max_norm), None, None)


def launch_multi(states, step, groups, sched=None, host_step=None):
    """One nr_adam_multi launch over ``states`` with one nr_sumsq_partials launch per clip
    group -> per state the outputs p, g, m, v on the CPU (sentinels checked)."""
    from noisy_src import _hip
    bufs = [dict(zip("pgmv", [gbuf(t) for t in st])) for st in states]
    src = [(None, 1.0)] * len(states)
    for idxs, max_norm in groups:
        part = _partials([(bufs[i]["g"].buf, states[i][1].numel()) for i in idxs])
        for i in idxs:
            src[i] = (part, max_norm)
    arr = (_hip.NrAdamSpan * len(states))(*[_span_struct(b, st[0].numel(), *sc)
                                            for b, st, sc in zip(bufs, states, src)])
    _ok("nr_adam_multi", arr, len(states), LR, B1, B2, EPS, step if host_step is None else host_step, sched)
    torch.cuda.synchronize()
    for b in bufs:
        for t in b.values():
            t.check()
    for part in {id(p): p for p, _ in src if p is not None}.values():
        part.check()
    return [{k: t.out.cpu() for k, t in b.items()} for b in bufs]


def launch_step(state, step, max_norm):
    """nr_sumsq into a zeroed accumulator (``max_norm`` not None) + nr_adam_step."""
    b = dict(zip("pgmv", [gbuf(t) for t in state]))
    n = state[0].numel()
    acc = None
    if max_norm is not None:
        acc = gbuf(torch.zeros(1))
        _ok("nr_sumsq", b["g"].buf, n, acc.buf, _workspace())
    _ok("nr_adam_step", b["p"].buf, b["g"].buf, b["m"].buf, b["v"].buf, n, LR, B1, B2, EPS, step,
        None if acc is None else acc.buf, 1.0 if max_norm is None else float(max_norm))
    torch.cuda.synchronize()
    for t in b.values():
        t.check()
    if acc is not None:
        acc.check()
    return {k: t.out.cpu() for k, t in b.items()}


def check_outputs(tag, got, want, t32, state, coef, nsum):
    """The yardstick bound for p, g, m, v, the per-element bound on the clipped gradient,
    and a bit-unchanged ``g`` wherever the coefficient is exactly 1."""
    n = state[0].numel()
    err = {k: ei.distance(k, got[k], want[k]) for k in "pgmv"}
    e32 = {k: ei.distance(k, t32[k].reshape(-1), want[k]) for k in "pgmv"}
    scale = {k: (want[k].abs().max().item() if n else 0.0) for k in "pgmv"}
    _record(**tag, n=n, err=err, e32=e32, scale=scale, coef=None if coef is None else coef.item())
    for k in "pgmv":
        assert got[k].shape == (n,) and torch.isfinite(got[k]).all(), (tag, k)
    if n == 0:
        return
    if coef is None or coef.item() == 1.0:
        assert torch.equal(got["g"].view(torch.int32), state[1].view(torch.int32)), tag
    else:
        rel = (chain(nsum) / 2 + 4) * U
        assert bool(((got["g"].double() - want["g"]).abs() <= rel * want["g"].abs()).all()), tag
    for k in "pgmv":
        assert err[k] <= ei.yardstick_bound(F_ADAM, e32[k], want[k]), (tag, k, err[k], e32[k], scale[k])


SCALES = [1e-6, 1.0, 1e3]
STEPS = [1, 2, 1000, 250000]
REGIMES = ["none", "above", "below", "zero_g"]
SMALL_N = [1, 2, 3, 5, 30, 1023, 1024]
LARGE_N = [2097152, 2097156, 2097159]
# at the large sizes: every scale, step and regime once, not their product
LARGE_COMBOS = [(1.0, 1, "above"), (1e-6, 2, "below"), (1e3, 1000, "none"), (1.0, 250000, "zero_g"),
                (1e3, 2, "above")]


def _max_norm(regime, g, s):
    """None (no clip), 1 / 100 or 100 times the gradient norm; 1.0 over zero gradients."""
    if regime == "none":
        return None
    if regime == "zero_g":
        return 1.0
    return float(g.double().norm()) * (0.01 if regime == "above" else 100.0)


@functools.lru_cache(maxsize=1)
def _case_reference(n, s, step, regime):
    """The state and both references of one case, shared by the two entry points."""
    state = adam_state(n, s, step, seed=n % 1000 + 7, zero_g=regime == "zero_g")
    max_norm = _max_norm(regime, state[1], s)
    groups = [] if max_norm is None else [([0], max_norm)]
    return (state, max_norm, groups) + reference_step([state], step, groups)


def _one_case(api, n, s, step, regime):
    state, max_norm, groups, want, t32, coef = _case_reference(n, s, step, regime)
    if api == "multi":
        got = launch_multi([state], step, groups)[0]
    else:
        got = launch_step(state, step, max_norm)
    if regime in ("below", "zero_g"):
        assert coef[0].item() == 1.0
    if regime == "above":
        assert coef[0].item() < 0.011
    check_outputs(dict(test="adam", api=api, s=s, step=step, regime=regime), got, want[0], t32[0], state, coef[0], n)


@pytest.mark.parametrize("n", SMALL_N)
def test_adam_small_sizes_vs_fp64(n):
    """nr_adam_step / nr_adam_multi at 1 .. 1024 elements (scalar only, float4 + tail,
    float4 only; one block and more), every gradient scale, step number and clip regime."""
    for s in SCALES:
        for step in STEPS:
            for regime in REGIMES:
                for api in ("step", "multi"):
                    _one_case(api, n, s, step, regime)


@pytest.mark.parametrize("api", ["step", "multi"])
@pytest.mark.parametrize("s,step,regime", LARGE_COMBOS)
@pytest.mark.parametrize("n", LARGE_N)
def test_adam_grid_stride_vs_fp64(n, s, step, regime, api):
    """Exactly one grid pass, a second float4 trip, and n % 4 != 0 (adam_kernel: float4 and
    a wrapped scalar tail; adam_multi_kernel: the all-scalar form, four trips)."""
    _one_case(api, n, s, step, regime)


MULTI_N = [2097159, 1, 0, 30, 4, 1023, 3, 262148]
MULTI_GROUPS = [([0, 1, 2, 3], 1.0), ([4, 5, 6], 0.1)]


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_multi_eight_spans_two_clip_groups(step):
    """One launch of eight spans (the grid sized by the longest, one span empty), clip
    groups A (spans 0-3, max_norm 1.0) and B (spans 4-6, 0.1) and span 7 without a clip:
    every span is held to its own group's coefficient."""
    states = [adam_state(n, 1.0, step, seed=300 + 5 * k) for k, n in enumerate(MULTI_N)]
    want, t32, coef = reference_step(states, step, MULTI_GROUPS)
    got = launch_multi(states, step, MULTI_GROUPS)
    assert coef[0] is coef[3] and coef[4] is coef[6] and coef[7] is None
    assert coef[0].item() < 1e-3 and 1e-3 < coef[4].item() < 1e-2
    nsum = [sum(MULTI_N[:4])] * 4 + [sum(MULTI_N[4:7])] * 3 + [0]
    for k in range(len(states)):
        check_outputs(dict(test="adam_eight_spans", api="multi", step=step, span=k), got[k], want[k], t32[k],
                      states[k], coef[k], nsum[k])


@pytest.mark.parametrize("n", [30, 1023, 1024])
def test_adam_multi_device_schedule(n):
    """``sched``, the device pair a captured graph reads: holding fp32(adam_sched_values)
    of the host arguments' step the outputs are bit-equal to the host-scalar call; holding
    another step's pair while the host arguments say ``step``, they are the other step's."""
    from noisy_src import ops
    state = adam_state(n, 1.0, 1000, seed=400 + n)
    groups = [([0], 0.5)]

    def pair(step):
        return torch.tensor(ops.adam_sched_values(LR, B1, B2, step), dtype=torch.float32).to(DEV)

    host = {step: launch_multi([state], step, groups)[0] for step in (2, 1000)}
    assert not torch.equal(host[2]["p"], host[1000]["p"])
    same = launch_multi([state], 1000, groups, sched=pair(1000))[0]
    other = launch_multi([state], 2, groups, sched=pair(2), host_step=1000)[0]
    for k in "pgmv":
        assert torch.equal(same[k].view(torch.int32), host[1000][k].view(torch.int32)), k
        assert torch.equal(other[k].view(torch.int32), host[2][k].view(torch.int32)), k


# --------------------------------------------------------------------- NaN norm --
def test_nan_gradient_norm_poisons_its_clip_group_only():
    """One NaN gradient element in a clip group of two spans: as with torch
    (clamp(nan) = nan) every element of g, m, v and p of both spans is NaN afterwards, in
    nr_adam_multi and in nr_adam_step; a span outside the group is what it is alone."""
    states = [adam_state(n, 1.0, 1000, seed=500 + n) for n in (30, 5, 1023)]
    states[1][1][3] = float("nan")
    groups = [([0, 1], 1.0), ([2], 1.0)]
    _, t32, _ = reference_step(states, 1000, groups)
    got = launch_multi(states, 1000, groups)
    alone = launch_multi(states[2:], 1000, [([0], 1.0)])[0]
    for k in "pgmv":
        for i in (0, 1):
            assert bool(torch.isnan(t32[i][k]).all()), ("torch", i, k)
            assert bool(torch.isnan(got[i][k]).all()), (i, k)
        assert torch.equal(got[2][k].view(torch.int32), alone[k].view(torch.int32)), k
    single = launch_step(states[1], 1000, 1.0)
    assert all(bool(torch.isnan(single[k]).all()) for k in "pgmv")


# ------------------------------------------------- FusedAdam, the generic path --
def _fused_vs_torch(ps, ts, opt, topt, clip_at, steps=6, lr=1e-2):
    from test_fused_adam_host import _compare
    g = torch.Generator().manual_seed(11)
    scales = (1.0, 1e-3, 3e-2, 1.0, 10.0, 1e-2)
    for k in range(1, steps + 1):
        for p, t in zip(ps, ts):
            gr = torch.randn(t.shape, generator=g) * scales[k - 1]
            p.grad, t.grad = gr.to(DEV), gr.clone()
        clip = clip_at(k)
        opt.step(clip_groups=[([ps[i] for i in idxs], mn) for idxs, mn in clip])
        for idxs, mn in clip:
            torch.nn.utils.clip_grad_norm_([ts[i] for i in idxs], mn)
        topt.step()
        torch.cuda.synchronize()
        _compare(opt, topt, ps, ts, k)


def test_fused_adam_pose_shaped_parameters_on_device():
    """test_fused_adam_host's pose-shaped scenario on the kernels: separately allocated
    (10, 3), (10, 3), (1,), (2,) parameters (all-scalar spans) in two clip groups, 6 steps
    against torch.optim.Adam on CPU copies, under the host test's bound and step-counter
    assertions."""
    from noisy_src.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    ts = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(10, 3), (10, 3), (1,), (2,)]]
    ps = [torch.nn.Parameter(t.detach().to(DEV)) for t in ts]
    opt, topt = FusedAdam(ps, lr=1e-2), torch.optim.Adam(ts, lr=1e-2)
    _fused_vs_torch(ps, ts, opt, topt, lambda k: [([0, 1], 0.1), ([2, 3], 0.05)])


def test_fused_adam_split_and_rejoin_on_device():
    """Two views A, B of one device buffer: stepped jointly, A alone in a clip group at
    steps 2 and 4 (the run splits), jointly again; against torch.optim.Adam on CPU copies."""
    from noisy_src.optim import FusedAdam
    flat = torch.randn(20, generator=torch.Generator().manual_seed(5))
    dev = flat.to(DEV)
    ps = [torch.nn.Parameter(dev[:8].view(2, 4)), torch.nn.Parameter(dev[8:])]
    ts = [torch.nn.Parameter(flat[:8].clone().view(2, 4)), torch.nn.Parameter(flat[8:].clone())]
    opt, topt = FusedAdam(ps, lr=1e-2), torch.optim.Adam(ts, lr=1e-2)
    _fused_vs_torch(ps, ts, opt, topt, lambda k: [([0], 0.5)] if k in (2, 4) else ())
    assert len(opt._flat_state) == 1 and next(iter(opt._flat_state.values()))[0].numel() == 20
