"""CPU: adam_ref (the oracle of the optimizer-tail tests) against torch itself.

The restatement runs in float64 next to ``torch.nn.utils.clip_grad_norm_`` +
``torch.optim.Adam`` on float64 parameters whose Adam state (step, exp_avg, exp_avg_sq) is
injected through ``opt.state``.  Three consecutive steps, neither side re-synchronised
after the injection, agree to within 8 fp64 ulps per element, in two parts that between
them cover every operation of the restatement:

  the step  ``adam_step`` given the coefficient torch applied (recomputed bit for bit from
            the norm ``clip_grad_norm_`` returns, by torch's own three operations): every
            element of p, exp_avg, exp_avg_sq and the clipped gradient within 8 ulps
  the clip  ``clip_coef`` from the fp64 sum of squares within 8 ulps of that coefficient
            (torch takes the norm of the tensors' norms, another association of one sum)

Run with its own coefficient, the restatement keeps p, exp_avg_sq and the gradient within
the same 8 ulps of their elements.  exp_avg is a difference, ``m + 0.1 (g - m)``: a 1-ulp
change of the coefficient moves an element that cancels by more ulps of the *result* than
it has of the operands (25 were seen), so there it is held to 8 ulps of its largest operand."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adam_ref  # noqa: E402

F64 = torch.float64
ULPS = 8


def _ulp(x):
    """The spacing of float64 at |x| (at least that of the smallest normal)."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs().clamp_min(2.0 ** -1022)).exponent - 53)


def _assert_ulps(got, want, what, scale=None):
    d = ((got - want).abs() / _ulp(want if scale is None else scale)).max().item()
    assert d <= ULPS, (what, d)


@pytest.mark.parametrize("own_coef", [False, True], ids=["torch_coef", "own_coef"])
@pytest.mark.parametrize("rel_norm", [None, 0.1, 1e6], ids=["no_clip", "clipped", "clip_inactive"])
@pytest.mark.parametrize("step0", [0, 1, 999])
@pytest.mark.parametrize("scale", [1e-6, 1.0, 1e3])
def test_adam_ref_matches_torch_in_fp64(scale, step0, rel_norm, own_coef):
    max_norm = None if rel_norm is None else rel_norm * scale  # below / far above the norm of 54 draws
    g = torch.Generator().manual_seed(int(step0) + 7)
    shapes = [(10, 3), (7,), (1,), (4, 4)]
    lr = 5e-4
    ps = [torch.randn(s, generator=g, dtype=F64) for s in shapes]
    ms = [(0.1 * torch.randn(s, generator=g, dtype=F64) if step0 else torch.zeros(s, dtype=F64)) for s in shapes]
    vs = [(torch.rand(s, generator=g, dtype=F64) * scale ** 2 if step0 else torch.zeros(s, dtype=F64)) for s in shapes]
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.Adam(tp, lr=lr)
    if step0:
        for p, m, v in zip(tp, ms, vs):
            opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    p_, m_, v_ = [torch.cat([t.reshape(-1) for t in ts]).clone() for ts in (ps, ms, vs)]
    for k in range(1, 4):
        grads = [torch.randn(s, generator=g, dtype=F64) * scale for s in shapes]
        for p, gr in zip(tp, grads):
            p.grad = gr.clone()
        g_ = torch.cat([gr.reshape(-1) for gr in grads])
        m_old, g_raw = m_.clone(), g_.clone()
        coef = None
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
            applied = torch.clamp(max_norm / (total + 1e-6), max=1.0)  # clip_grad_norm_'s own operations
            coef = adam_ref.clip_coef((g_ * g_).sum(), max_norm)
            assert coef.dtype == F64 and bool(coef < 1) == (rel_norm == 0.1)
            _assert_ulps(coef, applied, ("coef", k))
            if not own_coef:
                coef = applied
        opt.step()
        adam_ref.adam_step(p_, g_, m_, v_, step0 + k, lr, coef=coef)
        assert all(int(opt.state[p]["step"]) == step0 + k for p in tp)
        _assert_ulps(p_, torch.cat([p.detach().reshape(-1) for p in tp]), ("p", k))
        _assert_ulps(g_, torch.cat([p.grad.reshape(-1) for p in tp]), ("g", k))
        _assert_ulps(v_, torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in tp]), ("v", k))
        want_m = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in tp])
        if own_coef:
            operand = torch.maximum(want_m.abs(), torch.maximum(m_old.abs(), 0.1 * g_raw.abs()))
            _assert_ulps(m_, want_m, ("m", k), scale=operand)
        else:
            _assert_ulps(m_, want_m, ("m", k))


def test_clip_coef_edges():
    """Exactly 1 below the norm, NaN for a NaN norm, 0 for an infinite one, and the dtype
    of its argument."""
    assert adam_ref.clip_coef(torch.tensor(0.0), 1.0).item() == 1.0
    assert adam_ref.clip_coef(torch.tensor(0.25), 1.0).item() == 1.0
    assert torch.isnan(adam_ref.clip_coef(torch.tensor(float("nan")), 1.0))
    assert adam_ref.clip_coef(torch.tensor(float("inf")), 1.0).item() == 0.0
    c = adam_ref.clip_coef(torch.tensor(4.0, dtype=torch.float32), 1.0)
    assert c.dtype == torch.float32 and abs(c.item() - 1.0 / (2.0 + 1e-6)) <= 2.0 ** -24
    assert adam_ref.clip_coef(4.0, 1.0).dtype == F64
