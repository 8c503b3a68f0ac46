"""GPU: the robust photometric losses (nr_robust_fwd_bwd, nr_composite_robust,
ops.composite_loss, the trainers' ``loss`` / ``loss_scale``) against tests/robust_ref.py.

Parity bound of the seed entry.  The truth is robust_ref in fp64 on the kernel's own fp32
inputs; robust_ref in fp32 performs the kernel's operations in the kernel's documented order
(include/nerf_hip.h), so its distance from the truth, E32, is what that arithmetic costs.
The kernel is held to ``edge_inputs.yardstick_bound(4, E32, want)``: at most 4 x E32 (its sum
runs in another order, and its log1p may differ in the last place), with the floor of
4 x 2^-24 x max|want| for a restatement that happens to be exact.  With ``NR_WRITE_PROFILES``
set the errors and bounds go to profiles/robust_loss_parity.json.

Everything else is an identity (bit for bit) or borrows a bound that an existing test holds
the same quantity to: the loss words of the fused and the separate path 1e-6 relative
(test_composite_mse.py, another summation order), the op chain rtol 1e-3 / atol 1e-4
(test_parity_ops.py's composite backward), the trainers' flat gradients 1e-3 relative and the
translation gradient 2 x the fp32 oracle's own distance from fp64 + 1e-3 (test_distortion.py).
The oracle-only checks in front show that a dropped weight moves each compared gradient by
more than ten times its tolerance.
"""
import copy
import itertools
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
import robust_ref as R  # noqa: E402
from oracle import refimpl as ref  # noqa: E402
from test_distortion import (NC, NF, RAYS, _capture_grads, _flat_grad, _nets, _ray_batches, _rc, _rel,  # noqa: E402
                             _scene)
from test_edge_shapes import guarded, poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
F32, F64 = torch.float32, torch.float64
NR_EARG = -22
KIND = {k: i for i, k in enumerate(R.KINDS)}
_records = []


@pytest.fixture(scope="module", autouse=True)
def _write_profile():
    yield
    if os.environ.get("NR_WRITE_PROFILES") and _records:
        (ROOT / "profiles" / "robust_loss_parity.json").write_text(json.dumps(
            {"bound": "max(4 x fp32-vs-fp64 error of the restatement in the kernel's order, 4 x 2^-24 x max|want|)",
             "cases": _records}, indent=1) + "\n")


def _args(args):
    from noisy_src import _hip
    return [_hip.ptr(a) if isinstance(a, torch.Tensor) else a for a in args] + [_hip.stream_ptr()]


def _call(name, *args):
    from noisy_src import _hip
    _hip.call(name, *_args(args))


def _raw(name, *args):
    """The entry point's return code and message, without raising."""
    from noisy_src import _hip
    rc = getattr(_hip.load(), name)(*_args(args))
    return rc, _hip.last_error()


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# -------------------------------------------------------------- 1. the seed entry --
def _seed_run(pred, target, kind, c, scale=1.0, with_g=True, with_loss=True):
    B = pred.shape[0]
    loss2 = guarded((2,)) if with_loss else None
    g = guarded((B, 3)) if with_g else None
    _call("nr_robust_fwd_bwd", pred.to(DEV), target.to(DEV), B, KIND[kind], c, scale,
          None if loss2 is None else loss2.buf, None if g is None else g.buf)
    torch.cuda.synchronize()
    for o in (loss2, g):
        if o is not None:
            o.check()
    return (None if loss2 is None else loss2.out.cpu()), (None if g is None else g.out.cpu())


@pytest.mark.parametrize("B,equal", [(1, False), (5, False), (700, False), (5, True)])
@pytest.mark.parametrize("c", [0.02, 0.1, 2.0])
@pytest.mark.parametrize("kind", R.KINDS)
def test_seed_entry_vs_fp64(kind, c, B, equal):
    pred, target = R.inputs(B, equal=equal)
    scale = 0.5
    loss2, g = _seed_run(pred, target, kind, c, scale)
    want = dict(zip(("rho", "mse", "g_pred"), R.loss_and_grad(pred, target, kind, c, scale, F64)))
    o32 = dict(zip(("rho", "mse", "g_pred"), R.loss_and_grad(pred, target, kind, c, scale, F32)))
    got = {"rho": loss2[0], "mse": loss2[1], "g_pred": g}
    rec = dict(kind=kind, c=c, B=B, equal=equal)
    for k in want:
        err, e32 = ei.distance(k, got[k], want[k]), ei.distance(k, o32[k], want[k])
        bound = ei.yardstick_bound(4, e32, want[k])
        rec[k] = dict(err=err, e32=e32, bound=bound, scale=want[k].abs().max().item())
    _records.append(rec)
    print("ROBUST_PARITY " + json.dumps(rec))
    for k in want:
        assert torch.isfinite(got[k]).all(), k
        assert rec[k]["err"] <= rec[k]["bound"], (k, rec[k])
    if equal:
        assert all(int(torch.count_nonzero(got[k])) == 0 for k in got)
    # both outputs are nullable, and leaving one out changes nothing in the other
    l_only, _ = _seed_run(pred, target, kind, c, scale, with_g=False)
    _, g_only = _seed_run(pred, target, kind, c, scale, with_loss=False)
    assert _same(l_only, loss2) and _same(g_only, g)


# ------------------------------------------------------------ 2. exact identities --
@pytest.mark.parametrize("B", [1, 5, 700])
def test_huber_over_every_residual_is_the_mse_bit_for_bit(B):
    pred, target = R.inputs(B, seed=1)
    loss2, g = _seed_run(pred, target, "huber", 2.0, 0.5)
    loss, gm = guarded((1,)), guarded((B, 3))
    _call("nr_mse_fwd_bwd", pred.to(DEV), target.to(DEV), B, 0.5, loss.buf, gm.buf)
    torch.cuda.synchronize()
    assert _same(g, gm.out.cpu())
    assert _same(loss2[0:1], loss.out.cpu()) and _same(loss2[1:2], loss.out.cpu())
    m2, gk = _seed_run(pred, target, "mse", 0.1, 0.5)
    assert _same(gk, g) and _same(m2, loss2)


def _inputs(B, S, seed=0, zero_frac=0.3):
    """test_composite_mse.py's draw."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(B, S, 3, generator=g)
    sigma = torch.randn(B, S, generator=g) * 3
    sigma[torch.rand(B, S, generator=g) < zero_frac] = 0.0
    z = torch.sort(2 + 4 * torch.rand(B, S, generator=g), -1).values
    return dict(rgb=rgb, sigma=sigma, z=z, rd=torch.randn(B, 3, generator=g), noise=None,
                target=torch.rand(B, 3, generator=g), rd_init=torch.randn(B, 3, generator=g))


OUTS = ("rgb_map", "depth", "acc", "weights", "g_rgb", "g_sigma", "g_rays_d")


def _buffers(B, S, rd_init, with_rd=True, nloss=2, fill=None):
    """Guarded outputs; ``fill``: NaN instead of the finite pattern (g_rays_d is accumulated
    onto, so it starts from ``rd_init``)."""
    def buf(shape):
        full = (shape[0] + 1, *shape[1:])
        return guarded(shape, init=None if fill is None else torch.full(full, fill))
    o = dict(rgb_map=buf((B, 3)), depth=buf((B,)), acc=buf((B,)), weights=buf((B, S)), g_rgb=buf((B, S, 3)),
             g_sigma=buf((B, S)), loss=buf((nloss,)))
    o["g_rays_d"] = guarded((B, 3), init=torch.cat([rd_init, torch.full((1, 3), 7.5)])) if with_rd else None
    return o


def _front(dv):
    return dv["rgb"], dv["sigma"], dv["z"], dv["rd"], dv["noise"]


def _dev(c):
    return {k: (None if v is None else v.to(DEV)) for k, v in c.items()}


def _robust(dv, kind, c, white=1, scale=0.5, with_rd=True, ticket=None, ws=None, fill=None):
    """nr_composite_robust into guarded buffers -> {name: device tensor}."""
    from noisy_src import _hip
    B, S = dv["z"].shape
    o = _buffers(B, S, dv["rd_init"].cpu(), with_rd, 2, fill)
    if ws is None:
        ws = torch.empty(int(_hip.load().nr_composite_robust_workspace_bytes(B)), device=DEV, dtype=torch.uint8)
    _call("nr_composite_robust", *_front(dv), dv["target"], B, S, white, KIND[kind], c, scale, o["rgb_map"].buf,
          o["depth"].buf, o["acc"].buf, o["weights"].buf, o["loss"].buf, o["g_rgb"].buf, o["g_sigma"].buf,
          None if o["g_rays_d"] is None else o["g_rays_d"].buf, ticket, ws)
    torch.cuda.synchronize()
    if ticket is not None:
        assert int(torch.count_nonzero(ticket)) == 0
    return _checked(o)


def _checked(o):
    out = {}
    for k, v in o.items():
        if v is not None:
            v.check()
            out[k] = v.out
    return out


def _mse(dv, white=1, scale=0.5, with_rd=True, ticket=None):
    from noisy_src import _hip
    B, S = dv["z"].shape
    o = _buffers(B, S, dv["rd_init"].cpu(), with_rd, 1)
    ws = torch.empty(int(_hip.load().nr_composite_mse_workspace_bytes(B)), device=DEV, dtype=torch.uint8)
    _call("nr_composite_mse", *_front(dv), dv["target"], B, S, white, scale, o["rgb_map"].buf, o["depth"].buf,
          o["acc"].buf, o["weights"].buf, o["loss"].buf, o["g_rgb"].buf, o["g_sigma"].buf,
          None if o["g_rays_d"] is None else o["g_rays_d"].buf, ticket, ws)
    torch.cuda.synchronize()
    return _checked(o)


def _separate(dv, kind, c, white=1, scale=0.5, with_rd=True):
    """nr_composite_fwd -> nr_robust_fwd_bwd -> nr_composite_bwd."""
    B, S = dv["z"].shape
    o = _buffers(B, S, dv["rd_init"].cpu(), with_rd, 2)
    g_map = guarded((B, 3))
    _call("nr_composite_fwd", *_front(dv), B, S, white, o["rgb_map"].buf, o["depth"].buf, o["acc"].buf,
          o["weights"].buf)
    _call("nr_robust_fwd_bwd", o["rgb_map"].buf, dv["target"], B, KIND[kind], c, scale, o["loss"].buf, g_map.buf)
    _call("nr_composite_bwd", *_front(dv), B, S, white, g_map.buf, None, None, None, o["g_rgb"].buf, o["g_sigma"].buf,
          None if o["g_rays_d"] is None else o["g_rays_d"].buf)
    torch.cuda.synchronize()
    g_map.check()
    return _checked(o)


@pytest.mark.parametrize("ticket", [True, False], ids=["ticket", "second_launch"])
@pytest.mark.parametrize("S,B", [(65, 5), (192, 700), (64, 4096), (600, 5)])
def test_mse_kind_is_nr_composite_mse_bit_for_bit(S, B, ticket):
    dv = _dev(_inputs(B, S, seed=S + B))
    tk = torch.zeros(4, device=DEV, dtype=torch.int32) if ticket else None
    want = _mse(dv, ticket=tk)
    got = _robust(dv, "mse", 0.1, ticket=tk)
    for k in OUTS:
        assert _same(got[k], want[k]), k
    assert _same(got["loss"][0:1], got["loss"][1:2]) and _same(got["loss"][0:1], want["loss"])


@pytest.mark.parametrize("S", [65, 600])
def test_grad_scale_scales_only_the_gradients(S):
    dv = _dev(_inputs(5, S, seed=S))
    dv["rd_init"] = torch.zeros_like(dv["rd_init"])
    one, quarter = (_robust(dv, "cauchy", 0.1, scale=s) for s in (1.0, 0.25))
    for k in ("rgb_map", "depth", "acc", "weights", "loss"):
        assert _same(one[k], quarter[k]), k
    for k in ("g_rgb", "g_sigma", "g_rays_d"):
        assert one[k].abs().max() > 0 and _same(one[k] * 0.25, quarter[k]), k


# --------------------------------------------------------- 3. fused equals separate --
FUSED_S = [1, 2, 63, 64, 65, 130, 192, 512, 513, 600]
FUSED_B = [1, 3, 5, 700]


@pytest.mark.parametrize("B", FUSED_B)
@pytest.mark.parametrize("S", FUSED_S)
def test_fused_equals_separate(S, B):
    """Every combination of background, g_rays_d present / NULL, ticket present / NULL and
    input regime at this shape; the kind alternates between huber and cauchy below 513
    samples (the long form launches the separate kernels themselves: cauchy alone)."""
    tk = torch.zeros(4, device=DEV, dtype=torch.int32)
    n = 0
    for regime in ei.REGIMES:
        dv = _dev(ei.composite_inputs(S, B, regime))
        for white, with_rd, ticket in itertools.product((1, 0), (True, False), (True, False)):
            kind = "cauchy" if S > 512 or n % 2 else "huber"
            n += 1
            a = _separate(dv, kind, 0.1, white, with_rd=with_rd)
            f = _robust(dv, kind, 0.1, white, with_rd=with_rd, ticket=tk if ticket else None)
            tag = (regime, white, with_rd, ticket, kind)
            assert set(a) == set(f)
            for k in a:
                assert torch.isfinite(f[k]).all(), (k, tag)
                if k != "loss":
                    assert _same(a[k], f[k]), (k, tag)
            for la, lf in zip(a["loss"].tolist(), f["loss"].tolist()):
                assert abs(la - lf) <= 1e-6 * abs(la), (la, lf, tag)


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_fused_equals_separate_where_the_ticket_is_dropped(kind):
    dv = _dev(_inputs(4096, 64, seed=11))
    tk = torch.zeros(4, device=DEV, dtype=torch.int32)
    a = _separate(dv, kind, 0.1)
    f = _robust(dv, kind, 0.1, ticket=tk)
    for k in OUTS:
        assert _same(a[k], f[k]), k
    for la, lf in zip(a["loss"].tolist(), f["loss"].tolist()):
        assert abs(la - lf) <= 1e-6 * abs(la), (la, lf)
    assert f["loss"][0] != f["loss"][1]


# ------------------------------------------------------------------ 4. determinism --
@pytest.mark.parametrize("ticket", [True, False], ids=["ticket", "second_launch"])
@pytest.mark.parametrize("S,B", [(65, 5), (192, 700), (64, 4096), (600, 5)])
def test_bit_identical_runs_over_poisoned_scratch(S, B, ticket):
    from noisy_src import _hip
    dv = _dev(_inputs(B, S, seed=3 * S + B))
    tk = torch.zeros(4, device=DEV, dtype=torch.int32) if ticket else None
    runs = [_robust(dv, "geman_mcclure", 0.1, ticket=tk), _robust(dv, "geman_mcclure", 0.1, ticket=tk),
            _robust(dv, "geman_mcclure", 0.1, ticket=tk, fill=float("nan"),
                    ws=poisoned(_hip.load().nr_composite_robust_workspace_bytes(B)))]
    for k in runs[0]:
        assert torch.isfinite(runs[0][k]).all(), k
        assert _same(runs[0][k], runs[1][k]) and _same(runs[0][k], runs[2][k]), k


def test_workspace_bytes():
    from noisy_src import _hip
    f = _hip.load().nr_composite_robust_workspace_bytes
    assert [f(b) for b in (0, 1, 700, 4096)] == [0, 20, 14000, 81920]


# -------------------------------------------------------------- 5. argument errors --
def test_argument_errors():
    from noisy_src import _hip
    B, S = 5, 65
    dv = _dev(_inputs(B, S))
    o = _buffers(B, S, dv["rd_init"].cpu())
    ws = torch.empty(int(_hip.load().nr_composite_robust_workspace_bytes(B)), device=DEV, dtype=torch.uint8)
    g = guarded((B, 3))

    def fused(kind=3, c=0.1, loss=o["loss"].buf, workspace=ws, B=B, S=S, target=dv["target"]):
        return _raw("nr_composite_robust", *_front(dv), target, B, S, 1, kind, c, 1.0, o["rgb_map"].buf, o["depth"].buf,
                    o["acc"].buf, o["weights"].buf, loss, o["g_rgb"].buf, o["g_sigma"].buf, o["g_rays_d"].buf, None,
                    workspace)

    def seed(kind=3, c=0.1, pred=dv["target"], B=B):
        return _raw("nr_robust_fwd_bwd", pred, dv["target"], B, kind, c, 1.0, o["loss"].buf, g.buf)

    assert fused()[0] == 0 and seed()[0] == 0
    bad = [dict(kind=-1), dict(kind=5)] + [dict(c=c, kind=k) for c in (0.0, -1.0, float("nan"), float("inf"))
                                           for k in (0, 3)]
    for kw in bad + [dict(loss=None), dict(workspace=None), dict(B=0), dict(S=0), dict(target=None)]:
        rc, msg = fused(**kw)
        assert rc == NR_EARG and "nr_composite_robust" in msg, (kw, rc, msg)
    for kw in bad + [dict(pred=None), dict(B=0)]:
        rc, msg = seed(**kw)
        assert rc == NR_EARG and "nr_robust_fwd_bwd" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="nr_composite_robust"):
        from noisy_src import ops
        ops.composite_loss(dv["rgb"], dv["sigma"], dv["z"], dv["rd"], dv["target"], "cauchy", 0.0)


# ---------------------------------------------------- 6. the op chain vs the oracle --
def _close(x, y, rtol=1e-3, atol=1e-4):
    return torch.allclose(x.cpu(), y, rtol=rtol, atol=atol)


@pytest.mark.parametrize("B,S", [(300, 96), (5, 65)])
@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_op_chain_matches_the_oracle_with_extra_output_grads(kind, B, S):
    """``up``, the upstream gradient of the loss, puts the loss's share of every compared
    gradient (O(1 / B) per ray under a mean) above the comparison's atol of 1e-4, so the
    oracle-only check in front can hold; the depth and weight terms are test_composite_mse.py's."""
    from noisy_src import ops
    c, up = 0.1, {300: 75.0, 5: 3.0}[B]
    i = _inputs(B, S, seed=7)

    def oracle(k):
        a, s, d = (i[n].clone().requires_grad_(True) for n in ("rgb", "sigma", "rd"))
        out = ref.raw2outputs(a, s[..., None], i["z"], d)
        loss = R.loss(out["rgb_map"], i["target"], k, c)
        (up * loss + 0.1 * out["depth_map"].sum() + 0.01 * out["weights"].square().sum()).backward()
        return loss.detach(), out, a.grad, s.grad, d.grad

    want, plain = oracle(kind), oracle("mse")
    for x, y in zip(want[2:], plain[2:]):  # a dropped weight would show
        assert (x - y).abs().max() > 10 * (1e-3 * y.abs().max() + 1e-4)

    a, s, d = (i[n].to(DEV).requires_grad_(True) for n in ("rgb", "sigma", "rd"))
    loss, mse, rgb_map, depth, acc, w = ops.composite_loss(a, s, i["z"].to(DEV), d, i["target"].to(DEV), kind, c)
    assert not mse.requires_grad and loss.requires_grad
    (up * loss + 0.1 * depth.sum() + 0.01 * w.square().sum()).backward()
    assert abs(loss.item() - want[0].item()) < 1e-6
    assert abs(mse.item() - ((want[1]["rgb_map"] - i["target"]) ** 2).mean().item()) < 1e-6
    assert (rgb_map.cpu() - want[1]["rgb_map"]).abs().max() < 1e-5
    for name, x, y in (("rgb", a.grad, want[2]), ("sigma", s.grad, want[3]), ("rays_d", d.grad, want[4])):
        assert _close(x, y), (name, (x.cpu() - y).abs().max().item())
    # ops.robust_loss on the separate composite is the same loss and gradient
    a2, s2 = (i[n].to(DEV).requires_grad_(True) for n in ("rgb", "sigma"))
    l2 = ops.robust_loss(ops.composite(a2, s2, i["z"].to(DEV), i["rd"].to(DEV))[0], i["target"].to(DEV), kind, c)
    l2.backward()
    a3, s3 = (i[n].to(DEV).requires_grad_(True) for n in ("rgb", "sigma"))
    ops.composite_loss(a3, s3, i["z"].to(DEV), i["rd"].to(DEV), i["target"].to(DEV), kind, c)[0].backward()
    assert abs(l2.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert _same(a2.grad, a3.grad) and _same(s2.grad, s3.grad)


@pytest.mark.parametrize("path", ["composite_mse", "composite_loss_mse", "composite_loss_huber"])
@pytest.mark.parametrize("B,S", [(5, 65), (3, 600)], ids=["wave_per_ray", "three_pass"])
def test_fused_backward_is_exact_in_its_seed_and_its_extra_output_grads(B, S, path):
    """The one backward behind ops.composite_mse and ops.composite_loss, pinned by exact
    relations (no tolerance): (a) a fresh seed tensor 0.5 gives 0.5 x the gradients of the
    unit_grad() seed, bit for bit (a power of two: the products are exact); (b) with the
    loss unused, gradients arriving at rgb_map / depth / weights alone give ops.composite's
    backward of the same inputs; (c) both in one backward give the elementwise fp32 sum."""
    from noisy_src import ops
    dv = {k: (None if v is None else v.to(DEV)) for k, v in ei.composite_inputs(S, B, "random").items()}
    ups = (dv["g_map"], dv["g_depth"], dv["g_w"])

    def run(fused, seed, with_ups):
        leaves = [dv[n].clone().requires_grad_(True) for n in ("rgb", "sigma", "rd")]
        if not fused:
            out = ops.composite(leaves[0], leaves[1], dv["z"], leaves[2], noise=dv["noise"])
        elif path == "composite_mse":
            out = ops.composite_mse(leaves[0], leaves[1], dv["z"], leaves[2], dv["target"], noise=dv["noise"])
        else:
            out = ops.composite_loss(leaves[0], leaves[1], dv["z"], leaves[2], dv["target"], path.rsplit("_", 1)[1],
                                     0.1, noise=dv["noise"])
        rgb_map, depth, _, w = out[-4:]
        outs, gos = ([out[0]], [seed]) if seed is not None else ([], [])
        if with_ups:
            outs, gos = outs + [rgb_map, depth, w], gos + list(ups)
        return torch.autograd.grad(outs, leaves, grad_outputs=gos)

    unit = run(True, ops.unit_grad(dv["z"].device), False)
    assert all(g.abs().max() > 0 for g in unit)
    half = run(True, torch.full((), 0.5, device=DEV), False)
    extra = run(True, None, True)
    both = run(True, ops.unit_grad(dv["z"].device), True)
    plain = run(False, None, True)
    for name, u, h, e, b, p in zip(("rgb", "sigma", "rays_d"), unit, half, extra, both, plain):
        assert torch.equal(h, 0.5 * u), ("a", name)
        assert torch.equal(e, p), ("b", name)
        assert torch.equal(b, u + e), ("c", name)


# ---------------------------------------------------------------------- 7. trainers --
C = 0.1


def _oracle_loss(oc, of, o, d, tgt, tr, u, kind, c=C, weight=0.0, dtype=F32):
    import distortion_ref
    rc = _rc()
    out, aux = ref.render_rays(oc, of, o.to(dtype), d.to(dtype), rc, is_train=True, t_rand=tr.to(dtype), u=u.to(dtype),
                               return_aux=True)
    t = tgt.to(dtype)
    loss = R.loss(out["rgb_coarse"], t, kind, c) + R.loss(out["rgb_fine"], t, kind, c)
    if weight > 0:
        dist = distortion_ref.loss_rays_prefix(aux["weights_fine"], aux["z_fine"].detach(), rc.near, rc.far, F64).mean()
        loss = loss + weight * dist.to(dtype)
    return loss, out


@pytest.mark.parametrize("coarse_stream", [False, True])
def test_trainer_step_gradients_match_the_oracle_plus_the_restated_loss(coarse_stream):
    from noisy_src.engine import Trainer
    b = _ray_batches(1)[0]
    want = {}
    for kind in ("mse", "cauchy"):
        oc, of, _, _ = _nets()
        loss, out = _oracle_loss(oc, of, *b, kind)
        loss.backward()
        want[kind] = (_flat_grad(oc), _flat_grad(of), float(loss.detach()))
    for k in (0, 1):  # both networks see the kernel, far above the tolerance
        assert _rel(want["cauchy"][k], want["mse"][k]) > 10 * 1e-3
    _, _, mc, mf = _nets()
    tr = Trainer(mc, mf, _rc(), coarse_stream=coarse_stream, loss="cauchy", loss_scale=C)
    grads = []
    _capture_grads(tr.optimizer, (mc, mf), grads)
    m = tr.step(*b)
    assert tr.last_step_coarse_stream == coarse_stream
    assert _rel(grads[0], want["cauchy"][0]) < 1e-3 and _rel(grads[1], want["cauchy"][1]) < 1e-3
    assert abs(float(m["loss"]) - want["cauchy"][2]) < 1e-5 * want["cauchy"][2]
    assert torch.equal(m["loss"], m["loss_coarse"] + m["loss_fine"])
    mse_fine = ((m["rgb_fine"].double() - b[2].double()) ** 2).mean().item()
    assert abs(float(m["mse_fine"]) - mse_fine) <= 1e-6 * mse_fine
    assert float(m["mse_coarse"]) > float(m["loss_coarse"]) > 0 and float(m["mse_fine"]) > float(m["loss_fine"]) > 0


def test_trainer_with_mse_is_the_trainer_without_the_keyword():
    from noisy_src.engine import Trainer
    trainers = []
    for kw in ({}, {"loss": "mse", "loss_scale": 0.3}):
        _, _, mc, mf = _nets("bf16", seed=17)
        trainers.append(Trainer(mc, mf, _rc(), **kw))
    for b in _ray_batches(2):
        ms = [t.step(*b) for t in trainers]
        assert set(ms[0]) == set(ms[1]) and not any(k.startswith("mse_") for k in ms[1])
        assert torch.equal(ms[0]["loss"], ms[1]["loss"])
    for net in ("model_coarse", "model_fine"):
        assert torch.equal(getattr(trainers[0], net).flat_params(), getattr(trainers[1], net).flat_params())


def test_trainer_with_huber_and_the_distortion_term_matches_the_oracle():
    from noisy_src.engine import Trainer
    b = _ray_batches(1)[0]
    oc, of, mc, mf = _nets()
    loss, _ = _oracle_loss(oc, of, *b, "huber", weight=0.01)
    loss.backward()
    tr = Trainer(mc, mf, _rc(), loss="huber", loss_scale=C, distortion_weight=0.01)
    grads = []
    _capture_grads(tr.optimizer, (mc, mf), grads)
    m = tr.step(*b)
    assert _rel(grads[0], _flat_grad(oc)) < 1e-3 and _rel(grads[1], _flat_grad(of)) < 1e-3
    assert abs(float(m["loss"]) - float(loss)) < 1e-5 * float(loss)
    assert float(m["loss_distortion"]) > 0 and "mse_fine" in m


def _pose_setup():
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    fix = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    init = torch.from_numpy(fix["initial_poses"])[:3]
    data = synthetic_blender_data(torch.from_numpy(fix["ground_truth_poses"])[:3], H=16, W=16, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=RAYS)
    g = torch.Generator().manual_seed(6)
    tr_, u = torch.rand(RAYS, NC, generator=g).to(DEV), torch.rand(RAYS, NF, generator=g).to(DEV)
    return init, data, sampler, tr_, u


def test_pose_trainer_step_gradients_match_the_oracle_plus_the_restated_loss():
    from noisy_src.engine import PoseTrainer
    from noisy_src.train_pose_opt import CameraPoseParameters
    init, data, sampler, tr_, u = _pose_setup()
    batch = sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(5))

    def oracle(kind, dtype=F32):
        oc, of, _, _ = _nets()
        oc, of = copy.deepcopy(oc).to(dtype), copy.deepcopy(of).to(dtype)
        cam = ref.CameraPoseParameters(init.to(DEV, dtype)).to(dtype)
        ro, rd = ref.get_rays_from_pixels(batch.image_indices, batch.pixel_coords.to(dtype), cam.get_all_poses(),
                                          16, 16, data.focal)
        loss, _ = _oracle_loss(oc, of, ro, rd, batch.target_rgb, tr_, u, kind, dtype=dtype)
        loss = loss + 0.01 * torch.mean(cam.rotation_deltas ** 2) + 0.001 * torch.mean(cam.translation_deltas ** 2)
        loss.backward()
        return _flat_grad(oc), _flat_grad(of), cam.translation_deltas.grad, cam.rotation_deltas.grad, float(loss)

    want, plain, truth = oracle("cauchy"), oracle("mse"), oracle("cauchy", F64)
    t_tol = 2 * _rel(want[2], truth[2]) + 1e-3
    assert _rel(want[0], plain[0]) > 10 * 1e-3 and _rel(want[1], plain[1]) > 10 * 1e-3
    assert _rel(want[2], plain[2]) > 10 * t_tol

    _, _, mc, mf = _nets()
    cam = CameraPoseParameters(init.to(DEV))
    tr = PoseTrainer(mc, mf, cam, sampler, _rc(), loss="cauchy", loss_scale=C)
    grads = []
    orig = tr.optimizer_poses.step

    def pose_step(*a, **k):
        grads.extend([cam.translation_deltas.grad.clone(), cam.rotation_deltas.grad.clone()])
        return orig(*a, **k)

    tr.optimizer_poses.step = pose_step
    _capture_grads(tr.optimizer_nerf, (mc, mf), grads)
    m = tr.step(batch, optimize_poses=True, t_rand=tr_, u=u)
    gc, gf, gt, gr = grads
    assert _rel(gc, want[0]) < 1e-3 and _rel(gf, want[1]) < 1e-3
    assert abs(float(m["loss"]) - want[4]) < 1e-5 * want[4]
    assert int(torch.count_nonzero(gr)) == 0 and int(torch.count_nonzero(want[3])) == 0
    assert _rel(gt, truth[2]) < t_tol
    mse_fine = ((m["rgb_fine"].double() - batch.target_rgb.double()) ** 2).mean().item()
    assert abs(float(m["mse_fine"]) - mse_fine) <= 1e-6 * mse_fine and "mse_coarse" in m


# ----------------------------------------------------------------------- 8. refiner --
def test_refiner_with_huber_over_every_residual_is_the_default_refiner():
    from noisy_src.engine import PoseRefiner
    from noisy_src.train_pose_opt import CameraPoseParameters
    init, data, sampler, tr_, u = _pose_setup()
    batches = [sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(s)) for s in (5, 6)]
    final = {}
    for name, kw in (("default", {}), ("huber2", dict(loss="huber", loss_scale=2.0)),
                     ("huber005", dict(loss="huber", loss_scale=0.05))):
        _, _, mc, mf = _nets()
        cam = CameraPoseParameters(init.to(DEV), fixed_small_angle=True).to(DEV)
        with PoseRefiner(mc, mf, cam, sampler, _rc(), **kw) as refiner:
            for b in batches:
                m = refiner.step(b, t_rand=tr_, u=u)
        assert ("mse_fine" in m) == bool(kw)
        final[name] = torch.cat([cam.rotation_deltas.detach().reshape(-1), cam.translation_deltas.detach().reshape(-1)])
    assert final["default"].abs().max() > 0
    assert _same(final["default"], final["huber2"])
    assert not torch.equal(final["default"], final["huber005"])


# ------------------------------------------------------------------------- 9. graph --
def test_graphed_trainer_with_cauchy_equals_eager(tmp_path):
    """A fresh child (tests/robust_loss_graph_worker.py): three replays against three eager
    steps, losses, mse_* and parameters bit for bit."""
    subprocess.run([sys.executable, str(ROOT / "tests" / "robust_loss_graph_worker.py"), str(tmp_path)], check=True,
                   timeout=300)
    r = json.loads((tmp_path / "robust_loss_graph_report.json").read_text())
    assert r["replays"] == 3 and r["two_branch_capture"], r
    assert r["losses_equal"] and r["params_equal"] and r["robust_differs_from_mse"], r


# --------------------------------------------------------------------------- 10. CLI --
@pytest.mark.parametrize("module", ["train", "train_pose_opt"])
def test_cli_flags_reach_the_step_the_saved_arguments_the_psnr_and_the_console(module, tmp_path, capsys, monkeypatch):
    import importlib

    from noisy_src import run
    layout = json.loads((GOLDEN / "reference_artifacts.json").read_text())["layout"]
    _scene(tmp_path / "data")
    seen = []
    orig = run.IterationLog._write

    def spy(self, done):
        if done is not None:
            seen.append(dict(zip(done[1][1], done[0]), iteration=done[1][0]))
        return orig(self, done)

    monkeypatch.setattr(run.IterationLog, "_write", spy)
    pose = module == "train_pose_opt"
    extra = ["--pose_opt_delay", "1", "--rotation_noise", "5", "--noise_seed", "42"] if pose else []
    importlib.import_module("noisy_src." + module).main(
        ["--data_root", str(tmp_path / "data"), "--img_scale", "1.0", "--batch_size", "64", "--num_iters", "3",
         "--log_every", "1", "--num_samples", "8", "--num_samples_fine", "16", "--precision", "bf16",
         "--output_dir", str(tmp_path / "out"), "--loss", "cauchy", "--loss_scale", "0.1"] + extra)
    (run_dir,) = (tmp_path / "out").iterdir()
    cfg = json.loads((run_dir / "experiment_config.json").read_text())
    assert cfg["loss"] == "cauchy" and cfg["loss_scale"] == 0.1
    rows = (run_dir / "logs" / "train_metrics.csv").read_text().splitlines()
    assert rows[0] == layout["pose_opt" if pose else "train"]["csv_headers"]["train_metrics.csv"]
    cols = rows[0].split(",")
    assert len(rows) == 4 and len(seen) == 3
    for line, vm in zip(rows[1:], seen):
        row = dict(zip(cols, line.split(",")))
        assert int(row["iteration"]) == vm["iteration"]
        assert float(row["psnr"]) == -10.0 * math.log10(vm["mse_fine"])
        assert float(row["loss_fine"]) == vm["loss_fine"] and float(row["loss"]) == vm["loss"]
        assert 0 < vm["loss_fine"] < vm["mse_fine"] and 0 < vm["loss_coarse"] < vm["mse_coarse"]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "loss:" in ln]
    assert len(lines) == 3 and all("| cauchy(c=0.1) | " in ln for ln in lines), lines
