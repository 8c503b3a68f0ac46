"""GPU: the identities between the compositing entry points that their shared per-ray body
(composite.hip) guarantees and that no other test reaches.  test_edge_shapes and
test_composite_mse compare nr_composite_mse with the three separate launches only on a white
background and with every output present.  Here, at S = 1, 65 (K = 2), 512 (K = 8) and 513 (the
long form) and B = 5 (a full workgroup and one with three dead waves), through the guarded
buffers of test_edge_shapes, in the three input regimes of edge_inputs:

  * white = 0: nr_composite_mse == nr_composite_fwd -> nr_mse_fwd_bwd -> nr_composite_bwd, bit
    for bit, in every output but the loss (the same mean summed in another order: 1e-6
    relative, the bound of test_composite_mse_equals_separate);
  * depth / acc / weights NULL: the same rgb_map, g_rgb and g_sigma as with them present;
  * g_rays_d NULL: the same g_rgb and g_sigma, with the ticket and without.

Every expectation is exact (torch.equal): the values are the same expressions of the same
inputs, so there is no tolerance to derive."""
import functools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
from test_edge_shapes import _call, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FOLD_S = [1, 65, 512, 513]
B = 5
SCALE = 0.5


def _front(c):
    return [None if c[k] is None else c[k].to(DEV) for k in ("rgb", "sigma", "z", "rd", "noise")]


def _rd_init(c):
    return torch.cat([c["rd_init"], torch.full((1, 3), 7.5)])


def _finish(o, ticket=None):
    torch.cuda.synchronize()
    for k, v in o.items():
        v.check()
        assert torch.isfinite(v.out).all(), k
    if ticket is not None:
        assert torch.count_nonzero(ticket) == 0
    return {k: v.out.cpu() for k, v in o.items()}


def _fused(S, regime, white, outs, with_rd, ticket):
    """nr_composite_mse into guarded buffers; absent outputs are NULL and left out."""
    from noisy_src import _hip
    c = ei.composite_inputs(S, B, regime)
    o = dict(rgb_map=guarded((B, 3)), loss=guarded((1,)), g_rgb=guarded((B, S, 3)), g_sigma=guarded((B, S)))
    if outs:
        o.update(depth=guarded((B,)), acc=guarded((B,)), weights=guarded((B, S)))
    if with_rd:
        o["g_rays_d"] = guarded((B, 3), init=_rd_init(c))
    tk = torch.zeros(4, device=DEV, dtype=torch.int32) if ticket else None
    ws = torch.empty(int(_hip.load().nr_composite_mse_workspace_bytes(B)), device=DEV, dtype=torch.uint8)

    def buf(k):
        return o[k].buf if k in o else None

    _call("nr_composite_mse", *_front(c), c["target"].to(DEV), B, S, white, SCALE, buf("rgb_map"), buf("depth"),
          buf("acc"), buf("weights"), buf("loss"), buf("g_rgb"), buf("g_sigma"), buf("g_rays_d"), tk, ws)
    return _finish(o, tk)


@functools.lru_cache(maxsize=None)
def _fused_full(S, regime, white, ticket):
    """Every output present: the reference of the NULL-output tests (read, never changed)."""
    return _fused(S, regime, white, True, True, ticket)


@pytest.mark.parametrize("ticket", [True, False], ids=["ticket", "second_launch"])
@pytest.mark.parametrize("regime", ei.REGIMES)
@pytest.mark.parametrize("S", FOLD_S)
def test_fused_equals_separate_black_background(S, regime, ticket):
    c = ei.composite_inputs(S, B, regime)
    front, target = _front(c), c["target"].to(DEV)
    a = dict(rgb_map=guarded((B, 3)), depth=guarded((B,)), acc=guarded((B,)), weights=guarded((B, S)),
             g_rgb=guarded((B, S, 3)), g_sigma=guarded((B, S)), g_rays_d=guarded((B, 3), init=_rd_init(c)),
             loss=guarded((1,)), g_map=guarded((B, 3)))
    _call("nr_composite_fwd", *front, B, S, 0, a["rgb_map"].buf, a["depth"].buf, a["acc"].buf, a["weights"].buf)
    _call("nr_mse_fwd_bwd", a["rgb_map"].buf, target, B, SCALE, a["loss"].buf, a["g_map"].buf)
    _call("nr_composite_bwd", *front, B, S, 0, a["g_map"].buf, None, None, None, a["g_rgb"].buf, a["g_sigma"].buf,
          a["g_rays_d"].buf)
    sep = _finish(a)
    fused = _fused_full(S, regime, 0, ticket)
    assert set(fused) == set(sep) - {"g_map"}
    for k in fused:
        if k != "loss":
            assert torch.equal(sep[k], fused[k]), k
    ls, lf = sep["loss"].item(), fused["loss"].item()
    print(f"COMPOSITE_FOLD S={S} {regime} ticket={ticket} loss separate={ls!r} fused={lf!r}")
    assert abs(ls - lf) <= 1e-6 * abs(ls), (ls, lf)


@pytest.mark.parametrize("white", [0, 1], ids=["black", "white"])
@pytest.mark.parametrize("regime", ei.REGIMES)
@pytest.mark.parametrize("S", FOLD_S)
def test_fused_null_maps_write_the_same(S, regime, white):
    full = _fused_full(S, regime, white, True)
    got = _fused(S, regime, white, False, True, True)
    for k in ("rgb_map", "g_rgb", "g_sigma"):
        assert torch.equal(got[k], full[k]), k


@pytest.mark.parametrize("ticket", [True, False], ids=["ticket", "second_launch"])
@pytest.mark.parametrize("regime", ei.REGIMES)
@pytest.mark.parametrize("S", FOLD_S)
def test_fused_null_g_rays_d_writes_the_same(S, regime, ticket):
    full = _fused_full(S, regime, 0, ticket)
    got = _fused(S, regime, 0, True, False, ticket)
    for k in ("g_rgb", "g_sigma"):
        assert torch.equal(got[k], full[k]), k
