"""GPU: the fused MLP at ragged and tiny M, and every entry point on scratch the caller did
not initialise.

The MLP kernels work on 32-sample tiles, so a last tile is padded: its extra rows run on
zero inputs in the forward, carry dz == 0 through the backward and are summed, as exact
zeros, by the dW GEMM.  The parity tests hold the 16-bit paths to 1e-2 relative at M in the
thousands, where a few wrong padded rows would vanish, and ``saved`` / ``workspace`` always
come from ``torch.empty``.  Here the four entry points the autograd function calls
(nr_mlp_forward, nr_mlp_backward_dx, _dw, _reduce) run directly on buffers the test owns:

* the results of M samples must not depend, to the bit, on what lies in ``saved`` and
  ``workspace`` before the call (zeros vs 0xFF bytes: NaN in every float format, a huge
  value as an index), on what lies in the input buffers after row M (zeros vs NaN), nor on
  whether the padding rows hold nothing or other samples with a zero upstream gradient;
  nothing is written after row M of an output;
* at M = 1, 31, 33, 513 the gradients are those of the reference: fp64 autograd for fp32,
  the numerics model (refimpl.mfma_emulated_nerf) for bf16 / fp16, on inputs constructed
  free of ReLU kinks (edge_inputs.mlp_selected), under the bounds of test_parity_mlp;
* the 16-bit forward at scene scale, |x| in 4 .. 8 (more than 600 revolutions at 2^9 x).

The same zero-vs-0xFF comparison covers the other entry points whose workspace has no
zeroing contract: nr_get_rays_bwd, nr_sumsq, nr_sumsq_partials, nr_composite_mse,
nr_image_metrics, nr_depth_frame_u8.  Reading them (csrc/) shows every workspace field
written before it is read -- tile flags and block counts by tile_flags_kernel over whole
segments, the dW list and its count by the dX launch's segment leaders, every slab entry the
reduction reads by the dW workgroup of its chunk, one partial per workgroup of a fixed grid
elsewhere -- and these tests hold the code to that.

Distances are printed as ``EDGE_PARITY`` lines (profiles/edge_shapes_parity.json)."""
import copy
import ctypes
import functools
import sys
from pathlib import Path

import pytest
import torch

from oracle import refimpl as ref

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
from test_edge_shapes import _call, _record, guarded, poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
GUARD = 33  # sentinel rows behind every per-sample output: more than a tile


@functools.lru_cache(maxsize=None)
def _net(precision, case=None):
    """(oracle, HIP network with the oracle's weights, its packed weight images); ``case``
    names a config of edge_inputs.CONFIG_CASES, None is the default model."""
    from noisy_src.model import NeRF
    oracle = ei.oracle_net(precision, case=case)
    net = NeRF(ei.case_config(precision, case))
    net.load_state_dict(oracle.state_dict())
    net = net.to(DEV)
    net._ensure_flat()
    return oracle, net, net._packed_for_forward()


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def mlp_raw(precision, M, x, d, g_rgb, g_sigma, *, rgb, sigma, saved, workspace, g_x, g_d, g_params, dense,
            case=None, read_count=True):
    """The forward and the split backward on caller-supplied buffers, as
    noisy_src.model._MLPFunction runs them.  Returns the active-tile count the dX launch
    left in the workspace (``read_count=False``: launches only, nothing read back)."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    _, net, packed = _net(precision, case)
    cfg = _hip.NrMlpConfig.from_buffer_copy(net._nr_cfg)
    cfg.dense_backward = int(dense)
    c, st, flat = ctypes.byref(cfg), _hip.stream_ptr(), net._flat
    call("nr_mlp_forward", c, ptr(packed), ptr(flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(saved), st)
    if g_params is None:
        return None
    call("nr_mlp_backward_dx", c, ptr(packed), ptr(flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(saved),
         ptr(g_rgb), ptr(g_sigma), ptr(g_x), ptr(g_d), ptr(workspace), st)
    call("nr_mlp_backward_dw", c, M, ptr(saved), ptr(workspace), st)
    call("nr_mlp_backward_reduce", c, M, ptr(workspace), ptr(g_params), st)
    return active_tile_count(precision, M, workspace, case) if read_count else None


def active_tile_count(precision, M, workspace, case=None):
    """The active-tile count the last dX launch left in ``workspace`` (a read-back)."""
    from noisy_src import _hip
    off = int(_hip.load().nr_mlp_active_tiles_offset(ctypes.byref(_net(precision, case)[1]._nr_cfg), M))
    return int(workspace[off:off + 4].view(torch.int32).item())


def _padded(t, M, width, tail):
    """The first M rows of ``t`` in a buffer of whole tiles, ``tail`` behind row M."""
    buf = torch.full(((M + 31) // 32 * 32, width), tail)
    buf[:M] = t[:M].reshape(M, width)
    return buf.to(DEV)


def _buffers(precision, M, *, poison=False, want_in=True, case=None):
    """saved, workspace (zeros, or 0xFF bytes with ``poison``) and the outputs of M samples
    with GUARD sentinel rows.  A config without view directions has no g_d."""
    from noisy_src import _hip
    _, net, _ = _net(precision, case)
    cfg = ctypes.byref(net._nr_cfg)
    fill = poisoned if poison else (lambda n: torch.zeros(int(n), dtype=torch.uint8, device=DEV))
    o = dict(rgb=guarded((M, 3), GUARD), sigma=guarded((M,), GUARD), g_params=guarded((net._param_count,), 64))
    if want_in:
        o.update(g_x=guarded((M, 3), GUARD))
        if net.config.use_view_dirs:
            o.update(g_d=guarded((M, 3), GUARD))
    return dict(saved=fill(_hip.load().nr_mlp_saved_bytes(cfg, M)), ws=fill(_hip.load().nr_mlp_workspace_bytes(cfg, M)),
                out=o)


def _run_on(bufs, precision, M, x, d, g_rgb, g_sigma, *, tail=0.0, dense=1, case=None):
    """One forward + backward of the first M rows of the inputs on the buffers of
    ``_buffers``, as they are: nothing is refilled, so a second run sees what the first left
    in saved, workspace and the outputs.  The input buffers are padded to whole tiles with
    ``tail`` behind row M."""
    o = bufs["out"]
    count = mlp_raw(precision, M, _padded(x, M, 3, tail), _padded(d, M, 3, tail), _padded(g_rgb, M, 3, tail),
                    _padded(g_sigma, M, 1, tail), rgb=o["rgb"].buf, sigma=o["sigma"].buf, saved=bufs["saved"],
                    workspace=bufs["ws"], g_x=o["g_x"].buf if "g_x" in o else None,
                    g_d=o["g_d"].buf if "g_d" in o else None, g_params=o["g_params"].buf, dense=dense, case=case)
    torch.cuda.synchronize()
    return _results(o, count)


def _results(o, count):
    for v in o.values():
        v.check()  # nothing written behind row M
    res = {k: v.out.cpu() for k, v in o.items()}
    res["count"] = count
    return res


def _run(precision, M, x, d, g_rgb, g_sigma, *, tail=0.0, poison=False, dense=1, want_in=True, case=None):
    """``_run_on`` fresh buffers."""
    return _run_on(_buffers(precision, M, poison=poison, want_in=want_in, case=case), precision, M, x, d, g_rgb, g_sigma,
                   tail=tail, dense=dense, case=case)


# ------------------------------------------------- 1. padding independence --
@pytest.mark.parametrize("M", ei.RAGGED_M)
@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_padding_independence(precision, M):
    """(a) M samples on zero-filled saved / workspace, zeros behind row M of the inputs;
    (b) the same on 0xFF-filled saved / workspace with NaN behind row M of x, d, g_rgb,
    g_sigma; (c) M' = 32 ceil(M / 32) samples, the first M the same, the rest other finite
    samples whose upstream gradient is exactly zero.  All with dense_backward = 1 (the same
    tile list; make_sizes derives the dW chunking from the tile count, which M and M'
    share, so the extra rows add exact zeros in the same chunk layout).  rgb, sigma, g_x, g_d
    of the first M rows and g_params are bit-identical across the three and finite; the
    sentinel rows behind row M are untouched; the active-tile count is ceil(M / 32)."""
    Mp = (M + 31) // 32 * 32
    x, d = ei.mlp_candidates(Mp, seed=700 + M)
    g_rgb, g_sigma = ei.mlp_upstream(Mp, seed=800 + M)
    g_rgb[M:] = 0.0
    g_sigma[M:] = 0.0
    a = _run(precision, M, x, d, g_rgb, g_sigma)
    b = _run(precision, M, x, d, g_rgb, g_sigma, tail=float("nan"), poison=True)
    c = _run(precision, Mp, x, d, g_rgb, g_sigma)
    tiles = (M + 31) // 32
    assert a["count"] == b["count"] == c["count"] == tiles
    for k in ("rgb", "sigma", "g_x", "g_d", "g_params"):
        assert torch.isfinite(a[k]).all(), k
        assert a[k].abs().max() > 0, k
        assert _same_bits(a[k], b[k]), (k, "poisoned scratch", (a[k] - b[k]).abs().max().item())
        ck = c[k] if k == "g_params" else c[k][:M]
        assert _same_bits(a[k], ck), (k, "padded with live samples", (a[k] - ck).abs().max().item())
    if Mp > M:  # the padding samples of (c) received no gradient
        assert torch.count_nonzero(c["g_x"][M:]) == 0 and torch.count_nonzero(c["g_d"][M:]) == 0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_skipping_backward_on_poisoned_scratch(precision):
    """The default (skipping) backward at M = 513 with the upstream gradient of tiles 0 and 5
    exactly zero, so that the dX launch builds the dW kernel's tile list instead of taking
    the all-active identity path: zero-filled vs 0xFF-filled saved / workspace give the same
    bits, 15 of 17 tiles ran, and the samples of the skipped tiles get exactly zero g_x / g_d."""
    M = 513
    x, d = ei.mlp_candidates(M, seed=760)
    g_rgb, g_sigma = ei.mlp_upstream(M, seed=860)
    for t in (0, 5):
        g_rgb[32 * t: 32 * t + 32] = 0.0
        g_sigma[32 * t: 32 * t + 32] = 0.0
    a = _run(precision, M, x, d, g_rgb, g_sigma, dense=0)
    b = _run(precision, M, x, d, g_rgb, g_sigma, tail=float("nan"), poison=True, dense=0)
    assert a["count"] == b["count"] == 15
    for k in ("rgb", "sigma", "g_x", "g_d", "g_params"):
        assert torch.isfinite(a[k]).all() and _same_bits(a[k], b[k]), k
    for t in (0, 5):
        assert torch.count_nonzero(a["g_x"][32 * t: 32 * t + 32]) == 0
        assert torch.count_nonzero(a["g_d"][32 * t: 32 * t + 32]) == 0
    dense = _run(precision, M, x, d, g_rgb, g_sigma, dense=1)
    assert dense["count"] == 17 and _same_bits(dense["g_x"], a["g_x"]) and _same_bits(dense["g_d"], a["g_d"])
    rel = ((dense["g_params"] - a["g_params"]).norm() / dense["g_params"].norm()).item()
    assert rel < 1e-5, rel  # test_tile_skip's bound: one chunk here, so only dropped zeros differ


# --------------------------------------- 2. against the reference, same M --
def _named_rels(got_flat, named_grads):
    rels, off = {}, 0
    for name, g in named_grads:
        n = g.numel()
        a = got_flat[off:off + n].double().reshape(g.shape)
        rels[name] = ((a - g.double()).norm() / g.double().norm().clamp_min(1e-30)).item()
        off += n
    assert off == got_flat.numel()
    return rels


@pytest.mark.parametrize("M", ei.REF32_M)
def test_fp32_gradients_vs_fp64_at_tiny_m(M):
    """fp32 at M = 1 and 33 (a tile of one sample; one full tile and a tile of one): every
    parameter gradient and g_x, g_d vs fp64 autograd of the oracle under test_fp32_backward's
    rel < 2e-5, on kink-free samples (a kink within rounding would decide a one-sample
    gradient)."""
    oracle, _, _ = _net("fp32")
    x, d, _ = ei.mlp_selected("fp32", M)
    g_rgb, g_sigma = ei.mlp_upstream(M, seed=30 + M, scale=1.0)
    got = _run("fp32", M, x, d, g_rgb, g_sigma, tail=float("nan"), poison=True)
    o64 = ref.NeRF(oracle.config).double()
    o64.load_state_dict({k: v.double() for k, v in oracle.state_dict().items()})
    xr, dr = x.double().requires_grad_(True), d.double().requires_grad_(True)
    wr, ws = o64(xr, dr)
    ((wr * g_rgb.double()).sum() + (ws * g_sigma.double()).sum()).backward()
    assert (got["rgb"].double() - wr.detach()).abs().max() < 1e-4
    assert (got["sigma"].double() - ws.detach().reshape(-1)).abs().max() < 1e-4
    rels = _named_rels(got["g_params"], [(n, p.grad) for n, p in o64.named_parameters()])
    rels["g_x"] = ((got["g_x"].double() - xr.grad).norm() / xr.grad.norm()).item()
    rels["g_d"] = ((got["g_d"].double() - dr.grad).norm() / dr.grad.norm()).item()
    _record(test="mlp_fp32_vs_fp64", M=M, max_rel=max(rels.values()))
    for name, rel in rels.items():
        assert rel < 2e-5, (name, rel)


@pytest.mark.parametrize("M", ei.REF16_M)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_vs_numerics_model_at_ragged_m(precision, M):
    """bf16 / fp16 at M = 1, 31, 33, 513: forward and every parameter gradient vs the
    numerics model at the same M, under the bounds of
    test_16bit_non_default_configs_vs_numerics_model (rgb 1e-4, sigma 1e-3 max(1, |sigma|),
    gradients 1.5e-2 relative) -- at M in the thousands a wrong padded row vanishes inside
    them, here it would be a large part of the sum.  Inputs: edge_inputs.mlp_selected."""
    oracle, _, _ = _net(precision)
    x, d, _ = ei.mlp_selected(precision, M)
    g_rgb, g_sigma = ei.mlp_upstream(M, seed=40 + M)
    got = _run(precision, M, x, d, g_rgb, g_sigma, tail=float("nan"), poison=True)
    base = copy.deepcopy(oracle)
    emu = ref.mfma_emulated_nerf(base, precision)
    er, es = emu(x, d)
    ((er * g_rgb).sum() + (es * g_sigma).sum()).backward()
    e_rgb = (got["rgb"] - er.detach()).abs().max().item()
    e_sig = (got["sigma"] - es.detach().reshape(-1)).abs().max().item()
    assert torch.isfinite(got["g_params"]).all()
    rels = _named_rels(got["g_params"], [(n, p.grad) for n, p in base.named_parameters()])
    _record(test="mlp_16bit_vs_model", precision=precision, M=M, rgb=e_rgb, sigma=e_sig, max_rel=max(rels.values()))
    assert e_rgb < 1e-4, e_rgb
    assert e_sig < 1e-3 * max(1.0, es.abs().max().item()), e_sig
    for name, rel in rels.items():
        assert rel < 1.5e-2, (name, rel)


# ------------------------------------------------ 3. positions at scene scale --
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_forward_at_scene_scale(precision):
    """The 16-bit forward at M = 513 with |x| uniform in 4 .. 8 (the other tests stop at 1.5)
    vs the numerics model at the existing 1e-4 on rgb: 2^9 x / 2 pi exceeds 600 revolutions,
    which holds pe_rev's two-term argument reduction to its "absolute error ~1e-6"."""
    oracle, net, _ = _net(precision)
    M = 513
    x, d = ei.mlp_candidates(M, seed=900, lo=4.0, hi=8.0)
    rgb, sigma = guarded((M, 3), GUARD), guarded((M,), GUARD)
    mlp_raw(precision, M, x.to(DEV), d.to(DEV), None, None, rgb=rgb.buf, sigma=sigma.buf, saved=None, workspace=None,
            g_x=None, g_d=None, g_params=None, dense=0)
    torch.cuda.synchronize()
    rgb.check()
    sigma.check()
    with torch.no_grad():
        er, es = ref.mfma_emulated_nerf(oracle, precision)(x, d)
    e_rgb = (rgb.out.cpu() - er).abs().max().item()
    e_sig = (sigma.out.cpu() - es.reshape(-1)).abs().max().item()
    _record(test="mlp_16bit_scene_scale", precision=precision, rgb=e_rgb, sigma=e_sig, sigma_max=es.abs().max().item())
    assert e_rgb < 1e-4, e_rgb


# ------------------------- D. scratch independence of the other entry points --
def _both_scratch(nbytes, fn):
    """fn(workspace) on a zero-filled and on a 0xFF-filled workspace -> both results."""
    res = []
    for ws in (torch.zeros(int(nbytes), dtype=torch.uint8, device=DEV), poisoned(nbytes)):
        res.append(fn(ws))
        torch.cuda.synchronize()
    return res


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert torch.isfinite(x.double()).all() and _same_bits(x, y)


def test_get_rays_bwd_scratch():
    from noisy_src import _hip
    N = 37
    g = torch.Generator().manual_seed(51)
    dirs = torch.randn(N, 3, generator=g).to(DEV)
    c2w = torch.eye(4)
    c2w[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g)).Q
    c2w[:3, 3] = torch.randn(3, generator=g)
    c2w = c2w.to(DEV)
    g_ro, g_rd = torch.randn(N, 3, generator=g).to(DEV), torch.randn(N, 3, generator=g).to(DEV)

    def run(ws):
        g_dirs, g_c2w = guarded((N, 3)), guarded((4, 4), init=torch.zeros(5, 4))
        _call("nr_get_rays_bwd", dirs, c2w, N, g_ro, g_rd, g_dirs.buf, g_c2w.buf, ws)
        torch.cuda.synchronize()
        g_dirs.check()
        g_c2w.check()
        return g_dirs.out.clone(), g_c2w.out.clone()

    a, b = _both_scratch(_hip.load().nr_get_rays_bwd_workspace_bytes(), run)
    _assert_same(a, b)
    assert torch.allclose(a[1][:3, 3], g_ro.sum(0), rtol=1e-5, atol=1e-6) and a[1][:3, :3].abs().max() > 0


@pytest.mark.parametrize("n", [1, 10007])
def test_sumsq_scratch(n):
    from noisy_src import _hip
    x = torch.randn(n, generator=torch.Generator().manual_seed(52 + n)).to(DEV)

    def run(ws):
        acc = torch.zeros(2, device=DEV)
        _call("nr_sumsq", x, n, acc, ws)
        return (acc.clone(),)

    a, b = _both_scratch(_hip.load().nr_sumsq_workspace_bytes(), run)
    _assert_same(a, b)
    want = x.double().square().sum().item()
    assert a[0][1] == 0 and abs(a[0][0].item() - want) <= 1e-6 * want


def test_sumsq_partials_scratch():
    """The partials buffer is the only scratch, and it is OVERWRITTEN: 3 spans, one of
    length 1; prefilled with zeros or with 0xFF bytes."""
    from noisy_src import _hip
    g = torch.Generator().manual_seed(53)
    xs = [torch.randn(n, generator=g).to(DEV) for n in (10007, 1, 130)]
    ptrs = (ctypes.c_void_p * 3)(*[_hip.ptr(x) for x in xs])
    ns = (ctypes.c_int64 * 3)(*[x.numel() for x in xs])

    def run(ws):
        _hip.call("nr_sumsq_partials", ptrs, ns, 3, _hip.ptr(ws), _hip.stream_ptr())
        return (ws.view(torch.float32).clone(),)

    a, b = _both_scratch(_hip.load().nr_sumsq_workspace_bytes(), run)
    _assert_same(a, b)
    want = sum(x.double().square().sum().item() for x in xs)
    assert abs(a[0].double().sum().item() - want) <= 1e-6 * want


@pytest.mark.parametrize("S", [65, 513])
def test_composite_mse_scratch(S):
    """B = 5; the ticket is 0 before the call by contract and 0 after it; only the workspace
    (the per-ray squared errors, and the seed gradient of the long form) is poisoned."""
    from noisy_src import _hip
    B = 5
    c = ei.composite_inputs(S, B, "random")
    dv = {k: (None if v is None else v.to(DEV)) for k, v in c.items()}
    ticket = torch.zeros(4, device=DEV, dtype=torch.int32)

    def run(ws):
        o = dict(rgb_map=guarded((B, 3)), depth=guarded((B,)), acc=guarded((B,)), weights=guarded((B, S)),
                 loss=guarded((1,)), g_rgb=guarded((B, S, 3)), g_sigma=guarded((B, S)),
                 g_rd=guarded((B, 3), init=torch.zeros(B + 1, 3)))
        _call("nr_composite_mse", dv["rgb"], dv["sigma"], dv["z"], dv["rd"], dv["noise"], dv["target"], B, S, 1, 1.0,
              o["rgb_map"].buf, o["depth"].buf, o["acc"].buf, o["weights"].buf, o["loss"].buf, o["g_rgb"].buf,
              o["g_sigma"].buf, o["g_rd"].buf, ticket, ws)
        torch.cuda.synchronize()
        for v in o.values():
            v.check()
        assert torch.count_nonzero(ticket) == 0
        return [v.out.clone() for v in o.values()]

    a, b = _both_scratch(_hip.load().nr_composite_mse_workspace_bytes(B), run)
    _assert_same(a, b)


@pytest.mark.parametrize("C", [1, 3])
def test_image_metrics_scratch(C):
    """H = 17, W = 33: two tiles across and two down, both partly filled; nerf_hip.h says
    the workspace needs no initialisation."""
    from noisy_src import _hip
    from noisy_src.metrics import _WINDOW, _gaussian_1d, compute_mse, compute_ssim
    H, W = 17, 33
    g = torch.Generator().manual_seed(54 + C)
    pred, target = torch.rand(H, W, C, generator=g), torch.rand(H, W, C, generator=g)
    pd, td = pred.to(DEV), target.to(DEV)
    gw = (ctypes.c_float * _WINDOW)(*_gaussian_1d(_WINDOW).tolist())

    def run(ws):
        out = guarded((2,), init=torch.full((3,), -1.0, dtype=F64))
        _hip.call("nr_image_metrics", _hip.ptr(pd), _hip.ptr(td), H, W, C, gw, 0.01 ** 2, 0.03 ** 2, _hip.ptr(out.buf),
                  _hip.ptr(ws), _hip.stream_ptr())
        torch.cuda.synchronize()
        out.check()
        return (out.out.clone(),)

    a, b = _both_scratch(_hip.call("nr_image_metrics_workspace_bytes", H, W, C), run)
    _assert_same(a, b)
    n = H * W * C
    # (the values themselves are test_image_tail's subject: here only that they are the metrics)
    assert abs(a[0][0].item() / n - compute_ssim(pred, target).item()) < 1e-4
    assert abs(a[0][1].item() / n - compute_mse(pred.double(), target.double()).item()) < 1e-6


def test_depth_frame_u8_scratch():
    from noisy_src import _hip
    H, W = 17, 33
    depth = (torch.rand(H, W, generator=torch.Generator().manual_seed(55)) * 4 + 2).to(DEV)

    def run(ws):
        dst = guarded((H, W, 3), init=torch.full((H + 1, W, 3), 7, dtype=torch.uint8))
        _call("nr_depth_frame_u8", depth, H, W, dst.buf, ws)
        torch.cuda.synchronize()
        dst.check()
        return (dst.out.clone(),)

    a, b = _both_scratch(_hip.load().nr_depth_frame_u8_workspace_bytes(), run)
    assert _same_bits(a[0], b[0])
    assert a[0].float().std() > 0
