"""GPU: the frozen-field pair nr_mlp_forward_frozen / nr_mlp_backward_input against the
training pair nr_mlp_forward (with saved) / nr_mlp_backward_dx.

The frozen pair keeps only what an input-gradient backward reads (16-bit: the ReLU masks,
and of the dz images those of layer 0, of the layer after each skip and of dir_linear) and
runs the same products in the same order, so rgb, sigma, g_x and g_d must equal the
training pair's BIT FOR BIT: at ragged M (one sample; a tile minus / plus one; 16 tiles
minus / plus one sample, i.e. two forward workgroups and waves without a tile; 257 tiles
plus one sample, which crosses a 256-tile segment of the active-tile list), dense and
skipping, for every precision, for the configs that decide which dz images are stored and
which (XB, DB) kernel instance runs, and with either gradient pointer NULL.  The frozen
buffers are exactly as large as the size queries say: they carry guard bytes behind them,
and are once zero-filled and once 0xFF-filled (with NaN behind row M of the inputs).

Not only a self-comparison: in fp32, g_x / g_d against fp64 autograd of the oracle.
At the autograd level a NeRF with frozen parameters gives the input gradients of the same
network with live ones, leaves no parameter gradient and does not touch ``_last_gflat``."""
import ctypes
import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from oracle import refimpl as ref

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
from test_edge_shapes import guarded, poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 33          # sentinel rows behind every per-sample output: more than a tile
GUARD_BYTES = 4096  # sentinel bytes behind saved_frozen and the frozen workspace
FROZEN_M = [1, 31, 33, 511, 513, 8225]

CONFIGS = {
    "default": {},
    "no_skip": dict(skips=()),
    "skips_2_5": dict(skips=(2, 5)),
    "no_view_dirs": dict(use_view_dirs=False),
    "two_layers": dict(num_hidden_layers=2, skips=()),
    "pos_freqs_4": dict(pos_freqs=4),
}


@functools.lru_cache(maxsize=None)
def _net(precision, config="default"):
    """(oracle, HIP network with its weights, packed images) of a named config (of CONFIGS,
    or of edge_inputs.CONFIG_CASES for test_mlp_configs.py)."""
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    mc = ModelConfig(precision=precision, **(CONFIGS[config] if config in CONFIGS else ei.CONFIG_CASES[config][0]))
    torch.manual_seed(0)
    oracle = ref.NeRF(mc)
    net = NeRF(mc)
    net.load_state_dict(oracle.state_dict())
    net = net.to(DEV)
    net._ensure_flat()
    return oracle, net, net._packed_for_forward()


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _scratch(nbytes, poison, guard):
    """A scratch buffer of nbytes (zeros or 0xFF) with ``guard`` bytes of 0xA5 behind it."""
    buf = torch.full((int(nbytes) + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    buf[:int(nbytes)] = poisoned(nbytes) if poison else 0
    return buf


def _pair(precision, M, x, d, g_rgb, g_sigma, *, frozen, dense, poison=False, tail=0.0, config="default",
          want_x=True, want_d=True):
    """Forward + input-gradient backward of the first M rows through the frozen or the
    training entry points on buffers the test owns -> rgb, sigma, g_x, g_d on the host."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    _, net, packed = _net(precision, config)
    cfg = _hip.NrMlpConfig.from_buffer_copy(net._nr_cfg)
    cfg.dense_backward = int(dense)
    c, st, flat, lib = ctypes.byref(cfg), _hip.stream_ptr(), net._flat, _hip.load()
    Mp = (M + 31) // 32 * 32

    def padded(t, width):
        buf = torch.full((Mp, width), tail)
        buf[:M] = t[:M].reshape(M, width)
        return buf.to(DEV)

    xd, gr, gs = padded(x, 3), padded(g_rgb, 3), padded(g_sigma, 1)
    dd = padded(d, 3) if net.config.use_view_dirs else None
    want_d = want_d and dd is not None
    n_saved = (lib.nr_mlp_frozen_saved_bytes if frozen else lib.nr_mlp_saved_bytes)(c, M)
    n_ws = (lib.nr_mlp_frozen_workspace_bytes if frozen else lib.nr_mlp_workspace_bytes)(c, M)
    assert n_saved > 0 and n_ws > 0
    saved, ws = _scratch(n_saved, poison, GUARD_BYTES), _scratch(n_ws, poison, GUARD_BYTES)
    o = dict(rgb=guarded((M, 3), GUARD), sigma=guarded((M,), GUARD))
    if want_x:
        o["g_x"] = guarded((M, 3), GUARD)
    if want_d:
        o["g_d"] = guarded((M, 3), GUARD)
    fwd, bwd = ("nr_mlp_forward_frozen", "nr_mlp_backward_input") if frozen else ("nr_mlp_forward", "nr_mlp_backward_dx")
    call(fwd, c, ptr(packed), ptr(flat), ptr(xd), ptr(dd), M, ptr(o["rgb"].buf), ptr(o["sigma"].buf), ptr(saved), st)
    call(bwd, c, ptr(packed), ptr(flat), ptr(xd), ptr(dd), M, ptr(o["rgb"].buf), ptr(o["sigma"].buf), ptr(saved),
         ptr(gr), ptr(gs), ptr(o["g_x"].buf) if want_x else None, ptr(o["g_d"].buf) if want_d else None, ptr(ws), st)
    torch.cuda.synchronize()
    for v in o.values():
        v.check()  # nothing written behind row M
    for buf, n in ((saved, n_saved), (ws, n_ws)):
        assert bool((buf[int(n):] == 0xA5).all()), "written behind the size the query returned"
    return {k: v.out.cpu() for k, v in o.items()}


def _inputs(M, seed):
    Mp = (M + 31) // 32 * 32
    x, d = ei.mlp_candidates(Mp, seed=seed)
    g_rgb, g_sigma = ei.mlp_upstream(Mp, seed=seed + 100)
    return x, d, g_rgb, g_sigma


def _assert_equal(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.isfinite(got[k]).all(), (what, k)
        assert _same_bits(got[k], want[k]), (what, k, (got[k] - want[k]).abs().max().item())


@pytest.mark.parametrize("M", FROZEN_M)
@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_frozen_pair_bit_identical_to_training_pair(precision, M):
    """rgb, sigma, g_x, g_d of the frozen pair == the training pair's, dense and skipping, on
    zero-filled and on 0xFF-filled frozen buffers with NaN behind row M of the inputs."""
    x, d, g_rgb, g_sigma = _inputs(M, 1700 + M)
    for dense in (1, 0):
        want = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=False, dense=dense)
        assert want["g_x"].abs().max() > 0 and want["g_d"].abs().max() > 0
        a = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=True, dense=dense)
        b = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=True, dense=dense, poison=True, tail=float("nan"))
        _assert_equal(a, want, f"dense={dense} zero-filled")
        _assert_equal(b, want, f"dense={dense} poisoned")


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_frozen_skips_tiles_without_gradient(precision):
    """M = 513, dense_backward = 0, tiles 0 and 5 with an exactly zero upstream gradient: their
    samples get exactly zero g_x / g_d, every sample equals the training pair's."""
    M = 513
    x, d, g_rgb, g_sigma = _inputs(M, 1760)
    for t in (0, 5):
        g_rgb[32 * t: 32 * t + 32] = 0.0
        g_sigma[32 * t: 32 * t + 32] = 0.0
    want = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=False, dense=0)
    got = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=True, dense=0, poison=True, tail=float("nan"))
    _assert_equal(got, want, "skipping")
    for t in (0, 5):
        for k in ("g_x", "g_d"):
            assert torch.count_nonzero(got[k][32 * t: 32 * t + 32]) == 0, (k, t)
    assert torch.count_nonzero(got["g_x"][32:64]) > 0


@pytest.mark.parametrize("M", [33, 513])
@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "default"])
def test_frozen_pair_other_configs(config, M):
    """bf16: no skip (dz_0 and dz_c only), two skips (three trunk images), no view directions
    (DB = 0, no g_d), two layers, pos_freqs = 4 (XB = 1)."""
    x, d, g_rgb, g_sigma = _inputs(M, 1800 + M)
    for dense in (1, 0):
        want = _pair("bf16", M, x, d, g_rgb, g_sigma, frozen=False, dense=dense, config=config)
        got = _pair("bf16", M, x, d, g_rgb, g_sigma, frozen=True, dense=dense, config=config, poison=True,
                    tail=float("nan"))
        assert want["g_x"].abs().max() > 0
        assert ("g_d" in want) == (config != "no_view_dirs")
        _assert_equal(got, want, f"{config} dense={dense}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("which", ["x", "d"])
def test_frozen_one_gradient_only(precision, which):
    """g_x alone and g_d alone (the other pointer NULL) at M = 513."""
    M = 513
    x, d, g_rgb, g_sigma = _inputs(M, 1900)
    kw = dict(want_x=which == "x", want_d=which == "d")
    want = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=False, dense=0, **kw)
    got = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=True, dense=0, poison=True, tail=float("nan"), **kw)
    assert ("g_x" in got) == (which == "x") and ("g_d" in got) == (which == "d")
    _assert_equal(got, want, which)


def test_frozen_fp32_input_gradients_vs_fp64():
    """fp32, M = 33, kink-free samples (edge_inputs.mlp_selected): g_x and g_d of the frozen
    pair vs fp64 autograd of the oracle, rel < 2e-5 (test_fp32_gradients_vs_fp64_at_tiny_m's)."""
    M = 33
    oracle = ei.oracle_net("fp32")
    assert all(torch.equal(a, b) for a, b in zip(oracle.state_dict().values(), _net("fp32")[0].state_dict().values()))
    x, d, _ = ei.mlp_selected("fp32", M)
    g_rgb, g_sigma = ei.mlp_upstream(M, seed=30 + M, scale=1.0)
    got = _pair("fp32", M, x, d, g_rgb, g_sigma, frozen=True, dense=0, poison=True, tail=float("nan"))
    o64 = ref.NeRF(oracle.config).double()
    o64.load_state_dict({k: v.double() for k, v in oracle.state_dict().items()})
    xr, dr = x.double().requires_grad_(True), d.double().requires_grad_(True)
    wr, ws = o64(xr, dr)
    ((wr * g_rgb.double()).sum() + (ws * g_sigma.double()).sum()).backward()
    for k, g in (("g_x", xr.grad), ("g_d", dr.grad)):
        rel = ((got[k].double() - g).norm() / g.norm()).item()
        print(f"FROZEN_FP32 {k} rel {rel:.3e}")
        assert rel < 2e-5, (k, rel)


def test_frozen_entry_points_reject_and_accept_empty():
    """M == 0 is NR_OK without touching a buffer; a config outside the envelope is NR_EARG
    with the plan's message."""
    from noisy_src import _hip
    _, net, packed = _net("bf16")
    lib, c, p = _hip.load(), ctypes.byref(net._nr_cfg), _hip.ptr
    one = torch.zeros(64, device=DEV)
    assert lib.nr_mlp_forward_frozen(c, p(packed), p(net._flat), p(one), p(one), 0, p(one), p(one), p(one), None) == 0
    assert lib.nr_mlp_backward_input(c, p(packed), p(net._flat), p(one), p(one), 0, p(one), p(one), p(one), p(one),
                                     p(one), p(one), p(one), p(one), None) == 0
    bad = _hip.NrMlpConfig.from_buffer_copy(net._nr_cfg)
    bad.hidden = 128
    assert lib.nr_mlp_forward_frozen(ctypes.byref(bad), p(packed), p(net._flat), p(one), p(one), 1, p(one), p(one),
                                     p(one), None) != 0
    assert "hidden_dim" in _hip.last_error()
    torch.cuda.synchronize()
    assert torch.count_nonzero(one) == 0


# ------------------------------------------------------------------ autograd --
def _autograd_case(precision, window, M=513):
    """x.grad, d.grad with live parameters, then with frozen ones, on one network."""
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    torch.manual_seed(3)
    net = NeRF(ModelConfig(precision=precision)).to(DEV)
    if window:
        net.set_pe_window([1.0] * 4 + [0.5] + [0.0] * 5, [1.0, 1.0, 0.25, 0.0])
    x, d = ei.mlp_candidates(M, seed=2100)
    g_rgb, g_sigma = ei.mlp_upstream(M, seed=2200)
    g_rgb, g_sigma = g_rgb.to(DEV), g_sigma.to(DEV)
    res = {}
    for name, live in (("live", True), ("frozen", False)):
        for q in net.parameters():
            q.requires_grad_(live)
            q.grad = None
        if live:
            net._last_gflat = None
        marker = net._last_gflat
        xr, dr = x.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
        rgb, sigma = net(xr, dr)
        ((rgb * g_rgb).sum() + (sigma * g_sigma).sum()).backward()
        torch.cuda.synchronize()
        res[name] = dict(rgb=rgb.detach().cpu(), sigma=sigma.detach().cpu(), gx=xr.grad.cpu(), gd=dr.grad.cpu(),
                         pgrad=[q.grad for q in net.parameters()], gflat_same=net._last_gflat is marker,
                         gflat=net._last_gflat)
    return res


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_autograd_frozen_network(precision, window):
    res = _autograd_case(precision, window)
    live, frozen = res["live"], res["frozen"]
    assert all(g is not None for g in live["pgrad"]) and live["gflat"] is not None
    assert live["gx"].abs().max() > 0 and live["gd"].abs().max() > 0
    for k in ("rgb", "sigma", "gx", "gd"):
        assert _same_bits(frozen[k], live[k]), (k, (frozen[k] - live[k]).abs().max().item())
    assert all(g is None for g in frozen["pgrad"])
    assert frozen["gflat_same"], "_last_gflat was replaced by a frozen backward"


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[3])
import test_frozen_mlp as t
from noisy_src import model
assert model._FROZEN is False
res = t._autograd_case("bf16", False)
torch.save({k: res["frozen"][k] for k in ("rgb", "sigma", "gx", "gd")}, sys.argv[4])
"""


def test_env_switch_sends_frozen_network_through_training_kernels(tmp_path):
    """NR_MLP_FROZEN=0 (read at import: a fresh child process): a frozen network's forward and
    input gradients through the training kernels equal this process's frozen path."""
    root = Path(__file__).resolve().parents[1]
    out = tmp_path / "child.pt"
    env = dict(os.environ, NR_MLP_FROZEN="0")
    subprocess.run([sys.executable, "-c", _CHILD, str(root), str(root / "robust-nerf_amd"), str(root / "tests"),
                    str(out)], check=True, env=env, timeout=300)
    child = torch.load(out, weights_only=True)
    here = _autograd_case("bf16", False)["frozen"]
    for k in ("rgb", "sigma", "gx", "gd"):
        assert _same_bits(child[k], here[k]), k
