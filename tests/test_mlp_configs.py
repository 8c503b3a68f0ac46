"""GPU: the fused MLP at the boundaries of the ModelConfig space make_plan accepts.

The other GPU tests run the kernels on the default model, pos_freqs in {4, 6, 10},
dir_freqs in {2, 4}, depths {1, 2, 5, 7, 8} and a handful of skip sets.  The cases of
edge_inputs.CONFIG_CASES reach what those leave out: an encoding one column past a
32-column block, an encoding without trigonometric columns, a skip straight after layer 0,
adjacent skips, a skip at the last allowed layer, no view directions behind a skip, and
depth 16 (kMaxTrunk), where the dW job table, the reduce table and the fp32 weight streams
are closest to full (tests/test_plan.py sweeps the plan itself on the host).

Each (case, precision) runs at M = 33 -- one full tile and a tile of one sample, so that a
wrong padded row or block is a large part of every sum -- and the depth-16 cases also at
M = 513 (a 16-tile forward group plus one tile), with NaN behind row M of the inputs and
0xFF-filled saved / workspace (test_mlp_ragged._run).  The forward, every named parameter's
gradient, g_x and g_d are held to the reference of edge_inputs.config_case under the
project's existing bars (edge_inputs.config_bounds); test_edge_inputs_host.py asserts on
the CPU that the inputs are kink-free and plentiful, that every reference gradient is
nonzero, and that wrong-kernel mutations of the reference miss these bars.

Distances are printed as ``EDGE_PARITY`` lines (profiles/mlp_config_parity.json)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
from test_edge_shapes import _record  # noqa: E402
from test_mlp_ragged import _run  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ei.CONFIG_PRECISIONS)
@pytest.mark.parametrize("case,M", ei.CONFIG_RUNS, ids=lambda v: str(v))
def test_boundary_config_vs_reference(case, M, precision):
    """fp32 against fp64 autograd of the oracle (rgb, sigma 1e-4 absolute; every gradient
    2e-5 relative, test_fp32_backward's), bf16 / fp16 against the numerics model (rgb 1e-4,
    sigma 1e-3 max(1, |sigma|), parameter gradients 1.5e-2, g_x 2e-2, g_d 1e-2), per named
    parameter, and for pos_freqs = 5 also on the lone live column of the second encoding
    block by itself.  The active-tile count is ceil(M / 32).

    The depth-16 cases in bf16 / fp16 run the dX chain's instance that reads the ReLU masks
    in place: with the masks of all layers in LDS (201 KB at depth 16) nr_mlp_backward_dx
    used to return NR_EARG for every 16-bit model deeper than 10 layers.

    Where the numerics model is not a reference to 1.5e-2 -- trunk layers 0..2 of the
    depth-16 cases in fp16 (edge_inputs.ILL_CONDITIONED), where dz 2^14 is an fp16 subnormal
    throughout and the model's own twin with another summation order
    (edge_inputs.model_conditioning) is 0.11 / 0.05 / 0.02 from it -- the parameter's bound is
    1.5 x the twin's distance (0.16 / 0.07 / 0.03), which stays below the model's distance
    from the fp64 oracle on the same samples (0.2 / 0.1 / 0.05).  The kernels measured
    0.10 .. 0.12 / 0.04 .. 0.05 / 0.018 .. 0.021; all three numbers are recorded per
    parameter.  test_edge_inputs_host asserts that the twin justifies exactly that list."""
    c = ei.config_case(case, precision, M)
    want = c["want"]
    got = _run(precision, M, c["x"], c["d"], c["g_rgb"], c["g_sigma"], tail=float("nan"), poison=True, case=case)
    assert got["count"] == (M + 31) // 32
    for k in ("rgb", "sigma", "g_x", "g_d", "g_params"):
        assert k not in got or torch.isfinite(got[k]).all(), k
    assert ("g_d" in got) == (want["g_d"] is not None)
    grads, off = [], 0
    for name, w in want["grads"]:
        grads.append((name, got["g_params"][off:off + w.numel()].reshape(w.shape)))
        off += w.numel()
    assert off == got["g_params"].numel()
    dist = ei.config_distances(dict(got, grads=grads), want, case)
    worst = max((k for k in dist if k not in ("rgb", "sigma")), key=dist.get)
    _record(test="mlp_config_vs_reference", case=case, precision=precision, M=M, rgb=dist["rgb"], sigma=dist["sigma"],
            sigma_max=want["sigma"].abs().max().item(), g_x=dist["g_x"], g_d=dist.get("g_d"), max_rel=dist[worst],
            max_rel_at=worst)
    for name, bound in c["grad_bounds"].items():  # both numbers behind every bound that is not 1.5e-2
        _record(test="mlp_config_model_conditioning", case=case, precision=precision, M=M, parameter=name,
                twin_to_model=c["twin"][name], model_to_fp64_oracle=c["oracle"][name], bound=bound, kernel=dist[name])
    missed = ei.check_config_distances(dist, precision, want["sigma"].abs().max().item(), c["grad_bounds"])
    assert not missed, missed


# ------------------------------------------ bitwise identities on the same cases --
BITWISE_PRECISIONS = ["bf16", "fp32"]


@pytest.mark.parametrize("precision", BITWISE_PRECISIONS)
@pytest.mark.parametrize("case", list(ei.CONFIG_CASES))
def test_frozen_pair_equals_training_pair_bitwise(case, precision):
    """nr_mlp_forward_frozen + nr_mlp_backward_input == nr_mlp_forward + nr_mlp_backward_dx bit
    for bit in rgb, sigma, g_x and g_d at M = 33, the frozen buffers 0xFF-filled with NaN
    behind row M of the inputs.  For the depth-16 cases in bf16 this is the only run of the
    input-only dX chain's instance that reads the ReLU masks in place."""
    from test_frozen_mlp import _assert_equal, _pair
    M = 33
    x, d = ei.mlp_candidates(64, seed=610)
    g_rgb, g_sigma = ei.mlp_upstream(64, seed=611)
    train = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=False, dense=1, config=case)
    frozen = _pair(precision, M, x, d, g_rgb, g_sigma, frozen=True, dense=1, poison=True, tail=float("nan"), config=case)
    assert train["g_x"].abs().max() > 0 and train["sigma"].abs().max() >= 0
    _assert_equal(frozen, train, case)


def _raw_net(precision, case):
    """A fresh HIP network of the case (its own flat buffer and images: these tests write them)."""
    from noisy_src.model import NeRF
    net = NeRF(ei.case_config(precision, case))
    net.load_state_dict(ei.oracle_net(precision, case=case).state_dict())
    net = net.to("cuda")
    net._ensure_flat()
    return net


@pytest.mark.parametrize("precision", BITWISE_PRECISIONS)
@pytest.mark.parametrize("case", list(ei.CONFIG_CASES))
def test_adam_step_with_pack_table_equals_a_fresh_pack(case, precision):
    """After one nr_adam_multi step with the case's pack table, ``packed`` equals
    nr_mlp_pack of the stepped parameters byte for byte (and the step moved both)."""
    import ctypes
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    net = _raw_net(precision, case)
    packed = net._packed_for_forward()
    before, flat0 = packed.clone(), net._flat.clone()
    n = net._param_count
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 1e-2
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    table = net._pack_table()
    span = _hip.NrAdamSpan(ptr(net._flat), ptr(g), ptr(m), ptr(v), n, None, 1.0, ptr(table), ptr(packed))
    arr = (_hip.NrAdamSpan * 1)(span)
    call("nr_adam_multi", arr, 1, 5e-4, 0.9, 0.999, 1e-8, 1, None, _hip.stream_ptr())
    fresh = before.clone()  # the alignment gaps nr_mlp_pack never writes compare equal
    call("nr_mlp_pack", ctypes.byref(net._nr_cfg), ptr(net._flat), ptr(fresh), _hip.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.equal(net._flat, flat0) and not torch.equal(packed, before)
    assert torch.equal(packed, fresh), (packed != fresh).sum().item()


@pytest.mark.parametrize("precision", BITWISE_PRECISIONS)
@pytest.mark.parametrize("case", list(ei.CONFIG_CASES))
def test_window_fold_and_window_gradient(case, precision):
    """nr_mlp_fold_window with all-ones weights leaves ``packed`` byte-identical; a window that
    zeroes the top frequency changes the images, and nr_mlp_window_grad under it leaves
    exactly zero in that frequency's six columns of every weight that reads the encoding
    (position: layer 0 and the layers after a skip; direction: dir_linear) and every other
    gradient entry bit-identical.  pos0_dir0 has no frequency: the identity part only."""
    import ctypes
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    net = _raw_net(precision, case)
    cfg, c, st = net.config, ctypes.byref(net._nr_cfg), _hip.stream_ptr()
    packed = net._packed_for_forward()
    want = packed.clone()
    ones_p, ones_d = torch.ones(max(cfg.pos_freqs, 1), device="cuda"), torch.ones(max(cfg.dir_freqs, 1), device="cuda")
    use_d = bool(cfg.use_view_dirs)
    call("nr_mlp_fold_window", c, ptr(net._flat), ptr(ones_p), ptr(ones_d) if use_d else None, ptr(packed), st)
    torch.cuda.synchronize()
    assert torch.equal(packed, want)
    if cfg.pos_freqs == 0:
        return
    wp = ones_p.clone()
    wp[-1] = 0.0
    wd = None
    if use_d and cfg.dir_freqs > 0:
        wd = ones_d.clone()
        wd[-1] = 0.0
    call("nr_mlp_fold_window", c, ptr(net._flat), ptr(wp), ptr(wd), ptr(packed), st)
    torch.cuda.synchronize()
    assert not torch.equal(packed, want)
    g = torch.randn(net._param_count, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    g0 = g.clone()
    call("nr_mlp_window_grad", c, ptr(wp), ptr(wd), ptr(g), st)
    torch.cuda.synchronize()
    pos_dim, dir_dim = 3 * (1 + 2 * cfg.pos_freqs), 3 * (1 + 2 * cfg.dir_freqs)
    zeroed = {"pts_linears.0.weight": (pos_dim - 6, pos_dim)}
    zeroed.update({f"pts_linears.{i + 1}.weight": (pos_dim - 6, pos_dim) for i in cfg.skips})
    if wd is not None:
        zeroed["dir_linear.weight"] = (cfg.hidden_dim + dir_dim - 6, cfg.hidden_dim + dir_dim)
    off = 0
    for name, p in net.named_parameters():
        a, b = g[off:off + p.numel()].view(p.shape), g0[off:off + p.numel()].view(p.shape).clone()
        if name in zeroed:
            lo, hi = zeroed[name]
            assert torch.count_nonzero(a[:, lo:hi]) == 0 and torch.count_nonzero(b[:, lo:hi]) > 0, name
            b[:, lo:hi] = 0.0
        assert torch.equal(a, b), name
        off += p.numel()
    assert off == g.numel()


# ------------------------------------------------- input gradients at scene scale --
def _compare(got, want, grads_of=None):
    grads, off = [], 0
    for name, w in want["grads"]:
        grads.append((name, got["g_params"][off:off + w.numel()].reshape(w.shape)))
        off += w.numel()
    assert off == got["g_params"].numel()
    return dict(got, grads=grads)


@pytest.mark.parametrize("precision", ei.CONFIG_PRECISIONS)
def test_input_gradients_at_scene_scale(precision):
    """The default model at M = 513 with |x| uniform in 4 .. 10, where the pose path's g_x
    flows through the encoding's backward (16 bit: the hardware sine a quarter revolution on,
    times 2^k, after the two-term argument reduction; 2^9 x is beyond 800 revolutions): g_x,
    g_d and the gradients of layer 0 and of the layer after the skip.  fp32 against fp64
    autograd under 2e-5; bf16 / fp16 against the numerics model under g_x 2e-2, g_d 1e-2,
    parameters 1.5e-2; rgb 1e-4 as test_16bit_forward_at_scene_scale."""
    c = ei.scene_case(precision)
    M = ei.SCENE_M
    got = _run(precision, M, c["x"], c["d"], c["g_rgb"], c["g_sigma"], tail=float("nan"), poison=True)
    assert got["count"] == (M + 31) // 32
    for k in ("g_x", "g_d", "g_params"):
        assert torch.isfinite(got[k]).all(), k
    dist = ei.scene_distances(_compare(got, c["want"]), c["want"])
    assert set(dist) == {"rgb", "g_x", "g_d", "g_x[-1]", "g_d[-1]", *ei.SCENE_PARAMS}
    _record(test="mlp_scene_scale_gradients", precision=precision, M=M, **dist)
    missed = ei.check_config_distances(dist, precision, 1.0)
    assert not missed, missed


# ----------------------------- the fp16 backward across the callers' magnitudes --
@pytest.mark.parametrize("M", ei.FP16_SCALE_M)
@pytest.mark.parametrize("B,outlier", ei.FP16_SCALE_RUNS)
def test_fp16_backward_across_gradient_magnitudes(B, outlier, M):
    """fp16, the default model, upstream gradients of a mean loss over B rays, 2 / (3 B) randn
    for B in {65536, 4096, 512, 64, 8}, and for B = 4096 with one sample's g_sigma 1e4 times
    the others: the kernels are finite and meet the 16-bit bounds against the numerics model
    (rgb 1e-4, sigma 1e-3 max(1, |sigma|), parameter gradients 1.5e-2, g_x 2e-2, g_d 1e-2);
    the active-tile count is ceil(M / 32).

    The fp16 backward stores every dz scaled by 2^14 with round-to-nearest conversions and no
    saturation.  On the CPU the numerics model stays finite over this whole list (the largest
    stored value is 2.8e4, the outlier's head at M = 513) and no layer's stored dz is all
    zero; test_edge_inputs_host asserts it, so no scale is left out here.  The model's range:
    finite while every |g_sigma| and |g_rgb (1 - rgb) rgb| stays below 65504 / 2^14 = 3.998 --
    a mean-loss gradient 2 / (3 B) randn stays inside it for every B >= 1, a summed loss over
    more than a few samples does not -- and, downwards, no layer's dz is flushed to all zeros
    down to 2^-14 of the 4096-ray magnitude (1e-8), the smallest tried."""
    c = ei.fp16_scale_case(M, B, outlier)
    want = c["want"]
    got = _run("fp16", M, c["x"], c["d"], c["g_rgb"], c["g_sigma"], tail=float("nan"), poison=True)
    assert got["count"] == (M + 31) // 32
    for k in ("rgb", "sigma", "g_x", "g_d", "g_params"):
        assert torch.isfinite(got[k]).all(), k
    dist = ei.config_distances(_compare(got, want), want, None)
    worst = max((k for k in dist if k not in ("rgb", "sigma")), key=dist.get)
    _record(test="mlp_fp16_gradient_magnitude", B=B, outlier=outlier, M=M, scale=2.0 / (3 * B), rgb=dist["rgb"],
            sigma=dist["sigma"], g_x=dist["g_x"], g_d=dist["g_d"], max_rel=dist[worst], max_rel_at=worst,
            model_max_stored_dz=max(v.float().abs().max().item() for v in c["stored"]))
    missed = ei.check_config_distances(dist, "fp16", want["sigma"].abs().max().item())
    assert not missed, missed
