"""CPU: the input generators of test_edge_shapes.py and test_mlp_ragged.py (edge_inputs.py)
meet the conditions those GPU tests rely on, checked on the oracle alone."""
import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402

FLT_MIN = 2.0 ** -126


@pytest.mark.parametrize("B", ei.COMPOSITE_B)
@pytest.mark.parametrize("S", ei.COMPOSITE_S)
def test_surface_regime_is_opaque_then_dark(S, B):
    """Every ray has a sample with alpha == 1.0 exactly in fp32 behind its empty run (sigma
    <= 0, some exactly 0 where the run is long enough to hold both kinds), and, where the
    ray is long enough for four opaque samples (S >= 63 here), ray 0's transmittance is
    denormal or exactly 0 further on.  |rays_d| lies in 0.5 .. 2."""
    c = ei.composite_inputs(S, B, "surface")
    alpha, T, dists = ei.composite_terms_fp32(c)
    assert alpha.dtype == torch.float32
    assert torch.all((alpha == 1.0).any(-1))
    x = torch.relu(c["sigma"]) * dists
    assert torch.all(((x > 100) & (alpha == 1.0)).sum(-1) >= min(S, 3))
    first = (alpha == 1.0).float().argmax(-1)
    for b in range(B):
        assert torch.all(c["sigma"][b, : first[b]] <= 0)
    if S >= 63:
        assert 0 <= T[0].min() < FLT_MIN
        assert (c["sigma"] == 0).any() and (c["sigma"] < 0).any()
    n = c["rd"].norm(dim=-1)
    assert torch.all((n >= 0.5) & (n <= 2.0))


@pytest.mark.parametrize("B", ei.COMPOSITE_B)
@pytest.mark.parametrize("S", [s for s in ei.COMPOSITE_S if s >= 2])
def test_ties_regime_has_zero_deltas(S, B):
    z = ei.composite_inputs(S, B, "ties")["z"]
    delta = z[:, 1:] - z[:, :-1]
    assert torch.all(delta >= 0)
    assert torch.all(delta[:, 0] == 0) and torch.all(delta[:, -1] == 0)
    if S >= 63:
        assert (delta[:, 1:-1] == 0).any() and (delta > 0).any()


def test_random_regime_has_dead_samples():
    """sigma + noise <= 0 somewhere (where g_sigma must be exactly 0) and > 0 elsewhere."""
    c = ei.composite_inputs(65, 5, "random")
    s = c["sigma"] + c["noise"]
    assert (s <= 0).any() and (s > 0).any()


@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("S,B,white,regime", ei.COMPOSITE_CASES)
def test_composite_oracle32_error_is_a_yardstick(S, B, white, regime, with_g):
    """The fp32 oracle against the fp64 one, per output: finite, and either exactly zero
    (the floor of ``yardstick_bound`` then carries the bound) or positive; both oracles are
    finite in every regime, and g_sigma is exactly 0 on dead samples in both."""
    c = ei.composite_inputs(S, B, regime)
    w64 = ei.composite_oracle(c, white, with_g, torch.float64)
    w32 = ei.composite_oracle(c, white, with_g, torch.float32)
    dead = (c["sigma"] if c["noise"] is None else c["sigma"] + c["noise"]) <= 0
    for k in w64:
        assert torch.isfinite(w64[k]).all() and torch.isfinite(w32[k]).all(), k
        e = ei.distance(k, w32[k], w64[k])
        assert math.isfinite(e) and e >= 0.0, (k, e)
        assert ei.yardstick_bound(16, e, w64[k]) >= 0.0
    assert torch.count_nonzero(w64["g_sigma"][dead]) == 0 and torch.count_nonzero(w32["g_sigma"][dead]) == 0


@pytest.mark.parametrize("Nb", ei.PDF_SPIKE_NB)
def test_spike_weights_keep_a_share_of_live_buckets(Nb):
    """More than 0.3 of the u (given and linspace) fall into buckets with denom >= 1e-5 in
    the oracle, and none into a bucket within 10 % of that threshold, where fp32 and fp64
    could take different sides of the ``denom < 1e-5 -> 1`` rule."""
    bins, w, u = ei.pdf_spike_inputs(Nb)
    assert w.shape == (ei.PDF_SPIKE_B, Nb - 1)
    assert torch.count_nonzero(w[:2]) == 0 and torch.all((w[2:] == 100.0).sum(-1) == 1)
    for uu in (u, ei.linspace_u(ei.PDF_SPIKE_B, ei.PDF_SPIKE_NS)):
        den = ei.pdf_bucket_denominators(w, uu)
        assert (den >= 1e-5).double().mean() > 0.3
        assert not ((den > 0.9e-5) & (den < 1.1e-5)).any()
    assert (den < 1e-5).any()  # linspace's u = 1 sits past the last bucket: a degenerate one is there


@pytest.mark.parametrize("precision,M", [("fp32", m) for m in ei.REF32_M] + [(p, m) for p in ("bf16", "fp16")
                                                                               for m in ei.REF16_M])
def test_kink_free_selection_keeps_enough(precision, M):
    x, d, survivors = ei.mlp_selected(precision, M)
    assert survivors >= M and x.shape == (M, 3) and d.shape == (M, 3)
    oracle = ei.oracle_net(precision)
    if precision == "fp32":
        assert torch.all(ei.kink_free(oracle, x, d, 2e-6))
        return
    assert torch.all(ei.model_kink_free(oracle, precision, x, d, 1e-5))
    assert not ei.sine_sensitive(oracle, precision, x, d).any()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_model_preactivations_are_the_numerics_models(precision):
    """edge_inputs.model_preactivations restates the numerics model's forward to expose its
    pre-activations: its outputs equal the model's own bit for bit, and sigma / the hidden
    units are the ReLU of what it returns."""
    from oracle import refimpl as ref
    oracle = ei.oracle_net(precision)
    x, d = ei.mlp_candidates(300, seed=3)
    emu = ref.mfma_emulated_nerf(oracle, precision)
    with torch.no_grad():
        pre, rgb, sigma = ei.model_preactivations(emu, x, d)
        er, es = emu(x, d)
    assert torch.equal(rgb, er) and torch.equal(sigma, es)
    assert len(pre) == oracle.config.num_hidden_layers + 2 and torch.equal(torch.relu(pre[-2]), es)


def test_scene_scale_positions():
    x, _ = ei.mlp_candidates(513, seed=900, lo=4.0, hi=8.0)
    assert torch.all((x.abs() >= 4.0) & (x.abs() <= 8.0)) and (x < 0).any() and (x > 0).any()
    assert (512 * x.abs().max() / (2 * math.pi)) > 600  # revolutions at the top frequency


# ------------------------------------------- the boundary configs (test_mlp_configs.py) --
CONFIG_PARAMS = [(c, m, p) for c, m in ei.CONFIG_RUNS for p in ei.CONFIG_PRECISIONS]


@pytest.mark.parametrize("case,M,precision", CONFIG_PARAMS)
def test_config_case_inputs_reach_the_edge(case, M, precision):
    """Per (case, precision, M) of test_mlp_configs: at least M of the 3 M + 64 candidates
    survive the selection and the M taken are kink-free (and not sine-sensitive) against the
    reference of that precision; the reference is finite; every named parameter's reference
    gradient, g_x and g_d are nonzero; for the encoding with a lone live column in its
    second block, the gradient with respect to that column is nonzero in every layer that
    reads x_enc."""
    c = ei.config_case(case, precision, M)
    x, d, want = c["x"], c["d"], c["want"]
    assert c["survivors"] >= M and x.shape == (M, 3) and d.shape == (M, 3)
    oracle = ei.oracle_net(precision, case=case)
    cfg = oracle.config
    assert len(oracle.pts_linears) == cfg.num_hidden_layers
    if precision == "fp32":
        assert torch.all(ei.kink_free(oracle, x, d, 2e-6))
    else:
        assert torch.all(ei.model_kink_free(oracle, precision, x, d, 1e-5))
        assert not ei.sine_sensitive(oracle, precision, x, d).any()
    assert (want["g_d"] is not None) == bool(cfg.use_view_dirs)
    for k in ("rgb", "sigma", "g_x", "g_d"):
        if want[k] is not None:
            assert torch.isfinite(want[k]).all() and want[k].abs().max() > 0, k
    assert len(want["grads"]) == 2 * (cfg.num_hidden_layers + 4)
    for name, g in want["grads"]:
        assert torch.isfinite(g).all() and g.norm() > 0, name
    col = ei.live_column(case)
    assert (col == 32) == (case == "pos5_dir3")
    if col is not None:
        readers = [0] + [s + 1 for s in cfg.skips]
        for name, g in want["grads"]:
            if name in [f"pts_linears.{i}.weight" for i in readers]:
                assert g[:, col].norm() > 0, name
    # the reference is at distance zero from itself under every norm the GPU test uses
    dist = ei.config_distances(want, want, case)
    assert max(dist.values()) == 0.0 and not ei.check_config_distances(dist, precision, 1.0)
    if col is not None:
        assert any(k.endswith(f"[:, {col}]") for k in dist)


def _mutated_reference(case, precision, M, mutation, c=None):
    """The reference outputs of a mutated copy of the oracle on the test's own inputs
    (``c``: the inputs of another generator on the same model)."""
    import copy
    from oracle import refimpl as ref
    c = ei.config_case(case, precision, M) if c is None else c
    net = copy.deepcopy(ei.oracle_net(precision, case=case))
    cfg = copy.copy(net.config)
    x, d, g_rgb, g_sigma = c["x"], c["d"], c["g_rgb"], c["g_sigma"]
    if mutation == "drop_live_column":  # the lone column of the second encoding block reads as zero
        col = ei.live_column(case)

        class Enc(torch.nn.Module):
            def __init__(self, enc):
                super().__init__()
                self.enc, self.output_dim = enc, enc.output_dim

            def forward(self, v):
                e = self.enc(v)
                keep = torch.ones(e.shape[-1], dtype=e.dtype)
                keep[col] = 0
                return e * keep
        net.pos_encoder = Enc(net.pos_encoder)
    elif mutation == "swap_top_sin_cos":  # sine and cosine of the top frequency exchanged
        class Enc(torch.nn.Module):
            def __init__(self, enc):
                super().__init__()
                self.enc, self.output_dim = enc, enc.output_dim

            def forward(self, v):
                e = self.enc(v)
                n = e.shape[-1]
                idx = list(range(n - 6)) + list(range(n - 3, n)) + list(range(n - 6, n - 3))
                return e[..., idx]
        net.pos_encoder = Enc(net.pos_encoder)
    elif mutation == "omit_skip":  # the last skip concatenates zeros in place of x_enc
        s = max(cfg.skips)
        with torch.no_grad():
            net.pts_linears[s + 1].weight[:, : net.pts_linears[0].weight.shape[1]] = 0
    elif mutation == "zero_last_row":  # the tile of one sample computes nothing
        g_rgb, g_sigma = g_rgb.clone(), g_sigma.clone()
        g_rgb[-1] = 0
        g_sigma[-1] = 0
    elif mutation == "layer15_for_14":  # a weight image read one layer off
        with torch.no_grad():
            net.pts_linears[14].weight.copy_(net.pts_linears[15].weight)
            net.pts_linears[14].bias.copy_(net.pts_linears[15].bias)
    else:
        raise ValueError(mutation)
    out = ei.reference_outputs(net, precision, x, d, g_rgb, g_sigma)
    if mutation == "zero_last_row":
        out["rgb"][-1] = 0
        out["sigma"][-1] = 0
    return out


MUTATIONS = [("drop_live_column", "pos5_dir3", 33), ("swap_top_sin_cos", "pos5_dir3", 33),
             ("swap_top_sin_cos", "depth16_skip4", 33), ("omit_skip", "depth2_skip0", 33),
             ("omit_skip", "depth6_skips_1_2_4", 33), ("omit_skip", "depth3_skip1_no_view_dirs", 33),
             ("omit_skip", "depth16_skips_0_3_6_9_12", 513), ("zero_last_row", "pos0_dir0", 33),
             ("zero_last_row", "pos10_dir1", 33), ("zero_last_row", "depth16_skip4", 513),
             ("layer15_for_14", "depth16_skip4", 33), ("layer15_for_14", "depth16_skips_0_3_6_9_12", 33)]


@pytest.mark.parametrize("precision", ei.CONFIG_PRECISIONS)
@pytest.mark.parametrize("mutation,case,M", MUTATIONS)
def test_config_comparison_catches_a_wrong_kernel(mutation, case, M, precision):
    """test_mlp_configs can fail: a copy of the reference with one small wrong-kernel
    mutation (the lone live column dropped; sine and cosine of the top frequency swapped;
    one skip concatenation omitted; the last sample's row -- the tile of one -- zeroed;
    layer 15's weights used for layer 14) lies, on the test's own inputs and under its own
    norms, beyond the test's bounds.  The dropped column must also show in the norm of that
    column by itself (relative error 1), which does not depend on how large the rest of the
    matrix is."""
    c = ei.config_case(case, precision, M)
    mutant = _mutated_reference(case, precision, M, mutation)
    dist = ei.config_distances(mutant, c["want"], case)
    missed = ei.check_config_distances(dist, precision, c["want"]["sigma"].abs().max().item(), c["grad_bounds"])
    assert missed, (mutation, case, precision, max(dist.values()))
    # not the forward alone: the per-parameter gradient comparison (under its own bounds, the
    # 1.5 x twin ones included) and the input gradient catch it as well
    names = {name for name, _, _ in missed}
    assert any(n.startswith(("pts_linears", "feature", "dir_", "rgb_", "sigma_")) for n in names), missed
    assert names & {"g_x", "g_x[-1]"}, missed
    if mutation == "drop_live_column":
        assert any(name.endswith("[:, 32]") for name, _, _ in missed), missed


@pytest.mark.parametrize("case,M,precision", [p for p in CONFIG_PARAMS if p[2] != "fp32"])
def test_config_gradient_bounds_widen_only_where_the_model_is_ill_conditioned(case, M, precision):
    """edge_inputs.ILL_CONDITIONED is a static list: trunk layers 0..2 of the depth-16 cases in
    fp16.  The numerics model's own twin (another summation order, same roundings) justifies
    it: at every listed parameter the twin is farther than 1.5e-2 from the model, so no
    implementation can be asked for 1.5e-2 there; the bound, 1.5 x the twin's distance, stays
    below the model's distance from the fp64 oracle on the same samples; at every parameter
    off the list the bound is 1.5e-2 and the twin is within 1.7e-2 of the model (it exceeds
    1.5e-2 only at layer 10 of depth16_skip4, M = 513, bf16: 0.0157).  The mechanism: the
    stored dz 2^14 of the listed layers is an fp16 subnormal throughout."""
    c = ei.config_case(case, precision, M)
    listed = set(ei.ill_conditioned_names(case, precision))
    want = {f"pts_linears.{i}.{k}" for i in range(3) for k in ("weight", "bias")}
    assert listed == (want if precision == "fp16" and case.startswith("depth16") else set())
    assert set(c["grad_bounds"]) == listed
    for name, bound in c["grad_bounds"].items():
        assert c["twin"][name] > 1.5e-2, (name, c["twin"][name])
        assert bound == 1.5 * c["twin"][name] and 1.5e-2 < bound < 1.0 * c["oracle"][name] < 0.25, (name, bound)
    assert max(v for k, v in c["twin"].items() if k not in listed) < 1.7e-2
    if listed:
        from oracle import refimpl as ref
        seen = []
        orig = ref._GradRound.backward

        def spy(ctx, g):
            seen.append((g * ctx.scale).abs().max().item())
            return orig(ctx, g)
        ref._GradRound.backward = staticmethod(spy)
        try:
            ei.reference_outputs(ei.oracle_net(precision, case=case), precision, c["x"], c["d"], c["g_rgb"], c["g_sigma"])
        finally:
            ref._GradRound.backward = staticmethod(orig)
        assert len(seen) == 18 and max(seen[-3:]) < 2.0 ** -14  # backward order: layers 2, 1, 0 come last


@pytest.mark.parametrize("case", [None, *ei.CONFIG_CASES])
def test_sigma_head_is_alive_with_the_static_flip_list(case):
    """edge_inputs.SIGMA_HEAD_NEGATED names the cases whose oracle has the sigma head negated:
    with the list as it stands sigma is positive on at least a quarter of a probe set in
    every case; the listed cases are dead (share 0) without the flip, and no other case is
    below a quarter without it."""
    from oracle import refimpl as ref
    assert set(ei.SIGMA_HEAD_NEGATED) == {"depth16_skip4", "depth16_skips_0_3_6_9_12"}
    assert ei.sigma_alive_share(ei.oracle_net("fp32", case=case)) >= 0.25
    torch.manual_seed(0)
    plain = ei.sigma_alive_share(ref.NeRF(ei.case_config("fp32", case)))
    assert (plain == 0.0) if case in ei.SIGMA_HEAD_NEGATED else (plain >= 0.25)


# --------------------------------------------------- scene scale (section 3) --
@pytest.mark.parametrize("precision", ei.CONFIG_PRECISIONS)
def test_scene_case_inputs(precision):
    """At least 513 of the 1603 candidates with |x| in 4 .. 10 survive the selection, the 513
    taken are kink-free (16 bit: and not sine-sensitive) in that band, beyond 600 revolutions
    at the top frequency, and the reference's g_x, g_d and the gradients of the layers that
    read x_enc are finite and nonzero."""
    c = ei.scene_case(precision)
    x, d, want = c["x"], c["d"], c["want"]
    assert c["survivors"] >= ei.SCENE_M and x.shape == (ei.SCENE_M, 3)
    assert torch.all((x.abs() >= 4.0) & (x.abs() <= 10.0)) and x.abs().max() > 9.9 and (x < 0).any() and (x > 0).any()
    assert 512 * x.abs().max() / (2 * math.pi) > 800
    oracle = ei.oracle_net(precision)
    if precision == "fp32":
        assert torch.all(ei.kink_free(oracle, x, d, 2e-6))
    else:
        assert torch.all(ei.model_kink_free(oracle, precision, x, d, 1e-5))
        assert not ei.sine_sensitive(oracle, precision, x, d).any()
    grads = dict(want["grads"])
    for g in [want["g_x"], want["g_d"], *[grads[n] for n in ei.SCENE_PARAMS]]:
        assert torch.isfinite(g).all() and g.norm() > 0
    assert grads["pts_linears.5.weight"].shape[1] == 63 + 256  # the layer after the skip reads x_enc
    assert max(ei.scene_distances(want, want).values()) == 0.0


@pytest.mark.parametrize("precision", ei.CONFIG_PRECISIONS)
@pytest.mark.parametrize("mutation", ["swap_top_sin_cos", "omit_skip", "zero_last_row"])
def test_scene_comparison_catches_a_wrong_kernel(mutation, precision):
    """The scene-scale comparison can fail: the mutated reference misses its bounds, in g_x
    for the encoding mutation and in a parameter gradient for each."""
    c = ei.scene_case(precision)
    mutant = _mutated_reference(None, precision, ei.SCENE_M, mutation, c)
    missed = ei.check_config_distances(ei.scene_distances(mutant, c["want"]), precision, 1.0)
    names = {name for name, _, _ in missed}
    assert names & set(ei.SCENE_PARAMS), (mutation, missed)
    if mutation == "swap_top_sin_cos":
        assert "g_x" in names, missed


# ------------------------------- the fp16 gradient magnitudes (section 4) --
def _model_is_finite(want, stored):
    return all(torch.isfinite(v).all() for v in stored) and all(torch.isfinite(g).all() for _, g in want["grads"]) \
        and torch.isfinite(want["g_x"]).all() and torch.isfinite(want["g_d"]).all()


@pytest.mark.parametrize("M", ei.FP16_SCALE_M)
@pytest.mark.parametrize("B,outlier", ei.FP16_SCALE_RUNS)
def test_fp16_model_is_finite_across_gradient_magnitudes(B, outlier, M):
    """At every magnitude of test_fp16_backward_across_gradient_magnitudes the numerics model
    (dz scaled by 2^14 and stored in fp16) keeps every stored dz -- the ten MFMA layers' and
    the two heads' -- and every gradient finite, and no layer's stored dz is flushed to all
    zeros; so no scale is left out of the GPU list.  The selection keeps enough samples and
    the outlier is 1e4 times the typical g_sigma."""
    assert set(ei.FP16_BATCHES) == {65536, 4096, 512, 64, 8} and (4096, True) in ei.FP16_SCALE_RUNS
    c = ei.fp16_scale_case(M, B, outlier)
    assert c["survivors"] >= M and len(c["stored"]) == 12
    assert _model_is_finite(c["want"], c["stored"])
    for v in c["stored"]:
        assert v.dtype == torch.float16 and torch.count_nonzero(v) > 0
    assert max(v.float().abs().max().item() for v in c["stored"]) < ei.FP16_MAX
    if outlier:
        g = c["g_sigma"].abs().reshape(-1)
        assert g.max() == g[M // 2] and g.max() > 1e3 * g.median()
    for _, g in c["want"]["grads"]:
        assert g.norm() > 0


def test_fp16_model_finite_range():
    """The range written into test_fp16_backward_across_gradient_magnitudes and DESIGN.md:
    the model is finite while the largest |g_sigma| 2^14 rounds to a finite fp16 number
    (|g_sigma| < 65520 / 2^14 = 3.999) and overflows just beyond it; downwards no layer's
    stored dz is all zero at 2^-14 of the 4096-ray magnitude (1e-8)."""
    M = 513
    x, d, _ = ei.mlp_selected("fp16", M)
    g_rgb, g_sigma = ei.mlp_upstream(M, seed=70 + M, scale=1.0)
    top = g_sigma.abs().max().item()
    for peak, finite in ((3.9, True), (4.1, False)):
        want, stored = ei.fp16_model_run(x, d, g_rgb * (peak / top), g_sigma * (peak / top))
        assert _model_is_finite(want, stored) == finite, peak
    tiny = 2.0 / (3 * 4096) * 2.0 ** -14
    want, stored = ei.fp16_model_run(x, d, g_rgb * tiny, g_sigma * tiny)
    assert _model_is_finite(want, stored) and all(torch.count_nonzero(v) > 0 for v in stored)
