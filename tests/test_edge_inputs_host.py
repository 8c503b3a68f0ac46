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


# ------------------------------ active-tile patterns (test_tile_patterns.py) --
def _per(tiles, size):
    out = {}
    for t in tiles:
        out[t // size] = out.get(t // size, 0) + 1
    return out


def test_named_patterns_are_what_their_names_say():
    """The sizes, and per name the tile set with its active tiles per 256-tile segment, per
    64-tile block and per 4-tile flag word."""
    T, seg, blk, word = ei.n_tiles(ei.M_B), ei.SEG_TILES, ei.BLOCK_TILES, ei.WORD_TILES
    assert (ei.n_tiles(ei.M_A), ei.M_A % 32, ei.n_tiles(ei.M_B), ei.M_B % 32) == (321, 5, 641, 5)
    assert ei.n_tiles(ei.M_A) - seg == 65 and T - 2 * seg == 129  # segment 1 of M_A; segment 2 of M_B: 64 + 64 + 1 + 0
    nt = {n: ei.named_tiles(n) for n in ei.NAMED_PATTERNS}
    for n, t in nt.items():
        assert list(t) == sorted(set(t)) and 0 <= t[0] and t[-1] < T, n
    assert nt["first_only"] == (0,) and nt["last_partial_only"] == (640,)
    assert nt["seg_edges"] == (255, 256, 511, 512) and _per(nt["seg_edges"], seg) == {0: 1, 1: 2, 2: 1}
    assert nt["block_edges"] == (319, 320, 383, 384, 447, 448)
    assert _per(nt["block_edges"], seg) == {1: 6} and _per(nt["block_edges"], blk) == {4: 1, 5: 2, 6: 2, 7: 1}
    assert nt["word_edges"] == (3, 4, 7, 8, 12, 13, 14, 15, 16, 21, 26, 31)
    assert _per(nt["word_edges"], word) == {0: 1, 1: 2, 2: 1, 3: 4, 4: 1, 5: 1, 6: 1, 7: 1}
    assert [t % word for t in (16, 21, 26, 31)] == [0, 1, 2, 3]  # one tile at each byte position
    assert _per(nt["middle_only"], seg) == {1: 9}
    assert _per(nt["ends_only"], seg) == {0: 5, 2: 5} and 640 in nt["ends_only"]
    assert _per(nt["last_segment_empty"], seg) == {0: 5, 1: 5}
    for name, counts in (("per_part_3_4_5", (3, 4, 5)), ("per_part_7_8_9", (7, 8, 9))):
        assert _per(nt[name], seg) == dict(enumerate(counts))
        for s in range(3):  # spread over the segment: its first and its last tile, every block touched
            own = [t for t in nt[name] if t // seg == s]
            assert own[0] == s * seg and own[-1] == min(T, (s + 1) * seg) - 1
            assert len(_per(own, blk)) >= min(3, len(own))
    assert nt["one_full_segment"] == tuple(range(256, 512))
    assert nt["all_but_one"] == tuple(t for t in range(641) if t != 300)
    assert ei.REFERENCE_PATTERNS == [n for n in ei.NAMED_PATTERNS if n != "all_but_one"] and len(ei.NAMED_PATTERNS) == 12
    # the names that follow M, at M_A (the graph test's sequence)
    assert ei.named_tiles("seg_edges", ei.M_A) == (255, 256) and ei.named_tiles("last_partial_only", ei.M_A) == (320,)
    assert ei.named_tiles("one_full_segment", ei.M_A) == tuple(range(256))
    assert ei.named_tiles("all_active", ei.M_A) == tuple(range(321)) and ei.named_tiles("none_active", ei.M_A) == ()
    assert ei.STALE_SEQUENCE == ["all_active", "seg_edges", "none_active", "one_full_segment", "last_partial_only",
                                 "all_active"]


def test_sweep_order_and_counts():
    """Tiles 320, 255, 256, 0, then a permutation of the rest; counts 1 .. 41 = 2 (tiles // 16) + 1,
    which includes every other model's counts; (255, 256, 320) is the sweep's own first three."""
    order = ei.sweep_order()
    assert order[:4] == (320, 255, 256, 0) and sorted(order) == list(range(321))
    assert ei.SWEEP_COUNTS == list(range(1, 42)) and set(ei.OTHER_MODEL_COUNTS) <= set(ei.SWEEP_COUNTS)
    assert ei.sweep_tiles(3) == ei.OTHER_MODEL_SET == (255, 256, 320)
    assert ei.OTHER_MODEL_COUNTS == [1, 2, 7, 8, 9, 11, 12, 13, 14, 15, 19, 20, 21, 40, 41]
    assert [n for n in ei.OTHER_MODELS if n not in ei.CONFIG_CASES] == []


def _check_tile_case(c, precision, M, case=None, singles=0, kinks=False):
    """The scattered samples are the selected ones, in order; every other row has a zero
    upstream gradient; count and rows are what the tile set says."""
    rows, A = c["rows"], c["A"]
    partial = (ei.n_tiles(M) - 1) in c["tiles"]
    assert A == 32 * len(c["tiles"]) - (27 if partial else 0) + (A - ei.tile_rows(c["tiles"], M).numel())
    xs, ds, survivors = ei.tile_selected(precision, A + ei.SINGLES_SPARE * singles, case)
    assert survivors >= xs.shape[0] >= A and c["survivors"] == survivors
    if not singles:
        assert torch.equal(c["sel_x"], xs) and torch.equal(c["sel_d"], ds)
    for sx, sd in zip(c["sel_x"], c["sel_d"]):  # (single-component rows: A of the pool, see tile_case)
        assert ((xs == sx).all(-1) & (ds == sd).all(-1)).sum() == 1
    assert torch.equal(c["x"][rows], c["sel_x"]) and torch.equal(c["d"][rows], c["sel_d"])
    if kinks and A <= 1312:  # (the named patterns and the zero rule; the sweeps take the same path)
        oracle = ei.oracle_net(precision, case=case)
        if precision == "fp32":
            assert torch.all(ei.kink_free(oracle, c["sel_x"], c["sel_d"], 2e-6))
        else:
            assert torch.all(ei.model_kink_free(oracle, precision, c["sel_x"], c["sel_d"], 1e-5))
    other = torch.ones(M, dtype=torch.bool)
    other[rows] = False
    bx, bd = ei.mlp_candidates(M, seed=4000 + M)
    assert torch.equal(c["x"][other], bx[other]) and torch.equal(c["d"][other], bd[other])
    up = torch.cat([c["g_rgb"], c["g_sigma"]], -1)
    assert (up[rows] != 0).any(-1).all()
    quiet = up[other]
    assert ((quiet == 0) | (quiet.abs() == ei.DENORMAL)).all()
    assert c["count"] == int(c["active"].sum()) and c["active"].shape == (ei.n_tiles(M),)
    holding, active = set((rows // 32).tolist()), set(c["active"].nonzero().reshape(-1).tolist())
    denormal_only = set((torch.nonzero((up != 0).any(-1) & other).reshape(-1) // 32).tolist()) - holding
    assert holding <= active and active - holding == denormal_only  # (active without a reference row)


def _toothless(c, precision, case):
    """[(tile, largest move)] of teeth_tiles whose zeroed upstream moves no parameter's
    reference gradient by more than 3e-2: twice the loosest bound (1.5e-2), so a lost or a
    doubled tile cannot pass the comparison."""
    bad = []
    for t in ei.teeth_tiles(c):
        worst = max(ei.tile_moves(c, precision, case, t).values())
        if not worst > 3e-2:
            bad.append((t, worst))
    return bad


@pytest.mark.parametrize("precision", ei.TILE_PRECISIONS)
def test_named_pattern_cases_have_teeth(precision):
    """Every named pattern that is compared with the reference, at M_B: the builder's output
    is what it says, enough candidates survive the selection, and zeroing the first, a
    middle or the last active tile moves a parameter gradient of the reference by > 3e-2."""
    for name in ei.REFERENCE_PATTERNS:
        c = ei.named_case(precision, name)
        assert c["tiles"] == ei.named_tiles(name) and c["count"] == len(c["tiles"]), name
        assert c["active"].nonzero().reshape(-1).tolist() == list(c["tiles"]), name
        _check_tile_case(c, precision, ei.M_B, kinks=True)
        assert not _toothless(c, precision, None), name
    c = ei.named_case(precision, "all_but_one")
    assert c["want"] is None and c["count"] == 640 and not c["active"][300] and c["A"] == 640 * 32 - 27


@pytest.mark.parametrize("precision", ei.TILE_PRECISIONS)
def test_count_sweep_cases_have_teeth(precision):
    """Counts 1 .. 41 at M_A for the default model.  The smallest move over all counts and
    zeroed tiles: 0.068 (38 tiles) / 0.070 (16) / 0.069 (23) in fp32 / bf16 / fp16."""
    for n in ei.SWEEP_COUNTS:
        c = ei.tile_case(precision, ei.M_A, ei.sweep_tiles(n))
        assert c["count"] == n
        _check_tile_case(c, precision, ei.M_A)
        assert not _toothless(c, precision, None), n


@pytest.mark.parametrize("precision", ei.OTHER_MODEL_PRECISIONS)
@pytest.mark.parametrize("case", ei.OTHER_MODELS)
def test_other_model_cases_have_teeth(case, precision):
    """The three non-default models at M_A, every count of OTHER_MODEL_COUNTS and the set
    (255, 256, 320): the condition holds at every count (the smallest move is 0.052, depth 2
    in bf16 at 19 tiles), so no case's largest count was reduced."""
    for label, tiles in ei.other_model_sets():
        c = ei.tile_case(precision, ei.M_A, tiles, case)
        assert c["count"] == len(tiles)
        _check_tile_case(c, precision, ei.M_A, case)
        for k in ("g_x", "g_d"):
            assert (c["want"][k] is not None) == (k == "g_x" or case != "depth3_skip1_no_view_dirs")
        assert not _toothless(c, precision, case), (label, _toothless(c, precision, case))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_zero_rule_cases(precision):
    """Three tiles active through one component of one sample (g_sigma of a tile's sample 31,
    g_rgb[:, 2] of a tile's sample 0, g_sigma of row M - 1); a tile of -0.0 is not active on
    the host's ``!= 0`` and a tile whose only nonzero is 1e-42 (an fp32 denormal) is.  Each of
    the three single samples carries > 3e-2 of some parameter's reference gradient."""
    M = ei.M_A
    assert [(r // 32, r % 32, k) for r, k in ei.ZERO_SINGLES] == [(7, 31, 3), (256, 0, 2), (320, 4, 3)]
    assert ei.ZERO_SINGLES[2][0] == M - 1 and 0 < ei.DENORMAL < FLT_MIN
    assert torch.tensor(ei.DENORMAL, dtype=torch.float32) != 0  # not flushed on the host either
    want_active = {"single_components": [7, 256, 320], "negative_zero_tile": [7, 256, 320],
                   "denormal_only_tile": [7, 200, 256, 320]}
    for name in ei.ZERO_RULE_CASES:
        c = ei.zero_rule_case(precision, name)
        up = torch.cat([c["g_rgb"], c["g_sigma"]], -1)
        assert c["A"] == 3 and c["rows"].tolist() == [r for r, _ in ei.ZERO_SINGLES]
        for r, k in ei.ZERO_SINGLES:
            assert torch.count_nonzero(up[r // 32 * 32: r // 32 * 32 + 32]) == 1 and up[r, k] != 0
        assert c["active"].nonzero().reshape(-1).tolist() == want_active[name] and c["count"] == len(want_active[name])
        _check_tile_case(c, precision, M, singles=len(ei.ZERO_SINGLES), kinks=True)
        assert not _toothless(c, precision, None), name
        if name == "negative_zero_tile":
            t = up[130 * 32: 131 * 32]
            assert torch.all(t == 0) and torch.all(torch.signbit(t))
        if name == "denormal_only_tile":
            t = up[200 * 32: 201 * 32]
            assert torch.count_nonzero(t) == 1 and t[13, 3] == ei.DENORMAL


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_tile_moves_is_the_recomputed_reference(precision):
    """edge_inputs.tile_moves takes the reference of the zeroed tile's rows alone for the
    difference of the two references; here the reference IS recomputed with that tile's
    upstream gradient zeroed (per_part_3_4_5, its middle tile), and the two agree to 1e-3 of
    the move itself."""
    c = ei.named_case(precision, "per_part_3_4_5")
    tile = ei.teeth_tiles(c)[1]
    rows = c["rows"]
    g_rgb, g_sigma = c["g_rgb"].clone(), c["g_sigma"].clone()
    g_rgb[tile * 32: tile * 32 + 32] = 0
    g_sigma[tile * 32: tile * 32 + 32] = 0
    without = ei.reference_outputs(ei.oracle_net(precision), precision, c["x"][rows], c["d"][rows], g_rgb[rows], g_sigma[rows])
    moves = ei.tile_moves(c, precision, None, tile)
    for (n, g), (_, w) in zip(without["grads"], c["want"]["grads"]):
        literal = ei.rel(g, w)
        assert abs(literal - moves[n]) <= 1e-3 * moves[n] + 1e-7, (n, literal, moves[n])
    assert max(moves.values()) > 3e-2
