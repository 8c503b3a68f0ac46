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
