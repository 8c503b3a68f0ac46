"""GPU: the skipping MLP backward on structured active-tile patterns, against a reference.

test_tile_skip.py holds the skipping backward to the dense form of the same kernels on a
random 60 % of dead tiles at M in the thousands.  Here the active tiles are placed where
the index work of tile_flags_kernel, select_tile / seg_scan / seg_entry, place_segment and
mlp_dw_kernel's chunk split can go wrong -- on a flag-word, 64-tile-block or 256-tile-segment
boundary, with a whole segment empty, with W - 1 / W / W + 1 active tiles in a segment (W = 8
waves in 16 bit, 4 in fp32), with fewer active tiles than dW chunks -- and the gradients are
compared with a reference that shares nothing with the kernels: a sample whose upstream
gradient is zero contributes exactly nothing, so the reference of a pattern is
edge_inputs.reference_outputs on the active samples alone (fp64 autograd of the oracle for
fp32, the numerics model for bf16 / fp16), on kink-free samples (edge_inputs.tile_case; in
16 bit also without the samples at which the numerics model itself is unstable to a 16-bit
rounding flip, edge_inputs.jitter_fragile, where it is no reference to 1.5e-2).

Sizes, the smallest at which each mechanism exists: M_A = 10,245 (321 tiles in two segments;
segment 1 is one full 64-tile block and a block with a single tile of 5 samples) and
M_B = 20,485 (641 tiles in three segments; segment 2 has 129 tiles, its fourth block empty).
tests/test_plan.py asserts with plan_check that every model used here stages the dW list in
LDS at both sizes; the form that reads it from global memory (list_lds == 0) begins, for the
default model, at M = 1,597,441 in fp32 and 3,072,001 in 16 bit and is not run here, nor is
the form past kDenseCheckSegs (M > 8.4M: test_tile_skip.test_launch_past_the_dense_check).

Bounds, the project's own: fp32 2e-5 relative per named parameter and on g_x, g_d; 16 bit
1.5e-2 per parameter, rgb 1e-4, sigma 1e-3 max(1, |sigma|); the non-default models
edge_inputs.config_bounds.  Upstream magnitudes as test_mlp_ragged: 1 in fp32, a mean loss
over 4096 rays in 16 bit.  Beside the reference every case asserts: the count left in the
workspace equals the host's count of tiles with any ``!= 0`` component; g_x / g_d
bit-identical to a dense_backward = 1 run of the same inputs and exactly zero on every
inactive sample; g_params within test_tile_skip's 1e-5 of the dense run; guard rows
untouched.  Every skipping run has 0xFF-filled saved / workspace and NaN behind row M.
test_edge_inputs_host.py asserts on the CPU that the patterns are what their names say and
that the comparison has teeth: zeroing one active tile's upstream gradient moves some
parameter's reference gradient by more than 3e-2, twice the loosest bound.

Which values count as zero (test_zero_rule): -0.0 is zero, an fp32 denormal and a NaN
(test_tile_skip.test_nan_gradient_keeps_its_tile) are not; the hardware agrees with the
host's ``!= 0`` on both, so neither tile_flags_kernel nor DESIGN.md's rule changed.

Distances are printed as ``EDGE_PARITY`` lines (profiles/tile_pattern_parity.json)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
from test_edge_shapes import _record  # noqa: E402
from test_mlp_ragged import (_buffers, _padded, _results, _run, _run_on, _same_bits, active_tile_count,  # noqa: E402
                             mlp_raw)

pytestmark = pytest.mark.gpu
NAN = float("nan")
OUTPUTS = ("rgb", "sigma", "g_x", "g_d", "g_params")


def _skipping(precision, M, c, case=None):
    return _run(precision, M, c["x"], c["d"], c["g_rgb"], c["g_sigma"], tail=NAN, poison=True, dense=0, case=case)


def _check_against_dense(c, precision, M, got, case=None):
    """The assertions every case makes beside the reference -> the dense run."""
    dense = _run(precision, M, c["x"], c["d"], c["g_rgb"], c["g_sigma"], tail=NAN, poison=True, dense=1, case=case)
    assert dense["count"] == ei.n_tiles(M)
    assert got["count"] == c["count"], (got["count"], c["count"])  # the host's count, not the kernel's flags
    quiet = ~c["active"].repeat_interleave(ei.TILE)[:M]
    for k in ("rgb", "sigma", "g_x", "g_d"):
        if k in got:
            assert torch.isfinite(got[k]).all(), k
            assert _same_bits(got[k], dense[k]), (k, (got[k] - dense[k]).abs().max().item())
    for k in ("g_x", "g_d"):
        if k in got:
            assert torch.count_nonzero(got[k][quiet]) == 0, k
    assert torch.isfinite(got["g_params"]).all()
    if c["count"] == 0:
        assert torch.count_nonzero(got["g_params"]) == 0 and torch.count_nonzero(dense["g_params"]) == 0
    else:
        rel = ((dense["g_params"] - got["g_params"]).norm() / dense["g_params"].norm()).item()
        assert rel < 1e-5, rel
    return dense


def _check_against_reference(c, precision, M, got, case, pattern):
    """The active rows of ``got`` and its parameter gradients against c["want"]."""
    want, rows = c["want"], c["rows"]
    assert ("g_d" in got) == (want["g_d"] is not None)
    grads, off = [], 0
    for name, w in want["grads"]:
        grads.append((name, got["g_params"][off:off + w.numel()].reshape(w.shape)))
        off += w.numel()
    assert off == got["g_params"].numel()
    on_rows = {k: got[k][rows] for k in ("rgb", "sigma", "g_x", "g_d") if k in got}
    dist = ei.config_distances(dict(on_rows, grads=grads), want, case)
    worst = max((k for k in dist if k not in ("rgb", "sigma")), key=dist.get)
    _record(test="mlp_tile_pattern_vs_reference", pattern=pattern, model=case, precision=precision, M=M,
            count=c["count"], samples=c["A"], rgb=dist["rgb"], sigma=dist["sigma"], g_x=dist["g_x"], g_d=dist.get("g_d"),
            max_rel=dist[worst], max_rel_at=worst)
    if case is None:
        # the default model's bars: the last-row distances are test_mlp_configs' own, and in
        # 16 bit g_x / g_d are held to the dense run bit for bit rather than to the model
        drop = ("g_x[-1]", "g_d[-1]") + (() if precision == "fp32" else ("g_x", "g_d"))
        dist = {k: v for k, v in dist.items() if k not in drop}
    grad_bounds = None
    if ei.ill_conditioned_names(case, precision):
        _, _, grad_bounds = ei.model_conditioning(ei.oracle_net(precision, case=case), precision, c["x"][rows], c["d"][rows],
                                                  c["g_rgb"][rows], c["g_sigma"][rows], want,
                                                  ei.ill_conditioned_names(case, precision))
    missed = ei.check_config_distances(dist, precision, want["sigma"].abs().max().item(), grad_bounds)
    assert not missed, missed


def _check_case(c, precision, M, pattern, case=None):
    got = _skipping(precision, M, c, case)
    _check_against_dense(c, precision, M, got, case)
    if c["want"] is not None:
        _check_against_reference(c, precision, M, got, case, pattern)
    return got


# --------------------------------------------------------- 1. named patterns --
@pytest.mark.parametrize("precision", ei.TILE_PRECISIONS)
@pytest.mark.parametrize("name", ei.NAMED_PATTERNS)
def test_named_pattern(name, precision):
    """The named sets of edge_inputs.named_tiles at M_B.  ``all_but_one`` (every tile except
    300) would need 20k selected samples for its reference: it is compared with the dense run
    only, as test_tile_skip's cases are."""
    c = ei.named_case(precision, name)
    assert (c["want"] is None) == (name == "all_but_one")
    _check_case(c, precision, ei.M_B, name)


# ------------------------------------------- 2. which values count as zero --
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(ei.ZERO_RULE_CASES))
def test_zero_rule(name, precision):
    """M_A.  Three tiles are active through one component of one sample only (g_sigma of
    sample 31 of tile 7, g_rgb[:, 2] of sample 0 of tile 256, g_sigma of the last valid row):
    count 3, and the three samples' gradients are the reference's.  With a tile whose upstream
    gradient is -0.0 throughout the count stays 3 and that tile's g_x / g_d are exactly zero;
    with a tile whose only nonzero is 1e-42, an fp32 denormal, the count is 4 -- the host's
    ``!= 0`` in both."""
    c = ei.zero_rule_case(precision, name)
    assert c["count"] == (4 if name == "denormal_only_tile" else 3)
    got = _check_case(c, precision, ei.M_A, name)
    if name == "negative_zero_tile":
        sl = slice(130 * ei.TILE, 131 * ei.TILE)
        assert not c["active"][130] and torch.count_nonzero(got["g_x"][sl]) == 0
        assert torch.count_nonzero(got["g_d"][sl]) == 0


# ------------------------------------------------------------ 3. count sweep --
@pytest.mark.parametrize("precision", ei.TILE_PRECISIONS)
@pytest.mark.parametrize("count", ei.SWEEP_COUNTS)
def test_count_sweep(count, precision):
    """1 .. 41 active tiles at M_A, activated in a fixed order (tiles 320, 255, 256, 0, then a
    seeded permutation).  41 = 2 (tiles // 16) + 1 and tiles // 16 = 20 caps the dW chunks per
    job, so the sweep crosses count < chunks, = chunks, chunks + 1 and 2 chunks +- 1 for every
    job's chunk count (20 for every job of the default model at this size): chunks without a
    list entry must write a slab of zeros over the 0xFF bytes the reduction would read."""
    c = ei.tile_case(precision, ei.M_A, ei.sweep_tiles(count))
    _check_case(c, precision, ei.M_A, "sweep")


# ----------------------------------------------------------- 4. other models --
@pytest.mark.parametrize("precision", ei.OTHER_MODEL_PRECISIONS)
@pytest.mark.parametrize("label,tiles", ei.other_model_sets(), ids=[s[0] for s in ei.other_model_sets()])
@pytest.mark.parametrize("case", ei.OTHER_MODELS)
def test_other_models(case, label, tiles, precision):
    """M_A with a real list on the models test_mlp_configs only runs with every tile active:
    depth 16 with five skips (three x-jobs; 12 chunks per job in 16 bit, 7 / 13 / 14 in fp32),
    depth 3 without view directions (no g_d; 20 chunks), depth 2 with a skip after layer 0
    (20 chunks); counts around each chunk count and its double, and the set (255, 256, 320)."""
    c = ei.tile_case(precision, ei.M_A, tiles, case)
    got = _check_case(c, precision, ei.M_A, label, case)
    assert ("g_d" in got) == (case != "depth3_skip1_no_view_dirs")


# ---------------------------------------------------------- 5. stale scratch --
def _sequence_cases(precision, M):
    return [(name, ei.named_case(precision, name, M, selected=False)) for name in ei.STALE_SEQUENCE]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_stale_scratch_sequence(precision):
    """M_B, saved / workspace / outputs allocated once and never refilled between: all-active,
    seg_edges, no tile active, one_full_segment, last_partial_only, all-active.  Each step sees
    the flags, block counts, list, count, slabs and outputs of the step before; its g_params,
    g_x, g_d and count equal, bit for bit, the same pattern on freshly 0xFF-filled buffers."""
    M = ei.M_B
    bufs = _buffers(precision, M, poison=True)
    for step, (name, c) in enumerate(_sequence_cases(precision, M)):
        got = _run_on(bufs, precision, M, c["x"], c["d"], c["g_rgb"], c["g_sigma"], tail=NAN, dense=0)
        fresh = _skipping(precision, M, c)
        assert got["count"] == fresh["count"] == c["count"], (step, name)
        for k in OUTPUTS:
            assert _same_bits(got[k], fresh[k]), (step, name, k, (got[k] - fresh[k]).abs().max().item())


# ----------------------------------------------------------- 6. graph replay --
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graph_replay_with_a_changing_active_set(precision):
    """M_A.  nr_mlp_forward + nr_mlp_backward_dx + _dw + _reduce captured once on one stream,
    on static buffers, with an all-nonzero upstream gradient (the capture takes the dense
    order; nothing is read back inside it); then, per pattern of the stale-scratch sequence,
    the upstream gradient is copied in and the graph replayed once: every output and the
    count equal the eager call's on fresh buffers, bit for bit.  This is what --graph training
    replays as the field converges."""
    M = ei.M_A
    cases = _sequence_cases(precision, M)
    first = cases[0][1]
    assert first["count"] == ei.n_tiles(M)
    bufs = _buffers(precision, M, poison=True)
    o = bufs["out"]
    x, d = _padded(first["x"], M, 3, NAN), _padded(first["d"], M, 3, NAN)
    g_rgb, g_sigma = _padded(first["g_rgb"], M, 3, NAN), _padded(first["g_sigma"], M, 1, NAN)

    def launch():
        mlp_raw(precision, M, x, d, g_rgb, g_sigma, rgb=o["rgb"].buf, sigma=o["sigma"].buf, saved=bufs["saved"],
                workspace=bufs["ws"], g_x=o["g_x"].buf, g_d=o["g_d"].buf, g_params=o["g_params"].buf, dense=0,
                read_count=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for step, (name, c) in enumerate(cases):
        assert torch.equal(c["x"], first["x"]) and torch.equal(c["d"], first["d"])  # only the upstream gradient changes
        g_rgb[:M].copy_(c["g_rgb"])
        g_sigma[:M].copy_(c["g_sigma"])
        graph.replay()
        torch.cuda.synchronize()
        got = _results(o, active_tile_count(precision, M, bufs["ws"]))
        eager = _skipping(precision, M, c)
        assert got["count"] == eager["count"] == c["count"], (step, name)
        for k in OUTPUTS:
            assert _same_bits(got[k], eager[k]), (step, name, k, (got[k] - eager[k]).abs().max().item())


# ------------------------------------------- 7. the input-gradient-only pair --
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ei.REFERENCE_PATTERNS)
def test_frozen_pair_on_named_patterns(name, precision):
    """nr_mlp_forward_frozen / nr_mlp_backward_input on the named patterns at M_B, frozen
    buffers 0xFF-filled and NaN behind row M: rgb, sigma, g_x, g_d bit-identical to the
    training pair's, which are the ones test_named_pattern holds to the reference; exactly
    zero g_x / g_d on every inactive sample."""
    from test_frozen_mlp import _assert_equal, _pair
    M = ei.M_B
    c = ei.named_case(precision, name)
    args = (precision, M, c["x"], c["d"], c["g_rgb"], c["g_sigma"])
    train = _pair(*args, frozen=False, dense=0)
    frozen = _pair(*args, frozen=True, dense=0, poison=True, tail=NAN)
    _assert_equal(frozen, train, name)
    tested = _skipping(precision, M, c)  # test_named_pattern's run
    quiet = ~c["active"].repeat_interleave(ei.TILE)[:M]
    for k in ("g_x", "g_d"):
        assert _same_bits(frozen[k], tested[k]), k
        assert torch.count_nonzero(frozen[k][quiet]) == 0 and torch.count_nonzero(frozen[k][~quiet]) > 0, k
