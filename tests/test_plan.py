"""The fused-MLP layout plan, checked on the host: the dW jobs' wave shares cover every
parameter's gradient exactly once (tests/native/plan_check.cpp compiles the plan
source robust-nerf_amd/csrc/mlp_plan.cpp.inc with g++; no GPU)."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("plan") / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'robust-nerf_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "plan_check.cpp"),
                    "-o", str(exe)], check=True)
    return exe


# pos_freqs dir_freqs n_layers skip_mask use_view_dirs precision
CONFIGS = [(10, 4, 8, 1 << 4, 1, 1), (10, 4, 8, 1 << 4, 1, 0), (10, 4, 8, 1 << 4, 1, 2), (10, 4, 8, 1 << 4, 0, 1),
           (6, 2, 4, 1 << 1, 1, 1), (10, 4, 12, (1 << 3) | (1 << 7), 1, 1), (4, 1, 1, 0, 1, 1),
           # two and more skips: x-jobs of more than two dz layers exceed the dW staging
           (10, 4, 7, (1 << 2) | (1 << 5), 1, 1), (10, 4, 7, (1 << 2) | (1 << 5), 1, 0),
           (10, 4, 7, (1 << 2) | (1 << 5), 1, 2), (10, 4, 10, 0b10101010, 1, 1), (10, 4, 8, 0b100100, 1, 0)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_every_parameter_gradient_written_once(plan_check, cfg):
    r = subprocess.run([str(plan_check), *map(str, cfg)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unwritten 0 doubly written 0" in r.stdout
    assert "dW workgroup plan bad 0" in r.stdout


def test_too_many_dw_jobs_fails_cleanly(plan_check):
    """16 layers with a skip after every one: more dW jobs than the kernel arguments
    hold -- the plan refuses the config instead of overrunning its job table."""
    r = subprocess.run([str(plan_check), "10", "4", "16", str((1 << 15) - 1), "1", "1"], capture_output=True, text=True)
    assert r.returncode != 0 and "plan fail" in r.stdout, r.stdout


def _sweep_masks(n):
    """plan_check.cpp's valid skip masks at depth n (those below bit n - 1)."""
    full = (1 << (n - 1)) - 1 if n >= 2 else 0
    masks = {0, full & 0x55555555, full & 0xAAAAAAAA, full}
    for i in range(n - 1):
        masks.add(1 << i)
        masks.add((1 << i) | (1 << (n - 2)))
        if i + 2 < n:
            masks.add(3 << i)
    return masks


def test_sweep_of_the_whole_config_space(plan_check):
    """``plan_check --sweep`` in one process: pos_freqs 0..11, dir_freqs 0..5, depth 0..17,
    both view-direction settings, three precisions and per depth the skip masks none /
    singles / adjacent pairs / every other / all / pairs with n-2 / bits at n-1 and above.
    Every accepted config passes the single-config checks (each gradient written once,
    shares inside their grids and the staging limit, a good workgroup plan) with its job,
    reduce and fp32 weight-stream tables inside kMaxJobs / kMaxRed / kMaxChunks; every
    refusal has a reason; nothing outside the stated envelope is accepted; and the refused
    configs inside it are exactly those the refusal message names: num_hidden_layers +
    ceil((len(skips) + 1) / 2) > 23 (22 in fp32), here the all-skips masks at depth 16 and,
    in fp32, depth 15."""
    import time
    t0 = time.perf_counter()
    r = subprocess.run([str(plan_check), "--sweep"], capture_output=True, text=True)
    dt = time.perf_counter() - t0
    lines = r.stdout.splitlines()
    print(f"PLAN_SWEEP seconds {dt:.1f}: {lines[-2]}; {lines[-1]}")
    assert r.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")], "\n".join(lines[-20:])
    want = set()
    n_valid = 0
    for n in range(1, 17):
        for mask in _sweep_masks(n):
            for prec in (0, 1, 2):
                limit = 22 if prec == 0 else 23
                for pos in range(11):
                    for dirf in range(5):
                        for vd in (0, 1):
                            n_valid += 1
                            if n + (bin(mask).count("1") + 2) // 2 > limit:
                                want.add((pos, dirf, n, mask, vd, prec))
    got = set()
    for ln in lines:
        if ln.startswith("refused "):
            cfg, why = ln[len("refused "):].split(":", 1)
            assert "dW job shares exceed the 8-wave workgroup" in why and "23, or 22 in fp32" in why, ln
            got.add(tuple(map(int, cfg.split())))
    assert got == want and len(want) == 440
    assert {(n, m, p) for _, _, n, m, _, p in want} == {(16, 0x7FFF, 0), (16, 0x7FFF, 1), (16, 0x7FFF, 2),
                                                         (15, 0x3FFF, 0)}
    tot = dict(zip(lines[-2].split()[1::2], map(int, lines[-2].split()[2::2])))
    assert tot["failures"] == 0 and tot["refused_valid"] == 440 and tot["accepted"] == n_valid - 440
    assert tot["total"] == tot["accepted"] + tot["refused_valid"] + tot["refused_invalid"]
    assert lines[-1] == "sweep max n_jobs 24 of 24 n_red 20 of 20 fwd_chunks 159 bwd_chunks 140 of 176"


# the models of tests/test_tile_patterns.py (edge_inputs.OTHER_MODELS and the default one):
# n_layers, skip_mask, use_view_dirs
TILE_PATTERN_MODELS = {"default": (8, 1 << 4, 1), "depth16_skips_0_3_6_9_12": (16, 0b1001001001001, 1),
                       "depth3_skip1_no_view_dirs": (3, 1 << 1, 0), "depth2_skip0": (2, 1 << 0, 1)}


@pytest.mark.parametrize("prec", [0, 1, 2], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("model", list(TILE_PATTERN_MODELS))
def test_tile_pattern_sizes_stage_the_dw_list_in_lds(plan_check, model, prec):
    """``plan_check --list-lds``: at the two sizes of test_tile_patterns.py (10,245 and 20,485
    samples: 321 tiles in two segments, 641 in three) every model that file runs copies its dW
    chunk's list entries into LDS (list_lds != 0), so the form that reads the list from global
    memory is none of its cases; and the dW chunks per job at M = 10,245 are the ones its
    count sweeps are built around (tiles // 16 = 20 caps them)."""
    n, mask, vd = TILE_PATTERN_MODELS[model]
    r = subprocess.run([str(plan_check), "--list-lds", "10", "4", str(n), str(mask), str(vd), str(prec), "10245", "20485"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [dict(zip(ln.split()[0:8:2], map(int, ln.split()[1:8:2])), chunks=list(map(int, ln.split()[9:])))
            for ln in r.stdout.splitlines()]
    assert [(w["M"], w["tiles"], w["nseg"]) for w in rows] == [(10245, 321, 2), (20485, 641, 3)]
    assert all(w["list_lds"] > 0 for w in rows), rows
    chunks = set(rows[0]["chunks"])
    if model == "depth16_skips_0_3_6_9_12":
        assert len(rows[0]["chunks"]) == 20 + (prec == 0) and chunks == ({7, 13, 14} if prec == 0 else {12})
    else:
        assert chunks == {20}
    assert max(rows[1]["chunks"]) <= 641 // 16


def test_where_the_global_dw_list_begins(plan_check):
    """The default model's first M at which the dW list no longer fits in LDS beside the
    staging ring (list_lds == 0), the figure test_tile_patterns.py's docstring gives: 49,921
    tiles in fp32, 96,001 in 16 bit."""
    for prec, first in ((0, 1_597_441), (1, 3_072_001), (2, 3_072_001)):
        r = subprocess.run([str(plan_check), "--list-lds", "10", "4", "8", "16", "1", str(prec), str(first - 1), str(first)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        below, at = [int(ln.split()[7]) for ln in r.stdout.splitlines()]
        assert below > 0 and at == 0, r.stdout
