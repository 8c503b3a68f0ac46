"""The joint pose-optimisation step without a positional-encoding window against the same step
under a mid-schedule coarse-to-fine window (``NeRF.set_pe_window``), on one GPU.

The window costs the step two small launches per network pass: the fold of the window into the
packed images' encoding columns before each training forward (``nr_mlp_fold_window``) and the
scaling of the flat gradient's encoding columns after each backward (``nr_mlp_window_grad``),
plus, when the window changes, an in-place write of its weights.  This tool measures that cost.

Workload: bench.pose_opt_setup(800, 800) (BASELINE cfg #3), bf16 networks, 64 coarse + 128 fine
samples, every step optimising the poses.  Legs, each training its own copy of the model from
the same seed: ``off`` (no window), ``on`` (a window that stays at alpha = 0.34 L: ones, one
fractional weight, zeros) and ``moving`` (the window rewritten before every step, as a schedule
does during its ramp).  Cases: eager ``PoseTrainer`` at 1,024 and 4,096 rays, and the hipGraph
replay (``GraphedPoseTrainer``) at 512.  The legs of a case run in ONE process, alternating,
REPEATS times each; a run is WARMUP untimed steps, a device sync, STEPS timed steps over
pre-drawn pixel batches and a device sync.

Writes every run's ms/step to --out (default profiles/pe_window_ab.json) and prints one JSON line
per case.  There is no CPU path: without a GPU the tool fails.

python tools/pe_window_ab.py [--out FILE] [--steps 200] [--warmup 20] [--repeats 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]

CASES = (("eager", 1024), ("eager", 4096), ("graph", 512))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "pe_window_ab.json")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args(argv)
    if a.steps < 200 or a.warmup < 20 or a.repeats < 3:
        raise SystemExit("pe_window_ab: the protocol needs >= 200 timed steps, >= 20 warm-up steps and >= 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("pe_window_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")

    import bench
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import GraphedPoseTrainer, PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters, pe_window_weights

    dev = torch.device("cuda", 0)
    rc = RenderConfig(num_samples=64, num_samples_fine=128)
    cam0, sampler = bench.pose_opt_setup(800, 800, dev)

    def fixed(iteration, L):
        return pe_window_weights(0.34 * L, L)

    def moving(iteration, L):  # a different window at every step, always with a partial weight
        return pe_window_weights(L * (0.2 + 0.6 * ((iteration % 97) / 97.0)), L)

    def make_trainer(schedule):
        torch.manual_seed(42)
        mc, mf = create_nerf(ModelConfig(precision="bf16"))
        cam = CameraPoseParameters(cam0.initial_poses.clone(), fixed_small_angle=True)
        tr = PoseTrainer(mc.to(dev), mf.to(dev), cam, sampler, rc, pe_schedule=schedule)
        tr.set_pe_windows(0)
        return tr

    def timed(step, pool):
        for k in range(a.warmup):
            step(pool[k % len(pool)], k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.steps):
            step(pool[k % len(pool)], a.warmup + k)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    results = []
    for mode, B in CASES:
        sampler.batch_size = B
        gen = torch.Generator(device=dev).manual_seed(1000)
        pool = [sampler.sample_batch(generator=gen) for _ in range(4)]
        legs, graphs = {}, {}
        for name, schedule in (("off", None), ("on", fixed), ("moving", moving)):
            tr = make_trainer(schedule)
            if mode == "graph":
                tr = graphs[name] = GraphedPoseTrainer(tr, pool[0], warmup=1)
            # the fixed window is set once (make_trainer); only the moving one is rewritten per step
            legs[name] = (lambda b, k, tr=tr, it=(name == "moving"):
                          tr.step(b, optimize_poses=True, iteration=k if it else None))
        torch.manual_seed(1234)
        runs = {name: [] for name in legs}
        for _ in range(a.repeats):
            for name, step in legs.items():  # alternating: every leg sees the same machine state
                runs[name].append(round(timed(step, pool), 4))
        for g in graphs.values():
            assert sorted(g._graphs) == [True]  # the graph legs replayed the optimising graph
        med = {name: sorted(v)[len(v) // 2] for name, v in runs.items()}
        spread = {name: round(max(v) - min(v), 4) for name, v in runs.items()}
        rec = {"mode": mode, "B": B, "ms_per_step": runs, "median_ms": med, "spread_ms": spread,
               "on_minus_off_ms": round(med["on"] - med["off"], 4),
               "moving_minus_off_ms": round(med["moving"] - med["off"], 4),
               "on_over_off": round(med["on"] / med["off"], 4),
               "moving_over_off": round(med["moving"] / med["off"], 4),
               "final_loss": {name: float(step(pool[0], 0)["loss"]) for name, step in legs.items()}}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = {"tool": "tools/pe_window_ab.py", "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "samples": [rc.num_samples, rc.num_samples_fine], "image": [800, 800], "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "window": "alpha = 0.34 L per encoder",
           "results": results}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
