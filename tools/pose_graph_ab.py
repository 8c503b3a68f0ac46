"""Eager ``PoseTrainer.step`` against ``GraphedPoseTrainer.step`` (hipGraph replay) on one GPU.

Workload: bench.pose_opt_setup(800, 800) (BASELINE cfg #3: 100 views, the reference's noisy
initial poses), bf16 networks, 64 coarse + 128 fine samples, every step optimising the poses,
the randoms drawn per step as the eager step draws them.  For each batch size (default 512,
1024 and 4096 rays) the two legs run in ONE process, alternating, REPEATS times each; a run is
WARMUP untimed steps, a device sync, STEPS timed steps over pre-drawn pixel batches and a
device sync.  Each leg trains its own copy of the model from the same seed.

Writes every run's ms/step (so the spread -- the range of a leg's repeated runs -- is
visible) to --out (default profiles/pose_graph_ab.json) and prints one JSON line per batch
size (``final_loss`` only shows that both legs train: they consume different draws of the
shared RNG).  There is no CPU path: without a GPU the tool fails.

python tools/pose_graph_ab.py [--out FILE] [--steps 200] [--warmup 20] [--repeats 3] [B ...]"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("batches", nargs="*", type=int, default=[512, 1024, 4096])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "pose_graph_ab.json")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args(argv)
    if a.steps < 200 or a.warmup < 20 or a.repeats < 3:
        raise SystemExit("pose_graph_ab: the protocol needs >= 200 timed steps, >= 20 warm-up steps and >= 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("pose_graph_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")

    import bench
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import GraphedPoseTrainer, PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters

    dev = torch.device("cuda", 0)
    rc = RenderConfig(num_samples=64, num_samples_fine=128)
    cam0, sampler = bench.pose_opt_setup(800, 800, dev)

    def make_trainer():
        torch.manual_seed(42)
        mc, mf = create_nerf(ModelConfig(precision="bf16"))
        return PoseTrainer(mc.to(dev), mf.to(dev), CameraPoseParameters(cam0.initial_poses.clone()), sampler, rc)

    def timed(step, pool):
        for k in range(a.warmup):
            step(pool[k % len(pool)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.steps):
            step(pool[k % len(pool)])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    results = []
    for B in a.batches:
        sampler.batch_size = B
        gen = torch.Generator(device=dev).manual_seed(1000)
        pool = [sampler.sample_batch(generator=gen) for _ in range(4)]
        eager, captured = make_trainer(), make_trainer()
        graphed = GraphedPoseTrainer(captured, pool[0], warmup=1)
        legs = {"eager": lambda b: eager.step(b, optimize_poses=True),
                "graph": lambda b: graphed.step(b, optimize_poses=True)}
        torch.manual_seed(1234)
        runs = {name: [] for name in legs}
        for _ in range(a.repeats):
            for name, step in legs.items():  # alternating: both legs see the same machine state
                runs[name].append(round(timed(step, pool), 4))
        assert sorted(graphed._graphs) == [True]  # the graph leg replayed the optimising graph
        med = {name: sorted(v)[len(v) // 2] for name, v in runs.items()}
        spread = {name: round(max(v) - min(v), 4) for name, v in runs.items()}
        rec = {"B": B, "ms_per_step": runs, "median_ms": med, "spread_ms": spread,
               "graph_over_eager": round(med["graph"] / med["eager"], 4),
               "gain_ms": round(med["eager"] - med["graph"], 4),
               "gain_exceeds_spread": bool(min(runs["eager"]) - max(runs["graph"]) > 0
                                           and med["eager"] - med["graph"] > max(spread.values())),
               "final_loss": {name: float(step(pool[0])["loss"]) for name, step in legs.items()}}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = {"tool": "tools/pose_graph_ab.py", "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "samples": [rc.num_samples, rc.num_samples_fine], "image": [800, 800], "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "results": results}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
