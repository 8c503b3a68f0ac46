"""``PoseRefiner.step`` on the frozen-field kernels against the same step on the training
kernels (``NR_MLP_FROZEN=0``: saving forward, full dX chain, dW GEMM and reduce) on one GPU.

Workload: bench.pose_opt_setup(800, 800) (100 views, the reference's noisy initial poses),
bf16 networks with frozen parameters, 64 coarse + 128 fine samples, 512 and 4096 rays.  The
switch is read when ``noisy_src.model`` is imported, so each leg runs in a child process of
this driver; the legs alternate, REPEATS children each, on one box.  A child does, per batch
size, WARMUP untimed steps, a device sync, STEPS timed steps over pre-drawn pixel batches and
a device sync, and prints one JSON line.  With ``--kernels`` one more child per leg runs under
``rocprofv3 --kernel-trace --stats`` (fewer steps; its wall times are not used) and the
per-kernel totals of its stats file are recorded.

Writes every run's ms/step, the medians, the spread (range of a leg's runs) and
``frozen_over_training`` to --out (default profiles/frozen_step_ab.json).  No CPU path.

python tools/frozen_step_ab.py [--out FILE] [--steps 200] [--warmup 20] [--repeats 3] [--kernels] [B ...]"""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]


def worker(a) -> int:
    """One leg (this process's NR_MLP_FROZEN): a JSON line of ms/step per batch size."""
    import torch

    import bench
    from noisy_src import model
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import PoseRefiner
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters

    if not torch.cuda.is_available():
        raise SystemExit("frozen_step_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")
    dev = torch.device("cuda", 0)
    rc = RenderConfig(num_samples=64, num_samples_fine=128)
    cam0, sampler = bench.pose_opt_setup(800, 800, dev)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision="bf16"))
    mc, mf = mc.to(dev), mf.to(dev)
    res = {"frozen_kernels": bool(model._FROZEN), "ms_per_step": {}, "final_loss": {}}
    for B in a.batches:
        sampler.batch_size = B
        gen = torch.Generator(device=dev).manual_seed(1000)
        pool = [sampler.sample_batch(generator=gen) for _ in range(4)]
        cam = CameraPoseParameters(cam0.initial_poses.clone(), fixed_small_angle=True).to(dev)
        torch.manual_seed(1234)
        with PoseRefiner(mc, mf, cam, sampler, rc) as refiner:
            for k in range(a.warmup):
                refiner.step(pool[k % len(pool)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.steps):
                m = refiner.step(pool[k % len(pool)])
            torch.cuda.synchronize()
            res["ms_per_step"][str(B)] = round(1e3 * (time.perf_counter() - t0) / a.steps, 4)
            res["final_loss"][str(B)] = float(m["loss"])
    print("FROZEN_AB " + json.dumps(res), flush=True)
    return 0


def _child(a, frozen: bool, extra=(), prefix=(), steps=None, warmup=None):
    env = dict(os.environ, NR_MLP_FROZEN="1" if frozen else "0")
    cmd = [*prefix, sys.executable, str(Path(__file__).resolve()), "--worker", "--steps", str(steps or a.steps),
           "--warmup", str(warmup or a.warmup), *extra, *[str(b) for b in a.batches]]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    if out.returncode != 0:
        raise SystemExit(f"frozen_step_ab: a child failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("FROZEN_AB ")][-1]
    return json.loads(line[len("FROZEN_AB "):])


def _kernel_stats(a, frozen: bool):
    """Per-kernel totals of one profiled child: [{name, calls, total_us}], largest first."""
    with tempfile.TemporaryDirectory() as tmp:
        prefix = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--"]
        _child(a, frozen, prefix=prefix, steps=20, warmup=5)
        files = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not files:
            return None
        rows = []
        with open(files[0]) as fh:
            for r in csv.DictReader(fh):
                rows.append({"name": r.get("Name", "")[:120], "calls": int(r.get("Calls", 0) or 0),
                             "total_us": round(float(r.get("TotalDurationNs", 0) or 0) / 1e3, 1)})
        return sorted(rows, key=lambda r: -r["total_us"])[:24]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("batches", nargs="*", type=int, default=[512, 4096])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "frozen_step_ab.json")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="one rocprofv3 --kernel-trace --stats child per leg")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    if a.steps < 200 or a.warmup < 20 or a.repeats < 3:
        raise SystemExit("frozen_step_ab: the protocol needs >= 200 timed steps, >= 20 warm-up steps and >= 3 repeats")
    legs = {"training_kernels": False, "frozen_kernels": True}
    runs = {name: {str(b): [] for b in a.batches} for name in legs}
    losses = {}
    for _ in range(a.repeats):
        for name, frozen in legs.items():  # alternating: both legs see the same machine state
            r = _child(a, frozen)
            assert r["frozen_kernels"] == frozen
            for b, ms in r["ms_per_step"].items():
                runs[name][b].append(ms)
            losses[name] = r["final_loss"]
    results = []
    for b in (str(b) for b in a.batches):
        med = {n: sorted(runs[n][b])[len(runs[n][b]) // 2] for n in legs}
        spread = {n: round(max(runs[n][b]) - min(runs[n][b]), 4) for n in legs}
        rec = {"B": int(b), "ms_per_step": {n: runs[n][b] for n in legs}, "median_ms": med, "spread_ms": spread,
               "frozen_over_training": round(med["frozen_kernels"] / med["training_kernels"], 4),
               "final_loss": {n: losses[n][b] for n in legs}}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = {"tool": "tools/frozen_step_ab.py", "precision": "bf16", "samples": [64, 128], "image": [800, 800],
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "results": results}
    if a.kernels:
        out["kernel_stats"] = {name: _kernel_stats(a, frozen) for name, frozen in legs.items()}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
