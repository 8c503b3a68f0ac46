"""Host cost of the two training loops, one copy of the Python package against another.

``train.train`` and ``train_pose_opt.train_with_pose_optimization`` on one GPU, bf16, on a
synthetic scene (8 train / 2 val views of 128x128 random pixels, the golden run's poses)
handed in as ``train_data`` / ``val_data``: ITERS iterations with validation and checkpoints
beyond the run and ``log_every`` 100, at 512 and 1024 rays, eager and ``graph=True``.  A
cell's figure is the mean ``time_per_iter`` of train_metrics.csv in ms, the first SKIP rows
discarded: the loop's own clock, so it holds the step's host work and the loop's.

The driver starts one fresh process per package and repeat, alternating ``--parent`` (a
directory that holds another ``noisy_src``) and the tree, REPEATS times each, every process
under its own time limit and with NR_HIP_LIB naming the tree's library, and stops at the
first that fails.  Bar per cell: the tree's median may exceed the parent's by no more than
the parent's own max-to-min range.  Writes every value and the verdicts to --out (default
profiles/run_loop_ab.json).  There is no CPU path.

python tools/run_loop_ab.py --parent DIR [--out FILE]"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
ITERS, SKIP, REPEATS, BATCHES, LIMIT_S = 300, 50, 3, (512, 1024), 420


def worker() -> int:
    """One package (the first ``noisy_src`` on sys.path): one JSON line per cell."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("run_loop_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")
    import importlib
    from noisy_src.config import NeRFConfig
    from noisy_src.data import synthetic_blender_data
    train = importlib.import_module("noisy_src.train").train
    train_pose = importlib.import_module("noisy_src.train_pose_opt").train_with_pose_optimization
    poses = torch.from_numpy(np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*.npz"))[0])
                             ["ground_truth_poses"]).float()
    data = synthetic_blender_data(poses[:8], 128, 128, seed=0), synthetic_blender_data(poses[8:10], 128, 128, seed=1)
    quiet = lambda *a, **k: None  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        for loop in ("train", "pose"):
            for B in BATCHES:
                for graph in (False, True):
                    cfg = NeRFConfig()
                    cfg.model.precision = "bf16"
                    cfg.data.batch_size = B
                    cfg.train.num_iterations, cfg.train.log_every = ITERS, 100
                    cfg.train.val_every = cfg.train.save_every = 10 * ITERS
                    cfg.train.output_dir = Path(tmp)
                    name = cfg.train.experiment_name = f"{loop}_{B}_{'graph' if graph else 'eager'}"
                    kw = dict(train_data=data[0], val_data=data[1], log=quiet, graph=graph)
                    if loop == "train":
                        train(cfg, **kw)
                    else:  # the poses optimised from iteration 10 on: the timed rows are all of one kind
                        train_pose(cfg, pose_opt_delay=10, experiment_name=name, **kw)
                    rows = list(csv.DictReader((Path(tmp) / name / "logs" / "train_metrics.csv").open()))
                    assert len(rows) == ITERS, len(rows)
                    ms = 1e3 * statistics.fmean(float(r["time_per_iter"]) for r in rows[SKIP:])
                    print(json.dumps({"cell": name, "ms_per_iter": round(ms, 4)}), flush=True)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", type=Path, help="directory holding the other copy of noisy_src")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "run_loop_ab.json")
    ap.add_argument("--worker", action="store_true", help="(internal) measure the first noisy_src on sys.path")
    a = ap.parse_args(argv)
    if a.worker:
        return worker()
    if a.parent is None or not (a.parent / "noisy_src").is_dir():
        raise SystemExit("run_loop_ab: --parent must name a directory that holds noisy_src")
    tree = ROOT / "robust-nerf_amd"
    lib = tree / "noisy_src" / "lib" / "libnerf_hip.so"
    values = {}
    for rep in range(REPEATS):
        for leg, pkg in (("parent", a.parent.resolve()), ("tree", tree)):  # alternating: both see the same machine
            env = dict(os.environ, PYTHONPATH=str(pkg), NR_HIP_LIB=str(lib))
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--worker"], env=env, text=True,
                               stdout=subprocess.PIPE, timeout=LIMIT_S, check=True)
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    values.setdefault(rec["cell"], {"parent": [], "tree": []})[leg].append(rec["ms_per_iter"])
            print(f"repeat {rep} {leg} done", flush=True)
    cells = {}
    for cell, v in values.items():
        med = {leg: statistics.median(x) for leg, x in v.items()}
        spread = round(max(v["parent"]) - min(v["parent"]), 4)
        cells[cell] = {"ms_per_iter": v, "median_ms": med, "parent_range_ms": spread,
                       "tree_minus_parent_ms": round(med["tree"] - med["parent"], 4),
                       "pass": bool(med["tree"] - med["parent"] <= spread)}
        print(json.dumps({cell: cells[cell]}), flush=True)
    import torch
    out = {"tool": "tools/run_loop_ab.py", "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "iterations": ITERS, "discarded": SKIP, "repeats": REPEATS, "figure": "mean time_per_iter of "
           "train_metrics.csv, ms", "bar": "median(tree) - median(parent) <= max(parent) - min(parent)",
           "cells": cells, "pass": all(c["pass"] for c in cells.values())}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(out, indent=1) + "\n")
    return 0 if out["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
