"""One line per artefact of the run folders that ``noisy_src.train`` and
``noisy_src.train_pose_opt`` write, for comparing two copies of the Python package.

Runs the command lines of CASES on the 3-train / 2-val 16x16 scene of
tests/test_entry_points.py against whichever ``noisy_src`` comes first on sys.path (the
tree's when PYTHONPATH names no other) and the library NR_HIP_LIB names (default: that
package's own build), and prints what they left behind.  Run it once per package, each in
a fresh process, and diff the two outputs: a refactor of the loops changes no line.

    NR_HIP_LIB=$PWD/robust-nerf_amd/noisy_src/lib/libnerf_hip.so PYTHONPATH=/path/to/parent_pkg \\
        python tools/run_folder_manifest.py > parent.txt
    python tools/run_folder_manifest.py > tree.txt && diff parent.txt tree.txt
    python tools/run_folder_manifest.py [--leaves] [CASE ...]

Per case: the sorted file list of the run folder; train_metrics.csv without the columns of
CSV_DROPPED; val_metrics.csv whole; every .json without the keys of JSON_DROPPED (at any
depth); for every checkpoint and final_poses.pt one SHA-256 per tensor leaf and the repr of
every other leaf, walked in sorted key order, and folded into one SHA-256 per top-level key of
the file (``--leaves`` prints every leaf instead, to find the one behind a line that differs);
the captured console lines with the numbers of LOG_MASKS masked.  Run timestamps
(YYYYMMDD_HHMMSS, in the pose runs' folder names) are masked everywhere.  The runs use relative
--data_root / --output_dir inside a temp dir, so no path in a config differs.  There is no
CPU path."""
import contextlib
import csv
import hashlib
import importlib
import io
import json
import os
import re
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path += [str(ROOT / "robust-nerf_amd"), str(ROOT / "tests")]  # after PYTHONPATH: another package there wins

COMMON = "--data_root data --img_scale 1.0 --precision bf16 --seed 7 --noise_seed 3".split()
TRAIN = "--batch_size 100 --num_iters 12 --val_every 4 --save_every 5 --log_every 1 --rotation_noise 1".split()
POSE = ("--batch_size 128 --num_iters 8 --pose_opt_delay 3 --val_every 3 --save_every 4 --log_every 1 "
        "--rotation_noise 5 --translation_noise_pct 5").split()
POSE_ALL = POSE + ("--c2f 0.1 0.5 --fixed_small_angle --learn_focal xy --focal_init_scale 1.05 "
                   "--distortion_weight 0.01").split()
CASES = {  # name -> (module, flags); 768 rays / 100: the epoch's tail batch of "train" has 68 rays
    "train": ("train", TRAIN),
    "train_graph": ("train", TRAIN + ["--graph"]),
    "train_coarse": ("train", "--no_hierarchical --batch_size 64 --num_iters 3".split()),
    "train_distortion": ("train", "--distortion_weight 0.01 --batch_size 128 --num_iters 4 --val_every 2".split()),
    "pose": ("train_pose_opt", POSE),
    "pose_graph": ("train_pose_opt", POSE + ["--graph"]),
    "pose_all": ("train_pose_opt", POSE_ALL),
    "pose_all_graph": ("train_pose_opt", POSE_ALL + ["--graph"]),
    "pose_clean": ("train_pose_opt", "--init_mode clean --no_learn_rotation --num_iters 3 --val_every 100".split()),
}
CSV_DROPPED = ("time_per_iter", "rays_per_sec")  # wall-clock columns of train_metrics.csv
JSON_DROPPED = ("timestamp", "start_time", "end_time", "total_time_seconds")  # wall-clock keys of the .json files
LOG_MASKS = ((r"time: [\d.]+", "time: #"), (r"rays/s: \d+", "rays/s: #"), (r"[\d.]+ min", "# min"))
TIMESTAMP = re.compile(r"\d{8}_\d{6}")
EVERY_LEAF = False


def emit(case, what, text):
    print(TIMESTAMP.sub("<timestamp>", f"{case} {what} {text}"))


def without(obj, dropped):
    if isinstance(obj, dict):
        return {k: without(v, dropped) for k, v in obj.items() if k not in dropped}
    return [without(v, dropped) for v in obj] if isinstance(obj, list) else obj


def leaves(obj, path=""):
    if isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from leaves(obj[k], f"{path}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from leaves(v, f"{path}/{i}")
    elif isinstance(obj, torch.Tensor):
        raw = obj.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        yield path, f"{obj.dtype} {tuple(obj.shape)} {hashlib.sha256(raw).hexdigest()}"
    else:
        yield path, repr(obj)


def manifest(case, run, log_text):
    files = sorted(p.relative_to(run).as_posix() for p in run.rglob("*") if p.is_file())
    emit(case, "files", " ".join(files))
    for name in files:
        path = run / name
        if name == "logs/train_metrics.csv":
            rows = list(csv.reader(path.open()))
            keep = [i for i, col in enumerate(rows[0]) if col not in CSV_DROPPED]
            for n, row in enumerate(rows):
                emit(case, f"{name}:{n}", ",".join(row[i] for i in keep))
        elif name.endswith(".csv"):
            for n, row in enumerate(path.read_text().splitlines()):
                emit(case, f"{name}:{n}", row)
        elif name.endswith(".json"):
            emit(case, name, json.dumps(without(json.loads(path.read_text()), JSON_DROPPED), sort_keys=True))
        elif name.endswith(".pt"):
            for key, value in sorted(torch.load(path, map_location="cpu", weights_only=True).items()):
                lines = [f"{leaf} {text}" for leaf, text in leaves(value, f"/{key}")]
                if EVERY_LEAF:
                    for line in lines:
                        emit(case, name, line)
                else:
                    folded = hashlib.sha256(TIMESTAMP.sub("<timestamp>", "\n".join(lines)).encode()).hexdigest()
                    emit(case, f"{name}/{key}", f"{len(lines)} leaves {folded}")
    for n, line in enumerate(log_text.splitlines()):
        for pattern, masked in LOG_MASKS:
            line = re.sub(pattern, masked, line)
        emit(case, f"log:{n}", line)


def main() -> int:
    if not torch.cuda.is_available():
        raise SystemExit("run_folder_manifest: no GPU found (there is no CPU path)")
    from test_entry_points import _scene
    global EVERY_LEAF
    EVERY_LEAF = "--leaves" in sys.argv[1:]
    names = [a for a in sys.argv[1:] if a != "--leaves"] or list(CASES)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        _scene(Path("data"))
        for case in names:
            module, flags = CASES[case]
            mod = importlib.import_module(f"noisy_src.{module}")
            print(f"# {case}: {mod.__file__}", file=sys.stderr)
            out = Path("out") / case
            argv = COMMON + flags + ["--output_dir", str(out)]
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                mod.main(argv + ["--exp_name", "run"] if module == "train" else argv)
            runs = list(out.iterdir())
            assert len(runs) == 1, runs
            manifest(case, runs[0], log.getvalue())
        os.chdir(ROOT)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
