"""The joint pose step with the learned lens off and on, eager and replayed from a hipGraph.

Workload: bench.pose_opt_setup(800, 800) (BASELINE cfg #3: 100 views, the reference's noisy
initial poses), bf16 networks, 64 coarse + 128 fine samples, every step optimising the poses,
the randoms drawn per step as the eager step draws them.  For each batch size (default 512 and
4096 rays) the legs -- eager_off, eager_on, graph_off, graph_on ("off": no intrinsics, the step of
before; "on": a ``CameraIntrinsics`` in mode "shared" with ``learn_principal`` and
``learn_distortion``, so the 18-row ray backward and three more clip groups in the pose Adam) --
run in ONE process, alternating, REPEATS times each; a run is
WARMUP untimed steps, a device sync, STEPS timed steps over pre-drawn pixel batches and a device
sync.  Each leg trains its own copy of the model from the same seed.

``--tree DIR`` imports the package (and bench.py) from another checkout of the project, e.g. the
parent commit with its own built library; a tree whose ``CameraIntrinsics`` has no lens runs the
"off" legs only, and ``--off-only`` makes this tree do the same (the eager legs are bound by the host,
whose pace depends on what else the process has run, so trees are compared in like processes).
"Off" is the code path of before, so it is expected within the run-to-run spread of the parent;
"on" is reported, not asserted.

Writes every run's ms/step (so the spread -- the range of a leg's repeated runs -- is visible)
to --out (default profiles/lens_ab.json; with --label, under that key of the file, so
that several trees can share it) and prints one JSON line per batch size.  There is no CPU
path: without a GPU the tool fails.

python tools/lens_ab.py [--tree DIR] [--label NAME] [--off-only] [--out FILE] [--steps 200]
                        [--warmup 20] [--repeats 3] [B ...]"""
import argparse
import inspect
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("batches", nargs="*", type=int, default=[512, 4096])
    ap.add_argument("--tree", type=Path, default=ROOT)
    ap.add_argument("--label", type=str, default="this")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "lens_ab.json")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--off-only", action="store_true",
                    help="run the two 'off' legs alone: the process a tree without the feature runs, for a "
                         "like-for-like comparison with it")
    a = ap.parse_args(argv)
    if a.steps < 200 or a.warmup < 20 or a.repeats < 3:
        raise SystemExit("lens_ab: the protocol needs >= 200 timed steps, >= 20 warm-up steps and >= 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("lens_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")
    tree = a.tree.resolve()
    sys.path[:0] = [str(tree), str(tree / "robust-nerf_amd")]

    import bench
    import noisy_src.train_pose_opt as tpo
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import GraphedPoseTrainer, PoseTrainer
    from noisy_src.model import create_nerf

    assert Path(tpo.__file__).resolve().is_relative_to(tree), (tpo.__file__, tree)
    has_on = (hasattr(tpo, "CameraIntrinsics") and not a.off_only
              and "learn_principal" in inspect.signature(tpo.CameraIntrinsics.__init__).parameters)
    dev = torch.device("cuda", 0)
    rc = RenderConfig(num_samples=64, num_samples_fine=128)
    cam0, sampler = bench.pose_opt_setup(800, 800, dev)

    def make_trainer(on):
        torch.manual_seed(42)
        mc, mf = create_nerf(ModelConfig(precision="bf16"))
        extra = {}
        if on:
            ds = sampler.dataset
            extra["intrinsics"] = tpo.CameraIntrinsics(ds.focal, "shared", learn_principal=True, learn_distortion=True,
                                                       image_size=(ds.W, ds.H)).to(dev)
        return PoseTrainer(mc.to(dev), mf.to(dev), tpo.CameraPoseParameters(cam0.initial_poses.clone()), sampler, rc,
                           **extra)

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
        legs, graphs = {}, []
        for on in (False, True) if has_on else (False,):
            eager, captured = make_trainer(on), make_trainer(on)
            graphed = GraphedPoseTrainer(captured, pool[0], warmup=1)
            graphs.append(graphed)
            tag = "on" if on else "off"
            legs[f"eager_{tag}"] = lambda b, t=eager: t.step(b, optimize_poses=True)
            legs[f"graph_{tag}"] = lambda b, g=graphed: g.step(b, optimize_poses=True)
        torch.manual_seed(1234)
        runs = {name: [] for name in legs}
        for _ in range(a.repeats):
            for name, step in legs.items():  # alternating: every leg sees the same machine state
                runs[name].append(round(timed(step, pool), 4))
        assert all(sorted(g._graphs) == [True] for g in graphs)  # the graph legs replayed the optimising graph
        med = {name: sorted(v)[len(v) // 2] for name, v in runs.items()}
        spread = {name: round(max(v) - min(v), 4) for name, v in runs.items()}
        rec = {"B": B, "ms_per_step": runs, "median_ms": med, "spread_ms": spread,
               "final_loss": {name: float(step(pool[0])["loss"]) for name, step in legs.items()}}
        if has_on:
            rec["on_minus_off_ms"] = {k: round(med[f"{k}_on"] - med[f"{k}_off"], 4) for k in ("eager", "graph")}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    entry = {"tool": "tools/lens_ab.py", "device": torch.cuda.get_device_name(0), "precision": "bf16",
             "samples": [rc.num_samples, rc.num_samples_fine], "image": [800, 800], "steps": a.steps,
             "warmup": a.warmup, "repeats": a.repeats, "results": results}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    doc = json.loads(a.out.read_text()) if a.out.exists() else {}
    doc[a.label] = entry
    a.out.write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
