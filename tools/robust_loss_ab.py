"""What a robust photometric loss costs: the fused compositing launch per loss kind against
nr_composite_mse, and the training step with ``loss="mse"`` against ``loss="cauchy"``.

* ``launch``: microseconds per launch at B = 4096, S = 64 and 192 (tools/composite_bits.py
  ``time``'s inputs and method: LAUNCHES launches between two HIP events after WARMUP
  launches), for nr_composite_mse and nr_composite_robust with each kind of
  ``ops.LOSS_KINDS`` at c = 0.1.  All entries run in ONE process and alternate: a round
  times one window of every entry, REPEATS rounds, the median per entry.  At this B the
  entry points drop the ticket, so each figure includes the one-block loss sum.
* ``step``: milliseconds per ``Trainer.step`` on bench.py's flagship workload (BASELINE
  cfg #2: 4,096 lego rays, bf16, 64 coarse + 128 fine samples, ``coarse_stream="auto"``),
  one trainer per kind on its own copy of the model, alternating, ``--repeats`` runs of
  ``--steps`` timed steps after ``--warmup`` untimed ones, a device sync at both ends.

python tools/robust_loss_ab.py [--out FILE] [--steps 200] [--warmup 20] [--repeats 3]
The result becomes the "feature" entry of FILE (default profiles/robust_loss_ab.json), whose
other entries are kept.  There is no CPU path."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd"), str(ROOT / "tests")]
DEV = "cuda"
SCALE_C = 0.1
LAUNCHES, REPEATS, WARMUP = 200, 5, 50
STEP_KINDS = ("mse", "cauchy")


def window_us(launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        launch()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / LAUNCHES


def launch_times():
    import edge_inputs as ei
    from noisy_src import _hip, ops
    from noisy_src._hip import call, ptr
    stream = _hip.stream_ptr()
    B = 4096
    out = {"B": B, "c": SCALE_C, "launches": LAUNCHES, "repeats": REPEATS, "warmup": WARMUP, "us": {}}
    for S in (64, 192):
        c = {k: (None if v is None else v.to(DEV)) for k, v in ei.composite_inputs(S, B, "random").items()}
        front = [ptr(c[k]) for k in ("rgb", "sigma", "z", "rd", "noise")]
        nan = float("nan")
        rgb_map, depth, acc, weights = (torch.full(s, nan, device=DEV) for s in ((B, 3), (B,), (B,), (B, S)))
        loss2, g_rgb, g_sigma = (torch.full(s, nan, device=DEV) for s in ((2,), (B, S, 3), (B, S)))
        g_rd = torch.zeros(B, 3, device=DEV)
        ticket = torch.zeros(4, device=DEV, dtype=torch.int32)
        ws = torch.full((int(_hip.load().nr_composite_robust_workspace_bytes(B)) // 4,), nan, device=DEV)
        tail = (ptr(g_rgb), ptr(g_sigma), ptr(g_rd), ptr(ticket), ptr(ws), stream)
        maps = (ptr(rgb_map), ptr(depth), ptr(acc), ptr(weights), ptr(loss2))
        entries = {"nr_composite_mse": lambda: call("nr_composite_mse", *front, ptr(c["target"]), B, S, 1, 1.0, *maps,
                                                    *tail)}
        for k, kind in enumerate(ops.LOSS_KINDS):
            entries[f"nr_composite_robust/{kind}"] = (
                lambda k=k: call("nr_composite_robust", *front, ptr(c["target"]), B, S, 1, k, SCALE_C, 1.0, *maps,
                                 *tail))
        for launch in entries.values():
            for _ in range(WARMUP):
                launch()
        torch.cuda.synchronize()
        windows = {name: [] for name in entries}
        for _ in range(REPEATS):
            for name, launch in entries.items():  # alternating: every entry sees the same machine state
                windows[name].append(round(window_us(launch), 3))
        base = statistics.median(windows["nr_composite_mse"])
        for name, w in windows.items():
            med = statistics.median(w)
            out["us"][f"{name}/S{S}"] = {"median": round(med, 3), "windows": w, "minus_mse": round(med - base, 3)}
    return out


def step_times(steps, warmup, repeats):
    import bench
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import Trainer
    from noisy_src.model import create_nerf
    dev = torch.device("cuda", 0)
    B, rc = 4096, RenderConfig(num_samples=64, num_samples_fine=128)
    pool = [bench.lego_rays(B, k, dev) for k in range(4)]

    def make_trainer(kind):
        torch.manual_seed(42)
        mc, mf = create_nerf(ModelConfig(precision="bf16"))
        return Trainer(mc.to(dev), mf.to(dev), rc, coarse_stream="auto", loss=kind, loss_scale=SCALE_C)

    def timed(tr):
        for k in range(warmup):
            tr.step(*pool[k % len(pool)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            tr.step(*pool[k % len(pool)])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    legs = {kind: make_trainer(kind) for kind in STEP_KINDS}
    torch.manual_seed(1234)
    runs = {kind: [] for kind in legs}
    for _ in range(repeats):
        for kind, tr in legs.items():
            runs[kind].append(round(timed(tr), 4))
    med = {k: statistics.median(v) for k, v in runs.items()}
    last = {kind: tr.step(*pool[0]) for kind, tr in legs.items()}
    return {"rays": B, "precision": "bf16", "samples": [rc.num_samples, rc.num_samples_fine], "steps": steps,
            "warmup": warmup, "repeats": repeats, "ms_per_step": runs, "median_ms": med,
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in runs.items()},
            "cauchy_minus_mse_ms": round(med["cauchy"] - med["mse"], 4),
            "final": {kind: {k: float(v) for k, v in m.items() if k.startswith(("loss", "mse_"))}
                      for kind, m in last.items()}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "robust_loss_ab.json")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("robust_loss_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")
    doc = {"tool": "tools/robust_loss_ab.py", "device": torch.cuda.get_device_name(0), "launch": launch_times(),
           "step": step_times(a.steps, a.warmup, a.repeats)}
    print(json.dumps(doc), flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    # the file also holds the parent-against-tree runs of bench.py: only "feature" is this tool's
    whole = json.loads(a.out.read_text()) if a.out.exists() else {}
    whole["feature"] = doc
    a.out.write_text(json.dumps(whole, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
