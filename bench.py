#!/usr/bin/env python3
"""Benchmark of the NeRF training hot path on MI355X (BASELINE.json, config #2).

One step = one reference training iteration (noisy_src/train.py:455-465):
render coarse (64 stratified samples) + fine (128 inverse-CDF samples) for a
batch of rays, MSE losses, backward through every HIP kernel, joint gradient
clip, Adam, LambdaLR; with N GPUs the flat gradients are all-reduced over RCCL
first.  Workload: lego 800x800 camera geometry (focal 1111.1, the 100 training
poses of the reference's outputs/*/final_poses.pt fixture), 4096 rays per GPU
per step (weak scaling), bf16 MFMA MLP with fp32 master weights.  The scene
content is synthetic (random targets): the lego dataset is not available here.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--precision bf16|fp16|fp32]
                    [--num-samples 64 --num-samples-fine 128] [--global-batch G] [--pose-opt]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line (metric,
value, unit, ms_per_step, ...).  --dump-outputs DIR also writes what the last timed step
returned (and the parameters it left) as DIR/<name>.npy; the inputs are seeded, so two
builds can be compared output for output.  --full adds everything else the benchmark
measures: the per-kernel timings and rooflines, the recorded PSNR comparison, the batch
assembly cost, the trained-state leg and the CPU baseline.

(BASELINE cfg #5 is --precision fp16 --num-samples 128 --num-samples-fine 256; cfg #3 is
--pose-opt; cfg #4's strong-scaling leg is --global-batch 4096 under torchrun, where every
rank draws the same global batches and trains on its contiguous slice.)

For N > 1 the driver runs it under torch.distributed.run (one rank per GPU).
Rank 0 prints ONE JSON line.
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

METRIC = "training rays/sec + test PSNR, lego 800² 64c+128f, at 1/2/4/8 MI355X"
MACS_PER_EVAL = 593_408  # MLP multiply-adds per sample (forward)
PEAK_TFLOPS = {"bf16": 2516.6, "fp16": 2516.6, "fp32": 157.3}  # dense MFMA (256 CU x 2.4 GHz); MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0  # HBM3E spec peak; MI355X_MICROARCH.md (~6300 achievable)

# Algorithmic work per sample of each fused-MLP kernel (default 8x256 model, L=10/4):
#   forward: every linear layer's multiply-adds (MFMA-bound);
#   backward dX: the W^T products of the dX chain without the x_enc rows (no g_x in training);
#   dW: it must read every saved layer input and every dz once (HBM-bound; unpadded widths).
MACS_DX = 128 * (256 + 27) + 256 * 256 + 7 * 256 * 256
DW_FEATURES = (63 + 8 * 256 + 256 + 27 + 128) + (8 * 256 + 256 + 128 + 1 + 3)
# kernels behind each entry point (16-bit forward / dX: the row-block-major kernels)
KERNEL_OF = {"nr_mlp_forward": ("mlp_fwd_rbm_kernel", "mlp_fwd_kernel"),
             "nr_mlp_backward_dx": ("mlp_bwd_rbm_kernel", "mlp_bwd_kernel"),
             "nr_mlp_backward_dw": ("mlp_dw_kernel",), "nr_mlp_backward_reduce": ("mlp_dw_reduce_kernel",)}


def traffic_of(kernels, M: int, prec: str):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC pass
    (profiles/traffic.json, written by tools/traffic.py: 2 x FETCH_SIZE + WRITE_SIZE,
    the gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md), or None."""
    f = ROOT / "profiles" / "traffic.json"
    if not f.exists():
        return None
    for rec in json.loads(f.read_text()).get("kernels", []):
        if rec["kernel"] in kernels and rec["M"] == M and rec["precision"] == prec:
            return rec["bytes_per_launch"]
    return None


def source_hash() -> str:
    """sha1 over the HIP sources and the ABI header (tools/prof_summary.py stamps the same
    hash into every kernel summary it writes)."""
    import hashlib
    h = hashlib.sha1()
    files = sorted((ROOT / "robust-nerf_amd" / "csrc").glob("*")) + [ROOT / "include" / "nerf_hip.h"]
    for f in files:
        if f.suffix in (".hip", ".inc", ".hpp", ".h"):
            h.update(f.name.encode())
            h.update(f.read_bytes())
    return h.hexdigest()[:12]


def rocprof_summary(prec: str):
    """The committed rocprofv3 kernel-trace summary of the benchmarked sources: the newest
    profiles/r*_kernel_summary.csv (tools/prof_summary.py, same bench.py command) whose
    source_hash equals this tree's, as {(kernel, M): row}, plus its file name."""
    import csv
    files = sorted((ROOT / "profiles").glob("r*_kernel_summary.csv"), key=lambda f: f.name.split("_kernel_summary")[0])
    want = source_hash()
    for f in reversed(files):
        rows = {}
        with open(f) as fh:
            for r in csv.DictReader(fh):
                # a summary stamped with an overridden hash (NR_SOURCE_HASH) is not a
                # same-source measurement
                if r.get("source_hash") != want or r.get("hash_overridden"):
                    break
                # the slab reduction is not precision-templated: its rows carry no precision
                if r.get("M_samples") and r.get("precision") in (prec, ""):
                    rows[(r["kernel"], int(r["M_samples"]))] = r
        if rows:
            return rows, f"profiles/{f.name}"
    return {}, None


def _flops_of(entry: str, M: int) -> float:
    return 2.0 * mfma_macs_of(entry) * M


def _alg_bytes_of(entry: str, M: int, prec: str, n_params: int) -> float:
    esize = 4 if prec == "fp32" else 2
    if entry == "nr_mlp_backward_dw":
        return DW_FEATURES * esize * M + 4 * n_params
    if entry == "nr_mlp_backward_reduce":
        return 4 * n_params * 2
    return 0.0


def bound_of(entry: str, M: int, prec: str, counted_bytes):
    """The roofline that bounds one launch: the larger of its MFMA floor (algorithmic
    FLOPs / dense peak) and its HBM floor (counted PMC bytes -- or the algorithmic
    bytes where there are none -- / 8 TB/s).  The training forward and dX are MFMA work
    whose saved-image / dz stores make the HBM floor the higher one."""
    t_mfma = _flops_of(entry, M) / (PEAK_TFLOPS[prec] * 1e12)
    nbytes = counted_bytes if counted_bytes else _alg_bytes_of(entry, M, prec, 0)
    t_hbm = (nbytes or 0.0) / (PEAK_HBM_GBS * 1e9)
    return ("hbm" if t_hbm >= t_mfma else "mfma"), t_mfma * 1e3, t_hbm * 1e3


def mfma_macs_of(entry: str) -> int:
    """MFMA multiply-adds per sample of one fused-MLP launch (SURVEY.md §8d basis): the
    forward's layers, the dX chain's W^T products, dW's outer products (one per weight)."""
    return {"nr_mlp_forward": MACS_PER_EVAL, "nr_mlp_backward_dx": MACS_DX,
            "nr_mlp_backward_dw": MACS_PER_EVAL}.get(entry, 0)


def mfma_roofline(entry: str, M: int, ms: float, prec: str):
    """the MLP is bounded by its MFMA FLOPs.  (achieved TFLOP/s, frac of
    the dense peak, work description) of one launch."""
    macs = mfma_macs_of(entry)
    tf = 2.0 * macs * M / (ms * 1e-3) / 1e12
    return tf, tf / PEAK_TFLOPS[prec], f"2 x {macs} MAC x {M} samples"


def roofline_of(entry: str, M: int, ms: float, prec: str, n_params: int, counted_bytes=None):
    """(bound, achieved, peak, unit, work-per-launch description) of one fused-MLP launch
    on the stored-activation HBM basis: the bytes THIS design stores / reads (a design
    choice, not the algorithm's: the headline roofline is ``mfma_roofline``)."""
    esize = 4 if prec == "fp32" else 2
    bound, _, _ = bound_of(entry, M, prec, counted_bytes)
    if entry in ("nr_mlp_forward", "nr_mlp_backward_dx") and bound == "mfma":
        macs = MACS_PER_EVAL if entry == "nr_mlp_forward" else MACS_DX
        return "mfma", 2.0 * macs * M / (ms * 1e-3) / 1e12, PEAK_TFLOPS[prec], "TFLOP/s", \
            f"2 x {macs} MAC x {M} samples"
    if entry in ("nr_mlp_forward", "nr_mlp_backward_dx"):
        # byte-bound MFMA kernel: the bytes it must move are its stores (saved images / dz)
        return "hbm", counted_bytes / (ms * 1e-3) / 1e9, PEAK_HBM_GBS, "GB/s", \
            f"{counted_bytes:.0f} counted HBM bytes (PMC, profiles/traffic.json)"
    if entry == "nr_mlp_backward_dw":
        nbytes = DW_FEATURES * esize * M + 4 * n_params
        return "hbm", nbytes / (ms * 1e-3) / 1e9, PEAK_HBM_GBS, "GB/s", \
            f"{DW_FEATURES} features x {esize} B x {M} samples + {n_params} fp32 grads"
    nbytes = 4 * n_params * 2
    return "hbm", nbytes / (ms * 1e-3) / 1e9, PEAK_HBM_GBS, "GB/s", f"{n_params} fp32 grads"


def kernel_table(wcalls, prec: str, n_params: int, rp_rows=None, active=None):
    """Per fused-MLP launch key: its launch ms, counted HBM bytes (PMC), the counted-byte
    rate, MFMA / HBM floors and the bound; plus the step's counted MLP bytes.  The ms is the
    committed same-source rocprof timed-region average (``ms_source`` "rocprof") when one
    exists for the key -- the headline's basis, so every fraction here agrees with it and
    the launches sum to at most the step -- else the HIP-event-bracketed warm-up mean,
    labelled "bracketed" and given no fractions (a bracketed launch carries queue gaps).
    ``active``: {M: active-tile fraction}; MFMA fractions count the executed tiles."""
    out, step_bytes = {}, 0.0
    for key, (n, live_ms) in sorted(wcalls.items()):
        entry, M = key.split("[M=")[0], int(key.split("[M=")[1].rstrip("]"))
        kern = KERNEL_OF.get(entry, (entry,))
        rp = next((rp_rows[(k, M)] for k in kern if rp_rows and (k, M) in rp_rows), None)
        rp_ms = float(rp.get("timed_avg_ms") or rp["avg_ms"]) if rp else None
        ms = rp_ms if rp_ms else live_ms
        tb = traffic_of(kern, M, prec if entry != "nr_mlp_backward_reduce" else "")
        bound, f_mfma, f_hbm = bound_of(entry, M, prec, tb)
        rec = {"ms": round(ms, 4), "ms_source": "rocprof" if rp_ms else "bracketed", "bound": bound,
               "mfma_floor_ms": round(f_mfma, 4), "hbm_floor_ms": round(f_hbm, 4)}
        if tb:
            rec["counted_bytes"] = tb
            step_bytes += tb
        if rp_ms:
            af = (active or {}).get(M, 1.0) if entry != "nr_mlp_forward" else 1.0
            fl = _flops_of(entry, M) * af
            if fl:
                rec["mfma_tflops"] = round(fl / (ms * 1e-3) / 1e12, 1)
                rec["mfma_frac"] = round(fl / (ms * 1e-3) / 1e12 / PEAK_TFLOPS[prec], 4)
                if af < 1.0:
                    rec["active_tile_frac"] = round(af, 4)
            if tb:
                rec["counted_GBps"] = round(tb / (ms * 1e-3) / 1e9, 1)
                rec["counted_hbm_frac"] = round(tb / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)
            alg = _alg_bytes_of(entry, M, prec, n_params)
            if alg and tb:
                rec["counted_over_algorithmic"] = round(tb / alg, 4)
        out[key] = rec
    return out, step_bytes


def headline_roofline(tflops: float, live_ms: float, rocprof_ms, prec: str, active: float = 1.0):
    """The dominant kernel on SURVEY §8d's MFMA basis: the algorithmic FLOPs of the work it
    EXECUTED per launch (its active 32-sample tiles; all of them at bare init) over its
    launch time -- the committed rocprof average of these sources when there is one
    (reproducible from profiles/), else the live HIP-event time."""
    ach = (tflops * live_ms / rocprof_ms if rocprof_ms else tflops) * active
    return {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_TFLOPS[prec], "unit": "TFLOP/s",
            "frac": round(ach / PEAK_TFLOPS[prec], 4)}


def rank_topology(pg, dev, step_ms_median: float, allreduce):
    """Self-check of a data-parallel run: the process group's size, the device
    every rank bound, each rank's median step time and its measured all-reduce times
    (HIP events around GradAllReducer's wait), gathered to every rank."""
    import torch.distributed as dist
    props = torch.cuda.get_device_properties(dev)
    mine = [float(dist.get_rank(pg)), float(dev.index), float(getattr(props, "pci_bus_id", -1)),
            float(getattr(props, "pci_device_id", -1)), step_ms_median,
            allreduce["span_ms"] if allreduce else -1.0, allreduce["exposed_ms"] if allreduce else -1.0]
    t = torch.tensor(mine, device=dev if dist.get_backend(pg) == "nccl" else "cpu", dtype=torch.float64)
    allt = [torch.empty_like(t) for _ in range(dist.get_world_size(pg))]
    dist.all_gather(allt, t, group=pg)
    ranks = []
    for v in (x.tolist() for x in allt):
        r = {"rank": int(v[0]), "device": int(v[1]), "pci_bus_id": int(v[2]), "pci_device_id": int(v[3]),
             "step_ms_median": round(v[4], 4)}
        if v[5] >= 0:
            r["allreduce_span_ms"] = round(v[5], 4)
            r["allreduce_exposed_ms"] = round(v[6], 4)
        ranks.append(r)
    return {"backend": dist.get_backend(pg), "world_size": dist.get_world_size(pg),
            "distinct_devices": len({(r["pci_bus_id"], r["pci_device_id"], r["device"]) for r in ranks}),
            "allreduce_steps": allreduce["steps"] if allreduce else 0,
            "allreduce_note": "HIP events on the compute stream over the last warm-up steps (eager; outside the "
                              "timed region): span = first gradient all-reduce launched (fine net, during the "
                              "coarse backward) -> all reduced; exposed = the step's wait for it in "
                              "GradAllReducer.finish" if allreduce else "not timed (fewer than 2 warm-up steps)",
            "ranks": ranks}


def lego_rays(n_rays: int, seed: int, device, size: int = 800):
    """Rays of the lego training cameras at size x size (focal from camera_angle_x,
    data.py:147-150)."""
    g = torch.Generator().manual_seed(seed)
    fix = sorted((ROOT / "tests" / "golden").glob("final_poses_*.npz"))[0]
    poses = torch.from_numpy(np.load(fix)["ground_truth_poses"])
    H = W = size
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    img = torch.randint(0, poses.shape[0], (n_rays,), generator=g)
    i = torch.randint(0, W, (n_rays,), generator=g).float()
    j = torch.randint(0, H, (n_rays,), generator=g).float()
    dirs = torch.stack([(i - W / 2) / focal, -(j - H / 2) / focal, -torch.ones_like(i)], -1)
    R = poses[img, :3, :3]
    d = torch.einsum("bij,bj->bi", R, dirs)
    d = d / d.norm(dim=-1, keepdim=True)
    o = poses[img, :3, 3]
    tgt = torch.rand(n_rays, 3, generator=g)
    return o.to(device), d.to(device), tgt.to(device)


def pose_opt_setup(H: int, W: int, device):
    """BASELINE cfg #3 inputs: the lego training cameras (GT poses of the reference's
    final_poses.pt fixture), the reference's own noisy initialisation for 5 deg rotation +
    5 % translation noise (initial_poses of that run's fixture) as the learnable poses,
    and an H x W synthetic image stack for the pixel sampler (train_pose_opt.py:640-700)."""
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import create_pixel_dataset
    from noisy_src.train_pose_opt import CameraPoseParameters
    fix = sorted((ROOT / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0]
    z = np.load(fix)
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"]), H=H, W=W, device=device)
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"]).to(device))
    _, sampler = create_pixel_dataset(data)
    return cam, sampler


def psnr_record():
    """The latest committed test-PSNR records (profiles/r*_psnr_parity*.json, written by
    tests/psnr_parity.py on the GPU box): RECORDED, not measured in this run.  The main
    one anneals the LR (lr_decay = 1: paired differences resolve to a few hundredths of a
    dB); `reference_schedule` is the reference's own LambdaLR (lr_decay = 250,
    train.py:405-411), under which equal-iteration runs stay chaotic."""
    def one(f):
        rec = json.loads(f.read_text())
        if "summary" not in rec:
            return None
        return {"recorded": True, "source": f"profiles/{f.name} (tests/psnr_parity.py)",
                "commit": rec.get("commit"), "scene": rec.get("scene", "analytic 3-sphere scene, lego train cameras"),
                "iters": rec["iters"], "seeds": rec["seeds"],
                "mean_db": {k: round(v["mean"], 3) for k, v in rec["summary"].items()},
                "lr_decay": rec.get("lr_decay"),
                "paired_delta_db_vs_ref": {k: v.get("paired_mean_db", v["delta_mean_db"])
                                           for k, v in rec["delta_vs_ref"].items()},
                "paired_se_db": {k: v.get("paired_se_db", v["se_of_delta_db"]) for k, v in rec["delta_vs_ref"].items()},
                **({"paired_ci90_db": {k: v["paired_ci90_db"] for k, v in rec["delta_vs_ref"].items()},
                    "within_0p1_db_tost": {k: v["within_0p1_db_tost"] for k, v in rec["delta_vs_ref"].items()}}
                   if all("paired_ci90_db" in v for v in rec["delta_vs_ref"].values()) else {})}
    # per schedule, the record with the most seeds (then the latest name): pooled records
    # (tests/psnr_parity.py --merge) supersede the batches they pool
    recs = []
    for f in sorted((ROOT / "profiles").glob("r*_psnr_parity*.json")):
        r = json.loads(f.read_text())
        recs.append((r.get("seeds") or 0, f.name, f, r.get("lr_decay")))
    main = [f for _, _, f, ld in sorted(recs) if ld in (1, None)]
    ref = [f for _, _, f, ld in sorted(recs) if ld == 250]
    out = one(main[-1]) if main else None
    if out is not None and ref:
        out["reference_schedule"] = one(ref[-1])
    return out


def _cpu_model() -> str:
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_leg(rc, n_rays: int, steps: int, warmup: int):
    """Per-step wall times of the oracle's reference train step (train.py:68-119 + the
    scheduler step; the rays/s interval of train.py:455-465) on the host CPU."""
    from oracle import refimpl as ref
    torch.manual_seed(42)
    mc, mf = ref.create_nerf()
    if not rc.use_hierarchical:
        mf = None
    state = ref.TrainState(mc, mf)
    o, d, t = lego_rays(n_rays, 123, "cpu", size=400)  # cfg #1: img_scale 0.5
    times = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        ref.train_step(mc, mf, state, o, d, t, rc)
        if k >= warmup:
            times.append(time.perf_counter() - t0)
    times.sort()
    q = lambda f: times[min(len(times) - 1, int(f * len(times)))]  # noqa: E731
    return {"rays_per_s_median": n_rays / q(0.5), "rays_per_s_p10": n_rays / q(0.9), "rays_per_s_p90": n_rays / q(0.1),
            "step_s_median": q(0.5), "steps": steps, "warmup": warmup, "seconds": sum(times)}


def cpu_baseline(steps: int = 50, warmup: int = 5, context_steps: int = 3):
    """the reference CPU path -- the oracle (op-for-op torch restatement of
    the reference; the reference itself is not shipped to the GPU box) -- on BASELINE
    cfg #1 (lego 400x400 cameras, coarse-only 64 samples, 256-ray batch, fp32), 5 warm-up
    + 50 timed steps, median/p10/p90, all host cores the process may use; plus a few
    steps of 64c+128f at 256 rays for context."""
    from types import SimpleNamespace
    affinity = len(os.sched_getaffinity(0))
    # the GPU box grants a CPU share (OMP_NUM_THREADS) smaller than the machine's affinity mask
    threads = min(affinity, int(os.environ.get("OMP_NUM_THREADS", affinity)))
    torch.set_num_threads(threads)
    rc1 = SimpleNamespace(near=2.0, far=6.0, num_samples=64, num_samples_fine=128, use_hierarchical=False,
                          perturb=True, raw_noise_std=0.0, white_background=True)
    c1 = _cpu_leg(rc1, 256, steps, warmup)
    rc2 = SimpleNamespace(**{**rc1.__dict__, "use_hierarchical": True})
    c2 = _cpu_leg(rc2, 256, context_steps, 1)
    return {"value": round(c1["rays_per_s_median"], 2), "unit": "rays/s", "cores": threads, "kind": "port",
            "sample": f"BASELINE cfg #1: oracle/refimpl.py train_step (fp32 torch CPU), lego 400x400 camera rays, "
                      f"coarse-only 64 samples, 256 rays, {warmup} warm-up + {steps} timed steps "
                      f"({c1['seconds']:.1f} s); value = median",
            "p10_p50_p90_rays_per_s": [round(c1["rays_per_s_p10"], 2), round(c1["rays_per_s_median"], 2),
                                       round(c1["rays_per_s_p90"], 2)],
            "cpu_model": _cpu_model(), "affinity_cpus": affinity, "threads": threads,
            "threads_note": ("torch threads = min(len(sched_getaffinity), OMP_NUM_THREADS): the GPU box's affinity "
                             "mask lists the whole machine's CPUs, but a one-GPU job's CPU share is "
                             "OMP_NUM_THREADS (16) cores, so more threads would oversubscribe that share"
                             if threads < affinity else "torch threads = len(sched_getaffinity)"),
            "context_64c128f_256rays": {"rays_per_s_median": round(c2["rays_per_s_median"], 2),
                                        "steps": context_steps, "seconds": round(c2["seconds"], 1)}}


def active_tile_fracs(*nets):
    """{M: mean fraction of the 32-sample tiles the backward ran on} from the counts the
    networks recorded (NeRF._tile_counts, the kernels' own active-tile count), then stop
    recording."""
    acc = {}
    for net in nets:
        if net is None or net._tile_counts is None:
            continue
        for M, c in net._tile_counts:
            a = acc.setdefault(M, [0, 0])
            a[0] += int(c.item())
            a[1] += (M + 31) // 32
        net._tile_counts = None
    return {M: a / t for M, (a, t) in acc.items() if t}


# tests/psnr_parity.py's analytic scene: three soft-edged coloured spheres inside the lego
# cameras' view, empty space elsewhere (white background)
SPHERES = [((0.0, 0.0, 0.0), 0.7, (0.9, 0.2, 0.1)), ((0.8, 0.3, 0.2), 0.35, (0.1, 0.7, 0.2)),
           ((-0.5, -0.6, 0.4), 0.45, (0.2, 0.3, 0.9))]


def sphere_scene_field(pts):
    sigma = torch.zeros(pts.shape[:-1], device=pts.device)
    rgb = torch.ones(*pts.shape[:-1], 3, device=pts.device)
    for c, r, col in SPHERES:
        d = (pts - torch.tensor(c, device=pts.device)).norm(dim=-1)
        sg = 40.0 * torch.sigmoid((r - d) * 40.0)
        w = (sg / (sigma + sg + 1e-6))[..., None]
        rgb = rgb * (1 - w) + torch.tensor(col, device=pts.device) * w
        sigma = sigma + sg
    return rgb, sigma


def sphere_scene_rays(size: int, device):
    """Every pixel ray of the 100 lego training cameras at size x size (views 0..89 train,
    90..99 test) and the scene's ground truth, composited by the HIP kernels at 256
    deterministic samples per ray."""
    from noisy_src import ops
    from noisy_src.rays import get_ray_directions, get_rays
    fix = sorted((ROOT / "tests" / "golden").glob("final_poses_*.npz"))[0]
    poses = torch.from_numpy(np.load(fix)["ground_truth_poses"]).float().to(device)
    focal = 0.5 * size / math.tan(0.5 * 0.6911112070083618)
    dirs = get_ray_directions(size, size, focal).to(device)
    o, d = zip(*[get_rays(dirs, p) for p in poses])
    o, d = torch.stack(o).reshape(-1, 3), torch.stack(d).reshape(-1, 3)
    with torch.no_grad():
        pts, z = ops.stratified_sample(o, d, 2.0, 6.0, 256)
        rgb, sigma = sphere_scene_field(pts)
        gt = ops.composite(rgb.contiguous(), sigma.contiguous(), z, d)[0]
    return o, d, gt


def train_sphere_state(precision: str, device, iters: int = 2000, size: int = 64, batch: int = 1024, seed: int = 0):
    """A trained state: engine.Trainer on the sphere scene for ``iters``
    iterations at ``batch`` rays from the seed-42 init.  Returns (trainer, (o, d, gt),
    number of training rays)."""
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import Trainer
    from noisy_src.model import create_nerf
    o, d, gt = sphere_scene_rays(size, device)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision=precision))
    tr = Trainer(mc.to(device), mf.to(device), RenderConfig())
    n_train = 90 * size * size
    g = torch.Generator(device=device).manual_seed(seed)
    for _ in range(iters):
        idx = torch.randint(0, n_train, (batch,), device=device, generator=g)
        tr.step(o[idx], d[idx], gt[idx])
    torch.cuda.synchronize()
    return tr, (o, d, gt), n_train


def trained_state_leg(precision: str, device, B: int = 4096, steps: int = 50, iters: int = 2000):
    """The same cfg #2 training step (64c+128f, B rays) on a TRAINED state, where the
    backward skips the tiles with exactly zero incoming gradient (empty space: sigma == 0;
    behind surfaces: transmittance underflowed to 0).  Same box, same state, alternating
    skip / dense / skip runs of ``steps`` steps (the dense form is NrMlpConfig.dense_backward,
    the reference's full backward): rays/s of each, the active-tile fraction the kernels
    counted, and the fine dW launch on the executed work (HIP events, bracketed)."""
    from noisy_src import _hip
    t0 = time.perf_counter()
    tr, (o, d, gt), n_train = train_sphere_state(precision, device, iters=iters)
    train_s = time.perf_counter() - t0
    g = torch.Generator(device=device).manual_seed(77)
    pool = []
    for _ in range(4):
        idx = torch.randint(0, n_train, (B,), device=device, generator=g)
        pool.append((o[idx].contiguous(), d[idx].contiguous(), gt[idx].contiguous()))
    nets = (tr.model_coarse, tr.model_fine)
    Mf = B * (tr.render_config.num_samples + tr.render_config.num_samples_fine)

    def run(dense: bool):
        for net in nets:
            net._nr_cfg.dense_backward = int(dense)
        for k in range(3):
            tr.step(*pool[k % 4])
        for net in nets:
            net._tile_counts = []
        timer = _hip.CallTimer(["nr_mlp_backward_dw", "nr_mlp_backward_dx"])
        _hip.set_timer(timer)
        for k in range(4):
            tr.step(*pool[k % 4])
        _hip.set_timer(None)
        act = active_tile_fracs(*nets)
        calls = timer.summary()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(steps):
            tr.step(*pool[k % 4])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        dw = calls.get(f"nr_mlp_backward_dw[M={Mf}]", (0, float("nan")))[1]
        dx = calls.get(f"nr_mlp_backward_dx[M={Mf}]", (0, float("nan")))[1]
        af = act.get(Mf, 1.0)
        return {"rays_per_s": round(B * steps / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3),
                "active_tile_frac": {str(k): round(v, 4) for k, v in sorted(act.items())},
                "fine_dw_ms_bracketed": round(dw, 4), "fine_dx_ms_bracketed": round(dx, 4),
                "fine_dw_executed_mfma_frac": round(2 * MACS_PER_EVAL * Mf * af / (dw * 1e-3) / 1e12
                                                    / PEAK_TFLOPS[precision], 4)}

    a1 = run(False)
    dn = run(True)
    a2 = run(False)
    for net in nets:
        net._nr_cfg.dense_backward = 0
    skip_v = (a1["rays_per_s"] + a2["rays_per_s"]) / 2
    return {"metric": "training rays/sec on a trained state (zero-gradient tiles skipped)",
            "workload": f"sphere scene seen by the lego training cameras (64x64 views), {iters} iterations at "
                        f"1024 rays from the seed-42 init ({train_s:.1f} s), then {B}-ray steps, "
                        f"{tr.render_config.num_samples}c+{tr.render_config.num_samples_fine}f, {precision}",
            "value": round(skip_v, 1), "unit": "rays/s",
            "dense_value": dn["rays_per_s"], "skip_over_dense": round(skip_v / dn["rays_per_s"], 4),
            "runs": {"skip_a": a1, "dense": dn, "skip_b": a2},
            "note": "same box and state, alternating; the headline value stays the bare-init cfg #2 step"}


def batch_assembly_ms(device, B: int, steps: int = 50):
    """the per-step cost of the reference's batch assembly, timed on its own
    (the reference's rays/s interval excludes it, train.py:455): RaySampler over the
    device ray table of 100 lego 800x800 training views (64 M rays, 2.3 GB resident),
    one nr_gather_rays launch per batch, and PixelSampler.sample_batch (pose-opt)."""
    from noisy_src.data import RayDataset, RaySampler, synthetic_blender_data
    from noisy_src.data_pose_opt import create_pixel_dataset
    fix = sorted((ROOT / "tests" / "golden").glob("final_poses_*.npz"))[0]
    data = synthetic_blender_data(torch.from_numpy(np.load(fix)["ground_truth_poses"]), 800, 800, device=device)
    sampler = RaySampler(RayDataset(data, B), B, shuffle=True)
    it = iter(sampler)
    _, psampler = create_pixel_dataset(data)
    psampler.batch_size = B
    out = {}
    for name, fn in (("ray_sampler", lambda: next(it)), ("pixel_sampler", psampler.sample_batch)):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out[name] = round(s.elapsed_time(e) / steps, 4)
    del sampler, it, psampler, data
    torch.cuda.empty_cache()
    return out


EVAL_METRIC = "eval render rays/sec (render_image of a full test view, chunk 4096), lego 800² 64c+128f"


def eval_bench(args, dev, world: int, rank: int, pg):
    """the eval path of the metric's test PSNR -- ``train.render_image``
    (reference train.py:122-160 / inference.py:75-105) of a whole 800x800 view of the
    lego cameras through ``NeRFRenderer`` at the reference's eval chunk of 4096 rays,
    deterministic (det=True, no perturbation), forward-only fused MLP.  One step = one
    640,000-ray image; with N ranks each renders its own views (inference.py's test
    split sharded round-robin)."""
    from noisy_src import _hip
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.model import create_nerf
    from noisy_src.rendering import NeRFRenderer
    from noisy_src.train import render_image
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision=args.precision))
    mc, mf = mc.to(dev), mf.to(dev)
    rcfg = RenderConfig(num_samples=args.num_samples, num_samples_fine=args.num_samples_fine)
    renderer = NeRFRenderer(mc, mf, rcfg)
    fix = sorted((ROOT / "tests" / "golden").glob("final_poses_*.npz"))[0]
    poses = torch.from_numpy(np.load(fix)["ground_truth_poses"]).to(dev)
    H = W = 800
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    chunk = args.eval_chunk
    views = [poses[(rank + world * k) % poses.shape[0]] for k in range(args.warmup + args.steps)]
    fwd_key = f"nr_mlp_forward[M={chunk * (rcfg.num_samples + rcfg.num_samples_fine)}]"
    for k in range(args.warmup):
        render_image(renderer, views[k], H, W, focal, chunk_size=chunk)
    timer = _hip.CallTimer(["nr_mlp_forward"], keys=[fwd_key])
    _hip.set_timer(timer)
    if pg is not None:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        out = render_image(renderer, views[args.warmup + k], H, W, focal, chunk_size=chunk)
    torch.cuda.synchronize()
    if pg is not None:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    _hip.set_timer(None)
    if pg is not None:
        tt = torch.tensor([dt], device=dev)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt)
    assert torch.isfinite(out["rgb"]).all()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)  # the last rendered view
    rays = H * W
    value = world * rays * args.steps / dt
    evals = rcfg.num_samples + (rcfg.num_samples + rcfg.num_samples_fine)
    flop_ray = 2.0 * MACS_PER_EVAL * evals  # forward only: 303.8 MFLOP per ray at 64c+128f
    calls = timer.summary()
    n_launch, ms = calls.get(fwd_key, (0, float("nan")))
    Mf = int(fwd_key.split("[M=")[1].rstrip("]"))
    fine_tf = 2.0 * MACS_PER_EVAL * Mf / (ms * 1e-3) / 1e12
    return {
        "metric": EVAL_METRIC,
        "value": round(value, 1),
        "unit": "rays/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / args.steps, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic (random-init networks; lego 800x800 training cameras of the reference's GT poses)",
        "config": {"workload": f"render_image of one 800x800 view per step per GPU, chunk {chunk}, "
                               f"{rcfg.num_samples}c+{rcfg.num_samples_fine}f, det=True",
                   "rays_per_step": rays, "chunk": chunk, "parallelism": f"views sharded over {world} GPU(s)"},
        "roofline": {"bound": "mfma", "kernel": f"mlp_fwd_rbm_kernel via nr_mlp_forward (M={Mf}, fine net, inference)",
                     "achieved": round(fine_tf, 1), "peak": PEAK_TFLOPS[args.precision], "unit": "TFLOP/s",
                     "frac": round(fine_tf / PEAK_TFLOPS[args.precision], 4), "traffic": None,
                     "work_per_launch": f"2 x {MACS_PER_EVAL} MAC x {Mf} samples", "launch_ms": round(ms, 4),
                     "launches": n_launch},
        # whole-render forward MFMA fraction: rays/s x forward FLOP per ray / (GPUs x peak)
        "flop_per_ray": flop_ray,
        "step_mfma_frac": round(value * flop_ray / (world * PEAK_TFLOPS[args.precision] * 1e12), 4),
    }


DUMP_BYTES = 64 << 20  # --dump-outputs writes at most this much in all


def dump_outputs(dirname: str, arrays) -> None:
    """Write {name: tensor} as <dirname>/<name>.npy (float32; float64 stays float64).
    Every array gets an equal share of DUMP_BYTES; a larger one is cut to a fixed, seeded
    sample of its flattened elements (ascending indices)."""
    arrays = {k: v for k, v in arrays.items() if isinstance(v, torch.Tensor)}
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    cap = DUMP_BYTES // 8 // max(1, len(arrays))  # elements per array
    for name, t in arrays.items():
        a = t.detach().to("cpu", torch.float64 if t.dtype == torch.float64 else torch.float32).numpy()
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))
            a = a.reshape(-1)[idx]
        np.save(d / f"{name}.npy", a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 200; --eval: 10 images)")
    ap.add_argument("--warmup", type=int, default=None, help="warm-up steps (default 20; --eval: 2 images)")
    ap.add_argument("--eval", action="store_true",
                    help="time the eval path instead (render_image of full 800x800 views, chunk 4096)")
    ap.add_argument("--eval-chunk", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4096, help="rays per GPU per step")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--num-samples", type=int, default=64)
    ap.add_argument("--num-samples-fine", type=int, default=128)
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling (BASELINE cfg #4): one shared global batch of this many rays, "
                         "sliced over the ranks (default 0: weak scaling, --batch rays per GPU)")
    ap.add_argument("--cpu-steps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-trained", action="store_true",
                    help="skip the trained-state line (the step on a trained sphere-scene state, skip vs dense)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the training step as one captured hipGraph (engine.GraphedTrainer; with "
                         "data parallelism the RCCL all-reduces are captured too)")
    ap.add_argument("--dp", action="store_true",
                    help="join an RCCL process group even at N=1 (the data-parallel step, all-reduce hooks active)")
    ap.add_argument("--coarse-stream", nargs="?", const="on", default="auto", choices=("auto", "on", "off"),
                    help="run the coarse network's chain (forward, loss, backward) on a second stream beside "
                         "the fine one (engine.Trainer(coarse_stream=...); with --graph: two branches of the "
                         "graph); auto (default): only in a graph replay of <= 1024 rays, where it pays")
    ap.add_argument("--pose-opt", action="store_true",
                    help="BASELINE cfg #3: joint pose optimisation step (train_pose_opt, poses optimising)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (losses, rgb_fine) and the "
                         "parameters it left as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and report everything beside the headline: per-kernel timings and "
                         "rooflines, the recorded PSNR comparison, the batch assembly cost, the trained-state "
                         "leg (--no-trained skips it) and the CPU baseline (--no-cpu-baseline skips it)")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 10 if args.eval else 200
    if args.warmup is None:
        args.warmup = 2 if args.eval else 20

    # stdout carries exactly ONE line, the JSON record: anything else written to fd 1 (the
    # RCCL init banner, library chatter) goes to stderr
    json_out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # NR_BENCH_BACKEND=gloo rehearses the multi-rank path with ranks sharing one GPU
    # (RCCL refuses two ranks on one device); the measured runs use "nccl" (= RCCL)
    backend = os.environ.get("NR_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    if world > 1 or args.dp:
        import torch.distributed as dist
        if world == 1:  # --dp without torchrun: a world-1 group of this process
            import socket
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", str(port)), ("RANK", "0"),
                         ("WORLD_SIZE", "1")):
                os.environ.setdefault(k, v)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        pg = dist.group.WORLD

    if args.eval:
        out = eval_bench(args, dev, world, rank, pg)
        if rank == 0:
            print(json.dumps(out), file=json_out, flush=True)
        if pg is not None:
            torch.distributed.destroy_process_group()
        return

    from noisy_src import _hip
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.engine import PoseTrainer, Trainer
    from noisy_src.model import create_nerf

    torch.manual_seed(42)  # train.py:319 set_seed(42); identical init on every rank
    mc, mf = create_nerf(ModelConfig(precision=args.precision))
    mc, mf = mc.to(dev), mf.to(dev)
    rcfg = RenderConfig(num_samples=args.num_samples, num_samples_fine=args.num_samples_fine)
    strong = args.global_batch > 0
    if strong:
        if args.global_batch % world:
            raise SystemExit(f"--global-batch {args.global_batch} is not divisible by {world} ranks")
        B = args.global_batch // world
        sl = slice(rank * B, (rank + 1) * B)
    else:
        B = args.batch
    if args.pose_opt:
        # rays come from (image, pixel) and the learnable poses INSIDE the step; the
        # pixel draws (sampler.sample_batch) stay outside it, as batch sampling does below
        cam, sampler = pose_opt_setup(800, 800, dev)
        sampler.batch_size = B
        trainer = PoseTrainer(mc, mf, cam, sampler, rcfg, process_group=pg)
        if strong:  # every rank draws the same global batches and takes its slice
            sampler.batch_size = args.global_batch
            gen = torch.Generator(device=dev).manual_seed(1000)
            pool = [sampler.sample_batch(generator=gen).slice(sl) for _ in range(4)]
        else:
            gen = torch.Generator(device=dev).manual_seed(1000 * rank)
            pool = [sampler.sample_batch(generator=gen) for _ in range(4)]
    else:
        trainer = Trainer(mc, mf, rcfg, process_group=pg,
                          coarse_stream={"auto": "auto", "on": True, "off": False}[args.coarse_stream])
        if strong:
            pool = [tuple(x[sl] for x in lego_rays(args.global_batch, 1000 + k, dev)) for k in range(4)]
        else:
            pool = [lego_rays(B, 1000 * rank + k, dev) for k in range(4)]
    torch.manual_seed(1234 + rank)

    def step(k):
        if args.pose_opt:
            return trainer.step(pool[k % len(pool)], optimize_poses=True)
        o, d, t = pool[k % len(pool)]
        return trainer.step(o, d, t)

    # --full: every fused-MLP entry point is timed over the last warm-up steps (kernel_ms)
    # to find the dominant kernel; inside the timed region only that kernel's launches
    # carry HIP events (each bracketed call costs a few us of queue gap).  A plain run
    # brackets nothing
    mlp_entries = ["nr_mlp_forward", "nr_mlp_backward_dx", "nr_mlp_backward_dw", "nr_mlp_backward_reduce"]
    wtimer = _hip.CallTimer(mlp_entries) if args.full else None
    # the data-parallel all-reduce is timed over the same warm-up steps (HIP events around
    # GradAllReducer's launch and wait), not inside the timed region: at small host-bound
    # batches the extra event records would lengthen the measured steps
    reducer = getattr(trainer, "reducer", None)
    for k in range(args.warmup):
        if k == args.warmup // 2:
            if reducer is not None:
                reducer.timing = []
            if args.full:
                _hip.set_timer(wtimer)
                for net in (mc, mf):  # the backward's active-tile counts (work it executed)
                    net._tile_counts = []
        step(k)
    _hip.set_timer(None)
    torch.cuda.synchronize()
    active = active_tile_fracs(mc, mf) if args.full else {}
    ar_timing = reducer.timing_summary() if reducer is not None else None
    if reducer is not None:
        reducer.timing = None
    wcalls = wtimer.summary() if args.full else {}
    # dominant kernel = largest total time per step (no warm-up: time them all live)
    dom_key = max(wcalls, key=lambda k: wcalls[k][0] * wcalls[k][1]) if wcalls else None

    if args.graph:
        # one captured hipGraph per step: no Python runs inside the timed region, so the
        # dominant kernel is timed over the eager warm-up steps above (and by rocprof)
        from noisy_src.engine import GraphedTrainer
        if args.pose_opt:
            raise SystemExit("--graph: Trainer steps only (not --pose-opt)")
        if pg is not None and backend != "nccl":
            raise SystemExit("--graph with data parallelism needs the nccl (RCCL) backend")
        gtr = GraphedTrainer(trainer, *pool[0], warmup=2)

        def step(k):  # noqa: F811
            o, d, t = pool[k % len(pool)]
            return gtr.step(o, d, t)
        for k in range(3):
            step(k)
    timer = _hip.CallTimer(mlp_entries, keys=[dom_key] if dom_key else None) if args.full else None
    _hip.set_timer(timer)
    if pg is not None:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    # per-step HIP events on the launching stream (no host sync inside the loop) give the
    # step-time distribution; value itself is the whole timed region
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        evs[k].record()
        m = step(k)
    evs[-1].record()
    torch.cuda.synchronize()
    if pg is not None:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    _hip.set_timer(None)
    loss = float(m["loss"])
    if pg is not None:
        tt = torch.tensor([dt], device=dev)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt)

    per_step = sorted(a.elapsed_time(b) for a, b in zip(evs, evs[1:]))
    step_pcts = [round(per_step[min(len(per_step) - 1, int(q * len(per_step)))], 4) for q in (0.1, 0.5, 0.9)]
    topology = None
    if pg is not None:
        topology = rank_topology(pg, dev, step_pcts[1], ar_timing)
    if args.dump_outputs and rank == 0:
        # what a caller of the timed step holds after the last one: the metrics it returned
        # and the parameters (and, with --pose-opt, the poses) it left
        arrays = dict(m, params_coarse=mc.flat_params(), params_fine=mf.flat_params())
        if args.pose_opt:
            arrays["poses"] = torch.cat([p.detach().reshape(-1) for p in cam.parameters()])
        dump_outputs(args.dump_outputs, arrays)
    if args.full:
        calls = timer.summary() if not args.graph else {dom_key: wcalls[dom_key]}
        if dom_key is None:
            wcalls = calls
            dom_key = max(calls, key=lambda k: calls[k][0] * calls[k][1])
        n_launch, ms = calls[dom_key]  # live, over the timed region
        entry, M = dom_key.split("[M=")[0], int(dom_key.split("[M=")[1].rstrip("]"))
        kern = KERNEL_OF.get(entry, (entry,))
        dom_traffic = traffic_of(kern, M, args.precision)
        n_params = mf.flat_params().numel()
        bound, achieved, peak, unit, work = roofline_of(entry, M, ms, args.precision, n_params, dom_traffic)
        mf_tf, _, mf_work = mfma_roofline(entry, M, ms, args.precision)
        dom_active = active.get(M, 1.0) if entry != "nr_mlp_forward" else 1.0
        if not mfma_macs_of(entry):
            # a dominant launch without MFMA work (e.g. the slab reduction): its byte roofline
            mf_tf, mf_work = None, work
        elif dom_active < 1.0:
            mf_work += f" x active-tile fraction {dom_active:.4f}"
        # the committed rocprofv3 kernel trace of this tree (same bench command): its average
        # for the dominant kernel, and the fraction it gives
        rp_rows, rp_src = rocprof_summary(args.precision)
        rp = next((rp_rows[(k, M)] for k in kern if (k, M) in rp_rows), None)
        rp_ms = float(rp.get("timed_avg_ms") or rp["avg_ms"]) if rp else None
        ktab, step_bytes = kernel_table(wcalls, args.precision, n_params, rp_rows, active)
    value = world * B * args.steps / dt
    out = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "rays/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / args.steps, 3),
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic (lego 800x800 camera rays from the reference's GT poses; random targets)",
        "config": {
            "workload": (f"lego 800x800 joint pose-opt (5 deg rot + 5% trans noisy init, SE(3) pose grads) "
                         if args.pose_opt else "lego 800x800 ")
                        + f"hierarchical {rcfg.num_samples}c+{rcfg.num_samples_fine}f training step, "
                        + (f"global batch {args.global_batch} rays sliced over {world} GPU(s)" if strong
                           else f"{B} rays per GPU"),
            "global_batch": world * B,
            "num_samples": rcfg.num_samples,
            "num_samples_fine": rcfg.num_samples_fine,
            "parallelism": f"dp{world}" + (" (RCCL process group, all-reduce in the step)" if pg is not None
                                           and world == 1 else ""),
            **({"execution": "hipGraph replay (engine.GraphedTrainer)"} if args.graph else {}),
            **({"coarse_stream": "coarse chain on a second stream"}
               if getattr(trainer, "last_step_coarse_stream", False) else {}),
        },
        # whole-step MFMA fraction: rays/s x training FLOP/ray / (GPUs x peak)
        "step_mfma_frac": round(value * 6 * MACS_PER_EVAL * (2 * rcfg.num_samples + rcfg.num_samples_fine)
                                / (world * PEAK_TFLOPS[args.precision] * 1e12), 4),
        "step_ms_p10_p50_p90": step_pcts,
        "final_loss": round(loss, 6),
    }
    if args.full:
        out.update({
            # headline: the dominant kernel on SURVEY §8d's MFMA basis (algorithmic FLOPs per
            # launch over its launch time); the stored-activation HBM view rides beside it
            "roofline": {
                # frac: from the committed rocprof kernel-trace average of these sources when
                # one exists (reproducible from profiles/), else from the live launch time;
                # MFMA basis, or the byte basis for a launch without MFMA work
                **(headline_roofline(mf_tf, ms, rp_ms, args.precision, dom_active) if mf_tf is not None else {
                    "bound": bound, "achieved": round(achieved * ms / rp_ms if rp_ms else achieved, 2), "peak": peak,
                    "unit": unit, "frac": round((achieved * ms / rp_ms if rp_ms else achieved) / peak, 4)}),
                "kernel": f"{kern[0]} via {entry} (M={M} samples, fine net)",
                "frac_basis": (f"rocprof_ms: timed-region average of {rp_src} (same source_hash)" if rp_ms
                               else "launch_ms: HIP events on the launching stream over the eager warm-up steps "
                               "(a graph replay runs no Python)" if args.graph
                               else "launch_ms: live HIP events on the launching stream over the timed region"),
                "traffic": dom_traffic,
                "work_per_launch": mf_work,
                # the backward's executed share of the 32-sample tiles of this launch (tiles with
                # a nonzero incoming gradient, counted by the kernels over the warm-up steps)
                "active_tile_frac": round(dom_active, 4),
                # HIP events around each launch over the timed region: carries queue gaps, so it
                # is context only (no fraction is taken from it when a rocprof average exists)
                "launch_ms_bracketed": round(ms, 4),
                "launches": n_launch,
                "rocprof_ms": round(rp_ms, 4) if rp_ms else None,
                "rocprof_source": rp_src if rp_ms else None,
                "source_hash": source_hash(),
                "stored_activation_bytes_design": {
                    "bound": bound, "achieved": round(achieved * ms / rp_ms if rp_ms else achieved, 2), "peak": peak,
                    "unit": unit, "frac": round((achieved * ms / rp_ms if rp_ms else achieved) / peak, 4),
                    "work_per_launch": work,
                    "note": "bytes this decomposition chooses to store and re-read (saved activations, dz), "
                            "not algorithmic work"},
            },
            # per fused-MLP launch: live ms (last warm-up steps), counted PMC bytes and their
            # rate, MFMA / HBM floors and the bound they give (profiles/traffic.json)
            "kernels": ktab,
            # the step's counted MLP bytes over the step time, against 8 TB/s
            "step_hbm_bytes": step_bytes or None,
            "step_hbm_frac": round(step_bytes / (dt / args.steps) / (PEAK_HBM_GBS * 1e9), 4) if step_bytes else None,
            # per-launch ms of every fused-MLP key: the rocprof timed-region average where the
            # committed same-source summary has it, else the bracketed warm-up mean (labelled)
            "kernel_ms": {k: v["ms"] for k, v in ktab.items()},
            "kernel_ms_source": sorted({v["ms_source"] for v in ktab.values()}),
            # each key launches once per step: the fused-MLP launches' share of ms_per_step
            "kernel_ms_sum": round(sum(v["ms"] for v in ktab.values()), 4),
            "active_tile_frac": {str(k): round(v, 4) for k, v in sorted(active.items())},
            # the lego test split is not available offline: the PSNR half of the
            # metric is the recorded equal-iteration comparison on the analytic scene
            "psnr": psnr_record(),
        })
    if topology is not None:
        out["topology"] = topology
    if args.full and rank == 0 and world == 1:
        out["batch_assembly_ms_per_step"] = batch_assembly_ms(dev, B)
    if (args.full and rank == 0 and world == 1 and not args.pose_opt and not args.graph and not strong
            and not args.no_trained and (rcfg.num_samples, rcfg.num_samples_fine) == (64, 128)):
        out["trained_state"] = trained_state_leg(args.precision, dev, B=B)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.pose_opt:
        out["cpu_baseline"] = cpu_baseline(steps=args.cpu_steps)
    if rank == 0:
        print(json.dumps(out), file=json_out, flush=True)
    if pg is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
