"""One SHA-256 per output array of the compositing entry points of composite.hip and of
nr_sample_hierarchical, and (``time``) the duration of the compositing entry points.

Loads the library that NR_HIP_LIB names (default: the tree's build), runs the entry points
below on the seeded inputs of tests/edge_inputs.py through the raw ABI and prints
``<case>/<output> <sha256>`` lines.  Run it once per library, each in a fresh process, and
diff the two outputs: a refactor of composite.hip or sampling.hip changes no line.

    NR_HIP_LIB=/path/to/parent.so python tools/composite_bits.py > parent.txt
    python tools/composite_bits.py > tree.txt && diff parent.txt tree.txt

Cases: nr_composite_fwd (depth / acc / weights present and NULL), nr_composite_bwd (g_depth /
g_acc / g_w all present and all NULL, g_rays_d present and NULL; its g_map is nr_mse_fwd_bwd's
gradient of the forward's rgb_map, whose loss word is hashed as well), nr_composite_mse
(nullable outputs, g_rays_d and the ticket each present and NULL; the loss word and the ticket
are hashed) and nr_composite_robust (the five loss kinds at c = 0.1, the ticket present and
NULL; both loss words and the ticket are hashed) at S = 1 .. 600 (wave per ray up to 512,
thread per ray beyond), B = 1, 3, 5 (dead waves in the last workgroup) and 700, both
backgrounds, the three regimes of edge_inputs; nr_composite_mse and nr_composite_robust also
at B = 4096, S = 64, where the entry points drop the ticket.
nr_sample_hierarchical at edge_inputs.HIER_SIZES (sample_hier_kernel<1, 2, 4, 8>) and at
(256, 512) (the long kernel), B = 1 and 5, points, view directions and u each present and NULL.
Every output buffer starts as NaN; g_rays_d, which is accumulated, starts from the case's
seeded non-zero buffer.

``time`` prints one JSON line: microseconds per launch of the three entry points at B = 4096,
S = 64 and 192, the median of REPEATS windows of LAUNCHES launches between two HIP events.
There is no CPU path."""
import hashlib
import itertools
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd"), str(ROOT / "tests")]
DEV = "cuda"
NAN = float("nan")
BITS_S = (1, 2, 63, 64, 65, 130, 192, 511, 512, 513, 600)
BITS_B = (1, 3, 5, 700)
LOSS_KINDS, ROBUST_C = ("mse", "huber", "charbonnier", "cauchy", "geman_mcclure"), 0.1  # the header's NR_LOSS_* order
LAUNCHES, REPEATS, WARMUP = 200, 5, 50


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def emit(case, **arrays):
    for name, t in arrays.items():
        print(f"{case}/{name} {hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()}")


def device_case(S, B, regime):
    import edge_inputs as ei
    return {k: (None if v is None else v.to(DEV)) for k, v in ei.composite_inputs(S, B, regime).items()}


def composite_bits(S, B, white, regime, mse_only=False):
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    stream = _hip.stream_ptr()
    c = device_case(S, B, regime)
    front = [ptr(c[k]) for k in ("rgb", "sigma", "z", "rd", "noise")]
    case = f"S{S}/B{B}/white{white}/{regime}"
    scale = 0.5
    for outs in ((True, False) if not mse_only else ()):
        o = dict(rgb_map=nans(B, 3))
        if outs:
            o.update(depth=nans(B), acc=nans(B), weights=nans(B, S))
        call("nr_composite_fwd", *front, B, S, white, ptr(o["rgb_map"]), ptr(o.get("depth")), ptr(o.get("acc")),
             ptr(o.get("weights")), stream)
        emit(f"composite_fwd/{case}/outs{int(outs)}", **o)
        if outs:  # the seed of the backward: nr_mse_fwd_bwd on this rgb_map
            loss, g_map = nans(1), nans(B, 3)
            call("nr_mse_fwd_bwd", ptr(o["rgb_map"]), ptr(c["target"]), B, scale, ptr(loss), ptr(g_map), stream)
            emit(f"mse_fwd_bwd/{case}", loss=loss, g_map=g_map)
            call("nr_mse_fwd_bwd", ptr(o["rgb_map"]), ptr(c["target"]), B, scale, ptr(loss), None, stream)
            emit(f"mse_fwd_bwd/{case}/g_null", loss=loss)
    for with_g, with_rd in (itertools.product((True, False), repeat=2) if not mse_only else ()):
        o = dict(g_rgb=nans(B, S, 3), g_sigma=nans(B, S))
        if with_rd:
            o["g_rays_d"] = c["rd_init"].clone()
        g = [ptr(c[k]) if with_g else None for k in ("g_depth", "g_acc", "g_w")]
        call("nr_composite_bwd", *front, B, S, white, ptr(g_map), *g, ptr(o["g_rgb"]), ptr(o["g_sigma"]),
             ptr(o.get("g_rays_d")), stream)
        emit(f"composite_bwd/{case}/g{int(with_g)}/rd{int(with_rd)}", **o)
    ws_bytes = int(_hip.load().nr_composite_mse_workspace_bytes(B))
    for outs, with_rd, ticket in itertools.product((True, False), repeat=3):
        o = dict(rgb_map=nans(B, 3), loss=nans(1), g_rgb=nans(B, S, 3), g_sigma=nans(B, S))
        if outs:
            o.update(depth=nans(B), acc=nans(B), weights=nans(B, S))
        if with_rd:
            o["g_rays_d"] = c["rd_init"].clone()
        if ticket:
            o["ticket"] = torch.zeros(4, device=DEV, dtype=torch.int32)
        ws = nans(ws_bytes // 4)
        call("nr_composite_mse", *front, ptr(c["target"]), B, S, white, scale, ptr(o["rgb_map"]), ptr(o.get("depth")),
             ptr(o.get("acc")), ptr(o.get("weights")), ptr(o["loss"]), ptr(o["g_rgb"]), ptr(o["g_sigma"]),
             ptr(o.get("g_rays_d")), ptr(o.get("ticket")), ptr(ws), stream)
        emit(f"composite_mse/{case}/outs{int(outs)}/rd{int(with_rd)}/ticket{int(ticket)}", **o)
    ws_bytes = int(_hip.load().nr_composite_robust_workspace_bytes(B))
    for (kind, name), ticket in itertools.product(enumerate(LOSS_KINDS), (True, False)):
        o = dict(rgb_map=nans(B, 3), depth=nans(B), acc=nans(B), weights=nans(B, S), loss2=nans(2), g_rgb=nans(B, S, 3),
                 g_sigma=nans(B, S), g_rays_d=c["rd_init"].clone())
        if ticket:
            o["ticket"] = torch.zeros(4, device=DEV, dtype=torch.int32)
        ws = nans(ws_bytes // 4)
        call("nr_composite_robust", *front, ptr(c["target"]), B, S, white, kind, ROBUST_C, scale, ptr(o["rgb_map"]),
             ptr(o["depth"]), ptr(o["acc"]), ptr(o["weights"]), ptr(o["loss2"]), ptr(o["g_rgb"]), ptr(o["g_sigma"]),
             ptr(o["g_rays_d"]), ptr(o.get("ticket")), ptr(ws), stream)
        emit(f"composite_robust/{case}/{name}/ticket{int(ticket)}", **o)


def hier_bits():
    import edge_inputs as ei
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    stream = _hip.stream_ptr()
    for (Nc, Nf), B in itertools.product(list(ei.HIER_SIZES) + [(256, 512)], (1, 5)):
        o, d, z, w, u = (t.to(DEV) for t in ei.hier_inputs(Nc, Nf, B))
        T = Nc + Nf
        for pts, vd, with_u in itertools.product((True, False), repeat=3):
            out = dict(z_fine=nans(B, T))
            if pts:
                out["pts"] = nans(B, T, 3)
            if vd:
                out["viewdirs"] = nans(B * T, 3)
            call("nr_sample_hierarchical", ptr(o), ptr(d), ptr(z), ptr(w), ptr(u) if with_u else None, B, Nc, Nf,
                 ptr(out["z_fine"]), ptr(out.get("pts")), ptr(out.get("viewdirs")), stream)
            emit(f"sample_hierarchical/Nc{Nc}_Nf{Nf}/B{B}/pts{int(pts)}/vd{int(vd)}/u{int(with_u)}", **out)


def bits():
    import edge_inputs as ei
    for S, B, white, regime in itertools.product(BITS_S, BITS_B, (1, 0), ei.REGIMES):
        composite_bits(S, B, white, regime)
    for white, regime in itertools.product((1, 0), ei.REGIMES):
        composite_bits(64, 4096, white, regime, mse_only=True)
    hier_bits()


def median_us(launch):
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            launch()
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b) / LAUNCHES)
    return round(statistics.median(us), 3), [round(x, 3) for x in us]


def time_entries():
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    stream = _hip.stream_ptr()
    B = 4096
    out = {"lib": os.path.relpath(_hip.lib_path(), ROOT), "launches": LAUNCHES, "repeats": REPEATS, "B": B, "us": {}}
    for S in (64, 192):
        c = device_case(S, B, "random")
        front = [ptr(c[k]) for k in ("rgb", "sigma", "z", "rd", "noise")]
        rgb_map, depth, acc, weights = nans(B, 3), nans(B), nans(B), nans(B, S)
        loss, g_rgb, g_sigma, g_rd = nans(1), nans(B, S, 3), nans(B, S), torch.zeros(B, 3, device=DEV)
        ticket = torch.zeros(4, device=DEV, dtype=torch.int32)
        ws = nans(int(_hip.load().nr_composite_mse_workspace_bytes(B)) // 4)
        entries = {
            "nr_composite_fwd": lambda: call("nr_composite_fwd", *front, B, S, 1, ptr(rgb_map), ptr(depth), ptr(acc),
                                             ptr(weights), stream),
            "nr_composite_bwd": lambda: call("nr_composite_bwd", *front, B, S, 1, ptr(c["g_map"]), None, None, None,
                                             ptr(g_rgb), ptr(g_sigma), ptr(g_rd), stream),
            "nr_composite_mse": lambda: call("nr_composite_mse", *front, ptr(c["target"]), B, S, 1, 1.0, ptr(rgb_map),
                                             ptr(depth), ptr(acc), ptr(weights), ptr(loss), ptr(g_rgb), ptr(g_sigma),
                                             ptr(g_rd), ptr(ticket), ptr(ws), stream),
        }
        for name, launch in entries.items():
            med, windows = median_us(launch)
            out["us"][f"{name}/S{S}"] = {"median": med, "windows": windows}
    print(json.dumps(out))


def main() -> int:
    if not torch.cuda.is_available():
        raise SystemExit("composite_bits: no GPU found (there is no CPU path)")
    from noisy_src import _hip
    _hip.load()
    print(f"# {_hip.lib_path()}", file=sys.stderr)
    if sys.argv[1:] == ["time"]:
        time_entries()
    elif not sys.argv[1:]:
        bits()
    else:
        raise SystemExit("usage: composite_bits.py [time]")
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
