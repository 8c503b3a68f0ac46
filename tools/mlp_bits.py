"""One SHA-256 per output array of every nr_mlp_* entry point, and the A/B of two builds.

    NR_HIP_LIB=/path/to/lib.so python tools/mlp_bits.py            # the hashes of one library
    python tools/mlp_bits.py --compare OLD.so NEW.so [--json OUT]  # both, each in a fresh child

The first form loads the library that NR_HIP_LIB names (default: the tree's build), runs the
entry points on fixed seeded inputs and prints ``<case>/<array> <sha256>`` lines.  The second
runs it once per library, each in a fresh child process with its own time limit, stops at the
first child that fails, and compares the two outputs line by line: a refactor of the fused
MLP's host layer or kernels changes no line.  Exit status 1 when a line differs.

Cases.  Precisions fp32, bf16, fp16.  Models: the default (XB = 2, DB = 1), the default without
view directions (DB = 0), pos_freqs = 4 with and without view directions (XB = 1), depth 1
without skips (the trunk loops run zero times), depth 12 with skips at 4 and 8 (the 16-bit dX
chain takes its masks-in-place instance).  M = 0, 1, 33 (a ragged second tile), 257 (9 tiles:
more than one workgroup in every chain) and 8,193 (257 tiles: a second 256-tile segment).
Incoming gradients: dense random, all zero (every workgroup idle), every tile with index
= 1 (mod 3) zeroed, and at M = 8,193 only the last tile active.  dense_backward = 1 once per
precision, on the default model.  Calls: nr_mlp_pack, nr_mlp_pack_table, nr_mlp_fold_window
with a ramp window and a forward on its images, nr_mlp_window_grad, nr_mlp_forward with and
without `saved`, nr_mlp_backward_dx with no input gradient, with g_x alone and with both,
nr_mlp_backward_dw, nr_mlp_backward_reduce and the active-tile count, nr_mlp_forward_frozen and
nr_mlp_backward_input with both gradients and with g_x alone.

Output buffers start as NaN; `saved` and `workspace` are filled with the byte 0xA5 before each
call and hashed whole, so the bytes a call leaves alone compare equal.  There is no CPU path."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]
CHILD_TIMEOUT_S = 90
NAN = float("nan")
# name: pos_freqs, dir_freqs, n_layers, skip_mask, use_view_dirs
MODELS = {
    "default": (10, 4, 8, 1 << 4, 1),
    "default_novd": (10, 4, 8, 1 << 4, 0),
    "pos4": (4, 4, 8, 1 << 4, 1),
    "pos4_novd": (4, 4, 8, 1 << 4, 0),
    "depth1": (10, 4, 1, 0, 1),
    "depth12_skips4_8": (10, 4, 12, (1 << 4) | (1 << 8), 1),
}
PRECS = {"fp32": 0, "bf16": 1, "fp16": 2}
SIZES = (0, 1, 33, 257, 8193)


def hashes() -> int:
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mlp_bits: no GPU found (there is no CPU path)")
    from noisy_src import _hip
    from noisy_src._hip import NrMlpConfig, call, ptr

    lib = _hip.load()
    st = _hip.stream_ptr()
    dev = "cuda"
    print(f"# {_hip.lib_path().name}", file=sys.stderr)

    # hashing (which releases the GIL) runs on a few threads behind the GPU work; the lines
    # are printed in the order of the calls, at most kPending arrays waiting
    pool, pending, kPending = ThreadPoolExecutor(8), deque(), 24

    def drain(limit):
        while len(pending) > limit:
            label, fut = pending.popleft()
            print(f"{label} {fut.result()}")

    def emit(case, **arrays):
        for name, t in arrays.items():
            host = t.cpu().contiguous().numpy()
            pending.append((f"{case}/{name}", pool.submit(lambda h=host: hashlib.sha256(h).hexdigest())))
        drain(kPending)

    def nans(rows, *shape):  # at least one row: the entry points refuse a null pointer before they look at M
        return torch.full((max(rows, 1), *shape), NAN, device=dev)

    def rand(gen, *shape):
        return torch.randn(*shape, generator=gen).to(dev)

    def raw(nbytes):  # a buffer of 0xA5 bytes, 256-byte aligned by the allocator
        return torch.full((max(int(nbytes), 16),), 0xA5, dtype=torch.uint8, device=dev)

    def grads(gen, M, pattern):
        R = max(M, 1)
        g_rgb, g_sigma = torch.randn(R, 3, generator=gen) * 1e-3, torch.randn(R, generator=gen) * 1e-3
        tile = torch.arange(R) // 32
        keep = {"dense": torch.ones(R, dtype=torch.bool), "zero": torch.zeros(R, dtype=torch.bool),
                "mod3": tile % 3 != 1, "last": tile == (M - 1) // 32}[pattern]
        return (g_rgb * keep[:, None]).to(dev), (g_sigma * keep).to(dev)

    def backward(case, cfg, M, packed, params, x, d, use_vd, n_params, g_rgb, g_sigma):
        c = ctypes.byref(cfg)
        rgb, sigma = nans(M, 3), nans(M)
        saved = raw(lib.nr_mlp_saved_bytes(c, M))
        call("nr_mlp_forward", c, ptr(packed), ptr(params), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(saved), st)
        ws_bytes = lib.nr_mlp_workspace_bytes(c, M)
        modes = ("none", "g_x") + (("both",) if use_vd else ())
        for mode in modes:
            ws = raw(ws_bytes)
            g_x = nans(M, 3) if mode != "none" else None
            g_d = nans(M, 3) if mode == "both" else None
            call("nr_mlp_backward_dx", c, ptr(packed), ptr(params), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(saved),
                 ptr(g_rgb), ptr(g_sigma), ptr(g_x), ptr(g_d), ptr(ws), st)
            out = {"workspace": ws}
            if g_x is not None:
                out["g_x"] = g_x
            if g_d is not None:
                out["g_d"] = g_d
            if M > 0:
                off = lib.nr_mlp_active_tiles_offset(c, M)
                out["active_tiles"] = ws[off:off + 4]
            emit(f"{case}/backward_dx/{mode}", **out)
        # the dW GEMM and its reduction, over what the last dX call left
        g_params = nans(n_params)
        call("nr_mlp_backward_dw", c, M, ptr(saved), ptr(ws), st)
        call("nr_mlp_backward_reduce", c, M, ptr(ws), ptr(g_params), st)
        emit(f"{case}/backward_dw_reduce", workspace=ws, g_params=g_params)

    def frozen_backward(case, cfg, M, packed, params, x, d, use_vd, g_rgb, g_sigma, rgb, sigma, saved_f):
        c = ctypes.byref(cfg)
        ws_bytes = lib.nr_mlp_frozen_workspace_bytes(c, M)
        for mode in ("g_x",) + (("both",) if use_vd else ()):
            ws = raw(ws_bytes)
            g_x, g_d = nans(M, 3), nans(M, 3) if mode == "both" else None
            call("nr_mlp_backward_input", c, ptr(packed), ptr(params), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma),
                 ptr(saved_f), ptr(g_rgb), ptr(g_sigma), ptr(g_x), ptr(g_d), ptr(ws), st)
            out = {"workspace": ws, "g_x": g_x}
            if g_d is not None:
                out["g_d"] = g_d
            emit(f"{case}/backward_input/{mode}", **out)

    for pname, prec in PRECS.items():
        for mname, (L, Ld, n, skips, use_vd) in MODELS.items():
            cfg = NrMlpConfig(L, Ld, 256, n, skips, use_vd, prec, 0)
            c = ctypes.byref(cfg)
            gen = torch.Generator().manual_seed(1000 * prec + len(mname))
            n_params = lib.nr_mlp_param_count(c)
            if n_params < 0:
                raise SystemExit(f"mlp_bits: {pname}/{mname} refused: {_hip.last_error()}")
            params = (torch.randn(n_params, generator=gen) * 0.08).to(dev)
            top = f"{pname}/{mname}"
            # ---- packing, its destination table, the positional-encoding window
            packed = raw(lib.nr_mlp_packed_bytes(c))
            call("nr_mlp_pack", c, ptr(params), ptr(packed), st)
            table = raw(lib.nr_mlp_pack_table_bytes(c))
            call("nr_mlp_pack_table", c, ptr(table.view(torch.int32)), st)
            emit(f"{top}/pack", packed=packed, table=table)
            w_pos = torch.linspace(0, 1, L).to(dev)
            w_dir = torch.linspace(0, 1, Ld).to(dev) if use_vd else None
            folded = packed.clone()
            call("nr_mlp_fold_window", c, ptr(params), ptr(w_pos), ptr(w_dir), ptr(folded), st)
            g_win = rand(gen, n_params)
            call("nr_mlp_window_grad", c, ptr(w_pos), ptr(w_dir), ptr(g_win), st)
            emit(f"{top}/window", folded=folded, window_grad=g_win)
            for M in SIZES:
                case = f"{top}/M{M}"
                x = (torch.rand(max(M, 1), 3, generator=gen) * 3 - 1.5).to(dev)
                d = torch.nn.functional.normalize(torch.randn(max(M, 1), 3, generator=gen), dim=-1).to(dev) if use_vd else None
                # ---- the three forwards, and one on the windowed images
                for tag, images in (("forward_infer", packed), ("forward_window", folded)):
                    rgb, sigma = nans(M, 3), nans(M)
                    call("nr_mlp_forward", c, ptr(images), ptr(params), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), None, st)
                    emit(f"{case}/{tag}", rgb=rgb, sigma=sigma)
                rgb, sigma = nans(M, 3), nans(M)
                saved = raw(lib.nr_mlp_saved_bytes(c, M))
                call("nr_mlp_forward", c, ptr(packed), ptr(params), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(saved), st)
                emit(f"{case}/forward_train", rgb=rgb, sigma=sigma, saved=saved)
                rgb, sigma = nans(M, 3), nans(M)
                saved_f = raw(lib.nr_mlp_frozen_saved_bytes(c, M))
                call("nr_mlp_forward_frozen", c, ptr(packed), ptr(params), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma),
                     ptr(saved_f), st)
                emit(f"{case}/forward_frozen", rgb=rgb, sigma=sigma, saved_frozen=saved_f)
                # ---- the backwards, per pattern of incoming gradient
                for pattern in ("dense", "zero", "mod3") + (("last",) if M == SIZES[-1] else ()):
                    g_rgb, g_sigma = grads(gen, M, pattern)
                    backward(f"{case}/{pattern}", cfg, M, packed, params, x, d, use_vd, n_params, g_rgb, g_sigma)
                    frozen_backward(f"{case}/{pattern}", cfg, M, packed, params, x, d, use_vd, g_rgb, g_sigma, rgb, sigma,
                                    saved_f)
                if mname == "default" and M == 257:  # every tile through the backward, some with zero gradients
                    dense = NrMlpConfig(L, Ld, 256, n, skips, use_vd, prec, 1)
                    g_rgb, g_sigma = grads(gen, M, "mod3")
                    backward(f"{case}/mod3_dense_backward", dense, M, packed, params, x, d, use_vd, n_params, g_rgb, g_sigma)
    torch.cuda.synchronize()
    drain(0)
    return 0


def compare(old: str, new: str, out) -> int:
    runs = []
    for lib in (old, new):
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, __file__], env={**os.environ, "NR_HIP_LIB": str(Path(lib).resolve())},
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:  # run() has killed the child
            print(f"mlp_bits: the child for {lib} passed its {CHILD_TIMEOUT_S} s limit; nothing more was run")
            return 2
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
            print(f"mlp_bits: the child for {lib} ended with status {r.returncode}; nothing more was run")
            return 2
        lines = dict(ln.split() for ln in r.stdout.splitlines() if ln and not ln.startswith("#"))
        runs.append({"lib": lib, "sha256": hashlib.sha256(Path(lib).read_bytes()).hexdigest(), "arrays": len(lines),
                     "seconds": round(time.time() - t0, 1), "lines": lines})
    a, b = runs[0]["lines"], runs[1]["lines"]
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    digest = hashlib.sha256("".join(f"{k} {v}\n" for k, v in sorted(a.items())).encode()).hexdigest()
    res = {"tool": "tools/mlp_bits.py", "command": f"python tools/mlp_bits.py --compare {old} {new}",
           "old": {k: v for k, v in runs[0].items() if k != "lines"},
           "new": {k: v for k, v in runs[1].items() if k != "lines"},
           "old_lines_sha256": digest, "differing_lines": differ, "identical": not differ}
    print(json.dumps(res, indent=1))
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(res, indent=1) + "\n")
    return 1 if differ else 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--json")
    args = ap.parse_args()
    return compare(*args.compare, args.json) if args.compare else hashes()


if __name__ == "__main__":
    sys.exit(main())
