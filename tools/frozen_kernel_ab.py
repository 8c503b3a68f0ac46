"""Kernel-level A/B of the frozen-field MLP pair (default model; bf16, or --precision) on one
GPU: the saving forward, the masks-only forward and the inference forward; the dX stage with
and without input gradients against the input-only backward; and the dW GEMM + reduce a frozen
step no longer runs.  NR_HIP_LIB selects the library, so two builds are timed in two runs.
Raw C-ABI calls on buffers made once, HIP events around each call, the legs alternating,
20 warm-up rounds and 200 timed ones at M = 98,304 and 786,432 (512 and 4,096 rays of 192
fine samples).  Writes the medians and the 10th / 90th percentiles to
profiles/frozen_kernel_ab.json (or the path given).  No CPU path.

python tools/frozen_kernel_ab.py [OUT.json] [--precision bf16|fp16|fp32]"""
import argparse, ctypes, json, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]
import torch
from noisy_src import _hip
from noisy_src._hip import call, ptr
from noisy_src.config import ModelConfig
from noisy_src.model import NeRF

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=str(ROOT / "profiles" / "frozen_kernel_ab.json"))
ap.add_argument("--precision", default="bf16", choices=("bf16", "fp16", "fp32"))
args = ap.parse_args()
dev = "cuda"
torch.manual_seed(0)
net = NeRF(ModelConfig(precision=args.precision)).to(dev)
net._ensure_flat()
packed = net._packed_for_forward()
cfg = ctypes.byref(net._nr_cfg)
lib = _hip.load()
out = {}
for M in (98304, 786432):
    x = (torch.rand(M, 3, device=dev) * 3 - 1.5)
    d = torch.nn.functional.normalize(torch.randn(M, 3, device=dev), dim=-1)
    rgb, sigma = torch.empty(M, 3, device=dev), torch.empty(M, device=dev)
    g_rgb = torch.randn(M, 3, device=dev) * 1e-4
    g_sigma = torch.randn(M, device=dev) * 1e-4
    g_x, g_d = torch.empty(M, 3, device=dev), torch.empty(M, 3, device=dev)
    sv_t = torch.empty(lib.nr_mlp_saved_bytes(cfg, M), dtype=torch.uint8, device=dev)
    sv_f = torch.empty(lib.nr_mlp_frozen_saved_bytes(cfg, M), dtype=torch.uint8, device=dev)
    ws_t = torch.empty(lib.nr_mlp_workspace_bytes(cfg, M), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(lib.nr_mlp_frozen_workspace_bytes(cfg, M), dtype=torch.uint8, device=dev)
    st = _hip.stream_ptr()
    legs = {
        "fwd_train": lambda: call("nr_mlp_forward", cfg, ptr(packed), ptr(net._flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(sv_t), st),
        "fwd_frozen": lambda: call("nr_mlp_forward_frozen", cfg, ptr(packed), ptr(net._flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(sv_f), st),
        "fwd_infer": lambda: call("nr_mlp_forward", cfg, ptr(packed), ptr(net._flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), None, st),
        "bwd_dx": lambda: call("nr_mlp_backward_dx", cfg, ptr(packed), ptr(net._flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(sv_t), ptr(g_rgb), ptr(g_sigma), ptr(g_x), ptr(g_d), ptr(ws_t), st),
        "bwd_dx_noinput": lambda: call("nr_mlp_backward_dx", cfg, ptr(packed), ptr(net._flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(sv_t), ptr(g_rgb), ptr(g_sigma), None, None, ptr(ws_t), st),
        "bwd_input": lambda: call("nr_mlp_backward_input", cfg, ptr(packed), ptr(net._flat), ptr(x), ptr(d), M, ptr(rgb), ptr(sigma), ptr(sv_f), ptr(g_rgb), ptr(g_sigma), ptr(g_x), ptr(g_d), ptr(ws_f), st),
        "bwd_dw_reduce": lambda: (call("nr_mlp_backward_dw", cfg, M, ptr(sv_t), ptr(ws_t), st), call("nr_mlp_backward_reduce", cfg, M, ptr(ws_t), ptr(torch.empty(net._param_count, device=dev)), st)),
    }
    # valid state for every leg
    legs["fwd_train"](); legs["fwd_frozen"](); legs["bwd_dx"](); legs["bwd_input"]()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for it in range(20 + 200):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if it >= 20:
                times[k].append(e0.elapsed_time(e1))
    res = {k: {"median_ms": statistics.median(v), "p10": sorted(v)[len(v)//10], "p90": sorted(v)[9*len(v)//10]} for k, v in times.items()}
    out[M] = res
    print(M, json.dumps(res), flush=True)
dst = Path(args.out)
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text(json.dumps({"tool": "tools/frozen_kernel_ab.py", "lib": _hip.lib_path().name, "precision": args.precision, "warmup": 20, "timed": 200,
                           "unit": "ms", "results": out}, indent=1) + "\n")
