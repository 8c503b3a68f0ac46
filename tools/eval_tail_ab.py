"""The per-image tail of the evaluation loop, host form against fused form, on one GPU.

One 800 x 800 view is rendered once from a random-init bf16 renderer (the image content
does not matter to either form's cost).  The tail is what ``evaluate_test_set`` does with
it after the render: PSNR / SSIM / MSE as host floats, and the pred, gt, comparison and
depth frames as host uint8 arrays (PNG encoding, identical in both forms, is left out).

* host:  ``compute_psnr`` / ``compute_ssim`` / ``compute_mse`` with one ``.item()`` each,
  fp32 device-to-host copies and numpy quantisation, ``depth_to_colormap`` on the host.
* fused: ``metrics.image_metrics`` (one launch pair, one 16-byte read-back) and the
  frame kernels, the frames copied as bytes.

The two forms alternate in ONE process, REPEATS timed repetitions each after WARMUP
untimed ones, each repetition from a device synchronise to a device synchronise.  Writes
every repetition's milliseconds, both medians, the device and the source hash to --out
(default profiles/eval_tail_ab.json).  There is no CPU path: without a GPU the tool fails.

python tools/eval_tail_ab.py [--out FILE] [--repeats 20] [--warmup 3] [--size 800]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "eval_tail_ab.json")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_tail_ab: no GPU found (this is a measurement on the MI355X; there is no CPU path)")

    import bench
    from noisy_src import inference
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.metrics import compute_mse, compute_psnr, compute_ssim, image_metrics
    from noisy_src.model import create_nerf
    from noisy_src.rendering import NeRFRenderer

    dev = "cuda"
    golden = ROOT / "tests" / "golden"
    poses = torch.from_numpy(np.load(sorted(golden.glob("final_poses_*.npz"))[0])["ground_truth_poses"][:1])
    data = synthetic_blender_data(poses, H=a.size, W=a.size, device=dev)
    torch.manual_seed(0)
    mc, mf = create_nerf(ModelConfig(precision="bf16"))
    renderer = NeRFRenderer(mc.to(dev), mf.to(dev), RenderConfig())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = inference.render_image(renderer, data.poses[0], data.H, data.W, data.focal)
    torch.cuda.synchronize()
    first_render_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    out = inference.render_image(renderer, data.poses[0], data.H, data.W, data.focal)
    torch.cuda.synchronize()
    render_ms = 1e3 * (time.perf_counter() - t0)
    pred, depth, target = out["rgb"], out["depth"], data.images[0]

    def quantise(img):
        return (img.cpu().numpy() * 255).clip(0, 255).astype(np.uint8)

    def host():
        m = {"psnr": compute_psnr(pred, target).item(), "ssim": compute_ssim(pred, target).item(),
             "mse": compute_mse(pred, target).item()}
        frames = [quantise(pred), quantise(target), quantise(torch.cat([target, pred], dim=1)),
                  quantise(inference.depth_to_colormap(depth))]
        return m, frames

    def fused():
        m = image_metrics(pred, target)
        H, W, C = pred.shape
        both = torch.empty(H, 2 * W, C, device=pred.device, dtype=torch.uint8)
        inference.frame_u8(target, out=both, x0=0)
        inference.frame_u8(pred, out=both, x0=W)
        cmp_frame = both.cpu().numpy()
        frames = [np.ascontiguousarray(cmp_frame[:, W:]), np.ascontiguousarray(cmp_frame[:, :W]), cmp_frame,
                  inference.depth_frame_u8(depth).cpu().numpy()]
        return m, frames

    legs = {"host": host, "fused": fused}
    (mh, fh), (mf_, ff) = host(), fused()
    same_bytes = all(np.array_equal(x, y) for x, y in zip(fh, ff))
    for _ in range(a.warmup):
        for leg in legs.values():
            leg()
    runs = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():  # alternating: both legs see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            runs[name].append(round(1e3 * (time.perf_counter() - t0), 4))
    med = {name: round(statistics.median(v), 4) for name, v in runs.items()}
    rec = {"tool": "tools/eval_tail_ab.py", "device": torch.cuda.get_device_name(0),
           "source_hash": bench.source_hash(), "image": [a.size, a.size], "repeats": a.repeats, "warmup": a.warmup,
           "render_ms": round(render_ms, 3), "first_render_ms": round(first_render_ms, 3), "median_ms": med,
           "spread_ms": {name: round(max(v) - min(v), 4) for name, v in runs.items()},
           "fused_over_host": round(med["fused"] / med["host"], 4),
           "tail_share_of_render": {name: round(med[name] / render_ms, 4) for name in legs},
           "frames_identical": bool(same_bytes),
           "metrics": {"host": mh, "fused": mf_}, "ms": runs}
    print(json.dumps({k: v for k, v in rec.items() if k != "ms"}), flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
