"""
Image-quality metrics — drop-in for ShawnnnLiu/Robust-NeRF ``noisy_src/metrics.py``.

Evaluation-side, not the training hot path: PSNR / MSE / SSIM run
as device tensor ops on the rendered image where it lies (no host round trip).
LPIPS needs the ``lpips`` package and VGG weights from the network (metrics.py:119-168);
neither exists offline, so ``LPIPSMetric`` reports itself unavailable and returns
None, which ``compute_all_metrics`` skips exactly as the reference does.
``image_metrics`` is the fused form of the three (``nr_image_metrics``, csrc/image.hip):
SSIM and the squared error in fp64 in one launch pair, read back once.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F


def compute_psnr(pred: torch.Tensor, target: torch.Tensor, max_val: float = 1.0) -> torch.Tensor:
    """Reference metrics.py:15-40: 20 log10(max) - 10 log10(mean((pred - target)^2))."""
    mse = torch.mean((pred - target) ** 2)
    if mse == 0:
        return torch.tensor(float("inf"))
    return 20.0 * torch.log10(torch.tensor(max_val)) - 10.0 * torch.log10(mse)


def compute_mse(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Reference metrics.py:43-45."""
    return torch.mean((pred - target) ** 2)


def _gaussian_1d(size: int, sigma: float = 1.5) -> torch.Tensor:
    coords = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _gaussian_window(size: int, sigma: float = 1.5) -> torch.Tensor:
    g = _gaussian_1d(size, sigma)
    return g.outer(g)


def compute_ssim(pred: torch.Tensor, target: torch.Tensor, window_size: int = 11, C1: float = 0.01 ** 2,
                 C2: float = 0.03 ** 2) -> torch.Tensor:
    """Reference metrics.py:48-116: mean SSIM with an 11x11 Gaussian window (sigma 1.5),
    zero padding, per-channel (grouped) convolutions."""
    pred = pred.float()
    target = target.float()
    if pred.dim() == 3:
        pred = pred.permute(2, 0, 1).unsqueeze(0)
        target = target.permute(2, 0, 1).unsqueeze(0)
    elif pred.dim() == 2:
        pred = pred.unsqueeze(0).unsqueeze(0)
        target = target.unsqueeze(0).unsqueeze(0)
    C = pred.shape[1]
    window = _gaussian_window(window_size).to(pred.device)[None, None].expand(C, 1, window_size, window_size)
    pad = window_size // 2

    def blur(x):
        return F.conv2d(x, window, padding=pad, groups=C)

    mu_p, mu_t = blur(pred), blur(target)
    mu_p2, mu_t2, mu_pt = mu_p ** 2, mu_t ** 2, mu_p * mu_t
    s_p = blur(pred ** 2) - mu_p2
    s_t = blur(target ** 2) - mu_t2
    s_pt = blur(pred * target) - mu_pt
    ssim_map = ((2 * mu_pt + C1) * (2 * s_pt + C2)) / ((mu_p2 + mu_t2 + C1) * (s_p + s_t + C2))
    return ssim_map.mean()


class LPIPSMetric:
    """Reference metrics.py:119-168.  The ``lpips`` package and its VGG weights are not
    available offline: ``available`` is False and calls return None."""

    def __init__(self, net: str = "vgg", device: str = "cuda"):
        self.net = net
        self.device = device
        try:  # pragma: no cover - not installed in this image
            import lpips  # noqa: F401
            self.available = False  # weights would need a download; never fetched here
        except ImportError:
            self.available = False

    def __call__(self, pred: torch.Tensor, target: torch.Tensor) -> Optional[torch.Tensor]:
        return None


def compute_all_metrics(pred: torch.Tensor, target: torch.Tensor,
                        lpips_metric: Optional[LPIPSMetric] = None) -> Dict[str, float]:
    """Reference metrics.py:171-205."""
    metrics = {
        "mse": compute_mse(pred, target).item(),
        "psnr": compute_psnr(pred, target).item(),
        "ssim": compute_ssim(pred, target).item(),
    }
    if lpips_metric is not None:
        v = lpips_metric(pred, target)
        if v is not None:
            metrics["lpips"] = v.item()
    return metrics


_WINDOW = 11
IMAGE_METRICS_TILE = (16, 32)  # (rows, columns) of one workgroup's output tile, csrc/image.hip kTileH / kTileW


def image_metric_sums(pred: torch.Tensor, target: torch.Tensor, C1: float = 0.01 ** 2,
                      C2: float = 0.03 ** 2) -> torch.Tensor:
    """Device float64 ``[sum(ssim_map), sum((pred - target)^2)]`` of one (H,W,C) or (H,W)
    image pair from ``nr_image_metrics``: one launch pair, nothing read back.  The fp32
    pixels are promoted and the blur, the map and the sums are all fp64."""
    import ctypes

    from . import _hip
    if pred.shape != target.shape or pred.dim() not in (2, 3):
        raise ValueError(f"image_metrics: need two (H,W,C) or (H,W) images of one shape, got {tuple(pred.shape)} "
                         f"and {tuple(target.shape)}")
    p, t = pred.detach().float().contiguous(), target.detach().float().contiguous()
    pp, tp = _hip.ptr(p), _hip.ptr(t)
    H, W = p.shape[:2]
    C = p.shape[2] if p.dim() == 3 else 1
    nbytes = _hip.call("nr_image_metrics_workspace_bytes", H, W, C)
    if nbytes < 0:
        raise RuntimeError(f"image_metrics: {_hip.last_error()}")
    ws = torch.empty(nbytes, device=p.device, dtype=torch.uint8)
    out = torch.empty(2, device=p.device, dtype=torch.float64)
    g = (ctypes.c_float * _WINDOW)(*_gaussian_1d(_WINDOW).tolist())
    _hip.call("nr_image_metrics", pp, tp, H, W, C, g, float(C1), float(C2), _hip.ptr(out), _hip.ptr(ws),
              _hip.stream_ptr())
    return out


def image_metrics(pred: torch.Tensor, target: torch.Tensor) -> Dict[str, float]:
    """MSE, PSNR and SSIM (reference metrics.py:15-116, max_val 1) of one image pair from
    the fused fp64 kernel, read back in one 16-byte copy: one sync per image, not three.
    No CPU fallback: CPU tensors raise."""
    import math
    n = pred.numel()
    ssim_sum, sq_sum = image_metric_sums(pred, target).tolist()
    mse = sq_sum / n
    return {"mse": mse, "psnr": float("inf") if mse == 0 else -10.0 * math.log10(mse), "ssim": ssim_sum / n}
