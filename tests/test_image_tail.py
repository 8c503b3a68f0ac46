"""GPU: the fused image tail of the evaluation loop (csrc/image.hip) -- ``image_metrics``
(fp64 SSIM and squared-error sums) against a float64 CPU oracle and the unchanged fp32
``compute_ssim``, the 8-bit frame kernels against the host quantisation byte for byte,
and ``evaluate_test_set(fused_tail=True)`` against the host tail.

Bounds.  Against the float64 oracle every operation on both sides is fp64 (unit roundoff
1.1e-16) over ~1e2 operations per pixel, and the worst amplification is the 1/C2 of the
variance term (< 1e4): ~1e-10, asserted as 1e-9 absolute on SSIM and 1e-12 relative on
MSE.  Against fp32 ``compute_ssim`` the bound is 1e-4: the fourth decimal the entry point
prints, 4x the worst fp32 formulation error measured on the ill-conditioned kind (2.3e-5)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from noisy_src import _hip, inference, metrics
from noisy_src.metrics import compute_ssim, image_metric_sums, image_metrics

pytestmark = pytest.mark.gpu

TH, TW = metrics.IMAGE_METRICS_TILE
SHAPES = [(5, 7, 3), (11, 11, 3), (16, 16), (TH, TW, 3), (TH + 1, TW + 1, 3), (33, 47, 3), (70, 45, 3)]
KINDS = ["uniform", "smooth", "white_block"]
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _pair(shape, kind, seed=0):
    """(pred, target) fp32 CPU images of one kind."""
    g = torch.Generator().manual_seed(seed + 17 * len(shape) + shape[0])
    H, W = shape[:2]
    if kind == "uniform":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    yy = torch.arange(H, dtype=torch.float32).view(H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, W)
    if kind == "smooth":
        target = 0.5 + 0.4 * torch.sin(yy / 3.0) * torch.cos(xx / 4.0)
        sigma = 0.02
    else:  # white background, a textured block: E[x^2] - mu^2 cancels near 1 against C2
        target = torch.ones(H, W)
        target[H // 4:max(H // 4 + 1, 3 * H // 4), W // 4:max(W // 4 + 1, 3 * W // 4)] = 0.5
        sigma = 0.01
    if len(shape) == 3:
        target = target.unsqueeze(-1).repeat(1, 1, shape[2])
    if kind == "white_block":
        block = target < 1.0
        target = torch.where(block, torch.rand(shape, generator=g), target)
    pred = (target + sigma * torch.randn(shape, generator=g)).clamp(0, 1)
    return pred, target


def _oracle(pred, target):
    """float64 on the CPU: the reference formula with the window built from the same fp32
    1-D weights -> (mean SSIM, MSE)."""
    p, t = pred.double(), target.double()
    if p.dim() == 2:
        p, t = p.unsqueeze(-1), t.unsqueeze(-1)
    p, t = p.permute(2, 0, 1).unsqueeze(0), t.permute(2, 0, 1).unsqueeze(0)
    C = p.shape[1]
    g = metrics._gaussian_1d(11).double()
    window = g.outer(g)[None, None].expand(C, 1, 11, 11)

    def blur(x):
        return F.conv2d(x, window, padding=5, groups=C)

    mu_p, mu_t = blur(p), blur(t)
    mu_p2, mu_t2, mu_pt = mu_p ** 2, mu_t ** 2, mu_p * mu_t
    s_p, s_t, s_pt = blur(p * p) - mu_p2, blur(t * t) - mu_t2, blur(p * t) - mu_pt
    ssim_map = ((2 * mu_pt + C1) * (2 * s_pt + C2)) / ((mu_p2 + mu_t2 + C1) * (s_p + s_t + C2))
    return ssim_map.mean().item(), ((p - t) ** 2).mean().item()


@pytest.fixture(scope="module")
def cases():
    """Every (shape, kind): the CPU pair, its float64 oracle and the device pair, built once."""
    out = {}
    for shape in SHAPES:
        for kind in KINDS:
            pred, target = _pair(shape, kind)
            out[shape, kind] = (pred.cuda(), target.cuda(), _oracle(pred, target))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_metrics_matches_float64_oracle_and_fp32_ssim(cases, shape, kind):
    pred, target, (want_ssim, want_mse) = cases[shape, kind]
    got = image_metrics(pred, target)
    assert set(got) == {"mse", "psnr", "ssim"}
    fp32 = compute_ssim(pred, target).item()
    print(f"{shape} {kind}: ssim {got['ssim']!r} oracle {want_ssim!r} |d| {abs(got['ssim'] - want_ssim):.3e}; "
          f"mse rel {abs(got['mse'] - want_mse) / want_mse:.3e}; fp32 compute_ssim |d| {abs(got['ssim'] - fp32):.3e}")
    assert abs(got["ssim"] - want_ssim) <= 1e-9
    assert abs(got["mse"] - want_mse) <= 1e-12 * want_mse
    assert got["psnr"] == pytest.approx(-10.0 * np.log10(want_mse), abs=1e-9)
    assert abs(got["ssim"] - fp32) <= 1e-4


@pytest.mark.parametrize("shape", [(5, 7, 3), (TH + 1, TW + 1, 3), (70, 45, 3)], ids=lambda s: "x".join(map(str, s)))
def test_image_metrics_is_deterministic(cases, shape):
    pred, target, _ = cases[shape, "white_block"]
    a, b = image_metric_sums(pred, target), image_metric_sums(pred, target)
    assert a.dtype == torch.float64 and a.shape == (2,)
    assert torch.equal(a, b)


def test_image_metrics_non_contiguous_input(cases):
    pred, target, _ = cases[(33, 47, 3), "smooth"]
    wide = torch.rand(33, 60, 3, device="cuda")
    wide[:, 5:52] = pred
    view = wide[:, 5:52]
    assert not view.is_contiguous()
    assert torch.equal(image_metric_sums(view, target), image_metric_sums(pred, target))


def test_image_metrics_identical_images():
    img = torch.rand(11, 11, 3, device="cuda")
    got = image_metrics(img, img.clone())
    assert got["mse"] == 0.0 and got["psnr"] == float("inf") and got["ssim"] == pytest.approx(1.0, abs=1e-12)


def test_image_metrics_refusals():
    for shape, word in (((4, 4, 2), "C=2"), ((0, 5, 3), "H=0"), ((5, 0, 3), "W=0")):
        with pytest.raises(RuntimeError, match=r"H >= 1, W >= 1, C in \{1, 3\}.*" + word):
            image_metrics(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    # the entry point itself refuses, whatever the workspace function was told
    p = torch.zeros(4, 4, 2, device="cuda")
    out = torch.zeros(2, device="cuda", dtype=torch.float64)
    ws = torch.zeros(64, device="cuda", dtype=torch.uint8)
    import ctypes
    g = (ctypes.c_float * 11)(*metrics._gaussian_1d(11).tolist())
    rc = _hip.load().nr_image_metrics(p.data_ptr(), p.data_ptr(), 4, 4, 2, g, C1, C2, out.data_ptr(), ws.data_ptr(),
                                      _hip.stream_ptr())
    assert rc == -22 and "C must be 1 or 3" in _hip.last_error()


def _quantise(img: torch.Tensor) -> np.ndarray:
    """save_image's host arithmetic."""
    return (img.cpu().numpy() * 255).clip(0, 255).astype(np.uint8)


def test_frame_u8_matches_host_quantisation():
    g = torch.Generator().manual_seed(1)
    exact = torch.cat([torch.arange(256, dtype=torch.float32) / 255, torch.tensor([0.0, 1.0])]).view(2, 43, 3)
    # (420,420,3) is more elements than one pass of the capped grid covers
    for img in (torch.rand(37, 53, 3, generator=g) * 1.4 - 0.2, exact, torch.rand(13, 9, 1, generator=g),
                torch.rand(420, 420, 3, generator=g) * 1.4 - 0.2):
        got = inference.frame_u8(img.cuda())
        assert got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), _quantise(img))


def test_frame_u8_writes_zero_for_non_finite_input():
    img = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.5, 3e38, -3e38]).view(1, 2, 3).cuda()
    assert inference.frame_u8(img).cpu().flatten().tolist() == [0, 0, 0, 127, 255, 0]


def test_comparison_frame_from_two_strided_calls():
    g = torch.Generator().manual_seed(2)
    target, pred = torch.rand(19, 23, 3, generator=g), torch.rand(19, 23, 3, generator=g) * 1.4 - 0.2
    both = torch.full((19, 46, 3), 7, device="cuda", dtype=torch.uint8)
    inference.frame_u8(target.cuda(), out=both, x0=0)
    inference.frame_u8(pred.cuda(), out=both, x0=23)
    assert np.array_equal(both.cpu().numpy(), _quantise(torch.cat([target, pred], dim=1)))
    with pytest.raises(ValueError):
        inference.frame_u8(pred.cuda(), out=both, x0=24)


@pytest.mark.parametrize("kind", ["random", "ramp", "constant", "many_blocks"])
def test_depth_frame_u8_matches_host_colormap(kind):
    g = torch.Generator().manual_seed(3)
    depth = {"random": lambda: 2 + 4 * torch.rand(33, 47, generator=g),
             "ramp": lambda: torch.linspace(2, 6, 33 * 47).view(33, 47),
             "constant": lambda: torch.full((16, 16), 3.0),
             # more pixels than the 256 x 256 threads of the min/max pass cover at once
             "many_blocks": lambda: 2 + 4 * torch.rand(300, 250, generator=g)}[kind]()
    got = inference.depth_frame_u8(depth.cuda()).cpu().numpy()
    assert got.shape == depth.shape + (3,)
    assert np.array_equal(got, _quantise(inference.depth_to_colormap(depth)))
    if kind == "constant":  # max == min: n = 0 everywhere, blue
        assert (got == np.array([0, 0, 255], dtype=np.uint8)).all()


def test_evaluate_test_set_fused_tail_matches_host_tail(tmp_path):
    from pathlib import Path

    from PIL import Image

    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.model import create_nerf
    from noisy_src.noise import NoiseConfig
    from noisy_src.rendering import NeRFRenderer
    golden = Path(__file__).resolve().parent / "golden"
    poses = torch.from_numpy(np.load(sorted(golden.glob("final_poses_*.npz"))[0])["ground_truth_poses"][:3])
    data = synthetic_blender_data(poses, H=16, W=16, device="cuda")
    torch.manual_seed(0)
    mc, mf = create_nerf(ModelConfig(precision="bf16"))
    renderer = NeRFRenderer(mc.cuda(), mf.cuda(), RenderConfig())
    for name, fused in (("host", False), ("fused", True)):
        inference.evaluate_test_set(renderer, data, tmp_path / name, NoiseConfig(), device="cuda",
                                    log=lambda *_: None, fused_tail=fused)
    host = json.loads((tmp_path / "host" / "per_image_metrics.json").read_text())
    fused = json.loads((tmp_path / "fused" / "per_image_metrics.json").read_text())
    assert len(host) == len(fused) == 3
    for a, b in zip(host, fused):
        assert set(a) == set(b) and a["image"] == b["image"]
        assert abs(a["psnr"] - b["psnr"]) <= 1e-4
        assert abs(a["ssim"] - b["ssim"]) <= 1e-4
    for f in ("test_metrics.json", "experiment_config.json"):
        assert set(json.loads((tmp_path / "host" / f).read_text())) == set(
            json.loads((tmp_path / "fused" / f).read_text())), f
    pngs = sorted(p.name for p in (tmp_path / "host").glob("*.png"))
    assert len(pngs) == 12 and pngs == sorted(p.name for p in (tmp_path / "fused").glob("*.png"))
    for n in pngs:
        a, b = np.array(Image.open(tmp_path / "host" / n)), np.array(Image.open(tmp_path / "fused" / n))
        assert a.shape == b.shape and np.array_equal(a, b), n
