"""CPU: the host side of the learned focal length (``train_pose_opt --learn_focal``).

The four new entry points in the header, the ctypes table and the built library;
``CameraIntrinsics``; the two new flags; checkpoints without an ``intrinsics`` entry;
``pose_eval``'s focal report; and the yardstick of the device tests (learn_focal_ref.py): its
gradient with respect to (fx, fy) against ``torch.autograd.gradcheck``, and the sign of
dL/dlog_scale on the refinement scene that test_learn_focal.py asks the device for."""
import ctypes
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import learn_focal_ref as R  # noqa: E402
import pose_refine_scene as S  # noqa: E402

from noisy_src import _hip  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "nerf_hip.h"

c_vp, c_i, c_i64, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
# name -> (return type, argument types, the header's parameter list)
NEW_SYMBOLS = {
    "nr_ray_directions_xy": (
        c_i, [c_i, c_i, c_f, c_f, c_f, c_f, c_vp, c_vp],
        "int H, int W, float fx, float fy, float cx, float cy, float* dirs, nr_stream_t stream"),
    "nr_rays_from_pixels_intr_fwd": (
        c_i, [c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_i, c_vp, c_vp, c_vp, c_vp],
        "const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H, int W, const float* fxy, "
        "int B, float* rays_o, float* rays_d, int* bad_index, nr_stream_t stream"),
    "nr_rays_from_pixels_intr_bwd": (
        c_i, [c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
        "const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H, int W, const float* fxy, "
        "int B, const float* g_rays_o, const float* g_rays_d, float* g_poses, float* g_fxy, void* workspace, "
        "nr_stream_t stream"),
    "nr_rays_from_pixels_intr_bwd_workspace_bytes": (c_i64, [c_i], "int n_img"),
}


def test_new_symbols_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, (res, args, params) in NEW_SYMBOLS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in nerf_hip.h"
        assert " ".join(m.group(1).split()) == params, name
        assert name in _hip._SIGNATURES, f"{name} is not in the ctypes table"
        assert _hip._SIGNATURES[name] == (res, args), name
    lib = _hip.lib_path()
    assert lib.exists(), "library not built (run __graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s(nr_[a-z0-9_]+)", out))
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    # a host function: callable without a device
    fn = _hip.load().nr_rays_from_pixels_intr_bwd_workspace_bytes
    assert fn(300) == 300 * 2 * 4 and fn(1) == 8


# ------------------------------------------------------------ CameraIntrinsics --
@pytest.mark.parametrize("mode,n", [("shared", 1), ("xy", 2)])
def test_camera_intrinsics_shapes_and_start(mode, n):
    from noisy_src.train_pose_opt import CameraIntrinsics
    focal = 555.5555419921875 * 1.05  # a product that is no fp32 number
    cam = CameraIntrinsics(focal, mode)
    assert [k for k, _ in cam.named_parameters()] == ["log_scale"]
    assert cam.log_scale.shape == (n,) and torch.count_nonzero(cam.log_scale) == 0
    f = cam.fxy()
    assert f.shape == (2,) and f.dtype == torch.float32 and f.is_contiguous() and f.requires_grad
    # at zero: focal_init exactly (exp(0) == 1, x * 1 == x), the fp32 rounding of the number a
    # fixed-focal run hands its kernel
    want = torch.tensor([focal, focal], dtype=torch.float32)
    assert torch.equal(f.detach(), want) and torch.equal(cam.focal_init, want)
    assert float(cam.focal_error_pct(focal)) < 1e-5
    f.sum().backward()
    assert cam.log_scale.grad.shape == (n,)
    assert torch.allclose(cam.log_scale.grad, torch.full((n,), focal * (2 // n)))  # shared: both axes add


def test_camera_intrinsics_pair_and_bad_arguments():
    from noisy_src.train_pose_opt import CameraIntrinsics
    cam = CameraIntrinsics((50.0, 70.0), "xy")
    with torch.no_grad():
        cam.log_scale.copy_(torch.tensor([0.1, -0.2]))
    want = torch.tensor([50.0, 70.0]) * torch.exp(torch.tensor([0.1, -0.2]))
    assert torch.equal(cam.fxy().detach(), want)
    assert cam.fxy_values() == tuple(want.tolist())
    with pytest.raises(ValueError, match="mode"):
        CameraIntrinsics(50.0, "both")
    with pytest.raises(ValueError, match="positive"):
        CameraIntrinsics(0.0)
    with pytest.raises(ValueError, match="positive"):
        CameraIntrinsics((1.0, 2.0, 3.0))


@pytest.mark.parametrize("mode", ["shared", "xy"])
def test_camera_intrinsics_state_dict_round_trip(mode, tmp_path):
    from noisy_src.train_pose_opt import CameraIntrinsics
    cam = CameraIntrinsics(61.25, mode)
    with torch.no_grad():
        cam.log_scale.add_(0.03)
    state = cam.state_dict()
    assert sorted(state) == ["focal_init", "log_scale"]
    torch.save({"intrinsics": state}, tmp_path / "c.pt")
    loaded = torch.load(tmp_path / "c.pt", weights_only=True)["intrinsics"]  # as inference loads checkpoints
    other = CameraIntrinsics(1.0, mode)
    other.load_state_dict(loaded)
    assert torch.equal(other.fxy(), cam.fxy())
    rebuilt = CameraIntrinsics.from_state_dict(loaded)
    assert rebuilt.mode == mode and torch.equal(rebuilt.fxy(), cam.fxy())


# ------------------------------------------------------------- flags, consumers --
def test_parser_accepts_the_new_flags():
    from noisy_src.train_pose_opt import build_arg_parser
    ap = build_arg_parser()
    off = ap.parse_args([])
    assert off.learn_focal is None and off.focal_init_scale == 1.0
    a = ap.parse_args(["--learn_focal", "shared", "--focal_init_scale", "1.05"])
    assert a.learn_focal == "shared" and a.focal_init_scale == 1.05
    assert ap.parse_args(["--learn_focal", "xy"]).learn_focal == "xy"
    with pytest.raises(SystemExit):
        ap.parse_args(["--learn_focal", "none"])


def test_checkpoint_without_intrinsics_still_loads(tmp_path):
    """``inference.intrinsics_fxy`` / ``checkpoint_intrinsics``: None for a checkpoint of
    before (the dataset's focal length is used), the learned pair for one with the entry."""
    from noisy_src.inference import checkpoint_intrinsics, intrinsics_fxy
    from noisy_src.train_pose_opt import CameraIntrinsics
    old = {"iteration": 3, "model_coarse": {}, "camera_params": {}}
    assert intrinsics_fxy(old) is None
    torch.save(old, tmp_path / "old.pt")
    assert checkpoint_intrinsics(tmp_path / "old.pt") is None
    cam = CameraIntrinsics(80.0, "xy")
    with torch.no_grad():
        cam.log_scale.copy_(torch.tensor([0.01, -0.02]))
    torch.save(dict(old, intrinsics=cam.state_dict()), tmp_path / "new.pt")
    fx, fy = checkpoint_intrinsics(tmp_path / "new.pt")
    assert (fx, fy) == cam.fxy_values() and fx > 80.0 > fy


def test_pose_eval_reports_the_focal_error(tmp_path):
    from noisy_src import pose_eval as pe
    assert pe.focal_errors({"optimized_poses": None}) == {}
    rec = {"initial_focal": torch.tensor([105.0, 105.0]), "optimized_focal": torch.tensor([101.0, 99.0]),
           "ground_truth_focal": torch.tensor([100.0, 100.0])}
    out = pe.focal_errors(rec)
    assert out["initial_focal_error_pct"] == pytest.approx([5.0, 5.0])
    assert out["optimized_focal_error_pct"] == pytest.approx([1.0, -1.0])
    assert out["optimized_focal_error_pct_mean_abs"] == pytest.approx(1.0)
    # the command line: a file of before keeps its keys, one with the entries gains "focal"
    import json
    poses = S.ring_poses(4, torch.Generator().manual_seed(0))
    base = {"initial_poses": poses, "optimized_poses": poses, "ground_truth_poses": poses, "pose_errors": {}}
    torch.save(base, tmp_path / "a.pt")
    torch.save(dict(base, **rec), tmp_path / "b.pt")
    pe.main([str(tmp_path / "a.pt"), "--out", str(tmp_path / "a.json")])
    pe.main([str(tmp_path / "b.pt"), "--out", str(tmp_path / "b.json")])
    a, b = json.loads((tmp_path / "a.json").read_text()), json.loads((tmp_path / "b.json").read_text())
    assert "focal" not in a and set(b) == set(a) | {"focal"}
    assert b["focal"]["optimized_focal"] == [101.0, 99.0]


def test_training_metrics_column_only_when_learning():
    from noisy_src.logger import TrainingMetrics
    assert "focal_error_pct" not in TrainingMetrics(iteration=0, loss=1.0, loss_coarse=1.0).to_dict()
    assert TrainingMetrics(iteration=0, loss=1.0, loss_coarse=1.0, focal_error_pct=2.5).to_dict()["focal_error_pct"] == 2.5


# ------------------------------------------------------------------ the yardstick --
def _small_case(B=9, n_img=3, H=5, W=7):
    g = torch.Generator().manual_seed(3)
    poses = S.ring_poses(n_img, g)
    img = torch.randint(0, n_img, (B,), generator=g)
    pix = torch.stack([torch.randint(0, W, (B,), generator=g), torch.randint(0, H, (B,), generator=g)], -1).double()
    return img, pix, poses, H, W


def test_reference_passes_gradcheck_in_fxy():
    img, pix, poses, H, W = _small_case()
    fxy = torch.tensor([6.5, 4.25], dtype=R.F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda f: rays_d_only(img, pix, poses, H, W, f), (fxy,), eps=1e-6, atol=1e-7)
    per_ray = fxy.detach().expand(img.shape[0], 2).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda f: rays_d_only(img, pix, poses, H, W, f), (per_ray,), eps=1e-6, atol=1e-7)


def rays_d_only(img, pix, poses, H, W, f):
    return R.rays_ref(img, pix, poses, H, W, f)[1]


def test_reference_matches_the_oracle_at_equal_focal_lengths():
    """fx == fy: the restatement is the oracle's get_rays_from_pixels / get_ray_directions."""
    from oracle import refimpl as ref
    img, pix, poses, H, W = _small_case()
    o, d = R.rays_ref(img, pix, poses, H, W, torch.tensor([6.5, 6.5], dtype=R.F64))
    wo, wd = ref.get_rays_from_pixels(img, pix, poses, H, W, 6.5)
    # the oracle builds its direction table in fp32 (entries below 1 here: 6e-8 each) and casts
    assert (o - wo).abs().max() < 1e-15 and (d - wd).abs().max() < 1e-6
    assert (R.directions_ref(H, W, 6.5, 6.5) - ref.get_ray_directions(H, W, 6.5).double()).abs().max() < 1e-6
    # the per-ray terms add up to the gradient of the shared pair
    g_ro, g_rd = torch.randn(9, 3, dtype=R.F64), torch.randn(9, 3, dtype=R.F64)
    fxy = torch.tensor([6.5, 4.25], dtype=R.F64, requires_grad=True)
    o, d = R.rays_ref(img, pix, poses, H, W, fxy)
    ((o * g_ro).sum() + (d * g_rd).sum()).backward()
    total, abs_sum, _ = R.focal_grad_ref(img, pix, poses, H, W, fxy.detach(), g_ro, g_rd)
    assert (total - fxy.grad).abs().max() < 1e-14 and bool((abs_sum >= total.abs()).all())
    zero, zabs, _ = R.focal_grad_ref(img, pix, poses, H, W, fxy.detach(), g_ro, None)
    assert torch.count_nonzero(zero) == 0 and torch.count_nonzero(zabs) == 0


@pytest.fixture(scope="module")
def scene():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return S.build(S.SEED)


def test_scene_pulls_a_wrong_focal_length_back(scene):
    """The end-to-end check of test_learn_focal.py, in fp64: at 60 * s the loss rises with
    log_scale, at 60 / s it falls, and ``SCALE`` is the first candidate with both signs."""
    first = None
    for s in R.SCALE_CANDIDATES:
        up, down = R.scene_grad(scene, s), R.scene_grad(scene, 1.0 / s)
        print(f"LEARN_FOCAL_SCENE s {s}: dL/dlog_scale {up:.4e} at 60 s, {down:.4e} at 60 / s")
        if up > 0 and down < 0:
            first = s
            break
    assert first == R.SCALE, (first, R.SCALE)
