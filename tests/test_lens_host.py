"""CPU: the host side of the learned lens (``train_pose_opt --learn_principal
--learn_distortion --lens_init``).

The four new entry points in the header, the ctypes table and the built library;
``CameraIntrinsics`` as it was and with a lens; the new flags; ``pose_eval``'s lens report and
the logger's columns, with and without the entries; and the yardstick of the device tests
(lens_ref.py): ``gradcheck`` in all six numbers, equality with learn_focal_ref.py at a centred
principal point and zero k, the conditions on the kernel tests' inputs, and the signs of
dL/dk1 and dL/dprincipal on the refinement scene that test_lens.py asks the device for."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import learn_focal_ref as RF  # noqa: E402
import lens_ref as R  # noqa: E402
import pose_refine_scene as S  # noqa: E402

from noisy_src import _hip  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "nerf_hip.h"

c_vp, c_i, c_i64, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
# name -> (return type, argument types, the header's parameter list)
NEW_SYMBOLS = {
    "nr_ray_directions_lens": (
        c_i, [c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_vp, c_vp],
        "int H, int W, float fx, float fy, float cx, float cy, float k1, float k2, float* dirs, nr_stream_t stream"),
    "nr_rays_from_pixels_lens_fwd": (
        c_i, [c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_i, c_vp, c_vp, c_vp, c_vp],
        "const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H, int W, const float* lens, "
        "int B, float* rays_o, float* rays_d, int* bad_index, nr_stream_t stream"),
    "nr_rays_from_pixels_lens_bwd": (
        c_i, [c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
        "const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H, int W, const float* lens, "
        "int B, const float* g_rays_o, const float* g_rays_d, float* g_poses, float* g_lens, void* workspace, "
        "nr_stream_t stream"),
    "nr_rays_from_pixels_lens_bwd_workspace_bytes": (c_i64, [c_i], "int n_img"),
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
    fn = _hip.load().nr_rays_from_pixels_lens_bwd_workspace_bytes
    assert fn(300) == 300 * 6 * 4 and fn(1) == 24
    assert _hip.load().nr_abi_version() == 5  # additive: the version stays


# ------------------------------------------------------------ CameraIntrinsics --
@pytest.mark.parametrize("mode", ["shared", "xy"])
def test_camera_intrinsics_built_as_before_is_unchanged(mode):
    from noisy_src.train_pose_opt import CameraIntrinsics
    focal = 555.5555419921875 * 1.05
    cam = CameraIntrinsics(focal, mode)
    assert [k for k, _ in cam.named_parameters()] == ["log_scale"]
    assert sorted(cam.state_dict()) == ["focal_init", "log_scale"]
    assert not cam.has_lens
    assert torch.equal(cam.fxy().detach(), torch.tensor([focal, focal], dtype=torch.float32))
    assert torch.equal(cam.camera(), cam.fxy()) and cam.camera_values() == cam.fxy_values()
    with pytest.raises(ValueError, match="lens"):
        cam.lens()


@pytest.mark.parametrize("principal,distortion", [(True, False), (False, True), (True, True)])
def test_camera_intrinsics_lens_parameters_and_start(principal, distortion):
    """Only what was asked for is registered; at zero the lens is {f, f, W/2, H/2, 0, 0}
    exactly (for an odd W too: W/2 is a binary fraction, and f * 0 adds an exact zero)."""
    from noisy_src.train_pose_opt import CameraIntrinsics
    focal = 555.5555419921875 * 1.05  # a product that is no fp32 number
    cam = CameraIntrinsics(focal, "shared", learn_principal=principal, learn_distortion=distortion, image_size=(7, 5))
    want = ["log_scale"] + (["principal"] if principal else []) + (["radial"] if distortion else [])
    assert [k for k, _ in cam.named_parameters()] == want and cam.has_lens
    for name in want[1:]:
        p = getattr(cam, name)
        assert p.shape == (2,) and torch.count_nonzero(p) == 0
    lens = cam.lens()
    assert lens.shape == (6,) and lens.dtype == torch.float32 and lens.is_contiguous() and lens.requires_grad
    f32 = float(torch.tensor(focal, dtype=torch.float32))
    assert torch.equal(lens.detach(), torch.tensor([f32, f32, 3.5, 2.5, 0.0, 0.0]))
    assert cam.lens_values() == (f32, f32, 3.5, 2.5, 0.0, 0.0) and cam.camera_values() == cam.lens_values()
    assert torch.equal(cam.fxy().detach(), lens.detach()[:2])
    (lens * torch.arange(1.0, 7.0)).sum().backward()
    if principal:  # cx = W/2 + focal_init_x * principal[0]: in units of the focal length
        assert torch.allclose(cam.principal.grad, torch.tensor([3.0, 4.0]) * f32)
    if distortion:
        assert torch.equal(cam.radial.grad, torch.tensor([5.0, 6.0]))


def test_camera_intrinsics_lens_values_follow_the_parameters():
    from noisy_src.train_pose_opt import CameraIntrinsics
    cam = CameraIntrinsics((50.0, 70.0), "xy", learn_principal=True, learn_distortion=True, lens_init=(0.11, -0.03),
                           image_size=(7, 5))
    assert torch.equal(cam.radial.detach(), torch.tensor([0.11, -0.03]))
    with torch.no_grad():
        cam.principal.copy_(torch.tensor([0.01, -0.02]))
        cam.log_scale.copy_(torch.tensor([0.1, -0.2]))
    fxy = torch.tensor([50.0, 70.0]) * torch.exp(torch.tensor([0.1, -0.2]))
    # the principal point moves in units of focal_init, not of the current focal length
    want = torch.cat([fxy, torch.tensor([3.5, 2.5]) + torch.tensor([50.0, 70.0]) * torch.tensor([0.01, -0.02]),
                      torch.tensor([0.11, -0.03])])
    assert torch.equal(cam.lens().detach(), want)


def test_camera_intrinsics_held_focal_and_held_calibration():
    """``learn_focal=False`` and a ``lens_init`` without ``learn_distortion`` are buffers
    (``log_scale_held``, ``radial_held``): no parameter, so no optimizer can move them; an
    optimizer step on everything the module offers leaves them where they were."""
    from noisy_src.train_pose_opt import CameraIntrinsics
    cam = CameraIntrinsics(60.0, "xy", learn_focal=False, learn_principal=True, lens_init=(0.2, 0.01),
                           image_size=(16, 16))
    assert [k for k, _ in cam.named_parameters()] == ["principal"]
    assert sorted(cam.state_dict()) == ["focal_init", "image_size", "log_scale_held", "principal", "radial_held"]
    before = cam.lens().detach().clone()
    assert torch.equal(before, torch.tensor([60.0, 60.0, 8.0, 8.0, 0.2, 0.01]))
    opt = torch.optim.Adam(cam.parameters(), lr=1e-2)
    for _ in range(3):
        opt.zero_grad()
        (cam.lens() * torch.arange(1.0, 7.0)).sum().backward()
        opt.step()
    after = cam.lens().detach()
    assert torch.equal(after[:2], before[:2]) and torch.equal(after[4:], before[4:])  # held: never moves
    assert bool((after[2:4] != before[2:4]).all())  # learned: moved
    # a calibration alone is a lens too, with the focal length still learned
    held = CameraIntrinsics(60.0, lens_init=(0.2, 0.0), image_size=(16, 16))
    assert [k for k, _ in held.named_parameters()] == ["log_scale"] and held.has_lens
    assert held.lens_values() == (60.0, 60.0, 8.0, 8.0, float(torch.tensor(0.2)), 0.0)


def test_camera_intrinsics_bad_arguments():
    from noisy_src.train_pose_opt import CameraIntrinsics
    with pytest.raises(ValueError, match="image_size"):
        CameraIntrinsics(60.0, learn_principal=True)
    with pytest.raises(ValueError, match="image_size"):
        CameraIntrinsics(60.0, learn_distortion=True, image_size=(16, 0))
    with pytest.raises(ValueError, match="lens_init"):
        CameraIntrinsics(60.0, learn_distortion=True, lens_init=(0.1,), image_size=(16, 16))
    with pytest.raises(ValueError, match="lens_init"):
        CameraIntrinsics(60.0, learn_distortion=True, lens_init=(0.1, float("nan")), image_size=(16, 16))
    with pytest.raises(ValueError, match="learn_focal"):
        CameraIntrinsics(60.0, learn_focal=False)
    with pytest.raises(ValueError, match="mode"):
        CameraIntrinsics(60.0, "both", learn_principal=True, image_size=(16, 16))


STATE_FORMS = {
    "old_shared": (dict(mode="shared"), ["focal_init", "log_scale"]),
    "old_xy": (dict(mode="xy"), ["focal_init", "log_scale"]),
    "principal": (dict(mode="shared", learn_principal=True, image_size=(7, 5)),
                  ["focal_init", "image_size", "log_scale", "principal"]),
    "all": (dict(mode="xy", learn_principal=True, learn_distortion=True, lens_init=(0.11, -0.03), image_size=(7, 5)),
            ["focal_init", "image_size", "log_scale", "principal", "radial"]),
    "held_focal": (dict(mode="shared", learn_focal=False, learn_distortion=True, image_size=(7, 5)),
                   ["focal_init", "image_size", "log_scale_held", "radial"]),
    "calibration": (dict(mode="shared", lens_init=(0.2, 0.01), image_size=(7, 5)),
                    ["focal_init", "image_size", "log_scale", "radial_held"]),
}


@pytest.mark.parametrize("form", list(STATE_FORMS))
def test_camera_intrinsics_state_dict_round_trip(form, tmp_path):
    """Which keys are present says which options were on: ``from_state_dict`` rebuilds the same
    module, parameters and values, from a file loaded as inference loads checkpoints."""
    from noisy_src.train_pose_opt import CameraIntrinsics
    kw, keys = STATE_FORMS[form]
    kw = dict(kw)
    cam = CameraIntrinsics(61.25, kw.pop("mode"), **kw)
    with torch.no_grad():
        for k, p in enumerate(cam.parameters()):
            p.add_(0.01 * (k + 1))
    state = cam.state_dict()
    assert sorted(state) == keys
    torch.save({"intrinsics": state}, tmp_path / "c.pt")
    loaded = torch.load(tmp_path / "c.pt", weights_only=True)["intrinsics"]
    rebuilt = CameraIntrinsics.from_state_dict(loaded)
    assert rebuilt.mode == cam.mode and rebuilt.has_lens == cam.has_lens
    assert [k for k, _ in rebuilt.named_parameters()] == [k for k, _ in cam.named_parameters()]
    assert sorted(rebuilt.state_dict()) == keys
    assert torch.equal(rebuilt.camera(), cam.camera()) and rebuilt.camera().numel() == (6 if cam.has_lens else 2)


# ------------------------------------------------------------- flags, consumers --
def test_parser_accepts_the_new_flags():
    from noisy_src.train_pose_opt import build_cli_parser
    ap = build_cli_parser()
    off = ap.parse_args([])
    assert off.learn_principal is False and off.learn_distortion is False and tuple(off.lens_init) == (0.0, 0.0)
    a = ap.parse_args(["--learn_principal", "--learn_distortion", "--lens_init", "0.1", "-0.02"])
    assert a.learn_principal and a.learn_distortion and tuple(a.lens_init) == (0.1, -0.02)
    assert a.learn_focal is None  # the focal length may be held while the lens is learned
    b = ap.parse_args(["--lens_init", "0.1", "0", "--learn_focal", "xy"])
    assert tuple(b.lens_init) == (0.1, 0.0) and b.learn_focal == "xy" and not b.learn_distortion
    with pytest.raises(SystemExit):
        ap.parse_args(["--lens_init", "0.1"])


def test_checkpoint_intrinsics_gives_two_or_six_numbers(tmp_path):
    from noisy_src.inference import checkpoint_intrinsics, intrinsics_fxy
    from noisy_src.train_pose_opt import CameraIntrinsics
    old = {"iteration": 3, "model_coarse": {}, "camera_params": {}}
    assert intrinsics_fxy(old) is None
    plain = CameraIntrinsics(80.0, "xy")
    assert intrinsics_fxy(dict(old, intrinsics=plain.state_dict())) == (80.0, 80.0)
    cam = CameraIntrinsics(80.0, "xy", learn_principal=True, learn_distortion=True, lens_init=(0.25, 0.0),
                           image_size=(16, 12))
    torch.save(dict(old, intrinsics=cam.state_dict()), tmp_path / "new.pt")
    assert checkpoint_intrinsics(tmp_path / "new.pt") == (80.0, 80.0, 8.0, 6.0, 0.25, 0.0)


def test_pose_eval_reports_the_lens(tmp_path):
    from noisy_src import pose_eval as pe
    assert pe.lens_errors({"optimized_poses": None}) == {}
    rec = {"initial_lens": torch.tensor([100.0, 100.0, 8.0, 8.0, 0.25, 0.0]),
           "optimized_lens": torch.tensor([101.0, 99.0, 8.5, 7.75, 0.125, -0.5]),
           "ground_truth_lens": torch.tensor([100.0, 100.0, 8.0, 8.0, 0.0, 0.0])}
    out = pe.lens_errors(rec)
    assert out["optimized_lens"] == [101.0, 99.0, 8.5, 7.75, 0.125, -0.5]
    assert [out[f"initial_{n}_error"] for n in ("cx", "cy", "k1", "k2")] == [0.0, 0.0, 0.25, 0.0]
    assert [out[f"optimized_{n}_error"] for n in ("cx", "cy", "k1", "k2")] == [0.5, -0.25, 0.125, -0.5]
    with pytest.raises(ValueError, match="six"):
        pe.lens_errors(dict(rec, optimized_lens=torch.ones(2)))
    # the command line: a file of before keeps its keys; the lens stands beside the pose errors
    poses = S.ring_poses(4, torch.Generator().manual_seed(0))
    base = {"initial_poses": poses, "optimized_poses": poses, "ground_truth_poses": poses, "pose_errors": {}}
    torch.save(base, tmp_path / "a.pt")
    torch.save(dict(base, **rec), tmp_path / "b.pt")
    pe.main([str(tmp_path / "a.pt"), "--out", str(tmp_path / "a.json")])
    pe.main([str(tmp_path / "b.pt"), "--out", str(tmp_path / "b.json")])
    a, b = json.loads((tmp_path / "a.json").read_text()), json.loads((tmp_path / "b.json").read_text())
    assert "lens" not in a and set(b) == set(a) | {"lens"}
    assert b["lens"]["optimized_k1_error"] == 0.125
    assert {k: v for k, v in b.items() if k != "lens"} == a  # not folded into the pose errors


def test_training_metrics_columns_only_with_a_lens():
    from noisy_src.logger import TrainingMetrics
    from noisy_src.run import LENS_COLUMNS
    plain = TrainingMetrics(iteration=0, loss=1.0, loss_coarse=1.0).to_dict()
    assert not set(LENS_COLUMNS) & set(plain)
    focal = TrainingMetrics(iteration=0, loss=1.0, loss_coarse=1.0, focal_error_pct=2.5).to_dict()
    assert not set(LENS_COLUMNS) & set(focal)
    row = TrainingMetrics(iteration=0, loss=1.0, loss_coarse=1.0, lens_cx=8.5, lens_cy=8.0, lens_k1=0.1, lens_k2=0.0)
    d = row.to_dict()
    assert [d[k] for k in LENS_COLUMNS] == [8.5, 8.0, 0.1, 0.0] and "focal_error_pct" not in d
    assert list(d)[-4:] == list(LENS_COLUMNS)  # behind the columns of before


def test_render_image_rejects_a_malformed_camera():
    from noisy_src.train import render_image
    with pytest.raises(ValueError, match="fxy"):
        render_image(None, torch.eye(4), 4, 4, 5.0, fxy=(1.0, 2.0, 3.0))


# ------------------------------------------------------------------ the yardstick --
def _small_case(B=9, n_img=3):
    g = torch.Generator().manual_seed(3)
    poses = S.ring_poses(n_img, g)
    img = torch.randint(0, n_img, (B,), generator=g)
    pix = torch.stack([torch.randint(0, R.W, (B,), generator=g), torch.randint(0, R.H, (B,), generator=g)], -1).double()
    return img, pix, poses


def test_reference_passes_gradcheck_in_all_six_numbers():
    img, pix, poses = _small_case()
    lens = R.lens64(R.LIVE).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: R.rays_ref(img, pix, poses, x)[1], (lens,), eps=1e-6, atol=1e-7)
    per_ray = lens.detach().expand(img.shape[0], 6).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: R.rays_ref(img, pix, poses, x)[1], (per_ray,), eps=1e-6, atol=1e-7)
    # the per-ray terms add up to the gradient of the shared lens
    g_ro, g_rd = torch.randn(9, 3, dtype=R.F64), torch.randn(9, 3, dtype=R.F64)
    o, d = R.rays_ref(img, pix, poses, lens)
    ((o * g_ro).sum() + (d * g_rd).sum()).backward()
    total, abs_sum, _ = R.lens_grad_ref(img, pix, poses, lens.detach(), g_ro, g_rd)
    assert (total - lens.grad).abs().max() < 1e-13 and bool((abs_sum >= total.abs()).all())
    assert bool((total.abs() > 0).all())
    zero, zabs, _ = R.lens_grad_ref(img, pix, poses, lens.detach(), g_ro, None)
    assert torch.count_nonzero(zero) == 0 and torch.count_nonzero(zabs) == 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_reference_equals_the_focal_restatement_at_a_neutral_lens(dtype):
    """Centred principal point, k = 0: s is exactly 1 and x * 1 == x, so the rays are
    learn_focal_ref.rays_ref's to the bit, in fp32 as in fp64; the direction table too."""
    img, pix, poses = _small_case()
    for lens in (R.NEUTRAL, R.NEUTRAL_XY):
        x = torch.tensor(lens, dtype=torch.float32).to(dtype)
        o, d = R.rays_ref(img, pix.to(dtype), poses.to(dtype), x)
        wo, wd = RF.rays_ref(img, pix.to(dtype), poses.to(dtype), R.H, R.W, x[:2])
        assert torch.equal(o, wo) and torch.equal(d, wd)
        fx, fy = x[:2].tolist()
        assert torch.equal(R.directions_ref(R.H, R.W, x.tolist(), dtype), RF.directions_ref(R.H, R.W, fx, fy, dtype))
    assert R.neutral(R.H, R.W, R.FOCAL) == R.NEUTRAL and R.neutral(R.H, R.W, 7.3, 5.9) == R.NEUTRAL_XY


def test_forward_inputs_carry_the_device_bounds():
    """Conditions on test_lens.py's forward inputs, not on the kernel: at the live lens torch's
    own fp32 is within 1e-6 of fp64 (so the bound asked of the device is one fp32 can meet),
    and swapping cx with cy, or k1 with k2, misses the fp64 rays by more than 1e-3 (so the
    device test can tell them apart)."""
    img, pix, poses, _, _ = R.case(257, 3)
    _, want = R.rays_ref(img, pix.double(), poses.double(), R.lens64(R.LIVE))
    _, d32 = R.rays_ref(img, pix, poses, torch.tensor(R.LIVE, dtype=torch.float32))
    err = (d32.double() - want).abs().max().item()
    print(f"LENS_FWD_INPUTS fp32 restatement vs fp64: {err:.3e}")
    assert err < 1e-6
    for a, b in ((2, 3), (4, 5), (0, 1)):
        _, other = R.rays_ref(img, pix.double(), poses.double(), R.lens64(R.swapped(R.LIVE, a, b)))
        miss = (other - want).abs().max().item()
        print(f"LENS_FWD_INPUTS {R.NAMES[a]} <-> {R.NAMES[b]}: {miss:.3e}")
        assert miss > 1e-3
    # and the table of nr_ray_directions_lens's test
    t = R.directions_ref(R.H, R.W, R.lens64(R.LIVE).tolist())
    for a, b in ((2, 3), (4, 5)):
        assert (R.directions_ref(R.H, R.W, R.lens64(R.swapped(R.LIVE, a, b)).tolist()) - t).abs().max() > 1e-3


@pytest.fixture(scope="module")
def scene():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return S.build(S.SEED)


def test_scene_pulls_a_wrong_lens_back(scene):
    """The end-to-end check of test_lens.py, in fp64, on batch 0 from the true poses: at
    k1 = +K the loss rises with k1 and at -K it falls, ``K`` being the first candidate with
    both signs; and with the principal point half a pixel right (left) of the centre the loss
    rises (falls) with cx."""
    first = None
    for k in R.K_CANDIDATES:
        up, down = R.scene_grad(scene, R.scene_lens(k1=k))[4], R.scene_grad(scene, R.scene_lens(k1=-k))[4]
        print(f"LENS_SCENE K {k}: dL/dk1 {up:.4e} at +K, {down:.4e} at -K")
        if up > 0 and down < 0:
            first = k
            break
    assert first == R.K, (first, R.K)
    right = R.scene_grad(scene, R.scene_lens(principal_px=R.PRINCIPAL_OFFSET_PX))[2]
    left = R.scene_grad(scene, R.scene_lens(principal_px=-R.PRINCIPAL_OFFSET_PX))[2]
    print(f"LENS_SCENE dL/dcx {right:.4e} at +{R.PRINCIPAL_OFFSET_PX} px, {left:.4e} at -{R.PRINCIPAL_OFFSET_PX} px")
    assert right > 0 and left < 0
