"""GPU: the learned lens (principal point, radial distortion), from the kernels to the trainers.

``nr_rays_from_pixels_lens_fwd/bwd`` (six numbers {fx, fy, cx, cy, k1, k2} read from device
memory) against the fixed-focal and the ``_intr_`` kernels bit for bit at a neutral lens and
against the fp64 restatement of lens_ref.py at a live one; ``ops.ray_directions_lens``; the
sign and value of dL/dk1 and dL/dprincipal through the renderer on the refinement scene;
``PoseTrainer`` and ``GraphedPoseTrainer`` with a lens; the command-line chain; and the
data-parallel step with the lens gradient in the pose buffer.

Shapes: H = 5, W = 7 (not square), poses from the golden fixture, random cotangents, a
sentinel row behind every output; the workspace and g_lens start as NaN, so a partial or a
result that is not written shows."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lens_ref as R  # noqa: E402
import pose_refine_scene as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
H, W = R.H, R.W
FOCAL = R.FOCAL
FXY = R.NEUTRAL_XY[:2]
NAN = float("nan")


def _rows(t, B):
    """``t`` on the device as the first B rows of a zeroed buffer one row longer, so that a
    zero-size batch still has an address."""
    buf = torch.zeros((B + 1, *t.shape[1:]), dtype=t.dtype, device=DEV)
    buf[:B] = t.to(DEV)
    return buf


def _entry(camera):
    """(entry infix, the kernel's camera argument): the fixed-focal kernel for a number, the
    intrinsics kernel for a pair, the lens kernel for six numbers."""
    from noisy_src._hip import ptr
    if isinstance(camera, float):
        return "", camera, None
    t = torch.tensor(camera, device=DEV, dtype=torch.float32)
    return {2: "_intr", 6: "_lens"}[len(camera)], ptr(t), t


def _fwd(img, pix, poses, camera):
    """(rays_o, rays_d), the sentinel rows behind them checked."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    B = img.shape[0]
    i, p, P = _rows(img, B), _rows(pix, B), poses.to(DEV)
    ro, rd = torch.full((B + 1, 3), -7.0, device=DEV), torch.full((B + 1, 3), -7.0, device=DEV)
    infix, arg, keep = _entry(camera)
    call(f"nr_rays_from_pixels{infix}_fwd", ptr(i), ptr(p), ptr(P), P.shape[0], H, W, arg, B, ptr(ro), ptr(rd), None,
         _hip.stream_ptr())
    assert torch.equal(ro[B:], torch.full((1, 3), -7.0, device=DEV)) and torch.equal(rd[B:], ro[B:])
    return ro[:B], rd[:B]


def _bwd(img, pix, poses, camera, g_ro, g_rd):
    """g_poses of the fixed-focal kernel (a number), or (g_poses, g_camera) of the intrinsics
    kernel (a pair) or the lens kernel (six), whose workspace and g_camera start as NaN."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    B, n_img = img.shape[0], poses.shape[0]
    i, p, P, go = _rows(img, B), _rows(pix, B), poses.to(DEV), _rows(g_ro, B)
    gd = _rows(g_rd, B) if g_rd is not None else None
    g_poses = torch.zeros(n_img + 1, 4, 4, device=DEV)
    infix, arg, keep = _entry(camera)
    if infix == "":
        call("nr_rays_from_pixels_bwd", ptr(i), ptr(p), ptr(P), n_img, H, W, arg, B, ptr(go), ptr(gd), ptr(g_poses),
             _hip.stream_ptr())
        assert torch.count_nonzero(g_poses[n_img]) == 0
        return g_poses[:n_img]
    n = len(camera)
    n_ws = int(getattr(_hip.load(), f"nr_rays_from_pixels{infix}_bwd_workspace_bytes")(n_img)) // 4
    assert n_ws == n * n_img
    ws = torch.full((n_ws + n,), NAN, device=DEV)
    g_cam = torch.full((n + 1,), NAN, device=DEV)
    call(f"nr_rays_from_pixels{infix}_bwd", ptr(i), ptr(p), ptr(P), n_img, H, W, arg, B, ptr(go), ptr(gd), ptr(g_poses),
         ptr(g_cam), ptr(ws), _hip.stream_ptr())
    # nothing behind the buffers was written
    assert torch.isnan(ws[n_ws:]).all() and torch.isnan(g_cam[n]) and torch.count_nonzero(g_poses[n_img]) == 0
    if B > 0:
        assert torch.isfinite(ws[:n_ws]).all()  # every image's partial was written, an empty image's too
    return g_poses[:n_img], g_cam[:n]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ----------------------------------------------------------------------- forward --
@pytest.mark.parametrize("n_img", [1, 3, 300])
@pytest.mark.parametrize("B", [0, 1, 257, 600])
def test_forward_at_a_neutral_lens_equals_the_other_two_kernels(B, n_img):
    from noisy_src import ops
    img, pix, poses, _, _ = R.case(B, n_img)
    o1, d1 = _fwd(img, pix, poses, FOCAL)
    o2, d2 = _fwd(img, pix, poses, R.NEUTRAL)
    assert o2.shape == (B, 3) and torch.equal(o1, o2) and torch.equal(d1, d2)
    o3, d3 = _fwd(img, pix, poses, FXY)
    o4, d4 = _fwd(img, pix, poses, R.NEUTRAL_XY)
    assert torch.equal(o3, o4) and torch.equal(d3, d4)
    if B:
        assert torch.isfinite(d2).all() and not torch.equal(d3, d1)
        # and through the public operator: a (6,) tensor dispatches to the lens pair
        args = (img.to(DEV), pix.to(DEV), poses.to(DEV), H, W)
        o5, d5 = ops.rays_from_pixels(*args, torch.tensor(R.NEUTRAL, device=DEV))
        o6, d6 = ops.rays_from_pixels(*args, torch.tensor(R.NEUTRAL_XY, device=DEV))
        assert torch.equal(o5, o1) and torch.equal(d5, d1) and torch.equal(o6, o3) and torch.equal(d6, d3)


def test_forward_live_lens_vs_fp64():
    """Max abs error below 1e-6, test_parity_ops.py's bound for this operator; cx and cy, k1
    and k2 are not interchangeable (test_lens_host.py checks on the CPU that these inputs tell
    them apart by more than 1e-3)."""
    from noisy_src import ops
    img, pix, poses, _, _ = R.case(257, 3)
    o, d = _fwd(img, pix, poses, R.LIVE)
    wo, wd = R.rays_ref(img, pix.double(), poses.double(), R.lens64(R.LIVE))
    err = (d.double().cpu() - wd).abs().max().item()
    print(f"LENS_FWD live lens vs fp64: rays_d {err:.3e}")
    assert (o.double().cpu() - wo).abs().max() < 1e-6
    assert err < 1e-6, err
    for a, b in ((2, 3), (4, 5)):
        _, other = _fwd(img, pix, poses, R.swapped(R.LIVE, a, b))
        assert (other.double().cpu() - wd).abs().max() > 1e-3, (a, b)
    o2, d2 = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), poses.to(DEV), H, W, torch.tensor(R.LIVE, device=DEV))
    assert torch.equal(o2, o) and torch.equal(d2, d)


def test_ops_rejects_a_malformed_focal_tensor():
    from noisy_src import ops
    img, pix, poses, _, _ = R.case(4, 3)
    args = (img.to(DEV), pix.to(DEV), poses.to(DEV), H, W)
    for bad in (torch.ones(4, device=DEV), torch.ones(5, device=DEV), torch.ones(6, device=DEV, dtype=torch.float64),
                torch.ones(12, device=DEV)[::2], torch.ones(1, 6, device=DEV)):
        with pytest.raises(ValueError, match="focal"):
            ops.rays_from_pixels(*args, bad)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.rays_from_pixels(*args, torch.ones(6))


# ---------------------------------------------------------------------- backward --
BWD_CASES = {  # test_learn_focal.py's
    "one_image_600": dict(B=600, n_img=3, images=[1]),       # the stride loop runs three times; images 0, 2 empty
    "three_images_257": dict(B=257, n_img=3, images=[0, 2]),  # image 1 without a ray
    "300_images": dict(B=600, n_img=300),                      # the final reduction strides over its 256 threads
}


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_backward_vs_the_other_kernels_and_fp64(name):
    """g_poses: the fixed-focal kernel's bits at the neutral lens (and the ``_intr_`` kernel's
    at fx != fy, with its two focal sums); at the live lens within 1e-5 (relative norm, rotation
    block and translation column: test_pose_rotation.py's bound for this reduction) of fp64
    autograd.  g_lens: |g - g64| <= 1e-4 * sum_b |c_b| per component, with sum_b |c_b| the fp64
    sum of the absolute per-ray terms (fp32 unit roundoff 6e-8 x (about 60 operations per term +
    at most 600 additions) ~ 4e-5, margin ~ 2.5)."""
    img, pix, poses, g_ro, g_rd = R.case(**BWD_CASES[name])
    want = _bwd(img, pix, poses, FOCAL, g_ro, g_rd)
    got, _ = _bwd(img, pix, poses, R.NEUTRAL, g_ro, g_rd)
    assert want.abs().max() > 0 and torch.equal(got, want)
    want_xy, want_fxy = _bwd(img, pix, poses, FXY, g_ro, g_rd)
    got_xy, got_lens = _bwd(img, pix, poses, R.NEUTRAL_XY, g_ro, g_rd)
    assert torch.equal(got_xy, want_xy) and torch.equal(got_lens[:2], want_fxy)
    for lens in (R.NEUTRAL, R.LIVE):
        g_poses, g_lens = _bwd(img, pix, poses, lens, g_ro, g_rd)
        g64, abs64, p64 = R.lens_grad_ref(img, pix, poses, R.lens64(lens), g_ro, g_rd)
        err = (g_lens.double().cpu() - g64).abs()
        print(f"LENS_BWD {name} lens {lens}: g_lens {g_lens.tolist()} fp64 {g64.tolist()} |err| {err.tolist()} "
              f"bound {(1e-4 * abs64).tolist()}")
        assert bool((abs64 > 0).all()) and bool((g64.abs() > 0).all())
        assert bool((err <= 1e-4 * abs64).all()), (err, 1e-4 * abs64)
        assert _rel(g_poses[:, :3, :3], p64[:, :3, :3]) < 1e-5 and _rel(g_poses[:, :3, 3], p64[:, :3, 3]) < 1e-5
        assert torch.count_nonzero(g_poses[:, 3, :]) == 0
    used = set(img.tolist())
    empty = [k for k in range(poses.shape[0]) if k not in used]
    assert torch.count_nonzero(g_poses[empty]) == 0


def test_backward_without_ray_direction_gradient_gives_exact_zeros():
    img, pix, poses, g_ro, _ = R.case(257, 3)
    g_poses, g_lens = _bwd(img, pix, poses, R.LIVE, g_ro, None)
    assert torch.equal(g_lens, torch.zeros(6, device=DEV))
    assert torch.equal(g_poses, _bwd(img, pix, poses, FOCAL, g_ro, None))
    assert torch.count_nonzero(g_poses[:, :3, :3]) == 0 and g_poses[:, :3, 3].abs().max() > 0


@pytest.mark.parametrize("n_img", [3, 300])
def test_backward_of_an_empty_batch(n_img):
    img, pix, poses, g_ro, g_rd = R.case(0, n_img)
    g_poses, g_lens = _bwd(img, pix, poses, R.LIVE, g_ro, g_rd)
    assert torch.equal(g_lens, torch.zeros(6, device=DEV)) and torch.count_nonzero(g_poses) == 0


def test_backward_is_deterministic():
    img, pix, poses, g_ro, g_rd = R.case(600, 300, seed=5)
    a, b = _bwd(img, pix, poses, R.LIVE, g_ro, g_rd), _bwd(img, pix, poses, R.LIVE, g_ro, g_rd)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a[1].abs().min() > 0


def test_out_of_range_image_index():
    """Unvalidated: NaN rays for those rows, the others untouched; the validating mode raises
    (the flag is set); g_lens and g_poses are finite and equal the batch with those rays given
    zero cotangents in a valid image, to the bit (exact zeros in the same positions of the same
    sums): nothing contributed."""
    from noisy_src import ops
    img, pix, poses, g_ro, g_rd = R.case(257, 3, seed=9)
    bad = img.clone()
    bad_rows = torch.tensor([0, 100, 256])
    bad[bad_rows] = torch.tensor([3, -1, 1 << 40])
    o, d = _fwd(bad, pix, poses, R.LIVE)
    keep = torch.ones(257, dtype=torch.bool)
    keep[bad_rows] = False
    assert torch.isnan(o[bad_rows]).all() and torch.isnan(d[bad_rows]).all()
    o_ok, d_ok = _fwd(img, pix, poses, R.LIVE)
    assert torch.equal(o[keep], o_ok[keep]) and torch.equal(d[keep], d_ok[keep])
    lens = torch.tensor(R.LIVE, device=DEV)
    with pytest.raises(IndexError):
        ops.rays_from_pixels(bad.to(DEV), pix.to(DEV), poses.to(DEV), H, W, lens, validate=True)
    ops.rays_from_pixels(img.to(DEV), pix.to(DEV), poses.to(DEV), H, W, lens, validate=True)
    g_poses, g_lens = _bwd(bad, pix, poses, R.LIVE, g_ro, g_rd)
    assert torch.isfinite(g_lens).all() and torch.isfinite(g_poses).all()
    z_ro, z_rd = g_ro.clone(), g_rd.clone()
    z_ro[bad_rows] = 0
    z_rd[bad_rows] = 0
    w_poses, w_lens = _bwd(img, pix, poses, R.LIVE, z_ro, z_rd)
    assert torch.equal(g_lens, w_lens) and torch.equal(g_poses, w_poses)
    # and against fp64 with the rays removed
    g64, abs64, _ = R.lens_grad_ref(img[keep], pix[keep], poses, R.lens64(R.LIVE), g_ro[keep], g_rd[keep])
    assert bool(((g_lens.double().cpu() - g64).abs() <= 1e-4 * abs64).all())


def test_autograd_function_returns_both_gradients():
    """``ops.rays_from_pixels`` with a (6,) tensor: gradients for the poses and the lens, the
    kernels' values; a detached lens gets none."""
    from noisy_src import ops
    img, pix, poses, g_ro, g_rd = R.case(257, 3)
    P = poses.to(DEV).requires_grad_(True)
    lens = torch.tensor(R.LIVE, device=DEV, requires_grad=True)
    o, d = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), P, H, W, lens)
    ((o * g_ro.to(DEV)).sum() + (d * g_rd.to(DEV)).sum()).backward()
    w_poses, w_lens = _bwd(img, pix, poses, R.LIVE, g_ro, g_rd)
    assert lens.grad.shape == (6,) and torch.equal(P.grad, w_poses) and torch.equal(lens.grad, w_lens)
    P2 = poses.to(DEV).requires_grad_(True)
    o, d = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), P2, H, W, lens.detach())
    ((o * g_ro.to(DEV)).sum() + (d * g_rd.to(DEV)).sum()).backward()
    assert torch.equal(P2.grad, w_poses)


# ----------------------------------------------------------- ray_directions_lens --
def test_ray_directions_lens():
    from noisy_src import ops
    same = ops.ray_directions_lens(H, W, *R.NEUTRAL_XY, DEV)
    assert same.shape == (H, W, 3) and torch.equal(same, ops.ray_directions_xy(H, W, *R.NEUTRAL_XY[:4], DEV))
    assert torch.equal(ops.ray_directions_lens(H, W, *R.NEUTRAL, DEV), ops.ray_directions(H, W, FOCAL, W / 2.0, H / 2.0, DEV))
    off = (7.3, 5.9, 3.2, 2.9, 0.0, 0.0)  # k = 0 off centre: still _xy's bits
    assert torch.equal(ops.ray_directions_lens(H, W, *off, DEV), ops.ray_directions_xy(H, W, *off[:4], DEV))
    got = ops.ray_directions_lens(H, W, *R.LIVE, DEV)
    want = R.directions_ref(H, W, R.lens64(R.LIVE).tolist())
    assert (got.double().cpu() - want).abs().max() < 1e-6
    for a, b in ((2, 3), (4, 5)):
        assert (ops.ray_directions_lens(H, W, *R.swapped(R.LIVE, a, b), DEV).double().cpu() - want).abs().max() > 1e-3
    # the table, turned into rays by nr_get_rays, gives the pixel kernel's rays: the same model
    # and the same rounding on the evaluation path as on the training path
    from noisy_src.rays import get_rays
    img = torch.zeros(H * W, dtype=torch.int64)
    pix = torch.stack(torch.meshgrid(torch.arange(W), torch.arange(H), indexing="xy"), -1).reshape(-1, 2).float()
    pose = R.fixture_poses(1)
    _, d = _fwd(img, pix, pose, R.LIVE)
    _, t = get_rays(got, pose[0].to(DEV).contiguous())
    assert torch.equal(d, t.reshape(-1, 3))
    # a larger table than one block, odd sizes
    big_lens = (7.3, 5.9, 9.1, 16.9, 0.011, -0.0003)
    big = ops.ray_directions_lens(33, 19, *big_lens, DEV)
    want = R.directions_ref(33, 19, R.lens64(big_lens).tolist())
    assert (big.double().cpu() - want).abs().max() < 1e-6 * max(1.0, want.abs().max().item())


# ------------------------------------------------------- end to end on the scene --
@pytest.fixture(scope="module")
def scene():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return S.build(S.SEED)


def _device_nets(scene, precision="fp32"):
    from noisy_src.model import NeRF
    nets = []
    for o in (scene.coarse, scene.fine):
        net = NeRF(S.model_config(precision))
        net.load_state_dict({k: v.float() for k, v in o.state_dict().items()})
        nets.append(net.to(DEV))
    return nets


def _device_scene_grad(scene, nets, k1, principal_px):
    """(the lens the device read (6,) on the CPU, dL/dradial[0], dL/dprincipal[0]) on batch 0
    from the true poses, through ``CameraIntrinsics.lens()`` and the device renderer."""
    from noisy_src import ops
    from noisy_src.rendering import render_rays
    from noisy_src.train_pose_opt import CameraIntrinsics
    img, pix, target, _, u = scene.batches[0]
    cam = CameraIntrinsics(S.FOCAL, "shared", learn_principal=True, learn_distortion=True, lens_init=(k1, 0.0),
                           image_size=(S.W, S.H)).to(DEV)
    with torch.no_grad():
        cam.principal[0] = principal_px / S.FOCAL
    lens = cam.lens()
    ro, rd = ops.rays_from_pixels(img.to(DEV), pix.float().to(DEV), scene.gt_poses.float().to(DEV), S.H, S.W, lens)
    out = render_rays(nets[0], nets[1], ro, rd, scene.rc, is_train=True, u=u.float().to(DEV),
                      target_rgb=target.float().to(DEV))
    (out["loss_coarse"] + out["loss_fine"]).backward()
    return lens.detach().cpu(), float(cam.radial.grad[0]), float(cam.principal.grad[0])


def test_scene_gradient_pulls_the_lens_back(scene):
    """dL/dk1 through the device renderer at k1 = +K and -K, and dL/dprincipal[0] with the
    principal point 0.5 px right and left of the centre: the signs the fp64 renderer gives
    (test_lens_host.py), and the fp64 values at the lens the device read, as close as torch's
    own fp32 path: relative error below 2 x torch32 + 1e-3 (test_learn_focal.py's bound)."""
    nets = _device_nets(scene)
    cases = [("k1", R.K, 0.0, 1.0), ("k1", -R.K, 0.0, -1.0),
             ("principal", 0.0, R.PRINCIPAL_OFFSET_PX, 1.0), ("principal", 0.0, -R.PRINCIPAL_OFFSET_PX, -1.0)]
    for what, k1, px, sign in cases:
        lens, g_k1, g_pr = _device_scene_grad(scene, nets, k1, px)
        assert lens[4] == torch.tensor(k1, dtype=torch.float32) and abs(float(lens[2]) - (S.W / 2.0 + px)) < 1e-5
        g64, g32 = R.scene_grad(scene, lens), R.scene_grad(scene, lens, torch.float32)
        # dL/dprincipal[0] = focal_init * dL/dcx
        got, w64, w32 = (g_k1, g64[4], g32[4]) if what == "k1" else (g_pr, S.FOCAL * g64[2], S.FOCAL * g32[2])
        ours, torch32 = abs(got - w64) / abs(w64), abs(w32 - w64) / abs(w64)
        print(f"LENS_SCENE_DEVICE {what} k1 {k1} offset {px} px: device {got:.6e} fp64 {w64:.6e} torch32 {w32:.6e} "
              f"rel {ours:.3e} (torch32 {torch32:.3e})")
        assert got * sign > 0 and w64 * sign > 0
        assert ours < 2 * torch32 + 1e-3, (ours, torch32)


# -------------------------------------------------------------------- PoseTrainer --
LOSS_KEYS = ("loss", "loss_coarse", "loss_fine")
B_TRAIN = 64


def _pose_trainer(lens, precision="bf16", seed=17, **cam_kw):
    """3 views of 16 x 16, 16 coarse + 32 fine samples; ``lens``: None (no intrinsics), or the
    keyword options of ``CameraIntrinsics`` at the dataset's focal length."""
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraIntrinsics, CameraPoseParameters
    z = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"])[:3], H=16, W=16, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=B_TRAIN)
    torch.manual_seed(seed)
    mc, mf = create_nerf(ModelConfig(precision=precision))
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(DEV), fixed_small_angle=True, **cam_kw)
    intr = CameraIntrinsics(data.focal, "shared", image_size=(16, 16), **lens).to(DEV) if lens is not None else None
    rc = RenderConfig(num_samples=16, num_samples_fine=32)
    return PoseTrainer(mc.to(DEV), mf.to(DEV), cam, sampler, rc, intrinsics=intr), rc


def _batches(trainer, rc, n):
    out = []
    for k in range(n):
        batch = trainer.pixel_sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(300 + k))
        g = torch.Generator().manual_seed(400 + k)
        out.append((batch, torch.rand(B_TRAIN, rc.num_samples, generator=g).to(DEV),
                    torch.rand(B_TRAIN, rc.num_samples_fine, generator=g).to(DEV)))
    return out


def _assert_same_training_state(a, b):
    for na, nb in ((a.model_coarse, b.model_coarse), (a.model_fine, b.model_fine)):
        assert torch.equal(na.flat_params(), nb.flat_params())
    for pa, pb in zip(a.camera_params.parameters(), b.camera_params.parameters()):
        assert torch.equal(pa.detach(), pb.detach())


BOTH = dict(learn_principal=True, learn_distortion=True)


def test_pose_trainer_with_a_neutral_lens_equals_plain_step():
    """Both options on, everything at zero: the lens is the dataset's centred pinhole exactly,
    so the rays, and with them the losses, both networks' and the poses' updates of one
    optimising step, are those of a trainer without intrinsics (each lens parameter has its own
    clip group, so none changes the poses' clip factor); and every lens parameter has moved."""
    plain, rc = _pose_trainer(None)
    learn, _ = _pose_trainer(BOTH)
    (batch, t_rand, u), = _batches(plain, rc, 1)
    mp = plain.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    ml = learn.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    assert [float(mp[k]) for k in LOSS_KEYS] == [float(ml[k]) for k in LOSS_KEYS]
    _assert_same_training_state(plain, learn)
    assert all(p.detach().abs().max() > 0 for p in learn.camera_params.parameters())  # the poses did move
    names = [k for k, _ in learn.intrinsics.named_parameters()]
    assert names == ["log_scale", "principal", "radial"]
    for name, p in learn.intrinsics.named_parameters():
        v = p.detach()
        assert torch.isfinite(v).all() and bool((v.abs() > 0).all()), (name, v)
        assert bool((v.abs() <= 1.0001e-4).all()), (name, v)  # Adam's first step: at most the learning rate
    assert len(learn.optimizer_poses.param_groups[0]["params"]) == len(plain.optimizer_poses.param_groups[0]["params"]) + 3


def test_pose_trainer_before_the_delay_leaves_the_lens_alone():
    plain, rc = _pose_trainer(None)
    learn, _ = _pose_trainer(BOTH)
    for batch, t_rand, u in _batches(plain, rc, 2):
        mp = plain.step(batch, optimize_poses=False, t_rand=t_rand, u=u)
        ml = learn.step(batch, optimize_poses=False, t_rand=t_rand, u=u)
        assert [float(mp[k]) for k in LOSS_KEYS] == [float(ml[k]) for k in LOSS_KEYS]
        assert all(p.grad is None for p in learn.intrinsics.parameters())
    _assert_same_training_state(plain, learn)
    assert all(torch.count_nonzero(p.detach()) == 0 for p in learn.intrinsics.parameters())


@pytest.mark.parametrize("option", ["learn_principal", "learn_distortion"])
def test_each_option_alone_gets_the_pose_optimizer(option):
    """Both --no_learn_* flags and a held focal length: no learnable pose, the one lens
    parameter still trains, and the held focal length never moves."""
    tr, rc = _pose_trainer({option: True, "learn_focal": False, "lens_init": (0.25, 0.0)}, learn_rotation=False,
                           learn_translation=False)
    assert not list(tr.camera_params.parameters()) and tr.optimizer_poses is not None
    name = {"learn_principal": "principal", "learn_distortion": "radial"}[option]
    assert [k for k, _ in tr.intrinsics.named_parameters()] == [name]
    before = tr.intrinsics.lens().detach().clone()
    for batch, t_rand, u in _batches(tr, rc, 2):
        tr.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    after = tr.intrinsics.lens().detach()
    moved = slice(2, 4) if option == "learn_principal" else slice(4, 6)
    assert bool((after[moved] != before[moved]).all()), (before, after)
    held = torch.ones(6, dtype=torch.bool)
    held[moved] = False
    assert torch.equal(after[held], before[held])
    assert torch.equal(after[:2], torch.full((2,), float(tr.pixel_sampler.dataset.focal), device=DEV))


# ------------------------------------------------------------- GraphedPoseTrainer --
def test_graphed_pose_trainer_with_a_lens_equals_eager(tmp_path):
    """A fresh child (tests/lens_graph_worker.py): six steps, frozen x 2 then optimising x 4,
    graphed against eager with a lens that starts at a non-zero ``lens_init`` and changes on
    every optimising step; parameters, poses and the lens parameters bit for bit, both graphs
    captured."""
    subprocess.run([sys.executable, str(ROOT / "tests" / "lens_graph_worker.py"), str(tmp_path)], check=True, timeout=300)
    r = json.loads((tmp_path / "lens_graph_report.json").read_text())
    assert r["captured"] == [False, True], r
    assert r["losses_equal"] and r["params_equal"] and r["poses_equal"] and r["lens_params_equal"], r
    assert r["n_lens_params"] == 3 and r["every_lens_entry_moved"] and r["replays_after_a_lens_update"] >= 2, r


# ------------------------------------------------------------------------- CLI --
def _write_scene(root: Path, n=3, size=16):
    from PIL import Image
    poses = np.load(sorted(GOLDEN.glob("final_poses_*.npz"))[0])["ground_truth_poses"]
    scene = root / "lego"
    rng = np.random.default_rng(0)
    for split in ("train", "val", "test"):
        (scene / split).mkdir(parents=True, exist_ok=True)
        frames = []
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "RGBA").save(
                scene / split / f"r_{i}.png")
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": poses[i].tolist()})
        (scene / f"transforms_{split}.json").write_text(json.dumps({"camera_angle_x": 0.6911112, "frames": frames}))


def test_cli_chain_train_infer_evaluate(tmp_path):
    """``train_pose_opt --learn_principal --learn_distortion --lens_init 0.25 -0.05 --graph`` with
    the focal length held (frozen and optimising graphs, a validation mid-way), then
    ``inference`` on its checkpoint (renders and refines with the learned lens) and ``pose_eval``
    on its final_poses.pt (the lens report)."""
    from noisy_src import inference, pose_eval
    from noisy_src.train_pose_opt import main
    _write_scene(tmp_path / "data")
    main(["--data_root", str(tmp_path / "data"), "--img_scale", "1.0", "--batch_size", "64", "--num_iters", "8",
          "--pose_opt_delay", "3", "--val_every", "4", "--num_samples", "16", "--num_samples_fine", "32",
          "--precision", "bf16", "--output_dir", str(tmp_path / "out"), "--graph", "--learn_principal",
          "--learn_distortion", "--lens_init", "0.25", "-0.05"])
    run, = list((tmp_path / "out").iterdir())
    ck = torch.load(run / "checkpoint_latest.pt", weights_only=True, map_location="cpu")
    assert sorted(ck["intrinsics"]) == ["focal_init", "image_size", "log_scale_held", "principal", "radial"]
    assert torch.count_nonzero(ck["intrinsics"]["log_scale_held"]) == 0  # held: never moved
    pr, rad = ck["intrinsics"]["principal"], ck["intrinsics"]["radial"]
    assert bool((pr.abs() > 0).all()) and bool((pr.abs() < 1e-3).all())
    assert bool((rad != torch.tensor([0.25, -0.05])).all()) and bool(((rad - torch.tensor([0.25, -0.05])).abs() < 1e-3).all())
    assert len(ck["optimizer_poses"]["state"]) == 4  # rotations, translations, principal, radial
    fin = torch.load(run / "final_poses.pt", weights_only=True)
    gt = fin["ground_truth_lens"]
    assert gt.shape == (6,) and gt[2:].tolist() == [8.0, 8.0, 0.0, 0.0]
    assert fin["initial_lens"].tolist() == gt[:2].tolist() + [8.0, 8.0, 0.25, float(torch.tensor(-0.05))]
    assert torch.equal(fin["optimized_lens"][:2], gt[:2]) and bool((fin["optimized_lens"][2:] != fin["initial_lens"][2:]).all())
    header, *rows = (run / "logs" / "train_metrics.csv").read_text().splitlines()
    cols = header.split(",")
    k1 = [float(r.split(",")[cols.index("lens_k1")]) for r in rows]
    cx = [float(r.split(",")[cols.index("lens_cx")]) for r in rows]
    # iterations 0..2 run before the delay: the row of iteration i holds the lens after its step
    assert len(k1) == 8 and all(k == 0.25 for k in k1[:3]) and k1[-1] != 0.25
    assert all(c == 8.0 for c in cx[:3]) and cx[-1] != 8.0
    cfg = json.loads((run / "experiment_config.json").read_text())
    assert cfg["lens"]["learn_principal"] and cfg["lens"]["lens_init"] == [0.25, -0.05] and "learn_focal" not in cfg

    lens = inference.checkpoint_intrinsics(run / "checkpoint_latest.pt")
    assert len(lens) == 6 and list(lens) == pytest.approx(fin["optimized_lens"].tolist())
    inference.main([str(run / "checkpoint_latest.pt"), "--mode", "test", "--data_root", str(tmp_path / "data"),
                    "--output_dir", str(tmp_path / "inf"), "--refine_poses", "2", "--refine_rays_per_view", "64"])
    summ = json.loads((tmp_path / "inf" / "test_metrics.json").read_text())
    assert summ["n_images"] == 3 and np.isfinite(summ["psnr_mean"]) and "pose_refinement" in summ
    pose_eval.main([str(run / "final_poses.pt")])
    rep = json.loads((run / "aligned_pose_errors.json").read_text())
    assert rep["lens"]["initial_k1_error"] == 0.25 and rep["lens"]["optimized_lens"] == pytest.approx(list(lens))
    assert rep["focal"]["optimized_focal_error_pct"] == pytest.approx([0.0, 0.0], abs=1e-4)  # held


def test_render_image_uses_the_lens():
    """``render_image`` (the validation and inference renders): six numbers go to
    ``ops.ray_directions_lens``; a caller who passes a pair, or nothing, gets what they got."""
    from noisy_src import ops
    from noisy_src.train import render_image
    seen = []

    def renderer(ro, rd, chunk_size, is_train):
        seen.append(rd)
        z = torch.zeros(ro.shape[0], device=DEV)
        return {"rgb_coarse": rd, "depth_coarse": z, "acc_coarse": z}

    pose = R.fixture_poses(1)[0].to(DEV)
    for fxy in (None, FXY, R.NEUTRAL_XY, R.LIVE):
        render_image(renderer, pose, H, W, FOCAL, fxy=fxy)
    plain, pair, neutral, live = seen
    assert torch.equal(pair, neutral) and not torch.equal(pair, plain) and not torch.equal(live, pair)
    from noisy_src.rays import get_rays
    _, want = get_rays(ops.ray_directions_lens(H, W, *R.LIVE, DEV), pose.contiguous())
    assert torch.equal(live, want.reshape(-1, 3))


# ------------------------------------------------------------------ data parallel --
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _check_two_ranks_against_one(tmp_path, share_gpu):
    steps = 2
    worker = ROOT / "tests" / "lens_dist_worker.py"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", LENS_DIST_SHARE_GPU="1" if share_gpu else "0")
    subprocess.run([sys.executable, str(worker), str(tmp_path), str(steps)], check=True, env=env, timeout=300)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                    "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(worker), str(tmp_path),
                    str(steps)], check=True, env=env, timeout=300)
    one, r0, r1 = (torch.load(tmp_path / f"lens_rank{r}_of{w}.pt", weights_only=True) for r, w in ((0, 1), (0, 2), (1, 2)))
    for k in ("nets", "poses", "lens_params", "lens", "pose_grads"):
        assert torch.equal(r0[k], r1[k]), k  # identical reduced gradients -> identical updates
    assert (r0["nets"] - one["nets"]).abs().max() < 2 * steps * 5e-4
    assert one["lens_params"].shape == (6,) and bool((one["lens"] != torch.tensor(one["lens"].tolist()[:2] + [8.0, 8.0, 0.25, -0.05])).any())
    # the averaged gradient of the first step, the lens entries (log_scale (2), principal,
    # radial) at the end of the pose buffer: the one-process gradient of the whole batch, to
    # summation order
    g1, g2 = one["pose_grads"][0], r0["pose_grads"][0]
    assert g1.shape == (2 * 3 * 3 + 6,) and g1[-6:].abs().min() > 0
    rel_pose, rel_lens = _rel(g2[:-6], g1[:-6]), _rel(g2[-6:], g1[-6:])
    print(f"LENS_DP pose-gradient rel {rel_pose:.3e}, lens-gradient rel {rel_lens:.3e}")
    assert rel_pose < 1e-4 and rel_lens < 1e-4


def test_two_ranks_sharing_one_gpu_match_one_process_with_a_lens(tmp_path):
    """Data parallel with a learned lens, two ranks over gloo on one GPU against one process
    (as test_distributed_gpu.py runs the pose step): the lens gradient rides at the end of the
    pose-gradient all-reduce, no collective of its own (test_learn_focal.py's bounds)."""
    _check_two_ranks_against_one(tmp_path, share_gpu=True)


def test_two_ranks_match_one_process_with_a_lens(tmp_path):
    """The same with one GPU per rank; skipped where test_learn_focal.py's two-GPU test skips."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    _check_two_ranks_against_one(tmp_path, share_gpu=False)
