"""GPU: the learned focal length, from the kernels to the trainers.

``nr_rays_from_pixels_intr_fwd/bwd`` (focal lengths (fx, fy) read from device memory) against
the fixed-focal kernels bit for bit at fx == fy and against the fp64 restatement of
learn_focal_ref.py otherwise; ``ops.ray_directions_xy``; the sign and value of dL/dlog_scale
through the renderer on the refinement scene; ``PoseTrainer`` and ``GraphedPoseTrainer`` with
``CameraIntrinsics``; and the data-parallel step with the focal gradient in the pose buffer.

Shapes: H = 5, W = 7 (not square: an fx/fy or W/H mix-up shows), poses from the golden
fixture, random cotangents; the focal workspace and g_fxy start as NaN, so a partial or a
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
import learn_focal_ref as R  # noqa: E402
import pose_refine_scene as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
H, W = 5, 7
FOCAL = 7.3
FXY = (7.3, 5.9)
NAN = float("nan")


def _fixture_poses(n):
    z = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    gt = torch.from_numpy(z["ground_truth_poses"]).float()
    return gt[torch.arange(n) % gt.shape[0]].contiguous()  # n_img = 300 repeats the fixture's views


def _case(B, n_img, images=None, seed=0):
    """img (B,), pix (B, 2), poses (n_img, 4, 4), g_ro, g_rd (B, 3) on the CPU; ``images``: the
    image indices the rays are drawn from (default: all)."""
    g = torch.Generator().manual_seed(1000 * B + n_img + seed)
    pool = torch.arange(n_img) if images is None else torch.tensor(images)
    img = pool[torch.randint(0, len(pool), (B,), generator=g)]
    pix = torch.stack([torch.randint(0, W, (B,), generator=g), torch.randint(0, H, (B,), generator=g)], -1).float()
    return img, pix, _fixture_poses(n_img), torch.randn(B, 3, generator=g), torch.randn(B, 3, generator=g)


def _rows(t, B):
    """``t`` on the device as the first B rows of a zeroed buffer one row longer, so that a
    zero-size batch still has an address."""
    buf = torch.zeros((B + 1, *t.shape[1:]), dtype=t.dtype, device=DEV)
    buf[:B] = t.to(DEV)
    return buf


def _fwd(img, pix, poses, focal):
    """(rays_o, rays_d, sentinel rows): the fixed-focal kernel for a number, the intrinsics
    kernel for a pair."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    B = img.shape[0]
    i, p, P = _rows(img, B), _rows(pix, B), poses.to(DEV)
    ro, rd = torch.full((B + 1, 3), -7.0, device=DEV), torch.full((B + 1, 3), -7.0, device=DEV)
    if isinstance(focal, float):
        call("nr_rays_from_pixels_fwd", ptr(i), ptr(p), ptr(P), P.shape[0], H, W, focal, B, ptr(ro), ptr(rd), None,
             _hip.stream_ptr())
    else:
        f = torch.tensor(focal, device=DEV, dtype=torch.float32)
        call("nr_rays_from_pixels_intr_fwd", ptr(i), ptr(p), ptr(P), P.shape[0], H, W, ptr(f), B, ptr(ro), ptr(rd), None,
             _hip.stream_ptr())
    assert torch.equal(ro[B:], torch.full((1, 3), -7.0, device=DEV)) and torch.equal(rd[B:], ro[B:])
    return ro[:B], rd[:B]


def _bwd(img, pix, poses, focal, g_ro, g_rd):
    """g_poses of the fixed-focal kernel (a number), or (g_poses, g_fxy) of the intrinsics
    kernel (a pair), whose workspace and g_fxy start as NaN."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    B, n_img = img.shape[0], poses.shape[0]
    i, p, P, go = _rows(img, B), _rows(pix, B), poses.to(DEV), _rows(g_ro, B)
    gd = _rows(g_rd, B) if g_rd is not None else None
    g_poses = torch.zeros(n_img, 4, 4, device=DEV)
    if isinstance(focal, float):
        call("nr_rays_from_pixels_bwd", ptr(i), ptr(p), ptr(P), n_img, H, W, focal, B, ptr(go), ptr(gd), ptr(g_poses),
             _hip.stream_ptr())
        return g_poses
    f = torch.tensor(focal, device=DEV, dtype=torch.float32)
    n_ws = int(_hip.load().nr_rays_from_pixels_intr_bwd_workspace_bytes(n_img)) // 4
    assert n_ws == 2 * n_img
    ws = torch.full((n_ws + 2,), NAN, device=DEV)
    g_fxy = torch.full((3,), NAN, device=DEV)
    call("nr_rays_from_pixels_intr_bwd", ptr(i), ptr(p), ptr(P), n_img, H, W, ptr(f), B, ptr(go), ptr(gd), ptr(g_poses),
         ptr(g_fxy), ptr(ws), _hip.stream_ptr())
    assert torch.isnan(ws[n_ws:]).all() and torch.isnan(g_fxy[2])  # nothing behind the buffers was written
    if B > 0:
        assert torch.isfinite(ws[:n_ws]).all()  # every image's partial was written
    return g_poses, g_fxy[:2]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ----------------------------------------------------------------------- forward --
@pytest.mark.parametrize("n_img", [1, 3, 300])
@pytest.mark.parametrize("B", [0, 1, 257, 600])
def test_forward_equals_fixed_focal_kernel_at_equal_focal_lengths(B, n_img):
    from noisy_src import ops
    img, pix, poses, _, _ = _case(B, n_img)
    o1, d1 = _fwd(img, pix, poses, FOCAL)
    o2, d2 = _fwd(img, pix, poses, (FOCAL, FOCAL))
    assert o2.shape == (B, 3) and torch.equal(o1, o2) and torch.equal(d1, d2)
    if B:
        assert torch.isfinite(d2).all()
        # and through the public operator: a (2,) tensor dispatches to the new Function
        f = torch.tensor([FOCAL, FOCAL], device=DEV)
        o3, d3 = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), poses.to(DEV), H, W, f)
        o4, d4 = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), poses.to(DEV), H, W, FOCAL)
        assert torch.equal(o3, o1) and torch.equal(d3, d1) and torch.equal(o4, o1) and torch.equal(d4, d1)


def test_forward_unequal_focal_lengths_vs_fp64():
    """Max abs error below 1e-6, test_parity_ops.py's bound for this operator."""
    img, pix, poses, _, _ = _case(257, 3)
    o, d = _fwd(img, pix, poses, FXY)
    wo, wd = R.rays_ref(img, pix.double(), poses.double(), H, W, torch.tensor(FXY, dtype=torch.float32).double())
    assert (o.double().cpu() - wo).abs().max() < 1e-6
    assert (d.double().cpu() - wd).abs().max() < 1e-6, (d.double().cpu() - wd).abs().max()
    # fx and fy are not interchangeable here
    _, swapped = _fwd(img, pix, poses, FXY[::-1])
    assert (swapped.double().cpu() - wd).abs().max() > 1e-3


def test_ops_rejects_a_malformed_focal_tensor():
    from noisy_src import ops
    img, pix, poses, _, _ = _case(4, 3)
    args = (img.to(DEV), pix.to(DEV), poses.to(DEV), H, W)
    for bad in (torch.ones(1, device=DEV), torch.ones(2, device=DEV, dtype=torch.float64), torch.ones(4, device=DEV)[::2]):
        with pytest.raises(ValueError, match="focal"):
            ops.rays_from_pixels(*args, bad)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.rays_from_pixels(*args, torch.ones(2))


# ---------------------------------------------------------------------- backward --
BWD_CASES = {
    "one_image_600": dict(B=600, n_img=3, images=[1]),       # the stride loop runs three times; images 0, 2 empty
    "three_images_257": dict(B=257, n_img=3, images=[0, 2]),  # image 1 without a ray
    "300_images": dict(B=600, n_img=300),                      # the final reduction strides over its 256 threads
}


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_backward_vs_fixed_focal_kernel_and_fp64(name):
    """g_poses: the fixed-focal kernel's bits at fx == fy; at fx != fy within 1e-5 (relative
    norm, rotation block and translation column: test_pose_rotation.py's bound for this
    reduction) of fp64 autograd.  g_fxy: |g - g64| <= 1e-4 * sum_b |c_b| per axis, with
    sum_b |c_b| the fp64 sum of the absolute per-ray terms (fp32 unit roundoff 6e-8 x (about
    40 operations per term + at most 600 additions) ~ 4e-5, margin ~ 2.5)."""
    img, pix, poses, g_ro, g_rd = _case(**BWD_CASES[name])
    want = _bwd(img, pix, poses, FOCAL, g_ro, g_rd)
    got, _ = _bwd(img, pix, poses, (FOCAL, FOCAL), g_ro, g_rd)
    assert want.abs().max() > 0 and torch.equal(got, want)
    for fxy in ((FOCAL, FOCAL), FXY):
        g_poses, g_fxy = _bwd(img, pix, poses, fxy, g_ro, g_rd)
        g64, abs64, p64 = R.focal_grad_ref(img, pix, poses, H, W, torch.tensor(fxy, dtype=torch.float32), g_ro, g_rd)
        err = (g_fxy.double().cpu() - g64).abs()
        print(f"LEARN_FOCAL_BWD {name} fxy {fxy}: g_fxy {g_fxy.tolist()} fp64 {g64.tolist()} |err| {err.tolist()} "
              f"bound {(1e-4 * abs64).tolist()}")
        assert bool((abs64 > 0).all()) and bool((g64.abs() > 0).all())
        assert bool((err <= 1e-4 * abs64).all()), (err, 1e-4 * abs64)
        assert _rel(g_poses[:, :3, :3], p64[:, :3, :3]) < 1e-5 and _rel(g_poses[:, :3, 3], p64[:, :3, 3]) < 1e-5
        assert torch.count_nonzero(g_poses[:, 3, :]) == 0
    used = set(img.tolist())
    empty = [k for k in range(poses.shape[0]) if k not in used]
    assert torch.count_nonzero(g_poses[empty]) == 0


def test_backward_without_ray_direction_gradient_gives_exact_zeros():
    img, pix, poses, g_ro, _ = _case(257, 3)
    g_poses, g_fxy = _bwd(img, pix, poses, FXY, g_ro, None)
    assert torch.equal(g_fxy, torch.zeros(2, device=DEV))
    assert torch.equal(g_poses, _bwd(img, pix, poses, FOCAL, g_ro, None))
    assert torch.count_nonzero(g_poses[:, :3, :3]) == 0 and g_poses[:, :3, 3].abs().max() > 0


@pytest.mark.parametrize("n_img", [3, 300])
def test_backward_of_an_empty_batch(n_img):
    img, pix, poses, g_ro, g_rd = _case(0, n_img)
    g_poses, g_fxy = _bwd(img, pix, poses, FXY, g_ro, g_rd)
    assert torch.equal(g_fxy, torch.zeros(2, device=DEV)) and torch.count_nonzero(g_poses) == 0


def test_backward_is_deterministic():
    img, pix, poses, g_ro, g_rd = _case(600, 300, seed=5)
    a, b = _bwd(img, pix, poses, FXY, g_ro, g_rd), _bwd(img, pix, poses, FXY, g_ro, g_rd)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a[1].abs().min() > 0


def test_out_of_range_image_index():
    """Unvalidated: NaN rays for those rows, the others untouched; the validating mode raises;
    g_fxy and g_poses are finite and equal the batch with those rays removed, to the bit (a
    thread's removed rays sat in its own sum as skipped terms, so the order is the same)."""
    from noisy_src import ops
    img, pix, poses, g_ro, g_rd = _case(257, 3, seed=9)
    bad = img.clone()
    bad_rows = torch.tensor([0, 100, 256])
    bad[bad_rows] = torch.tensor([3, -1, 1 << 40])
    o, d = _fwd(bad, pix, poses, FXY)
    keep = torch.ones(257, dtype=torch.bool)
    keep[bad_rows] = False
    assert torch.isnan(o[bad_rows]).all() and torch.isnan(d[bad_rows]).all()
    o_ok, d_ok = _fwd(img, pix, poses, FXY)
    assert torch.equal(o[keep], o_ok[keep]) and torch.equal(d[keep], d_ok[keep])
    f = torch.tensor(FXY, device=DEV)
    with pytest.raises(IndexError):
        ops.rays_from_pixels(bad.to(DEV), pix.to(DEV), poses.to(DEV), H, W, f, validate=True)
    ops.rays_from_pixels(img.to(DEV), pix.to(DEV), poses.to(DEV), H, W, f, validate=True)
    g_poses, g_fxy = _bwd(bad, pix, poses, FXY, g_ro, g_rd)
    assert torch.isfinite(g_fxy).all() and torch.isfinite(g_poses).all()
    # the same rays with the bad ones given zero cotangents in a valid image: their terms are
    # exact zeros in the same positions of the same sums
    z_ro, z_rd = g_ro.clone(), g_rd.clone()
    z_ro[bad_rows] = 0
    z_rd[bad_rows] = 0
    w_poses, w_fxy = _bwd(img, pix, poses, FXY, z_ro, z_rd)
    assert torch.equal(g_fxy, w_fxy) and torch.equal(g_poses, w_poses)
    # and against fp64 with the rays removed
    g64, abs64, _ = R.focal_grad_ref(img[keep], pix[keep], poses, H, W, torch.tensor(FXY), g_ro[keep], g_rd[keep])
    assert bool(((g_fxy.double().cpu() - g64).abs() <= 1e-4 * abs64).all())


def test_autograd_function_returns_both_gradients():
    """``ops.rays_from_pixels`` with a tensor focal: gradients for the poses and the pair, the
    kernels' values; a detached pair gets none."""
    from noisy_src import ops
    img, pix, poses, g_ro, g_rd = _case(257, 3)
    P = poses.to(DEV).requires_grad_(True)
    f = torch.tensor(FXY, device=DEV, requires_grad=True)
    o, d = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), P, H, W, f)
    ((o * g_ro.to(DEV)).sum() + (d * g_rd.to(DEV)).sum()).backward()
    w_poses, w_fxy = _bwd(img, pix, poses, FXY, g_ro, g_rd)
    assert torch.equal(P.grad, w_poses) and torch.equal(f.grad, w_fxy)
    P2 = poses.to(DEV).requires_grad_(True)
    o, d = ops.rays_from_pixels(img.to(DEV), pix.to(DEV), P2, H, W, f.detach())
    ((o * g_ro.to(DEV)).sum() + (d * g_rd.to(DEV)).sum()).backward()
    assert torch.equal(P2.grad, w_poses)


# ------------------------------------------------------------- ray_directions_xy --
def test_ray_directions_xy():
    from noisy_src import ops
    same = ops.ray_directions_xy(H, W, FOCAL, FOCAL, W / 2.0, H / 2.0, DEV)
    assert same.shape == (H, W, 3) and torch.equal(same, ops.ray_directions(H, W, FOCAL, W / 2.0, H / 2.0, DEV))
    got = ops.ray_directions_xy(H, W, FXY[0], FXY[1], W / 2.0, H / 2.0, DEV)
    fx, fy = torch.tensor(FXY, dtype=torch.float32).double().tolist()
    assert (got.double().cpu() - R.directions_ref(H, W, fx, fy)).abs().max() < 1e-6
    assert (got.double().cpu() - R.directions_ref(H, W, fy, fx)).abs().max() > 1e-3
    # a larger table than one block, odd sizes
    big = ops.ray_directions_xy(33, 19, FXY[0], FXY[1], 9.5, 16.5, DEV)
    assert (big.double().cpu() - R.directions_ref(33, 19, fx, fy)).abs().max() < 1e-5  # entries up to ~3


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


def _device_scene_grad(scene, nets, scale):
    from noisy_src import ops
    from noisy_src.rendering import render_rays
    from noisy_src.train_pose_opt import CameraIntrinsics
    img, pix, target, _, u = scene.batches[0]
    cam = CameraIntrinsics(S.FOCAL * scale, "shared").to(DEV)
    ro, rd = ops.rays_from_pixels(img.to(DEV), pix.float().to(DEV), scene.gt_poses.float().to(DEV), S.H, S.W, cam.fxy())
    out = render_rays(nets[0], nets[1], ro, rd, scene.rc, is_train=True, u=u.float().to(DEV),
                      target_rgb=target.float().to(DEV))
    (out["loss_coarse"] + out["loss_fine"]).backward()
    return float(cam.log_scale.grad)


def test_scene_gradient_pulls_the_focal_length_back(scene):
    """dL/dlog_scale through the device renderer at 60 * SCALE and 60 / SCALE: the signs the
    fp64 renderer gives (test_learn_focal_host.py), and the fp64 values.  test_pose_refine.py
    compares its pose gradients bit for bit with another device path and holds no tolerance
    against fp64; the project's bound for a pose gradient through the renderer against the
    fp64 oracle is test_pose_rotation.py's: as close as torch's own fp32 path, relative error
    below 2 x torch32 + 1e-3."""
    nets = _device_nets(scene)
    for scale, sign in ((R.SCALE, 1.0), (1.0 / R.SCALE, -1.0)):
        got = _device_scene_grad(scene, nets, scale)
        g64, g32 = R.scene_grad(scene, scale), R.scene_grad(scene, scale, torch.float32)
        ours, torch32 = abs(got - g64) / abs(g64), abs(g32 - g64) / abs(g64)
        print(f"LEARN_FOCAL_SCENE_DEVICE scale {scale:.5f}: device {got:.6e} fp64 {g64:.6e} torch32 {g32:.6e} "
              f"rel {ours:.3e} (torch32 {torch32:.3e})")
        assert got * sign > 0 and g64 * sign > 0
        assert ours < 2 * torch32 + 1e-3, (ours, torch32)


# -------------------------------------------------------------------- PoseTrainer --
LOSS_KEYS = ("loss", "loss_coarse", "loss_fine")
B_TRAIN = 64


def _pose_trainer(mode, precision="bf16", seed=17):
    """3 views of 16 x 16, 16 coarse + 32 fine samples; ``mode``: None (no intrinsics),
    "shared" or "xy" (CameraIntrinsics at the dataset's focal length, log_scale = 0)."""
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
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(DEV), fixed_small_angle=True)
    intr = CameraIntrinsics(data.focal, mode).to(DEV) if mode is not None else None
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


@pytest.mark.parametrize("mode", ["shared", "xy"])
def test_pose_trainer_with_intrinsics_at_zero_equals_plain_step(mode):
    """log_scale = 0 gives the dataset's focal length exactly, so the rays, and with them the
    losses, both networks' and the poses' updates of one optimising step, are those of a
    trainer without intrinsics; the focal length has its own clip group, and has moved."""
    plain, rc = _pose_trainer(None)
    learn, _ = _pose_trainer(mode)
    (batch, t_rand, u), = _batches(plain, rc, 1)
    mp = plain.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    ml = learn.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    assert [float(mp[k]) for k in LOSS_KEYS] == [float(ml[k]) for k in LOSS_KEYS]
    _assert_same_training_state(plain, learn)
    assert all(p.detach().abs().max() > 0 for p in learn.camera_params.parameters())  # the poses did move
    ls = learn.intrinsics.log_scale.detach()
    assert ls.shape == ((1,) if mode == "shared" else (2,))
    assert torch.isfinite(ls).all() and bool((ls.abs() > 0).all()), ls
    assert bool((ls.abs() <= 1.0001e-4).all()), ls  # Adam's first step: at most the learning rate
    assert len(learn.optimizer_poses.param_groups[0]["params"]) == len(plain.optimizer_poses.param_groups[0]["params"]) + 1


def test_pose_trainer_before_the_delay_leaves_the_focal_length_alone():
    plain, rc = _pose_trainer(None)
    learn, _ = _pose_trainer("shared")
    for batch, t_rand, u in _batches(plain, rc, 2):
        mp = plain.step(batch, optimize_poses=False, t_rand=t_rand, u=u)
        ml = learn.step(batch, optimize_poses=False, t_rand=t_rand, u=u)
        assert [float(mp[k]) for k in LOSS_KEYS] == [float(ml[k]) for k in LOSS_KEYS]
        assert learn.intrinsics.log_scale.grad is None
    _assert_same_training_state(plain, learn)
    assert torch.count_nonzero(learn.intrinsics.log_scale.detach()) == 0


def test_focal_length_alone_gets_the_pose_optimizer():
    """Both --no_learn_* flags: no learnable pose, the focal length still trains."""
    from noisy_src.engine import PoseTrainer
    from noisy_src.train_pose_opt import CameraIntrinsics, CameraPoseParameters
    base, rc = _pose_trainer(None)
    cam = CameraPoseParameters(base.camera_params.initial_poses, learn_rotation=False, learn_translation=False)
    assert not list(cam.parameters())
    intr = CameraIntrinsics(base.pixel_sampler.dataset.focal * 1.05, "xy").to(DEV)
    tr = PoseTrainer(base.model_coarse, base.model_fine, cam, base.pixel_sampler, rc, intrinsics=intr)
    assert tr.optimizer_poses is not None
    (batch, t_rand, u), = _batches(base, rc, 1)
    tr.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    assert bool((intr.log_scale.detach().abs() > 0).all())


# ------------------------------------------------------------- GraphedPoseTrainer --
def test_graphed_pose_trainer_with_intrinsics_equals_eager(tmp_path):
    """A fresh child (tests/learn_focal_graph_worker.py): six steps, frozen x 2 then optimising
    x 4, graphed against eager with a focal length that changes on every optimising step;
    parameters, poses and log_scale bit for bit, both graphs captured."""
    subprocess.run([sys.executable, str(ROOT / "tests" / "learn_focal_graph_worker.py"), str(tmp_path)], check=True,
                   timeout=300)
    r = json.loads((tmp_path / "learn_focal_graph_report.json").read_text())
    assert r["captured"] == [False, True], r
    assert r["losses_equal"] and r["params_equal"] and r["poses_equal"] and r["log_scale_equal"], r
    assert r["log_scale_moved"] > 0 and r["replays_after_a_focal_update"] >= 2, r


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
    """``train_pose_opt --learn_focal xy --focal_init_scale 1.05 --graph`` (frozen and optimising
    graphs, a validation mid-way), then ``inference`` on its checkpoint (renders and refines
    with the learned pair) and ``pose_eval`` on its final_poses.pt (the focal report)."""
    from noisy_src import inference, pose_eval
    from noisy_src.train_pose_opt import main
    _write_scene(tmp_path / "data")
    main(["--data_root", str(tmp_path / "data"), "--img_scale", "1.0", "--batch_size", "64", "--num_iters", "8",
          "--pose_opt_delay", "3", "--val_every", "4", "--num_samples", "16", "--num_samples_fine", "32",
          "--precision", "bf16", "--output_dir", str(tmp_path / "out"), "--graph", "--learn_focal", "xy",
          "--focal_init_scale", "1.05"])
    run, = list((tmp_path / "out").iterdir())
    ck = torch.load(run / "checkpoint_latest.pt", weights_only=True, map_location="cpu")
    assert sorted(ck["intrinsics"]) == ["focal_init", "log_scale"]
    ls = ck["intrinsics"]["log_scale"]
    assert ls.shape == (2,) and bool((ls.abs() > 0).all()) and bool((ls.abs() < 1e-3).all())
    assert len(ck["optimizer_poses"]["state"]) == 3  # rotations, translations, log_scale
    fin = torch.load(run / "final_poses.pt", weights_only=True)
    gt = fin["ground_truth_focal"]
    assert torch.equal(fin["initial_focal"], ck["intrinsics"]["focal_init"])
    assert torch.allclose(fin["initial_focal"], gt * 1.05) and not torch.equal(fin["optimized_focal"], fin["initial_focal"])
    header, *rows = (run / "logs" / "train_metrics.csv").read_text().splitlines()
    col = header.split(",").index("focal_error_pct")
    errs = [float(r.split(",")[col]) for r in rows]
    assert len(errs) == 8 and all(abs(e - 5.0) < 1e-3 for e in errs[:3]) and errs[-1] != errs[0]
    cfg = json.loads((run / "experiment_config.json").read_text())
    assert cfg["learn_focal"] == {"mode": "xy", "focal_init_scale": 1.05}

    fxy = inference.checkpoint_intrinsics(run / "checkpoint_latest.pt")
    assert list(fxy) == pytest.approx(fin["optimized_focal"].tolist())
    inference.main([str(run / "checkpoint_latest.pt"), "--mode", "test", "--data_root", str(tmp_path / "data"),
                    "--output_dir", str(tmp_path / "inf"), "--refine_poses", "2", "--refine_rays_per_view", "64"])
    summ = json.loads((tmp_path / "inf" / "test_metrics.json").read_text())
    assert summ["n_images"] == 3 and np.isfinite(summ["psnr_mean"]) and "pose_refinement" in summ
    pose_eval.main([str(run / "final_poses.pt")])
    rep = json.loads((run / "aligned_pose_errors.json").read_text())
    assert rep["focal"]["initial_focal_error_pct"] == pytest.approx([5.0, 5.0], abs=1e-3)
    assert rep["focal"]["optimized_focal"] == pytest.approx(list(fxy))


# ------------------------------------------------------------------ data parallel --
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def check_two_ranks_against_one(tmp_path, run_two_ranks):
    """``run_two_ranks``: starts the two-rank run of tests/learn_focal_dist_worker.py."""
    steps = 2
    worker = ROOT / "tests" / "learn_focal_dist_worker.py"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    subprocess.run([sys.executable, str(worker), str(tmp_path), str(steps)], check=True, env=env, timeout=300)
    run_two_ranks(worker, steps, env)
    one, r0, r1 = (torch.load(tmp_path / f"focal_rank{r}_of{w}.pt", weights_only=True) for r, w in ((0, 1), (0, 2), (1, 2)))
    for k in ("nets", "poses", "log_scale", "pose_grads"):
        assert torch.equal(r0[k], r1[k]), k  # identical reduced gradients -> identical updates
    assert (r0["nets"] - one["nets"]).abs().max() < 2 * steps * 5e-4
    assert one["log_scale"].abs().max() > 0
    # the averaged gradient of the first step, the focal entries at the end of the pose buffer:
    # the one-process gradient of the whole batch, to summation order
    g1, g2 = one["pose_grads"][0], r0["pose_grads"][0]
    assert g1[-2:].abs().min() > 0
    rel_pose, rel_focal = _rel(g2[:-2], g1[:-2]), _rel(g2[-2:], g1[-2:])
    print(f"LEARN_FOCAL_DP pose-gradient rel {rel_pose:.3e}, focal-gradient rel {rel_focal:.3e}")
    assert rel_pose < 1e-4 and rel_focal < 1e-4


def test_two_ranks_match_one_process_with_intrinsics(tmp_path):
    """Data parallel with learned intrinsics, one GPU per rank: the focal gradient rides in
    the pose-gradient all-reduce (the bounds of test_distributed_gpu.py's pose test)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")

    def run(worker, steps, env):
        subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(worker), str(tmp_path),
                        str(steps)], check=True, env=env, timeout=300)

    check_two_ranks_against_one(tmp_path, run)
