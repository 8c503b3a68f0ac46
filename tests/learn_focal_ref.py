"""The yardstick of the learned-focal-length tests (test_learn_focal_host.py on the CPU,
test_learn_focal.py on the device): the rays of pixels under per-axis focal lengths as a plain
torch restatement, differentiable by autograd in any dtype, and the scene of the end-to-end
check.

``rays_ref`` restates ``nr_rays_from_pixels_intr_fwd``: pixel (u, v) (truncated like the
reference's ``.long()`` table lookup) -> camera-frame direction ((u - W/2)/fx, -(v - H/2)/fy,
-1) -> world direction R d, normalised; origin t.  test_learn_focal_host.py holds it to
``torch.autograd.gradcheck`` with respect to (fx, fy).

The end-to-end scene is pose_refine_scene.py's (true poses, images rendered at FOCAL = 60):
rendering its first batch at ``60 * s`` must pull ``log_scale`` down for s > 1 and up for
1 / s.  ``SCALE`` is the first s of 1.02, 1.05, 1.10 for which the fp64 renderer gives both
signs; test_learn_focal_host.py asserts that it is."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_refine_scene as S  # noqa: E402
from oracle import refimpl as ref  # noqa: E402

F64 = torch.float64
SCALE_CANDIDATES = (1.02, 1.05, 1.10)
SCALE = 1.02


def directions_ref(H, W, fx, fy, dtype=F64):
    """``nr_ray_directions_xy`` with the principal point at the image centre: (H, W, 3)."""
    j, i = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    return torch.stack([(i - W / 2.0) / fx, -((j - H / 2.0) / fy), -torch.ones_like(i)], -1)


def rays_ref(img, pix, poses, H, W, fxy):
    """(rays_o, rays_d) of pixels ``pix`` (B, 2) of images ``img`` (B,) under ``poses`` (N, 4, 4)
    and focal lengths ``fxy``: (2,), or (B, 2) for one pair per ray (the gradient with respect
    to it is then the per-ray term of dL/dfxy)."""
    dtype = poses.dtype
    u, v = pix[:, 0].long().to(dtype), pix[:, 1].long().to(dtype)
    fx, fy = fxy[..., 0], fxy[..., 1]
    d = torch.stack([(u - W / 2.0) / fx, -((v - H / 2.0) / fy), -torch.ones_like(u)], -1)
    R, t = poses[img, :3, :3], poses[img, :3, 3]
    w = (d[:, None, :] * R).sum(-1)
    return t, w / w.norm(dim=-1, keepdim=True)


def focal_grad_ref(img, pix, poses, H, W, fxy, g_ro, g_rd):
    """fp64 autograd: (dL/dfxy (2,), sum over the rays of |per-ray term| (2,), dL/dposes) for
    L = <g_ro, rays_o> + <g_rd, rays_d>; every input is cast to fp64 first."""
    p = poses.double().clone().requires_grad_(True)
    per_ray = fxy.double().expand(img.shape[0], 2).clone().requires_grad_(True)
    ro, rd = rays_ref(img, pix.double(), p, H, W, per_ray)
    loss = (ro * g_ro.double()).sum()
    if g_rd is not None:
        loss = loss + (rd * g_rd.double()).sum()
    gp, gf = torch.autograd.grad(loss, (p, per_ray), allow_unused=True)
    if gf is None:
        gf = torch.zeros_like(per_ray)
    return gf.sum(0), gf.abs().sum(0), gp


def scene_loss(scene, log_scale, scale, batch=0, dtype=F64):
    """loss_coarse + loss_fine of the scene's batch ``batch`` rendered from the TRUE poses with
    both focal lengths at ``FOCAL * scale * exp(log_scale)`` (``log_scale``: (1,), the shared
    mode of ``CameraIntrinsics``), by the reference's restated renderer in ``dtype``."""
    img, pix, target, t_rand, u = scene.batches[batch]
    nets = []
    for o in (scene.coarse, scene.fine):
        n = ref.NeRF(o.config).to(dtype)
        n.load_state_dict({k: v.to(dtype) for k, v in o.state_dict().items()})
        nets.append(n)
    focal = torch.tensor([S.FOCAL * scale, S.FOCAL * scale], dtype=torch.float32).to(dtype)
    ro, rd = rays_ref(img, pix.to(dtype), scene.gt_poses.float().to(dtype), S.H, S.W, focal * torch.exp(log_scale))
    out = ref.render_rays(nets[0], nets[1], ro, rd, scene.rc, is_train=True, t_rand=t_rand.to(dtype), u=u.to(dtype))
    t = target.float().to(dtype)
    return ((out["rgb_coarse"] - t) ** 2).mean() + ((out["rgb_fine"] - t) ** 2).mean()


def scene_grad(scene, scale, dtype=F64):
    """dL/dlog_scale at log_scale = 0 (a Python float, computed in ``dtype``)."""
    ls = torch.zeros(1, dtype=dtype, requires_grad=True)
    scene_loss(scene, ls, scale, dtype=dtype).backward()
    return float(ls.grad)
