"""The yardstick of the learned-lens tests (test_lens_host.py on the CPU, test_lens.py on the
device): ``learn_focal_ref.rays_ref`` with the six numbers of a lens, as a plain torch
restatement, differentiable by autograd in any dtype, and the scene of the end-to-end check.

The model (NeRF-- / SCNeRF form, the polynomial on the ray side, so closed form), for the
pixel (u, v) truncated like the reference's ``.long()`` table lookup, lens =
(fx, fy, cx, cy, k1, k2)::

    xn = (u - cx)/fx        yn = (v - cy)/fy
    r2 = xn*xn + yn*yn      s  = 1 + r2*(k1 + k2*r2)
    d  = (xn*s, -(yn*s), -1)     then R d, normalised; origin t

``rays_ref`` restates ``nr_rays_from_pixels_lens_fwd``, ``directions_ref``
``nr_ray_directions_lens``; test_lens_host.py holds ``rays_ref`` to ``torch.autograd.gradcheck``
in all six numbers and to ``learn_focal_ref.rays_ref`` at a centred principal point and k = 0.

The end-to-end scene is pose_refine_scene.py's (true poses, images rendered by a centred
pinhole at FOCAL = 60): rendering its first batch under ``k1 = +K`` must pull k1 down and under
``-K`` up; a principal point half a pixel off centre must be pulled back.  The scene sees only
r2 <= 0.036, so K is large: the first of 0.25, 0.5, 1.0 for which the fp64 renderer gives both
signs; test_lens_host.py asserts that it is."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_refine_scene as S  # noqa: E402
from oracle import refimpl as ref  # noqa: E402

F64 = torch.float64
NAMES = ("fx", "fy", "cx", "cy", "k1", "k2")
K_CANDIDATES = (0.25, 0.5, 1.0)
K = 0.25
PRINCIPAL_OFFSET_PX = 0.5


# The kernel tests' shapes and lenses (test_lens.py; test_lens_host.py checks on the CPU that
# these inputs can carry the bounds asked of the device).  H != W, and fx != fy, cx != cy,
# k1 != k2 in the live lens, so that a mix-up of any pair shows.
H, W = 5, 7
FOCAL = 7.3
NEUTRAL = (7.3, 7.3, 3.5, 2.5, 0.0, 0.0)
NEUTRAL_XY = (7.3, 5.9, 3.5, 2.5, 0.0, 0.0)
LIVE = (7.3, 5.9, 3.2, 2.9, 0.11, -0.03)
GOLDEN = Path(__file__).resolve().parent / "golden"


def fixture_poses(n):
    import numpy as np
    z = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    gt = torch.from_numpy(z["ground_truth_poses"]).float()
    return gt[torch.arange(n) % gt.shape[0]].contiguous()  # n_img = 300 repeats the fixture's views


def case(B, n_img, images=None, seed=0):
    """test_learn_focal.py's case: img (B,), pix (B, 2), poses (n_img, 4, 4), g_ro, g_rd (B, 3) on
    the CPU; ``images``: the image indices the rays are drawn from (default: all)."""
    g = torch.Generator().manual_seed(1000 * B + n_img + seed)
    pool = torch.arange(n_img) if images is None else torch.tensor(images)
    img = pool[torch.randint(0, len(pool), (B,), generator=g)]
    pix = torch.stack([torch.randint(0, W, (B,), generator=g), torch.randint(0, H, (B,), generator=g)], -1).float()
    return img, pix, fixture_poses(n_img), torch.randn(B, 3, generator=g), torch.randn(B, 3, generator=g)


def lens64(lens):
    """Six numbers rounded to fp32 (what the device reads), as an fp64 tensor."""
    return torch.tensor(lens, dtype=torch.float32).double()


def swapped(lens, a, b):
    out = list(lens)
    out[a], out[b] = out[b], out[a]
    return tuple(out)


def neutral(H, W, fx, fy=None):
    """The lens of a centred pinhole: (fx, fy, W/2, H/2, 0, 0) as six Python floats."""
    return (fx, fx if fy is None else fy, W / 2.0, H / 2.0, 0.0, 0.0)


def _distort(xn, yn, k1, k2):
    r2 = xn * xn + yn * yn
    s = 1 + r2 * (k1 + k2 * r2)
    return torch.stack([xn * s, -(yn * s), -torch.ones_like(xn)], -1)


def directions_ref(H, W, lens, dtype=F64):
    """``nr_ray_directions_lens``: (H, W, 3) from six numbers."""
    fx, fy, cx, cy, k1, k2 = lens
    j, i = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    return _distort((i - cx) / fx, (j - cy) / fy, k1, k2)


def rays_ref(img, pix, poses, lens):
    """(rays_o, rays_d) of pixels ``pix`` (B, 2) of images ``img`` (B,) under ``poses`` (N, 4, 4)
    and ``lens``: (6,), or (B, 6) for one lens per ray (the gradient with respect to it is then
    the per-ray term of dL/dlens).  Computed in ``poses.dtype``."""
    dtype = poses.dtype
    u, v = pix[:, 0].long().to(dtype), pix[:, 1].long().to(dtype)
    fx, fy, cx, cy, k1, k2 = (lens[..., e] for e in range(6))
    d = _distort((u - cx) / fx, (v - cy) / fy, k1, k2)
    R, t = poses[img, :3, :3], poses[img, :3, 3]
    w = (d[:, None, :] * R).sum(-1)
    return t, w / w.norm(dim=-1, keepdim=True)


def lens_grad_ref(img, pix, poses, lens, g_ro, g_rd):
    """fp64 autograd: (dL/dlens (6,), sum over the rays of |per-ray term| (6,), dL/dposes) for
    L = <g_ro, rays_o> + <g_rd, rays_d>; every input is cast to fp64 first."""
    p = poses.double().clone().requires_grad_(True)
    per_ray = lens.double().expand(img.shape[0], 6).clone().requires_grad_(True)
    ro, rd = rays_ref(img, pix.double(), p, per_ray)
    loss = (ro * g_ro.double()).sum()
    if g_rd is not None:
        loss = loss + (rd * g_rd.double()).sum()
    gp, gl = torch.autograd.grad(loss, (p, per_ray), allow_unused=True)
    if gl is None:
        gl = torch.zeros_like(per_ray)
    return gl.sum(0), gl.abs().sum(0), gp


def scene_lens(k1=0.0, principal_px=0.0):
    """The scene's lens with ``k1`` and the principal point ``principal_px`` pixels right of the
    centre: a (6,) fp32 tensor (what the device reads)."""
    return torch.tensor([S.FOCAL, S.FOCAL, S.W / 2.0 + principal_px, S.H / 2.0, k1, 0.0], dtype=torch.float32)


def scene_loss(scene, lens, batch=0, dtype=F64):
    """loss_coarse + loss_fine of the scene's batch ``batch`` rendered from the TRUE poses under
    ``lens``, by the reference's restated renderer in ``dtype``."""
    img, pix, target, t_rand, u = scene.batches[batch]
    nets = []
    for o in (scene.coarse, scene.fine):
        n = ref.NeRF(o.config).to(dtype)
        n.load_state_dict({k: v.to(dtype) for k, v in o.state_dict().items()})
        nets.append(n)
    ro, rd = rays_ref(img, pix.to(dtype), scene.gt_poses.float().to(dtype), lens)
    out = ref.render_rays(nets[0], nets[1], ro, rd, scene.rc, is_train=True, t_rand=t_rand.to(dtype), u=u.to(dtype))
    t = target.float().to(dtype)
    return ((out["rgb_coarse"] - t) ** 2).mean() + ((out["rgb_fine"] - t) ** 2).mean()


def scene_grad(scene, lens, dtype=F64, batch=0):
    """dL/dlens (six Python floats, computed in ``dtype``) at the fp32 values ``lens`` (6,).
    dL/dprincipal[0] of ``CameraIntrinsics`` is FOCAL times entry 2 (cx = W/2 + FOCAL *
    principal[0])."""
    leaf = lens.detach().float().cpu().to(dtype).requires_grad_(True)
    scene_loss(scene, leaf, batch, dtype).backward()
    return [float(g) for g in leaf.grad]
