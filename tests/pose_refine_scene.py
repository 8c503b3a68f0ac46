"""The small scene of the pose-refinement tests (test_pose_refine_host.py on the CPU in fp64,
test_pose_refine.py on the device in fp32), built from a seed alone:

* a random-init ``ref.NeRF`` pair, which is the frozen field: ModelConfig(pos_freqs=4,
  dir_freqs=1) and the fine network a copy of the coarse one.  (With the default 10
  frequencies a random-init network is noise at the scale of a pixel, which no pose can be
  read from, and two different random networks disagree about the image, so that the
  coarse loss pulls away from the true pose);
* 4 views of 16 x 16 pixels on a ring of radius 4 looking at the origin, their images
  rendered by that same pair at the TRUE poses, deterministically (``is_train=False``),
  with 16 coarse + 32 fine samples;
* initial poses = the true ones turned by 0.5 degrees about a random axis and moved by
  0.02 in a random direction;
* 100 fixed batches of 64 rays (image, pixel) with their inverse-CDF uniforms ``u``; the
  coarse samples are not jittered (``perturb=False``), FOCAL = 60 (a 15 degree view of the
  field's centre: 0.5 degrees are half a pixel).

``SEED`` is the first of seeds 0..7 at which the fp64 oracle (``oracle_refine``: the
reference's restated renderer, a ``torch.linalg.matrix_exp`` pose map, torch's Adam with the
0.1 clip) at least halves both mean pose errors; test_pose_refine_host.py asserts that."""
import copy
import math
from types import SimpleNamespace

import torch

from oracle import refimpl as ref

SEED = 0
H = W = 16
FOCAL = 60.0
POS_FREQS = 4
N_VIEWS, N_STEPS, N_RAYS = 4, 100, 64
ROT_DEG, TRANS = 0.5, 0.02
POSE_LR, MAX_NORM = 1e-3, 0.1
F64 = torch.float64


def model_config(precision="fp32"):
    from noisy_src.config import ModelConfig
    return ModelConfig(pos_freqs=POS_FREQS, dir_freqs=1, precision=precision)


def render_config():
    from noisy_src.config import RenderConfig
    return RenderConfig(num_samples=16, num_samples_fine=32, perturb=False, raw_noise_std=0.0)


def skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def pose_map(init, w, dt):
    """R = exp([w]x) R_0, t = t_0 + dt (the SE(3) map of CameraPoseParameters), any dtype."""
    out = torch.zeros_like(init)
    out[:, :3, :3] = torch.linalg.matrix_exp(skew(w)) @ init[:, :3, :3]
    out[:, :3, 3] = init[:, :3, 3] + dt
    out[:, 3, 3] = 1.0
    return out


def rays_of(img, pix, poses):
    """Rays of pixels (image index, (u, v)) under ``poses`` (data_pose_opt.py's gather)."""
    dirs = ref.get_ray_directions(H, W, FOCAL).to(poses.dtype)[pix[:, 1].long(), pix[:, 0].long()]
    R, t = poses[img, :3, :3], poses[img, :3, 3]
    d = (dirs[:, None, :] * R).sum(-1)
    return t, d / d.norm(dim=-1, keepdim=True)


def ring_poses(n, g):
    """Look-at-origin cameras at radius 4 with varied azimuth and height."""
    out = torch.zeros(n, 4, 4, dtype=F64)
    for k in range(n):
        th = 2 * math.pi * (k + 0.3 * torch.rand((), generator=g, dtype=F64).item()) / n
        pos = torch.tensor([4 * math.cos(th) * 0.9, 4 * math.sin(th) * 0.9, 4 * 0.436 * (1 if k % 2 else -1)], dtype=F64)
        pos = 4 * pos / pos.norm()
        fwd = -pos / pos.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=F64))
        right = right / right.norm()
        up = torch.linalg.cross(right, fwd)
        out[k, :3, 0], out[k, :3, 1], out[k, :3, 2], out[k, :3, 3], out[k, 3, 3] = right, up, -fwd, pos, 1.0
    return out


def _unit(n, g):
    v = torch.randn(n, 3, generator=g, dtype=F64)
    return v / v.norm(dim=-1, keepdim=True)


def build(seed=SEED):
    """The scene as a namespace: coarse, fine (fp64 oracle networks), gt_poses, init_poses,
    images (4,16,16,3), batches [(img, pix, target, t_rand, u)] -- all fp64 on the CPU."""
    from noisy_src.config import ModelConfig
    rc = render_config()
    torch.manual_seed(seed)
    coarse = ref.NeRF(model_config()).double()
    fine = copy.deepcopy(coarse)
    for p in list(coarse.parameters()) + list(fine.parameters()):
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(1000 + seed)
    gt = ring_poses(N_VIEWS, g)
    vv, uu = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    pix_all = torch.stack([uu.flatten(), vv.flatten()], -1)
    images = []
    with torch.no_grad():
        for k in range(N_VIEWS):
            o, d = rays_of(torch.full((H * W,), k), pix_all, gt)
            images.append(ref.render_rays(coarse, fine, o, d, rc, is_train=False)["rgb_fine"].reshape(H, W, 3))
    images = torch.stack(images)
    init = pose_map(gt, _unit(N_VIEWS, g) * math.radians(ROT_DEG), _unit(N_VIEWS, g) * TRANS)
    batches = []
    for _ in range(N_STEPS):
        img = torch.randint(0, N_VIEWS, (N_RAYS,), generator=g)
        pix = torch.stack([torch.randint(0, W, (N_RAYS,), generator=g), torch.randint(0, H, (N_RAYS,), generator=g)],
                          -1).double()
        target = images[img, pix[:, 1].long(), pix[:, 0].long()]
        t_rand = torch.rand(N_RAYS, rc.num_samples, generator=g, dtype=F64)
        u = torch.rand(N_RAYS, rc.num_samples_fine, generator=g, dtype=F64)
        batches.append((img, pix, target, t_rand, u))
    return SimpleNamespace(seed=seed, coarse=coarse, fine=fine, rc=rc, gt_poses=gt, init_poses=init, images=images,
                           batches=batches)


def mean_errors(poses, gt):
    """(mean rotation error in degrees, mean translation error) of poses against gt."""
    from noisy_src.pose_eval import pose_error
    e = [pose_error(gt[i].double().cpu(), poses[i].double().cpu()) for i in range(gt.shape[0])]
    return (sum(x["rotation_error_deg"] for x in e) / len(e), sum(x["translation_error"] for x in e) / len(e))


def oracle_refine(scene):
    """The refinement in fp64 on the CPU -> (final poses, losses of every step)."""
    w = torch.zeros(N_VIEWS, 3, dtype=F64, requires_grad=True)
    dt = torch.zeros(N_VIEWS, 3, dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([w, dt], lr=POSE_LR)
    losses = []
    for img, pix, target, t_rand, u in scene.batches:
        opt.zero_grad(set_to_none=True)
        o, d = rays_of(img, pix, pose_map(scene.init_poses, w, dt))
        out = ref.render_rays(scene.coarse, scene.fine, o, d, scene.rc, is_train=True, t_rand=t_rand, u=u)
        loss = ((out["rgb_coarse"] - target) ** 2).mean() + ((out["rgb_fine"] - target) ** 2).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([w, dt], MAX_NORM)
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        return pose_map(scene.init_poses, w, dt), losses
