"""The yardstick of the feature-interaction tests (test_feature_interaction_host.py on the CPU,
test_feature_interaction.py on the device): ONE restatement of the whole joint
pose-optimisation step with every optional feature switched on together -- the coarse-to-fine
positional-encoding window, the learned focal length, the distortion regulariser and a robust
photometric loss -- in plain torch, differentiable by autograd, in any dtype.

It composes the yardsticks the per-feature tests already use and adds no mathematics of its
own: ``oracle.refimpl.CameraPoseParameters`` (live Rodrigues) -> ``learn_focal_ref.rays_ref``
with ``fxy = focal * exp(log_scale)`` -> ``oracle.refimpl.render_rays`` over oracle networks
whose two encoders are column-weighted (``_Scaled``) -> ``robust_ref.loss`` on both maps +
``distortion_ref.loss_rays_prefix`` on the fine weights (z detached) + the two pose
regularisers (0.01, 0.001).  ``restate`` returns the loss, every metric of the step and the
gradients of the coarse parameters, the fine parameters, the rotation deltas, the translation
deltas and ``log_scale``.

The scene (``scene()``) is the smallest at which all of it is live, the one the per-feature
trainer tests use: 3 views of 16 x 16 from the committed rot5.0deg_trans5.0pct fixture, 64
rays, 8 coarse + 16 fine samples with injected draws, the default ``ModelConfig`` with both
sigma biases at 1, rotation and translation deltas 0.05 randn(3, 3), ``log_scale`` = (0.08,
-0.06) in mode "xy", the window ``pe_window_weights(0.34 L, L)`` on both encoders (L = 10:
three open bands, one fractional, six closed), Cauchy at c = 0.1 and a distortion weight of
0.01.  Everything here runs on the CPU; the device tests copy the tensors over.

``_cols``, ``_Scaled``, ``_enc_columns`` and ``_folded_oracle`` are the windowed-oracle pieces
of test_pe_window.py, which imports them from here.
"""
import sys
from dataclasses import dataclass, field, replace
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distortion_ref  # noqa: E402
import learn_focal_ref  # noqa: E402
import robust_ref  # noqa: E402
from oracle import refimpl as ref  # noqa: E402

F32, F64 = torch.float32, torch.float64
GOLDEN = Path(__file__).resolve().parent / "golden"

N_VIEWS, H, W = 3, 16, 16
RAYS, NC, NF = 64, 8, 16
KIND, C, WEIGHT = "cauchy", 0.1, 0.01
ROT_REG, TRANS_REG = 0.01, 0.001
LOG_SCALE = (0.08, -0.06)
FRAC = 0.34          # the window of the first step: alpha = 0.34 L
FRAC_NEXT = 0.44     # the second step's: one more band opens (L = 10: 4.4 -> four open, one fractional)
FEATURES = ("window", "robust", "distortion", "focal")
CAMERA = ("rotation", "translation", "log_scale")
GRADS = ("coarse", "fine") + CAMERA


# ------------------------------------------------- windowed oracles (from test_pe_window.py) --
def _cols(w, dtype=torch.float64):
    """The per-column scale of an encoder's output: 1 on the 3 raw columns, w_k on the 6 of frequency k."""
    return torch.tensor([1.0] * 3 + [wk for wk in w for _ in range(6)], dtype=dtype)


class _Scaled(nn.Module):
    """An oracle encoder with its output columns weighted."""

    def __init__(self, enc, cols):
        super().__init__()
        self.enc, self.cols = enc, cols

    def forward(self, x):
        return self.enc(x) * self.cols.to(x.dtype)


def _enc_columns(cfg):
    """(parameter name, first column, encoder) of every weight that reads an encoding."""
    out = [("pts_linears.0.weight", 0, "pos")]
    out += [(f"pts_linears.{i + 1}.weight", 0, "pos") for i in sorted(cfg.skips)]
    if cfg.use_view_dirs:
        out.append(("dir_linear.weight", cfg.hidden_dim, "dir"))
    return out


def _folded_oracle(cfg, state, window):
    """An fp32 oracle whose weights carry the window: W * s in fp32 on the encoding columns,
    which is exactly what the fold converts to the images' precision."""
    o = ref.NeRF(cfg)
    o.load_state_dict({k: v.detach().float().cpu() for k, v in state.items()})
    params = dict(o.named_parameters())
    with torch.no_grad():
        for name, c0, which in _enc_columns(cfg):
            w = window[0] if which == "pos" else window[1]
            if w is not None:
                s = _cols(w, torch.float32)
                params[name][:, c0:c0 + s.numel()] *= s
    return o


def windowed_oracle(cfg, state, window, dtype):
    """oracle.refimpl.NeRF in ``dtype`` with its two encoders' outputs times the column weights."""
    o = ref.NeRF(cfg).to(dtype)
    o.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in state.items()})
    pos, dir_ = window
    if pos is not None:
        o.pos_encoder = _Scaled(o.pos_encoder, _cols(pos, dtype))
    if dir_ is not None:
        o.dir_encoder = _Scaled(o.dir_encoder, _cols(dir_, dtype))
    return o


# ----------------------------------------------------------------------------------- scene --
def band_weights(frac, L) -> List[float]:
    """``pe_window_weights(frac * L, L)`` rounded to the fp32 numbers the network's window
    tensor holds, so that every dtype of the restatement reads the same inputs."""
    from noisy_src.train_pose_opt import pe_window_weights
    return torch.tensor(pe_window_weights(frac * L, L), dtype=F64).to(F32).double().tolist()


def window(frac, cfg) -> Tuple[List[float], List[float]]:
    """(pos, dir) weights at alpha = frac * L per encoder."""
    return band_weights(frac, cfg.pos_freqs), band_weights(frac, cfg.dir_freqs)


@dataclass
class State:
    """What a step reads and an optimizer moves, in fp32 on the CPU."""
    coarse: Dict[str, torch.Tensor]
    fine: Dict[str, torch.Tensor]
    rot: torch.Tensor          # (3, 3) rotation deltas
    trans: torch.Tensor        # (3, 3) translation deltas
    log_scale: torch.Tensor    # (2,)
    window: Tuple[Optional[List[float]], Optional[List[float]]]


@dataclass
class Scene:
    cfg: object
    rc: object
    init_poses: torch.Tensor   # (3, 4, 4) fp32
    focal: float
    images: torch.Tensor       # (3, H, W, 3) fp32
    img: torch.Tensor          # (RAYS,) int64
    pix: torch.Tensor          # (RAYS, 2) fp32 (u, v)
    target: torch.Tensor       # (RAYS, 3) fp32
    t_rand: torch.Tensor       # (RAYS, NC)
    u: torch.Tensor            # (RAYS, NF)
    state: State
    features: Tuple[str, ...] = field(default=FEATURES)


def scene(seed: int = 0, log_scale=LOG_SCALE) -> Scene:
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.data import synthetic_blender_data
    cfg, rc = ModelConfig(), RenderConfig(num_samples=NC, num_samples_fine=NF)
    fix = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(fix["ground_truth_poses"])[:N_VIEWS], H=H, W=W, device="cpu")
    g, gd = torch.Generator().manual_seed(100 + seed), torch.Generator().manual_seed(200 + seed)
    images = data.images.float()
    img, pix, target, t_rand, u = draw_batch(images, g)
    torch.manual_seed(seed)
    oc, of = ref.create_nerf(cfg)
    with torch.no_grad():
        for n in (oc, of):
            n.sigma_linear.bias.fill_(1.0)  # a field that absorbs: the weights spread over the ray
    state = State(coarse={k: t.detach().clone() for k, t in oc.state_dict().items()},
                  fine={k: t.detach().clone() for k, t in of.state_dict().items()},
                  rot=0.05 * torch.randn(N_VIEWS, 3, generator=gd), trans=0.05 * torch.randn(N_VIEWS, 3, generator=gd),
                  log_scale=torch.tensor(log_scale, dtype=F32), window=window(FRAC, cfg))
    return Scene(cfg=cfg, rc=rc, init_poses=torch.from_numpy(fix["initial_poses"])[:N_VIEWS].float(),
                 focal=float(data.focal), images=images, img=img, pix=pix, target=target, t_rand=t_rand, u=u, state=state)


def draw_batch(images, g):
    """(image indices, pixel (u, v), colours, t_rand, u) of RAYS pixels drawn with replacement
    by the CPU generator ``g``: the same batch on every machine, whatever the device's RNG."""
    idx = torch.randint(0, N_VIEWS * H * W, (RAYS,), generator=g)
    img, rem = idx // (H * W), idx % (H * W)
    v, u_pix = rem // W, rem % W
    return (img, torch.stack([u_pix, v], -1).float(), images[img, v, u_pix], torch.rand(RAYS, NC, generator=g),
            torch.rand(RAYS, NF, generator=g))


def without(sc: Scene, feature: str) -> Scene:
    """The scene with one feature switched off (the leave-one-out of the host test)."""
    assert feature in sc.features
    return replace(sc, features=tuple(f for f in sc.features if f != feature))


# ----------------------------------------------------------------------------- restatement --
def flat_grad(net) -> torch.Tensor:
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in net.parameters()])


def rel(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def restate(sc: Scene, state: Optional[State] = None, dtype=F64, emulate: Optional[str] = None,
            optimize_poses: bool = True) -> Dict[str, object]:
    """One ``PoseTrainer.step`` of ``sc`` at ``state`` (default: the scene's own) restated in
    ``dtype``: {"loss", "metrics": {loss_coarse, loss_fine, mse_coarse, mse_fine,
    loss_distortion}, "grads": {coarse, fine, rotation, translation, log_scale}}.

    ``emulate="bf16"``: the networks are ``ref.mfma_emulated_nerf`` of the FOLDED oracle (the
    window in the weights, as the kernels hold it); ``dtype`` must be fp32, and the network
    gradients are then those of the folded weights.  ``optimize_poses=False``: the frozen
    shape -- poses and focal length enter detached, no regulariser, camera gradients None.
    A feature missing from ``sc.features`` is off: no window, MSE, weight 0, log_scale 0."""
    st = sc.state if state is None else state
    on = set(sc.features)
    win = st.window if "window" in on else (None, None)
    if emulate is not None:
        assert dtype == F32
        nets = [ref.mfma_emulated_nerf(_folded_oracle(sc.cfg, s, win), emulate) for s in (st.coarse, st.fine)]
        bases = [n.base for n in nets]
    else:
        nets = bases = [windowed_oracle(sc.cfg, s, win, dtype) for s in (st.coarse, st.fine)]
    cam = ref.CameraPoseParameters(sc.init_poses.to(dtype)).to(dtype)
    with torch.no_grad():
        cam.rotation_deltas.copy_(st.rot.to(dtype))
        cam.translation_deltas.copy_(st.trans.to(dtype))
    ls = (st.log_scale if "focal" in on else torch.zeros(2)).detach().clone().to(dtype).requires_grad_(True)
    fxy = torch.tensor([sc.focal, sc.focal], dtype=F32).to(dtype) * torch.exp(ls)
    poses = cam.get_all_poses()
    if not optimize_poses:
        poses, fxy = poses.detach(), fxy.detach()
    ro, rd = learn_focal_ref.rays_ref(sc.img, sc.pix.to(dtype), poses, H, W, fxy)
    out, aux = ref.render_rays(nets[0], nets[1], ro, rd, sc.rc, is_train=True, t_rand=sc.t_rand.to(dtype),
                               u=sc.u.to(dtype), return_aux=True)
    t = sc.target.to(dtype)
    kind = KIND if "robust" in on else "mse"
    m = {"loss_coarse": robust_ref.loss(out["rgb_coarse"], t, kind, C),
         "loss_fine": robust_ref.loss(out["rgb_fine"], t, kind, C),
         "mse_coarse": ((out["rgb_coarse"] - t) ** 2).mean(), "mse_fine": ((out["rgb_fine"] - t) ** 2).mean()}
    loss = m["loss_coarse"] + m["loss_fine"]
    if "distortion" in on:
        m["loss_distortion"] = distortion_ref.loss_rays_prefix(aux["weights_fine"], aux["z_fine"].detach(), sc.rc.near,
                                                               sc.rc.far, F64).mean().to(dtype)
        loss = loss + WEIGHT * m["loss_distortion"]
    if optimize_poses:
        loss = loss + ROT_REG * torch.mean(cam.rotation_deltas ** 2) + TRANS_REG * torch.mean(cam.translation_deltas ** 2)
    loss.backward()
    grads = {"coarse": flat_grad(bases[0]), "fine": flat_grad(bases[1]),
             "rotation": cam.rotation_deltas.grad if optimize_poses else None,
             "translation": cam.translation_deltas.grad if optimize_poses else None,
             "log_scale": ls.grad if optimize_poses else None}
    return {"loss": float(loss.detach()), "metrics": {k: float(v.detach()) for k, v in m.items()}, "grads": grads}


# ------------------------------------------------------------------------ the device side --
def device_batch(batch, dev):
    """(PixelBatch, t_rand, u) on ``dev`` of a ``draw_batch`` tuple (or a Scene's own batch)."""
    from noisy_src.data_pose_opt import PixelBatch
    if isinstance(batch, Scene):
        batch = (batch.img, batch.pix, batch.target, batch.t_rand, batch.u)
    img, pix, target, t_rand, u = (t.to(dev) for t in batch)
    return PixelBatch(img, pix, target, in_range=True), t_rand, u


def device_nets(sc: Scene, precision: str, dev, state: Optional[State] = None):
    """The project's two networks with the oracle's parameters (no window set)."""
    from noisy_src.model import create_nerf
    st = sc.state if state is None else state
    mc, mf = create_nerf(replace(sc.cfg, precision=precision))
    mc.load_state_dict(st.coarse)
    mf.load_state_dict(st.fine)
    return mc.to(dev), mf.to(dev)


def device_camera(sc: Scene, dev, state: Optional[State] = None, fixed_small_angle: bool = False):
    """(CameraPoseParameters, CameraIntrinsics in mode "xy", PixelSampler) at the state's deltas and log_scale."""
    from types import SimpleNamespace

    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.train_pose_opt import CameraIntrinsics, CameraPoseParameters
    st = sc.state if state is None else state
    cam = CameraPoseParameters(sc.init_poses.to(dev), fixed_small_angle=fixed_small_angle)
    intr = CameraIntrinsics(sc.focal, "xy").to(dev)
    with torch.no_grad():
        cam.rotation_deltas.copy_(st.rot)
        cam.translation_deltas.copy_(st.trans)
        intr.log_scale.copy_(st.log_scale)
    ds = PixelDataset(SimpleNamespace(H=H, W=W, focal=sc.focal, images=sc.images.to(dev)))
    return cam, intr, PixelSampler(ds, batch_size=RAYS)


def device_trainer(sc: Scene, precision: str, dev, fracs=(FRAC, FRAC_NEXT), **kw):
    """The real ``PoseTrainer`` with all four keywords at the scene's state; ``iteration=k``
    of a step selects the window ``fracs[k]``.  ``kw`` overrides the trainer's keywords."""
    from noisy_src.engine import PoseTrainer
    mc, mf = device_nets(sc, precision, dev)
    cam, intr, sampler = device_camera(sc, dev)
    args = dict(pe_schedule=lambda it, L: band_weights(fracs[it], L), intrinsics=intr, distortion_weight=WEIGHT,
                loss=KIND, loss_scale=C)
    args.update(kw)
    return PoseTrainer(mc, mf, cam, sampler, sc.rc, **args)


def read_state(trainer, window) -> State:
    """The trainer's current parameters, deltas and log_scale as a ``State`` under ``window``."""
    cam = trainer.camera_params
    return State(coarse={k: v.detach().cpu().clone() for k, v in trainer.model_coarse.state_dict().items()},
                 fine={k: v.detach().cpu().clone() for k, v in trainer.model_fine.state_dict().items()},
                 rot=cam.rotation_deltas.detach().cpu().clone(), trans=cam.translation_deltas.detach().cpu().clone(),
                 log_scale=trainer.intrinsics.log_scale.detach().cpu().clone(), window=window)
