"""GPU: the coarse-to-fine positional encoding (``NeRF.set_pe_window``).

The window is folded into the packed weight images (``nr_mlp_fold_window``) and the flat
gradient is scaled back (``nr_mlp_window_grad``); the MLP kernels themselves do not know
about it.  Checked here: the all-ones window is the identity bit for bit, the standalone
windowed encoding against the fp64 formula, the fp32 network against the fp64 oracle with
windowed encoders, the 16-bit networks against the numerics model of an oracle with folded
weights, the three ways a fold can go stale, and the hipGraph replay with a window that
changes at every step (tests/pe_window_graph_worker.py).

The standing window has ones, one fractional weight and zeros: alpha = 0.34 L per encoder
(L = 10: [1, 1, 1, 0.345, 0 x 6]; L = 4: [1, 0.287, 0, 0])."""
import copy
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from oracle import refimpl as ref

sys.path.insert(0, str(Path(__file__).resolve().parent))
from feature_interaction_ref import _cols, _enc_columns, _folded_oracle, windowed_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]


def _weights(L, frac=0.34):
    from noisy_src.train_pose_opt import pe_window_weights
    return pe_window_weights(frac * L, L)


def _window_of(cfg, frac=0.34):
    return _weights(cfg.pos_freqs, frac), (_weights(cfg.dir_freqs, frac) if cfg.use_view_dirs else None)


def _windowed_oracle64(cfg, state, window):
    """oracle.refimpl.NeRF in fp64 with its two encoders' outputs times the column weights."""
    return windowed_oracle(cfg, state, window, torch.float64)


def _kink_free(model, x, d, eps):
    """Samples whose ReLU pre-activations in ``model`` (run in fp64) all stay >= eps from 0
    (tests/test_parity_mlp.py::_kink_free, for a model that is given, not rebuilt)."""
    m64 = copy.deepcopy(model).double()
    mins = []
    hooks = [m.register_forward_hook(lambda m, i, out: mins.append(out.abs().min(dim=-1).values))
             for m in list(m64.pts_linears) + [m64.dir_linear, m64.sigma_linear]]
    with torch.no_grad():
        m64(x.double(), None if d is None else d.double())
    for h in hooks:
        h.remove()
    return torch.stack(mins, -1).min(-1).values >= eps


def _inputs(M, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, 3, generator=g) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1)
    return x, d


def _net(precision, seed=0, **model_kw):
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    cfg = ModelConfig(precision=precision, **model_kw)
    torch.manual_seed(seed)
    oracle = ref.NeRF(cfg)
    net = NeRF(cfg)
    net.load_state_dict(oracle.state_dict())
    return cfg, net.to(DEV)


def _expected(cfg, net, window, x, d):
    """What the network must compute under ``window`` at its current parameters: fp32, the
    fp64 oracle with windowed encoders; 16 bit, the numerics model of the folded oracle."""
    state = net.state_dict()
    nowin = (None, None)
    with torch.no_grad():
        if cfg.precision == "fp32":
            rgb, sig = _windowed_oracle64(cfg, state, window or nowin)(x.double(), None if d is None else d.double())
        else:
            rgb, sig = ref.mfma_emulated_nerf(_folded_oracle(cfg, state, window or nowin), cfg.precision)(x, d)
    return rgb, sig


def _assert_forward(cfg, net, window, x, d, what):
    with torch.no_grad():
        rgb, sig = net(x.to(DEV), None if d is None else d.to(DEV))
    er, es = _expected(cfg, net, window, x, d)
    e_rgb = (rgb.cpu().double() - er.double()).abs().max().item()
    e_sig = (sig.cpu().double() - es.double()).abs().max().item()
    print(what, cfg.precision, f"rgb {e_rgb:.3e} sigma {e_sig:.3e}")
    assert e_rgb < 1e-4 and e_sig < 1e-4, (what, e_rgb, e_sig)


# ------------------------------------------------------------------ 1. identity --
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_ones_window_is_the_identity_on_images_and_gradient(precision):
    """After nr_mlp_pack the fold with all-ones weights (and with null pointers) leaves the
    images byte-identical, a fold with the standing window changes them and a second fold with
    ones restores them; nr_mlp_window_grad with ones leaves a gradient bit-identical."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    cfg, net = _net(precision)
    net._ensure_flat()
    packed = net._packed_for_forward()
    want = packed.clone()
    c = ctypes.byref(net._nr_cfg)
    ones_p, ones_d = torch.ones(cfg.pos_freqs, device=DEV), torch.ones(cfg.dir_freqs, device=DEV)
    st = _hip.stream_ptr()
    call("nr_mlp_fold_window", c, ptr(net._flat), ptr(ones_p), ptr(ones_d), ptr(packed), st)
    assert torch.equal(packed, want)
    call("nr_mlp_fold_window", c, ptr(net._flat), None, None, ptr(packed), st)
    assert torch.equal(packed, want)
    wp, wd = (torch.tensor(w, device=DEV, dtype=torch.float32) for w in _window_of(cfg))
    call("nr_mlp_fold_window", c, ptr(net._flat), ptr(wp), ptr(wd), ptr(packed), st)
    assert not torch.equal(packed, want)
    call("nr_mlp_fold_window", c, ptr(net._flat), ptr(ones_p), None, ptr(packed), st)
    assert torch.equal(packed, want)
    g = torch.randn(net._param_count, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    g0 = g.clone()
    call("nr_mlp_window_grad", c, ptr(ones_p), ptr(ones_d), ptr(g), st)
    assert torch.equal(g, g0)
    call("nr_mlp_window_grad", c, ptr(wp), ptr(wd), ptr(g), st)
    assert not torch.equal(g, g0)
    # only the encoding columns changed, and by their weights
    off = 0
    for name, p in net.named_parameters():
        n = p.numel()
        a, b = g[off:off + n].view(p.shape), g0[off:off + n].view(p.shape)
        hit = [e for e in _enc_columns(cfg) if e[0] == name]
        if hit:
            _, c0, which = hit[0]
            s = _cols(_window_of(cfg)[0 if which == "pos" else 1], torch.float32).to(DEV)
            b = b.clone()
            b[:, c0:c0 + s.numel()] *= s
        assert torch.equal(a, b), name
        off += n


def _pose_trainer(precision, rc, fixed_small_angle=False, pe_schedule=None):
    """The sizes of tests/pose_graph_worker.py: 3 views of 16 x 16, 128 rays, 32 + 32 samples."""
    import numpy as np
    from noisy_src.config import ModelConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters
    z = np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"])[:3], H=16, W=16, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=128)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision=precision))
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(DEV), fixed_small_angle=fixed_small_angle)
    return PoseTrainer(mc.to(DEV), mf.to(DEV), cam, sampler, rc, pe_schedule=pe_schedule)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_ones_window_trains_bit_identically(precision):
    """Two PoseTrainer steps under an all-ones window end with parameters torch.equal to two
    steps without one (the fold writes the bytes nr_mlp_pack wrote, the gradient times 1.0)."""
    from noisy_src.config import RenderConfig
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    plain = _pose_trainer(precision, rc, fixed_small_angle=True)
    ones = _pose_trainer(precision, rc, fixed_small_angle=True, pe_schedule=lambda it, L: [1.0] * L)
    for k in range(2):
        g = torch.Generator().manual_seed(500 + k)
        batch = plain.pixel_sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(600 + k))
        t_rand, u = torch.rand(128, 32, generator=g).to(DEV), torch.rand(128, 32, generator=g).to(DEV)
        la = plain.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
        lb = ones.step(batch, optimize_poses=True, t_rand=t_rand, u=u, iteration=k)
        assert float(la["loss"]) == float(lb["loss"])
    assert ones.model_fine.pe_window() == ([1.0] * 10, [1.0] * 4)
    for a, b in ((plain.model_coarse, ones.model_coarse), (plain.model_fine, ones.model_fine)):
        assert torch.equal(a.flat_params(), b.flat_params())
    for pa, pb in zip(plain.camera_params.parameters(), ones.camera_params.parameters()):
        assert torch.equal(pa.detach(), pb.detach())
    assert plain.camera_params.rotation_deltas.detach().abs().max() > 0  # the rotations were live


# ------------------------------------------------------- 2. standalone encoding --
@pytest.mark.parametrize("L", [4, 10])
def test_standalone_windowed_encoding(L):
    """ops.positional_encoding(window=) and the network's own encoder, M = 37, C = 3, against
    gamma_w in fp64; bounds of test_parity_ops.py::test_positional_encoding_fwd_bwd."""
    from noisy_src import ops
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    w = _weights(L)
    x = torch.rand(37, 3, generator=torch.Generator().manual_seed(7)) * 8 - 4
    xr = x.double().requires_grad_(True)
    parts = [xr]
    for k in range(L):
        parts += [w[k] * torch.sin(2.0 ** k * xr), w[k] * torch.cos(2.0 ** k * xr)]
    want = torch.cat(parts, dim=-1)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(8))
    want.backward(go.double())
    xg = x.clone().to(DEV).requires_grad_(True)
    out = ops.positional_encoding(xg, L, window=torch.tensor(w, device=DEV, dtype=torch.float32))
    err = (out.detach().cpu().double() - want.detach()).abs().max().item()
    out.backward(go.to(DEV))
    gerr = (xg.grad.cpu().double() - xr.grad).abs().max().item()
    print(f"L={L}: forward {err:.3e}, backward max abs {gerr:.3e} of {xr.grad.abs().max().item():.3e}")
    assert out.shape == (37, 3 * (1 + 2 * L))
    assert err < 2e-6
    assert torch.allclose(xg.grad.cpu().double(), xr.grad, rtol=1e-4, atol=1e-3)
    zero = [3 + 6 * k + j for k in range(L) if w[k] == 0.0 for j in range(6)]
    assert zero and (out.detach()[:, zero] == 0).all()
    # the module inside a network uses the network's window; without one, the plain encoding
    net = NeRF(ModelConfig(pos_freqs=L)).to(DEV)
    plain = net.pos_encoder(x.to(DEV))
    net.set_pe_window(w, None)
    assert torch.equal(net.pos_encoder(x.to(DEV)), out.detach())
    net.set_pe_window(None, None)
    assert torch.equal(net.pos_encoder(x.to(DEV)), plain)


# ----------------------------------------------------------- 3. fp32 network --
_FP32_CONFIGS = {
    "default": dict(),
    "pos4": dict(pos_freqs=4),
    "depth5_skips1_3": dict(num_hidden_layers=5, skips=(1, 3)),
    "no_view_dirs": dict(use_view_dirs=False),
}


@pytest.mark.parametrize("name", sorted(_FP32_CONFIGS))
def test_fp32_windowed_network_vs_fp64_oracle(name):
    """M = 300 (nine full tiles and a partial one).  Forward 1e-4 abs; every parameter
    gradient, g_x and g_d to 2e-5 relative on kink-free samples (bounds and selection of
    test_parity_mlp.py::test_fp32_backward); weight-gradient columns of a zero weight are 0.0."""
    cfg, net = _net("fp32", **_FP32_CONFIGS[name])
    window = _window_of(cfg)
    x, d = _inputs(300)
    if not cfg.use_view_dirs:
        d = None
    net.set_pe_window(*window)
    _assert_forward(cfg, net, window, x, d, name)
    o64 = _windowed_oracle64(cfg, net.state_dict(), window)
    keep = _kink_free(o64, x, d, eps=2e-6).float()[:, None]
    print(name, "keep", round(keep.mean().item(), 3))
    assert keep.mean() > 0.5
    g = torch.Generator().manual_seed(3)
    gr = torch.randn(300, 3, generator=g) * keep
    gs = torch.randn(300, 1, generator=g) * keep
    xr = x.double().requires_grad_(True)
    dr = None if d is None else d.double().requires_grad_(True)
    wr, ws = o64(xr, dr)
    ((wr * gr.double()).sum() + (ws * gs.double()).sum()).backward()
    xg = x.clone().to(DEV).requires_grad_(True)
    dg = None if d is None else d.clone().to(DEV).requires_grad_(True)
    rgb, sig = net(xg, dg)
    ((rgb * gr.to(DEV)).sum() + (sig * gs.to(DEV)).sum()).backward()
    grads = {}
    for (pname, pr), pg in zip(o64.named_parameters(), net.parameters()):
        a, b = pg.grad.double().cpu(), pr.grad
        grads[pname] = pg.grad
        rel = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
        print(name, pname, f"{rel:.3e}")
        assert rel < 2e-5, (pname, rel)
    for a, b in ((xg, xr), (dg, dr)):
        if a is None:
            continue
        rel = ((a.grad.double().cpu() - b.grad).norm() / b.grad.norm()).item()
        print(name, "input", f"{rel:.3e}")
        assert rel < 2e-5, rel
    for pname, c0, which in _enc_columns(cfg):
        s = _cols(window[0 if which == "pos" else 1])
        zero = (s == 0).nonzero().flatten() + c0
        live = (s != 0).nonzero().flatten() + c0
        assert zero.numel() > 0
        assert (grads[pname][:, zero.to(DEV)] == 0.0).all(), pname
        assert (grads[pname][:, live.to(DEV)] != 0.0).any(), pname


# ------------------------------------------------------------ 4. bf16 and fp16 --
_16BIT_CONFIGS = {"default": dict(), "depth5_skips1_3": dict(num_hidden_layers=5, skips=(1, 3))}


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(_16BIT_CONFIGS))
def test_16bit_windowed_network_vs_numerics_model(precision, name):
    """M = 3000 against ref.mfma_emulated_nerf of the oracle with folded weights, its weight
    gradients mapped back by s.  Bounds, gradient scale and kink-free selection of
    test_parity_mlp.py::test_16bit_non_default_configs_vs_numerics_model: 1e-4 forward,
    1.5e-2 relative per parameter, more than half of the samples kept."""
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    cfg = ModelConfig(precision=precision, **_16BIT_CONFIGS[name])
    torch.manual_seed(11)
    oracle = ref.NeRF(cfg)
    net = NeRF(cfg)
    net.load_state_dict(oracle.state_dict())
    net = net.to(DEV)
    window = _window_of(cfg)
    net.set_pe_window(*window)
    M = 3000
    x, d = _inputs(M, seed=13)
    _assert_forward(cfg, net, window, x, d, name)
    folded = _folded_oracle(cfg, oracle.state_dict(), window)
    emu = ref.mfma_emulated_nerf(folded, precision)
    keep = _kink_free(folded, x, d, eps=1e-5).float()[:, None]
    assert keep.mean() > 0.5, keep.mean()
    g = torch.Generator().manual_seed(17)
    scale = 2.0 / (3 * 4096)
    gr = torch.randn(M, 3, generator=g) * keep * scale
    gs = torch.randn(M, 1, generator=g) * keep * scale
    er, es = emu(x, d)
    ((er * gr).sum() + (es * gs).sum()).backward()
    rgb, sig = net(x.to(DEV), d.to(DEV))
    ((rgb * gr.to(DEV)).sum() + (sig * gs.to(DEV)).sum()).backward()
    enc = {e[0]: e for e in _enc_columns(cfg)}
    rels = {}
    for (pname, pe), pg in zip(emu.base.named_parameters(), net.parameters()):
        a, b = pg.grad.cpu(), pe.grad.clone()
        if pname in enc:  # dL/d(W * s) -> dL/dW
            _, c0, which = enc[pname]
            s = _cols(window[0 if which == "pos" else 1], torch.float32)
            b[:, c0:c0 + s.numel()] *= s
            assert (a[:, c0:c0 + s.numel()][:, s == 0] == 0.0).all(), pname
        assert torch.isfinite(a).all(), pname
        rels[pname] = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    print(name, precision, "keep", round(keep.mean().item(), 3), "max grad rel", max(rels.values()))
    for pname, rel in rels.items():
        assert rel < 1.5e-2, (name, pname, rel)


# --------------------------------------------------------------- 5. staleness --
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_window_change_refolds(precision):
    """(a) Two no_grad forwards with the window changed in between (and a repeated forward in
    between, which must not need a fold): the second is the new window's network."""
    cfg, net = _net(precision)
    x, d = _inputs(300)
    w1 = _window_of(cfg)
    net.set_pe_window(*w1)
    _assert_forward(cfg, net, w1, x, d, "first window")
    key = net._fold_key
    _assert_forward(cfg, net, w1, x, d, "first window again")
    assert net._fold_key == key and key is not None
    w2 = _window_of(cfg, frac=0.71)
    net.set_pe_window(*w2)
    _assert_forward(cfg, net, w2, x, d, "second window")
    net.set_pe_window(w1[0], None)
    _assert_forward(cfg, net, (w1[0], None), x, d, "position window only")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_adam_step_then_forward_is_folded_again(precision):
    """(b) A FusedAdam step with refresh_images=True rewrites the images' encoding columns
    unfolded: the forward after it is the windowed network at the new parameters."""
    from noisy_src.optim import FusedAdam
    cfg, net = _net(precision)
    x, d = _inputs(300)
    window = _window_of(cfg)
    net.set_pe_window(*window)
    # the trainers' learning rate: Adam's first step moves every parameter by about lr
    opt = FusedAdam(list(net.parameters()), lr=5e-4, refresh_images=True)
    before = net.flat_params().clone()
    g = torch.Generator().manual_seed(3)
    gr, gs = torch.randn(300, 3, generator=g).to(DEV), torch.randn(300, 1, generator=g).to(DEV)
    rgb, sig = net(x.to(DEV), d.to(DEV))
    ((rgb * gr).sum() + (sig * gs).sum()).backward()
    images = net._packed
    opt.step()
    assert net._packed is images and net._packed_key is not None  # refreshed in the step, not re-packed
    assert not torch.equal(net.flat_params(), before)
    _assert_forward(cfg, net, window, x, d, "after the fused step")
    # zero-weight columns got a zero gradient: Adam left them where they were
    off = 0
    for pname, p in net.named_parameters():
        n = p.numel()
        for ename, c0, which in _enc_columns(cfg):
            if ename == pname:
                s = _cols(window[0 if which == "pos" else 1])
                zero = ((s == 0).nonzero().flatten() + c0).to(DEV)
                assert torch.equal(p.detach()[:, zero], before[off:off + n].view(p.shape)[:, zero]), pname
        off += n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_removing_the_window_unfolds(precision):
    """(c) After set_pe_window(None, None) the forward is the plain network's."""
    cfg, net = _net(precision)
    x, d = _inputs(300)
    window = _window_of(cfg)
    net.set_pe_window(*window)
    _assert_forward(cfg, net, window, x, d, "window")
    net.set_pe_window(None, None)
    _assert_forward(cfg, net, None, x, d, "window removed")
    with torch.no_grad():
        rgb, sig = net(x.to(DEV), d.to(DEV))
    _, plain = _net(precision)
    with torch.no_grad():
        pr, ps = plain(x.to(DEV), d.to(DEV))
    assert torch.equal(rgb, pr) and torch.equal(sig, ps)  # bit for bit a network that never had one


# ------------------------------------------------------------------------ CLI --
def _scene(root: Path, n_train=3, n_val=2, size=16):
    import numpy as np
    from PIL import Image
    poses = np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*.npz"))[0])["ground_truth_poses"]
    scene = root / "lego"
    rng = np.random.default_rng(0)
    for split, n in (("train", n_train), ("val", n_val)):
        (scene / split).mkdir(parents=True, exist_ok=True)
        frames = []
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "RGBA").save(
                scene / split / f"r_{i}.png")
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": poses[i].tolist()})
        (scene / f"transforms_{split}.json").write_text(json.dumps({"camera_angle_x": 0.6911112, "frames": frames}))


def test_cli_c2f_records_and_restores_the_window(tmp_path):
    """``--c2f 0 2 --fixed_small_angle --graph`` for 8 iterations: the run ends half way up the
    ramp (alpha = L / 2), experiment_config.json records both options, the checkpoint carries
    the window under "mi355x", and inference.load_checkpoint renders with it."""
    from noisy_src import inference
    from noisy_src.train_pose_opt import main, pe_window_weights
    _scene(tmp_path / "data")
    main(["--data_root", str(tmp_path / "data"), "--img_scale", "1.0", "--batch_size", "128", "--num_iters", "8",
          "--pose_opt_delay", "3", "--val_every", "4", "--rotation_noise", "5", "--translation_noise_pct", "5",
          "--noise_seed", "42", "--precision", "bf16", "--output_dir", str(tmp_path / "out"), "--graph",
          "--c2f", "0", "2", "--fixed_small_angle"])
    (run,) = list((tmp_path / "out").iterdir())
    cfg = json.loads((run / "experiment_config.json").read_text())
    assert cfg["c2f"] == [0.0, 2.0] and cfg["fixed_small_angle"] is True
    ck = torch.load(run / "checkpoint_latest.pt", weights_only=True, map_location="cpu")
    want = {"pos": pe_window_weights(5.0, 10), "dir": pe_window_weights(2.0, 4)}
    got = ck["mi355x"]["pe_window"]
    assert got["pos"] == pytest.approx(want["pos"], abs=1e-7) and got["dir"] == pytest.approx(want["dir"], abs=1e-7)
    assert list(ck["model_coarse"]) == list(ref.NeRF().state_dict())  # the reference's keys only
    mid = torch.load(run / "checkpoint_0000004.pt", weights_only=True, map_location="cpu")
    assert mid["mi355x"]["pe_window"]["pos"] == pytest.approx(pe_window_weights(10 * 4 / 16, 10), abs=1e-7)
    finals = torch.load(run / "final_poses.pt", weights_only=True)
    rot = finals["optimized_poses"][:, :3, :3] - finals["initial_poses"][:, :3, :3]
    assert rot.abs().amax(dim=(1, 2)).min() > 0  # fixed_small_angle reached the pose parameters
    renderer, _, _ = inference.load_checkpoint(run / "checkpoint_latest.pt", device=DEV)
    for net in (renderer.model_coarse, renderer.model_fine):
        pos, dir_ = net.pe_window()
        assert pos == pytest.approx(want["pos"], abs=1e-7) and dir_ == pytest.approx(want["dir"], abs=1e-7)
    x, d = _inputs(300)
    net = renderer.model_fine
    cfg_m = net.config
    _assert_forward(cfg_m, net, (want["pos"], want["dir"]), x, d, "restored checkpoint")


# ------------------------------------------------------------ 6. graph replay --
def test_graph_replay_with_a_moving_window(tmp_path):
    """One fresh child: a GraphedPoseTrainer whose window changes at every step (frozen and
    optimising graphs, fixed_small_angle=True) against the eager PoseTrainer, bit for bit."""
    subprocess.run([sys.executable, str(ROOT / "tests" / "pe_window_graph_worker.py"), str(tmp_path)], check=True,
                   timeout=300)
    r = json.loads((tmp_path / "pe_window_graph_report.json").read_text())
    assert r["captured"] == [False, True], r
    assert r["replays"] >= 4, r
    assert r["windows_distinct"] >= 6, r
    assert r["losses_equal"] and r["params_equal"] and r["poses_equal"] and r["eval_equal"], r
    assert r["rotations_moved"] > 0, r
    assert r["differs_from_no_window"], r
