"""GPU: the distortion regulariser (csrc/distortion.hip, ops.distortion_loss, the trainers'
``distortion_weight``) against tests/distortion_ref.py.

Parity bound.  The truth is the restatement's O(S^2) form in fp64 on the kernel's own fp32
inputs, evaluated on the CPU.  The same form in fp32 is what plain fp32 arithmetic makes of
those inputs; its distance from the truth, E32 (the maximum over the batch), is the yardstick:
the kernel may be at most 4 x E32 away (the factor covers the prefix form's other summation
order, up to 2x in fp32), with a floor of one fp32 ulp of the quantity itself -- of the loss
for ``loss`` and each ``loss_rays`` entry, of the ray's largest gradient entry for its
``g_weights`` -- because no fp32 output can be asked to be closer than its own rounding.  With
``NR_WRITE_PROFILES`` set, the measured errors and the bounds go to
profiles/distortion_parity.json.

The chain test uses test_parity_ops.py's composite-backward tolerances (rtol 1e-3, atol 1e-4);
the trainer tests test_parity_fullsize.py's fp32 step bounds (relative L2 of a network's flat
gradient below 1e-3; the translation gradient as close to the fp64 truth as torch's fp32
evaluation of the reference, 2 x + 1e-3).  Both first check, on the oracle alone, that the
distortion term's share of the compared gradient is far above that tolerance, so a step that
dropped the term would fail.
"""
import copy
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distortion_ref as R  # noqa: E402
from oracle import refimpl as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
F32, F64 = torch.float32, torch.float64

S_ALL = (1, 2, 63, 64, 65, 192, 513, 4096)
SHAPES = [(S, B) for S in S_ALL for B in ((5,) if S == 4096 else (1, 5, 64))]
KINDS = (("uniform", 2.0, 6.0), ("peaked", 0.5, 3.0), ("ties", 2.0, 6.0), ("zero", 0.5, 3.0))
_records = []


@pytest.fixture(scope="module", autouse=True)
def _write_profile():
    yield
    if os.environ.get("NR_WRITE_PROFILES") and _records:
        (ROOT / "profiles" / "distortion_parity.json").write_text(json.dumps(
            {"bound": "max(4 x fp32-vs-fp64 error of the O(S^2) form, 1 fp32 ulp)", "cases": _records}, indent=1) + "\n")


def _ulp32(x):
    x = abs(float(x))
    return 0.0 if x == 0.0 else 2.0 ** (math.frexp(x)[1] - 1 - 23)


def _inputs(kind, S, B, near, far):
    g = torch.Generator().manual_seed(7000 + 10 * S + B)
    z = R.sorted_z(B, S, near, far, g, ties=kind == "ties")
    if kind == "zero":
        return torch.zeros(B, S), z
    sigma = R.peaked_sigma(B, S) if kind == "peaked" else R.uniform_sigma(B, S, g)
    return R.composite_weights(sigma, z), z


def _run(w, z, near, far, grad_scale=1.0, poison=False):
    """nr_distortion_loss through the C ABI with every output: (loss, loss_rays, g_weights)."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    B, S = z.shape
    wd, zd = w.to(DEV).contiguous(), z.to(DEV).contiguous()
    loss = torch.empty((), device=DEV)
    rays = torch.empty(B, device=DEV)
    g = torch.empty(B, S, device=DEV)
    ws = torch.zeros(int(_hip.load().nr_distortion_workspace_bytes(B)), device=DEV, dtype=torch.uint8)
    if poison:
        ws.fill_(0xFF)  # NaN as fp32 and as fp64
        g.fill_(float("nan"))
        rays.fill_(float("nan"))
        loss.fill_(float("nan"))
    call("nr_distortion_loss", ptr(wd), ptr(zd), B, S, float(near), float(far), float(grad_scale), ptr(loss), ptr(rays),
         ptr(g), ptr(ws), _hip.stream_ptr())
    return loss.cpu(), rays.cpu(), g.cpu()


# ------------------------------------------------------------------------- parity --
@pytest.mark.parametrize("S,B", SHAPES)
def test_parity_with_the_fp64_restatement(S, B):
    for kind, near, far in KINDS:
        w, z = _inputs(kind, S, B, near, far)
        loss, rays, g = _run(w, z, near, far)
        if kind == "zero":
            assert float(loss) == 0.0 and not rays.any() and not g.any(), kind
            _records.append(dict(S=S, B=B, kind=kind, near=near, far=far, exact_zero=True))
            continue
        l64, r64, g64 = R.pairs_loss_and_grad(w, z, near, far, F64)
        l32, r32, g32 = R.pairs_loss_and_grad(w, z, near, far, F32)
        e32 = dict(loss=abs(float(l32.double() - l64)), rays=float((r32.double() - r64).abs().max()),
                   grad=float((g32.double() - g64).abs().max()))
        err_loss = abs(float(loss.double() - l64))
        err_rays = (rays.double() - r64).abs()
        err_grad = (g.double() - g64).abs().amax(-1)
        bound_loss = max(4 * e32["loss"], _ulp32(l64))
        bound_rays = torch.tensor([max(4 * e32["rays"], _ulp32(v)) for v in r64], dtype=F64)
        bound_grad = torch.tensor([max(4 * e32["grad"], _ulp32(v)) for v in g64.abs().amax(-1)], dtype=F64)
        rec = dict(S=S, B=B, kind=kind, near=near, far=far, loss=float(l64), e32=e32,
                   err=dict(loss=err_loss, rays=float(err_rays.max()), grad=float(err_grad.max())),
                   bound=dict(loss=bound_loss, rays=float(bound_rays.min()), grad=float(bound_grad.min())))
        _records.append(rec)
        print("DISTORTION_PARITY " + json.dumps(rec))
        assert err_loss <= bound_loss, rec
        assert bool((err_rays <= bound_rays).all()), rec
        assert bool((err_grad <= bound_grad).all()), rec


def test_grad_scale_scales_only_the_gradient():
    w, z = _inputs("uniform", 65, 5, 2.0, 6.0)
    l1, r1, g1 = _run(w, z, 2.0, 6.0, 1.0)
    l2, r2, g2 = _run(w, z, 2.0, 6.0, 0.25)  # a power of two: exact
    assert torch.equal(l1, l2) and torch.equal(r1, r2) and torch.equal(g1 * 0.25, g2)


# -------------------------------------------------------------------- determinism --
@pytest.mark.parametrize("S,B", [(65, 5), (192, 64), (513, 5)])
def test_bit_identical_from_run_to_run_and_over_poisoned_scratch(S, B):
    w, z = _inputs("uniform", S, B, 2.0, 6.0)
    a = _run(w, z, 2.0, 6.0)
    b = _run(w, z, 2.0, 6.0)
    c = _run(w, z, 2.0, 6.0, poison=True)
    for x, y, p in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, p)
        assert bool(torch.isfinite(p).all())


# -------------------------------------------------------------------------- the op --
def test_op_matches_the_entry_point_and_gives_only_weights_a_gradient():
    from noisy_src import ops
    w, z = _inputs("uniform", 65, 5, 2.0, 6.0)
    loss, _, g = _run(w, z, 2.0, 6.0, 0.5)
    wd = w.to(DEV).requires_grad_(True)
    zd = z.to(DEV).requires_grad_(True)
    out = ops.distortion_loss(wd, zd, 2.0, 6.0, grad_scale=0.5)
    assert torch.equal(out.detach().cpu(), loss)
    out.backward(ops.unit_grad(out.device))
    assert torch.equal(wd.grad.cpu(), g) and zd.grad is None
    with torch.no_grad():  # nothing asks for a gradient: none is computed
        assert torch.equal(ops.distortion_loss(wd, zd, 2.0, 6.0).cpu(), loss)
    with pytest.raises(ValueError, match="same"):
        ops.distortion_loss(wd, zd[:, :-1], 2.0, 6.0)
    with pytest.raises(RuntimeError, match="nr_distortion_loss"):
        ops.distortion_loss(wd, zd, 6.0, 2.0)


# ---------------------------------------------------------- chain through compositing --
@pytest.mark.parametrize("grad_scale,upstream", [(1.0, None), (0.37, None), (1.0, 0.7)])
def test_chain_through_composite_mse(grad_scale, upstream):
    """composite_mse -> distortion_loss on its weights -> backward against the oracle's
    raw2outputs + MSE + the restated term under torch autograd (B = 5, S = 65)."""
    from noisy_src import ops
    B, S, near, far = 5, 65, 2.0, 6.0
    g = torch.Generator().manual_seed(31)
    z = R.sorted_z(B, S, near, far, g)
    rgb, sigma = torch.rand(B, S, 3, generator=g), 3.0 * torch.rand(B, S, generator=g)
    rd = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 1.1
    tgt = torch.rand(B, 3, generator=g)

    def oracle(with_term):
        r, s = rgb.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
        out = ref.raw2outputs(r, s[..., None], z, rd)
        total = ((out["rgb_map"] - tgt) ** 2).mean()
        if with_term:
            total = total + grad_scale * R.loss_rays_prefix(out["weights"], z, near, far, F64).mean().float()
        total.backward(torch.tensor(1.0 if upstream is None else upstream))
        return r.grad, s.grad

    want_rgb, want_sigma = oracle(True)
    _, plain_sigma = oracle(False)
    # the term moves g_sigma by over ten times the tolerance below (g_rgb it does not reach)
    assert float((want_sigma - plain_sigma).abs().max()) > 10 * 1e-4

    r, s = rgb.to(DEV).requires_grad_(True), sigma.to(DEV).requires_grad_(True)
    loss, _, _, _, weights = ops.composite_mse(r, s, z.to(DEV), rd.to(DEV), tgt.to(DEV))
    dl = ops.distortion_loss(weights, z.to(DEV), near, far, grad_scale=grad_scale)
    seed = ops.unit_grad(loss.device) if upstream is None else torch.tensor(upstream, device=DEV)
    (loss + dl).backward(seed)
    for name, got, want in (("rgb", r.grad.cpu(), want_rgb), ("sigma", s.grad.cpu(), want_sigma)):
        assert torch.allclose(got, want, rtol=1e-3, atol=1e-4), (name, float((got - want).abs().max()))


# ------------------------------------------------------------------------- trainers --
NC, NF, RAYS, WEIGHT = 8, 16, 64, 0.01


def _rc():
    from noisy_src.config import RenderConfig
    return RenderConfig(num_samples=NC, num_samples_fine=NF)


def _nets(precision="fp32", seed=0):
    """(oracle coarse, oracle fine, coarse, fine) with equal parameters, sigma bias 1 (a field
    that absorbs: the weights spread over the ray and the term has something to act on)."""
    from noisy_src.config import ModelConfig
    from noisy_src.model import create_nerf
    cfg = ModelConfig(precision=precision)
    torch.manual_seed(seed)
    oc, of = ref.create_nerf(cfg)
    with torch.no_grad():
        for n in (oc, of):
            n.sigma_linear.bias.fill_(1.0)
    mc, mf = create_nerf(cfg)
    mc.load_state_dict(oc.state_dict())
    mf.load_state_dict(of.state_dict())
    return oc.to(DEV), of.to(DEV), mc.to(DEV), mf.to(DEV)


def _ray_batches(n, seed=23):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        o = torch.randn(RAYS, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
        d = torch.nn.functional.normalize(torch.randn(RAYS, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1)
        out.append([t.to(DEV) for t in (o, d, torch.rand(RAYS, 3, generator=g), torch.rand(RAYS, NC, generator=g),
                                        torch.rand(RAYS, NF, generator=g))])
    return out


def _flat_grad(net):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in net.parameters()])


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _capture_grads(optimizer, nets, store):
    orig = optimizer.step

    def step(*a, **k):
        store.extend(_flat_grad(n).clone() for n in nets)
        return orig(*a, **k)

    optimizer.step = step


def _oracle_loss(oc, of, o, d, tgt, tr, u, weight, dtype=F32):
    rc = _rc()
    out, aux = ref.render_rays(oc, of, o.to(dtype), d.to(dtype), rc, is_train=True, t_rand=tr.to(dtype), u=u.to(dtype),
                               return_aux=True)
    t = tgt.to(dtype)
    loss = ((out["rgb_coarse"] - t) ** 2).mean() + ((out["rgb_fine"] - t) ** 2).mean()
    dist = R.loss_rays_prefix(aux["weights_fine"], aux["z_fine"].detach(), rc.near, rc.far, F64).mean()
    return loss + weight * dist.to(dtype), dist


def test_trainer_at_weight_zero_is_the_trainer_without_the_keyword():
    from noisy_src.engine import Trainer
    trainers = []
    for kw in ({}, {"distortion_weight": 0.0}):
        _, _, mc, mf = _nets("bf16", seed=17)
        trainers.append(Trainer(mc, mf, _rc(), **kw))
    for b in _ray_batches(2):
        ms = [t.step(*b) for t in trainers]
        assert "loss_distortion" not in ms[1] and torch.equal(ms[0]["loss"], ms[1]["loss"])
    for na, nb in zip((trainers[0].model_coarse, trainers[0].model_fine), (trainers[1].model_coarse, trainers[1].model_fine)):
        assert torch.equal(na.flat_params(), nb.flat_params())


@pytest.mark.parametrize("coarse_stream", [False, True])
def test_trainer_step_gradients_match_the_oracle_plus_the_restated_term(coarse_stream):
    from noisy_src.engine import Trainer
    b = _ray_batches(1)[0]
    want = {}
    for weight in (0.0, WEIGHT):
        oc, of, _, _ = _nets()
        loss, dist = _oracle_loss(oc, of, *b, weight)
        loss.backward()
        want[weight] = (_flat_grad(oc), _flat_grad(of), float(loss), float(dist))
    assert torch.equal(want[0.0][0], want[WEIGHT][0])  # the coarse network never sees the term
    assert _rel(want[WEIGHT][1], want[0.0][1]) > 10 * 1e-3  # the fine one does, far above the tolerance
    got = {}
    for weight in (0.0, WEIGHT):
        _, _, mc, mf = _nets()
        tr = Trainer(mc, mf, _rc(), coarse_stream=coarse_stream, distortion_weight=weight)
        grads = []
        _capture_grads(tr.optimizer, (mc, mf), grads)
        got[weight] = (grads, tr.step(*b))
        assert tr.last_step_coarse_stream == coarse_stream
    grads, m = got[WEIGHT]
    assert torch.equal(grads[0], got[0.0][0][0])  # coarse gradient: bit-identical to the weight-0 step
    assert not torch.equal(grads[1], got[0.0][0][1])
    assert _rel(grads[0], want[WEIGHT][0]) < 1e-3 and _rel(grads[1], want[WEIGHT][1]) < 1e-3
    # the weights agree with the oracle's to 2e-5 (test_parity_ops.py) and |dL/dw| stays below 2
    assert abs(float(m["loss_distortion"]) - want[WEIGHT][3]) < 1e-4 * want[WEIGHT][3]
    assert abs(float(m["loss"]) - want[WEIGHT][2]) < 1e-5 * want[WEIGHT][2]
    assert torch.equal(m["loss_fine"], got[0.0][1]["loss_fine"])  # the MSE metrics are not the term's
    assert abs(float(m["loss"]) - (float(got[0.0][1]["loss"]) + WEIGHT * float(m["loss_distortion"]))) < 1e-6


def test_trainer_without_a_fine_network_regularises_the_coarse_one():
    from noisy_src.engine import Trainer
    b = _ray_batches(1)[0]
    grads = {}
    for weight in (0.0, WEIGHT):
        _, _, mc, _ = _nets()
        tr = Trainer(mc, None, _rc(), distortion_weight=weight)
        store = []
        _capture_grads(tr.optimizer, (mc,), store)
        m = tr.step(*b)
        grads[weight] = store[0]
        assert ("loss_distortion" in m) == (weight > 0)
    assert not torch.equal(grads[0.0], grads[WEIGHT])


def test_pose_trainer_step_gradients_match_the_oracle_plus_the_restated_term():
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.train_pose_opt import CameraPoseParameters
    fix = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    init = torch.from_numpy(fix["initial_poses"])[:3]
    H = W = 16
    data = synthetic_blender_data(torch.from_numpy(fix["ground_truth_poses"])[:3], H=H, W=W, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=RAYS)
    batch = sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(5))
    g = torch.Generator().manual_seed(6)
    tr_, u = torch.rand(RAYS, NC, generator=g).to(DEV), torch.rand(RAYS, NF, generator=g).to(DEV)

    def oracle(weight, dtype=F32):
        oc, of, _, _ = _nets()
        oc, of = copy.deepcopy(oc).to(dtype), copy.deepcopy(of).to(dtype)
        cam = ref.CameraPoseParameters(init.to(DEV, dtype)).to(dtype)
        ro, rd = ref.get_rays_from_pixels(batch.image_indices, batch.pixel_coords.to(dtype), cam.get_all_poses(), H, W,
                                          data.focal)
        loss, dist = _oracle_loss(oc, of, ro, rd, batch.target_rgb, tr_, u, weight, dtype)
        loss = loss + 0.01 * torch.mean(cam.rotation_deltas ** 2) + 0.001 * torch.mean(cam.translation_deltas ** 2)
        loss.backward()
        return _flat_grad(oc), _flat_grad(of), cam.translation_deltas.grad, cam.rotation_deltas.grad, float(loss)

    want, plain, truth = oracle(WEIGHT), oracle(0.0), oracle(WEIGHT, F64)
    assert _rel(want[1], plain[1]) > 10 * 1e-3 and _rel(want[2], plain[2]) > 10 * 1e-3  # the term's share

    got = {}
    for weight in (0.0, WEIGHT):
        _, _, mc, mf = _nets()
        cam = CameraPoseParameters(init.to(DEV))
        tr = PoseTrainer(mc, mf, cam, sampler, _rc(), distortion_weight=weight)
        grads = []
        orig = tr.optimizer_poses.step

        def pose_step(*a, _cam=cam, _grads=grads, _orig=orig, **k):
            _grads.extend([_cam.translation_deltas.grad.clone(), _cam.rotation_deltas.grad.clone()])
            return _orig(*a, **k)

        tr.optimizer_poses.step = pose_step
        _capture_grads(tr.optimizer_nerf, (mc, mf), grads)
        got[weight] = (grads, tr.step(batch, optimize_poses=True, t_rand=tr_, u=u))
    (gc, gf, gt, gr), m = got[WEIGHT]
    assert torch.equal(gc, got[0.0][0][0]) and not torch.equal(gf, got[0.0][0][1])
    assert _rel(gc, want[0]) < 1e-3 and _rel(gf, want[1]) < 1e-3
    assert abs(float(m["loss"]) - want[4]) < 1e-5 * want[4] and float(m["loss_distortion"]) > 0
    # the reference's rotation gradient at zero deltas is exactly zero, with the term as without
    assert int(torch.count_nonzero(gr)) == 0 and int(torch.count_nonzero(want[3])) == 0
    assert _rel(gt, truth[2]) < 2 * _rel(want[2], truth[2]) + 1e-3


# ------------------------------------------------------------------------------ CLI --
def _scene(root: Path, n_train=3, n_val=2, size=16):
    from PIL import Image
    poses = np.load(sorted(GOLDEN.glob("final_poses_*.npz"))[0])["ground_truth_poses"]
    rng = np.random.default_rng(0)
    for split, n in (("train", n_train), ("val", n_val)):
        (root / "lego" / split).mkdir(parents=True, exist_ok=True)
        frames = []
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "RGBA").save(
                root / "lego" / split / f"r_{i}.png")
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": poses[i].tolist()})
        (root / "lego" / f"transforms_{split}.json").write_text(
            json.dumps({"camera_angle_x": 0.6911112, "frames": frames}))


@pytest.mark.parametrize("module", ["train", "train_pose_opt"])
def test_cli_flag_reaches_the_step_the_saved_arguments_and_the_console_only(module, tmp_path, capsys):
    import importlib
    layout = json.loads((GOLDEN / "reference_artifacts.json").read_text())["layout"]
    _scene(tmp_path / "data")
    extra = ["--pose_opt_delay", "1", "--rotation_noise", "5", "--noise_seed", "42"] if module == "train_pose_opt" else []
    importlib.import_module("noisy_src." + module).main(
        ["--data_root", str(tmp_path / "data"), "--img_scale", "1.0", "--batch_size", "64", "--num_iters", "3",
         "--log_every", "1", "--num_samples", "8", "--num_samples_fine", "16", "--precision", "bf16",
         "--output_dir", str(tmp_path / "out"), "--distortion_weight", "0.01"] + extra)
    (run,) = (tmp_path / "out").iterdir()
    assert json.loads((run / "experiment_config.json").read_text())["distortion_weight"] == 0.01
    head = (run / "logs" / "train_metrics.csv").read_text().splitlines()[0]
    assert head == layout["pose_opt" if module == "train_pose_opt" else "train"]["csv_headers"]["train_metrics.csv"]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "loss:" in ln]
    assert len(lines) == 3 and all("| distortion: 0." in ln for ln in lines), lines


# ---------------------------------------------------------------------------- graph --
def test_graphed_trainer_with_distortion_equals_eager(tmp_path):
    """A fresh child (tests/distortion_graph_worker.py): three replays of a two-branch capture
    against three eager one-stream steps, losses and parameters bit for bit."""
    subprocess.run([sys.executable, str(ROOT / "tests" / "distortion_graph_worker.py"), str(tmp_path)], check=True,
                   timeout=300)
    r = json.loads((tmp_path / "distortion_graph_report.json").read_text())
    assert r["replays"] == 3 and r["two_branch_capture"], r
    assert r["losses_equal"] and r["params_equal"] and r["distortion_positive"], r
