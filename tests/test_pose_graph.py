"""GPU: the joint pose-optimisation step replayed from hipGraphs.

``nr_gather_pixels`` (the on-device ``PixelSampler.sample_batch``) against the reference's
index tables, ``engine.GraphedPoseTrainer`` (one graph for frozen poses, one for
optimising, captured lazily) against the eager ``PoseTrainer`` -- the replay runs the same
kernels in the same order, so everything is compared with ``torch.equal`` / ``==`` -- its
guards, ``python -m noisy_src.train_pose_opt --graph`` against the eager CLI, and the
capture of the data-parallel step over RCCL (tests/pose_graph_worker.py, world 1)."""
import ctypes
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"

# frozen / optimising steps interleaved: both graphs replay after each other
SEQUENCE = (False, False, True, True, True, False, True)


def _fixture_poses():
    z = np.load(sorted(GOLDEN.glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    return torch.from_numpy(z["ground_truth_poses"]), torch.from_numpy(z["initial_poses"])


# ------------------------------------------------------------ nr_gather_pixels --
N_IMG, H, W, B_GATHER = 3, 5, 7, 70


def _tables(images):
    """The reference's tables, by the torch expressions of its PixelDataset.__init__."""
    n_img, h, w = images.shape[:3]
    dev = images.device
    v, u = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev),
                          torch.arange(w, dtype=torch.float32, device=dev), indexing="ij")
    single = torch.stack([u.flatten(), v.flatten()], dim=-1)
    image_indices = torch.repeat_interleave(torch.arange(n_img, dtype=torch.long, device=dev), h * w)
    pixel_coords = single.unsqueeze(0).expand(n_img, -1, -1).reshape(-1, 2)
    return image_indices, pixel_coords, images.reshape(-1, 3)


@pytest.fixture(scope="module")
def small_scene():
    from noisy_src.data import synthetic_blender_data
    gt, _ = _fixture_poses()
    data = synthetic_blender_data(gt[:N_IMG], H=H, W=W, device=DEV)
    assert data.images.shape == (N_IMG, H, W, 3)
    n_pixels = N_IMG * H * W
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, n_pixels, (B_GATHER,), generator=g)
    idx[:8] = torch.tensor([0, H * W - 1, H * W, n_pixels - 1, 0, H * W, 17, 17])  # edges and repeats
    return data, idx.to(DEV), _tables(data.images)


def test_gather_pixels_matches_tables(small_scene):
    from noisy_src import ops
    data, idx, (t_img, t_pix, t_rgb) = small_scene
    img, pix, rgb = ops.gather_pixels(idx, data.images)
    assert img.dtype == torch.int64 and img.shape == (B_GATHER,)
    assert pix.shape == (B_GATHER, 2) and rgb.shape == (B_GATHER, 3)
    assert torch.equal(img, t_img[idx])
    assert torch.equal(pix, t_pix[idx])
    assert torch.equal(rgb, t_rgb[idx])


def test_gather_pixels_out_writes_in_place(small_scene):
    from noisy_src import ops
    data, idx, (t_img, t_pix, t_rgb) = small_scene
    out = (torch.full((B_GATHER,), -7, device=DEV, dtype=torch.int64),
           torch.full((B_GATHER, 2), -7.0, device=DEV), torch.full((B_GATHER, 3), -7.0, device=DEV))
    ptrs = [t.data_ptr() for t in out]
    got = ops.gather_pixels(idx, data.images, out=out)
    assert [t.data_ptr() for t in got] == ptrs
    assert all(a is b for a, b in zip(got, out))
    assert torch.equal(out[0], t_img[idx]) and torch.equal(out[1], t_pix[idx]) and torch.equal(out[2], t_rgb[idx])
    with pytest.raises(ValueError):
        ops.gather_pixels(idx, data.images, out=(out[0], out[1], out[2][:-1]))


def test_sample_batch_equals_table_gathers(small_scene):
    """Same RNG stream (one torch.randint) and the values of the three table gathers it
    replaces; the public table attributes still exist (built on first access)."""
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    data, _, (t_img, t_pix, t_rgb) = small_scene
    ds = PixelDataset(data)
    sampler = PixelSampler(ds, batch_size=B_GATHER)
    idx = torch.randint(0, ds.n_pixels, (B_GATHER,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    batch = sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(5))
    assert batch.in_range
    assert torch.equal(batch.image_indices, t_img[idx])
    assert torch.equal(batch.pixel_coords, t_pix[idx])
    assert torch.equal(batch.target_rgb, t_rgb[idx])
    out = [torch.empty(B_GATHER, device=DEV, dtype=torch.int64), torch.empty(B_GATHER, 2, device=DEV),
           torch.empty(B_GATHER, 3, device=DEV)]
    b2 = sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(5), out=out)
    assert b2.image_indices is out[0] and b2.pixel_coords is out[1] and b2.target_rgb is out[2]
    assert torch.equal(out[0], t_img[idx]) and torch.equal(out[1], t_pix[idx]) and torch.equal(out[2], t_rgb[idx])
    # the global RNG stream: one randint per batch, as before
    torch.manual_seed(9)
    want = torch.randint(0, ds.n_pixels, (B_GATHER,), device=DEV)
    after = torch.rand(3, device=DEV)
    torch.manual_seed(9)
    b3 = sampler.sample_batch()
    assert torch.equal(b3.target_rgb, t_rgb[want]) and torch.equal(torch.rand(3, device=DEV), after)
    assert torch.equal(ds.image_indices, t_img) and torch.equal(ds.pixel_coords, t_pix)
    assert torch.equal(ds.target_rgb, t_rgb)


@pytest.mark.parametrize("bad", [N_IMG * H * W, -1])
def test_gather_pixels_out_of_range(small_scene, bad):
    from noisy_src import ops
    data, idx, (t_img, t_pix, t_rgb) = small_scene
    i = idx.clone()
    i[3] = bad
    with pytest.raises(IndexError):
        ops.gather_pixels(i, data.images, validate=True)
    img, pix, rgb = ops.gather_pixels(i, data.images)  # unchecked: NaN row, image -1, the rest intact
    assert int(img[3]) == -1 and torch.isnan(pix[3]).all() and torch.isnan(rgb[3]).all()
    keep = torch.arange(B_GATHER, device=DEV) != 3
    assert torch.equal(img[keep], t_img[idx][keep]) and torch.equal(rgb[keep], t_rgb[idx][keep])
    ops.gather_pixels(idx, data.images, validate=True)  # in range: no error


# --------------------------------------------------------- GraphedPoseTrainer --
def _fresh_pack(net):
    """nr_mlp_pack of the current parameters over a copy of the images (so the alignment
    gaps nr_mlp_pack never writes compare equal)."""
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    out = net._packed.clone()
    call("nr_mlp_pack", ctypes.byref(net._nr_cfg), ptr(net._flat), ptr(out), _hip.stream_ptr())
    return out


def _rot0():
    """Live rotation deltas (theta ~ 0.05 rad) for the 3 views."""
    return 0.05 * torch.randn(3, 3, generator=torch.Generator().manual_seed(23))


def _pose_trainer(precision, rc, batch_size=128, seed=17, start="zero"):
    """3 views of 16 x 16, the fixture's noisy initial poses as the learnable ones.  ``start``:
    "zero" deltas (the reference's start: the rotation gradient is exactly 0 for ever),
    "rot0" (rotation deltas from ``_rot0``) or "fixed_small_angle" (zero deltas, the opt-in
    exact derivative at w = 0) -- the last two train the rotations."""
    from noisy_src.config import ModelConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters
    gt, init = _fixture_poses()
    data = synthetic_blender_data(gt[:3], H=16, W=16, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=batch_size)
    torch.manual_seed(seed)
    mc, mf = create_nerf(ModelConfig(precision=precision))
    cam = CameraPoseParameters(init[:3].to(DEV), fixed_small_angle=start == "fixed_small_angle")
    if start == "rot0":
        with torch.no_grad():
            cam.rotation_deltas.copy_(_rot0().to(DEV))
    return PoseTrainer(mc.to(DEV), mf.to(DEV), cam, sampler, rc)


def _batches(trainer, rc, n, B=128, randoms=True):
    out = []
    for k in range(n):
        batch = trainer.pixel_sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(300 + k))
        g = torch.Generator().manual_seed(400 + k)
        tr = torch.rand(B, rc.num_samples, generator=g).to(DEV) if randoms else None
        u = torch.rand(B, rc.num_samples_fine, generator=g).to(DEV) if randoms else None
        out.append((batch, tr, u))
    return out


LOSS_KEYS = ("loss", "loss_coarse", "loss_fine")


def _run(step, batches):
    """The losses of every step, read before the next replay overwrites them."""
    losses = []
    for (batch, tr, u), opt in zip(batches, SEQUENCE):
        m = step(batch, optimize_poses=opt, t_rand=tr, u=u)
        losses.append([float(m[k]) for k in LOSS_KEYS])
    return losses


@pytest.mark.parametrize("precision,start", [
    pytest.param("fp32", "zero", id="fp32"), pytest.param("bf16", "zero", id="bf16"),
    pytest.param("fp32", "rot0", id="fp32-rot0"), pytest.param("bf16", "rot0", id="bf16-rot0"),
    pytest.param("fp32", "fixed_small_angle", id="fp32-fixed_small_angle"),
    pytest.param("bf16", "fixed_small_angle", id="bf16-fixed_small_angle")])
def test_graphed_pose_trainer_equals_eager(precision, start):
    """Frozen and optimising replays interleaved (F F O O O F O; warmup=1: the first step of
    each shape is eager, the second is captured) equal the eager PoseTrainer: losses,
    parameters, packed images, poses, LR, Adam counters and moments, bit for bit.  From
    zero deltas the rotation gradient is exactly 0 on both sides; from ``rot0`` and with
    ``fixed_small_angle`` it is live, so a replay that failed to zero or re-read a buffer of
    the rotation-gradient chain would differ, and the rotations must have moved."""
    from noisy_src.config import RenderConfig
    from noisy_src.engine import GraphedPoseTrainer
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    eager, tr_g = _pose_trainer(precision, rc, start=start), _pose_trainer(precision, rc, start=start)
    assert torch.equal(eager.model_fine.flat_params(), tr_g.model_fine.flat_params())
    batches = _batches(eager, rc, len(SEQUENCE))
    le = _run(eager.step, batches)
    graphed = GraphedPoseTrainer(tr_g, *batches[0], warmup=1)
    lg = _run(graphed.step, batches)
    assert sorted(graphed._graphs) == [False, True]  # both shapes were captured
    for k, (a, b) in enumerate(zip(le, lg)):
        assert a == b, (k, a, b)
    for na, nb in ((eager.model_coarse, tr_g.model_coarse), (eager.model_fine, tr_g.model_fine)):
        assert torch.equal(na.flat_params(), nb.flat_params())
        assert torch.equal(nb._packed, _fresh_pack(nb))
    ca, cb = eager.camera_params, tr_g.camera_params
    assert torch.equal(ca.rotation_deltas.detach(), cb.rotation_deltas.detach())
    assert torch.equal(ca.translation_deltas.detach(), cb.translation_deltas.detach())
    assert cb.translation_deltas.detach().abs().max() > 0
    rot_start = _rot0().to(DEV) if start == "rot0" else torch.zeros(3, 3, device=DEV)
    if start == "zero":
        assert torch.equal(cb.rotation_deltas.detach(), rot_start)  # the reference's quirk
    else:
        assert (cb.rotation_deltas.detach() - rot_start).abs().amax(dim=1).min() > 1e-5  # every view's rotation moved
    n_opt = sum(SEQUENCE)
    for oa, ob, steps in ((eager.optimizer_nerf, tr_g.optimizer_nerf, len(SEQUENCE)),
                          (eager.optimizer_poses, tr_g.optimizer_poses, n_opt)):
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
        for pa, pb in zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"]):
            assert int(oa.state[pa]["step"]) == int(ob.state[pb]["step"]) == steps
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
    assert eager.scheduler_poses.last_epoch == tr_g.scheduler_poses.last_epoch == n_opt
    assert tr_g.optimizer_nerf.device_sched is None and tr_g.optimizer_poses.device_sched is None


def test_graphed_pose_trainer_draws_the_eager_randoms():
    """Without injected randoms the jitter and inverse-CDF uniforms are drawn by torch.rand
    into the static buffers before each step, in the eager step's order: from the same
    seed both train identically."""
    from noisy_src.config import RenderConfig
    from noisy_src.engine import GraphedPoseTrainer
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    eager, tr_g = _pose_trainer("bf16", rc), _pose_trainer("bf16", rc)
    batches = _batches(eager, rc, len(SEQUENCE), randoms=False)
    torch.manual_seed(77)
    le = _run(eager.step, batches)
    torch.manual_seed(77)
    graphed = GraphedPoseTrainer(tr_g, batches[0][0], warmup=1)
    lg = _run(graphed.step, batches)
    assert sorted(graphed._graphs) == [False, True]
    assert le == lg, (le, lg)
    assert torch.equal(eager.model_fine.flat_params(), tr_g.model_fine.flat_params())


def test_graphed_pose_trainer_guards():
    """An unvalidated batch is refused before any capture (the validating kernel's flag is
    read on the host), and a replay after the pose Adam's state was replaced raises."""
    from noisy_src.config import RenderConfig
    from noisy_src.data_pose_opt import PixelBatch
    from noisy_src.engine import GraphedPoseTrainer
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    tr = _pose_trainer("bf16", rc)
    (batch, t_rand, u), = _batches(tr, rc, 1)
    unchecked = PixelBatch(batch.image_indices, batch.pixel_coords, batch.target_rgb)
    assert not unchecked.in_range
    with pytest.raises(ValueError, match="in_range"):
        GraphedPoseTrainer(tr, unchecked, t_rand, u)
    graphed = GraphedPoseTrainer(tr, batch, t_rand, u, warmup=0)
    with pytest.raises(ValueError, match="in_range"):
        graphed.step(unchecked, optimize_poses=True, t_rand=t_rand, u=u)
    assert not graphed._graphs
    graphed.step(batch, optimize_poses=True, t_rand=t_rand, u=u)  # eager: creates the Adam state
    assert not graphed._graphs
    graphed.step(batch, optimize_poses=True, t_rand=t_rand, u=u)  # captured and replayed
    assert list(graphed._graphs) == [True]
    tr.optimizer_poses.load_state_dict(tr.optimizer_poses.state_dict())
    with pytest.raises(RuntimeError, match="replaced"):
        graphed.step(batch, optimize_poses=True, t_rand=t_rand, u=u)


# ------------------------------------------------------------------------ CLI --
def _scene(root: Path, n_train=3, n_val=2, size=16):
    from PIL import Image
    poses = np.load(sorted(GOLDEN.glob("final_poses_*.npz"))[0])["ground_truth_poses"]
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


def test_train_pose_opt_cli_graph_matches_eager(tmp_path):
    """``--graph``: iteration 0 eager, the frozen graph from iteration 1, iteration 3 (the
    first optimising one) eager, the optimising graph from iteration 4, validation
    mid-way.  Logged losses, weights, poses, Adam moments and final_poses.pt equal the
    eager run's bit for bit."""
    from noisy_src.train_pose_opt import main
    _scene(tmp_path / "data")
    cks, rows, finals = {}, {}, {}
    for name, extra in (("e", []), ("g", ["--graph"])):
        main(["--data_root", str(tmp_path / "data"), "--img_scale", "1.0", "--batch_size", "128", "--num_iters", "8",
              "--pose_opt_delay", "3", "--val_every", "4", "--rotation_noise", "5", "--translation_noise_pct", "5",
              "--noise_seed", "42", "--precision", "bf16", "--output_dir", str(tmp_path / name)] + extra)
        runs = list((tmp_path / name).iterdir())
        assert len(runs) == 1
        cks[name] = torch.load(runs[0] / "checkpoint_latest.pt", weights_only=True, map_location="cpu")
        rows[name] = [r.split(",")[:3] for r in (runs[0] / "logs" / "train_metrics.csv").read_text().splitlines()]
        finals[name] = torch.load(runs[0] / "final_poses.pt", weights_only=True)
    assert len(rows["g"]) == 9 and rows["g"] == rows["e"]
    for part in ("model_coarse", "model_fine", "camera_params"):
        assert list(cks["e"][part]) == list(cks["g"][part])
        for k, v in cks["e"][part].items():
            assert torch.equal(v, cks["g"][part][k]), (part, k)
    for opt in ("optimizer_nerf", "optimizer_poses"):
        assert len(cks["e"][opt]["state"]) > 0
        for k, v in cks["e"][opt]["state"].items():
            assert torch.equal(v["exp_avg"], cks["g"][opt]["state"][k]["exp_avg"]), (opt, k)
            assert float(v["step"]) == float(cks["g"][opt]["state"][k]["step"]), (opt, k)
    for k in ("initial_poses", "optimized_poses", "ground_truth_poses"):
        assert torch.equal(finals["e"][k], finals["g"][k]), k
    assert finals["e"]["pose_errors"] == finals["g"]["pose_errors"]
    assert (finals["g"]["optimized_poses"] - finals["g"]["initial_poses"]).abs().max() > 0


# ------------------------------------------------------------------ DP capture --
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_rccl_graphed_pose_step(tmp_path):
    """One fresh child in a world-1 RCCL group: the network all-reduces and the
    pose-gradient all-reduce are captured; 4 steps equal the plain PoseTrainer's."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
                    "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                    str(ROOT / "tests" / "pose_graph_worker.py"), str(tmp_path)], check=True, env=env, timeout=300)
    r = json.loads((tmp_path / "pose_graph_report.json").read_text())
    assert r["backend"] == "nccl" and r["world"] == 1
    assert r["captured"] == [False, True], r
    assert r["poses_moved"] > 0
    assert r["losses_equal"] and r["params_equal"] and r["poses_equal"], r
