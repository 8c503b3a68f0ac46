"""GPU: frozen-field pose refinement (engine.PoseRefiner) and its use by
inference.evaluate_test_set, on the scene of pose_refine_scene.py in fp32.

* One ``PoseRefiner.step`` leaves the pose gradients ``PoseTrainer.step`` leaves on the same
  batch, networks and injected uniforms, bit for bit (the trainer with its regulariser
  weights at 0: the refiner has none): downstream of the MLP's input gradients, which the
  frozen kernels reproduce exactly, the kernels and their inputs are the same.  The
  networks come out unchanged and without gradients, and get their requires_grad back.
* The 100 fixed steps of the scene: the fp64 oracle halves both mean pose errors
  (test_pose_refine_host.py); fp32 kernels and the fused fp32 Adam need not follow its
  trajectory, so the device is asked for a decrease of both, and of the loss.
* ``evaluate_test_set`` with refinement writes the new JSON keys; without the flags its JSON
  key sets are those it had before."""
import copy
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_refine_scene as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _sampler(scene):
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    ds = PixelDataset(SimpleNamespace(H=S.H, W=S.W, focal=S.FOCAL, images=scene.images.float().to(DEV)))
    return PixelSampler(ds, batch_size=S.N_RAYS)


def _batch(b):
    from noisy_src.data_pose_opt import PixelBatch
    img, pix, target, _, u = b
    return PixelBatch(img.to(DEV), pix.float().to(DEV), target.float().to(DEV)), u.float().to(DEV)


def _camera(scene):
    from noisy_src.train_pose_opt import CameraPoseParameters
    return CameraPoseParameters(scene.init_poses.float().to(DEV), fixed_small_angle=True).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


def test_refiner_needs_the_small_angle_jacobian(scene):
    from noisy_src.engine import PoseRefiner
    from noisy_src.train_pose_opt import CameraPoseParameters
    coarse, fine = _device_nets(scene)
    cam = CameraPoseParameters(scene.init_poses.float().to(DEV)).to(DEV)
    with pytest.raises(ValueError, match="fixed_small_angle"):
        PoseRefiner(coarse, fine, cam, _sampler(scene), scene.rc)
    assert all(p.requires_grad for p in coarse.parameters())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_refiner_step_leaves_the_trainer_steps_pose_gradients(scene, precision):
    from noisy_src.engine import PoseRefiner, PoseTrainer
    coarse, fine = _device_nets(scene, precision)
    sampler = _sampler(scene)
    batch, u = _batch(scene.batches[0])

    cam_t = _camera(scene)
    trainer = PoseTrainer(copy.deepcopy(coarse), copy.deepcopy(fine), cam_t, sampler, scene.rc,
                          rotation_reg_weight=0.0, translation_reg_weight=0.0)
    trainer.step(batch, optimize_poses=True, u=u)
    want = (cam_t.rotation_deltas.grad.clone(), cam_t.translation_deltas.grad.clone())

    before = [p.detach().clone() for p in list(coarse.parameters()) + list(fine.parameters())]
    gflat = (coarse._last_gflat, fine._last_gflat)
    cam_r = _camera(scene)
    with PoseRefiner(coarse, fine, cam_r, sampler, scene.rc, pose_lr=S.POSE_LR, max_norm=S.MAX_NORM) as refiner:
        assert not any(p.requires_grad for p in list(coarse.parameters()) + list(fine.parameters()))
        m = refiner.step(batch, u=u)
        got = (cam_r.rotation_deltas.grad.clone(), cam_r.translation_deltas.grad.clone())
    torch.cuda.synchronize()
    assert torch.isfinite(m["loss"]) and m["loss"].is_cuda
    for name, g, w in zip(("rotation", "translation"), got, want):
        assert w.abs().max() > 0, name
        assert torch.equal(_bits(g), _bits(w)), (name, (g - w).abs().max().item())
    after = list(coarse.parameters()) + list(fine.parameters())
    for p, b in zip(after, before):
        assert torch.equal(_bits(p), _bits(b)) and p.grad is None
        assert p.requires_grad, "close() gives requires_grad back"
    assert coarse._last_gflat is gflat[0] and fine._last_gflat is gflat[1]
    # the step moved the poses
    assert cam_r.rotation_deltas.abs().max() > 0 and cam_r.translation_deltas.abs().max() > 0


def test_refinement_reduces_pose_errors_on_the_device(scene):
    from noisy_src.engine import PoseRefiner
    coarse, fine = _device_nets(scene)
    cam = _camera(scene)
    sampler = _sampler(scene)
    r0, t0 = S.mean_errors(scene.init_poses, scene.gt_poses)
    losses = []
    with PoseRefiner(coarse, fine, cam, sampler, scene.rc, pose_lr=S.POSE_LR, max_norm=S.MAX_NORM) as refiner:
        for b in scene.batches:
            batch, u = _batch(b)
            losses.append(refiner.step(batch, u=u)["loss"])
    losses = torch.stack(losses).cpu()
    with torch.no_grad():
        r1, t1 = S.mean_errors(cam.get_all_poses(), scene.gt_poses)
    print(f"POSE_REFINE_DEVICE rot {r0:.4f} -> {r1:.4f} deg, trans {t0:.5f} -> {t1:.5f}, "
          f"loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert r1 < r0, (r0, r1)
    assert t1 < t0, (t0, t1)
    assert losses[-1] < losses[0]


TODAY_PER_IMAGE = {"image", "psnr", "ssim", "mse", "render_time"}
TODAY_NOISE = {"noise_rotation_error_deg", "noise_translation_error"}
TODAY_SUMMARY = {"psnr_mean", "psnr_std", "ssim_mean", "ssim_std", "mse_mean", "mse_std", "n_images"}
NEW_PER_IMAGE = {"pose_rotation_error_deg_before", "pose_rotation_error_deg_after", "pose_translation_error_before",
                 "pose_translation_error_after"}


def test_evaluate_test_set_with_and_without_refinement(scene, tmp_path):
    from noisy_src.inference import evaluate_test_set
    from noisy_src.noise import NoiseConfig
    from noisy_src.rendering import NeRFRenderer
    coarse, fine = _device_nets(scene)
    renderer = NeRFRenderer(coarse, fine, scene.rc)
    data = SimpleNamespace(images=scene.images[:2].float().to(DEV), poses=scene.gt_poses[:2].float().to(DEV), H=S.H,
                           W=S.W, focal=S.FOCAL)
    noise = NoiseConfig(rotation_noise_deg=0.5, translation_noise=0.02, seed=1)
    quiet = lambda *a, **k: None  # noqa: E731

    plain = evaluate_test_set(renderer, data, tmp_path / "plain", noise, DEV, chunk_size=256, save_images=False, log=quiet)
    per = json.loads((tmp_path / "plain" / "per_image_metrics.json").read_text())
    summ = json.loads((tmp_path / "plain" / "test_metrics.json").read_text())
    assert len(per) == 2
    for rec in per:
        keys = set(rec) - {"lpips"}
        assert TODAY_PER_IMAGE <= keys and TODAY_NOISE <= keys
        assert all(k in TODAY_PER_IMAGE or k.startswith("noise_") for k in keys), keys
    assert set(summ) - {"lpips_mean", "lpips_std"} == TODAY_SUMMARY | {"noise_config", "actual_noise"}
    assert set(plain) == set(summ)

    got = evaluate_test_set(renderer, data, tmp_path / "refined", noise, DEV, chunk_size=256, save_images=False,
                            log=quiet, refine_iters=5, refine_lr=1e-3, refine_rays_per_view=64, refine_seed=3)
    per_r = json.loads((tmp_path / "refined" / "per_image_metrics.json").read_text())
    summ_r = json.loads((tmp_path / "refined" / "test_metrics.json").read_text())
    for rec, base in zip(per_r, per):
        assert set(rec) == set(base) | NEW_PER_IMAGE
        assert abs(rec["pose_rotation_error_deg_before"] - base["noise_rotation_error_deg"]) < 1e-3
        assert rec["pose_rotation_error_deg_after"] != rec["pose_rotation_error_deg_before"]
    assert set(summ_r) == set(summ) | {"pose_refinement"}
    block = summ_r["pose_refinement"]
    assert block["iters"] == 5 and block["rays_per_view"] == 64 and block["seed"] == 3 and block["lr"] == 1e-3
    assert block["views_per_group"] == 4 and block["aligned_train_poses"] is False and block["sim3"] is None
    for k in NEW_PER_IMAGE:
        assert f"{k}_mean" in block
    assert got["pose_refinement"] == block
    # the networks were frozen only for the refinement
    assert all(p.requires_grad for p in coarse.parameters())

    # alignment alone: the gauge of the "train" poses is undone for the test poses
    from noisy_src import pose_eval as pe
    known = pe.Sim3(1.25, torch.linalg.matrix_exp(S.skew(torch.tensor([0.1, -0.2, 0.3], dtype=S.F64))),
                    torch.tensor([0.2, 0.1, -0.3], dtype=S.F64))
    learned = pe.to_learned_frame(known, scene.gt_poses)
    clean = NoiseConfig(rotation_noise_deg=0.0, translation_noise=0.0, seed=None)
    evaluate_test_set(renderer, data, tmp_path / "aligned", clean, DEV, chunk_size=256, save_images=False, log=quiet,
                      align_train_poses=(learned, scene.gt_poses))
    summ_a = json.loads((tmp_path / "aligned" / "test_metrics.json").read_text())
    assert abs(summ_a["pose_refinement"]["sim3"]["s"] - 1.25) < 1e-6
    assert summ_a["pose_refinement"]["pose_rotation_error_deg_before_mean"] < 1e-3
