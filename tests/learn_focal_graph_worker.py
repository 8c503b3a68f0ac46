"""Worker of tests/test_learn_focal.py::test_graphed_pose_trainer_with_intrinsics_equals_eager:
``GraphedPoseTrainer`` over a ``PoseTrainer`` with learned intrinsics, in a process of its own.

Six steps (frozen, frozen, then four optimising; warmup=0: the first step of each shape runs
eagerly because its Adam state is new, the second is captured, the rest replay) against the
eager ``PoseTrainer`` on the same batches.  The focal length starts 5 % off in mode "xy" and
changes on every optimising step, so the replays after the capture only match the eager steps
if the ray kernels read (fx, fy) from device memory rather than from the captured launch.
Writes ``<out>/learn_focal_graph_report.json``.
"""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEQUENCE = (False, False, True, True, True, True)
B = 64
LOSS_KEYS = ("loss", "loss_coarse", "loss_fine")


def _trainer(rc, dev):
    from noisy_src.config import ModelConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraIntrinsics, CameraPoseParameters
    z = np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"])[:3], H=16, W=16, device=dev)
    sampler = PixelSampler(PixelDataset(data), batch_size=B)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision="bf16"))
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(dev), fixed_small_angle=True)
    intr = CameraIntrinsics(data.focal * 1.05, "xy").to(dev)
    return PoseTrainer(mc.to(dev), mf.to(dev), cam, sampler, rc, intrinsics=intr)


def _state(tr):
    params = torch.cat([tr.model_coarse.flat_params(), tr.model_fine.flat_params()]).cpu()
    poses = torch.cat([p.detach().reshape(-1).cpu() for p in tr.camera_params.parameters()])
    return params, poses, tr.intrinsics.log_scale.detach().cpu()


def main():
    from noisy_src.config import RenderConfig
    from noisy_src.engine import GraphedPoseTrainer
    out = Path(sys.argv[1])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rc = RenderConfig(num_samples=16, num_samples_fine=32)
    eager, tr_g = _trainer(rc, dev), _trainer(rc, dev)
    data = []
    for k in range(len(SEQUENCE)):
        g = torch.Generator().manual_seed(500 + k)
        data.append((eager.pixel_sampler.sample_batch(generator=torch.Generator(device=dev).manual_seed(600 + k)),
                     torch.rand(B, rc.num_samples, generator=g).to(dev),
                     torch.rand(B, rc.num_samples_fine, generator=g).to(dev)))
    graphed = GraphedPoseTrainer(tr_g, *data[0], warmup=0)
    le, lg, replays_after_update = [], [], 0
    for (batch, t_rand, u), opt in zip(data, SEQUENCE):
        m = eager.step(batch, optimize_poses=opt, t_rand=t_rand, u=u)
        le.append([float(m[k]) for k in LOSS_KEYS])
        replayed = opt in graphed._graphs
        moved = bool(tr_g.intrinsics.log_scale.detach().abs().max() > 0)
        m = graphed.step(batch, optimize_poses=opt, t_rand=t_rand, u=u)
        lg.append([float(m[k]) for k in LOSS_KEYS])
        replays_after_update += int(replayed and opt and moved)
    torch.cuda.synchronize()
    (pa, qa, fa), (pb, qb, fb) = _state(eager), _state(tr_g)
    rep = dict(captured=sorted(graphed._graphs), losses_equal=le == lg, params_equal=bool(torch.equal(pa, pb)),
               poses_equal=bool(torch.equal(qa, qb)), log_scale_equal=bool(torch.equal(fa, fb)),
               log_scale=fb.tolist(), log_scale_moved=float(fb.abs().min()),
               replays_after_a_focal_update=replays_after_update)
    (out / "learn_focal_graph_report.json").write_text(json.dumps(rep, indent=1))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
