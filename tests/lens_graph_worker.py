"""Worker of tests/test_lens.py::test_graphed_pose_trainer_with_a_lens_equals_eager:
``GraphedPoseTrainer`` over a ``PoseTrainer`` with a learned lens, in a process of its own.

Six steps (frozen, frozen, then four optimising; warmup=0: the first step of each shape runs
eagerly because its Adam state is new, the second is captured, the rest replay) against the
eager ``PoseTrainer`` on the same batches.  The focal length starts 5 % off in mode "xy", the
radial terms at a non-zero ``lens_init`` and the principal point at the centre; all of them
change on every optimising step, so the replays after the capture only match the eager steps
if the ray kernels read the six numbers from device memory rather than from the captured
launch, and a value baked in at capture would show.  ``GraphedPoseTrainer`` binds nothing for
the lens beyond ``intrinsics.parameters()``.
Writes ``<out>/lens_graph_report.json``.
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
LENS_INIT = (0.25, -0.05)


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
    intr = CameraIntrinsics(data.focal * 1.05, "xy", learn_principal=True, learn_distortion=True,
                            lens_init=LENS_INIT, image_size=(16, 16)).to(dev)
    return PoseTrainer(mc.to(dev), mf.to(dev), cam, sampler, rc, intrinsics=intr)


def _state(tr):
    params = torch.cat([tr.model_coarse.flat_params(), tr.model_fine.flat_params()]).cpu()
    poses = torch.cat([p.detach().reshape(-1).cpu() for p in tr.camera_params.parameters()])
    return params, poses, torch.cat([p.detach().reshape(-1).cpu() for p in tr.intrinsics.parameters()])


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
    start = tr_g.intrinsics.lens().detach().clone()
    le, lg, replays_after_update = [], [], 0
    for (batch, t_rand, u), opt in zip(data, SEQUENCE):
        m = eager.step(batch, optimize_poses=opt, t_rand=t_rand, u=u)
        le.append([float(m[k]) for k in LOSS_KEYS])
        replayed = opt in graphed._graphs
        moved = bool((tr_g.intrinsics.lens().detach() != start).all())
        m = graphed.step(batch, optimize_poses=opt, t_rand=t_rand, u=u)
        lg.append([float(m[k]) for k in LOSS_KEYS])
        replays_after_update += int(replayed and opt and moved)
    torch.cuda.synchronize()
    (pa, qa, fa), (pb, qb, fb) = _state(eager), _state(tr_g)
    rep = dict(captured=sorted(graphed._graphs), losses_equal=le == lg, params_equal=bool(torch.equal(pa, pb)),
               poses_equal=bool(torch.equal(qa, qb)), lens_params_equal=bool(torch.equal(fa, fb)),
               lens_params=fb.tolist(), n_lens_params=len(list(tr_g.intrinsics.parameters())),
               lens=tr_g.intrinsics.lens_values(), lens_start=start.tolist(),
               every_lens_entry_moved=bool((tr_g.intrinsics.lens().detach() != start).all()),
               replays_after_a_lens_update=replays_after_update)
    (out / "lens_graph_report.json").write_text(json.dumps(rep, indent=1))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
