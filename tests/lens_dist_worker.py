"""Worker of tests/test_lens.py::test_two_ranks_match_one_process_with_a_lens: the data-parallel
joint pose step with a learned lens.

Every rank builds the same networks (seed 42), poses and ``CameraIntrinsics`` (mode "xy", 5 %
off, principal point and radial terms learned from a non-zero ``lens_init``), takes its
contiguous slice of one global batch and runs ``engine.PoseTrainer.step``, whose pose-gradient
all-reduce carries the lens gradient (log_scale, principal, radial) in its last six entries.  Rank r
uses GPU r when there is one, else GPU 0 (always GPU 0 with LENS_DIST_SHARE_GPU=1); the collective is gloo over device tensors, as in
tests/dist_train_worker.py (the launch / finish path is the one RCCL takes).
Writes ``<out>/lens_rank<r>_of<world>.pt``: the final network parameters, poses and lens
parameters, and the (all-reduced) pose + lens gradient right before every pose Adam step.
"""

import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

B = 128


def main():
    out, steps = Path(sys.argv[1]), int(sys.argv[2])
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    share = os.environ.get("LENS_DIST_SHARE_GPU") == "1"  # both ranks on GPU 0
    dev = torch.device("cuda", 0 if share else rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    pg = None
    if world > 1:
        dist.init_process_group("gloo")
        pg = dist.group.WORLD
    from noisy_src.config import ModelConfig, RenderConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraIntrinsics, CameraPoseParameters

    z = np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"])[:3], H=16, W=16, device=dev)
    sampler = PixelSampler(PixelDataset(data), batch_size=B)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision="fp32"))
    mc, mf = mc.to(dev), mf.to(dev)
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(dev), fixed_small_angle=True)
    intr = CameraIntrinsics(data.focal * 1.05, "xy", learn_principal=True, learn_distortion=True,
                            lens_init=(0.25, -0.05), image_size=(16, 16)).to(dev)
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    trainer = PoseTrainer(mc, mf, cam, sampler, rc, process_group=pg, intrinsics=intr)
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    grads = []
    orig = trainer.optimizer_poses.step

    def capture(*a, **k):  # the (all-reduced) pose and lens gradients right before the pose Adam
        grads.append(torch.cat([p.grad.reshape(-1) for p in list(cam.parameters()) + list(intr.parameters())]).cpu())
        return orig(*a, **k)

    trainer.optimizer_poses.step = capture
    for k in range(steps):
        g = torch.Generator().manual_seed(900 + k)
        tr = torch.rand(B, rc.num_samples, generator=g).to(dev)
        u = torch.rand(B, rc.num_samples_fine, generator=g).to(dev)
        batch = sampler.sample_batch(generator=torch.Generator(device=dev).manual_seed(700 + k))
        trainer.step(batch.slice(sl), optimize_poses=True, t_rand=tr[sl], u=u[sl])
    torch.cuda.synchronize()
    torch.save({"nets": torch.cat([mc.flat_params().cpu(), mf.flat_params().cpu()]),
                "poses": torch.cat([p.detach().reshape(-1).cpu() for p in cam.parameters()]),
                "lens_params": torch.cat([p.detach().reshape(-1).cpu() for p in intr.parameters()]),
                "lens": intr.lens().detach().cpu(), "pose_grads": torch.stack(grads)},
               out / f"lens_rank{rank}_of{world}.pt")
    if pg is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
