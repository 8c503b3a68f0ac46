"""Worker of tests/test_pose_graph.py::test_rccl_graphed_pose_step: the data-parallel
joint pose-optimisation step captured into hipGraphs over RCCL on one MI355X.

Run as ``torch.distributed.run --nproc-per-node=1`` (world 1): the process joins a
backend-"nccl" (= RCCL) group before anything touches the GPU.  A ``GraphedPoseTrainer``
of a ``PoseTrainer`` built with the process group (the two network all-reduces and the
pose-gradient all-reduce are captured inside the graphs) must leave the same parameters
and poses after 4 steps (frozen, frozen, optimising, optimising: the second of each
shape is the captured one) as a plain ``PoseTrainer`` without a group: at world 1 the SUM
is the identity and the backward seed's 1/world is 1.
Writes ``<out>/pose_graph_report.json``.
"""

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SEQUENCE = (False, False, True, True)
B = 128


def _trainer(rc, dev, group):
    from noisy_src.config import ModelConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters
    z = np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"])[:3], H=16, W=16, device=dev)
    sampler = PixelSampler(PixelDataset(data), batch_size=B)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision="bf16"))
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(dev))
    return PoseTrainer(mc.to(dev), mf.to(dev), cam, sampler, rc, process_group=group)


def _state(tr):
    params = torch.cat([tr.model_coarse.flat_params(), tr.model_fine.flat_params()]).cpu()
    poses = torch.cat([p.detach().reshape(-1).cpu() for p in tr.camera_params.parameters()])
    return params, poses


def main():
    from noisy_src.config import RenderConfig
    from noisy_src.engine import GraphedPoseTrainer
    out = Path(sys.argv[1])
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group("nccl", device_id=dev)  # before any other GPU work
    torch.cuda.set_device(dev)
    pg = dist.group.WORLD
    rep = {"world": dist.get_world_size(pg), "backend": dist.get_backend(pg)}
    t = torch.ones(4, device=dev)
    dist.all_reduce(t)  # RCCL initialises its communicator on the first collective
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    plain, dp = _trainer(rc, dev, None), _trainer(rc, dev, pg)
    data = []
    for k in range(len(SEQUENCE)):
        g = torch.Generator().manual_seed(500 + k)
        data.append((plain.pixel_sampler.sample_batch(generator=torch.Generator(device=dev).manual_seed(600 + k)),
                     torch.rand(B, rc.num_samples, generator=g).to(dev),
                     torch.rand(B, rc.num_samples_fine, generator=g).to(dev)))
    graphed = GraphedPoseTrainer(dp, *data[0], warmup=0)
    lp, lg = [], []
    for (batch, t_rand, u), opt in zip(data, SEQUENCE):
        lp.append(float(plain.step(batch, optimize_poses=opt, t_rand=t_rand, u=u)["loss"]))
        lg.append(float(graphed.step(batch, optimize_poses=opt, t_rand=t_rand, u=u)["loss"]))
    torch.cuda.synchronize()
    (pa, qa), (pb, qb) = _state(plain), _state(dp)
    rep.update(captured=sorted(graphed._graphs), losses_equal=lp == lg, params_equal=bool(torch.equal(pa, pb)),
               poses_equal=bool(torch.equal(qa, qb)), poses_moved=float(qb.abs().max()))
    (out / "pose_graph_report.json").write_text(json.dumps(rep, indent=1))
    print(json.dumps(rep))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
