"""Worker of tests/test_pe_window.py::test_graph_replay_with_a_moving_window: the joint
pose-optimisation step replayed from hipGraphs while the coarse-to-fine window changes at
every step.

Three ``PoseTrainer`` of the same seed (the sizes of tests/pose_graph_worker.py: 3 views of
16 x 16, 128 rays, 32 + 32 samples, bf16; ``fixed_small_angle=True`` so the rotation
gradients are live) run 8 steps, frozen and optimising interleaved: one eager with a
schedule, one through ``GraphedPoseTrainer`` with the same schedule (warmup=1: the first step
of each shape is eager, the second is captured, the rest replay), one eager without a window.
The graphed run must equal the eager one bit for bit -- losses, parameters, poses, and an
inference forward after the last replay (the replayed Adam rewrote the images unfolded
without the host seeing it) -- and differ from the run without a window.
Writes ``<out>/pe_window_graph_report.json``.
"""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEQUENCE = (False, False, False, True, True, True, False, True)
B = 128
DEV = "cuda"


def _schedule(iteration, num_freqs):
    from noisy_src.train_pose_opt import c2f_alpha, pe_window_weights
    # a new window at every one of the 8 steps, with ones, a fractional weight and zeros
    return pe_window_weights(c2f_alpha(iteration + 1, 12, 0.0, 1.0, num_freqs), num_freqs)


def _trainer(rc, schedule):
    from noisy_src.config import ModelConfig
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    from noisy_src.engine import PoseTrainer
    from noisy_src.model import create_nerf
    from noisy_src.train_pose_opt import CameraPoseParameters
    z = np.load(sorted((ROOT / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    data = synthetic_blender_data(torch.from_numpy(z["ground_truth_poses"])[:3], H=16, W=16, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=B)
    torch.manual_seed(42)
    mc, mf = create_nerf(ModelConfig(precision="bf16"))
    cam = CameraPoseParameters(torch.from_numpy(z["initial_poses"])[:3].to(DEV), fixed_small_angle=True)
    return PoseTrainer(mc.to(DEV), mf.to(DEV), cam, sampler, rc, pe_schedule=schedule)


def _state(tr):
    params = torch.cat([tr.model_coarse.flat_params(), tr.model_fine.flat_params()]).cpu()
    poses = torch.cat([p.detach().reshape(-1).cpu() for p in tr.camera_params.parameters()])
    return params, poses


def _eval(tr):
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(300, 3, generator=g) * 3 - 1.5).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=-1).to(DEV)
    with torch.no_grad():
        return torch.cat([torch.cat(net(x, d), dim=-1) for net in (tr.model_coarse, tr.model_fine)]).cpu()


def main():
    from noisy_src.config import RenderConfig
    from noisy_src.engine import GraphedPoseTrainer
    out = Path(sys.argv[1])
    rc = RenderConfig(num_samples=32, num_samples_fine=32)
    eager, tr_g, plain = _trainer(rc, _schedule), _trainer(rc, _schedule), _trainer(rc, None)
    data = []
    for k in range(len(SEQUENCE)):
        g = torch.Generator().manual_seed(500 + k)
        data.append((eager.pixel_sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(600 + k)),
                     torch.rand(B, rc.num_samples, generator=g).to(DEV),
                     torch.rand(B, rc.num_samples_fine, generator=g).to(DEV)))
    graphed = GraphedPoseTrainer(tr_g, *data[0], warmup=1)
    le, lg, windows, replays = [], [], set(), 0
    for k, ((batch, t_rand, u), opt) in enumerate(zip(data, SEQUENCE)):
        le.append(float(eager.step(batch, optimize_poses=opt, t_rand=t_rand, u=u, iteration=k)["loss"]))
        lg.append(float(graphed.step(batch, optimize_poses=opt, t_rand=t_rand, u=u, iteration=k)["loss"]))
        plain.step(batch, optimize_poses=opt, t_rand=t_rand, u=u, iteration=k)
        replays += opt in graphed._graphs
        windows.add(tuple(tr_g.model_fine.pe_window()[0]))
        assert tr_g.model_fine.pe_window() == eager.model_fine.pe_window()
    torch.cuda.synchronize()
    (pa, qa), (pb, qb), (pc, _) = _state(eager), _state(tr_g), _state(plain)
    rep = dict(captured=sorted(graphed._graphs), replays=replays, windows_distinct=len(windows),
               losses_equal=le == lg, params_equal=bool(torch.equal(pa, pb)), poses_equal=bool(torch.equal(qa, qb)),
               eval_equal=bool(torch.equal(_eval(eager), _eval(tr_g))),
               rotations_moved=float(tr_g.camera_params.rotation_deltas.detach().abs().max()),
               differs_from_no_window=not torch.equal(pa, pc), losses=[le, lg])
    (out / "pe_window_graph_report.json").write_text(json.dumps(rep, indent=1))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
