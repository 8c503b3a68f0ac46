"""One SHA-256 per parameter and per logged loss after three training steps of every trainer,
from a fixed seed, with ``noisy_src`` imported from the checkout that ``--tree`` names.

    python tools/loss_fold_step_bits.py --tree /path/to/parent > parent.txt
    python tools/loss_fold_step_bits.py --tree . > tree.txt && diff parent.txt tree.txt

A refactor of the loss path (ops.py, rendering.py, engine.py) changes no line.  Cases:
``Trainer`` on one stream, ``Trainer(coarse_stream=True)``, ``GraphedTrainer`` (around a
``coarse_stream="auto"`` trainer: one eager step, a capture with one warm-up step, three
replays), ``PoseTrainer`` optimising its poses and ``PoseRefiner``, each with ``loss`` "mse"
and "cauchy" (scale 0.1) and ``distortion_weight`` 0 and 0.01 (the refiner has no such
term).  64 rays, 8 coarse + 16 fine samples, the full-size networks with sigma bias 1 (as
tests/test_robust_loss.py's trainer tests), fp32, bf16 under the graph; the pose cases
use three 16 x 16 views around tests/golden's poses.  Printed per case: every parameter
after the last step, and per step ``metrics["loss"]`` and each ``loss_*`` / ``mse_*``
metric.  One process runs all cases.  There is no CPU path."""
import argparse
import hashlib
import itertools
import sys
from pathlib import Path

import numpy as np
import torch

DEV = "cuda"
RAYS, NC, NF, STEPS, SCALE = 64, 8, 16, 3, 0.1


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def nets(precision):
    from noisy_src.config import ModelConfig
    from noisy_src.model import create_nerf
    torch.manual_seed(17)
    pair = create_nerf(ModelConfig(precision=precision))
    for net in pair:
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        sd["sigma_linear.bias"].fill_(1.0)
        net.load_state_dict(sd)
    return pair[0].to(DEV), pair[1].to(DEV)


def ray_batches(n):
    g = torch.Generator().manual_seed(23)
    out = []
    for _ in range(n):
        o = torch.randn(RAYS, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
        d = torch.randn(RAYS, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
        d = torch.nn.functional.normalize(d, dim=-1)
        out.append([t.to(DEV) for t in (o, d, torch.rand(RAYS, 3, generator=g), torch.rand(RAYS, NC, generator=g),
                                        torch.rand(RAYS, NF, generator=g))])
    return out


def pose_setup(tree):
    from noisy_src.data import synthetic_blender_data
    from noisy_src.data_pose_opt import PixelDataset, PixelSampler
    fix = np.load(sorted((tree / "tests" / "golden").glob("final_poses_*rot5.0deg_trans5.0pct_*.npz"))[0])
    init = torch.from_numpy(fix["initial_poses"])[:3]
    data = synthetic_blender_data(torch.from_numpy(fix["ground_truth_poses"])[:3], H=16, W=16, device=DEV)
    sampler = PixelSampler(PixelDataset(data), batch_size=RAYS)
    g = torch.Generator().manual_seed(6)
    jitter = [(torch.rand(RAYS, NC, generator=g).to(DEV), torch.rand(RAYS, NF, generator=g).to(DEV))
              for _ in range(STEPS)]
    batches = [sampler.sample_batch(generator=torch.Generator(device=DEV).manual_seed(5 + k)) for k in range(STEPS)]
    return init.to(DEV), sampler, batches, jitter


def emit(case, steps, params):
    for k, m in enumerate(steps):
        for name in sorted(m):
            if name == "loss" or name.startswith(("loss_", "mse_")):
                print(f"{case}/step{k}/{name} {sha(m[name].float())}")
    for name, p in params:
        print(f"{case}/param/{name} {sha(p)}")


def net_params(mc, mf):
    return [(f"{tag}.{n}", p) for tag, net in (("coarse", mc), ("fine", mf)) for n, p in net.named_parameters()]


def run(tree):
    from noisy_src.config import RenderConfig
    from noisy_src.engine import GraphedTrainer, PoseRefiner, PoseTrainer, Trainer
    from noisy_src.train_pose_opt import CameraPoseParameters
    rc = RenderConfig(num_samples=NC, num_samples_fine=NF)
    init, sampler, pose_batches, jitter = pose_setup(tree)
    for kind, dw in itertools.product(("mse", "cauchy"), (0.0, 0.01)):
        tag = f"{kind}/dw{dw}"
        for name, cs in (("trainer", False), ("trainer_coarse_stream", True)):
            mc, mf = nets("fp32")
            tr = Trainer(mc, mf, rc, coarse_stream=cs, loss=kind, loss_scale=SCALE, distortion_weight=dw)
            emit(f"{name}/{tag}", [tr.step(*b) for b in ray_batches(STEPS)], net_params(mc, mf))
        mc, mf = nets("fp32")
        cam = CameraPoseParameters(init)
        tr = PoseTrainer(mc, mf, cam, sampler, rc, loss=kind, loss_scale=SCALE, distortion_weight=dw)
        steps = [tr.step(b, optimize_poses=True, t_rand=t, u=u) for b, (t, u) in zip(pose_batches, jitter)]
        emit(f"pose_trainer/{tag}", steps, net_params(mc, mf) + list(cam.named_parameters()))
    for kind in ("mse", "cauchy"):
        mc, mf = nets("fp32")
        cam = CameraPoseParameters(init, fixed_small_angle=True).to(DEV)
        with PoseRefiner(mc, mf, cam, sampler, rc, loss=kind, loss_scale=SCALE) as refiner:
            steps = [refiner.step(b, t_rand=t, u=u) for b, (t, u) in zip(pose_batches, jitter)]
        emit(f"pose_refiner/{kind}", steps, list(cam.named_parameters()))
    for kind, dw in itertools.product(("mse", "cauchy"), (0.0, 0.01)):  # the captures last
        mc, mf = nets("bf16")
        tr = Trainer(mc, mf, rc, coarse_stream="auto", loss=kind, loss_scale=SCALE, distortion_weight=dw)
        bs = ray_batches(2 + STEPS)
        tr.step(*bs[0])
        graphed = GraphedTrainer(tr, *bs[1], warmup=1)
        steps = [{k: v.clone() for k, v in graphed.step(*b).items()} for b in bs[2:]]
        emit(f"graphed_trainer/{kind}/dw{dw}", steps, net_params(mc, mf))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="the checkout whose noisy_src runs")
    tree = Path(ap.parse_args().tree).resolve()
    if not torch.cuda.is_available():
        raise SystemExit("loss_fold_step_bits: no GPU found (there is no CPU path)")
    sys.path[:0] = [str(tree), str(tree / "robust-nerf_amd")]
    import noisy_src
    if tree not in Path(noisy_src.__file__).resolve().parents:
        raise SystemExit(f"loss_fold_step_bits: noisy_src came from {noisy_src.__file__}, not from {tree}")
    print(f"# {tree}", file=sys.stderr)
    run(tree)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
