"""CPU: the pose-refinement scene of pose_refine_scene.py is a valid input -- the fp64 oracle
(the reference's restated renderer, a ``torch.linalg.matrix_exp`` pose map of this test's
own, torch's Adam with the 0.1 clip) at least halves both mean pose errors in the 100 fixed
steps.  test_pose_refine.py then asks the device, in fp32, only for a decrease.

Seed 0 is the first of seeds 0..7 and meets the bound with the perturbation the scene
states (0.5 degrees, 0.02); measured: rotation 0.500 -> 0.121 degrees, translation
0.0200 -> 0.0069."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_refine_scene as S  # noqa: E402


def _matrix_exp_pose(init, w, dt):
    """This file's own pose map: exp of the 4 x 4 twist-free generator of the rotation,
    composed with the initial pose, and the translation added."""
    K = torch.zeros(w.shape[0], 3, 3, dtype=w.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-w[:, 2], w[:, 1], w[:, 2], -w[:, 0],
                                                                             -w[:, 1], w[:, 0])
    out = init.clone()
    out[:, :3, :3] = torch.linalg.matrix_exp(K) @ init[:, :3, :3]
    out[:, :3, 3] = init[:, :3, 3] + dt
    return out


def test_scene_pose_map_is_the_matrix_exponential():
    g = torch.Generator().manual_seed(5)
    init = S.ring_poses(4, g)
    w, dt = 0.3 * torch.randn(4, 3, generator=g, dtype=S.F64), torch.randn(4, 3, generator=g, dtype=S.F64)
    got, want = S.pose_map(init, w, dt), _matrix_exp_pose(init, w, dt)
    assert (got - want).abs().max() < 1e-14
    R = got[:, :3, :3]
    assert (R @ R.transpose(1, 2) - torch.eye(3, dtype=S.F64)).abs().max() < 1e-13


def test_oracle_refinement_halves_both_pose_errors():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    sc = S.build(S.SEED)
    assert sc.images.std() > 1e-3, "the field renders a flat image: no pose can be read from it"
    r0, t0 = S.mean_errors(sc.init_poses, sc.gt_poses)
    assert abs(r0 - S.ROT_DEG) < 1e-6 and abs(t0 - S.TRANS) < 1e-9
    poses, losses = S.oracle_refine(sc)
    r1, t1 = S.mean_errors(poses, sc.gt_poses)
    print(f"POSE_REFINE_ORACLE seed {sc.seed}: rot {r0:.4f} -> {r1:.4f} deg, trans {t0:.5f} -> {t1:.5f}, "
          f"loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert r1 <= 0.5 * r0, (r0, r1)
    assert t1 <= 0.5 * t0, (t0, t1)
    assert losses[-1] < losses[0]
