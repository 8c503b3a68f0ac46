"""
Gauge alignment of optimised camera poses (no reference counterpart; BARF's evaluation
protocol).

Joint pose / field optimisation recovers the train poses only up to a global similarity:
the field is free to settle in any rotated, shifted and rescaled frame as long as the
poses move with it.  Comparing optimised and ground-truth poses in the raw frame
(``CameraPoseParameters.compute_pose_errors``) therefore mixes real error with gauge
drift.  ``align_sim3`` finds the similarity (Umeyama 1991, on the camera centres) that
maps the optimised poses onto the ground truth; ``aligned_pose_errors`` measures after
it; ``to_learned_frame`` carries ground-truth poses of other views (the test split)
into the frame the field was trained in.

Host code in fp64: a hundred poses are not a kernel's job.

    python -m noisy_src.pose_eval FINAL_POSES.pt [--out aligned_pose_errors.json]
"""

from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, NamedTuple

import numpy as np
import torch


class Sim3(NamedTuple):
    """x -> s R x + t (fp64): scale, (3,3) rotation, (3,) translation."""

    s: float
    R: torch.Tensor
    t: torch.Tensor

    def to_json(self) -> Dict[str, object]:
        return {"s": float(self.s), "R": self.R.tolist(), "t": self.t.tolist()}


def _poses64(poses) -> torch.Tensor:
    p = torch.as_tensor(np.asarray(poses.detach().cpu()) if isinstance(poses, torch.Tensor) else np.asarray(poses))
    p = p.to(torch.float64)
    if p.dim() != 3 or p.shape[1] < 3 or p.shape[2] != 4:
        raise ValueError(f"poses must be (N,4,4) or (N,3,4) camera-to-world matrices, got {tuple(p.shape)}")
    return p


def align_sim3(pred_poses, gt_poses) -> Sim3:
    """The similarity minimising sum |c_gt - (s R c_pred + t)|^2 over the camera centres
    (Umeyama), a proper rotation also when the best orthogonal map is a reflection.
    ValueError for fewer than 3 poses or centres whose covariance has rank < 2 (a point
    or a line leaves the rotation undetermined)."""
    x, y = _poses64(pred_poses)[:, :3, 3], _poses64(gt_poses)[:, :3, 3]
    if x.shape != y.shape:
        raise ValueError(f"align_sim3: {x.shape[0]} predicted poses against {y.shape[0]} ground-truth poses")
    n = x.shape[0]
    if n < 3:
        raise ValueError(f"align_sim3 needs at least 3 poses, got {n}")
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    var_x = (xc ** 2).sum() / n
    # both centre sets must span a plane: singular values of their own covariances
    for name, c in (("predicted", xc), ("ground-truth", yc)):
        sv = torch.linalg.svdvals(c.T @ c / n)
        if not sv[1] > 1e-12 * max(float(sv[0]), 1e-300):
            raise ValueError(f"align_sim3: the {name} camera centres have a covariance of rank < 2 "
                             "(coincident or collinear): the alignment is not determined")
    U, D, Vt = torch.linalg.svd(yc.T @ xc / n)
    S = torch.ones(3, dtype=torch.float64)
    if torch.linalg.det(U) * torch.linalg.det(Vt) < 0:
        S[2] = -1.0  # the reflection case: flip the weakest direction
    R = U @ torch.diag(S) @ Vt
    s = float((D * S).sum() / var_x)
    t = my - s * (R @ mx)
    return Sim3(s, R, t)


def apply_sim3(sim3: Sim3, poses) -> torch.Tensor:
    """Camera-to-world poses under the similarity: R' = R R_c2w, t' = s R t_c2w + t."""
    p = _poses64(poses)
    out = torch.zeros(p.shape[0], 4, 4, dtype=torch.float64)
    out[:, :3, :3] = sim3.R @ p[:, :3, :3]
    out[:, :3, 3] = sim3.s * (p[:, :3, 3] @ sim3.R.T) + sim3.t
    out[:, 3, 3] = 1.0
    return out


def to_learned_frame(sim3: Sim3, gt_poses) -> torch.Tensor:
    """The inverse of ``apply_sim3``: ground-truth-frame poses in the frame of the
    optimised poses ``sim3`` was aligned from."""
    p = _poses64(gt_poses)
    out = torch.zeros(p.shape[0], 4, 4, dtype=torch.float64)
    out[:, :3, :3] = sim3.R.T @ p[:, :3, :3]
    out[:, :3, 3] = ((p[:, :3, 3] - sim3.t) @ sim3.R) / sim3.s
    out[:, 3, 3] = 1.0
    return out


def pose_error(pose_gt: torch.Tensor, pose: torch.Tensor) -> Dict[str, float]:
    """``noise.compute_pose_error``'s two quantities (geodesic angle of R_gt^T R in degrees,
    centre distance) in fp64, the angle from atan2(sin, cos): acos loses half the digits
    next to 0, which is exactly where aligned errors live."""
    Rd = pose_gt[:3, :3].T @ pose[:3, :3]
    sin2 = torch.stack([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]).norm()
    ang = torch.atan2(sin2 / 2, (torch.trace(Rd) - 1) / 2)
    return {"rotation_error_deg": float(ang * 180 / np.pi),
            "translation_error": float(torch.norm(pose_gt[:3, 3] - pose[:3, 3]))}


def pose_error_summary(errs) -> Dict[str, float]:
    """Means, deviations and maxima with the keys of ``compute_pose_errors``."""
    r = [e["rotation_error_deg"] for e in errs]
    t = [e["translation_error"] for e in errs]
    return {"rotation_error_mean": float(np.mean(r)), "rotation_error_std": float(np.std(r)),
            "rotation_error_max": float(np.max(r)), "translation_error_mean": float(np.mean(t)),
            "translation_error_std": float(np.std(t)), "translation_error_max": float(np.max(t))}


def aligned_pose_errors(pred_poses, gt_poses) -> Dict[str, object]:
    """Per-pose errors of ``pred_poses`` against ``gt_poses`` after the similarity that best
    aligns them, with the summary keys of ``CameraPoseParameters.compute_pose_errors``, the
    per-pose records (``per_pose``) and the similarity (``sim3``)."""
    sim = align_sim3(pred_poses, gt_poses)
    aligned, gt = apply_sim3(sim, pred_poses), _poses64(gt_poses)
    errs = [pose_error(gt[i], aligned[i]) for i in range(gt.shape[0])]
    out: Dict[str, object] = dict(pose_error_summary(errs))
    out["per_pose"] = errs
    out["sim3"] = sim.to_json()
    return out


FOCAL_KEYS = ("initial_focal", "optimized_focal", "ground_truth_focal")


def focal_errors(record) -> Dict[str, object]:
    """The focal report of a ``final_poses.pt`` written with ``--learn_focal`` (the three
    ``*_focal`` entries, (fx, fy) each): the values and their errors against the ground
    truth in per cent, per axis and as the mean of the absolute values.  {} for a record
    without the entries.  The Sim(3) alignment does not touch this number: a focal length
    that is off by a factor is compensated by the cameras' distance to the scene, not by a
    global scale of the frame."""
    if not all(k in record for k in FOCAL_KEYS):
        return {}
    init, opt, gt = (torch.as_tensor(record[k], dtype=torch.float64).reshape(-1).expand(2) for k in FOCAL_KEYS)

    def pct(f):
        return ((f / gt - 1.0) * 100.0).tolist()

    e0, e1 = pct(init), pct(opt)
    return {"initial_focal": init.tolist(), "optimized_focal": opt.tolist(), "ground_truth_focal": gt.tolist(),
            "initial_focal_error_pct": e0, "optimized_focal_error_pct": e1,
            "initial_focal_error_pct_mean_abs": float(np.mean(np.abs(e0))),
            "optimized_focal_error_pct_mean_abs": float(np.mean(np.abs(e1)))}


LENS_KEYS = ("initial_lens", "optimized_lens", "ground_truth_lens")
LENS_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2")


def lens_errors(record) -> Dict[str, object]:
    """The lens report of a ``final_poses.pt`` written with a lens option (the three ``*_lens``
    entries, (fx, fy, cx, cy, k1, k2) each): the values, and for cx, cy (pixels), k1, k2 the
    differences against the ground truth, initial and optimised.  {} for a record without the
    entries.  The focal pair has its own report (``focal_errors``).  These numbers stand beside
    the pose errors and are not folded into them: k1 couples with the focal length (both scale
    the image about its centre, differently only in r^2) and a principal-point shift with a
    small rotation of every camera (both move the image sideways, differently only at second
    order), so an error in one is partly an error in the other, and neither is a gauge freedom
    the Sim(3) alignment could remove."""
    if not all(k in record for k in LENS_KEYS):
        return {}
    init, opt, gt = (torch.as_tensor(record[k], dtype=torch.float64).reshape(-1) for k in LENS_KEYS)
    if any(t.numel() != 6 for t in (init, opt, gt)):
        raise ValueError("pose_eval: the *_lens entries must hold six numbers (fx, fy, cx, cy, k1, k2)")
    out: Dict[str, object] = {"initial_lens": init.tolist(), "optimized_lens": opt.tolist(),
                              "ground_truth_lens": gt.tolist()}
    for e, name in enumerate(LENS_NAMES[2:], start=2):
        out[f"initial_{name}_error"] = float(init[e] - gt[e])
        out[f"optimized_{name}_error"] = float(opt[e] - gt[e])
    return out


def main(argv=None) -> None:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m noisy_src.pose_eval",
                                 description="Pose errors of a joint pose-optimisation run after Sim(3) gauge alignment")
    ap.add_argument("final_poses", type=Path, help="final_poses.pt written by noisy_src.train_pose_opt")
    ap.add_argument("--out", type=Path, default=None, help="JSON output (default: aligned_pose_errors.json beside it)")
    a = ap.parse_args(argv)
    d = torch.load(a.final_poses, map_location="cpu", weights_only=True)
    res = aligned_pose_errors(d["optimized_poses"], d["ground_truth_poses"])
    gt = _poses64(d["ground_truth_poses"])
    raw = _poses64(d["optimized_poses"])
    res["unaligned"] = pose_error_summary([pose_error(gt[i], raw[i]) for i in range(gt.shape[0])])
    focal = focal_errors(d)
    if focal:
        res["focal"] = focal
    lens = lens_errors(d)
    if lens:
        res["lens"] = lens
    out = a.out if a.out is not None else a.final_poses.parent / "aligned_pose_errors.json"
    out.write_text(json.dumps(res, indent=2))
    print(f"aligned: rot {res['rotation_error_mean']:.4f} deg, trans {res['translation_error_mean']:.5f} "
          f"(raw frame: rot {res['unaligned']['rotation_error_mean']:.4f} deg, "
          f"trans {res['unaligned']['translation_error_mean']:.5f}); scale {res['sim3']['s']:.6f}; wrote {out}")
    if focal:
        print(f"focal error: {focal['initial_focal_error_pct_mean_abs']:.3f} % -> "
              f"{focal['optimized_focal_error_pct_mean_abs']:.3f} % (mean |f / f_gt - 1| over fx, fy)")
    if lens:
        print("lens error (initial -> optimised, not part of the pose errors): " + "; ".join(
            f"{n} {lens[f'initial_{n}_error']:+.5f} -> {lens[f'optimized_{n}_error']:+.5f}" for n in LENS_NAMES[2:])
            + " (cx, cy in pixels)")


if __name__ == "__main__":
    main()
