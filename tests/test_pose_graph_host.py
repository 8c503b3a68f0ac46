"""CPU: the host-side surface of the hipGraph replay of the joint pose-optimisation step
(no kernel runs): the ``--graph`` flag of ``noisy_src.train_pose_opt``, the argument
checks that fire before any device work, and the measurement tool's refusal to run
without a GPU."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_train_pose_opt_parser_has_graph_flag():
    from noisy_src.train_pose_opt import build_arg_parser
    ap = build_arg_parser()
    assert ap.parse_args([]).graph is False
    assert ap.parse_args(["--graph"]).graph is True
    assert "1024 rays" in " ".join(ap.format_help().split())  # the help quotes the measured table


def test_gather_pixels_is_declared_and_has_no_cpu_path():
    from noisy_src import _hip, ops
    res, args = _hip._SIGNATURES["nr_gather_pixels"]
    assert res is _hip.c_i and len(args) == 11  # the header's eleven arguments, stream last
    with pytest.raises(RuntimeError, match="CPU"):
        ops.gather_pixels(torch.zeros(4, dtype=torch.int64), torch.zeros(1, 2, 2, 3))


def test_graphed_pose_trainer_refuses_unvalidated_batch_first():
    """in_range=False is refused before anything else is touched (no trainer needed)."""
    from noisy_src.data_pose_opt import PixelBatch
    from noisy_src.engine import GraphedPoseTrainer
    batch = PixelBatch(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 2), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="in_range"):
        GraphedPoseTrainer(None, batch)


def test_pose_graph_ab_fails_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")  # hide any GPU from the child
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "pose_graph_ab.py"), "--out", "/dev/null"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "no GPU" in r.stderr
