"""GPU: ``python -m noisy_src.inference`` (reference inference.py:446-612) on a checkpoint
written by ``python -m noisy_src.train``: the three modes' files, the ``--precision``
override, and the test views sharded over two ranks under torch.distributed.run."""
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NOISE_ARGS = ["--rotation_noise", "1.0", "--noise_seed", "3"]


def _scene(root: Path, n_train=3, n_val=2, n_test=3, size=16):
    from PIL import Image
    poses = np.load(sorted(GOLDEN.glob("final_poses_*.npz"))[0])["ground_truth_poses"]
    scene = root / "lego"
    rng = np.random.default_rng(0)
    for split, n in (("train", n_train), ("val", n_val), ("test", n_test)):
        (scene / split).mkdir(parents=True, exist_ok=True)
        frames = []
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "RGBA").save(
                scene / split / f"r_{i}.png")
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": poses[i].tolist()})
        (scene / f"transforms_{split}.json").write_text(json.dumps({"camera_angle_x": 0.6911112, "frames": frames}))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One 2-iteration bf16 training run and one ``--mode test`` evaluation of it, shared."""
    from noisy_src import inference
    from noisy_src.train import main as train_main
    tmp = tmp_path_factory.mktemp("cli")
    _scene(tmp / "data")
    train_main(["--data_root", str(tmp / "data"), "--img_scale", "1.0", "--batch_size", "128", "--num_iters", "2",
                "--output_dir", str(tmp / "out"), "--exp_name", "t", "--precision", "bf16"])
    ckpt = tmp / "out" / "t" / "checkpoint_latest.pt"
    before = set(ckpt.parent.iterdir())
    inference.main([str(ckpt), "--mode", "test", "--data_root", str(tmp / "data")] + NOISE_ARGS)
    new = sorted(set(ckpt.parent.iterdir()) - before)
    return {"tmp": tmp, "ckpt": ckpt, "data": tmp / "data", "new": new}


def test_mode_test(run):
    assert len(run["new"]) == 1  # one folder, beside the checkpoint
    out = run["new"][0]
    assert out.is_dir() and out.name.startswith("test_lego_rot1.0deg")
    summary = json.loads((out / "test_metrics.json").read_text())
    assert summary["n_images"] == 3
    assert summary["noise_config"] == {"rotation_noise_deg": 1.0, "translation_noise": 0.0, "seed": 3}
    assert set(summary["actual_noise"]) == {"rotation_error_mean_deg", "rotation_error_std_deg",
                                            "translation_error_mean", "translation_error_std"}
    recs = json.loads((out / "per_image_metrics.json").read_text())
    assert [r["image"] for r in recs] == [0, 1, 2]
    for r in recs:
        assert {"psnr", "ssim", "mse", "render_time", "noise_rotation_error_deg"} <= set(r)
        assert math.isfinite(r["psnr"]) and -1 <= r["ssim"] <= 1
        assert r["psnr"] == pytest.approx(-10 * math.log10(r["mse"]), abs=1e-9)
    assert json.loads((out / "experiment_config.json").read_text())["mode"] == "test"
    pngs = sorted(p.name for p in out.glob("*.png"))
    assert pngs == sorted(f"{k}_{i:03d}.png" for k in ("pred", "gt", "comparison", "depth") for i in range(3))


def test_mode_video(run):
    from noisy_src import inference
    out = run["tmp"] / "video"
    inference.main([str(run["ckpt"]), "--mode", "video", "--n_frames", "3", "--data_root", str(run["data"]),
                    "--output_dir", str(out)] + NOISE_ARGS)
    assert sorted(p.name for p in (out / "frames").iterdir()) == [f"frame_{i:04d}.png" for i in range(3)]
    cfg = json.loads((out / "video_config.json").read_text())
    assert cfg["n_frames"] == 3 and cfg["fps"] == 30 and cfg["noise_config"]["seed"] == 3


def test_mode_single(run):
    """``--mode single`` renders one test view under the pose it has in the full run."""
    from noisy_src import inference
    out = run["tmp"] / "single"
    inference.main([str(run["ckpt"]), "--mode", "single", "--image_index", "1", "--data_root", str(run["data"]),
                    "--output_dir", str(out)] + NOISE_ARGS)
    recs = json.loads((out / "per_image_metrics.json").read_text())
    assert len(recs) == 1 and recs[0]["image"] == 1
    full = json.loads((run["new"][0] / "per_image_metrics.json").read_text())[1]
    for k in ("psnr", "ssim", "noise_rotation_error_deg"):
        assert recs[0][k] == full[k], k
    assert sorted(p.name for p in out.glob("*.png")) == ["comparison_001.png", "depth_001.png", "gt_001.png",
                                                         "pred_001.png"]
    with pytest.raises(SystemExit):
        inference.main([str(run["ckpt"]), "--mode", "single", "--image_index", "3", "--data_root", str(run["data"]),
                        "--output_dir", str(out)])


def test_precision_override(run, monkeypatch):
    """``--precision fp32`` evaluates the bf16-trained checkpoint in the fp32 parity mode.
    The project holds the bf16 rgb maps within DRIFT_MARGIN x the recorded max-abs drift of
    the fp32 oracle (tests/test_parity_fullsize.py, cfg #2).  Pixels that each move by at
    most d move the RMSE by at most d (triangle inequality), so PSNR = -20 log10(RMSE)
    moves by at most 20 log10(1 + d / RMSE)."""
    from test_parity_fullsize import DRIFT_MARGIN, DRIFT_RECORDED

    from noisy_src import inference
    loaded = []
    real = inference.load_checkpoint

    def spy(*a, **kw):
        loaded.append(real(*a, **kw))
        return loaded[-1]

    monkeypatch.setattr(inference, "load_checkpoint", spy)
    out = run["tmp"] / "fp32"
    inference.main([str(run["ckpt"]), "--mode", "single", "--image_index", "0", "--precision", "fp32", "--data_root",
                    str(run["data"]), "--output_dir", str(out)] + NOISE_ARGS)
    renderer = loaded[0][0]
    assert renderer.model_coarse.config.precision == "fp32" and renderer.model_fine.config.precision == "fp32"
    assert real(run["ckpt"], "cuda")[0].model_coarse.config.precision == "bf16"  # the stored one, without the flag
    got = json.loads((out / "per_image_metrics.json").read_text())[0]
    bf16 = json.loads((run["new"][0] / "per_image_metrics.json").read_text())[0]
    d = DRIFT_MARGIN * DRIFT_RECORDED["cfg2"]["rgb_max_abs"]
    bound = 20 * math.log10(1 + d / math.sqrt(min(got["mse"], bf16["mse"])))
    print(f"psnr fp32 {got['psnr']!r} bf16 {bf16['psnr']!r} bound {bound:.3e} dB")
    assert abs(got["psnr"] - bf16["psnr"]) <= bound


def test_two_ranks_match_one_process(run):
    """torchrun mode: the test views sharded over two ranks (gloo here: the two ranks share
    one GPU and RCCL refuses that); rank 0 writes the same per-image records."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NR_DIST_BACKEND="gloo",
               PYTHONPATH=os.pathsep.join([str(ROOT / "robust-nerf_amd"), os.environ.get("PYTHONPATH", "")]))
    out = run["tmp"] / "two"
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                    "127.0.0.1", "--master-port", str(_free_port()), "-m", "noisy_src.inference", str(run["ckpt"]),
                    "--mode", "test", "--data_root", str(run["data"]), "--output_dir", str(out)] + NOISE_ARGS,
                   check=True, env=env, timeout=600, cwd=str(ROOT))
    two = json.loads((out / "per_image_metrics.json").read_text())
    one = json.loads((run["new"][0] / "per_image_metrics.json").read_text())
    assert len(two) == len(one) == 3
    for a, b in zip(one, two):
        for k in ("image", "psnr", "ssim"):
            assert a[k] == b[k], (k, a, b)
    assert json.loads((out / "experiment_config.json").read_text())["ranks"] == 2
    assert len(list(out.glob("*.png"))) == 12
