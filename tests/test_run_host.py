"""CPU: the run harness the two training loops share (``noisy_src.run``; no kernel runs):
the flag tables of both command lines, the validation / checkpoint cadence, the noise
flags, the checkpoint and ``experiment_config.json`` writers and the validation loop."""
import json
from argparse import Namespace
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
LAYOUT = json.loads((ROOT / "tests" / "golden" / "reference_artifacts.json").read_text())["layout"]

# (option string, type, default, action class) of every action, in order, as the parsers were
# before they shared ``add_common_args``
TRAIN_FLAGS = [
    ("--help", None, "==SUPPRESS==", "_HelpAction"),
    ("--scene", str, "lego", "_StoreAction"),
    ("--data_root", str, None, "_StoreAction"),
    ("--img_scale", float, 0.5, "_StoreAction"),
    ("--batch_size", int, 1024, "_StoreAction"),
    ("--num_iters", int, 200000, "_StoreAction"),
    ("--lr", float, 0.0005, "_StoreAction"),
    ("--no_hierarchical", None, False, "_StoreTrueAction"),
    ("--num_samples", int, 64, "_StoreAction"),
    ("--num_samples_fine", int, 128, "_StoreAction"),
    ("--rotation_noise", float, 0.0, "_StoreAction"),
    ("--translation_noise", float, 0.0, "_StoreAction"),
    ("--translation_noise_pct", float, 0.0, "_StoreAction"),
    ("--noise_seed", int, None, "_StoreAction"),
    ("--log_every", int, 100, "_StoreAction"),
    ("--val_every", int, 5000, "_StoreAction"),
    ("--save_every", int, 10000, "_StoreAction"),
    ("--output_dir", str, "outputs", "_StoreAction"),
    ("--exp_name", str, "auto", "_StoreAction"),
    ("--device", str, "cuda", "_StoreAction"),
    ("--seed", int, 42, "_StoreAction"),
    ("--precision", str, "fp32", "_StoreAction"),
    ("--graph", None, False, "_StoreTrueAction"),
    ("--distortion_weight", float, 0.0, "_StoreAction"),
]
POSE_FLAGS = [
    ("--help", None, "==SUPPRESS==", "_HelpAction"),
    ("--scene", str, "lego", "_StoreAction"),
    ("--data_root", str, None, "_StoreAction"),
    ("--img_scale", float, 0.5, "_StoreAction"),
    ("--batch_size", int, 1024, "_StoreAction"),
    ("--num_iters", int, 50000, "_StoreAction"),
    ("--lr", float, 0.0005, "_StoreAction"),
    ("--init_mode", str, "noisy", "_StoreAction"),
    ("--pose_lr", float, 0.0001, "_StoreAction"),
    ("--pose_opt_delay", int, 1000, "_StoreAction"),
    ("--no_learn_rotation", None, False, "_StoreTrueAction"),
    ("--no_learn_translation", None, False, "_StoreTrueAction"),
    ("--rotation_reg_weight", float, 0.01, "_StoreAction"),
    ("--translation_reg_weight", float, 0.001, "_StoreAction"),
    ("--rotation_noise", float, 0.0, "_StoreAction"),
    ("--translation_noise", float, 0.0, "_StoreAction"),
    ("--translation_noise_pct", float, 0.0, "_StoreAction"),
    ("--noise_seed", int, None, "_StoreAction"),
    ("--no_hierarchical", None, False, "_StoreTrueAction"),
    ("--num_samples", int, 64, "_StoreAction"),
    ("--num_samples_fine", int, 128, "_StoreAction"),
    ("--log_every", int, 100, "_StoreAction"),
    ("--val_every", int, 2500, "_StoreAction"),
    ("--save_every", int, 10000, "_StoreAction"),
    ("--output_dir", str, "outputs", "_StoreAction"),
    ("--device", str, "cuda", "_StoreAction"),
    ("--seed", int, 42, "_StoreAction"),
    ("--precision", str, "fp32", "_StoreAction"),
    ("--graph", None, False, "_StoreTrueAction"),
    ("--c2f", float, None, "_StoreAction"),
    ("--fixed_small_angle", None, False, "_StoreTrueAction"),
    ("--learn_focal", str, None, "_StoreAction"),
    ("--focal_init_scale", float, 1.0, "_StoreAction"),
    ("--distortion_weight", float, 0.0, "_StoreAction"),
]


@pytest.mark.parametrize("module, table", [("train", TRAIN_FLAGS), ("train_pose_opt", POSE_FLAGS)])
def test_parser_tables(module, table):
    import importlib
    ap = importlib.import_module(f"noisy_src.{module}").build_arg_parser()
    got = [(a.option_strings[-1], a.type, a.default, type(a).__name__) for a in ap._actions]
    assert got == table
    if module == "train_pose_opt":
        c2f = next(a for a in ap._actions if a.dest == "c2f")
        assert c2f.nargs == 2 and c2f.metavar == ("START", "END")
    choices = {a.dest: a.choices for a in ap._actions if a.choices}
    assert choices.pop("precision") == ["fp32", "bf16", "fp16"]
    assert choices == ({} if module == "train" else {"init_mode": ["noisy", "clean"], "learn_focal": ["shared", "xy"]})


def test_both_modules_export_the_one_set_seed():
    import importlib
    run, train, train_pose_opt = (importlib.import_module(f"noisy_src.{m}") for m in ("run", "train", "train_pose_opt"))
    assert train.set_seed is run.set_seed and train_pose_opt.set_seed is run.set_seed
    assert "set_seed" in train.__all__ and "set_seed" in train_pose_opt.__all__
    assert train.checkpoint_config is run.checkpoint_config and train.noise_dict is run.noise_dict
    assert train_pose_opt.create_nerf_for is run.create_nerf_for


V, S = "val", "save"
DUE = {  # (val_every, save_every) -> due(i, ...) at i = 0 .. 12
    (2, 3): [None, None, V, S, V, None, V, None, V, S, V, None, V],
    (4, 100): [None, None, None, None, V, None, None, None, V, None, None, None, V],
    (5, 5): [None, None, None, None, None, V, None, None, None, None, V, None, None],
    (1, 1): [None] + [V] * 12,
}


@pytest.mark.parametrize("every", list(DUE))
def test_due(every):
    from noisy_src.run import due
    assert [due(i, *every) for i in range(13)] == DUE[every]


def _noise_args(**kw):
    return Namespace(**{**dict(rotation_noise=0.0, translation_noise=0.0, translation_noise_pct=0.0, noise_seed=7), **kw})


def test_noise_config_from_args():
    from noisy_src.noise import NoiseConfig
    from noisy_src.run import noise_config_from_args
    assert noise_config_from_args(_noise_args()) is None
    assert noise_config_from_args(_noise_args(rotation_noise=1.5)) == NoiseConfig(rotation_noise_deg=1.5, seed=7)
    assert noise_config_from_args(_noise_args(translation_noise=0.02)) == NoiseConfig(translation_noise=0.02, seed=7)
    assert noise_config_from_args(_noise_args(translation_noise_pct=5.0)) == NoiseConfig(translation_noise_pct=5.0,
                                                                                         seed=7)


BASE_KEYS = {"iteration", "model_coarse", "config", "mi355x"}


def test_base_checkpoint_and_write_checkpoint(tmp_path):
    from noisy_src.config import NeRFConfig
    from noisy_src.noise import NoiseConfig
    from noisy_src.run import base_checkpoint, write_checkpoint
    coarse, fine = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    cfg = NeRFConfig()
    cfg.model.precision = "bf16"
    assert set(base_checkpoint(4, coarse, None, cfg)) == BASE_KEYS
    assert set(base_checkpoint(4, coarse, fine, cfg)) == BASE_KEYS | {"model_fine"}
    assert set(base_checkpoint(4, coarse, None, cfg, metrics={"psnr": 1.0})) == BASE_KEYS | {"metrics"}
    assert set(base_checkpoint(4, coarse, None, cfg, NoiseConfig(1.0, seed=3))) == BASE_KEYS | {"noise_config"}
    ckpt = base_checkpoint(4, coarse, fine, cfg, NoiseConfig(1.0, seed=3), {"psnr": 21.5, "ssim": 0.5})
    assert set(ckpt) == BASE_KEYS | {"model_fine", "metrics", "noise_config"}
    assert ckpt["noise_config"] == {"rotation_noise_deg": 1.0, "translation_noise": 0.0, "translation_noise_pct": 0.0,
                                    "seed": 3}
    assert ckpt["mi355x"] == {"precision": "bf16"} and "precision" not in ckpt["config"]["model"]

    run = tmp_path / "a" / "run"  # does not exist yet
    write_checkpoint(run, 4, ckpt)
    assert sorted(f.name for f in run.iterdir()) == ["checkpoint_0000004.pt", "checkpoint_latest.pt"]
    write_checkpoint(run, 8, ckpt, is_best=True)
    assert sorted(f.name for f in run.iterdir()) == ["checkpoint_0000004.pt", "checkpoint_0000008.pt",
                                                      "checkpoint_best.pt", "checkpoint_latest.pt"]
    for name in ("checkpoint_0000004.pt", "checkpoint_latest.pt", "checkpoint_best.pt"):
        back = torch.load(run / name, weights_only=True)
        assert set(back) == set(ckpt) and back["iteration"] == 4 and back["metrics"] == ckpt["metrics"]
        assert back["config"] == ckpt["config"]
        assert torch.equal(back["model_coarse"]["weight"], coarse.weight)
        assert torch.equal(back["model_fine"]["bias"], fine.bias)


OURS = {"data_parallel_ranks", "distortion_weight"}  # what this project adds to the reference's keys


def test_write_experiment_config(tmp_path):
    from noisy_src.config import NeRFConfig
    from noisy_src.noise import NoiseConfig
    from noisy_src.run import NO_NOISE, write_experiment_config
    cfg = NeRFConfig()

    def written(noise_config, kind):
        if kind == "train":
            write_experiment_config(tmp_path, cfg, "name", 2, noise_config, NO_NOISE,
                                    after_batch={"img_scale": cfg.data.img_scale}, extra={"distortion_weight": 0.0})
        else:
            write_experiment_config(tmp_path, cfg, "name", 2, noise_config, extra={"distortion_weight": 0.0},
                                    after_name={"init_mode": "noisy", "pose_optimization": {"pose_lr": 1e-4}})
        return json.loads((tmp_path / "experiment_config.json").read_text())

    for kind in ("train", "pose_opt"):
        for nc in (None, NoiseConfig(rotation_noise_deg=2.0, seed=5)):
            assert set(written(nc, kind)) == set(LAYOUT[kind]["experiment_config_keys"]) | OURS, kind
    zeros = {"rotation_noise_deg": 0, "translation_noise": 0, "translation_noise_pct": 0, "seed": None,
             "has_noise": False}
    assert written(None, "train")["noise_config"] == zeros
    assert written(None, "pose_opt")["noise_config"] is None
    noisy = {"rotation_noise_deg": 2.0, "translation_noise": 0.0, "translation_noise_pct": 0.0, "seed": 5,
             "has_noise": True}
    for kind in ("train", "pose_opt"):
        d = written(NoiseConfig(rotation_noise_deg=2.0, seed=5), kind)
        assert d["noise_config"] == noisy and d["data_parallel_ranks"] == 2 and d["experiment_name"] == "name"
    # the reference's key order, this project's keys at the end
    assert list(written(None, "train")) == ["scene", "experiment_name", "noise_config", "num_iterations", "batch_size",
                                            "img_scale", "timestamp", "data_parallel_ranks", "distortion_weight"]
    assert list(written(None, "pose_opt")) == ["scene", "experiment_name", "init_mode", "pose_optimization",
                                               "noise_config", "num_iterations", "batch_size", "timestamp",
                                               "data_parallel_ranks", "distortion_weight"]


class _StubLogger:
    def __init__(self):
        self.calls = []

    def log_images(self, tag, pred, gt, iteration, depth=None):
        self.calls.append((tag, iteration, float(pred[0, 0, 0]), float(gt[0, 0, 0]), float(depth[0, 0])))


def test_evaluate_views():
    from noisy_src.metrics import compute_ssim
    from noisy_src.run import evaluate_views
    # four 12x12 views: view v renders the constant 0.5 + 0.1 v against a target of 0.5, so
    # its MSE is (0.1 v)^2 exactly up to fp32 rounding and its PSNR -10 log10 of that
    target = torch.full((12, 12, 3), 0.5)
    preds = {v: torch.full((12, 12, 3), 0.5 + 0.1 * v) for v in (1, 2, 3, 4)}
    rendered = []

    def render_view(v):
        rendered.append(v)
        return {"rgb": preds[v], "depth": torch.full((12, 12), float(v))}

    views = [(f"tag{v}", v, target) for v in (1, 2, 3, 4)]
    logger = _StubLogger()
    vm = evaluate_views(render_view, iter(views), logger, 9)
    assert rendered == [1, 2, 3, 4] and vm.iteration == 9 and vm.lpips is None
    mse = [float(((preds[v] - target) ** 2).mean()) for v in (1, 2, 3, 4)]
    psnr = [-10.0 * torch.log10(torch.tensor(m)).item() for m in mse]
    ssim = [compute_ssim(preds[v], target).item() for v in (1, 2, 3, 4)]
    assert vm.per_image_psnr == pytest.approx(psnr, rel=1e-6) and vm.per_image_ssim == ssim
    assert vm.psnr == pytest.approx(sum(psnr) / 4, rel=1e-6)
    assert vm.mse == pytest.approx(sum(mse) / 4, rel=1e-6) and vm.ssim == pytest.approx(sum(ssim) / 4, rel=1e-6)
    assert mse == pytest.approx([0.01, 0.04, 0.09, 0.16], rel=1e-5)
    # PNGs of the first three views only, under the tags the caller chose
    assert [(c[0], c[1]) for c in logger.calls] == [("tag1", 9), ("tag2", 9), ("tag3", 9)]
    assert [c[2:] for c in logger.calls] == [pytest.approx((0.5 + 0.1 * v, 0.5, float(v))) for v in (1, 2, 3)]

    vm = evaluate_views(render_view, views[:2])  # no logger, no metric
    assert vm.iteration == 0 and vm.lpips is None and len(vm.per_image_psnr) == 2
    vm = evaluate_views(render_view, views[:2], lpips_metric=lambda pred, tgt: torch.tensor(0.25))
    assert vm.lpips == 0.25
    vm = evaluate_views(render_view, views[:2], lpips_metric=lambda pred, tgt: None)  # an unavailable metric
    assert vm.lpips is None
