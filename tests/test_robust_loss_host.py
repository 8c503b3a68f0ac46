"""CPU: the robust photometric loss family (tests/robust_ref.py, the yardstick of
test_robust_loss.py) is what include/nerf_hip.h states, and its host plumbing: the names in
enum order, the trainers' validation, both command lines' flags and the PSNR the iteration
log writes."""
import math
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import robust_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
F64 = torch.float64
SCALES = (0.02, 0.1, 2.0)


def _residuals(n=4001):
    """Residuals over the colour range and beyond, both signs, none exactly at +-c or 0."""
    g = torch.Generator().manual_seed(3)
    return torch.cat([torch.rand(n, generator=g, dtype=F64) * 2 - 1, torch.tensor([1.5, -1.5, 1e-4, -1e-7], dtype=F64)])


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("c", SCALES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_autograd_of_rho_is_two_d_w(kind, c):
    d = _residuals().requires_grad_(True)
    (g,) = torch.autograd.grad(R.rho(d, kind, c).sum(), d)
    want = 2.0 * d.detach() * R.weight(d.detach(), kind, c)
    assert _rel(g, want) < 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
def test_rho_is_quadratic_below_the_scale_and_the_mse_at_a_huge_one(kind):
    pred, target = (t.double() for t in R.inputs(500))
    l_mse, _, g_mse = R.loss_and_grad(pred, target, "mse", 1.0)
    l, l2, g = R.loss_and_grad(pred, target, kind, 1e6)
    assert abs(l - l_mse) < 1e-9 * l_mse and l2 == l_mse and _rel(g, g_mse) < 1e-9
    # the closed form is autograd's gradient of the differentiable form
    p = pred.clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(R.loss(p, target, kind, 0.1), p)
    assert _rel(R.loss_and_grad(pred, target, kind, 0.1)[2], ga) < 1e-12


def test_charbonnier_is_the_textbook_form_without_its_cancellation():
    d = _residuals()
    for c in SCALES:
        q = (d / R._c(c, F64)) ** 2
        assert _rel(R.rho(d, "charbonnier", c), 2 * R._c(c, F64) ** 2 * (torch.sqrt(1 + q) - 1)) < 1e-9


@pytest.mark.parametrize("c", SCALES)
def test_gradient_bounds(c):
    d = torch.linspace(-50 * c, 50 * c, 200001, dtype=F64)
    cc = float(R._c(c, F64))
    mag = {k: (2.0 * d * R.weight(d, k, c)).abs().max().item() for k in R.KINDS}
    assert mag["huber"] <= 2 * cc * (1 + 1e-12)
    assert mag["charbonnier"] < 2 * cc
    assert mag["cauchy"] <= cc * (1 + 1e-12)
    assert mag["geman_mcclure"] <= 0.65 * cc
    assert mag["mse"] == pytest.approx(100 * cc)  # and the MSE's is unbounded


def test_robust_gradients_are_far_from_the_mse_gradient():
    """At c = 0.1 on uniform colours a dropped weight cannot hide under any test tolerance."""
    pred, target = R.inputs(700)
    g_mse = R.loss_and_grad(pred, target, "mse", 0.1)[2]
    for kind in R.KINDS[1:]:
        assert _rel(R.loss_and_grad(pred, target, kind, 0.1)[2], g_mse) > 0.5, kind


def test_loss_kinds_match_the_header_enum():
    from noisy_src import _hip, ops
    text = (ROOT / "include" / "nerf_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{([^}]*NR_LOSS_[^}]*)\}", text).group(1)
    names, value = [], 0
    for item in (s.strip() for s in body.split(",")):
        if not item:
            continue
        name, _, v = item.partition("=")
        value = int(v) if v.strip() else value
        names.append((name.strip(), value))
        value += 1
    assert [n for n, _ in names] == ["NR_LOSS_" + k.upper() for k in ops.LOSS_KINDS]
    assert [v for _, v in names] == list(range(len(ops.LOSS_KINDS)))
    for n, v in names:
        assert getattr(_hip, n) == v
    assert tuple(ops.LOSS_KINDS) == R.KINDS
    assert [ops.loss_kind_index(k) for k in ops.LOSS_KINDS] == list(range(5))
    with pytest.raises(ValueError, match="loss kind"):
        ops.loss_kind_index("l1")


def test_trainers_validate_kind_and_scale():
    import inspect

    from noisy_src.engine import PoseRefiner, PoseTrainer, Trainer, _check_photometric
    for cls in (Trainer, PoseTrainer, PoseRefiner):
        p = inspect.signature(cls.__init__).parameters
        assert p["loss"].default == "mse" and p["loss_scale"].default == 0.1, cls
    assert _check_photometric("cauchy", 0.25) == ("cauchy", 0.25)
    assert _check_photometric("mse", 1) == ("mse", 1.0)
    with pytest.raises(ValueError, match="loss must be one of"):
        _check_photometric("l1", 0.1)
    for kind in ("mse", "huber"):  # the scale is checked under the MSE too
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="loss_scale"):
                _check_photometric(kind, bad)


@pytest.mark.parametrize("module", ["train", "train_pose_opt"])
def test_both_command_lines_parse_the_flags(module):
    import importlib

    from noisy_src import ops
    from noisy_src.run import COMMON_ARGS
    ap = importlib.import_module(f"noisy_src.{module}").build_cli_parser()
    a = ap.parse_args([])
    assert a.loss == "mse" and a.loss_scale == 0.1
    a = ap.parse_args(["--loss", "geman_mcclure", "--loss_scale", "0.25"])
    assert a.loss == "geman_mcclure" and a.loss_scale == 0.25
    assert next(x for x in ap._actions if x.dest == "loss").choices == list(ops.LOSS_KINDS)
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss", "l1"])
    assert {"loss", "loss_scale"} <= set(COMMON_ARGS)


def test_inference_parses_the_refine_loss_flags():
    from noisy_src.inference import build_arg_parser
    a = build_arg_parser().parse_args(["ckpt.pt"])
    assert a.refine_loss == "mse" and a.refine_loss_scale == 0.1
    a = build_arg_parser().parse_args(["ckpt.pt", "--refine_loss", "huber", "--refine_loss_scale", "0.05"])
    assert a.refine_loss == "huber" and a.refine_loss_scale == 0.05


class _Logger:
    def __init__(self):
        self.rows = []

    def log_training(self, m):
        self.rows.append(m)


def _iteration_log(lines):
    """An IterationLog without its device-side queue (LaggedScalars pins host memory)."""
    from noisy_src.run import IterationLog
    ilog = IterationLog.__new__(IterationLog)
    ilog.logger, ilog.process_group, ilog.log = _Logger(), None, lines.append
    ilog.line = lambda vm, lr, rps, meta: "mid"
    ilog.batch_size, ilog.num_iterations, ilog.log_every = 64, 10, 1
    ilog.start = ilog.t_prev = 0.0
    return ilog


def test_iteration_log_takes_the_psnr_from_the_mse_when_it_is_there():
    lines = []
    ilog = _iteration_log(lines)
    keys = ["loss", "loss_coarse", "loss_fine", "mse_coarse", "mse_fine"]
    ilog._write(([0.03, 0.02, 0.01, 0.08, 0.04], (1, keys, 5e-4, 0.5, None)))
    ilog._write(([0.03, 0.02, 0.01], (2, keys[:3], 5e-4, 0.5, None)))
    ilog._write(([0.02, 0.02, 0.08], (3, ["loss", "loss_coarse", "mse_coarse"], 5e-4, 0.5, None)))
    ilog._write(([0.02, 0.02], (4, ["loss", "loss_coarse"], 5e-4, 0.5, None)))
    rows = ilog.logger.rows
    assert [r.psnr for r in rows] == [-10 * math.log10(v) for v in (0.04, 0.01, 0.08, 0.02)]
    assert rows[0].loss == 0.03 and rows[0].loss_coarse == 0.02 and rows[0].loss_fine == 0.01  # what is minimised
    assert len(lines) == 4


def test_loss_line_names_a_robust_kind_only():
    from noisy_src.run import loss_line
    assert loss_line("mse", 0.1) == ""
    assert loss_line("cauchy", 0.1) == "cauchy(c=0.1) | "
