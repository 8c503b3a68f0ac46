"""CPU: the distortion regulariser's yardstick (tests/distortion_ref.py) against itself and
against known answers, the new flag on both entry points, and the argument errors of
``nr_distortion_loss`` (returned before any launch, so they need no device).

The GPU file (test_distortion.py) holds the kernel to ``pairs_loss_and_grad`` in fp64; here
that function, the prefix form the kernel implements and the closed-form gradient are all
tied to autograd of the definition's double sum."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distortion_ref as R  # noqa: E402

F64 = torch.float64
CASES = [(1, 2.0, 6.0), (65, 2.0, 6.0), (192, 0.5, 3.0), (768, 2.0, 6.0)]


def _inputs(S, near, far, kind, B=3):
    g = torch.Generator().manual_seed(1000 + S)
    z = R.sorted_z(B, S, near, far, g, ties=kind == "ties")
    sigma = R.peaked_sigma(B, S) if kind == "peaked" else R.uniform_sigma(B, S, g)
    return R.composite_weights(sigma, z), z


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("kind", ["uniform", "peaked", "ties"])
@pytest.mark.parametrize("S,near,far", CASES)
def test_prefix_form_equals_the_double_sum_in_fp64(S, near, far, kind):
    w, z = _inputs(S, near, far, kind)
    lp, rp, gp = R.loss_and_grad(w, z, near, far, F64, R.loss_rays_pairs)
    lx, rx, gx = R.loss_and_grad(w, z, near, far, F64, R.loss_rays_prefix)
    assert _rel(rx, rp) < 1e-13 and _rel(gx, gp) < 1e-13 and abs(float(lx - lp)) < 1e-13 * float(lp)


@pytest.mark.parametrize("kind", ["uniform", "peaked", "ties"])
@pytest.mark.parametrize("S,near,far", CASES)
def test_closed_form_gradient_equals_autograd(S, near, far, kind):
    w, z = _inputs(S, near, far, kind)
    B = w.shape[0]
    _, rays, g = R.loss_and_grad(w, z, near, far, F64, R.loss_rays_pairs)
    assert _rel(R.grad_closed(w, z, near, far, F64) / B, g) < 1e-13
    # the autograd-free O(S^2) evaluation the GPU tests use as their truth
    lm, rm, gm = R.pairs_loss_and_grad(w, z, near, far, F64)
    assert _rel(rm, rays) < 1e-13 and _rel(gm, g) < 1e-13 and abs(float(lm - rays.mean())) < 1e-13 * float(lm)


def test_zero_weights_give_zero():
    z = R.sorted_z(2, 65, 2.0, 6.0, torch.Generator().manual_seed(1))
    w = torch.zeros(2, 65)
    for form in (R.loss_rays_pairs, R.loss_rays_prefix):
        loss, rays, g = R.loss_and_grad(w, z, 2.0, 6.0, F64, form)
        assert float(loss) == 0.0 and not rays.any() and not g.any()
    assert not R.grad_closed(w, z, 2.0, 6.0).any()


def test_single_sample_known_answer():
    """S = 1: one interval [s, 1], no pair term: L = w^2 (1 - s) / 3."""
    w, z, near, far = torch.tensor([[0.7]]), torch.tensor([[3.0]]), 2.0, 6.0
    s = (3.0 - near) / (far - near)
    for form in (R.loss_rays_pairs, R.loss_rays_prefix):
        rays = form(w, z, near, far, F64)
        assert abs(float(rays[0]) - float(w.double()[0, 0]) ** 2 * (1.0 - s) / 3.0) < 1e-15
    assert abs(float(R.grad_closed(w, z, near, far)[0, 0]) - 2.0 * float(w.double()[0, 0]) * (1.0 - s) / 3.0) < 1e-15


def test_two_spikes_known_answer():
    """Two weights of sum 1 at samples a < b of an otherwise empty ray:
    L = 2 w_a w_b |m_a - m_b| + (w_a^2 d_a + w_b^2 d_b) / 3."""
    near, far, S, a, b = 0.5, 3.0, 9, 2, 6
    z = torch.linspace(near, far, S + 1)[:-1].reshape(1, S).float()
    w = torch.zeros(1, S)
    w[0, a], w[0, b] = 0.25, 0.75
    m, d = R.intervals(z, near, far)
    want = 2 * 0.25 * 0.75 * abs(float(m[0, a] - m[0, b])) + (0.25 ** 2 * float(d[0, a]) + 0.75 ** 2 * float(d[0, b])) / 3
    assert abs(float(m[0, b] - m[0, a]) - (b - a) / S) < 1e-7  # uniform samples: midpoints (b - a) / S apart
    for form in (R.loss_rays_pairs, R.loss_rays_prefix):
        assert abs(float(form(w, z, near, far, F64)[0]) - want) < 1e-15


@pytest.mark.parametrize("module", ["train", "train_pose_opt"])
def test_flag_parses_and_defaults_to_zero(module):
    import importlib
    ap = importlib.import_module("noisy_src." + module).build_arg_parser()
    assert ap.parse_args([]).distortion_weight == 0.0
    assert ap.parse_args(["--distortion_weight", "0.01"]).distortion_weight == 0.01


def test_trainers_take_the_keyword_and_refuse_a_negative_weight():
    import inspect
    from noisy_src.engine import PoseTrainer, Trainer
    for cls in (Trainer, PoseTrainer):
        assert inspect.signature(cls.__init__).parameters["distortion_weight"].default == 0.0
    from noisy_src.engine import _check_distortion_weight
    for bad in (-0.01, float("nan")):
        with pytest.raises(ValueError, match="distortion_weight"):
            _check_distortion_weight(bad)


def test_op_refuses_cpu_tensors_and_mismatched_shapes():
    from noisy_src import ops
    with pytest.raises(RuntimeError, match="CPU"):
        ops.distortion_loss(torch.zeros(2, 4), torch.zeros(2, 4), 2.0, 6.0)


def test_argument_errors_before_any_launch():
    """B < 1, S < 1, S > 4096, far <= near and each null pointer: NR_EARG with a message.  The
    pointers are never read on the host, so a host buffer stands in for device memory."""
    from noisy_src import _hip
    if not _hip.lib_path().exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    L = _hip.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert L.nr_distortion_workspace_bytes(5) >= 5 * 4 and L.nr_distortion_workspace_bytes(0) == 0

    def call(weights=p, z=p, B=4, S=8, near=2.0, far=6.0, loss=p, ws=p):
        return L.nr_distortion_loss(weights, z, B, S, near, far, 1.0, loss, None, None, ws, None)

    for kw in (dict(B=0), dict(B=-3), dict(S=0), dict(S=4097), dict(far=2.0), dict(near=6.0, far=2.0),
               dict(weights=None), dict(z=None), dict(loss=None), dict(ws=None)):
        assert call(**kw) == -22, kw
        assert "nr_distortion_loss" in _hip.last_error(), kw
