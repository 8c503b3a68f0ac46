"""CPU: the inputs of the feature-interaction tests can tell a broken interaction from a working
one.  tests/feature_interaction_ref.py restates the joint pose-optimisation step with the
coarse-to-fine window, the learned focal length, the distortion term and the Cauchy loss all
switched on; test_feature_interaction.py holds ``PoseTrainer.step`` to it with a comparison
floor of 1e-3 (relative 2-norm) on every gradient.  A comparison at that floor only notices a
dropped or mis-associated feature if the feature moves the gradient by far more than the
floor, so this file pins, on the fp64 restatement alone:

* with any one feature left out, each of the five gradients (coarse network, fine network,
  rotation deltas, translation deltas, log_scale) differs from the all-on gradient by at
  least 1e-2, ten times the floor;
* the one exception is exact: the distortion term never reaches the coarse network (the fine
  samples are drawn from detached coarse weights), so that gradient is unchanged bit for bit;
* every entry of the three camera gradients is non-zero (live Rodrigues: the rotation chain
  is not dead as it is at zero deltas);
* torch's own fp32 evaluation stays far below the floor, so the floor is a statement about
  the kernels and not about the scene."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import feature_interaction_ref as X  # noqa: E402

SHARE = 1e-2  # ten times the 1e-3 floor of the device comparison


@pytest.fixture(scope="module")
def all_on():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    sc = X.scene()
    return sc, X.restate(sc)


def test_scene_is_the_one_the_issue_describes(all_on):
    sc, _ = all_on
    pos, dir_ = sc.state.window
    assert pos[:3] == [1.0, 1.0, 1.0] and 0.0 < pos[3] < 1.0 and pos[4:] == [0.0] * 6
    assert dir_[0] == 1.0 and 0.0 < dir_[1] < 1.0 and dir_[2:] == [0.0, 0.0]
    nxt = X.window(X.FRAC_NEXT, sc.cfg)[0]
    assert nxt[:4] == [1.0] * 4 and 0.0 < nxt[4] < 1.0 and nxt[5:] == [0.0] * 5  # one more band opens
    assert sc.img.unique().tolist() == [0, 1, 2] and sc.target.shape == (X.RAYS, 3)
    assert sc.state.rot.abs().min() > 0 and sc.state.trans.abs().min() > 0
    assert sc.state.log_scale.tolist() == pytest.approx(list(X.LOG_SCALE))


def test_every_camera_gradient_entry_is_live(all_on):
    _, full = all_on
    for k in X.CAMERA:
        g = full["grads"][k]
        assert g.shape == ((3, 3) if k != "log_scale" else (2,))
        assert int(torch.count_nonzero(g)) == g.numel(), (k, g)
    m = full["metrics"]
    assert m["loss_distortion"] > 0 and m["mse_coarse"] > m["loss_coarse"] > 0 and m["mse_fine"] > m["loss_fine"] > 0


@pytest.mark.parametrize("feature", X.FEATURES)
def test_leaving_one_feature_out_moves_every_gradient_it_reaches(all_on, feature):
    sc, full = all_on
    less = X.restate(X.without(sc, feature))
    shares = {k: X.rel(less["grads"][k], full["grads"][k]) for k in X.GRADS}
    print("FEATURE_SHARE", feature, {k: f"{v:.3e}" for k, v in shares.items()})
    for k, share in shares.items():
        if feature == "distortion" and k == "coarse":
            assert torch.equal(less["grads"][k], full["grads"][k])  # the one exact zero
        else:
            assert share >= SHARE, (feature, k, share)


def test_fp32_restatement_sits_far_below_the_comparison_floor(all_on):
    sc, full = all_on
    f32 = X.restate(sc, dtype=X.F32)
    for k in X.GRADS:
        d = X.rel(f32["grads"][k], full["grads"][k])
        print("FEATURE_TORCH32", k, f"{d:.3e}")
        assert d < 1e-5, (k, d)
    assert abs(f32["loss"] - full["loss"]) < 1e-6 * full["loss"]


def test_frozen_shape_has_no_camera_gradient_and_the_same_network_gradients_without_regulariser(all_on):
    sc, full = all_on
    frozen = X.restate(sc, optimize_poses=False)
    assert all(frozen["grads"][k] is None for k in X.CAMERA)
    # the regulariser does not reach the networks: their gradients are those of the optimising step
    for k in ("coarse", "fine"):
        assert torch.equal(frozen["grads"][k], full["grads"][k])
    assert frozen["loss"] < full["loss"]
