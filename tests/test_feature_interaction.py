"""GPU: the joint pose-optimisation step with every optional feature switched on together --
coarse-to-fine window, learned focal length ("xy"), Cauchy loss and distortion term, with live
rotations -- against the one fp64 restatement of tests/feature_interaction_ref.py, whose
inputs test_feature_interaction_host.py shows to tell a dropped feature from a working one
(every feature moves every gradient it reaches by at least 1e-2).

Each feature's own tests switch on that feature alone; here the code between them is held:
the distortion gradient that reaches the network through ``weights`` beside the robust seed
(and ``nr_mlp_window_grad`` after it), the focal gradient fed by a ``g_rays_d`` of three
sources, the refold of the images the fused Adam rewrote under a window that has moved, and
the metrics a step (or a graph replay) returns.

Bounds, all taken from the per-feature tests:

* fp32, both networks' flat gradients: relative 2-norm below 1e-3 of the fp32 oracle
  (test_distortion.py);
* fp32, rotation, translation and log_scale gradients: ``ours < 2 x torch32 + 1e-3`` against
  fp64, torch32 the fp32 oracle's own distance (test_pose_rotation.py, test_learn_focal.py);
* metrics: 1e-5 relative, the distortion term 1e-4 (test_distortion.py); ``loss`` equals the
  sum of the step's own metrics and the regularisers to 1e-6 absolute;
* bf16, camera gradients: ``ours <= max(0.5 x D16, 2e-2)`` against the oracle rendered over
  ``ref.mfma_emulated_nerf`` of the folded oracle, D16 that model's distance from the fp32
  oracle (test_pose_gradient_through_render_live_rotation_bf16).

The second step runs after the fused Adam has rewritten the images unfolded and the poses and
the focal length have moved, under a window with one more band open; it is compared with the
restatement at the trainer's state read back after the first step, so a step that folded with
the first step's window (or not at all), or read the first step's (fx, fy) or poses, shows.  (A
fold that is stale because the HOST did not see the images change -- a graph replay -- is the
worker's business: it runs an inference forward, a replay under an unchanged window and a second
inference forward.)  With ``NR_WRITE_PROFILES`` set the measured distances go to
profiles/feature_interaction_parity.json.

Measured on an MI355X (profiles/feature_interaction_parity.json), nothing near its bound:
fp32 network gradients 4e-7 to 9e-7 of the fp32 oracle (bound 1e-3); fp32 camera gradients
6e-8 to 1.2e-6 of fp64 over both steps (torch32 1.5e-7 to 9e-7, so the bound is 1e-3); metrics
4e-9 to 1.4e-7 relative, the loss identity 4e-9 absolute; bf16 camera gradients 3e-5 to 4.4e-4
of the numerics model (D16 3.6e-3 to 3.7e-2, so the bound is 2e-2).

Relations that need no oracle: the hipGraph replay (tests/feature_interaction_graph_worker.py),
``Trainer(coarse_stream=True)`` with both extras, and ``PoseRefiner`` against the training
path's pose gradient."""
import copy
import functools
import json
import os
import subprocess
import sys
from dataclasses import replace
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import feature_interaction_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
SCALARS = ("loss_coarse", "loss_fine", "mse_coarse", "mse_fine", "loss_distortion")
# the pose learning rate of the two-step run: one Adam step then moves the deltas and log_scale
# by 5e-2, not by the default 1e-4, so that a second step computed from the first step's poses
# or (fx, fy) has EVERY gradient off by over ten times the comparison floor
# (test_second_step_saw_a_moved_state asserts it on the restatement; at 1e-2 the stale (fx, fy)
# moved the two network gradients by 8e-3 only); the first step's gradients do not depend on it
POSE_LR = 5e-2
_records = []


@pytest.fixture(scope="module", autouse=True)
def _write_profile():
    yield
    if os.environ.get("NR_WRITE_PROFILES") and _records:
        (ROOT / "profiles" / "feature_interaction_parity.json").write_text(json.dumps(
            {"bounds": {"networks_fp32": "rel 2-norm vs the fp32 oracle < 1e-3",
                        "camera_fp32": "rel 2-norm vs fp64 < 2 x torch32 + 1e-3",
                        "camera_bf16": "rel 2-norm vs the bf16 numerics model <= max(0.5 x D16, 2e-2)"},
             "cases": _records}, indent=1) + "\n")


def _record(**kw):
    _records.append(kw)
    print("FEATURE_INTERACTION_PARITY " + json.dumps(kw))


@functools.lru_cache(maxsize=None)
def _scene():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return X.scene()


def _capture(trainer, store):
    """The gradients as the optimizers' ``step`` receives them (before the fused clip)."""
    nerf, poses = trainer.optimizer_nerf.step, trainer.optimizer_poses.step
    cam, intr = trainer.camera_params, trainer.intrinsics

    def nerf_step(*a, **k):
        store["coarse"], store["fine"] = (X.flat_grad(n).clone() for n in (trainer.model_coarse, trainer.model_fine))
        return nerf(*a, **k)

    def pose_step(*a, **k):
        store["rotation"], store["translation"] = cam.rotation_deltas.grad.clone(), cam.translation_deltas.grad.clone()
        store["log_scale"] = intr.log_scale.grad.clone()
        return poses(*a, **k)

    trainer.optimizer_nerf.step, trainer.optimizer_poses.step = nerf_step, pose_step


@functools.lru_cache(maxsize=None)
def _two_steps(precision):
    """Two optimising steps of the all-on trainer (iteration 0: the scene's window, iteration 1:
    one more band) on the scene's batch.  Per step: the state the step started from, the
    captured gradients and the metrics."""
    sc = _scene()
    tr = X.device_trainer(sc, precision, DEV, pose_lr=POSE_LR)
    batch, t_rand, u = X.device_batch(sc, DEV)
    grads = {}
    _capture(tr, grads)
    steps = []
    for k, frac in enumerate((X.FRAC, X.FRAC_NEXT)):
        state = X.read_state(tr, X.window(frac, sc.cfg))
        m = tr.step(batch, optimize_poses=True, t_rand=t_rand, u=u, iteration=k)
        assert tuple(tr.model_fine.pe_window()[0]) == tuple(state.window[0])
        steps.append(dict(state=state, grads={n: g.cpu() for n, g in grads.items()},
                          metrics={n: float(m[n]) for n in SCALARS + ("loss",)}))
        grads.clear()
    return steps


@functools.lru_cache(maxsize=None)
def _oracles(step, precision):
    """The restatement at the state ``_two_steps(precision)[step]`` started from: fp64, fp32
    and (bf16 only) over the numerics model.  Step 0 starts from the scene's own state."""
    sc = _scene()
    state = _two_steps(precision)[step]["state"]
    out = {"f64": X.restate(sc, state), "f32": X.restate(sc, state, X.F32)}
    if precision == "bf16":
        out["emu"] = X.restate(sc, state, X.F32, emulate="bf16")
    return out


def test_first_step_starts_from_the_scene():
    sc, st = _scene(), _two_steps("fp32")[0]["state"]
    assert torch.equal(st.rot, sc.state.rot) and torch.equal(st.trans, sc.state.trans)
    assert torch.equal(st.log_scale, sc.state.log_scale) and st.window == sc.state.window
    assert all(torch.equal(st.fine[k], v) for k, v in sc.state.fine.items())


# ------------------------------------------- 2 + 3. the step against the restatement, fp32 --
@pytest.mark.parametrize("step", [0, 1], ids=["first_step", "second_step_refolded"])
def test_fp32_step_matches_the_restatement(step):
    got, want = _two_steps("fp32")[step], _oracles(step, "fp32")
    g, g32, g64 = got["grads"], want["f32"]["grads"], want["f64"]["grads"]
    nets = {k: X.rel(g[k], g32[k]) for k in ("coarse", "fine")}
    ours = {k: X.rel(g[k], g64[k]) for k in X.CAMERA}
    torch32 = {k: X.rel(g32[k], g64[k]) for k in X.CAMERA}
    m, m64 = got["metrics"], want["f64"]["metrics"]
    scalars = {k: abs(m[k] - m64[k]) / m64[k] for k in SCALARS}
    scalars["loss"] = abs(m["loss"] - want["f64"]["loss"]) / want["f64"]["loss"]
    st = got["state"]
    regs = X.ROT_REG * float(st.rot.double().pow(2).mean()) + X.TRANS_REG * float(st.trans.double().pow(2).mean())
    identity = abs(m["loss"] - (m["loss_coarse"] + m["loss_fine"] + X.WEIGHT * m["loss_distortion"] + regs))
    _record(test="step_fp32", step=step, networks_vs_fp32_oracle=nets, camera_ours=ours, camera_torch32=torch32,
            metrics_rel=scalars, loss_identity_abs=identity)
    for k in X.CAMERA:
        assert int(torch.count_nonzero(g[k])) == g[k].numel(), k
    for k, d in nets.items():
        assert d < 1e-3, (k, d)
    for k in X.CAMERA:
        assert ours[k] < 2 * torch32[k] + 1e-3, (k, ours[k], torch32[k])
    for k, d in scalars.items():
        assert d < (1e-4 if k == "loss_distortion" else 1e-5), (k, d)
    assert identity < 1e-6, identity


def test_second_step_saw_a_moved_state():
    """The second comparison only means a refold if the first step moved what it reads."""
    a, b = (s["state"] for s in _two_steps("fp32"))
    assert not torch.equal(a.rot, b.rot) and not torch.equal(a.trans, b.trans)
    assert bool((a.log_scale != b.log_scale).all())
    assert a.window != b.window and b.window[0][3] == 1.0 and 0.0 < b.window[0][4] < 1.0
    col = a.fine["pts_linears.0.weight"][:, 3:3 + 6 * 4], b.fine["pts_linears.0.weight"][:, 3:3 + 6 * 4]
    assert not torch.equal(*col)  # the open bands' columns were rewritten by the fused Adam
    # and the restatement tells each stale input from the current one by ten times the floor on
    # every gradient: the old window, no window at all (images left unfolded), the old focal
    # length and the old poses
    sc, want = _scene(), _oracles(1, "fp32")["f64"]["grads"]
    shares = {}
    for name, stale in (("window", replace(b, window=a.window)), ("unfolded", replace(b, window=(None, None))),
                        ("fxy", replace(b, log_scale=a.log_scale)), ("poses", replace(b, rot=a.rot, trans=a.trans))):
        g = X.restate(sc, stale)["grads"]
        shares[name] = {k: X.rel(g[k], want[k]) for k in X.GRADS}
    print("FEATURE_INTERACTION_STALE " + json.dumps(shares))
    for name, share in shares.items():
        assert min(share.values()) > 1e-2, (name, share)


# ------------------------------------------------------------------------------- bf16 --
@pytest.mark.parametrize("step", [0, 1], ids=["first_step", "second_step_refolded"])
def test_bf16_camera_gradients_match_the_numerics_model(step):
    got, want = _two_steps("bf16")[step], _oracles(step, "bf16")
    g, g16, g32 = got["grads"], want["emu"]["grads"], want["f32"]["grads"]
    ours = {k: X.rel(g[k], g16[k]) for k in X.CAMERA}
    d16 = {k: X.rel(g16[k], g32[k]) for k in X.CAMERA}
    _record(test="step_bf16", step=step, camera_ours=ours, camera_D16=d16)
    for k in X.CAMERA:
        assert int(torch.count_nonzero(g16[k])) == g16[k].numel(), k
        assert ours[k] <= max(0.5 * d16[k], 2e-2), (k, ours[k], d16[k])


# ----------------------------------------------------------------------- the frozen shape --
def test_frozen_step_leaves_no_camera_gradient_and_matches_the_restatement():
    sc = _scene()
    tr = X.device_trainer(sc, "fp32", DEV)
    batch, t_rand, u = X.device_batch(sc, DEV)
    grads = {}
    _capture(tr, grads)
    m = tr.step(batch, optimize_poses=False, t_rand=t_rand, u=u, iteration=0)
    assert set(grads) == {"coarse", "fine"}  # the pose Adam did not step
    assert tr.camera_params.rotation_deltas.grad is None and tr.camera_params.translation_deltas.grad is None
    assert tr.intrinsics.log_scale.grad is None
    after = X.read_state(tr, sc.state.window)
    assert torch.equal(after.rot, sc.state.rot) and torch.equal(after.log_scale, sc.state.log_scale)
    want = X.restate(sc, dtype=X.F32, optimize_poses=False)
    nets = {k: X.rel(grads[k], want["grads"][k]) for k in ("coarse", "fine")}
    loss = abs(float(m["loss"]) - want["loss"]) / want["loss"]
    _record(test="frozen_fp32", networks_vs_fp32_oracle=nets, loss_rel=loss)
    for k, d in nets.items():
        assert d < 1e-3, (k, d)
    assert loss < 1e-5
    assert float(m["loss"]) == float(m["loss_coarse"] + m["loss_fine"] + X.WEIGHT * m["loss_distortion"])


# ------------------------------------------------------- 4. relations that need no oracle --
def test_graphed_pose_trainer_with_every_feature_equals_eager(tmp_path):
    """A fresh child (tests/feature_interaction_graph_worker.py): frozen x 2 then optimising x 4,
    graphed against eager with a window that changes at every step and a focal length that
    changes on every optimising step; parameters, poses, log_scale and every returned metric
    (``mse_*`` and ``loss_distortion`` among them) bit for bit, both graphs captured.  Then an
    inference forward, one more replay under the same window and a second inference forward,
    which only matches the eager trainer's if the replay marked the images as unfolded."""
    subprocess.run([sys.executable, str(ROOT / "tests" / "feature_interaction_graph_worker.py"), str(tmp_path)],
                   check=True, timeout=300)
    r = json.loads((tmp_path / "feature_interaction_graph_report.json").read_text())
    assert r["captured"] == [False, True], r
    assert r["metrics_unequal"] == [], r
    assert r["params_equal"] and r["poses_equal"] and r["log_scale_equal"], r
    # the replay under an unchanged window, between two inference forwards: the second one folded again
    assert r["window_unchanged_over_the_unseen_replay"] and r["images_key_unchanged_over_it"], r
    assert r["eval_equal_before_the_unseen_replay"] and r["eval_equal_after_the_unseen_replay"], r
    assert r["log_scale_moved"] > 0 and r["rotations_moved"] > 0, r
    assert r["replays_after_a_focal_update"] >= 2 and r["replays_after_a_window_change"] >= 2, r
    assert r["windows_distinct"] == 6, r


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_coarse_stream_with_both_extras_equals_one_stream(precision):
    """test_coarse_stream.py's claim with the robust loss and the distortion term both on (the
    term joins the fine chain on the main stream, the summed loss is built on the coarse one):
    two steps, every metric, the parameters and the Adam state bit for bit."""
    from noisy_src.engine import Trainer
    sc = _scene()
    g = torch.Generator().manual_seed(23)
    batches = []
    for _ in range(2):
        o = torch.randn(X.RAYS, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
        d = torch.nn.functional.normalize(torch.randn(X.RAYS, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1)
        batches.append([t.to(DEV) for t in (o, d, torch.rand(X.RAYS, 3, generator=g), torch.rand(X.RAYS, X.NC, generator=g),
                                            torch.rand(X.RAYS, X.NF, generator=g))])
    trainers = []
    for cs in (False, True):
        mc, mf = X.device_nets(sc, precision, DEV)
        trainers.append(Trainer(mc, mf, sc.rc, coarse_stream=cs, loss=X.KIND, loss_scale=X.C, distortion_weight=X.WEIGHT))
    one, two = trainers
    for k, b in enumerate(batches):
        m1, m2 = one.step(*b), two.step(*b)
        assert not one.last_step_coarse_stream and two.last_step_coarse_stream
        assert set(m1) == set(m2) and {"mse_coarse", "mse_fine", "loss_distortion"} <= set(m1)
        for name in m1:
            assert torch.equal(m1[name], m2[name]), (k, name)
        assert float(m1["loss"]) == float(m1["loss_coarse"] + m1["loss_fine"] + X.WEIGHT * m1["loss_distortion"])
    for na, nb in ((one.model_coarse, two.model_coarse), (one.model_fine, two.model_fine)):
        assert torch.equal(na.flat_params(), nb.flat_params())
    sa, sb = list(one.optimizer._flat_state.values()), list(two.optimizer._flat_state.values())
    assert len(sa) == len(sb) > 0
    for (ma, va), (mb, vb) in zip(sa, sb):
        assert torch.equal(ma, mb) and torch.equal(va, vb)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_refiner_on_windowed_networks_leaves_the_training_paths_pose_gradient(precision):
    """``PoseRefiner(loss="cauchy", fxy=<the learned pair>)`` on networks that carry the window
    (frozen parameters: ``nr_mlp_forward_frozen`` / ``nr_mlp_backward_input``) against
    ``PoseTrainer`` over the same state with its regularisers and the distortion weight at 0
    (live parameters: the training kernels, as test_pose_refine.py selects them): the MLP's
    input gradients are identical, and everything downstream of them is the same kernels on
    the same inputs, so the pose gradients agree bit for bit."""
    from noisy_src.engine import PoseRefiner, PoseTrainer
    sc = _scene()
    batch, t_rand, u = X.device_batch(sc, DEV)
    coarse, fine = X.device_nets(sc, precision, DEV)
    for net in (coarse, fine):
        net.set_pe_window(*sc.state.window)

    cam_t, intr, sampler = X.device_camera(sc, DEV, fixed_small_angle=True)
    trainer = PoseTrainer(copy.deepcopy(coarse), copy.deepcopy(fine), cam_t, sampler, sc.rc, rotation_reg_weight=0.0,
                          translation_reg_weight=0.0, intrinsics=intr, loss=X.KIND, loss_scale=X.C)
    assert trainer.model_fine.pe_window() == fine.pe_window()
    fxy = intr.fxy().detach().clone()  # before the step moves log_scale
    trainer.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    want = (cam_t.rotation_deltas.grad.clone(), cam_t.translation_deltas.grad.clone())
    assert all(p.grad is not None for p in trainer.model_fine.parameters())  # the training kernels ran

    cam_r, _, _ = X.device_camera(sc, DEV, fixed_small_angle=True)
    with PoseRefiner(coarse, fine, cam_r, sampler, sc.rc, fxy=fxy, loss=X.KIND, loss_scale=X.C) as refiner:
        m = refiner.step(batch, t_rand=t_rand, u=u)
        got = (cam_r.rotation_deltas.grad.clone(), cam_r.translation_deltas.grad.clone())
    assert "mse_fine" in m and all(p.grad is None for p in fine.parameters())
    for name, a, b in zip(("rotation", "translation"), got, want):
        assert int(torch.count_nonzero(b)) == b.numel(), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, (a - b).abs().max().item())
