"""Worker of tests/test_feature_interaction.py::test_graphed_pose_trainer_with_every_feature_equals_eager:
``GraphedPoseTrainer`` over the all-on ``PoseTrainer`` of tests/feature_interaction_ref.py
(coarse-to-fine window, learned focal length in mode "xy", Cauchy loss, distortion term, live
rotations; bf16), in a process of its own.

Six steps (frozen, frozen, then four optimising; warmup=0: the first step of each shape runs
eagerly because its Adam state is new, the second is captured, the rest replay) against the
eager ``PoseTrainer`` on the same batches.  ``iteration`` advances, so every step has a window
of its own, and the focal length moves on every optimising step: a replay only matches the
eager step if it reads the window tensors, (fx, fy) and both loss words per network from
device memory and not from the captured launch.  Every returned metric is compared, the
robust step's ``mse_*`` and ``loss_distortion`` among them.

Then the one case in which only ``GraphedPoseTrainer``'s own bookkeeping keeps an inference
forward right: an inference forward with frozen parameters (it folds, and the network remembers
that its images are folded for this window), a seventh step replayed with ``iteration=None`` (the window does not
change, so the window version the fold is keyed on does not either, and the replayed Adam
rewrites the images unfolded without the host seeing it), and a second inference forward, which
must fold again.  After any of the six steps before it the window version has moved, and an
inference forward would refold whatever the replay left behind.  Both forwards are compared
with the eager trainer's.
Writes ``<out>/feature_interaction_graph_report.json``.
"""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd"), str(ROOT / "tests")]

import torch  # noqa: E402

import feature_interaction_ref as X  # noqa: E402

SEQUENCE = (False, False, True, True, True, True)
FRACS = (0.34, 0.44, 0.54, 0.64, 0.74, 0.84)  # alpha = 3.4 ... 8.4 of L = 10: a new band at every step
METRICS = ("loss", "loss_coarse", "loss_fine", "mse_coarse", "mse_fine", "loss_distortion", "rgb_fine")


def _state(tr):
    params = torch.cat([tr.model_coarse.flat_params(), tr.model_fine.flat_params()]).cpu()
    poses = torch.cat([p.detach().reshape(-1).cpu() for p in tr.camera_params.parameters()])
    return params, poses, tr.intrinsics.log_scale.detach().cpu().clone()


def _eval(tr, dev):
    """An inference forward of both networks with their parameters frozen for its duration, as
    ``PoseRefiner`` or a renderer over a loaded checkpoint runs them: the fused MLP folds on every
    forward whose parameters need a gradient, and consults its fold key only on this path."""
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(300, 3, generator=g) * 3 - 1.5).to(dev)
    d = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=-1).to(dev)
    nets = (tr.model_coarse, tr.model_fine)
    params = [p for net in nets for p in net.parameters()]
    for p in params:
        p.requires_grad_(False)
    try:
        with torch.no_grad():
            return torch.cat([torch.cat(net(x, d), dim=-1) for net in nets]).cpu()
    finally:
        for p in params:
            p.requires_grad_(True)


def main():
    from noisy_src.engine import GraphedPoseTrainer
    out = Path(sys.argv[1])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sc = X.scene()
    eager, tr_g = (X.device_trainer(sc, "bf16", dev, fracs=FRACS) for _ in range(2))
    g = torch.Generator().manual_seed(700)
    data = [X.device_batch(X.draw_batch(sc.images, g), dev) for _ in SEQUENCE]
    graphed = GraphedPoseTrainer(tr_g, *data[0], warmup=0)
    unequal, captured_window, after_focal, after_window, windows = [], {}, 0, 0, set()
    for k, ((batch, t_rand, u), opt) in enumerate(zip(data, SEQUENCE)):
        me = eager.step(batch, optimize_poses=opt, t_rand=t_rand, u=u, iteration=k)
        me = {n: me[n].detach().cpu().clone() for n in METRICS}
        replayed = opt in graphed._graphs
        moved = bool(tr_g.intrinsics.log_scale.detach().cpu().ne(sc.state.log_scale).any())
        mg = graphed.step(batch, optimize_poses=opt, t_rand=t_rand, u=u, iteration=k)
        assert set(METRICS) <= set(mg), sorted(mg)
        mg = {n: mg[n].detach().cpu().clone() for n in METRICS}
        unequal += [(k, n) for n in METRICS if not torch.equal(me[n], mg[n])]
        win = tuple(tr_g.model_fine.pe_window()[0])
        assert tr_g.model_fine.pe_window() == eager.model_fine.pe_window()
        windows.add(win)
        if opt in graphed._graphs and not replayed:
            captured_window[opt] = win  # this call captured (and replayed once under the capture's window)
        after_focal += int(replayed and opt and moved)
        after_window += int(replayed and win != captured_window[opt])
    # an inference forward, a replay under the same window, an inference forward
    eval_before = bool(torch.equal(_eval(eager, dev), _eval(tr_g, dev)))
    folded_for = [n._fold_key for n in (tr_g.model_coarse, tr_g.model_fine)]
    batch, t_rand, u = X.device_batch(X.draw_batch(sc.images, g), dev)
    version = tr_g.model_fine._pe_window.version
    me = eager.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    assert True in graphed._graphs
    mg = graphed.step(batch, optimize_poses=True, t_rand=t_rand, u=u)
    unequal += [(len(SEQUENCE), n) for n in METRICS if not torch.equal(me[n].cpu(), mg[n].cpu())]
    same_window = tr_g.model_fine._pe_window.version == version and tr_g.model_fine.pe_window() == eager.model_fine.pe_window()
    # the host's view of the images did not change over the replay: only the replay's own mark tells the fold is gone
    same_images = all(k is not None and n._packed_key == k[0]
                      for n, k in zip((tr_g.model_coarse, tr_g.model_fine), folded_for))
    eval_after = bool(torch.equal(_eval(eager, dev), _eval(tr_g, dev)))
    torch.cuda.synchronize()
    (pa, qa, fa), (pb, qb, fb) = _state(eager), _state(tr_g)
    rep = dict(captured=sorted(graphed._graphs), metrics_unequal=unequal, params_equal=bool(torch.equal(pa, pb)),
               poses_equal=bool(torch.equal(qa, qb)), log_scale_equal=bool(torch.equal(fa, fb)),
               eval_equal_before_the_unseen_replay=eval_before, eval_equal_after_the_unseen_replay=eval_after,
               window_unchanged_over_the_unseen_replay=bool(same_window), images_key_unchanged_over_it=bool(same_images),
               log_scale=fb.tolist(), log_scale_moved=float((fb - sc.state.log_scale).abs().min()),
               rotations_moved=float((tr_g.camera_params.rotation_deltas.detach().cpu() - sc.state.rot).abs().max()),
               windows_distinct=len(windows), replays_after_a_focal_update=after_focal,
               replays_after_a_window_change=after_window)
    (out / "feature_interaction_graph_report.json").write_text(json.dumps(rep, indent=1))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
