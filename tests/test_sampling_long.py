"""GPU parity of the long-ray sampler: nr_sample_hierarchical at 512 < Nc + Nf <= 4096 and
nr_sample_pdf at 513 < Nb <= 4097 (one workgroup per ray, sorted in runs of 512) vs the
oracle on identical inputs, and the render / training step on top of it at 256 + 512.

Weights are ``rand + 0.5``: an error in a cdf value is amplified by bin width / bin mass,
and with ``rand + 0.05`` (test_parity_ops) a CPU model of the kernel's fp32 arithmetic is
8.7e-5 from the oracle at 2048 + 2048, which leaves the project's 1e-4 no margin; with
``rand + 0.5`` it is 2.0e-5 there and 7e-6 at 256 + 512.  Tolerance: the project's 1e-4.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import refimpl as ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
DEV = "cuda"
B = 37  # not a multiple of the short path's four rays per workgroup
SIZES = [(256, 257), (256, 512), (600, 100), (3, 1021), (2048, 2048)]


def _gt_poses():
    f = sorted(GOLDEN.glob("final_poses_*.npz"))[0]
    return torch.from_numpy(np.load(f)["ground_truth_poses"])


def _rays(n, seed=0, hw=100):
    """Lego-like rays: camera poses from the reference's GT poses fixture."""
    g = torch.Generator().manual_seed(seed)
    poses = _gt_poses()
    focal = 0.5 * hw / np.tan(0.5 * 0.6911112070083618)
    dirs = ref.get_ray_directions(hw, hw, focal).reshape(-1, 3)
    img = torch.randint(0, 100, (n,), generator=g)
    pix = torch.randint(0, hw * hw, (n,), generator=g)
    o, d = zip(*[ref.get_rays(dirs[pix[b]], poses[img[b]]) for b in range(n)])
    return torch.stack(o), torch.stack(d), g


def _inputs(Nc, Nf, seed=3):
    o, d, _ = _rays(B, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    tr = torch.rand(B, Nc, generator=g)
    _, z = ref.sample_along_rays(o, d, 2.0, 6.0, Nc, t_rand=tr)
    w = torch.rand(B, Nc, generator=g) + 0.5
    u = torch.rand(B, Nf, generator=g)
    return o, d, z.contiguous(), w, u


def _hip_hier(o, d, z, w, Nf, det, u):
    from noisy_src import rays
    pts, zf = rays.sample_hierarchical(o.to(DEV), d.to(DEV), z.to(DEV), w.to(DEV), Nf, det=det,
                                       u=None if det else u.to(DEV))
    return pts.cpu(), zf.cpu()


def _coarse_places(zf, z):
    """For each row, the places in the sorted row ``zf`` of the coarse depths ``z`` (the k-th
    of equal coarse depths takes the k-th of the equal entries), by searchsorted."""
    zs = torch.sort(z, dim=-1).values.contiguous()
    first = torch.searchsorted(zs, zs, right=False)
    occ = torch.arange(zs.shape[-1]).expand_as(zs) - first
    pos = torch.searchsorted(zf.contiguous(), zs, right=False) + occ
    return zs, pos


def _assert_hier(pts, zf, wpts, wzf, z):
    assert zf.shape == wzf.shape and pts.shape == wpts.shape
    assert torch.all(zf[:, 1:] >= zf[:, :-1])
    ez, ep = (zf - wzf).abs().max().item(), (pts - wpts).abs().max().item()
    print(f"max|zf - oracle| {ez:.3e}  max|pts - oracle| {ep:.3e}")
    assert ez < 1e-4
    assert ep < 1e-4
    zs, pos = _coarse_places(zf, z)
    assert pos.max() < zf.shape[-1]
    assert torch.equal(torch.gather(zf, -1, pos), zs)  # every coarse depth, bit for bit


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_sample_hierarchical_long(Nc, Nf, det):
    o, d, z, w, u = _inputs(Nc, Nf)
    pts, zf = _hip_hier(o, d, z, w, Nf, det, u)
    wpts, wzf = ref.sample_hierarchical(o, d, z, w, Nf, det=det, u=None if det else u)
    _assert_hier(pts, zf, wpts, wzf, z)


@pytest.mark.parametrize("det", [True, False])
def test_sample_hierarchical_long_any_input_order(det):
    """Coarse depths (and their weights) reversed in every second row: the output is the
    sorted multiset whatever the input order.  Sorting is 1-Lipschitz in the max norm, so
    the 1e-4 bound on the samples carries over to the sorted rows."""
    Nc, Nf = 256, 512
    o, d, z, w, u = _inputs(Nc, Nf, seed=5)
    z, w = z.clone(), w.clone()
    z[1::2] = z[1::2].flip(-1)
    w[1::2] = w[1::2].flip(-1)
    z, w = z.contiguous(), w.contiguous()
    pts, zf = _hip_hier(o, d, z, w, Nf, det, u)
    wpts, wzf = ref.sample_hierarchical(o, d, z, w, Nf, det=det, u=None if det else u)
    _assert_hier(pts, zf, wpts, wzf, z)


def test_sample_hierarchical_long_duplicates():
    """u takes only 8 distinct values per row, so the fine samples are full of exact ties:
    the ranks of equal values must still be distinct (a permutation), i.e. the row is the
    sorted multiset of the coarse depths and exactly Nf samples."""
    Nc, Nf = 256, 512
    o, d, z, w, _ = _inputs(Nc, Nf, seed=7)
    g = torch.Generator().manual_seed(8)
    vals = torch.rand(B, 8, generator=g)
    u = torch.gather(vals, -1, torch.randint(0, 8, (B, Nf), generator=g))
    _, zf = _hip_hier(o, d, z, w, Nf, False, u)
    assert torch.all(zf[:, 1:] >= zf[:, :-1])
    zs, pos = _coarse_places(zf, z)
    assert pos.max() < Nc + Nf
    assert torch.equal(torch.gather(zf, -1, pos), zs)
    keep = torch.ones(B, Nc + Nf, dtype=torch.bool)
    keep.scatter_(-1, pos, False)
    assert torch.all(keep.sum(-1) == Nf)  # the coarse depths took Nc distinct places
    s = zf[keep].reshape(B, Nf)  # already sorted: a subsequence of a sorted row
    want_s = ref.sample_pdf(0.5 * (z[:, 1:] + z[:, :-1]), w[:, 1:-1], Nf, det=False, u=u)
    assert len(torch.unique(want_s[0])) <= 8
    assert (s - torch.sort(want_s, dim=-1).values).abs().max() < 1e-4
    assert torch.equal(zf, torch.sort(torch.cat([z, s], -1), dim=-1).values)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("Ns", [1, 130])
@pytest.mark.parametrize("Nb", [514, 1366, 4097])
def test_sample_pdf_long(Nb, Ns, det):
    from noisy_src import rays
    g = torch.Generator().manual_seed(2)
    n = 5
    bins = torch.sort(torch.rand(n, Nb, generator=g) * 4 + 2, dim=-1).values
    w = torch.rand(n, Nb - 1, generator=g) + 0.5
    u = torch.rand(n, Ns, generator=g)
    got = rays.sample_pdf(bins.to(DEV), w.to(DEV), Ns, det=det, u=None if det else u.to(DEV)).cpu()
    want = ref.sample_pdf(bins, w, Ns, det=det, u=None if det else u)
    err = (got - want).abs().max().item()
    print(f"max|samples - oracle| {err:.3e}")
    assert got.shape == want.shape and err < 1e-4


@pytest.mark.parametrize("det", [True, False])
def test_sample_pdf_long_zero_weights(det):
    """All-zero weights: the uniform pdf over 1365 bins."""
    from noisy_src import rays
    g = torch.Generator().manual_seed(21)
    n, Nb, Ns = 5, 1366, 130
    bins = torch.sort(torch.rand(n, Nb, generator=g) * 4 + 2, dim=-1).values
    w = torch.zeros(n, Nb - 1)
    u = torch.rand(n, Ns, generator=g)
    got = rays.sample_pdf(bins.to(DEV), w.to(DEV), Ns, det=det, u=None if det else u.to(DEV)).cpu()
    want = ref.sample_pdf(bins, w, Ns, det=det, u=None if det else u)
    assert (got - want).abs().max() < 1e-4


def _valid_small_call():
    from noisy_src import rays
    o, d, z, w, u = _inputs(64, 128, seed=11)
    pts, zf = rays.sample_hierarchical(o.to(DEV), d.to(DEV), z.to(DEV), w.to(DEV), 128, u=u.to(DEV))
    wpts, wzf = ref.sample_hierarchical(o, d, z, w, 128, u=u)
    assert (zf.cpu() - wzf).abs().max() < 1e-4 and (pts.cpu() - wpts).abs().max() < 1e-4


def test_refusals_name_the_limit():
    from noisy_src import rays
    o, d, z, w, u = _inputs(2048, 2049)
    with pytest.raises(RuntimeError, match="4096"):
        rays.sample_hierarchical(o.to(DEV), d.to(DEV), z.to(DEV), w.to(DEV), 2049, u=u.to(DEV))
    _valid_small_call()
    bins = torch.sort(torch.rand(2, 4098) * 4 + 2, dim=-1).values
    with pytest.raises(RuntimeError, match="4097"):
        rays.sample_pdf(bins.to(DEV), torch.rand(2, 4097).to(DEV), 16, det=True)
    _valid_small_call()


def test_viewdirs_output_long():
    from noisy_src import ops
    Nc, Nf = 256, 512
    o, d, z, w, u = _inputs(Nc, Nf, seed=13)
    d = d * (1 + 0.1 * torch.rand(B, 1, generator=torch.Generator().manual_seed(14)))  # |d| != 1
    od, dd = o.to(DEV), d.to(DEV)
    pts, zf, vd = ops.sample_hierarchical(od, dd, z.to(DEV), w.to(DEV), Nf, u=u.to(DEV), viewdirs=True)
    assert torch.equal(vd, ops.expand_viewdirs(dd, Nc + Nf))
    assert (pts - (od[:, None, :] + dd[:, None, :] * zf[..., None])).abs().max() <= 1e-6


# ---------------------------------------------------------------- end to end, 256 + 512
E2E_RAYS = 64


def _nets(precision="fp32", seed=0):
    from noisy_src.config import ModelConfig
    from noisy_src.model import create_nerf
    cfg = ModelConfig(precision=precision)
    torch.manual_seed(seed)
    oc, of = ref.create_nerf(cfg)
    torch.manual_seed(seed)
    mc, mf = create_nerf(cfg)
    mc.load_state_dict(oc.state_dict())
    mf.load_state_dict(of.state_dict())
    return oc, of, mc.to(DEV), mf.to(DEV)


def _rcfg():
    from noisy_src.config import RenderConfig
    return RenderConfig(num_samples=256, num_samples_fine=512)


def _e2e_batch(seed):
    o, d, g = _rays(E2E_RAYS, seed=seed, hw=80)
    tgt = torch.rand(E2E_RAYS, 3, generator=g)
    tr, u = torch.rand(E2E_RAYS, 256, generator=g), torch.rand(E2E_RAYS, 512, generator=g)
    return o, d, tgt, tr, u


@pytest.fixture(scope="module")
def oracle_step():
    """One reference train step (fp32, CPU) at 64 rays x (256 + 512), computed once."""
    oc, of, _, _ = _nets()
    o, d, tgt, tr, u = _e2e_batch(31)
    return ref.train_step(oc, of, ref.TrainState(oc, of), o, d, tgt, _rcfg(), t_rand=tr, u=u)


@pytest.mark.parametrize("is_train", [True, False])
def test_render_rays_long(is_train):
    from noisy_src.rendering import render_rays
    oc, of, mc, mf = _nets()
    o, d, _, tr, u = _e2e_batch(30)
    rc = _rcfg()
    with torch.no_grad():
        got = render_rays(mc, mf, o.to(DEV), d.to(DEV), rc, is_train=is_train, t_rand=tr.to(DEV), u=u.to(DEV))
        want = ref.render_rays(oc, of, o, d, rc, is_train=is_train, t_rand=tr, u=u)
    errs = {k: (got[k].cpu() - want[k]).abs().max().item()
            for k in ("rgb_coarse", "rgb_fine", "depth_coarse", "depth_fine", "acc_coarse", "acc_fine")}
    print(errs)
    for k, e in errs.items():
        assert e < (1e-4 if "rgb" in k or "acc" in k else 5e-4), (k, e)


def test_train_step_long_matches_oracle(oracle_step):
    from noisy_src.engine import Trainer
    _, _, mc, mf = _nets()
    o, d, tgt, tr, u = _e2e_batch(31)
    got = Trainer(mc, mf, _rcfg()).step(o.to(DEV), d.to(DEV), tgt.to(DEV), t_rand=tr.to(DEV), u=u.to(DEV))
    want = oracle_step
    print(got["loss"].item(), want["loss"], got["loss_fine"].item(), want["loss_fine"])
    assert abs(got["loss"].item() - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
    assert abs(got["loss_fine"].item() - want["loss_fine"]) < 1e-5


# Drift of a 16-bit step from the fp32 oracle, in the form test_parity_fullsize holds it to:
# the recorded value times a 1.5 margin.  Recorded for bf16: rgb maps within 1.038e-4 of
# the fp32 oracle (cfg #2; 9.2e-5 for cfg #4).  A composited colour is a weighted mean of
# the samples' colours (weights sum to <= 1), so its error does not grow with the samples
# per ray; and with |rgb - target| <= 1, loss = mean((rgb - target)^2) moves by at most
# 2 e + e^2 when every rgb moves by at most e.
DRIFT_MARGIN = 1.5
BF16_RGB_DRIFT_RECORDED = 1.038e-4


def test_train_step_long_bf16(oracle_step):
    from noisy_src.engine import Trainer
    _, _, mc, mf = _nets("bf16")
    o, d, tgt, tr, u = _e2e_batch(31)
    got = Trainer(mc, mf, _rcfg()).step(o.to(DEV), d.to(DEV), tgt.to(DEV), t_rand=tr.to(DEV), u=u.to(DEV))
    loss, loss_f = got["loss"].item(), got["loss_fine"].item()
    print(loss, loss_f, oracle_step["loss_fine"])
    assert np.isfinite(loss) and np.isfinite(loss_f)
    e = DRIFT_MARGIN * BF16_RGB_DRIFT_RECORDED
    assert abs(loss_f - oracle_step["loss_fine"]) < 2 * e + e * e
