"""GPU: the per-ray kernels at their dispatch edges, each against the oracle run in fp64.

The parity tests compare every kernel with the oracle at one comfortable shape.  Here each
kernel runs at the sizes where its code takes another path, through the raw C ABI into
buffers the test owns (sentinel rows after every output, which must come back bit for bit):

  kernel / instantiation                       reached by
  -------------------------------------------  ------------------------------------------------
  composite_{fwd,bwd}_wave_kernel (S <= 512)   test_composite_vs_fp64, S = 1, 2, 63, 64 (K = 1),
    K = ceil(S / 64) samples per lane            65 (K = 2, half the lanes empty), 511, 512 (K = 8)
  composite_{fwd,bwd}_kernel (thread per ray)  test_composite_vs_fp64, S = 513
  composite_mse_wave_kernel / the long form    test_composite_mse_equals_separate, S = 1, 2, 65,
                                                 512 / 513, with and without a ticket
  a partly filled workgroup (4 rays)           B = 1 and B = 5 (one full, one with one ray) everywhere
  sample_hier_kernel<1>                        (3, 1), (3, 61) T = 64, (32, 32), (64, 1) T = 65 -> <2>
  sample_hier_kernel<2>                        (64, 1), (65, 63) T = 128, (66, 62)
  sample_hier_kernel<4>                        (129, 127) T = 256, (64, 128)
  sample_hier_kernel<8>                        (130, 127) T = 257, (256, 256) T = 512, (3, 509), (511, 1)
  lane-63 wrap of z_vals_mid                   Nc = 65, 66 (register 0 -> 1), 129, 130 (1 -> 2),
                                                 256 (.. -> 3; bins end at lane 62), 511 (.. -> 7)
  sample_pdf_kernel, build_cdf's stride of 64  Nb = 2, 3 (one and two weights), 64, 65, 66, 513 (the limit)
  stratified_kernel, linspace_at n == 1        N = 1; N = 2 (both ends, no interior); N = 64
  pe_kernel / pe_bwd_kernel                    C = 1, 3; L = 1 (n == 1), 4, 10; include_input 0 / 1;
                                                 log_sampling 0 / 1; M = 1, 257 (two workgroups)

Bounds.  Where a parity test already holds a kernel to a number, that number is used
unchanged against the fp64 oracle (1e-4 for the samplers with rand + 0.5 weights, 2e-6 / 1e-5
for the stratified depths / points, 2e-6 for the encoding where f |x| <= 64).  For the
compositing, and for the encoding at arguments of up to thousands of radians, the yardstick
is the oracle's own fp32 run against its fp64 run on the same inputs, per output tensor
(2-norm; max norm for rgb_map / depth / acc): ``err_kernel <= max(F err_oracle32,
4 2^-24 max|want|)`` with one F per kernel family, the smallest power of two that is at
least twice the largest ratio measured on an MI355X (never above 16).  Each test prints its
distances as an ``EDGE_PARITY`` line; one full run is kept in profiles/edge_shapes_parity.json.

Measured on an MI355X, err_kernel / err_oracle32 over the cases whose error is above the
floor (the median over all cases is 1.0 for every output):

  positional encoding   forward beyond 64 radians 1.00, backward 1.25            -> F_PE = 4
  composite             weights 1.29, g_rgb 1.47, depth 3.6, acc 4.8, rgb_map 5.6
                        (S = 511 .. 513, B = 5), g_sigma 4.5 (S = 64, B = 1), and
                        g_rays_d 13.7, 12.4, 4.2 -- every one at B = 1               -> F_COMPOSITE = 16

F_COMPOSITE is the cap: twice the largest ratio would ask for 32, which the rule forbids, and
every case holds under 16.  The ratios above 6 all belong to g_rays_d at B = 1.  g_rays_d of
a ray is ONE scalar, g_norm = sum_i g_x_i (-sigma_i delta_i), times d / |d| (composite.hip),
so at B = 1 the "tensor" is one fp32 number and the ratio compares two single roundings (at
B = 5, where the norm runs over five scalars, the largest is 4.1; the median over all cases
is 1.0).  This test found that sum to be the weak spot: accumulated in fp32, as the kernels
first did, [512-1-False-random-all_grads] was 1.54e-8 from the fp64 value (6.9 half-ulps of
3.8e-2) against the fp32 oracle's 8.8e-10, ratio 17.5, and four more cases exceeded 6.  The
terms cancel, so the accumulation and not the terms set the error; the backward kernels now
sum the same fp32 products in fp64 (wave_sum_f64), which brings that case to 8.8e-10.  The
yardstick itself moves with the host: torch's CPU reductions follow the vector width, and
the fp32 oracle's error for that case is 1.54e-8 on another CPU."""
import json
import sys
from pathlib import Path

import pytest
import torch

from oracle import refimpl as ref

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edge_inputs as ei  # noqa: E402
from test_sampling_long import _assert_hier, _coarse_places  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

# the factors of the docstring above (measured ratios: profiles/edge_shapes_parity.json)
F_COMPOSITE = 16
F_PE = 4


def _record(**kw):
    print("EDGE_PARITY " + json.dumps(kw))


class _Guarded:
    """A device buffer of ``shape`` with ``rows_after`` sentinel rows behind it."""

    def __init__(self, shape, rows_after, init):
        self.n = shape[0]
        self.buf = init.to(DEV).contiguous()
        assert self.buf.shape == (shape[0] + rows_after, *shape[1:])
        self._sentinel = self.buf[self.n:].clone()

    @property
    def out(self):
        return self.buf[: self.n]

    def check(self):
        """The sentinel rows are bit-unchanged."""
        assert torch.equal(self.buf[self.n:].contiguous().view(torch.uint8), self._sentinel.view(torch.uint8))


def guarded(shape, rows_after=1, init=None):
    """A buffer for an output of ``shape``: a fixed finite pattern for outputs that are
    overwritten, or ``init`` (payload + sentinel rows, random) for accumulated ones."""
    shape = tuple(shape)
    full = (shape[0] + rows_after, *shape[1:])
    if init is None:
        n = 1
        for s in full:
            n *= s
        init = ((torch.arange(n) % 251).float() * 0.5 - 60.25).reshape(full)
    return _Guarded(shape, rows_after, init)


def poisoned(nbytes):
    """Scratch a caller did not initialise: every byte 0xFF, which is NaN as fp32, bf16 and
    fp16 and a huge value as uint32."""
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=DEV)


def _call(name, *args):
    from noisy_src import _hip
    _hip.call(name, *[_hip.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _hip.stream_ptr())


def _gp(g):
    return None if g is None else g.buf


# ------------------------------------------------------------------ composite --
def _composite_raw(c, white, with_g, rd_init=None):
    """nr_composite_fwd + nr_composite_bwd on the case ``c`` through guarded buffers."""
    B, S = c["z"].shape
    dv = {k: (None if v is None else v.to(DEV)) for k, v in c.items()}
    o = dict(rgb_map=guarded((B, 3)), depth=guarded((B,)), acc=guarded((B,)), weights=guarded((B, S)),
             g_rgb=guarded((B, S, 3)), g_sigma=guarded((B, S)),
             g_rays_d=guarded((B, 3), init=torch.zeros(B + 1, 3) if rd_init is None else rd_init))
    _call("nr_composite_fwd", dv["rgb"], dv["sigma"], dv["z"], dv["rd"], dv["noise"], B, S, int(white),
          o["rgb_map"].buf, o["depth"].buf, o["acc"].buf, o["weights"].buf)
    _call("nr_composite_bwd", dv["rgb"], dv["sigma"], dv["z"], dv["rd"], dv["noise"], B, S, int(white), dv["g_map"],
          dv["g_depth"] if with_g else None, dv["g_acc"] if with_g else None, dv["g_w"] if with_g else None,
          o["g_rgb"].buf, o["g_sigma"].buf, o["g_rays_d"].buf)
    torch.cuda.synchronize()
    for v in o.values():
        v.check()
    return {k: v.out.cpu() for k, v in o.items()}


@pytest.mark.parametrize("with_g", [True, False], ids=["all_grads", "rgb_only"])
@pytest.mark.parametrize("S,B,white,regime", ei.COMPOSITE_CASES)
def test_composite_vs_fp64(S, B, white, regime, with_g):
    """nr_composite_fwd / nr_composite_bwd vs the fp64 oracle and fp64 autograd, in the
    three input regimes of edge_inputs.composite_inputs (random; surface: empty samples,
    then alpha == 1 exactly, then a transmittance that underflows; ties: delta == 0), with
    g_depth / g_acc / g_weights present or NULL.  Every output is finite, within
    ``max(F_COMPOSITE err_oracle32, floor)`` of the fp64 result, and leaves its sentinel row
    alone; g_sigma is exactly 0 wherever sigma + noise <= 0; g_rays_d accumulated onto a
    random buffer is that buffer plus the result over zeros, to the bit (one IEEE add); the
    forward with its nullable outputs NULL writes the same rgb_map."""
    c = ei.composite_inputs(S, B, regime)
    want = ei.composite_oracle(c, white, with_g, F64)
    o32 = ei.composite_oracle(c, white, with_g, torch.float32)
    got = _composite_raw(c, white, with_g)
    err = {k: ei.distance(k, got[k], want[k]) for k in want}
    e32 = {k: ei.distance(k, o32[k], want[k]) for k in want}
    scale = {k: want[k].abs().max().item() for k in want}
    _record(test="composite", S=S, B=B, white=white, regime=regime, with_g=with_g, err=err, e32=e32, scale=scale)
    for k in want:
        assert got[k].shape == want[k].shape and torch.isfinite(got[k]).all(), k
    for k in want:
        assert err[k] <= ei.yardstick_bound(F_COMPOSITE, e32[k], want[k]), (k, err[k], e32[k], scale[k])
    dead = (c["sigma"] if c["noise"] is None else c["sigma"] + c["noise"]) <= 0
    assert torch.count_nonzero(got["g_sigma"][dead]) == 0
    # accumulation onto a non-zero buffer, sentinel row included
    init = torch.cat([c["rd_init"], torch.full((1, 3), 7.5)])
    acc = _composite_raw(c, white, with_g, rd_init=init)
    assert torch.equal(acc["g_rays_d"], c["rd_init"] + got["g_rays_d"])
    for k in ("g_rgb", "g_sigma", "rgb_map", "weights"):
        assert torch.equal(acc[k], got[k]), k
    # depth / acc / weights are nullable
    dv = [None if v is None else v.to(DEV) for v in (c["rgb"], c["sigma"], c["z"], c["rd"], c["noise"])]
    only = guarded((B, 3))
    _call("nr_composite_fwd", *dv, B, S, int(white), only.buf, None, None, None)
    torch.cuda.synchronize()
    only.check()
    assert torch.equal(only.out.cpu(), got["rgb_map"])


@pytest.mark.parametrize("ticket", [True, False], ids=["ticket", "second_launch"])
@pytest.mark.parametrize("regime", ei.REGIMES)
@pytest.mark.parametrize("B", ei.COMPOSITE_B)
@pytest.mark.parametrize("S", ei.MSE_S)
def test_composite_mse_equals_separate(S, B, regime, ticket):
    """nr_composite_mse stays bit-identical to nr_composite_fwd, nr_mse_fwd_bwd and
    nr_composite_bwd in sequence at the edges test_fused_equals_separate does not reach
    (one and two samples, K = 2, both sides of the switch to the long form, a partly filled
    workgroup), with the in-launch loss sum (ticket) and without; the loss is the same mean
    summed in another order, the ticket is 0 afterwards, sentinel rows stay."""
    from noisy_src import _hip
    c = ei.composite_inputs(S, B, regime)
    dv = {k: (None if v is None else v.to(DEV)) for k, v in c.items()}
    init = torch.cat([c["rd_init"], torch.full((1, 3), 7.5)])
    scale = 0.5

    def buffers():
        return dict(rgb_map=guarded((B, 3)), depth=guarded((B,)), acc=guarded((B,)), weights=guarded((B, S)),
                    g_rgb=guarded((B, S, 3)), g_sigma=guarded((B, S)), g_rays_d=guarded((B, 3), init=init),
                    loss=guarded((1,)))

    a = buffers()
    g_map = guarded((B, 3))
    front = (dv["rgb"], dv["sigma"], dv["z"], dv["rd"], dv["noise"])
    _call("nr_composite_fwd", *front, B, S, 1, a["rgb_map"].buf, a["depth"].buf, a["acc"].buf, a["weights"].buf)
    _call("nr_mse_fwd_bwd", a["rgb_map"].buf, dv["target"], B, scale, a["loss"].buf, g_map.buf)
    _call("nr_composite_bwd", *front, B, S, 1, g_map.buf, None, None, None, a["g_rgb"].buf, a["g_sigma"].buf,
          a["g_rays_d"].buf)
    f = buffers()
    tk = torch.zeros(4, device=DEV, dtype=torch.int32) if ticket else None
    ws = torch.empty(int(_hip.load().nr_composite_mse_workspace_bytes(B)), device=DEV, dtype=torch.uint8)
    _call("nr_composite_mse", *front, dv["target"], B, S, 1, scale, f["rgb_map"].buf, f["depth"].buf, f["acc"].buf,
          f["weights"].buf, f["loss"].buf, f["g_rgb"].buf, f["g_sigma"].buf, f["g_rays_d"].buf, tk, ws)
    torch.cuda.synchronize()
    g_map.check()
    for k in a:
        a[k].check()
        f[k].check()
        assert torch.isfinite(f[k].out).all(), k
        if k != "loss":
            assert torch.equal(a[k].out, f[k].out), k
    la, lf = a["loss"].out.item(), f["loss"].out.item()
    assert abs(la - lf) <= 1e-6 * abs(la), (la, lf)
    if ticket:
        assert torch.count_nonzero(tk) == 0


# ------------------------------------------------------------------- sampling --
def _hier_raw(o, d, z, w, Nf, det, u, pts=True, vd=False):
    """nr_sample_hierarchical into guarded buffers -> (pts, z_fine, viewdirs) on the CPU."""
    B, Nc = z.shape
    T = Nc + Nf
    zf = guarded((B, T))
    po = guarded((B, T, 3)) if pts else None
    vo = guarded((B * T, 3), rows_after=T) if vd else None
    _call("nr_sample_hierarchical", o.to(DEV), d.to(DEV), z.to(DEV), w.to(DEV), None if det else u.to(DEV), B, Nc, Nf,
          zf.buf, _gp(po), _gp(vo))
    torch.cuda.synchronize()
    for b in (zf, po, vo):
        if b is not None:
            b.check()
    return (None if po is None else po.out.cpu()), zf.out.cpu(), (None if vo is None else vo.out.cpu())


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Nc,Nf", ei.HIER_SIZES)
def test_sample_hierarchical_short_vs_fp64(Nc, Nf, B, det):
    """Every sample_hier_kernel<R> and every lane-63 wrap (the table above) under
    test_sampling_long's bounds against the fp64 oracle: sorted, z and pts within 1e-4,
    every coarse depth present bit for bit; and the depths alone (pts NULL) are the same."""
    o, d, z, w, u = ei.hier_inputs(Nc, Nf, B)
    wpts, wzf = ei.hier_oracle64(o, d, z, w, Nf, det, u)
    pts, zf, _ = _hier_raw(o, d, z, w, Nf, det, u)
    _record(test="sample_hier", Nc=Nc, Nf=Nf, B=B, det=det, z_err=(zf - wzf).abs().max().item(),
            pts_err=(pts - wpts).abs().max().item())
    _assert_hier(pts, zf, wpts, wzf, z)
    _, zf_only, _ = _hier_raw(o, d, z, w, Nf, det, u, pts=False)
    assert torch.equal(zf_only, zf)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("Nc,Nf", ei.HIER_PORT_SIZES)
def test_sample_hierarchical_short_any_input_order(Nc, Nf, det):
    """test_sample_hierarchical_long_any_input_order at a short size: coarse depths (and
    their weights) reversed in every second row; the output is the sorted multiset."""
    o, d, z, w, u = ei.hier_inputs(Nc, Nf, 5, seed=5)
    z, w = z.clone(), w.clone()
    z[1::2] = z[1::2].flip(-1)
    w[1::2] = w[1::2].flip(-1)
    z, w = z.contiguous(), w.contiguous()
    wpts, wzf = ei.hier_oracle64(o, d, z, w, Nf, det, u)
    pts, zf, _ = _hier_raw(o, d, z, w, Nf, det, u)
    _assert_hier(pts, zf, wpts, wzf, z)


@pytest.mark.parametrize("Nc,Nf", ei.HIER_PORT_SIZES)
def test_sample_hierarchical_short_duplicates(Nc, Nf):
    """test_sample_hierarchical_long_duplicates at a short size: u takes 8 distinct values
    per row, so the fine samples are full of exact ties; the row is still the sorted
    multiset of the coarse depths and exactly Nf samples."""
    B = 5
    o, d, z, w, _ = ei.hier_inputs(Nc, Nf, B, seed=7)
    g = torch.Generator().manual_seed(8)
    vals = torch.rand(B, 8, generator=g)
    u = torch.gather(vals, -1, torch.randint(0, 8, (B, Nf), generator=g))
    _, zf, _ = _hier_raw(o, d, z, w, Nf, False, u)
    assert torch.all(zf[:, 1:] >= zf[:, :-1])
    zs, pos = _coarse_places(zf, z)
    assert pos.max() < Nc + Nf
    assert torch.equal(torch.gather(zf, -1, pos), zs)
    keep = torch.ones(B, Nc + Nf, dtype=torch.bool)
    keep.scatter_(-1, pos, False)
    assert torch.all(keep.sum(-1) == Nf)
    s = zf[keep].reshape(B, Nf)
    want_s = ei.pdf_oracle64(0.5 * (z[:, 1:] + z[:, :-1]), w[:, 1:-1], Nf, False, u)
    assert len(torch.unique(want_s[0])) <= 8
    assert (s - torch.sort(want_s, dim=-1).values).abs().max() < 1e-4
    assert torch.equal(zf, torch.sort(torch.cat([z, s], -1), dim=-1).values)


@pytest.mark.parametrize("Nc,Nf", ei.HIER_PORT_SIZES)
def test_viewdirs_output_short(Nc, Nf):
    """test_viewdirs_output_long at a short size, |d| in 0.5 .. 2: the viewdirs output equals
    nr_expand_viewdirs, lies within 1e-6 of d / |d| in fp64, and pts = o + d z."""
    from noisy_src import ops
    B = 5
    o, d, z, w, u = ei.hier_inputs(Nc, Nf, B, seed=13)
    pts, zf, vd = _hier_raw(o, d, z, w, Nf, False, u, vd=True)
    assert torch.equal(vd, ops.expand_viewdirs(d.to(DEV), Nc + Nf).cpu())
    unit = d.double() / d.double().norm(dim=-1, keepdim=True)
    assert (vd.double().reshape(B, Nc + Nf, 3) - unit[:, None, :]).abs().max() < 1e-6
    assert (pts - (o[:, None, :] + d[:, None, :] * zf[..., None])).abs().max() <= 1e-6


def _pdf_raw(bins, w, Ns, det, u):
    B, Nb = bins.shape
    out = guarded((B, Ns))
    _call("nr_sample_pdf", bins.to(DEV), w.to(DEV), None if det else u.to(DEV), B, Nb, Ns, out.buf)
    torch.cuda.synchronize()
    out.check()
    return out.out.cpu()


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Ns", ei.PDF_NS)
@pytest.mark.parametrize("Nb", ei.PDF_NB)
def test_sample_pdf_short_vs_fp64(Nb, Ns, B, det):
    """sample_pdf_kernel from its smallest Nb to its largest (513: above it the long-ray
    kernel takes over), around build_cdf's stride of 64, one or two samples and more than a
    wave of them, vs the fp64 oracle within 1e-4 (weights rand + 0.5)."""
    bins, w, u = ei.pdf_inputs(Nb, Ns, B)
    got = _pdf_raw(bins, w, Ns, det, u)
    want = ei.pdf_oracle64(bins, w, Ns, det, u)
    err = (got - want).abs().max().item()
    _record(test="sample_pdf", Nb=Nb, Ns=Ns, B=B, det=det, err=err)
    assert got.shape == want.shape and torch.isfinite(got).all() and err < 1e-4, err


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("Nb", ei.PDF_SPIKE_NB)
def test_sample_pdf_short_spike_weights(Nb, det):
    """A trained ray's weights, all zero but one spike (test_sample_pdf_degenerate_weights'
    style): the invariants everywhere -- inside the bins, monotone in u -- and the values
    within 1e-4 of the fp64 oracle wherever its bucket is non-degenerate (denom >= 1e-5);
    test_edge_inputs_host asserts that this is more than 0.3 of the samples and that no
    bucket sits at the threshold."""
    bins, w, u = ei.pdf_spike_inputs(Nb)
    B, Ns = ei.PDF_SPIKE_B, ei.PDF_SPIKE_NS
    got = _pdf_raw(bins, w, Ns, det, u)
    want = ei.pdf_oracle64(bins, w, Ns, det, u)
    assert torch.isfinite(got).all()
    assert torch.all(got >= bins[:, :1] - 1e-6) and torch.all(got <= bins[:, -1:] + 1e-6)
    uu = ei.linspace_u(B, Ns) if det else u
    gs = torch.gather(got, -1, torch.argsort(uu, dim=-1))
    assert torch.all(gs[:, 1:] >= gs[:, :-1] - 1e-6)
    ok = ei.pdf_bucket_denominators(w, uu) >= 1e-5
    assert ok.double().mean() > 0.3
    err = (got - want)[ok].abs().max().item()
    _record(test="sample_pdf_spike", Nb=Nb, det=det, share=ok.double().mean().item(), err=err)
    assert err < 1e-4, err


# ----------------------------------------------------------------- stratified --
@pytest.mark.parametrize("outputs", [True, False], ids=["pts_viewdirs", "z_only"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("perturb", [True, False])
@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("N", [1, 2, 64])
def test_stratified_vs_fp64(N, lindisp, perturb, B, outputs):
    """nr_stratified_sample at one sample (linspace_at's n == 1 branch: z = near, no bin to
    perturb in), two (both ends, no interior sample) and 64, in depth and in disparity, with
    and without t_rand, with and without the pts / viewdirs outputs, vs the oracle in fp64:
    z within 2e-6, pts within 1e-5 (test_stratified's bounds), viewdirs within 1e-6."""
    g = torch.Generator().manual_seed(40 + N + 2 * B)
    o, d = ei.rays(B, g)
    tr = torch.rand(B, N, generator=g) if perturb else None
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)  # the oracle's own linspace in fp64 too
    try:
        wpts, wz = ref.sample_along_rays(o.double(), d.double(), 2.0, 6.0, N, perturb=perturb, lindisp=lindisp,
                                         t_rand=None if tr is None else tr.double())
    finally:
        torch.set_default_dtype(prev)
    assert wz.dtype == F64 and wz.shape == (B, N)
    z = guarded((B, N))
    pts = guarded((B, N, 3)) if outputs else None
    vd = guarded((B * N, 3), rows_after=N) if outputs else None
    _call("nr_stratified_sample", o.to(DEV), d.to(DEV), None if tr is None else tr.to(DEV), 2.0, 6.0, int(lindisp), B,
          N, z.buf, _gp(pts), _gp(vd))
    torch.cuda.synchronize()
    z.check()
    ez = (z.out.cpu() - wz).abs().max().item()
    rec = dict(test="stratified", N=N, lindisp=lindisp, perturb=perturb, B=B, z_err=ez)
    if outputs:
        pts.check()
        vd.check()
        rec["pts_err"] = (pts.out.cpu() - wpts).abs().max().item()
        unit = d.double() / d.double().norm(dim=-1, keepdim=True)
        rec["vd_err"] = (vd.out.cpu().double().reshape(B, N, 3) - unit[:, None, :]).abs().max().item()
    _record(**rec)
    assert ez <= 2e-6, ez
    if outputs:
        assert rec["pts_err"] <= 1e-5 and rec["vd_err"] < 1e-6, rec


# -------------------------------------------------------- positional encoding --
@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("logs", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("inc", [True, False], ids=["input", "no_input"])
@pytest.mark.parametrize("L", [1, 4, 10])
@pytest.mark.parametrize("C", [1, 3])
def test_positional_encoding_vs_fp64(C, L, inc, logs, M):
    """nr_positional_encoding / _bwd for C = 1 and 3, L = 1 (linspace_at's n == 1 branch), 4
    and 10, with and without the input block, log and linear frequency bands, one sample and
    257, |x| <= 4, vs the oracle's module in fp64 (its fp32 frequency bands promoted, as
    ``.double()`` leaves them).  Forward: within 2e-6 wherever f |x| <= 64; beyond (up to
    2048 radians) and for the backward's g_x the yardstick is torch's fp32 sin / cos of the
    fp32 product against fp64, under F_PE."""
    g = torch.Generator().manual_seed(1000 * C + 10 * L + M)
    x = torch.rand(M, C, generator=g) * 8 - 4
    enc = ref.PositionalEncoding(L, include_input=inc, log_sampling=logs)
    D = C * enc.output_dim
    g_out = torch.randn(M, D, generator=g)

    def oracle(dtype):
        e = ref.PositionalEncoding(L, include_input=inc, log_sampling=logs).to(dtype)
        xx = x.to(dtype).requires_grad_(True)
        out = e(xx)
        (gx,) = torch.autograd.grad((out * g_out.to(dtype)).sum(), xx)
        return out.detach(), gx

    w64, gx64 = oracle(F64)
    w32, gx32 = oracle(torch.float32)
    out, gx = guarded((M, D)), guarded((M, C))
    xd = x.to(DEV)
    _call("nr_positional_encoding", xd, M, C, L, int(inc), int(logs), out.buf)
    _call("nr_positional_encoding_bwd", xd, M, C, L, int(inc), int(logs), g_out.to(DEV), gx.buf)
    torch.cuda.synchronize()
    out.check()
    gx.check()
    got, ggx = out.out.cpu(), gx.out.cpu()
    assert got.shape == w64.shape and torch.isfinite(got).all() and torch.isfinite(ggx).all()
    # the argument f |x| of every output column (0 for the input block)
    f = enc.freq_bands.double().repeat_interleave(2 * C)
    f = torch.cat([torch.zeros(C if inc else 0, dtype=F64), f])
    arg = f[None, :] * x.double().abs().repeat(1, enc.output_dim)
    small = arg <= 64
    e_small = (got.double() - w64)[small].abs().max().item()
    rec = dict(test="pe", C=C, L=L, inc=inc, logs=logs, M=M, fwd_small=e_small, arg_max=arg.max().item())
    big = ~small
    if big.any():
        rec["fwd_big"] = (got.double() - w64)[big].abs().max().item()
        rec["fwd_big_e32"] = (w32.double() - w64)[big].abs().max().item()
    rec["bwd"] = (ggx.double() - gx64).norm().item()
    rec["bwd_e32"] = (gx32.double() - gx64).norm().item()
    rec["bwd_scale"] = gx64.abs().max().item()
    _record(**rec)
    assert e_small <= 2e-6, e_small
    if big.any():
        assert rec["fwd_big"] <= max(F_PE * rec["fwd_big_e32"], ei.FLOOR), rec
    assert rec["bwd"] <= ei.yardstick_bound(F_PE, rec["bwd_e32"], gx64), rec
