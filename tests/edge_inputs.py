"""Input generators and fp64 references shared by test_edge_shapes.py, test_mlp_ragged.py
(GPU) and test_edge_inputs_host.py (CPU).  Everything here runs on the CPU, on the oracle
alone; the host test asserts that each generator meets the condition its GPU test relies on
(an exactly opaque sample, an underflowed transmittance, delta == 0, enough non-degenerate
buckets, enough kink-free samples), so a GPU test cannot pass on inputs that miss the edge.

Case lists live here too, so that the CPU and the GPU tests walk the same cases."""
import copy
import functools
import itertools

import torch

from oracle import refimpl as ref

F64 = torch.float64

# ------------------------------------------------------------------ composite --
COMPOSITE_S = [1, 2, 63, 64, 65, 511, 512, 513]  # wave-per-ray up to 512 (K = ceil(S / 64)), thread-per-ray above
COMPOSITE_B = [1, 5]  # four rays per workgroup: a partly filled one, and one past the first
REGIMES = ["random", "surface", "ties"]
COMPOSITE_CASES = list(itertools.product(COMPOSITE_S, COMPOSITE_B, [True, False], REGIMES))
MSE_S = [1, 2, 65, 512, 513]


def _unit(n, g):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=-1)


@functools.lru_cache(maxsize=None)
def composite_inputs(S, B, regime):
    """fp32 inputs of one compositing case (a dict of CPU tensors).

    random   the draw of test_parity_ops.test_composite_fwd_bwd (sigma = 20 randn, sorted
             z) with the sigma noise of raw_noise_std > 0;
    surface  per ray: a run of empty samples (sigma exactly 0, or negative), then 3 to 6
             samples with sigma * delta * |d| = 150 (alpha == 1 exactly in fp32, each
             multiplying the transmittance by 1e-10), then the random draw behind them;
             ray 0 has 6 opaque samples whenever S allows, so its transmittance reaches 0;
    ties     the random draw with exact duplicates in z (delta == 0) at random places and
             in the first and the last pair.
    |rays_d| lies in 0.5 .. 2.  Upstream gradients for every output, a target for the MSE
    form and a random buffer that g_rays_d is accumulated onto come with it."""
    g = torch.Generator().manual_seed(100_000 * REGIMES.index(regime) + 10 * S + B)
    rd = (_unit(B, g) * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=F64))).float()
    z = torch.sort(torch.rand(B, S, generator=g) * 4 + 2, dim=-1).values
    rgb = torch.rand(B, S, 3, generator=g)
    sigma = torch.randn(B, S, generator=g) * 20
    noise = None
    if regime == "random":
        noise = torch.randn(B, S, generator=g) * 0.5
    elif regime == "ties":
        dup = torch.rand(B, S, generator=g) < 0.2
        if S >= 2:
            dup[:, 1] = True
            dup[:, S - 1] = True
        dup[:, 0] = False
        for i in range(1, S):  # z[i] = z[i - 1] where marked; runs of marks give runs of ties
            z[:, i] = torch.where(dup[:, i], z[:, i - 1], z[:, i])
    elif regime == "surface":
        dn = rd.norm(dim=-1)
        delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B, 1), 1e10)], -1)
        for b in range(B):
            k_op = min(S, 6 if b == 0 else int(torch.randint(3, 7, (1,), generator=g)))
            n_empty = int(torch.randint(0, (S - k_op) // 2 + 1, (1,), generator=g))
            empty = torch.where(torch.rand(n_empty, generator=g) < 0.5, torch.zeros(n_empty),
                                -20 * torch.rand(n_empty, generator=g))
            sigma[b, :n_empty] = empty
            sl = slice(n_empty, n_empty + k_op)
            sigma[b, sl] = 150.0 / (delta[b, sl].clamp_min(1e-6) * dn[b])
    else:
        raise ValueError(regime)
    return dict(rgb=rgb, sigma=sigma, z=z.contiguous(), rd=rd, noise=noise,
                g_map=torch.randn(B, 3, generator=g), g_depth=0.1 * torch.randn(B, generator=g),
                g_acc=torch.randn(B, generator=g), g_w=torch.randn(B, S, generator=g),
                target=torch.rand(B, 3, generator=g), rd_init=torch.randn(B, 3, generator=g))


def _raw2outputs_one_sample(rgb, sigma, z_vals, rays_d, raw_noise_std=0.0, white_background=True, noise=None):
    """ref.raw2outputs for S == 1.  The reference shapes its "infinite distance at the end"
    from ``dists[..., :1]`` (rendering.py:69-72), which is EMPTY when there is one sample: it
    then composites nothing and returns (B, 0) weights.  The kernels follow the recurrence
    the reference states (the last sample's delta is 1e10), also for a ray of one sample,
    so the reference for S == 1 is the oracle's own expression, line for line, with that
    one column shaped from z_vals."""
    sigma = sigma.squeeze(-1)
    dists = torch.full_like(z_vals[..., :1], 1e10)
    dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    if raw_noise_std > 0.0:
        sigma = sigma + noise
    alpha = 1.0 - torch.exp(-torch.relu(sigma) * dists)
    transmittance = torch.cumprod(
        torch.cat([torch.ones_like(alpha[..., :1]), 1.0 - alpha + 1e-10], dim=-1), dim=-1)[..., :-1]
    weights = alpha * transmittance
    rgb_map = torch.sum(weights[..., None] * rgb, dim=-2)
    depth_map = torch.sum(weights * z_vals, dim=-1)
    acc_map = torch.sum(weights, dim=-1)
    if white_background:
        rgb_map = rgb_map + (1.0 - acc_map[..., None])
    return {"rgb_map": rgb_map, "depth_map": depth_map, "acc_map": acc_map, "weights": weights}


def composite_oracle(c, white, with_g, dtype):
    """The oracle's raw2outputs in ``dtype`` on the case ``c``, and autograd's gradients of
    sum(rgb_map g_map) [+ sum(depth g_depth) + sum(acc g_acc) + sum(weights g_w)]."""
    rgb, sigma, rd = (c[k].to(dtype).clone().requires_grad_(True) for k in ("rgb", "sigma", "rd"))
    noise = None if c["noise"] is None else c["noise"].to(dtype)
    raw2outputs = ref.raw2outputs if sigma.shape[-1] > 1 else _raw2outputs_one_sample
    out = raw2outputs(rgb, sigma[..., None], c["z"].to(dtype), rd, raw_noise_std=0.0 if noise is None else 1.0,
                      white_background=white, noise=noise)
    loss = (out["rgb_map"] * c["g_map"].to(dtype)).sum()
    if with_g:
        loss = loss + (out["depth_map"] * c["g_depth"].to(dtype)).sum() + (out["acc_map"] * c["g_acc"].to(dtype)).sum()
        loss = loss + (out["weights"] * c["g_w"].to(dtype)).sum()
    g_rgb, g_sigma, g_rd = torch.autograd.grad(loss, (rgb, sigma, rd))
    return dict(rgb_map=out["rgb_map"].detach(), depth=out["depth_map"].detach(), acc=out["acc_map"].detach(),
                weights=out["weights"].detach(), g_rgb=g_rgb, g_sigma=g_sigma, g_rays_d=g_rd)


MAX_NORM = ("rgb_map", "depth", "acc")  # the per-ray maps: max norm; the rest: 2-norm
FLOOR = 4 * 2.0 ** -24


def distance(name, got, want):
    d = got.double() - want.double()
    return (d.abs().max() if name in MAX_NORM else d.norm()).item()


def yardstick_bound(F, err32, want):
    """``max(F err_oracle32, 4 2^-24 max|want|)``: the kernel is another association of the
    same fp32 products and sums, so its distance from the fp64 result is held to a small
    multiple F of the fp32 oracle's own; the floor covers an oracle that is exact."""
    return max(F * err32, FLOOR * want.abs().max().item())


def composite_terms_fp32(c):
    """alpha and the transmittance before each sample, in the oracle's fp32 arithmetic."""
    sig = c["sigma"] if c["noise"] is None else c["sigma"] + c["noise"]
    dists = torch.cat([c["z"][:, 1:] - c["z"][:, :-1], torch.full_like(c["z"][:, :1], 1e10)], -1)
    dists = dists * c["rd"].norm(dim=-1, keepdim=True)
    alpha = 1.0 - torch.exp(-torch.relu(sig) * dists)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    return alpha, T, dists


# ------------------------------------------------------------------- sampling --
# (Nc, Nf): R = values per lane of sample_hier_kernel<R>, T = Nc + Nf
HIER_SIZES = [(3, 1), (3, 61), (32, 32), (64, 1), (65, 63), (66, 62), (129, 127), (130, 127), (256, 256), (3, 509),
              (511, 1)]
HIER_PORT_SIZES = [(64, 128), (129, 127)]
PDF_NB = [2, 3, 64, 65, 66, 513]
PDF_NS = [1, 2, 64, 65]
PDF_SPIKE_NB = [nb for nb in PDF_NB if nb >= 64]
PDF_SPIKE_NS, PDF_SPIKE_B = 65, 5


def rays(B, g):
    o = torch.randn(B, 3, generator=g)
    d = (_unit(B, g) * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=F64))).float()
    return o, d


def linspace_u(B, n):
    """det=True's u: torch.linspace(0, 1, n) in fp32, as the reference builds it."""
    return torch.linspace(0.0, 1.0, n).expand(B, n).contiguous()


@functools.lru_cache(maxsize=None)
def hier_inputs(Nc, Nf, B, seed=0):
    """Rays with |d| in 0.5 .. 2, perturbed stratified coarse depths in [2, 6], weights
    rand + 0.5 (test_sampling_long's conditioning argument) and uniforms u."""
    g = torch.Generator().manual_seed(1_000_000 * seed + 1000 * Nc + 2 * Nf + B)
    o, d = rays(B, g)
    _, z = ref.sample_along_rays(o, d, 2.0, 6.0, Nc, t_rand=torch.rand(B, Nc, generator=g))
    w = torch.rand(B, Nc, generator=g) + 0.5
    u = torch.rand(B, Nf, generator=g)
    return o, d, z.contiguous(), w, u


def hier_oracle64(o, d, z, w, Nf, det, u):
    uu = linspace_u(z.shape[0], Nf) if det else u
    pts, zf = ref.sample_hierarchical(o.double(), d.double(), z.double(), w.double(), Nf, det=False, u=uu.double())
    return pts, zf


@functools.lru_cache(maxsize=None)
def pdf_inputs(Nb, Ns, B):
    g = torch.Generator().manual_seed(7000 * Nb + 10 * Ns + B)
    bins = torch.sort(torch.rand(B, Nb, generator=g) * 4 + 2, dim=-1).values.contiguous()
    w = torch.rand(B, Nb - 1, generator=g) + 0.5
    u = torch.rand(B, Ns, generator=g)
    return bins, w, u


def pdf_oracle64(bins, w, Ns, det, u):
    uu = linspace_u(bins.shape[0], Ns) if det else u
    return ref.sample_pdf(bins.double(), w.double(), Ns, det=False, u=uu.double())


@functools.lru_cache(maxsize=None)
def pdf_spike_inputs(Nb):
    """The weights of test_sample_pdf_degenerate_weights on PDF_SPIKE_B rays: the first two
    all zero (the uniform pdf), the others one spike of 100 (at another bin in each) over
    1e-3 rand.  The bucket of a u whose denominator lies within 10 % of the reference's
    ``denom < 1e-5 -> 1`` threshold would be decided by rounding, so the first seed without
    such a u (given or linspace) is taken; test_edge_inputs_host asserts the outcome."""
    B, Ns = PDF_SPIKE_B, PDF_SPIKE_NS
    for k in range(64):
        g = torch.Generator().manual_seed(21 + Nb + 1000 * k)
        bins = torch.sort(torch.rand(B, Nb, generator=g) * 4 + 2, dim=-1).values.contiguous()
        w = torch.rand(B, Nb - 1, generator=g) * 1e-3
        w[torch.arange(B), torch.randint(0, Nb - 1, (B,), generator=g)] = 100.0
        w[:2] = 0.0
        u = torch.rand(B, Ns, generator=g)
        den = torch.cat([pdf_bucket_denominators(w, u), pdf_bucket_denominators(w, linspace_u(B, Ns))])
        if not ((den > 0.9e-5) & (den < 1.1e-5)).any():
            break
    return bins, w, u


def pdf_bucket_denominators(w, uu):
    """The oracle's bucket denominator ``cdf[above] - cdf[below]`` of every u, in fp64."""
    wp = w.double() + 1e-5
    cdf = torch.cat([torch.zeros(w.shape[0], 1, dtype=F64), torch.cumsum(wp / wp.sum(-1, keepdim=True), -1)], -1)
    idx = torch.searchsorted(cdf, uu.double().contiguous(), right=True)
    c0 = torch.gather(cdf, -1, (idx - 1).clamp(min=0))
    c1 = torch.gather(cdf, -1, idx.clamp(max=cdf.shape[-1] - 1))
    return c1 - c0


# -------------------------------------------------------------------- the MLP --
RAGGED_M = [1, 31, 33, 511, 513]
REF16_M = [1, 31, 33, 513]
REF32_M = [1, 33]


def oracle_net(precision, seed=0):
    from noisy_src.config import ModelConfig
    torch.manual_seed(seed)
    return ref.NeRF(ModelConfig(precision=precision))


def mlp_candidates(n, seed, lo=0.0, hi=1.5):
    """Positions with |x_c| uniform in [lo, hi] (random signs) and unit view directions."""
    g = torch.Generator().manual_seed(seed)
    mag = lo + (hi - lo) * torch.rand(n, 3, generator=g)
    x = mag * (2.0 * torch.randint(0, 2, (n, 3), generator=g) - 1.0)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return x, d


def kink_free(oracle, x, d, eps):
    """test_parity_mlp._kink_free: every fp64 ReLU pre-activation at least eps from 0."""
    o64 = ref.NeRF(oracle.config).double()
    o64.load_state_dict({k: v.double() for k, v in oracle.state_dict().items()})
    mins = []
    hooks = [m.register_forward_hook(lambda m, i, out: mins.append(out.abs().min(dim=-1).values))
             for m in list(o64.pts_linears) + [o64.dir_linear, o64.sigma_linear]]
    with torch.no_grad():
        o64(x.double(), d.double())
    for h in hooks:
        h.remove()
    return torch.stack(mins, -1).min(-1).values >= eps


def model_preactivations(emu, x, d):
    """The ReLU pre-activations of the numerics model (refimpl.MfmaEmulatedNeRF.forward
    without its gradient rounding, which is the identity in the forward) and its outputs;
    test_edge_inputs_host holds the outputs to the model's own, bit for bit."""
    b = emu.base
    x_enc = b.pos_encoder(x)
    h, pre = x_enc, []
    for i, layer in enumerate(b.pts_linears):
        pre.append(emu._lin(h, layer))
        h = torch.relu(pre[-1])
        if i in b.config.skips:
            h = torch.cat([x_enc, h], dim=-1)
    pre.append(torch.nn.functional.linear(h, b.sigma_linear.weight, b.sigma_linear.bias))
    sigma = torch.relu(pre[-1])
    h_color = torch.cat([emu._lin(h, b.feature_linear), b.dir_encoder(d)], dim=-1)
    pre.append(emu._lin(h_color, b.dir_linear))
    rgb = torch.sigmoid(torch.nn.functional.linear(torch.relu(pre[-1]), b.rgb_linear.weight, b.rgb_linear.bias))
    return pre, rgb, sigma


def model_kink_free(oracle, precision, x, d, eps):
    """Every ReLU pre-activation of the numerics model at least eps from 0: the kernels round
    like the model, so only summation-order differences (~1e-6) can move a unit across."""
    with torch.no_grad():
        pre, _, _ = model_preactivations(ref.mfma_emulated_nerf(oracle, precision), x, d)
    return torch.stack([p.abs().min(dim=-1).values for p in pre], -1).min(-1).values >= eps


class _Sine64Encoding(torch.nn.Module):
    """The oracle's encoding with the sines taken in fp64 and rounded to fp32 once."""

    def __init__(self, enc):
        super().__init__()
        self.enc = copy.deepcopy(enc).double()
        self.output_dim = enc.output_dim

    def forward(self, x):
        return self.enc(x.double()).float()


def sine_sensitive(oracle, precision, x, d):
    """Samples whose numerics-model forward moves by more than 1e-4 when the encoding is
    computed with an fp64 sine instead of torch's fp32 one: there a sine within rounding
    of a 16-bit boundary decides the result (test_16bit_input_gradients' outliers)."""
    alt = copy.deepcopy(oracle)
    alt.pos_encoder = _Sine64Encoding(oracle.pos_encoder)
    alt.dir_encoder = _Sine64Encoding(oracle.dir_encoder)
    with torch.no_grad():
        r0, s0 = ref.mfma_emulated_nerf(oracle, precision)(x, d)
        r1, s1 = ref.mfma_emulated_nerf(alt, precision)(x, d)
    return ((r0 - r1).abs().amax(-1) > 1e-4) | ((s0 - s1).abs().amax(-1) > 1e-4)


@functools.lru_cache(maxsize=None)
def mlp_selected(precision, M):
    """(x, d, number of survivors): the first M of 3 M + 64 candidates that are kink-free
    with margin -- 2e-6 against the fp64 oracle for fp32 (test_fp32_backward's), 1e-5
    against the numerics model for the 16-bit paths (16-bit operands move a pre-activation
    by ~1e-3, so the fp64 oracle's kinks are not the model's) -- and, for the 16-bit paths,
    not ``sine_sensitive``."""
    oracle = oracle_net(precision)
    x, d = mlp_candidates(3 * M + 64, seed=500 + M)
    if precision == "fp32":
        keep = kink_free(oracle, x, d, 2e-6)
    else:
        keep = model_kink_free(oracle, precision, x, d, 1e-5) & ~sine_sensitive(oracle, precision, x, d)
    return x[keep][:M].contiguous(), d[keep][:M].contiguous(), int(keep.sum())


def mlp_upstream(M, seed, scale=2.0 / (3 * 4096)):
    """Upstream gradients at the magnitude of a mean loss over 4096 rays."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, 3, generator=g) * scale, torch.randn(M, 1, generator=g) * scale
