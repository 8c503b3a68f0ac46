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


# Boundary ModelConfigs of the fused MLP (test_mlp_configs.py): name -> (ModelConfig
# arguments, what the case reaches).  None is the default model.
CONFIG_CASES = {
    "pos0_dir0": (dict(pos_freqs=0, dir_freqs=0), "3 live columns per encoding block, no sine at all"),
    "pos5_dir3": (dict(pos_freqs=5, dir_freqs=3),
                  "33 position columns (a second block with one live column), 21 direction columns"),
    "pos10_dir1": (dict(dir_freqs=1), "9 direction columns beside the full 63"),
    "depth2_skip0": (dict(num_hidden_layers=2, skips=(0,)),
                     "a skip directly after layer 0; the smallest net that has one"),
    "depth6_skips_1_2_4": (dict(num_hidden_layers=6, skips=(1, 2, 4)),
                           "adjacent skips and a skip at the last allowed layer (n - 2)"),
    "depth3_skip1_no_view_dirs": (dict(num_hidden_layers=3, skips=(1,), use_view_dirs=False),
                                  "last-allowed skip with DB = 0"),
    "depth16_skip4": (dict(num_hidden_layers=16), "the maximum depth: job, reduce and stream tables at their fullest"),
    "depth16_skips_0_3_6_9_12": (dict(num_hidden_layers=16, skips=(0, 3, 6, 9, 12)),
                                 "the maximum depth with six x_enc-reading layers: three x-jobs"),
}
CONFIG_PRECISIONS = ["fp32", "bf16", "fp16"]
# (case, M): every case at one full tile plus a tile of one sample; the depth-16 ones also
# at a 16-tile forward group plus one tile
CONFIG_RUNS = [(c, 33) for c in CONFIG_CASES] + [(c, 513) for c in CONFIG_CASES if c.startswith("depth16")]


def case_config(precision, case=None):
    from noisy_src.config import ModelConfig
    return ModelConfig(precision=precision, **(CONFIG_CASES[case][0] if case else {}))


# The default initialisation leaves the sigma head negative on every sample in these cases
# (depth 16: h barely depends on x), which would make g_sigma, and with it the head's
# reference gradients, exactly zero; their oracle has the head's weight and bias negated.
# test_edge_inputs_host asserts, per case, that sigma is alive on a quarter of a probe set
# with this list and that no case outside it needs the flip.
SIGMA_HEAD_NEGATED = ("depth16_skip4", "depth16_skips_0_3_6_9_12")


def oracle_net(precision, seed=0, case=None):
    """The oracle at its default initialisation (SIGMA_HEAD_NEGATED cases: see there)."""
    torch.manual_seed(seed)
    net = ref.NeRF(case_config(precision, case))
    if case in SIGMA_HEAD_NEGATED:
        with torch.no_grad():
            net.sigma_linear.weight.neg_()
            net.sigma_linear.bias.neg_()
    return net


def sigma_alive_share(net):
    with torch.no_grad():
        return (net(*mlp_candidates(256, seed=499))[1] > 0).float().mean().item()


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
    h_color = emu._lin(h, b.feature_linear)
    if b.config.use_view_dirs:
        h_color = torch.cat([h_color, b.dir_encoder(d)], dim=-1)
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
def mlp_selected(precision, M, case=None, lo=0.0, hi=1.5):
    """(x, d, number of survivors): the first M of 3 M + 64 candidates that are kink-free
    with margin -- 2e-6 against the fp64 oracle for fp32 (test_fp32_backward's), 1e-5
    against the numerics model for the 16-bit paths (16-bit operands move a pre-activation
    by ~1e-3, so the fp64 oracle's kinks are not the model's) -- and, for the 16-bit paths,
    not ``sine_sensitive``.  ``case`` names a config of CONFIG_CASES; lo, hi: the band of |x|."""
    oracle = oracle_net(precision, case=case)
    x, d = mlp_candidates(3 * M + 64, seed=500 + M, lo=lo, hi=hi)
    if precision == "fp32":
        keep = kink_free(oracle, x, d, 2e-6)
    else:
        keep = model_kink_free(oracle, precision, x, d, 1e-5) & ~sine_sensitive(oracle, precision, x, d)
    return x[keep][:M].contiguous(), d[keep][:M].contiguous(), int(keep.sum())


def mlp_upstream(M, seed, scale=2.0 / (3 * 4096)):
    """Upstream gradients at the magnitude of a mean loss over 4096 rays."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, 3, generator=g) * scale, torch.randn(M, 1, generator=g) * scale


# ------------------------------------------- the MLP: references per config --
def live_column(case):
    """The x_enc column that is alone in its 32-column block (pos_freqs = 5: column 32)."""
    pos_dim = 3 * (1 + 2 * case_config("fp32", case).pos_freqs)
    return pos_dim - 1 if pos_dim % 32 == 1 else None


class _Accumulate64(ref.MfmaEmulatedNeRF):
    """The numerics model with every MFMA layer's products summed in fp64 (forward and
    backward) and rounded to fp32 once: the same 16-bit operands and the same roundings
    of dz, another summation order -- as the kernels' is another one."""

    def _lin(self, x, lin):
        dt = self.dtype
        return torch.nn.functional.linear(ref._FwdRound.apply(x, dt).double(), ref._FwdRound.apply(lin.weight, dt).double(),
                                          lin.bias.double()).float()


def reference_outputs(net, precision, x, d, g_rgb, g_sigma, twin=False):
    """Forward and gradients of ``net`` (an oracle; left unchanged) at the reference the
    precision is held to: fp64 autograd for fp32, the numerics model for bf16 / fp16
    (``twin``: its _Accumulate64 form).
    -> dict(rgb, sigma, g_x, g_d (None without view directions), grads: [(name, grad)])."""
    if precision == "fp32":
        base = copy.deepcopy(net).double()
        model, dt = base, F64
    else:
        base = copy.deepcopy(net)
        model, dt = ref.mfma_emulated_nerf(base, precision), torch.float32
        if twin:
            model = _Accumulate64(base, model.dtype, model.scale)
    base.zero_grad()
    xr, dr = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, d))  # the caller's stay untouched
    wr, ws = model(xr, dr)
    ((wr * g_rgb.to(dt)).sum() + (ws * g_sigma.to(dt)).sum()).backward()
    return dict(rgb=wr.detach(), sigma=ws.detach().reshape(-1), g_x=xr.grad, g_d=dr.grad,
                grads=[(n, p.grad) for n, p in base.named_parameters()])


@functools.lru_cache(maxsize=None)
def config_case(case, precision, M):
    """Inputs and reference of one (case, precision, M) of CONFIG_RUNS, computed once:
    kink-free samples (mlp_selected), upstream gradients at test_mlp_ragged's magnitudes
    (1 for fp32, a mean loss over 4096 rays for the 16-bit paths)."""
    x, d, survivors = mlp_selected(precision, M, case)
    g_rgb, g_sigma = mlp_upstream(M, seed=60 + M, scale=1.0 if precision == "fp32" else 2.0 / (3 * 4096))
    net = oracle_net(precision, case=case)
    want = reference_outputs(net, precision, x, d, g_rgb, g_sigma)
    out = dict(x=x, d=d, g_rgb=g_rgb, g_sigma=g_sigma, survivors=survivors, want=want, grad_bounds={}, twin={},
               oracle={})
    if precision != "fp32":
        out["twin"], out["oracle"], out["grad_bounds"] = model_conditioning(
            net, precision, x, d, g_rgb, g_sigma, want, ill_conditioned_names(case, precision))
    return out


# The parameters at which the numerics model is no reference to 1.5e-2: (case prefix,
# precision) -> trunk layers.  A static list; test_edge_inputs_host asserts that the
# model's twin justifies every entry and nothing else.
ILL_CONDITIONED = {("depth16", "fp16"): (0, 1, 2)}
TWIN_FACTOR = 1.5


def ill_conditioned_names(case, precision):
    layers = next((v for (c, p), v in ILL_CONDITIONED.items() if case and case.startswith(c) and p == precision), ())
    return [f"pts_linears.{i}.{k}" for i in layers for k in ("weight", "bias")]


def model_conditioning(net, precision, x, d, g_rgb, g_sigma, want, names):
    """Where the numerics model stops being a reference to 1.5e-2, and the bound there.

    The 1.5e-2 gradient bound presumes that the kernels and the model make the same
    roundings of dz and differ in summation order only (~1e-4 relative in fp16).  Rounding
    amplifies that difference: a share d / s of the values, s being the rounding step
    relative to the values, rounds the other way, each by s, so d'^2 ~ d^2 + d s per layer.
    While dz 2^14 is a normal fp16 number (s = 2^-11) that stays at 1e-4; where it is
    subnormal (depth 16 at the default initialisation under a mean loss over 4096 rays: at
    most 12 steps of 2^-24 at layer 0) d grows by ~2.4 per layer down the trunk.  The model's
    _Accumulate64 twin measures it on the CPU: 0.11 / 0.046 / 0.018 / 0.0075 from the model
    at layers 0..3 of depth16_skip4 in fp16, 1e-4 .. 3e-3 everywhere else.

    -> (twin: name -> distance of the twin's gradient from the model's,
        oracle: name -> distance of the model's gradient from the fp64 oracle's,
        bounds: for the parameters ``names`` (ill_conditioned_names) TWIN_FACTOR = 1.5 x the
                twin's distance: what another summation order of the same arithmetic does
                to the model, with half as much again for a third order; it stays below 1.0 x
                the model's distance from the fp64 oracle on the same samples, the bound
                the issue of this test names).
    Every other parameter keeps 1.5e-2."""
    t = reference_outputs(net, precision, x, d, g_rgb, g_sigma, twin=True)
    o = reference_outputs(net, "fp32", x, d, g_rgb, g_sigma)
    twin = {n: rel(g, w) for (n, g), (_, w) in zip(t["grads"], want["grads"])}
    oracle = {n: rel(w, g) for (n, g), (_, w) in zip(o["grads"], want["grads"])}
    return twin, oracle, {n: TWIN_FACTOR * twin[n] for n in names}


# test_fp32_backward's and test_16bit_non_default_configs_vs_numerics_model's bars; g_x / g_d:
# test_16bit_input_gradients_vs_numerics_model's
def config_bounds(precision):
    if precision == "fp32":
        return dict(rgb=1e-4, sigma=lambda s: 1e-4, grad=2e-5, g_x=2e-5, g_d=2e-5)
    return dict(rgb=1e-4, sigma=lambda s: 1e-3 * max(1.0, s), grad=1.5e-2, g_x=2e-2, g_d=1e-2)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def config_distances(got, want, case):
    """Every distance test_mlp_configs asserts, of ``got`` (rgb, sigma, g_x, g_d, grads as
    [(name, grad)]) from the reference: forward max errors, one relative 2-norm per named
    parameter and per input gradient, and -- a second encoding block with one live column
    vanishes in a whole matrix's norm -- that column of every x_enc-reading layer alone."""
    out = {"rgb": (got["rgb"].double() - want["rgb"].double()).abs().max().item(),
           "sigma": (got["sigma"].double() - want["sigma"].double()).abs().max().item(),
           "g_x": rel(got["g_x"], want["g_x"])}
    out["g_x[-1]"] = rel(got["g_x"][-1], want["g_x"][-1])  # the tile of one sample, which a norm over 513 rows hides
    if want["g_d"] is not None:
        out["g_d"] = rel(got["g_d"], want["g_d"])
        out["g_d[-1]"] = rel(got["g_d"][-1], want["g_d"][-1])
    col = live_column(case)
    pos_dim = None if col is None else col + 1
    for (name, g), (_, w) in zip(got["grads"], want["grads"]):
        out[name] = rel(g, w)
        if col is not None and name.startswith("pts_linears") and name.endswith("weight") and w.shape[1] != 256:
            assert w.shape[1] in (pos_dim, pos_dim + 256)
            out[name + f"[:, {col}]"] = rel(g[:, col], w[:, col])
    return out


def check_config_distances(dist, precision, sigma_max, grad_bounds=None):
    """-> the list of (name, distance, bound) that miss config_bounds (``grad_bounds``:
    config_case's bounds of the parameters at which the numerics model is ill-conditioned)."""
    b = config_bounds(precision)
    missed = []
    for name, v in dist.items():
        bound = b["sigma"](sigma_max) if name == "sigma" else b.get(name.replace("[-1]", ""), b["grad"])
        bound = max(bound, (grad_bounds or {}).get(name, 0.0))
        if not v < bound:
            missed.append((name, v, bound))
    return missed


# -------------------------------------------- the MLP at scene scale (section 3) --
SCENE_M, SCENE_LO, SCENE_HI = 513, 4.0, 10.0
SCENE_PARAMS = ("pts_linears.0.weight", "pts_linears.0.bias", "pts_linears.5.weight", "pts_linears.5.bias")


@functools.lru_cache(maxsize=None)
def scene_case(precision):
    """The default model at M = 513 with |x_c| uniform in 4 .. 10 (lego positions reach 10):
    2^9 x exceeds 800 revolutions, and 2^k x is exact in fp32, so the references are well
    defined.  Kink-free samples by mlp_selected's rule; upstream as config_case."""
    x, d, survivors = mlp_selected(precision, SCENE_M, None, SCENE_LO, SCENE_HI)
    g_rgb, g_sigma = mlp_upstream(SCENE_M, seed=80, scale=1.0 if precision == "fp32" else 2.0 / (3 * 4096))
    want = reference_outputs(oracle_net(precision), precision, x, d, g_rgb, g_sigma)
    return dict(x=x, d=d, g_rgb=g_rgb, g_sigma=g_sigma, survivors=survivors, want=want)


def scene_distances(got, want):
    """g_x, g_d and the gradients of the layers that read x_enc (layer 0 and the layer
    after the skip): what flows through the encoding's backward.  rgb as the existing
    scene-scale forward test holds it."""
    dist = config_distances(got, want, None)
    return {k: v for k, v in dist.items() if k in ("rgb", "g_x", "g_d", "g_x[-1]", "g_d[-1]") + SCENE_PARAMS}


# ------------------------- the fp16 backward across gradient magnitudes (section 4) --
FP16_SCALE_M = [33, 513]
FP16_BATCHES = [65536, 4096, 512, 64, 8]
# (B, outlier): upstream gradients of a mean loss over B rays; outlier: one sample's g_sigma
# 1e4 times the others.  The numerics model stays finite at every one (asserted on the host),
# so every one is run on the GPU.
FP16_SCALE_RUNS = [(B, False) for B in FP16_BATCHES] + [(4096, True)]
FP16_MAX = 65504.0


def fp16_upstream(M, B, outlier):
    g_rgb, g_sigma = mlp_upstream(M, seed=70 + M, scale=2.0 / (3 * B))
    if outlier:
        g_sigma[M // 2] *= 1e4
    return g_rgb, g_sigma


def fp16_model_run(x, d, g_rgb, g_sigma):
    """The fp16 numerics model of the default net -> (its outputs, every dz it stores in
    fp16 -- scaled by 2^14 -- in backward order: the MFMA layers' and the two heads')."""
    stored = []
    orig_round, orig_head = ref._GradRound.backward, ref._HeadLinear.backward

    def spy_round(ctx, g):
        stored.append((g * ctx.scale).to(ctx.dtype))
        return orig_round(ctx, g)

    def spy_head(ctx, g):
        stored.append((g * ctx.scale).to(ctx.dtype))
        return orig_head(ctx, g)
    ref._GradRound.backward, ref._HeadLinear.backward = staticmethod(spy_round), staticmethod(spy_head)
    try:
        want = reference_outputs(oracle_net("fp16"), "fp16", x, d, g_rgb, g_sigma)
    finally:
        ref._GradRound.backward, ref._HeadLinear.backward = staticmethod(orig_round), staticmethod(orig_head)
    return want, stored


@functools.lru_cache(maxsize=None)
def fp16_scale_case(M, B, outlier):
    x, d, survivors = mlp_selected("fp16", M)
    g_rgb, g_sigma = fp16_upstream(M, B, outlier)
    want, stored = fp16_model_run(x, d, g_rgb, g_sigma)
    return dict(x=x, d=d, g_rgb=g_rgb, g_sigma=g_sigma, survivors=survivors, want=want, stored=stored)


# ------------------- the skipping backward on structured active-tile patterns --
# (test_tile_patterns.py)  A tile is 32 samples; tile_flags_kernel writes one flag byte per
# tile (four to a flag word) and one count per 64-tile block; a dX workgroup takes W active
# tiles (8 waves in 16 bit, 4 in fp32) of one 256-tile segment.
TILE, WORD_TILES, BLOCK_TILES, SEG_TILES = 32, 4, 64, 256
M_A = 10_245  # 321 tiles, two segments: segment 1 = one full block + a block of one 5-sample tile
M_B = 20_485  # 641 tiles, three segments: segment 2 = 129 tiles, its fourth block empty
TILE_PRECISIONS = ["bf16", "fp16", "fp32"]

_FIXED_PATTERNS = {  # at M_B
    "first_only": (0,),
    "block_edges": (319, 320, 383, 384, 447, 448),
    # a word boundary (3 | 4, 7 | 8), one full flag word (12 .. 15), one tile at each byte position (16, 21, 26, 31)
    "word_edges": (3, 4, 7, 8, 12, 13, 14, 15, 16, 21, 26, 31),
    "middle_only": (256, 259, 260, 319, 320, 383, 384, 449, 511),       # nine tiles, all in segment 1
    "ends_only": (0, 63, 64, 200, 255, 512, 575, 576, 639, 640),        # five each in segments 0 and 2
    "last_segment_empty": (0, 5, 63, 64, 255, 256, 300, 447, 448, 511),  # five each in segments 0 and 1
}
NAMED_PATTERNS = ["first_only", "last_partial_only", "seg_edges", "block_edges", "word_edges", "middle_only", "ends_only",
                  "last_segment_empty", "per_part_3_4_5", "per_part_7_8_9", "one_full_segment", "all_but_one"]
REFERENCE_PATTERNS = [n for n in NAMED_PATTERNS if n != "all_but_one"]  # (20k selected samples: dense run only)
# the stale-scratch and graph-replay tests walk these in this order, refilling nothing in between
STALE_SEQUENCE = ["all_active", "seg_edges", "none_active", "one_full_segment", "last_partial_only", "all_active"]


def n_tiles(M):
    return (M + TILE - 1) // TILE


def _spread(lo, size, n):
    """n tiles of [lo, lo + size): the first, the last and even steps between."""
    return [lo + (i * (size - 1)) // (n - 1) for i in range(n)]


def named_tiles(name, M=M_B):
    """The active tiles of a named pattern, increasing.  The names of _FIXED_PATTERNS and the
    per_part ones are sets at M_B; the others follow M: ``seg_edges`` the tile on either side
    of every segment boundary, ``one_full_segment`` the last segment of 256 tiles (segment 1
    at M_B, segment 0 at M_A), ``last_partial_only`` the last tile."""
    T = n_tiles(M)
    nseg = (T + SEG_TILES - 1) // SEG_TILES
    if name == "all_active":
        return tuple(range(T))
    if name == "none_active":
        return ()
    if name == "last_partial_only":
        assert M % TILE
        return (T - 1,)
    if name == "seg_edges":
        return tuple(t for s in range(1, nseg) for t in (s * SEG_TILES - 1, s * SEG_TILES))
    if name == "one_full_segment":
        s = T // SEG_TILES - 1
        return tuple(range(s * SEG_TILES, (s + 1) * SEG_TILES))
    assert M == M_B, (name, M)
    if name == "all_but_one":
        return tuple(t for t in range(T) if t != 300)
    if name.startswith("per_part_"):
        counts = [int(v) for v in name.split("_")[2:]]
        assert len(counts) == nseg
        return tuple(t for s, n in enumerate(counts) for t in _spread(s * SEG_TILES, min(SEG_TILES, T - s * SEG_TILES), n))
    return _FIXED_PATTERNS[name]


# the count sweep at M_A: the first n tiles of a fixed order -- the partial last tile, both
# sides of the segment boundary, tile 0, then a seeded permutation of the rest
SWEEP_COUNTS = list(range(1, 2 * (n_tiles(M_A) // 16) + 2))  # 1 .. 41; tiles // 16 caps the dW chunks per job
OTHER_MODELS = ["depth16_skips_0_3_6_9_12", "depth3_skip1_no_view_dirs", "depth2_skip0"]
OTHER_MODEL_COUNTS = [1, 2, 7, 8, 9, 11, 12, 13, 14, 15, 19, 20, 21, 40, 41]
OTHER_MODEL_SET = (255, 256, 320)
OTHER_MODEL_PRECISIONS = ["bf16", "fp32"]


@functools.lru_cache(maxsize=None)
def sweep_order(M=M_A):
    head = [n_tiles(M) - 1, SEG_TILES - 1, SEG_TILES, 0]
    rest = [t for t in range(n_tiles(M)) if t not in head]
    perm = torch.randperm(len(rest), generator=torch.Generator().manual_seed(4242)).tolist()
    return tuple(head + [rest[i] for i in perm])


def sweep_tiles(n, M=M_A):
    return tuple(sorted(sweep_order(M)[:n]))


def other_model_sets():
    """(id, tiles) of the non-default models' runs at M_A."""
    return [(f"count{n}", sweep_tiles(n)) for n in OTHER_MODEL_COUNTS] + [("seg_edges_last", OTHER_MODEL_SET)]


# Which values count as zero (M_A): three tiles that are active through ONE component of
# ONE sample -- g_sigma of sample 31 of tile 7, g_rgb[:, 2] of sample 0 of tile 256, and
# g_sigma of the last valid row M - 1 -- alone, with a tile (130) whose upstream is -0.0
# throughout, or with a tile (200) whose only nonzero is the fp32 denormal 1e-42 (g_sigma of
# its sample 13).  Components: 0..2 = g_rgb columns, 3 = g_sigma.
ZERO_SINGLES = ((7 * TILE + 31, 3), (256 * TILE, 2), (M_A - 1, 3))
ZERO_RULE_CASES = {
    "single_components": dict(),
    "negative_zero_tile": dict(negzero=(130,)),
    "denormal_only_tile": dict(denormal=((200 * TILE + 13, 3),)),
}
DENORMAL = 1e-42
SINGLES_SPARE = 8  # spare selected samples per single-component row (see tile_case)


class _Jittered(ref.MfmaEmulatedNeRF):
    """The numerics model with every MFMA layer's pre-activation moved by ``amp`` of its size
    (at least 1e-3): what some other summation orders do to it, as noise."""

    amp, gen = 4e-6, None  # (amp carries the sign of an antithetic run)

    def _lin(self, x, lin):
        out = super()._lin(x, lin)
        return out + out.detach().abs().clamp_min(1e-3) * self.amp * torch.randn(out.shape, generator=self.gen)


class _JitteredEncoding(torch.nn.Module):
    """The oracle's encoding with its sines and cosines moved by ``amp`` (absolute; the kernels'
    hardware sine behind pe_rev's argument reduction is ~1e-6 from torch's)."""

    def __init__(self, enc, gen, amp):
        super().__init__()
        self.enc, self.gen, self.amp, self.output_dim = enc, gen, amp, enc.output_dim

    def forward(self, v):
        e = self.enc(v)
        noise = self.amp * torch.randn(e.shape, generator=self.gen)
        noise[..., :v.shape[-1]] = 0.0  # the input's own columns are exact
        return e + noise


# JITTER_PAIRS antithetic pairs of runs: the same noise with either sign, so that a value within
# |noise| of a rounding boundary crosses it in one run of the pair whichever side it is on.
# One-sided runs miss half of them: with four such runs 2 of 287 GPU cases still met a fragile sample.
JITTER_PAIRS, JITTER_AMP, JITTER_TOL = 4, 4e-6, 1e-3


def jitter_fragile(oracle, precision, x, d):
    """16 bit: the samples whose input gradient under the numerics model moves by more than
    JITTER_TOL (relative, per sample) in any of 2 JITTER_PAIRS runs of the model with its sines
    and its MFMA pre-activations jittered by +-JITTER_AMP.

    Why: the model rounds the encoding, every activation and every dz to 16 bits.  A sine that
    the hardware computes 1e-6 off, or a pre-activation that another summation order moves by
    1e-7, can round the other way (2^-8 of its size in bf16), which moves the next layer's
    pre-activations by 3e-5 .. 4e-4 and carries ReLUs across zero far inside mlp_selected's
    1e-5 margin; ``sine_sensitive`` sees this only where the FORWARD moves, and a flipped
    ReLU at z ~ 0 moves only the backward.  For most samples nothing changes at all (the median
    move is exactly 0); for ~10 % in bf16 (2 % in fp16) the sample's backward path changes (its
    g_x moves by 1 % .. 100 %), and among a few hundred samples ONE such sample moves the
    trunk's parameter gradients by 1 .. 7 %.  On mlp_selected's samples the kernels measured
    1.5 .. 4.9e-2 from the model at trunk layers on 5 of the first 97 sample sets of
    test_tile_patterns -- the same figure for two patterns that share a sample set -- while
    every fp32 case, every forward and the dense run of the same kernels agreed; the model
    jittered like this is as far from itself.  Such a sample has no reference to 1.5e-2, so the
    patterns are built without them; the kernels then stay within 1.5e-3 (bf16) and 4.8e-3
    (fp16) of the model on every one of test_tile_patterns' 155 16-bit sample sets."""
    model = ref.mfma_emulated_nerf(copy.deepcopy(oracle), precision)
    g_rgb, g_sigma = mlp_upstream(x.shape[0], seed=4300, scale=upstream_scale(precision))

    def input_grads(m):
        xr, dr = x.clone().requires_grad_(True), d.clone().requires_grad_(True)
        wr, ws = m(xr, dr)
        ((wr * g_rgb).sum() + (ws * g_sigma).sum()).backward()
        return xr.grad if dr.grad is None else torch.cat([xr.grad, dr.grad], -1)

    g0 = input_grads(model)
    worst = torch.zeros(x.shape[0])
    for k in range(2 * JITTER_PAIRS):
        gen = torch.Generator().manual_seed(4400 + k // 2)  # the pair draws the same noise
        amp = JITTER_AMP * (1 - 2 * (k % 2))
        alt = copy.deepcopy(oracle)
        alt.pos_encoder = _JitteredEncoding(oracle.pos_encoder, gen, amp)
        alt.dir_encoder = _JitteredEncoding(oracle.dir_encoder, gen, amp)
        jit = _Jittered(alt, model.dtype, model.scale)
        jit.amp, jit.gen = amp, gen
        worst = torch.maximum(worst, (input_grads(jit) - g0).norm(dim=-1) / g0.norm(dim=-1).clamp_min(1e-30))
    return worst > JITTER_TOL


TILE_POOL = 41 * TILE  # the largest sample count of the sweeps at M_A


@functools.lru_cache(maxsize=None)
def _stable_pool(precision, n, case):
    xs, ds, _ = mlp_selected(precision, (2 * n if n <= TILE_POOL else n + n // 2) + 32, case)
    keep = ~jitter_fragile(oracle_net(precision, case=case), precision, xs, ds)
    return xs[keep].contiguous(), ds[keep].contiguous()


def tile_selected(precision, A, case=None):
    """(x, d, survivors) of the A samples a tile pattern scatters: fp32 mlp_selected(precision,
    A, case); 16 bit the first A samples of a pool, the samples of mlp_selected(precision,
    2 n + 32, case) that are not ``jitter_fragile``, with n = TILE_POOL for A up to it (the sets
    of the sweeps are nested, and the filter runs once per model); above it n = A of 1.5 A + 32.
    survivors: the size of the pool."""
    if precision == "fp32":
        return mlp_selected(precision, A, case)
    xs, ds = _stable_pool(precision, TILE_POOL if A <= TILE_POOL else A, case)
    return xs[:A].contiguous(), ds[:A].contiguous(), xs.shape[0]


def tile_rows(tiles, M):
    """The valid rows of ``tiles``, increasing."""
    if not len(tiles):
        return torch.zeros(0, dtype=torch.long)
    r = (torch.tensor(sorted(tiles))[:, None] * TILE + torch.arange(TILE)[None]).reshape(-1)
    return r[r < M]


def expected_active(g_rgb, g_sigma):
    """Per tile: any component ``!= 0`` on the host (so -0.0 is zero and a denormal or NaN is
    not) -> bool per tile."""
    M = g_rgb.shape[0]
    nz = (g_rgb != 0).any(-1) | (g_sigma.reshape(M, -1) != 0).any(-1)
    return torch.nn.functional.pad(nz, (0, (-M) % TILE)).reshape(-1, TILE).any(-1)


def upstream_scale(precision):
    """test_mlp_ragged's magnitudes: 1 for fp32, a mean loss over 4096 rays in 16 bit."""
    return 1.0 if precision == "fp32" else 2.0 / (3 * 4096)


@functools.lru_cache(maxsize=None)
def tile_case(precision, M, tiles, case=None, singles=(), negzero=(), denormal=(), selected=True):
    """Inputs of one active-tile pattern: M rows of x, d, g_rgb, g_sigma on the host.

    ``tiles`` are active throughout; ``singles`` = (row, component) are samples with that one
    component nonzero in an otherwise zero tile.  Those rows -- ``rows``, A of them -- hold the
    A kink-free samples of tile_selected(precision, A, case), in order, and the upstream
    gradient mlp_upstream(A) (singles: masked to the one component); with ``selected=False``
    (patterns that are compared with the dense run only) they keep the candidates below and
    take mlp_upstream(M).  Every other row holds an mlp_candidates sample with a zero
    upstream gradient: +0.0, or -0.0 throughout the tiles ``negzero``, or DENORMAL at the
    (row, component) entries of ``denormal``.  A sample with zero upstream gradient
    contributes exactly nothing, so ``want``, reference_outputs on the A rows alone, is the
    reference of the whole pattern (a DENORMAL entry adds less than 1e-38 to any sum).
    ``active``: expected_active of the host tensors; ``count`` their number."""
    tiles = tuple(sorted(tiles))
    T = n_tiles(M)
    assert all(0 <= t < T for t in tiles) and len(set(tiles)) == len(tiles)
    rows = torch.cat([tile_rows(tiles, M), torch.tensor([r for r, _ in singles], dtype=torch.long)]).sort().values
    A = rows.numel()
    assert rows.unique().numel() == A
    x, d = mlp_candidates(M, seed=4000 + M)
    g_rgb, g_sigma = torch.zeros(M, 3), torch.zeros(M, 1)
    scale = upstream_scale(precision)
    out = dict(tiles=tiles, rows=rows, A=A, survivors=None, want=None)
    if selected and A:
        xs, ds, out["survivors"] = tile_selected(precision, A + SINGLES_SPARE * len(singles), case)
        if singles:
            # a sample that is active through g_sigma alone needs sigma > 0 (ReLU'), or it is
            # active and contributes nothing: such rows take the next sample with a live sigma
            zr, zs = torch.zeros(xs.shape[0], 3), torch.zeros(xs.shape[0], 1)
            live = reference_outputs(oracle_net(precision, case=case), precision, xs, ds, zr, zs)["sigma"] > 0
            sigma_only = {r for r, comp in singles if comp == 3}
            free, order = list(range(xs.shape[0])), []
            for r in rows.tolist():
                order.append(next(i for i in free if live[i] or r not in sigma_only))
                free.remove(order[-1])
            xs, ds = xs[order], ds[order]
        assert xs.shape[0] == A, "too few kink-free candidates"
        out.update(sel_x=xs, sel_d=ds)
        ur, us = mlp_upstream(A, seed=4100 + A, scale=scale)
        x[rows], d[rows] = xs, ds
        g_rgb[rows], g_sigma[rows] = ur, us
    elif A:
        ur, us = mlp_upstream(M, seed=4100 + M, scale=scale)
        g_rgb[rows], g_sigma[rows] = ur[rows], us[rows]
    for r, comp in singles:
        keep = torch.cat([g_rgb[r], g_sigma[r]])[comp].clone()
        assert keep != 0
        g_rgb[r], g_sigma[r] = 0.0, 0.0
        (g_rgb[r] if comp < 3 else g_sigma[r])[comp % 3] = keep
    for t in negzero:
        g_rgb[t * TILE:(t + 1) * TILE] = -0.0
        g_sigma[t * TILE:(t + 1) * TILE] = -0.0
    for r, comp in denormal:
        (g_rgb[r] if comp < 3 else g_sigma[r])[comp % 3] = DENORMAL
    active = expected_active(g_rgb, g_sigma)
    out.update(x=x, d=d, g_rgb=g_rgb, g_sigma=g_sigma, active=active, count=int(active.sum()))
    if selected and A:
        out["want"] = reference_outputs(oracle_net(precision, case=case), precision, x[rows], d[rows], g_rgb[rows],
                                        g_sigma[rows])
    return out


def named_case(precision, name, M=M_B, selected=None):
    selected = name in REFERENCE_PATTERNS if selected is None else selected
    return tile_case(precision, M, named_tiles(name, M), selected=selected)


def zero_rule_case(precision, name):
    return tile_case(precision, M_A, (), singles=ZERO_SINGLES, **ZERO_RULE_CASES[name])


def tile_moves(c, precision, case, tile):
    """How far the reference's parameter gradients move when the upstream gradient of one
    active tile is zeroed: name -> |g - g_without| / |g|.  The reference is a sum over
    samples (every rounding of the numerics model is per sample), so g - g_without is the
    reference of that tile's rows alone; test_edge_inputs_host holds this shortcut to the
    recomputation itself."""
    rows = c["rows"]
    own = rows[(rows // TILE) == tile]
    assert own.numel() > 0
    part = reference_outputs(oracle_net(precision, case=case), precision, c["x"][own], c["d"][own], c["g_rgb"][own],
                             c["g_sigma"][own])
    return {n: (g.double().norm() / w.double().norm().clamp_min(1e-300)).item()
            for (n, g), (_, w) in zip(part["grads"], c["want"]["grads"])}


def teeth_tiles(c):
    """The first, a middle and the last tile that holds reference rows."""
    ts = sorted(set((c["rows"] // TILE).tolist()))
    return sorted({ts[0], ts[len(ts) // 2], ts[-1]})
