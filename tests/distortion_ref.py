"""The yardstick of the distortion-loss tests (test_distortion_host.py on the CPU,
test_distortion.py on the device): a plain torch restatement of the definition, differentiable
by autograd, in any dtype, plus the inputs both files share.

Per ray, with nondecreasing samples z_0 <= ... <= z_{S-1} in [near, far] and weights w_i:

    s_i = (z_i - near) / (far - near);  e_i = s_i (i < S), e_S = 1
    m_i = (e_i + e_{i+1}) / 2,  d_i = e_{i+1} - e_i
    L   = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i

``loss_rays_pairs`` evaluates exactly that, O(S^2); ``loss_rays_prefix`` the exclusive-prefix
form the kernel uses; ``grad_closed`` the closed-form dL/dw.  Every input is cast to ``dtype``
first, so ``dtype=torch.float64`` on fp32 inputs is the truth about those inputs and
``dtype=torch.float32`` is what plain fp32 arithmetic makes of them.
"""
import torch

F32, F64 = torch.float32, torch.float64


def intervals(z, near, far, dtype=F64):
    """(m, d): midpoints and lengths (B, S) of the normalised intervals, the last closed at 1."""
    s = (z.to(dtype) - near) / (far - near)
    e = torch.cat([s, torch.ones_like(s[..., :1])], -1)
    return 0.5 * (e[..., :-1] + e[..., 1:]), e[..., 1:] - e[..., :-1]


def loss_rays_pairs(w, z, near, far, dtype=F64):
    """L per ray (B,), the definition's double sum."""
    w = w.to(dtype)
    m, d = intervals(z, near, far, dtype)
    pair = (w[..., :, None] * w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum((-1, -2))
    return pair + (w * w * d).sum(-1) / 3.0


def loss_rays_prefix(w, z, near, far, dtype=F64):
    """L per ray (B,) from exclusive prefix sums: 2 sum_i w_i (m_i W_<i - M_<i) + self terms."""
    w = w.to(dtype)
    m, d = intervals(z, near, far, dtype)
    wm = w * m
    W_lt = torch.cumsum(w, -1) - w
    M_lt = torch.cumsum(wm, -1) - wm
    return 2.0 * (w * (m * W_lt - M_lt)).sum(-1) + (w * w * d).sum(-1) / 3.0


def grad_closed(w, z, near, far, dtype=F64):
    """dL/dw (B, S) of the per-ray L: 2 [m_i (W_<i - W_>i) - (M_<i - M_>i)] + (2/3) w_i d_i."""
    w = w.to(dtype)
    m, d = intervals(z, near, far, dtype)
    wm = w * m
    W_lt = torch.cumsum(w, -1) - w
    M_lt = torch.cumsum(wm, -1) - wm
    W_gt = w.sum(-1, keepdim=True) - W_lt - w
    M_gt = wm.sum(-1, keepdim=True) - M_lt - wm
    return 2.0 * (m * (W_lt - W_gt) - (M_lt - M_gt)) + (2.0 / 3.0) * w * d


def loss_and_grad(w, z, near, far, dtype=F64, form=loss_rays_pairs):
    """(mean L over the rays, L per ray, d(mean L)/dw by autograd) in ``dtype``."""
    wd = w.detach().to(dtype).requires_grad_(True)
    rays = form(wd, z, near, far, dtype)
    loss = rays.mean()
    (g,) = torch.autograd.grad(loss, wd)
    return loss.detach(), rays.detach(), g


def pairs_loss_and_grad(w, z, near, far, dtype=F64):
    """(mean L, L per ray, d(mean L)/dw) of the O(S^2) form without autograd, a few rays at a
    time so that S = 4096 fits: with A_ij = |m_i - m_j|, L = w.Aw + (1/3) sum w^2 d and
    dL/dw = 2 Aw + (2/3) w d (test_distortion_host.py holds it to autograd of
    ``loss_rays_pairs``)."""
    B, S = z.shape
    step = max(1, (1 << 24) // (S * S))
    rays, grads = [], []
    for a in range(0, B, step):
        wc = w[a:a + step].to(dtype)
        m, d = intervals(z[a:a + step], near, far, dtype)
        Aw = ((m[:, :, None] - m[:, None, :]).abs() @ wc[:, :, None])[..., 0]
        rays.append((wc * Aw).sum(-1) + (wc * wc * d).sum(-1) / 3.0)
        grads.append(2.0 * Aw + (2.0 / 3.0) * wc * d)
    rays = torch.cat(rays)
    return rays.mean(), rays, torch.cat(grads) / B


# ---- shared inputs (fp32, CPU) ---------------------------------------------------------------
def sorted_z(B, S, near, far, gen, ties=False):
    """Nondecreasing depths in [near, far]; with ``ties`` they repeat in runs of three."""
    z = near + (far - near) * torch.rand(B, S, generator=gen)
    if ties:
        z = z[:, torch.arange(S) // 3 * 3]
    return torch.sort(z, -1).values.to(F32)


def composite_weights(sigma, z):
    """raw2outputs' weights of densities ``sigma`` (B, S) along unit-length rays, by the oracle
    (the last interval is its 1e10, so whatever transmittance is left lands on the last sample)."""
    from oracle import refimpl as ref
    B, S = z.shape
    if S == 1:  # the oracle builds its intervals from z[1:] - z[:-1] and needs two samples
        return (1.0 - torch.exp(-torch.relu(sigma) * 1e10)).to(F32)
    rays_d = torch.zeros(B, 3)
    rays_d[:, 2] = 1.0
    return ref.raw2outputs(torch.zeros(B, S, 3), sigma[..., None], z, rays_d)["weights"].to(F32)


def uniform_sigma(B, S, gen):
    """sigma ~ U[0, 3)."""
    return 3.0 * torch.rand(B, S, generator=gen)


def peaked_sigma(B, S):
    """50 on (up to) six mid-ray samples over a 1e-3 floor."""
    sigma = torch.full((B, S), 1e-3)
    lo = max(0, S // 2 - 3)
    sigma[:, lo:min(S, lo + 6)] = 50.0
    return sigma
