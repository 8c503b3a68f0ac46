"""The yardstick of the robust-loss tests (test_robust_loss_host.py on the CPU,
test_robust_loss.py on the device): the loss family of include/nerf_hip.h in plain torch,
differentiable by autograd, in any dtype.

Per colour channel, with d = pred - target, a scale c > 0 and q = (d / c)^2:

    kind            rho(d)                                  w(d)   (rho' = 2 d w)
    mse             d^2                                     1
    huber           d^2 if |d| <= c else 2 c |d| - c^2      1 if |d| <= c else c / |d|
    charbonnier     2 d^2 / (1 + sqrt(1 + q))               1 / sqrt(1 + q)
    cauchy          c^2 log1p(q)                            1 / (1 + q)
    geman_mcclure   d^2 / (1 + q)                           1 / (1 + q)^2

The loss is the mean of rho over the 3B channels.  Every function casts its inputs to
``dtype`` first and then performs the kernel's operations in the kernel's documented order
(the header's "fp32 operation order"), one torch operation per rounding, with c the fp32
number the kernel receives.  So ``dtype=torch.float64`` on fp32 inputs is the truth about
those inputs and ``dtype=torch.float32`` is what the kernel's own arithmetic makes of them,
up to the order of the final sum and the last place of log1p.
"""
import torch

F32, F64 = torch.float32, torch.float64
KINDS = ("mse", "huber", "charbonnier", "cauchy", "geman_mcclure")


def _c(c, dtype):
    return torch.tensor(float(c), dtype=F32).to(dtype)


def rho(d, kind, c):
    """rho(d) elementwise in d's dtype; differentiable."""
    c = _c(c, d.dtype)
    d2 = d * d
    if kind == "mse":
        return d2
    if kind == "huber":
        a = d.abs()
        return torch.where(a <= c, d2, (2.0 * c) * a - c * c)
    u = d / c
    q = u * u
    if kind == "charbonnier":
        return (2.0 * d2) / (1.0 + torch.sqrt(1.0 + q))
    if kind == "cauchy":
        return (c * c) * torch.log1p(q)
    if kind == "geman_mcclure":
        return d2 / (1.0 + q)
    raise ValueError(kind)


def weight(d, kind, c):
    """The IRLS weight w(d) elementwise in d's dtype."""
    c = _c(c, d.dtype)
    if kind == "mse":
        return torch.ones_like(d)
    if kind == "huber":
        a = d.abs()
        # c / a only where it is used (a == 0 lies on the other branch)
        return torch.where(a <= c, torch.ones_like(d), c / torch.where(a <= c, torch.ones_like(a), a))
    u = d / c
    q = u * u
    if kind == "charbonnier":
        return 1.0 / torch.sqrt(1.0 + q)
    if kind == "cauchy":
        return 1.0 / (1.0 + q)
    if kind == "geman_mcclure":
        t = 1.0 + q
        return 1.0 / (t * t)
    raise ValueError(kind)


def loss(pred, target, kind, c):
    """mean rho(pred - target), differentiable, in pred's dtype."""
    return rho(pred - target.to(pred.dtype), kind, c).mean()


def loss_and_grad(pred, target, kind, c, scale=1.0, dtype=F64):
    """(mean rho, mean d^2, scale * d(mean rho)/d pred) in ``dtype``, closed form, in the
    kernel's order: g = ((2 d) inv) scale w with inv = 1 / (3B)."""
    d = pred.to(dtype) - target.to(dtype)
    n = d.numel()
    inv = torch.ones((), dtype=dtype) / n
    g = ((2.0 * d) * inv) * torch.tensor(float(scale), dtype=F32).to(dtype)
    if kind != "mse":
        g = g * weight(d, kind, c)
    return rho(d, kind, c).sum() * inv, (d * d).sum() * inv, g


def inputs(B, seed=0, equal=False):
    """Uniform colours and targets (B,3) in fp32; ``equal``: pred == target."""
    g = torch.Generator().manual_seed(9000 + 7 * B + seed)
    pred = torch.rand(B, 3, generator=g)
    return pred, pred.clone() if equal else torch.rand(B, 3, generator=g)
