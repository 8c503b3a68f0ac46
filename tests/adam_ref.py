"""CPU reference of the optimizer tail: clip_grad_norm_ + torch.optim.Adam on flat tensors.

A plain restatement of what the reference's training loops run after the backward
(train.py:112-117, train_pose_opt.py:398-409: ``clip_grad_norm_`` per clip group, then
``torch.optim.Adam`` with amsgrad=False and weight_decay=0), on flat tensors of any floating
dtype and in place, in torch's own order of operations:

    coef = min(1, max_norm / (sqrt(sumsq) + 1e-6))          NaN stays NaN (torch.clamp)
    g *= coef
    m.lerp_(g, 1 - b1)
    v = b2 v + (1 - b2) g^2
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)         bc1, bc2 in double

test_adam_ref.py holds it, in float64, to torch.optim.Adam + clip_grad_norm_ themselves, so
the tests of the HIP kernels and of FusedAdam's host logic compare against torch and never
against the code under test.  In float32 it is the stand-in kernel of
test_fused_adam_host.py; in float64 it is the oracle of test_optim_edges.py."""
import math

import torch

BETAS = (0.9, 0.999)
EPS = 1e-8


def clip_coef(sumsq, max_norm):
    """clip_grad_norm_'s coefficient from a squared norm, in the dtype of ``sumsq`` (a
    tensor, or a number taken as float64); a NaN norm gives NaN, as torch.clamp does."""
    if not isinstance(sumsq, torch.Tensor):
        sumsq = torch.tensor(sumsq, dtype=torch.float64)
    return torch.clamp(max_norm / (sumsq.sqrt() + 1e-6), max=1.0)


def sched_values(lr, b1, b2, step):
    """(lr / bc1, sqrt(bc2)) in double: the two scalars of a step that depend on its number."""
    return lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)


def adam_step(p, g, m, v, step, lr, betas=BETAS, eps=EPS, coef=None):
    """One Adam step in place on the flat tensors p, g, m, v of one dtype; ``step`` is the
    number of this step (>= 1), ``coef`` the clip coefficient g is scaled by first (None:
    no clip group; torch multiplies also by a coefficient of exactly 1)."""
    b1, b2 = betas
    if coef is not None:
        g.mul_(torch.as_tensor(coef).to(g.dtype))
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    step_size, bc2_sqrt = sched_values(lr, b1, b2, step)
    denom = (v.sqrt() / bc2_sqrt).add_(eps)
    p.addcdiv_(m, denom, value=-step_size)
