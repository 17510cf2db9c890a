"""Plain fp64 references of BatchNorm1d / LayerNorm (+ activation), forward and backward, as the
explicit formulas the kernels of csrc/norm.hip implement — the specification, not a call into
torch's fused ops (F.batch_norm refuses M = 1 in training).  Everything is computed from the fp32
input VALUES in double (x.double()), on whatever device the inputs live on.

    forward   mean = sum x / M,  var = sum (x - mean)^2 / M (biased),  rstd = 1 / sqrt(var + eps)
              xhat = (x - mean) rstd,  z = xhat gamma + beta,  y = act(z)
              run_mean' = (1 - m) run_mean + m mean
              run_var'  = (1 - m) run_var + m var M / (M - 1)      (M > 1; var itself for M = 1)
    backward  dz = dy act'(z),  dbeta = sum dz,  dgamma = sum dz xhat
              dx = gamma rstd (dz - dbeta / M - xhat dgamma / M)

LayerNorm is the same with the sums taken over a row's C columns instead of a channel's M rows
(dgamma / dbeta stay column sums over the rows).
"""
import math

import torch

ACT = {"none": 0, "relu": 1, "gelu": 2, "tanh": 3}
KINK = 1e-4   # ReLU pre-activations closer to 0 than this may fall on either side in fp32


def act_f(z, act):
    if act == "relu":
        return z.clamp_min(0)
    if act == "gelu":
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))
    if act == "tanh":
        return torch.tanh(z)
    assert act == "none", act
    return z


def act_d(z, act):
    if act == "relu":
        return (z > 0).to(z.dtype)
    if act == "gelu":
        return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    if act == "tanh":
        return 1 - torch.tanh(z) ** 2
    assert act == "none", act
    return torch.ones_like(z)


def bn_stats(x, eps):
    """(mean, biased var, rstd) per channel of x (M, C), double."""
    x = x.double()
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_running(mean, var, M, run_mean, run_var, momentum):
    unb = var * (M / (M - 1.0)) if M > 1 else var
    return ((1 - momentum) * run_mean.double() + momentum * mean,
            (1 - momentum) * run_var.double() + momentum * unb)


def bn_apply(x, mean, rstd, gamma, beta, act):
    """(y, z) from given statistics."""
    z = (x.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()
    return act_f(z, act), z


def bn_fwd(x, gamma, beta, act, eps=1e-5, run_mean=None, run_var=None, momentum=0.9):
    """dict(mean, var, rstd, z, y[, run_mean, run_var])."""
    mean, var, rstd = bn_stats(x, eps)
    y, z = bn_apply(x, mean, rstd, gamma, beta, act)
    out = dict(mean=mean, var=var, rstd=rstd, z=z, y=y)
    if run_mean is not None:
        out["run_mean"], out["run_var"] = bn_running(mean, var, x.shape[0], run_mean, run_var, momentum)
    return out


def bn_bwd(dy, x, gamma, beta, act, eps=1e-5):
    """dict(dx, dgamma, dbeta) from scratch (its own fp64 statistics)."""
    mean, _, rstd = bn_stats(x, eps)
    xhat = (x.double() - mean) * rstd
    g = gamma.double()
    dz = dy.double() * act_d(xhat * g + beta.double(), act)
    M = x.shape[0]
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    dx = g * rstd * (dz - dbeta / M - xhat * (dgamma / M))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def ln_fwd(x, gamma, beta, act, eps=1e-5):
    """dict(xhat, rstd, z, y) per row of x (R, C)."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    z = xhat * gamma.double() + beta.double()
    return dict(xhat=xhat, rstd=rstd[:, 0], z=z, y=act_f(z, act))


def ln_bwd(dy, x, gamma, beta, act, eps=1e-5):
    f = ln_fwd(x, gamma, beta, act, eps)
    xhat, rstd = f["xhat"], f["rstd"][:, None]
    g = gamma.double()
    dz = dy.double() * act_d(f["z"], act)
    gd = dz * g
    dx = rstd * (gd - gd.mean(1, keepdim=True) - xhat * (gd * xhat).mean(1, keepdim=True))
    return dict(dx=dx, dgamma=(dz * xhat).sum(0), dbeta=dz.sum(0))


def kink_mask(z, act):
    """Elements whose ReLU pre-activation lies within KINK of 0 (none for the smooth activations):
    the caller zeroes dy there, in the reference and in the kernel run alike."""
    if act != "relu":
        return torch.zeros_like(z, dtype=torch.bool)
    return z.abs() < KINK


def rel(a, b):
    """rel-L2 of a against the reference b (double); an all-zero reference compares absolutely."""
    a, b = a.double().reshape(-1), b.double().reshape(-1).to(a.device)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item() if b.norm() > 0 else (a - b).norm().item()
