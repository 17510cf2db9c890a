#!/usr/bin/env python3
"""Generate the Scattering1D gradient fixtures from the REFERENCE kymatio
(build container only, CPU; in the manner of tools/gen_golden.py).

For each configuration (J, Q, T, N, order, B) the reference's torch frontend
(ref/kymatio/kymatio/scattering1d/frontend/torch_frontend.py) runs in fp64 and
in fp32 on the same input x and the gradient of sum(w * S(x)) with a random
cotangent w is taken by torch autograd:

  tests/golden/scat_grad_<cfg>.npz : x (fp32), w (fp32), S64, S32, g64, g32
  config d also: x0, gq64, gq32 -- the gradient of 0.5 * ||S(x) - S(x0)||^2

T is always passed (the reference's torch frontend crashes on T=None).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_scat_grad.py [--only CFG]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(REF, "kymatio"))

torch.set_num_threads(8)

# cfg -> (J, Q, T, N, order, B); each the smallest that reaches its case (tests/test_gpu_scattering_grad.py)
CONFIGS = {
    "a": (2, 1, 4, 64, 2, 3),        # one level, n_pad 128; x[0] = 0: the zero-modulus subgradient
    "b": (3, 1, 8, 100, 1, 3),       # non-power-of-two N, first order (the fused forward's case)
    "c": (4, 4, 16, 256, 2, 3),      # level rows 512 / 256 / 128 / 64
    "d": (6, 16, 64, 512, 2, 2),     # kymatio's known-answer configuration
    "e": (4, 1, 16, 12000, 2, 2),    # n_pad 16384: rows 16384 (four-step), 8192, 4096
}


def _grad(sc, x, loss):
    x = x.clone().requires_grad_(True)
    S, _ = sc(x)
    loss(S).backward()
    return S.detach(), x.grad


def gen(cfg):
    from kymatio.torch import Scattering1D
    J, Q, T, N, order, B = CONFIGS[cfg]
    seed = 2000 + ord(cfg)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, N)).astype(np.float32)
    if cfg == "a":
        x[0] = 0
    t = time.time()
    sc32 = Scattering1D(J=J, shape=N, Q=Q, max_order=order, T=T)
    sc64 = Scattering1D(J=J, shape=N, Q=Q, max_order=order, T=T).double()
    xt = torch.from_numpy(x)
    with torch.no_grad():
        shape = sc32(xt)[0].shape
    w = rng.standard_normal(tuple(shape)).astype(np.float32)
    wt = torch.from_numpy(w)
    S64, g64 = _grad(sc64, xt.double(), lambda S: (wt.double() * S).sum())
    S32, g32 = _grad(sc32, xt, lambda S: (wt * S).sum())
    d = dict(x=x, w=w, S64=S64.numpy(), S32=S32.numpy(), g64=g64.numpy(), g32=g32.numpy())
    if cfg == "d":
        x0 = rng.standard_normal((B, N)).astype(np.float32)
        x0t = torch.from_numpy(x0)
        with torch.no_grad():
            T64, T32 = sc64(x0t.double())[0], sc32(x0t)[0]
        d["x0"] = x0
        d["gq64"] = _grad(sc64, xt.double(), lambda S: 0.5 * ((S - T64) ** 2).sum())[1].numpy()
        d["gq32"] = _grad(sc32, xt, lambda S: 0.5 * ((S - T32) ** 2).sum())[1].numpy()
    path = os.path.join(OUT, f"scat_grad_{cfg}.npz")
    np.savez_compressed(path, **d)
    r = np.sqrt(((d["g32"] - d["g64"]) ** 2).sum(-1) / (d["g64"] ** 2).sum(-1))
    print(f"{cfg}: S {tuple(shape)} fp32-vs-fp64 gradient rel-L2 max {r.max():.2e} "
          f"{time.time() - t:.2f}s -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(CONFIGS))
    a = ap.parse_args()
    for c in ([a.only] if a.only else sorted(CONFIGS)):
        gen(c)
