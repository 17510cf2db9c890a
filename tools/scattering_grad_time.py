#!/usr/bin/env python3
"""Time Scattering1D forward and forward + backward on the GPU.

Three variants per shape, alternated in one process (so clock and thermal drift
hit them alike), each timed with device events over windows of at least
--window seconds after a warm-up:

  forward          sc(x) under no_grad, as routed (fused kernels or the cascade)
  fwd_bwd_cascade  sc(x) with x.requires_grad on the level-grouped cascade, then
                   S.backward(w)            (csrc/scatter_bwd.hip)
  fwd_bwd_generic  the same through the per-filter generic core over the
                   differentiable torch_hip plugin ops (sc.cascade = False)

Prints one JSON line.  Usage:  python tools/scattering_grad_time.py [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-teb_amd"))

SHAPES = {   # name -> (J, Q, T, N, order, B)
    "config5_j8q12t256_n16384_o2_b64": (8, 12, 256, 16384, 2, 64),
    "j11q4t16_n4096_o1_b256": (11, 4, 16, 4096, 1, 256),
}


def window(fn, seconds):
    """ms per call of fn over one window of at least `seconds` (device events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total = 0, 0.0
    batch = 1
    while total < seconds * 1e3:
        t0.record()
        for _ in range(batch):
            fn()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1)
        calls += batch
        batch = min(2 * batch, 64)
    return total / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(SHAPES))
    a = ap.parse_args()
    from vaeteb.scattering import Scattering1D
    res = {"device": torch.cuda.get_device_name(0), "window_s": a.window, "rounds": a.rounds, "shapes": {}}
    for name, (J, Q, T, N, order, B) in SHAPES.items():
        if a.only and name != a.only:
            continue
        sc = Scattering1D(J=J, shape=N, Q=Q, max_order=order, T=T)
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(B, N, generator=gen).cuda()
        with torch.no_grad():
            S0 = sc(x)[0]
        w = torch.randn(S0.shape, generator=gen).cuda()
        xg = x.clone().requires_grad_(True)

        def forward():
            with torch.no_grad():
                sc.cascade = True
                sc(x)

        def fwd_bwd(cascade):
            def run():
                sc.cascade = cascade
                xg.grad = None
                sc(xg)[0].backward(w)
            return run

        variants = {"forward": forward, "fwd_bwd_cascade": fwd_bwd(True), "fwd_bwd_generic": fwd_bwd(False)}
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window(fn, a.window))
        r = {k + "_ms": round(statistics.median(v), 4) for k, v in ms.items()}
        r["forward_path"] = "fused" if sc._fused_ok() else "cascade"
        r["fwd_bwd_cascade_over_forward"] = round(r["fwd_bwd_cascade_ms"] / r["forward_ms"], 2)
        r["generic_over_cascade"] = round(r["fwd_bwd_generic_ms"] / r["fwd_bwd_cascade_ms"], 2)
        r["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        res["shapes"][name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
