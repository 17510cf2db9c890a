#!/usr/bin/env python3
"""Time the fused statistics pass (StatsAccumulator.update_windows, csrc/stats.hip) at the bench
shape — B windows, J=11 Q=4 T=16 N=4096 front-end, trim 30, all five fields — net of
FrontEnd.raw, beside the same statistics from a torch-op restatement of the reference's
per-channel fp64 loop on the device (what ref/hdf5_dataset/calculate_dataset_stats.py:134-221
does with device='cuda': widen to fp64, then per channel mask, transform, mask, index, sum).

Method: device events around `iters` back-to-back calls ending in a synchronise, after a warm-up
of every variant; the variants alternate within each round and the median over rounds is
reported.  "net" is (raw + statistics) - (raw alone); "direct" times the statistics calls
alone on buffers a previous raw() left.  Prints one JSON line.

Usage: python tools/stats_bench.py [--batch 256] [--rounds 7] [--iters 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-teb_amd"))

from vaeteb import synthetic  # noqa: E402
from vaeteb.frontend import FrontEnd, FrontEndPlan  # noqa: E402
from vaeteb.stats import SINGLE_FIELDS, StatsAccumulator, channel_kinds  # noqa: E402


class TorchLoopStats:
    """The reference's update rule restated with torch ops (fp64, one channel at a time)."""

    def __init__(self, fields, device):
        self.state = {f: (torch.zeros(C, dtype=torch.int64, device=device),
                          torch.zeros(C, dtype=torch.float64, device=device),
                          torch.zeros(C, dtype=torch.float64, device=device)) for f, C in fields.items()}

    def update(self, field, data, log_eps=1e-6):
        cnt, s, q = self.state[field]
        d = data.to(torch.float64)
        if field in SINGLE_FIELDS:
            v = d.flatten()
            v = v[torch.isfinite(v)]
            cnt[0] += v.numel()
            s[0] += torch.sum(v)
            q[0] += torch.sum(v ** 2)
            return
        kinds = channel_kinds(field, d.shape[1])
        zero = torch.tensor(0.0, device=d.device, dtype=torch.float64)
        for c in range(d.shape[1]):
            v = d[:, c, :].flatten()
            m = torch.isfinite(v)
            if kinds[c] == 1:
                v = torch.log(torch.maximum(v, zero) + log_eps)
                m = m & torch.isfinite(v)
            elif kinds[c] == 2:
                v = torch.asinh(v)
                m = m & torch.isfinite(v)
            v = v[m]
            if v.numel() == 0:
                continue
            cnt[c] += v.numel()
            s[c] += torch.sum(v)
            q[c] += torch.sum(v ** 2)

    def update_windows(self, fe, x):
        self.update_features(fe, fe.raw(x), x)

    def update_features(self, fe, r, x):
        t = fe.trim
        sl = slice(t, r["fhr_st"].shape[2] - t)
        self.update("fhr_st", r["fhr_st"][:, :, sl])
        self.update("fhr_ph", r["pairs"][:, :fe.C_ph, sl])
        self.update("fhr_up_ph", r["pairs"][:, fe.C_ph:, sl])
        cut = t * fe.plan.step
        self.update("fhr", x[:, 0, cut:x.shape[2] - cut])
        self.update("up", x[:, 1, cut:x.shape[2] - cut])


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-iters", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stats_bench needs the GPU: a CPU run cannot give a time")
    fe = FrontEnd(FrontEndPlan(11, 4, 16, 4096), stats=None, trim=30)
    x = torch.from_numpy(synthetic.batch(0, a.batch, 4096)).cuda()
    acc = StatsAccumulator.for_frontend(fe)
    loop = TorchLoopStats({"fhr": 1, "up": 1, "fhr_st": fe.C_st, "fhr_ph": fe.C_ph, "fhr_up_ph": fe.C_x}, "cuda")

    # results first: one update each from zero, compared
    acc.update_windows(fe, x)
    loop.update_windows(fe, x)
    torch.cuda.synchronize()
    worst = 0.0
    host = acc.host_state()
    for f, (cnt, s, q) in loop.state.items():
        assert np.array_equal(host[f][0], cnt.cpu().numpy()), f
        for got, ref in ((host[f][1], s), (host[f][2], q)):
            ref = ref.cpu().numpy()
            worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))))

    r = fe.raw(x)
    variants = {
        "raw": (lambda: fe.raw(x), a.iters),
        "raw+fused": (lambda: acc.update_windows(fe, x), a.iters),
        "fused_direct": (lambda: _fused_direct(acc, fe, r, x), a.iters),
        "raw+torch_loop": (lambda: loop.update_windows(fe, x), a.loop_iters),
        "torch_loop_direct": (lambda: loop.update_features(fe, r, x), a.loop_iters),
    }
    for fn, _ in variants.values():   # warm-up of every variant
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, it) in variants.items():
            ms[k].append(timed(fn, it))
    med = {k: statistics.median(v) for k, v in ms.items()}
    feat_bytes = 4 * a.batch * ((fe.C_st + fe.C_ph + fe.C_x) * fe.S_out + 2 * fe.N_out)
    print(json.dumps({
        "batch": a.batch, "rounds": a.rounds, "iters": a.iters, "loop_iters": a.loop_iters,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "fused_net_ms": round(med["raw+fused"] - med["raw"], 4),
        "torch_loop_net_ms": round(med["raw+torch_loop"] - med["raw"], 4),
        "bytes_read_by_the_pass": feat_bytes,
        "fused_direct_GBps": round(feat_bytes / med["fused_direct"] / 1e6, 1),
        "max_rel_diff_of_sums_fused_vs_torch_loop": worst,
    }))


def _fused_direct(acc, fe, r, x):
    t = fe.trim
    acc.update("fhr_st", r["fhr_st"], trim=t)
    acc.update("fhr_ph", r["pairs"][:, :fe.C_ph], in_C=r["pairs"].shape[1], trim=t)
    acc.update("fhr_up_ph", r["pairs"][:, fe.C_ph:], in_C=r["pairs"].shape[1], trim=t)
    for ch, f in enumerate(SINGLE_FIELDS):
        acc.update(f, x[:, ch], trim=t)


if __name__ == "__main__":
    main()
