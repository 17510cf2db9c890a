#!/usr/bin/env python3
"""Time the batched evaluation sweep (vaeteb.evaluate.GainSweep) against the literal loop over the
public API it replaces, which is the reference's structure (ref/model/graph_model.py:1832-1854): per
gain one forward on x_ph * g and one measure_transfer_entropy over the batch, then per sample a
.cpu() of the two rows, numpy variances for the VAF and an .item() of its transfer entropy — at B
recordings x the reference's five default gains, in the bench's precisions (conv / mlp / head bf16,
lstm 16-mixed), on seeded standard-normal fields.

A host clock around whole calls, each ending in a device synchronise (the loop's host work is part of
what it costs), every shape warmed first, the two variants alternated within each repeat (a window
is one loop call or --sweep-calls sweep calls, reported per call), median and min-max over the
repeats.  The largest differences of the two results are printed with the times.  One JSON line per
sequence length.

Usage:  python tools/eval_sweep_micro.py [--B 256] [--repeats 7] [--S 300 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-teb_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vaeteb.evaluate import DEFAULT_GAINS, GainSweep  # noqa: E402
from vaeteb.model import SeqVaeTeb  # noqa: E402


def loop(model, y_st, y_ph, x_ph, y_raw, gains):
    B = y_st.shape[0]
    te, vaf, vaf_u = (np.zeros((B, len(gains))) for _ in range(3))
    model.eval()
    with torch.no_grad():
        for k, g in enumerate(gains):
            x_scaled = x_ph * float(g)
            mu_pr = model(y_st, y_ph, x_scaled)["mu_pr"]
            kld_ps = model.measure_transfer_entropy(y_st, y_ph, x_scaled, reduce_mean=False).mean(dim=(1, 2))
            for i in range(B):
                gt, pr = y_raw[i].cpu().numpy(), mu_pr[i].cpu().numpy()
                var_gt = np.var(gt)
                v = 1.0 - np.var(gt - pr) / var_gt if var_gt > 1e-12 else 0.0
                vaf[i, k], vaf_u[i, k] = max(0.0, min(1.0, float(v))), float(v)
                te[i, k] = float(kld_ps[i].item())
    return te, vaf, vaf_u


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweep-calls", type=int, default=10, help="sweep calls per timed window (one loop call)")
    ap.add_argument("--S", type=int, nargs="*", default=[300, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_sweep_micro needs a GPU: nothing is measured without one")
    gains = DEFAULT_GAINS
    for S in a.S:
        torch.manual_seed(0)
        model = SeqVaeTeb(sequence_length=S, conv_precision="bf16", mlp_precision="bf16", head_precision="bf16",
                          lstm_precision="16-mixed").cuda()
        gen = torch.Generator().manual_seed(S)
        y_st, y_ph, x_ph, y_raw = (torch.randn(a.B, *s, generator=gen).cuda()
                                   for s in ((S, 43), (S, 44), (S, 130), (16 * S,)))
        sweep = GainSweep(model)
        for _ in range(2):                      # warm-up of both variants at the timed shapes
            torch.cuda.manual_seed(7)           # from one seed the sweep draws the loop's noise, row for row
            r = sweep(y_st, y_ph, x_ph, y_raw, gains)
            torch.cuda.manual_seed(7)
            te_l, vaf_l, vaf_u_l = loop(model, y_st, y_ph, x_ph, y_raw, gains)
        torch.cuda.synchronize()
        te_rel = float(np.abs(r.te.cpu().numpy() / te_l - 1).max())
        vaf_abs = float(np.abs(r.vaf.cpu().numpy() - vaf_l).max())
        # an untrained model reconstructs nothing (every VAF clamps to 0): the value before the clamp says more
        vaf_u_rel = float(np.abs((1 - r.vaf_unclamped.cpu().numpy()) / (1 - vaf_u_l) - 1).max())
        ts, tl = [], []
        for _ in range(a.repeats):              # alternated: drift hits both alike
            ts.append(timed(lambda: [sweep(y_st, y_ph, x_ph, y_raw, gains) for _ in range(a.sweep_calls)])[0]
                      / a.sweep_calls)
            tl.append(timed(lambda: loop(model, y_st, y_ph, x_ph, y_raw, gains))[0])
        ms, ml = statistics.median(ts), statistics.median(tl)
        print(json.dumps({"S": S, "B": a.B, "K": len(gains), "rows": a.B * len(gains),
                          "sweep_ms_median": round(ms, 3), "sweep_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                          "loop_ms_median": round(ml, 3), "loop_ms_min_max": [round(min(tl), 3), round(max(tl), 3)],
                          "loop_over_sweep": round(ml / ms, 2), "te_max_rel_diff": te_rel,
                          "vaf_max_abs_diff": vaf_abs, "one_minus_vaf_unclamped_max_rel_diff": vaf_u_rel,
                          "repeats": a.repeats}), flush=True)


if __name__ == "__main__":
    main()
