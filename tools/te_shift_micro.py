#!/usr/bin/env python3
"""Time the batched transfer-entropy-vs-shift sweep (vaeteb.te.ShiftSweep) against the literal
loop over the public API it replaces — FrontEnd.__call__ on the rolled window and
SeqVaeTeb.measure_transfer_entropy, one (recording, shift) at a time, which is how the reference
runs it (ref/model/graph_model.py:1320-1372) — at B recordings x the reference's 61 left shifts,
in the bench's precisions (conv / mlp / head bf16, lstm 16-mixed).

HIP events around whole calls (a call ends with its last kernel, the event waits for it), every
shape warmed first, the two variants alternated within each repeat (a window is one loop call or
--sweep-calls sweep calls, reported per call), median and min-max over the repeats.  The largest
relative difference of the two results is printed with the times.  One JSON line per geometry.

Usage:  python tools/te_shift_micro.py [--B 4] [--repeats 7] [--geometries 4096 5760]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-teb_amd"))

import torch  # noqa: E402

from vaeteb import synthetic  # noqa: E402
from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats  # noqa: E402
from vaeteb.model import SeqVaeTeb  # noqa: E402
from vaeteb.te import ShiftSweep, left_shifts  # noqa: E402


def loop(model, fe, x, shifts):
    out = []
    for b in range(x.shape[0]):
        for s in shifts:
            xr = x[b:b + 1].clone()
            xr[:, 1] = torch.roll(x[b:b + 1, 1], int(s), dims=-1)
            f = fe(xr)
            out.append(model.measure_transfer_entropy(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"]).mean())
    return torch.stack(out).view(x.shape[0], len(shifts))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweep-calls", type=int, default=10, help="sweep calls per timed window (one loop call)")
    ap.add_argument("--geometries", type=int, nargs="*", default=[4096, 5760])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("te_shift_micro needs a GPU: nothing is measured without one")
    shifts = left_shifts()
    for N in a.geometries:
        trim = 30 if N == 5760 else 0
        fe = FrontEnd(FrontEndPlan(11, 4, 16, N, device="cuda"), load_stats(11, 4, 16, 4096), trim=trim)
        torch.manual_seed(0)
        model = SeqVaeTeb(sequence_length=fe.S_out, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                          cross_phase_channels=fe.C_x, conv_precision="bf16", mlp_precision="bf16",
                          head_precision="bf16", lstm_precision="16-mixed").cuda()
        x = torch.from_numpy(synthetic.batch(0, a.B, N)).cuda()
        sweep = ShiftSweep(model, fe)
        for _ in range(2):                      # warm-up of both variants at the timed shapes
            te_s = sweep(x, shifts).te
            te_l = loop(model, fe, x, shifts)
        torch.cuda.synchronize()
        rel = ((te_s - te_l).abs() / te_l.abs()).max().item()
        ts, tl = [], []
        for _ in range(a.repeats):              # alternated: drift hits both alike
            ts.append(timed(lambda: [sweep(x, shifts) for _ in range(a.sweep_calls)])[0] / a.sweep_calls)
            tl.append(timed(lambda: loop(model, fe, x, shifts))[0])
        ms, ml = statistics.median(ts), statistics.median(tl)
        print(json.dumps({"N": N, "trim": trim, "B": a.B, "K": len(shifts), "rows": a.B * len(shifts),
                          "sweep_ms_median": round(ms, 3), "sweep_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                          "loop_ms_median": round(ml, 3), "loop_ms_min_max": [round(min(tl), 3), round(max(tl), 3)],
                          "loop_over_sweep": round(ml / ms, 2), "te_max_rel_diff": rel, "repeats": a.repeats}),
              flush=True)


if __name__ == "__main__":
    main()
