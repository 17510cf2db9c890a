#!/usr/bin/env python3
"""Time the whole-recording scorer of vaeteb.timeline on the device against the literal alternative,
in one process, the variants alternated.

Recordings: tools/windows_micro.py's set (64 synthetic recordings of 57,600 samples, 5760-sample
windows at half overlap, the default QualityGate), the product front-end (J 11, Q 4, T 16, trim 30:
300 steps / 4800 samples per window) and a SeqVaeTeb(sequence_length=300) with seeded weights.

  scorer     RecordingScorer end to end (host clock around synchronised calls)
  stitch     its timeline launches alone on the kept per-window kl / mu_pr: the accumulate calls in the
             scorer's batches, the finish passes and the metrics launch (device events, warmed up),
             with the bytes they move and the rate
  loop       per window, batch 1: frontend, model.reconstruction_metrics(..., elementwise=True,
             return_mu=True), .cpu(), numpy overlap-average — timed on the first `--loop-windows` kept
             windows and reported per window (and extrapolated to all of them)
  overlap    vaeteb.timeline.overlap_mean against SeqVaeTeb.get_predictions at B 256, N 300 rows of
             `--row` samples, stride 16, new_C 4800 (the (256, 300, 4800) canvas), device events

Reported, not gated.  Usage:  python tools/timeline_micro.py [--recordings 64] [--length 57600]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "vae-teb_amd"))
sys.path.insert(0, HERE)
from vaeteb import _lib  # noqa: E402
from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats  # noqa: E402
from vaeteb.model import SeqVaeTeb  # noqa: E402
from vaeteb.timeline import RecordingScorer, TimelineState, overlap_mean  # noqa: E402
from vaeteb.windows import QualityGate, RecordingWindows, gather  # noqa: E402
from windows_micro import recordings  # noqa: E402


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--length", type=int, default=57600, help="samples per recording (57600 = 4 h at 4 Hz)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--loop-windows", type=int, default=64)
    ap.add_argument("--row", type=int, default=64, help="row width C of the overlap_mean comparison")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    N = 5760
    fe = FrontEnd(FrontEndPlan(11, 4, 16, N, device="cuda"), load_stats(11, 4, 16, 4096), trim=30)
    torch.manual_seed(0)
    m = SeqVaeTeb(sequence_length=fe.S_out, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                  cross_phase_channels=fe.C_x).cuda()
    rw = RecordingWindows(recordings(a.recordings, a.length, N), N=N, overlap=0.5, gate=QualityGate(),
                          batch_size=a.batch)
    scorer = RecordingScorer(m, fe)
    S, n, L = fe.S_out, fe.N_out, m.latent_dim_z

    res = scorer(rw, keep_windows=True)                    # warm-up; its windows feed the kernel timing
    torch.cuda.synchronize()
    W = len(res.windows)
    lay = res.layout
    so, no = lay.window_offsets(res.windows.rec, res.windows.start, fe)
    so_d, no_d = torch.from_numpy(so).cuda(), torch.from_numpy(no).cuda()
    y = torch.randn(lay.n_samples, device="cuda")
    base = torch.from_numpy(lay.sample_base).cuda()
    met = torch.empty((len(lay.lengths), 5), device="cuda")
    kl, mu = res.windows.kl, res.windows.mu_pr

    def stitch_only():
        te_s, rc_s = TimelineState(lay.n_steps), TimelineState(lay.n_samples)
        for w0 in range(0, W, a.batch):
            te_s.accumulate(kl[w0:w0 + a.batch], so_d[w0:w0 + a.batch])
            rc_s.accumulate(mu[w0:w0 + a.batch], no_d[w0:w0 + a.batch])
        te_s.finish()
        recon, count = rc_s.finish()
        rc_s.finish(scale=res.denorm[0], shift=res.denorm[1])
        _lib.call("vt_timeline_metrics", _lib.ptr(y), _lib.ptr(recon), _lib.ptr(count), _lib.ptr(base), met.shape[0],
                  _lib.ptr(met), _lib.stream())

    # bytes: the window values once; 12 B read + 12 B written per position a call touches (and the 12 B
    # zero fill of each state); finish 12 B + 4 B per position; metrics two passes of 12 B per sample
    touched = 0
    for off, width, total in ((so, S, lay.n_steps), (no, n, lay.n_samples)):
        for w0 in range(0, W, a.batch):
            mark = np.zeros(total + 1, np.int32)
            np.add.at(mark, off[w0:w0 + a.batch], 1)
            np.add.at(mark, off[w0:w0 + a.batch] + width, -1)
            touched += int((np.cumsum(mark)[:-1] > 0).sum())
    moved = 4 * (kl.numel() + mu.numel()) + 24 * touched + 12 * (lay.n_steps + lay.n_samples) \
        + 16 * (lay.n_steps + 2 * lay.n_samples) + 24 * int((torch.cat(res.coverage) > 0).sum())

    hw = min(a.loop_windows, W)
    eps1 = torch.zeros(1, 1, S, L, device="cuda")

    def loop():
        te_t, te_c = np.zeros(lay.n_steps), np.zeros(lay.n_steps)
        rc_t, rc_c = np.zeros(lay.n_samples), np.zeros(lay.n_samples)
        for i in range(hw):
            x = gather(rw.buffer, rw.row_off_host[rw.kept[i]], N).view(1, 2, N)
            f = fe(x)
            r = m.reconstruction_metrics(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], eps=eps1,
                                         elementwise=True, return_mu=True)
            k1, m1 = r.kl.cpu().numpy().reshape(S, L), r.mu_pr.cpu().numpy().reshape(n)
            te_t[so[i]:so[i] + S] += k1.mean(-1, dtype=np.float64)
            te_c[so[i]:so[i] + S] += 1
            rc_t[no[i]:no[i] + n] += m1
            rc_c[no[i]:no[i] + n] += 1
        with np.errstate(invalid="ignore"):
            return te_t / te_c, te_c, rc_t / rc_c

    B, rows = 256, 300
    xo = torch.randn(B, rows, a.row, device="cuda")
    om = lambda: overlap_mean(xo, 16, 4800)
    gp = lambda: SeqVaeTeb.get_predictions(xo, 16, 4800)[1]

    for fn in (stitch_only, loop, om, gp):                 # warm-up of everything timed below
        fn()
    torch.cuda.synchronize()
    t_scorer, t_stitch, t_loop, t_om, t_gp = [], [], [], [], []
    for _ in range(a.reps):                                # alternated
        t_scorer.append(wall(lambda: scorer(rw))[0])
        t_stitch.append(events(stitch_only, a.kernel_reps))
        t_loop.append(wall(loop)[0])
        t_om.append(events(om, a.kernel_reps))
        t_gp.append(events(gp, max(a.kernel_reps // 4, 1)))
    ok = torch.equal(torch.isnan(om()), torch.isnan(gp())) and \
        torch.allclose(om(), gp(), rtol=1e-5, atol=1e-6, equal_nan=True)
    lt, lc, _ = loop()
    te0 = res.te_packed.cpu().numpy()
    cov = (lc > 0) & (lc == torch.cat(res.coverage_steps).cpu().numpy())     # steps the timed windows cover alone
    loop_agrees = bool(np.allclose(te0[cov], lt[cov], rtol=1e-5, atol=1e-7))
    med = lambda v: float(np.median(v))
    stitch_ms = med(t_stitch)
    print(json.dumps({
        "recordings": a.recordings, "length": a.length, "window": N, "windows": rw.n_windows, "kept": W,
        "batch": a.batch, "steps_per_window": S, "samples_per_window": n,
        "scorer_ms": round(med(t_scorer), 2), "scorer_ms_per_window": round(med(t_scorer) / max(W, 1), 4),
        "stitch_metrics_ms": round(stitch_ms, 4), "stitch_metrics_MB": round(moved / 1e6, 1),
        "stitch_metrics_GBps": round(moved / (stitch_ms * 1e-3) / 1e9, 1),
        "stitch_share_of_scorer": round(stitch_ms / med(t_scorer), 4),
        "loop_windows_timed": hw, "loop_ms_per_window": round(med(t_loop) / max(hw, 1), 3),
        "loop_ms_all_windows_extrapolated": round(med(t_loop) / max(hw, 1) * W, 1),
        "loop_over_scorer": round(med(t_loop) / max(hw, 1) * W / med(t_scorer), 2),
        "loop_te_agrees": loop_agrees,
        "overlap_shape": [B, rows, a.row], "overlap_canvas": [B, rows, 4800],
        "overlap_mean_ms": round(med(t_om), 4), "get_predictions_ms": round(med(t_gp), 3),
        "get_predictions_over_overlap_mean": round(med(t_gp) / med(t_om), 1), "overlap_agrees": bool(ok)}))


if __name__ == "__main__":
    main()
