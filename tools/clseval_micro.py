#!/usr/bin/env python3
"""Time the classifier evaluation of vaeteb.clseval on the device against the literal alternative, in
one process, the variants alternated, medians reported.

Recordings: tools/windows_micro.py's synthetic set (default 512 recordings of 40,960 samples: 19
windows of 4096 at half overlap each, the default QualityGate), labels alternating 0 / 1, the bench
front-end (J 11, Q 4, T 16, N 4096: 256 steps per window, the classifier's attention takes at most 256)
and a SeqVaeTebClassifier(sequence_length=256) with seeded weights.  T = 401 thresholds, strike 2,
n_boot = 1000.

  evaluate   model.evaluate_recordings end to end (host clock around synchronised calls)
  score      the scoring loop alone: frontend, encode, classifier, softmax per batch
  forward    the literal scoring: per batch model(...) (with the decoder) and .cpu() of the probabilities
  alarm      vt_cls_alarm_sweep (device events)        | numpy: per threshold, per recording
  confusion  vt_cls_confusion, G epoch groups          | numpy: per threshold, per group boolean masks
  auc        torch.sort + vt_cls_auc_ranks, 1 + n_boot | numpy: a resampling loop, each replicate sorted
             replicates                                  and ranked on its own

The numpy sides are checked against the device results (exact for the integers, 1e-12 for the AUCs).
Reported, not gated.  Usage:  python tools/clseval_micro.py [--recordings 512] [--reps 3]
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
from vaeteb import clseval as ce  # noqa: E402
from vaeteb.classifier import SeqVaeTebClassifier  # noqa: E402
from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats  # noqa: E402
from vaeteb.windows import QualityGate, RecordingWindows  # noqa: E402
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


def alarm_numpy(p, base, thr, strike, mode):
    """The sweep as one would write it in numpy: per threshold, per recording (no gap rule)."""
    R, T = len(base) - 1, len(thr)
    first = np.full((R, T), -1, np.int32)
    for t in range(T):
        with np.errstate(invalid="ignore"):
            fire = p > thr[t]
        for r in range(R):
            f = fire[base[r]:base[r + 1]]
            if mode == "cumulative":
                hit = np.cumsum(f) >= strike
            else:
                c = np.cumsum(np.concatenate([[0], f]))
                hit = np.zeros(len(f), bool)
                if len(f) >= strike:
                    hit[strike - 1:] = (c[strike:] - c[:-strike]) == strike
            if hit.any():
                first[r, t] = int(np.argmax(hit))
    return first


def confusion_numpy(p, lab, thr, grp, G):
    out = np.zeros((G, len(thr), 4), np.int32)
    pos = lab != 0
    for t in range(len(thr)):
        with np.errstate(invalid="ignore"):
            pred = p > thr[t]
        for g in range(G):
            m = grp == g
            out[g, t] = [(m & pred & pos).sum(), (m & pred & ~pos).sum(), (m & ~pred & ~pos).sum(),
                         (m & ~pred & pos).sum()]
    return out


def auc_numpy(p, lab):
    """Tie-aware AUC of one sample by average ranks (the Mann-Whitney form)."""
    ok = ~np.isnan(p)
    p, lab = p[ok], lab[ok]
    n1 = int((lab != 0).sum())
    n0 = len(lab) - n1
    if n1 == 0 or n0 == 0:
        return float("nan")
    order = np.argsort(p, kind="stable")
    ps = p[order]
    head = np.concatenate([[True], ps[1:] != ps[:-1]])
    gid = np.cumsum(head) - 1
    start = np.nonzero(head)[0]
    size = np.diff(np.concatenate([start, [len(ps)]]))
    rank = (start + (size + 1) / 2.0)[gid]                            # average 1-based rank of each tie group
    r1 = rank[lab[order] != 0].sum()
    return (r1 - n1 * (n1 + 1) / 2.0) / (n1 * n0)


def boot_numpy(p, lab, rec, base, R, n_boot, seed):
    """A resampling loop over recordings with the evaluation's multiplicities."""
    mult = ce.multiplicities(R, n_boot, seed)
    out = np.empty(n_boot)
    idx = [np.arange(base[r], base[r + 1]) for r in range(R)]
    for b in range(n_boot):
        take = np.concatenate([np.tile(idx[r], mult[b, r]) for r in np.nonzero(mult[b])[0]] + [np.zeros(0, np.int64)])
        take = take.astype(np.int64)
        out[b] = auc_numpy(p[take], lab[take])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=512)
    ap.add_argument("--length", type=int, default=40960, help="samples per recording (40960 = 19 windows)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--groups", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    N = 4096
    fe = FrontEnd(FrontEndPlan(11, 4, 16, N, device="cuda"), load_stats(11, 4, 16, 4096))
    torch.manual_seed(0)
    m = SeqVaeTebClassifier(sequence_length=fe.S_out, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                            cross_phase_channels=fe.C_x).cuda()
    recs = recordings(a.recordings, a.length, N)
    for i, r in enumerate(recs):
        r.bg_label = bool(i % 2)
    rw = RecordingWindows(recs, N=N, overlap=0.5, gate=QualityGate(), batch_size=a.batch)
    R = len(recs)
    edges = np.linspace(0.0, float(a.length), a.groups + 1)
    kw = dict(strike=2, mode="consecutive", break_on_gap=False, epoch_bins=edges, n_boot=a.n_boot, seed=0)

    ev = m.evaluate_recordings(fe, rw, **kw)                          # warm-up; its p feeds the statistics
    torch.cuda.synchronize()
    W, S, L = len(ev.windows), fe.S_out, m.latent_dim_z
    rec, epoch = ev.windows.rec, ev.windows.epoch
    base = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=R))]).astype(np.int64)
    pd = ev.windows.p
    p = pd.cpu().numpy()
    # the seeded classifier gives nearly equal probabilities; spread them so that the sweep has work to do
    rng = np.random.Generator(np.random.PCG64(1))
    p = np.clip(p + 0.25 * rng.standard_normal(W).astype(np.float32), 0, 1).astype(np.float32)
    p = (np.round(p * 1024) / 1024).astype(np.float32)                # ties, as a saturating softmax gives
    pd = torch.from_numpy(p).cuda()
    lab = ev.windows.label
    grp = (np.digitize(epoch, edges) - 1).astype(np.int32)
    thr = ce.default_thresholds()
    lab_d, grp_d = torch.from_numpy(lab).cuda(), torch.from_numpy(grp).cuda()
    rec32 = rec.astype(np.int32)
    mult = np.concatenate([np.ones((1, R), np.int32), ce.multiplicities(R, a.n_boot, 0)])
    mult_d, rec_d = torch.from_numpy(mult).cuda(), torch.from_numpy(rec32).cuda()
    first_o = torch.empty((R, len(thr)), dtype=torch.int32, device="cuda")
    counts_o = torch.empty((a.groups, len(thr), 4), dtype=torch.int32, device="cuda")
    ranks_o = torch.empty((1 + a.n_boot, 1, 4), dtype=torch.int64, device="cuda")

    def score():
        for b in rw:
            f = fe(b.x)
            _, _, mu, _ = m.vae_model.encode(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"])
            torch.softmax(m.classifier(mu.contiguous()), dim=-1)

    def forward():
        out = []
        for b in rw:
            f = fe(b.x)
            o = m(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], eps=torch.zeros(b.x.shape[0], S, L, device="cuda"))
            out.append(o["probabilities"].cpu())
        return out

    k_alarm = lambda: ce.alarm_sweep(pd, base, thr, 2, "consecutive", out=first_o)
    k_conf = lambda: ce.confusion(pd, lab_d, thr, grp_d, a.groups, out=counts_o)
    k_auc = lambda: ce.auc_ranks(pd, lab_d, rec=rec_d, mult=mult_d, out=ranks_o)
    n_alarm = lambda: alarm_numpy(p, base, thr, 2, "consecutive")
    n_conf = lambda: confusion_numpy(p, lab, thr, grp, a.groups)
    n_boot = lambda: boot_numpy(p, lab, rec, base, R, a.n_boot, 0)

    m.eval()
    with torch.no_grad():
        for fn in (score, forward, k_alarm, k_conf, k_auc):           # warm-up of everything timed below
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in ("evaluate", "score", "forward", "alarm", "alarm_np", "conf", "conf_np", "auc", "auc_np")}
        for _ in range(a.reps):                                       # alternated
            t["evaluate"].append(wall(lambda: m.evaluate_recordings(fe, rw, **kw))[0])
            t["score"].append(wall(score)[0])
            t["forward"].append(wall(forward)[0])
            t["alarm"].append(events(k_alarm, a.kernel_reps))
            ta, first_n = wall(n_alarm)
            t["alarm_np"].append(ta)
            t["conf"].append(events(k_conf, a.kernel_reps))
            tc, counts_n = wall(n_conf)
            t["conf_np"].append(tc)
            t["auc"].append(events(k_auc, a.kernel_reps))
            tb, boot_n = wall(n_boot)
            t["auc_np"].append(tb)
    ranks = k_auc().cpu().numpy()
    auc_d = ce.auc_from_ranks(ranks[:, 0])
    agree = dict(alarm=bool(np.array_equal(k_alarm().cpu().numpy(), first_n)),
                 confusion=bool(np.array_equal(k_conf().cpu().numpy(), counts_n)),
                 auc=bool(abs(auc_d[0] - auc_numpy(p, lab)) <= 1e-12),
                 boot=bool(np.allclose(auc_d[1:], boot_n, rtol=0, atol=1e-12, equal_nan=True)))
    med = lambda k: float(np.median(t[k]))
    print(json.dumps({
        "recordings": R, "length": a.length, "window": N, "windows": rw.n_windows, "kept": W, "batch": a.batch,
        "thresholds": len(thr), "groups": a.groups, "n_boot": a.n_boot, "strike": 2,
        "evaluate_ms": round(med("evaluate"), 1), "score_ms": round(med("score"), 1),
        "forward_cpu_ms": round(med("forward"), 1), "forward_over_score": round(med("forward") / med("score"), 2),
        "statistics_share_of_evaluate": round(max(med("evaluate") - med("score"), 0.0) / med("evaluate"), 4),
        "alarm_ms": round(med("alarm"), 4), "alarm_numpy_ms": round(med("alarm_np"), 1),
        "alarm_numpy_over_kernel": round(med("alarm_np") / med("alarm"), 0),
        "confusion_ms": round(med("conf"), 4), "confusion_numpy_ms": round(med("conf_np"), 1),
        "confusion_numpy_over_kernel": round(med("conf_np") / med("conf"), 0),
        "auc_boot_ms": round(med("auc"), 4), "auc_boot_numpy_ms": round(med("auc_np"), 1),
        "auc_boot_numpy_over_kernel": round(med("auc_np") / med("auc"), 0), "agree": agree}))


if __name__ == "__main__":
    main()
