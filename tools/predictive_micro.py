#!/usr/bin/env python3
"""Time the K-draw predictive distribution (vaeteb.predictive.Predictive) against the literal
alternative it replaces: K eval-mode forwards over the batch, then torch.stack, logsumexp,
special.ndtr and histc on the (B, K, n) tensors on the device (no host work: the alternative is given
every advantage short of a kernel of its own) — at B recordings x K draws, in the bench's precisions
(conv / mlp / head bf16, lstm 16-mixed), on seeded standard-normal fields with one explicit eps for
both variants.

A host clock around whole calls, each ending in a device synchronise, every shape warmed first, the
two variants alternated within each repeat, median and min-max over the repeats.  The largest
differences of the two results are printed with the times.  The mixture kernel alone
(vt_pred_mixture_rows on the decoder outputs of the last call) is timed with device events over
--kernel-calls launches per repeat and reported in ms and in GB/s of its compulsory
2 * B * K * n * 4 bytes.  One JSON line per sequence length.

Usage:  python tools/predictive_micro.py [--B 256] [--K 16] [--repeats 7] [--S 300]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-teb_amd"))

import torch  # noqa: E402

from vaeteb import _lib  # noqa: E402
from vaeteb.model import SeqVaeTeb  # noqa: E402
from vaeteb.predictive import DEFAULT_LEVELS, Predictive  # noqa: E402


def loop(model, y_st, y_ph, x_ph, y_raw, eps, bins=20, levels=DEFAULT_LEVELS):
    """The definitions of vaeteb/predictive.py in ATen on (B, K, n) tensors."""
    K = eps.shape[1]
    model.eval()
    with torch.no_grad():
        fws = [model(y_st, y_ph, x_ph, eps=eps[:, k].contiguous()) for k in range(K)]
        mu = torch.stack([fw["mu_pr"] for fw in fws], 1)
        lv = torch.stack([fw["logvar_pr"] for fw in fws], 1)
        z = torch.stack([fw["z"] for fw in fws], 1)
        fw = fws[0]
        d = y_raw[:, None] - mu
        ell = -0.5 * (math.log(2 * math.pi) + lv + d * d * torch.exp(-lv))
        mean = mu.mean(1)
        var_a, var_e = lv.exp().mean(1), mu.var(1, unbiased=False)
        logdens = torch.logsumexp(ell, 1) - math.log(K)
        pit = torch.special.ndtr(d * torch.exp(-0.5 * lv)).mean(1)
        ll = ell.sum(-1)
        logw = 0.5 * (fw["logvar_post"][:, None] - fw["logvar_prior"][:, None] + eps ** 2
                      - (z - fw["mu_prior"][:, None]) ** 2 * torch.exp(-fw["logvar_prior"])[:, None]).sum((-2, -1))
        v = var_a + var_e
        hist = torch.stack([torch.histc(p, bins=bins, min=0.0, max=1.0) for p in pit])
        cov = torch.stack([((pit - 0.5).abs() <= lev / 2).float().mean(-1) for lev in levels], -1)
        return dict(mean=mean, var_aleatoric=var_a, var_epistemic=var_e, nll_mixture=-logdens.mean(-1),
                    nll_moment=(0.5 * (math.log(2 * math.pi) + v.log() + (y_raw - mean) ** 2 / v)).mean(-1),
                    sharpness=v.sqrt().mean(-1), pit_hist=hist, coverage=cov, elbo=(ll + logw).mean(-1),
                    iwae=torch.logsumexp(ll + logw, 1) - math.log(K))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def mixture_alone(y_raw, mu, lv, calls):
    """ms per launch of vt_pred_mixture_rows on (B, K, n) decoder outputs, by device events."""
    B, K, n = mu.shape
    P, st = _lib.ptr, _lib.stream()
    lev = torch.tensor(DEFAULT_LEVELS, dtype=torch.float64, device=mu.device)
    tiles = -(-n // _lib.lib().fns["vt_pred_tile"]())
    ws = torch.empty(B * tiles * (K + 3 + 20 + len(DEFAULT_LEVELS)), dtype=torch.float64, device=mu.device)
    outs = [torch.empty(B, n, device=mu.device) for _ in range(3)]
    launch = lambda: _lib.call("vt_pred_mixture_rows", P(y_raw), P(mu), P(lv), B, K, n, 20, P(lev), len(DEFAULT_LEVELS),
                               P(outs[0]), P(outs[1]), P(outs[2]), None, None, P(ws), st)
    launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-calls", type=int, default=20, help="mixture-kernel launches per timed window")
    ap.add_argument("--S", type=int, nargs="*", default=[300])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predictive_micro needs a GPU: nothing is measured without one")
    for S in a.S:
        torch.manual_seed(0)
        model = SeqVaeTeb(sequence_length=S, conv_precision="bf16", mlp_precision="bf16", head_precision="bf16",
                          lstm_precision="16-mixed").cuda()
        gen = torch.Generator().manual_seed(S)
        y_st, y_ph, x_ph, y_raw = (torch.randn(a.B, *s, generator=gen).cuda()
                                   for s in ((S, 43), (S, 44), (S, 130), (16 * S,)))
        eps = torch.randn(a.B, a.K, S, 32, generator=gen).cuda()
        pred = Predictive(model)
        for _ in range(2):                      # warm-up of both variants at the timed shapes
            r = pred(y_st, y_ph, x_ph, y_raw, n_samples=a.K, eps=eps, return_samples=True)
            l = loop(model, y_st, y_ph, x_ph, y_raw, eps)
        torch.cuda.synchronize()
        diff = {}
        for k in ("var_aleatoric", "var_epistemic", "nll_mixture", "nll_moment", "sharpness", "elbo", "iwae",
                  "coverage"):
            g, w = getattr(r, k).double(), l[k].double()
            diff[k + "_max_rel_diff"] = float(((g - w).abs() / w.abs().clamp_min(1e-30)).max())
        # the mean changes sign: its largest difference against the largest mean of that recording
        g, w = r.mean.double(), l["mean"].double()
        diff["mean_max_diff_over_row_max"] = float(((g - w).abs().amax(-1) / w.abs().amax(-1)).max())
        diff["pit_hist_max_count_diff"] = int((r.pit_hist - l["pit_hist"].to(torch.int32)).abs().max())
        mu_s, lv_s = r.mu_pr, r.logvar_pr
        tp, tl, tk = [], [], []
        for _ in range(a.repeats):              # alternated: drift hits both alike
            tp.append(timed(lambda: pred(y_st, y_ph, x_ph, y_raw, n_samples=a.K, eps=eps))[0])
            tl.append(timed(lambda: loop(model, y_st, y_ph, x_ph, y_raw, eps))[0])
            tk.append(mixture_alone(y_raw, mu_s, lv_s, a.kernel_calls))
        mp, ml, mk = statistics.median(tp), statistics.median(tl), statistics.median(tk)
        gbytes = 2 * a.B * a.K * 16 * S * 4 / 1e9
        rnd = lambda v: round(v, 3)
        print(json.dumps({"S": S, "B": a.B, "K": a.K, "rows": a.B * a.K,
                          "predictive_ms_median": rnd(mp), "predictive_ms_min_max": [rnd(min(tp)), rnd(max(tp))],
                          "loop_ms_median": rnd(ml), "loop_ms_min_max": [rnd(min(tl)), rnd(max(tl))],
                          "loop_over_predictive": round(ml / mp, 2),
                          "mixture_kernel_ms_median": round(mk, 4),
                          "mixture_kernel_ms_min_max": [round(min(tk), 4), round(max(tk), 4)],
                          "mixture_kernel_GBps": round(gbytes / (mk * 1e-3), 1), **diff, "repeats": a.repeats}),
              flush=True)


if __name__ == "__main__":
    main()
