"""Shared by tests/test_timeline_cpu.py and tests/test_gpu_timeline.py: float64 numpy restatements of
the timeline kernels (csrc/timeline.hip).  The CPU test pins them to hand cases and to
SeqVaeTeb.get_predictions; the GPU tests then use them as the expected values.

Bound of the overlap-average (derived, not tuned).  With m windows covering a position, weights w_j
and window values v_j, the kernel rounds v_j once (the inner mean, formed in double), forms m float32
products w_j v_j, adds them with m - 1 float32 sums and divides once; the weights and their sum are
small integers, exact in float32.  Each rounding moves the result by at most 2^-24 relative to the
magnitudes involved, all of which are bounded by sum_j w_j |v_j|, so with one spare

    |out - ref64| <= (m + 3) * 2^-24 * (sum_j w_j |v_j|) / (sum_j w_j).
"""
import numpy as np

U = 2.0 ** -24
DB = 10.0 / np.log(10.0)


def taper_weights(n):
    i = np.arange(n)
    return np.minimum(i + 1, n - i).astype(np.float64)


def stitch_np(vals, dst_off, lengths, total, blend="mean"):
    """vals (W, n) or (W, n, inner) float32; -> (out64 (total,) with NaN where uncovered, count int32,
    bound (total,): the per-position error allowed to the float32 kernel, 0 where uncovered).
    Windows are added in index order whatever dst_off holds (the kernel requires it ascending)."""
    vals = np.asarray(vals, np.float32)
    v = vals.astype(np.float64)
    if v.ndim == 3:
        v = v.mean(-1)
    W, n = v.shape
    wt = taper_weights(n) if blend == "taper" else np.ones(n)
    num, den, mag = np.zeros(total), np.zeros(total), np.zeros(total)
    count = np.zeros(total, np.int32)
    for j in range(W):
        ln = n if lengths is None else int(lengths[j])
        o = int(dst_off[j])
        num[o:o + ln] += wt[:ln] * v[j, :ln]
        mag[o:o + ln] += wt[:ln] * np.abs(v[j, :ln])
        den[o:o + ln] += wt[:ln]
        count[o:o + ln] += 1
    cov = count > 0
    out = np.full(total, np.nan)
    out[cov] = num[cov] / den[cov]
    bound = np.zeros(total)
    bound[cov] = (count[cov] + 3) * U * mag[cov] / den[cov]
    return out, count, bound


def overlap_mean_np(x, stride, new_C):
    """The placement of SeqVaeTeb.get_predictions (ref/model/vae_teb_model.py:1228-1246) through
    stitch_np: x (B, N, C) -> (out64 (B, new_C), count, bound)."""
    x = np.asarray(x, np.float32)
    B, N, C = x.shape
    rows, off, ln = [], [], []
    for b in range(B):
        for i in range(N):
            if i * stride >= new_C:
                break
            rows.append(x[b, i])
            off.append(b * new_C + i * stride)
            ln.append(min(max(new_C - i * stride, 0), C))
    if not rows:
        return np.full((B, new_C), np.nan), np.zeros((B, new_C), np.int32), np.zeros((B, new_C))
    out, count, bound = stitch_np(np.stack(rows), off, ln, B * new_C)
    return out.reshape(B, new_C), count.reshape(B, new_C), bound.reshape(B, new_C)


def metrics64(y, pr):
    """The metric definitions of ref/model/graph_model.py:1619-1645 in float64 on float32 1-D rows, the
    residual formed in float32 (the definitions tests/test_gpu_eval.py holds vt_recon_metrics_rows
    to): (vaf, mse, snr_db, vaf_unclamped)."""
    y, pr = np.asarray(y, np.float32), np.asarray(pr, np.float32)
    res = (y - pr).astype(np.float64)
    y64 = y.astype(np.float64)
    var_y, var_r = y64.var(), res.var()
    mse, sig = (res ** 2).mean(), (y64 ** 2).mean()
    vu = 1.0 - var_r / var_y if var_y > 1e-12 else 0.0
    snr = DB * np.log(sig / mse) if mse > 1e-12 else 100.0
    return float(np.clip(vu, 0.0, 1.0)), float(mse), float(snr), float(vu)


def masked_metrics_np(y, recon, count, base):
    """(R, 5) float64: metrics64 over the positions of [base[r], base[r+1]) with count > 0, and the
    covered fraction; NaN x 4 and 0 where none is covered."""
    R = len(base) - 1
    out = np.full((R, 5), np.nan)
    for r in range(R):
        a, b = int(base[r]), int(base[r + 1])
        cov = np.asarray(count[a:b]) > 0
        out[r, 4] = cov.mean() if b > a else 0.0
        if cov.any():
            out[r, :4] = metrics64(np.asarray(y[a:b])[cov], np.asarray(recon[a:b])[cov])
        else:
            out[r, 4] = 0.0
    return out
