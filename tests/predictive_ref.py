"""Float64 numpy reference of the predictive-distribution definitions (vaeteb/predictive.py's module
docstring), and the term magnitudes the GPU tests scale their bounds by.  Inputs are
taken as given (float32 arrays are widened first), shapes y (B, n), mu / lv (B, K, n)."""
import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)
_erfc = np.frompyfunc(math.erfc, 1, 1)


def ndtr(t):
    """The standard normal CDF in float64 (erfc keeps the lower tail's digits)."""
    t = np.asarray(t, np.float64)
    out = np.full(t.shape, np.nan)
    ok = ~np.isnan(t)
    out[ok] = 0.5 * _erfc(-t[ok] / math.sqrt(2.0)).astype(np.float64)
    return out


def lse(a, axis):
    """log sum exp along axis; -inf where every entry is -inf, NaN where any is NaN."""
    a = np.asarray(a, np.float64)
    mx = np.max(a, axis=axis, keepdims=True)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.log(np.sum(np.exp(a - safe), axis=axis, keepdims=True)) + safe
    return np.squeeze(out, axis=axis)


def log_terms(y, mu, lv):
    """l_ki (B, K, n) and its term magnitudes 1/2 (log 2pi + |lv| + d^2 exp(-lv))."""
    y, mu, lv = (np.asarray(a, np.float64) for a in (y, mu, lv))
    d = y[:, None, :] - mu
    q = d * d * np.exp(-lv)
    return -0.5 * (LOG_2PI + lv + q), 0.5 * (LOG_2PI + np.abs(lv) + q)


def logw(lv_q, lv_p, eps, z, mu_p):
    """(logw, magnitude) (B, K): lv_q, lv_p, mu_p (B, m), eps, z (B, K, m)."""
    lv_q, lv_p, eps, z, mu_p = (np.asarray(a, np.float64) for a in (lv_q, lv_p, eps, z, mu_p))
    q = (z - mu_p[:, None]) ** 2 * np.exp(-lv_p)[:, None]
    w = 0.5 * (lv_q[:, None] - lv_p[:, None] + eps ** 2 - q).sum(-1)
    mag = 0.5 * (np.abs(lv_q)[:, None] + np.abs(lv_p)[:, None] + eps ** 2 + q).sum(-1)
    return w, mag


def predictive(y, mu, lv, logw=None, bins=20, levels=(0.5, 0.9, 0.95)):
    """Every quantity of the definitions as float64 (pit_hist int64), plus the magnitudes:
    ll_mag (B, K); mix_mag (B,) = mean_i max_k |terms of l_ki|; moment_mag, sharp_mag (B,)."""
    y, mu, lv = (np.asarray(a, np.float64) for a in (y, mu, lv))
    B, K, n = mu.shape
    l, lmag = log_terms(y, mu, lv)
    mean = mu.mean(1)
    var_a = np.exp(lv).mean(1)
    var_e = ((mu - mean[:, None]) ** 2).mean(1)
    logdens = lse(l, 1) - math.log(K)
    pit = ndtr((y[:, None] - mu) * np.exp(-0.5 * lv)).mean(1)
    ll = l.sum(-1)
    v = var_a + var_e
    with np.errstate(divide="ignore", invalid="ignore"):
        mom_terms = np.stack([np.full_like(v, LOG_2PI), np.log(v), (y - mean) ** 2 / v])
    w = ll + (0.0 if logw is None else np.asarray(logw, np.float64))
    with np.errstate(invalid="ignore"):
        idx = np.minimum(bins - 1, np.floor(pit * bins))
    hist = np.stack([np.array([(idx[b] == j).sum() for j in range(bins)], np.int64) for b in range(B)])
    with np.errstate(invalid="ignore"):
        cov = np.stack([(np.abs(pit - 0.5) <= lev / 2).mean(-1) for lev in levels], -1) if len(levels) else \
            np.zeros((B, 0))
    return dict(l=l, mean=mean, var_aleatoric=var_a, var_epistemic=var_e, logdens=logdens, pit=pit, ll=ll,
                nll_mixture=-logdens.mean(-1), nll_moment=0.5 * mom_terms.sum(0).mean(-1),
                sharpness=np.sqrt(v).mean(-1), pit_hist=hist, coverage=cov, elbo=w.mean(-1),
                iwae=lse(w, 1) - math.log(K), ll_mag=lmag.sum(-1), mix_mag=lmag.max(1).mean(-1),
                moment_mag=0.5 * np.abs(mom_terms).sum(0).mean(-1), sharp_mag=np.sqrt(v).mean(-1))


def near_edge(pit, bins, levels, delta=2e-6):
    """Number of samples whose PIT lies within delta of a histogram edge or a coverage edge
    1/2 +- level/2: there a count may legitimately fall either side."""
    pit = np.asarray(pit, np.float64)
    edges = np.concatenate([np.arange(1, bins) / bins] + [np.array([0.5 - lev / 2, 0.5 + lev / 2]) for lev in levels])
    with np.errstate(invalid="ignore"):
        return int((np.abs(pit[..., None] - edges) <= delta).any(-1).sum())
