"""Numpy restatement of every definition of vaeteb.tenull (its module docstring),
deliberately naive: the surrogate rows materialised sample by sample from a plan, the KL per step in
float64, every count by a loop over recordings and variants (tests/test_tenull_cpu.py checks these
against a loop over every single comparison).  The tests hold the kernels of
csrc/tenull.hip, vt_fe_spectrum_surrogate and the host code of vaeteb/tenull.py to these."""
import numpy as np


def surrogate_index(N, shift, perm, block_len):
    """(N,) int64: the sample of the source channel that surrogate sample i reads,
    m((i - shift) mod N) with m the block permutation (identity in the tail and when perm is None)."""
    j = (np.arange(N, dtype=np.int64) - int(shift)) % N
    if perm is None:
        return j
    nblk = N // int(block_len)
    body = nblk * int(block_len)
    blk = np.minimum(j // int(block_len), nblk - 1)           # the tail's value is not used
    moved = np.asarray(perm, np.int64)[blk] * int(block_len) + j % int(block_len)
    return np.where(j < body, moved, j)


def materialise(x, plan):
    """(B, K+1, N): the up channel of every (recording, variant) row of the plan; x (B, 2, N)."""
    x = np.asarray(x)
    B, _, N = x.shape
    K1 = plan.src.shape[1]
    out = np.empty((B, K1, N), x.dtype)
    for b in range(B):
        for k in range(K1):
            idx = surrogate_index(N, plan.shift[b, k], None if plan.perm is None else plan.perm[b, k],
                                  plan.block_len)
            out[b, k] = x[int(plan.src[b, k]), 1, idx]
    return out


def kl_steps(mu_c, lv_q, mu_y, lv_p, K1):
    """ts (R, S) and te (R,) in float64 from float32 inputs: mu_c, lv_q (R, S, L) with R = B * K1, the
    prior mu_y, lv_p (B, S, L) read at row r // K1; the elementwise KL is
    0.5 (lv_p - lv_q - 1 + (exp(lv_q) + (mu_q - mu_y)^2) / exp(lv_p)) with mu_q = mu_c + mu_y."""
    mu_c, lv_q = np.asarray(mu_c, np.float64), np.asarray(lv_q, np.float64)
    my = np.repeat(np.asarray(mu_y, np.float64), K1, axis=0)
    lp = np.repeat(np.asarray(lv_p, np.float64), K1, axis=0)
    dm = (mu_c + my) - my
    kl = 0.5 * (lp - lv_q - 1.0 + (np.exp(lv_q) + dm * dm) / np.exp(lp))
    return kl.mean(-1), kl.mean((-2, -1))


def ge(a, b):
    """a >= b as a float32 comparison (scalars or arrays); a NaN on either side never counts."""
    with np.errstate(invalid="ignore"):
        return np.asarray(a, np.float32) >= np.asarray(b, np.float32)


def row_max(v):
    """The maximum of a float32 row skipping NaN, -inf when nothing is left."""
    v = np.asarray(v, np.float32)
    v = v[~np.isnan(v)]
    return v.max() if v.size else np.float32(-np.inf)


def stats(ts, te):
    """Every output of vt_tenull_stats from ts (B, K+1, S) and te (B, K+1) float32."""
    ts, te = np.asarray(ts, np.float32), np.asarray(te, np.float32)
    B, K1, S = ts.shape
    K = K1 - 1
    count_ge = np.zeros(B, np.int32)
    step_count_ge, max_count_ge = np.zeros((B, S), np.int32), np.zeros((B, S), np.int32)
    surr_mean, surr_sd = np.zeros(B), np.zeros(B)
    step_surr_mean = np.zeros((B, S), np.float32)
    for b in range(B):
        acc = np.zeros(S)
        for k in range(1, K1):
            count_ge[b] += int(ge(te[b, k], te[b, 0]))
            step_count_ge[b] += ge(ts[b, k], ts[b, 0])            # over the steps at once
            max_count_ge[b] += ge(row_max(ts[b, k]), ts[b, 0])
            acc += ts[b, k].astype(np.float64)
        surr = te[b, 1:].astype(np.float64)
        surr_mean[b] = surr.sum() / K
        with np.errstate(invalid="ignore", divide="ignore"):
            surr_sd[b] = np.sqrt(np.float64(((surr - surr_mean[b]) ** 2).sum()) / np.float64(K - 1))
        step_surr_mean[b] = (acc / K).astype(np.float32)
    group_sums = te.astype(np.float64).sum(0)
    return dict(count_ge=count_ge, step_count_ge=step_count_ge, max_count_ge=max_count_ge, surr_mean=surr_mean,
                surr_sd=surr_sd, step_surr_mean=step_surr_mean, group_sums=group_sums)


def quantised(B, K1, S, seed):
    """Test inputs ts (B, K1, S) and te (B, K1) float32 on eight distinct values, so that every
    comparison meets ties and >= against > matters."""
    rng = np.random.default_rng(seed)
    grid = (np.arange(8, dtype=np.float32) - 3) / 4
    return grid[rng.integers(0, 8, (B, K1, S))], grid[rng.integers(0, 8, (B, K1))]


def p_value(count, K):
    return (1.0 + np.asarray(count, np.float64)) / (K + 1)


def group_p(group_sums):
    g = np.asarray(group_sums, np.float64)
    return (1.0 + float((g[1:] >= g[0]).sum())) / len(g)
