"""Numpy restatement of every definition of vaeteb.clseval (its module docstring),
deliberately naive: Python loops for the strike rule, boolean masks for the counts, an O(W^2) pair
count in int64 for the AUC.  The tests hold the kernels of csrc/clseval.hip and the host code of
vaeteb/clseval.py to these, exactly."""
import numpy as np


def fires(p, thr):
    """(W,) bool: p > thr as a strict float32 comparison; a NaN p never fires."""
    with np.errstate(invalid="ignore"):
        return np.asarray(p, np.float32) > np.float32(thr)


def first_alarm(p, thr, strike, mode, ordinal=None):
    """One recording, one threshold: the least j at which the strike rule holds, -1 if none."""
    fire = fires(p, thr)
    run = 0
    for j in range(len(fire)):
        if mode == "consecutive":
            if ordinal is not None and j > 0 and int(ordinal[j]) != int(ordinal[j - 1]) + 1:
                run = 0
            run = run + 1 if fire[j] else 0
        elif mode == "cumulative":
            run += 1 if fire[j] else 0
        else:
            raise ValueError(mode)
        if run >= strike:
            return j
    return -1


def alarm_sweep(p, rec_base, thresholds, strike, mode, ordinal=None):
    """first (R, T) int32."""
    R, T = len(rec_base) - 1, len(thresholds)
    first = np.full((R, T), -1, np.int32)
    for r in range(R):
        a, b = int(rec_base[r]), int(rec_base[r + 1])
        o = None if ordinal is None else ordinal[a:b]
        for t in range(T):
            first[r, t] = first_alarm(p[a:b], thresholds[t], strike, mode, o)
    return first


def recording_counts(first, labels, n_r):
    """(T, 4) {tp, fp, tn, fn} of first >= 0 against labels, over recordings with a kept window."""
    out = np.zeros((first.shape[1], 4), np.int64)
    for t in range(first.shape[1]):
        for r in range(first.shape[0]):
            if n_r[r] == 0:
                continue
            alarm, pos = first[r, t] >= 0, labels[r] != 0
            out[t, 0 if alarm and pos else 1 if alarm else 3 if pos else 2] += 1
    return out


def select_threshold(thresholds, rec_counts, target_fpr):
    """The smallest grid threshold whose recording-level false-positive rate is <= target_fpr."""
    for t in range(len(thresholds)):
        fp, tn = int(rec_counts[t, 1]), int(rec_counts[t, 2])
        if fp + tn == 0:
            raise ValueError("no scored negative recording")
        if fp / (fp + tn) <= target_fpr:
            return t, float(thresholds[t])
    raise ValueError("no threshold qualifies")


def confusion(p, label, thresholds, group=None, G=1):
    """counts (G, T, 4) int32 {tp, fp, tn, fn}; group None: everything in group 0."""
    label = np.asarray(label) != 0
    grp = np.zeros(len(label), np.int64) if group is None else np.asarray(group)
    out = np.zeros((G, len(thresholds), 4), np.int32)
    for g in range(G):
        m = grp == g
        for t, th in enumerate(thresholds):
            pred = fires(p, th)
            out[g, t] = [(m & pred & label).sum(), (m & pred & ~label).sum(), (m & ~pred & ~label).sum(),
                         (m & ~pred & label).sum()]
    return out


def metrics(c):
    """One group's (tp, fp, tn, fn) -> accuracy, precision, recall, specificity, f1 in float64."""
    tp, fp, tn, fn = (float(v) for v in c)
    n = tp + fp + tn + fn
    return dict(accuracy=(tp + tn) / n if n else float("nan"),
                precision=tp / (tp + fp) if tp + fp else 0.0,
                recall=tp / (tp + fn) if tp + fn else 0.0,
                specificity=tn / (tn + fp) if tn + fp else float("nan"),
                f1=2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)


def pair_counts(p, label, weight=None):
    """(gt, eq, P, N) as Python ints: the O(W^2) pair count over (positive, negative) pairs; a window
    with NaN p has weight 0."""
    p = np.asarray(p, np.float32)
    w = np.ones(len(p), np.int64) if weight is None else np.asarray(weight, np.int64).copy()
    w[np.isnan(p)] = 0
    pos, neg = np.asarray(label) != 0, np.asarray(label) == 0
    pp, pn, wp, wn = p[pos], p[neg], w[pos], w[neg]
    with np.errstate(invalid="ignore"):
        ww = wp[:, None] * wn[None, :]
        gt = int((ww * (pp[:, None] > pn[None, :])).sum(dtype=np.int64))
        eq = int((ww * (pp[:, None] == pn[None, :])).sum(dtype=np.int64))
    return gt, eq, int(wp.sum()), int(wn.sum())


def auc(p, label, weight=None):
    gt, eq, P, N = pair_counts(p, label, weight)
    return (float(gt) + 0.5 * float(eq)) / (float(P) * float(N)) if P and N else float("nan")


def auc_ranks(p, label, rec=None, group=None, G=1, mult=None):
    """(Bt, G, 4) int64 {gt, eq, P, N}."""
    W = len(p)
    grp = np.zeros(W, np.int64) if group is None else np.asarray(group)
    Bt = 1 if mult is None else len(mult)
    out = np.zeros((Bt, G, 4), np.int64)
    for b in range(Bt):
        w = np.ones(W, np.int64) if mult is None else np.asarray(mult[b], np.int64)[np.asarray(rec, np.int64)]
        for g in range(G):
            out[b, g] = pair_counts(p, label, np.where(grp == g, w, 0))
    return out


def multiplicities(R, n_boot, seed):
    return np.random.Generator(np.random.PCG64(seed)).multinomial(R, np.full(R, 1 / R), size=n_boot)


def ordinals(rec_all, kept):
    """The ordinal of every kept window among all windows of its recording."""
    out, seen = [], {}
    for i, r in enumerate(rec_all):
        seen[r] = seen.get(r, -1) + 1
        out.append(seen[r])
    return np.asarray(out, np.int32)[np.asarray(kept, np.int64)]
