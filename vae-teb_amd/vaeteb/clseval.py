"""What the classifier is for: given labelled recordings, does it raise an alarm on the right ones, at
what false-positive rate, and how early?  The kept windows of a RecordingWindows are scored by the
classifier on the posterior mean of the latent (the decoder never runs), and the class-1 probability
p of every window goes through three integer statistics, one launch each (csrc/clseval.hip).

What is the reference's: the per-window table of test_classifier (guid, epoch_num, prob_class_0,
prob_class_1, predicted_class, true_label: ref/model/graph_model_refactored_cls.py:737-801), the
metrics of analyze_and_plot_classification_metrics (accuracy, precision, recall, specificity, F1 and
AUROC, overall and per epoch group: ref/utils/data_utils.py:1489-1660) and the idea of
test_classifier_with_strike_and_fpr (:1130-1220): sweep thresholds through a strike rule and take the
one that meets a target false-positive rate.  Its strike helpers are imported from a module that is
not in the reference tree, so the definitions below are this package's own contract.

Windows of recording r: its kept windows j = 0 .. n_r - 1 in ascending start; fire_j(t) = p_j > thr_t,
a strict float32 comparison; a NaN p never fires and counts as prediction 0.

    consecutive   run_j = fire_j ? run_{j-1} + 1 : 0; with break_on_gap the run restarts (run_{j-1}
                  taken as 0) when the window's ordinal among all windows of the recording, kept or
                  rejected, is not its predecessor's plus one: a window the gate dropped breaks a run
    cumulative    run_j = #{i <= j : fire_i}
    first[r, t]   the least j with run_j >= strike, -1 if none                       vt_cls_alarm_sweep
    rec_counts[t] {tp, fp, tn, fn} of first >= 0 against the labels, over recordings with n_r > 0
    threshold     as given, else the smallest grid threshold whose recording-level false-positive
                  rate fp / (fp + tn) is <= target_fpr (the rate does not increase with the threshold
                  in either mode, and no window fires at 1.0)
    alarm_epoch   the epoch of window first[r, t*]
    counts[g, t]  {tp, fp, tn, fn} of the windows of group g, a window's label its recording's;
                  group = np.digitize(epoch, epoch_bins) - 1, -1 or G = no group      vt_cls_confusion
    AUC           (gt + eq / 2) / (P N) in float64 from the integers
                  gt = sum_{i pos, j neg} w_i w_j [p_i > p_j], eq the same with ==, P, N the weighted
                  class sizes; NaN when P N = 0; a NaN p has weight 0                 vt_cls_auc_ranks
                  (the trapezoid area under sklearn's roc_curve: ties at half weight)
    bootstrap     over recordings (a cluster bootstrap): w_i = mult[b, rec_i] with
                  mult = Generator(PCG64(seed)).multinomial(R, 1/R, size=n_boot); replicates with
                  P N = 0 are invalid and left out of the percentiles

Not here: plots, the CS / no-bg CSV merges and the blood-gas analysis of the reference's script.
"""
import math

import numpy as np
import torch

from . import _lib
from .timeline import TimelineLayout, stitch

MODES = {"consecutive": 0, "cumulative": 1}
COLUMNS = ("guid", "epoch_num", "prob_class_0", "prob_class_1", "predicted_class", "true_label")
METRICS = ("accuracy", "precision", "recall", "specificity", "f1")


def default_thresholds():
    """The grid of 401 thresholds 0, 0.0025, ..., 1 (float32)."""
    return np.linspace(0, 1, 401).astype(np.float32)


def check_args(R, labels=None, strike=2, mode="consecutive", target_fpr=0.3, threshold=None, thresholds=None,
               epoch_bins=None, n_boot=1000, seed=0):
    """Every argument of an evaluation checked on the host, before any launch (ValueError).  Returns
    (labels (R,) uint8 or None, strike, mode code, target_fpr, threshold or None, thresholds (T,)
    float32, epoch_bins float64 or None, n_boot, seed)."""
    R = int(R)
    lab = None
    if labels is not None:
        a = np.asarray(labels)
        if a.shape != (R,):
            raise ValueError(f"labels must have shape ({R},), one per recording, got {a.shape}")
        if a.dtype != np.bool_ and not np.isin(a, (0, 1)).all():
            raise ValueError("labels must be 0 or 1")
        lab = np.ascontiguousarray(a.astype(np.uint8))
    if isinstance(strike, bool) or not isinstance(strike, (int, np.integer)) or strike < 1 or strike >= 2 ** 31:
        raise ValueError(f"strike must be an integer >= 1, got {strike!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    tf = float(target_fpr)
    if not 0.0 < tf < 1.0:
        raise ValueError(f"target_fpr must lie in (0, 1), got {target_fpr!r}")
    if threshold is not None:
        threshold = float(threshold)
        if not math.isfinite(threshold):
            raise ValueError(f"threshold must be finite, got {threshold!r}")
    thr = default_thresholds() if thresholds is None else np.asarray(thresholds)
    if thr.ndim != 1 or thr.size < 1 or thr.size > 1 << 24:
        raise ValueError(f"thresholds must be a 1-D array of 1 to 2^24 values, got shape {thr.shape}")
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    if not np.isfinite(thr).all() or np.any(np.diff(thr) < 0):
        raise ValueError("thresholds must be finite and ascending")
    bins = None
    if epoch_bins is not None:
        bins = np.ascontiguousarray(epoch_bins, dtype=np.float64)
        if bins.ndim != 1 or bins.size < 2 or bins.size > 65536 or not np.isfinite(bins).all() \
                or np.any(np.diff(bins) <= 0):
            raise ValueError("epoch_bins must be 2 to 65536 finite, strictly ascending edges")
    if isinstance(n_boot, bool) or not isinstance(n_boot, (int, np.integer)) or n_boot < 0:
        raise ValueError(f"n_boot must be an integer >= 0, got {n_boot!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError(f"seed must be a non-negative integer, got {seed!r}")
    return lab, int(strike), MODES[mode], tf, threshold, thr, bins, int(n_boot), int(seed)


def multiplicities(R, n_boot, seed=0):
    """(n_boot, R) int32: how often each recording is drawn in each bootstrap replicate."""
    R, n_boot = int(R), int(n_boot)
    if R == 0 or n_boot == 0:
        return np.zeros((n_boot, R), np.int32)
    g = np.random.Generator(np.random.PCG64(int(seed)))
    return g.multinomial(R, np.full(R, 1.0 / R), size=n_boot).astype(np.int32)


def window_ordinals(rec_all, kept):
    """(W,) int32: the ordinal of every kept window among all windows of its recording.  rec_all: the
    recording index of every window, kept or rejected, ascending; kept: the kept windows' indices."""
    rec_all = np.asarray(rec_all, np.int64)
    if rec_all.size == 0:
        return np.zeros(0, np.int32)
    head = np.searchsorted(rec_all, rec_all, side="left")
    return (np.arange(rec_all.size, dtype=np.int64) - head)[np.asarray(kept, np.int64)].astype(np.int32)


def recording_counts(first, labels, scored):
    """(T, 4) int64 {tp, fp, tn, fn}: the alarm first >= 0 against labels, over the scored recordings."""
    alarm = np.asarray(first) >= 0
    lab = np.asarray(labels).astype(bool)[:, None] & np.ones_like(alarm)
    use = np.asarray(scored).astype(bool)[:, None]
    c = [(alarm & lab & use).sum(0), (alarm & ~lab & use).sum(0), (~alarm & ~lab & use).sum(0),
         (~alarm & lab & use).sum(0)]
    return np.stack(c, axis=1).astype(np.int64)


def select_threshold(thresholds, rec_counts, target_fpr):
    """(index, threshold) of the smallest grid threshold whose recording-level false-positive rate
    fp / (fp + tn) is <= target_fpr.  ValueError without a negative recording, or when no grid
    threshold qualifies (a grid that stops short of the largest p)."""
    c = np.asarray(rec_counts, np.int64)
    neg = c[:, 1] + c[:, 2]
    if c.shape[0] == 0 or neg[0] == 0:
        raise ValueError("no scored negative recording: the false-positive rate is undefined")
    ok = np.nonzero(c[:, 1].astype(np.float64) / neg.astype(np.float64) <= float(target_fpr))[0]
    if ok.size == 0:
        raise ValueError(f"no threshold of the grid reaches a false-positive rate of {target_fpr}")
    return int(ok[0]), float(np.asarray(thresholds)[ok[0]])


def metrics_from_counts(counts):
    """counts (..., 4) integer {tp, fp, tn, fn} -> dict of float64 arrays (...): accuracy, precision,
    recall, specificity, f1, with the reference's conventions (sklearn's zero_division=0 for precision,
    recall and F1; specificity NaN without negatives; accuracy NaN for an empty group)."""
    c = np.asarray(counts).astype(np.float64)
    tp, fp, tn, fn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        n = tp + fp + tn + fn
        acc = np.where(n > 0, (tp + tn) / n, np.nan)
        prec = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        rec = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
        spec = np.where(tn + fp > 0, tn / (tn + fp), np.nan)
        f1 = np.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn), 0.0)
    return dict(accuracy=acc, precision=prec, recall=rec, specificity=spec, f1=f1)


def auc_from_ranks(ranks):
    """ranks (..., 4) int64 {gt, eq, P, N} -> (gt + eq / 2) / (P N) in float64, NaN where P N = 0."""
    r = np.asarray(ranks, np.int64)
    gt, eq, P, N = (r[..., i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((r[..., 2] != 0) & (r[..., 3] != 0), (gt + 0.5 * eq) / (P * N), np.nan)


# ------------------------------------------------------------------ the three statistics
def _dev(a, device, dtype):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype).contiguous()


def _check_p(p):
    if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.dtype != torch.float32 or not p.is_cuda:
        raise ValueError("p must be a float32 device tensor (W,)")
    return p.contiguous()


def alarm_sweep(p, rec_base, thresholds, strike=2, mode="consecutive", ordinal=None, out=None):
    """first (R, T) int32 on the device: vt_cls_alarm_sweep.  p (W,) float32 on the device; rec_base
    (R+1,) the CSR of the kept windows (host table, checked: ascending from 0 to W); thresholds (T,);
    ordinal (W,) int32 or None (no gap breaks a run)."""
    p = _check_p(p)
    W = p.shape[0]
    base = np.ascontiguousarray(rec_base, dtype=np.int64).reshape(-1)
    if base.size < 1 or base[0] != 0 or base[-1] != W or np.any(np.diff(base) < 0):
        raise ValueError(f"rec_base must ascend from 0 to the {W} windows")
    _, strike, mode, _, _, thr, _, _, _ = check_args(0, strike=strike, mode=mode, thresholds=thresholds)
    R, T = base.size - 1, thr.size
    o = None
    if ordinal is not None:
        if np.shape(ordinal) != (W,):
            raise ValueError(f"ordinal must have shape ({W},), got {np.shape(ordinal)}")
        o = _dev(ordinal, p.device, torch.int32)
    first = torch.empty((R, T), dtype=torch.int32, device=p.device) if out is None else out
    if tuple(first.shape) != (R, T) or first.dtype != torch.int32 or not first.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 ({R}, {T}) tensor")
    base_dev, thr_dev = _dev(base, p.device, torch.int64), _dev(thr, p.device, torch.float32)   # alive over the call
    _lib.call("vt_cls_alarm_sweep", _lib.ptr(p), W, _lib.ptr(base_dev), R, _lib.ptr(o), _lib.ptr(thr_dev), T, strike,
              mode, _lib.ptr(first), _lib.stream())
    return first


def _labels_groups(p, label, group, G):
    W = p.shape[0]
    if tuple(np.shape(label)) != (W,):
        raise ValueError(f"label must have shape ({W},), got {tuple(np.shape(label))}")
    if group is not None and tuple(np.shape(group)) != (W,):
        raise ValueError(f"group must have shape ({W},), got {tuple(np.shape(group))}")
    G = int(G)
    if G < 1 or G > 65535:
        raise ValueError(f"G must be in 1..65535, got {G}")
    return _dev(label, p.device, torch.uint8), None if group is None else _dev(group, p.device, torch.int32), G


def confusion(p, label, thresholds, group=None, G=1, out=None):
    """counts (G, T, 4) int32 {tp, fp, tn, fn} on the device: vt_cls_confusion.  label (W,) 0/1 per
    window; group (W,) int32 or None (one group)."""
    p = _check_p(p)
    lab, grp, G = _labels_groups(p, label, group, G)
    thr = check_args(0, thresholds=thresholds)[5]
    T = thr.size
    counts = torch.empty((G, T, 4), dtype=torch.int32, device=p.device) if out is None else out
    if tuple(counts.shape) != (G, T, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 ({G}, {T}, 4) tensor")
    thr_dev = _dev(thr, p.device, torch.float32)
    _lib.call("vt_cls_confusion", _lib.ptr(p), _lib.ptr(lab), _lib.ptr(grp), p.shape[0], G, _lib.ptr(thr_dev), T,
              _lib.ptr(counts), _lib.stream())
    return counts


def auc_ranks(p, label, rec=None, group=None, G=1, mult=None, out=None, sort=None):
    """(Bt, G, 4) int64 {gt, eq, P, N} on the device: one torch.sort of p (or sort=(p_sorted, order)
    from an earlier call), then vt_cls_auc_ranks.  mult (Bt, R) int32 multiplicities over the
    recordings rec (W,) of the windows, or None: one replicate, every weight 1."""
    p = _check_p(p)
    lab, grp, G = _labels_groups(p, label, group, G)
    W = p.shape[0]
    Bt, R, m, r = 1, 0, None, None
    if mult is not None:
        if rec is None or tuple(np.shape(rec)) != (W,):
            raise ValueError(f"mult needs rec of shape ({W},)")
        if len(np.shape(mult)) != 2:
            raise ValueError(f"mult must be (replicates, recordings), got shape {tuple(np.shape(mult))}")
        Bt, R = (int(s) for s in np.shape(mult))
        m, r = _dev(mult, p.device, torch.int32), _dev(rec, p.device, torch.int32)
    ps, order = torch.sort(p) if sort is None else sort
    ranks = torch.empty((Bt, G, 4), dtype=torch.int64, device=p.device) if out is None else out
    if tuple(ranks.shape) != (Bt, G, 4) or ranks.dtype != torch.int64 or not ranks.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 ({Bt}, {G}, 4) tensor")
    ps, order = ps.contiguous(), order.contiguous()
    _lib.call("vt_cls_auc_ranks", _lib.ptr(ps), _lib.ptr(order), W, _lib.ptr(lab),
              _lib.ptr(r), _lib.ptr(grp), G, _lib.ptr(m), Bt, R, _lib.ptr(ranks), _lib.stream())
    return ranks


# ------------------------------------------------------------------ result
class ClassifierWindows:
    """The kept windows: device p, p0 (W,) float32 the class-1 / class-0 probabilities; host rec,
    start, epoch, label (arrays) and guid (list)."""

    def __init__(self, p, p0, rec, start, epoch, guid, label):
        self.p, self.p0, self.rec, self.start, self.epoch, self.guid, self.label = p, p0, rec, start, epoch, guid, label

    def __len__(self):
        return len(self.guid)


class ClassifierEvaluation:
    """R recordings, W kept windows, T thresholds, G epoch groups.

    On the device: windows.p (W,) float32; prob[i] (L_i // step,) float32, the overlap-mean of the
    window probabilities over the steps each window covers (NaN where uncovered) with
    coverage_steps[i] int32; thresholds (T,) float32; first (R, T) int32; rec_counts (T, 4) int64;
    counts (G, T, 4) int32; ranks (1 + n_boot, 1, 4) and ranks_groups (1, G, 4) int64, the integers
    behind the AUCs (row 0 of ranks: every recording once).
    On the host (read once, after the last launch): threshold (float) and threshold_index (its grid
    index, None for a threshold given off the grid); alarm (R,) bool, alarm_epoch (R,) float64, NaN
    without an alarm; unscored, the list of recordings without a kept window; labels (R,) uint8; auc
    (float), auc_groups (G,), auc_boot (n_boot,) float64 with NaN for invalid replicates; auc_ci the
    (2.5, 97.5) percentiles over the n_valid valid replicates (NaN when there is none); strike, mode,
    target_fpr, epoch_bins, seed; layout, the TimelineLayout of prob."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def _counts_at(self, threshold):
        if threshold is None:
            threshold = self.threshold
        t32 = np.float32(threshold)
        thr = self._thr_host
        i = int(np.searchsorted(thr, t32))
        if i < thr.size and thr[i] == t32:
            return self.counts[:, i].cpu().numpy()
        w = self.windows
        c = confusion(w.p, self._label_dev, np.array([t32]), self._group_dev, self.counts.shape[0])
        return c[:, 0].cpu().numpy()

    def metrics(self, threshold=None):
        """accuracy, precision, recall, specificity, f1 of every group at `threshold` (default: the
        operating point), each (G,) float64, from the integer window counts (metrics_from_counts);
        counts: the (G, 4) integers.  A threshold off the grid is counted by one more launch."""
        c = self._counts_at(threshold)
        return dict(metrics_from_counts(c), counts=c)

    def rows(self, threshold=None):
        """One dict per kept window with the reference's CSV columns: guid, epoch_num, prob_class_0,
        prob_class_1, predicted_class (p > threshold, float32), true_label.  One host read."""
        w = self.windows
        if not len(w):
            return []
        t32 = np.float32(self.threshold if threshold is None else threshold)
        v = torch.stack([w.p0, w.p], 1).cpu().numpy()
        return [dict(guid=g, epoch_num=float(e), prob_class_0=float(r[0]), prob_class_1=float(r[1]),
                     predicted_class=int(r[1] > t32), true_label=int(l))
                for g, e, r, l in zip(w.guid, w.epoch, v, w.label)]


# ------------------------------------------------------------------ scorer
class ClassifierScorer:
    """scorer = ClassifierScorer(model, frontend); ev = scorer(windows) with a SeqVaeTebClassifier, a
    FrontEnd with statistics and a RecordingWindows.

    Per batch of kept windows: frontend(b.x), model.vae_model.encode(...), z = mu_post (sample=False:
    no noise is drawn, the device's random stream is untouched) or one torch.randn((b, 1, S, L)) and
    z = mu_post + eps exp(logvar_post / 2) through vt_pred_draw_rows (sample=True), then
    model.classifier(z) in eval mode and torch.softmax.  The decoder never runs; the model is left in
    eval mode.  The tables of the statistics come from the host arrays that RecordingWindows holds;
    the host reads the integer results once, after the last launch (twice when the threshold is
    chosen from the sweep), to form the operating point, the alarms and the float64 AUCs.

    labels: (R,) 0/1, default each recording's bg_label.  threshold: the operating point as given (it
    need not be on the grid), else chosen for target_fpr.  epoch_bins: the edges of the window groups
    (np.digitize), None: one group holding everything."""

    def __init__(self, model, frontend):
        self.model, self.frontend = model, frontend

    @torch.no_grad()
    def __call__(self, windows, labels=None, strike=2, mode="consecutive", target_fpr=0.3, threshold=None,
                 thresholds=None, epoch_bins=None, n_boot=1000, seed=0, sample=False, break_on_gap=True):
        fe, m = self.frontend, self.model
        p = fe.plan
        recs = windows.recordings
        R = len(recs)
        if labels is None:
            labels = np.array([r.bg_label for r in recs], np.uint8)
        lab, strike_, mode_, tf, threshold, thr, bins, n_boot, seed = check_args(
            R, labels, strike, mode, target_fpr, threshold, thresholds, epoch_bins, n_boot, seed)
        if fe.stats is None:
            raise RuntimeError("FrontEnd needs normalisation statistics (set_stats)")
        if p.N != windows.N:
            raise ValueError(f"front-end built for N = {p.N}, windows are N = {windows.N}")
        vae = m.vae_model
        if fe.S_out != vae.decoder.sequence_length:
            raise ValueError(f"the front-end gives {fe.S_out} steps, the model takes {vae.decoder.sequence_length}")
        if getattr(m.classifier, "use_attention", False) and (fe.S_out % 16 or fe.S_out > 256):
            raise ValueError(f"the classifier's attention takes a multiple of 16 steps up to 256, the front-end gives "
                             f"{fe.S_out}")
        layout = TimelineLayout(recs, step=p.step)
        kept = windows.kept
        rec, start = windows.rec[kept], windows.start[kept]
        step_off, _ = layout.window_offsets(rec, start, fe)
        W, S, L = len(rec), fe.S_out, m.latent_dim_z
        n_r = np.bincount(rec, minlength=R).astype(np.int64) if W else np.zeros(R, np.int64)
        rec_base = np.zeros(R + 1, np.int64)
        np.cumsum(n_r, out=rec_base[1:])
        scored = n_r > 0
        if threshold is None and not (scored & (lab == 0)).any():
            raise ValueError("no scored negative recording: the false-positive rate is undefined")
        ordinal = window_ordinals(windows.rec, kept) if break_on_gap else None
        dev = windows.buffer.device

        # ---- scoring
        m.eval()
        if getattr(vae, "h16_format", None):
            _lib.set_h16(vae.h16_format == "fp16")
        probs = torch.empty((W, 2), device=dev)
        epoch, guid = [], []
        w0 = 0
        for b in windows:
            nb = b.x.shape[0]
            f = fe(b.x)
            _, _, mu_post, lv_post = vae.encode(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"])
            z = mu_post.contiguous()
            if sample:
                eps = torch.randn((nb, 1, S, L), device=dev)
                lv, zs, logw = lv_post.contiguous(), torch.empty_like(z), torch.empty(nb, device=dev)
                _lib.call("vt_pred_draw_rows", _lib.ptr(z), _lib.ptr(lv), _lib.ptr(eps), None, None,
                          nb, 1, S * L, _lib.ptr(zs), _lib.ptr(logw), _lib.stream())
                z = zs
            logits = m.classifier(z)
            if logits.shape[-1] != 2:
                raise ValueError(f"a two-class classifier is evaluated, this one has {logits.shape[-1]} classes")
            probs[w0:w0 + nb].copy_(torch.softmax(logits, dim=-1))
            epoch.append(b.epoch)
            guid.extend(b.guid)
            w0 += nb
        assert w0 == W, (w0, W)
        epoch = np.concatenate(epoch) if epoch else np.zeros(0, np.float64)
        pw, p0 = probs[:, 1].contiguous(), probs[:, 0].contiguous()

        # ---- probability timelines
        if W:
            prob, count = stitch(pw[:, None].expand(W, S).contiguous(), step_off, layout.n_steps)
        else:
            prob = torch.full((layout.n_steps,), math.nan, device=dev)
            count = torch.zeros(layout.n_steps, dtype=torch.int32, device=dev)
        sb = layout.step_base
        cut = lambda t: [t[int(sb[i]):int(sb[i + 1])] for i in range(R)]

        # ---- statistics
        thr_dev = torch.from_numpy(thr).to(dev)
        wlab = lab[rec] if W else np.zeros(0, np.uint8)
        G = 1 if bins is None else bins.size - 1
        group = None if bins is None else (np.digitize(epoch, bins) - 1).astype(np.int32)
        wlab_dev = torch.from_numpy(wlab).to(dev)
        group_dev = None if group is None else torch.from_numpy(group).to(dev)
        first = alarm_sweep(pw, rec_base, thr, strike_, mode, ordinal)
        counts = confusion(pw, wlab_dev, thr, group_dev, G)
        mult = np.concatenate([np.ones((1, R), np.int32), multiplicities(R, n_boot, seed)])
        srt = torch.sort(pw)
        rec32 = rec.astype(np.int32)
        ranks = auc_ranks(pw, wlab_dev, rec=rec32, mult=mult, sort=srt)
        ranks_groups = ranks[:1] if group is None else auc_ranks(pw, wlab_dev, group=group_dev, G=G, sort=srt)
        lab_dev = torch.from_numpy(lab.astype(bool)).to(dev)[:, None]
        use = torch.from_numpy(scored).to(dev)[:, None]
        alarm_t = first >= 0
        rec_counts = torch.stack([(alarm_t & lab_dev & use).sum(0), (alarm_t & ~lab_dev & use).sum(0),
                                  (~alarm_t & ~lab_dev & use).sum(0), (~alarm_t & lab_dev & use).sum(0)], 1)

        # ---- the host's part: operating point, alarms, float64 AUCs
        if threshold is None:
            ti, threshold = select_threshold(thr, rec_counts.cpu().numpy(), tf)
            col = first[:, ti]
        else:
            t32 = np.float32(threshold)
            i = int(np.searchsorted(thr, t32))
            ti = i if i < thr.size and thr[i] == t32 else None
            col = first[:, ti] if ti is not None else alarm_sweep(pw, rec_base, np.array([t32]), strike_, mode,
                                                                   ordinal)[:, 0]
        col = col.cpu().numpy().astype(np.int64)
        alarm = col >= 0
        alarm_epoch = np.full(R, np.nan)
        alarm_epoch[alarm] = epoch[(rec_base[:-1] + col)[alarm]]
        rk = ranks.cpu().numpy()
        auc_all = auc_from_ranks(rk[:, 0])
        auc_boot = auc_all[1:]
        valid = ~np.isnan(auc_boot)
        n_valid = int(valid.sum())
        ci = tuple(np.percentile(auc_boot[valid], [2.5, 97.5]).tolist()) if n_valid else (math.nan, math.nan)
        auc_groups = auc_from_ranks(ranks_groups.cpu().numpy()[0])
        return ClassifierEvaluation(
            windows=ClassifierWindows(pw, p0, rec, start, epoch, guid, wlab), layout=layout, prob_packed=prob,
            prob=cut(prob), coverage_steps=cut(count), thresholds=thr_dev, first=first, rec_counts=rec_counts,
            threshold=float(threshold), threshold_index=ti, alarm=alarm, alarm_epoch=alarm_epoch,
            unscored=[i for i in range(R) if not scored[i]], labels=lab, counts=counts, ranks=ranks,
            ranks_groups=ranks_groups, auc=float(auc_all[0]), auc_groups=auc_groups, auc_boot=auc_boot, auc_ci=ci,
            n_valid=n_valid, strike=strike_, mode=mode, target_fpr=tf, epoch_bins=bins, seed=seed,
            break_on_gap=bool(break_on_gap), _thr_host=thr, _label_dev=wlab_dev, _group_dev=group_dev)
