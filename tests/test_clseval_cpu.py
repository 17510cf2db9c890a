"""Host side of the classifier evaluation (vaeteb/clseval.py) and its numpy reference
(tests/clseval_ref.py), without a GPU: the reference against hand-worked cases and sklearn, the
properties the definitions promise (monotone in the threshold, strike 1 alike in both modes), the
threshold-selection rule, the bootstrap multiplicities and every host validation error."""
import numpy as np
import pytest

import clseval_ref as ref
from vaeteb import clseval as ce


# ------------------------------------------------------------------ the reference, by hand
def test_strike_rule_hand_cases():
    p = np.array([0.9, 0.2, 0.9, 0.9, 0.5, 0.9], np.float32)
    # fires at 0.5: 1 0 1 1 0 1 (p == thr does not fire)
    assert ref.first_alarm(p, 0.5, 1, "consecutive") == 0
    assert ref.first_alarm(p, 0.5, 2, "consecutive") == 3
    assert ref.first_alarm(p, 0.5, 3, "consecutive") == -1
    assert ref.first_alarm(p, 0.5, 2, "cumulative") == 2
    assert ref.first_alarm(p, 0.5, 4, "cumulative") == 5
    assert ref.first_alarm(p, 0.5, 5, "cumulative") == -1
    assert ref.first_alarm(p, 0.49, 3, "consecutive") == 4          # now 0.5 fires too: 1 0 1 1 1 1
    # a gated window between kept windows 2 and 3 breaks the run; the next pair completes it
    o = np.array([0, 1, 2, 4, 5, 6], np.int32)
    assert ref.first_alarm(p, 0.49, 2, "consecutive", o) == 4
    assert ref.first_alarm(p, 0.49, 2, "cumulative", o) == 2         # ordinals do not matter here
    # NaN never fires and ends a run
    q = np.array([0.9, np.nan, 0.9, 0.9], np.float32)
    assert ref.first_alarm(q, 0.0, 2, "consecutive") == 3 and ref.first_alarm(q, 0.0, 2, "cumulative") == 2
    assert ref.first_alarm(np.zeros(0, np.float32), 0.0, 1, "consecutive") == -1


def test_sweep_counts_and_selection_hand_case():
    p = np.array([0.9, 0.9, 0.1, 0.6, 0.6, 0.7, 0.2, 0.8], np.float32)
    base = np.array([0, 2, 2, 5, 8])                                  # recording 1 has no window
    thr = np.array([0.0, 0.5, 0.65, 0.85, 1.0], np.float32)
    first = ref.alarm_sweep(p, base, thr, 2, "consecutive")
    assert first.tolist() == [[1, 1, 1, 1, -1], [-1] * 5, [1, 2, -1, -1, -1], [1, -1, -1, -1, -1]]
    labels = np.array([1, 1, 0, 0])
    rc = ref.recording_counts(first, labels, np.diff(base))
    assert rc.tolist() == [[1, 2, 0, 0], [1, 1, 1, 0], [1, 0, 2, 0], [1, 0, 2, 0], [0, 0, 2, 1]]
    assert np.array_equal(rc, ce.recording_counts(first, labels, np.diff(base) > 0))
    assert ref.select_threshold(thr, rc, 0.5) == (1, 0.5)
    assert ref.select_threshold(thr, rc, 0.3) == (2, float(np.float32(0.65)))
    for tf in (0.01, 0.3, 0.5, 0.99):
        assert ce.select_threshold(thr, rc, tf) == ref.select_threshold(thr, rc, tf)
    with pytest.raises(ValueError):
        ce.select_threshold(thr, ref.recording_counts(first, np.ones(4), np.diff(base)), 0.3)
    with pytest.raises(ValueError):
        ce.select_threshold(thr[:1], rc[:1], 0.3)                     # the grid stops short: nothing qualifies


def test_confusion_and_metrics_hand_case():
    p = np.array([0.9, 0.4, 0.6, np.nan, 0.5, 0.1], np.float32)
    lab = np.array([1, 1, 0, 1, 0, 0], np.uint8)
    c = ref.confusion(p, lab, np.array([0.5], np.float32))
    assert c.tolist() == [[[1, 1, 2, 2]]]                             # NaN: prediction 0; 0.5 does not fire
    g = np.array([0, 0, 1, 1, -1, 2], np.int32)
    c = ref.confusion(p, lab, np.array([0.5], np.float32), g, 2)
    assert c[:, 0].tolist() == [[1, 0, 0, 1], [0, 1, 0, 1]]
    m = ref.metrics([1, 1, 2, 2])
    assert m == dict(accuracy=0.5, precision=0.5, recall=1 / 3, specificity=2 / 3, f1=2 / 5)
    assert ref.metrics([0, 0, 3, 0]) == dict(accuracy=1.0, precision=0.0, recall=0.0, specificity=1.0, f1=0.0)
    e = ref.metrics([2, 0, 0, 1])
    assert np.isnan(e["specificity"]) and e["precision"] == 1.0
    counts = np.array([[1, 1, 2, 2], [0, 0, 3, 0], [2, 0, 0, 1], [0, 0, 0, 0]])
    got = ce.metrics_from_counts(counts)
    for i, row in enumerate(counts):
        want = ref.metrics(row)
        for k in ce.METRICS:
            assert got[k].dtype == np.float64
            assert got[k][i] == want[k] or (np.isnan(got[k][i]) and np.isnan(want[k])), (i, k)


def test_pair_count_auc_hand_cases():
    p = np.array([0.1, 0.4, 0.35, 0.8], np.float32)
    assert ref.pair_counts(p, [0, 0, 1, 1]) == (3, 0, 2, 2) and ref.auc(p, [0, 0, 1, 1]) == 0.75
    p = np.array([0.5, 0.5, 0.5, 0.2, np.nan], np.float32)
    assert ref.pair_counts(p, [1, 0, 0, 1, 1]) == (0, 2, 2, 2) and ref.auc(p, [1, 0, 0, 1, 1]) == 0.25
    assert ref.pair_counts(p, [1, 0, 0, 1, 1], [2, 3, 0, 1, 7]) == (0, 6, 3, 3)
    assert np.isnan(ref.auc(p, [1, 1, 1, 1, 1]))
    r = np.array([[3, 0, 2, 2], [0, 2, 2, 2], [0, 0, 0, 5], [0, 0, 3, 0]])
    a = ce.auc_from_ranks(r)
    assert a[0] == 0.75 and a[1] == 0.25 and np.isnan(a[2]) and np.isnan(a[3]) and a.dtype == np.float64


def test_pair_count_auc_vs_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.Generator(np.random.PCG64(7))
    for W, levels in ((50, 5), (400, 7), (400, 0), (1000, 64)):
        p = rng.random(W).astype(np.float32) if not levels else (rng.integers(0, levels, W) / levels).astype(np.float32)
        lab = rng.integers(0, 2, W)
        w = rng.integers(0, 4, W)
        assert abs(ref.auc(p, lab) - sk.roc_auc_score(lab, p)) <= 1e-12
        keep = w > 0
        assert abs(ref.auc(p, lab, w) - sk.roc_auc_score(lab[keep], p[keep], sample_weight=w[keep])) <= 1e-12
        fpr, tpr, _ = sk.roc_curve(lab, p)
        assert abs(ref.auc(p, lab) - sk.auc(fpr, tpr)) <= 1e-12


# ------------------------------------------------------------------ properties
def _random_case(seed, n_r=(0, 1, 7, 40, 3)):
    rng = np.random.Generator(np.random.PCG64(seed))
    base = np.concatenate([[0], np.cumsum(n_r)])
    p = (rng.integers(0, 9, base[-1]) / 8).astype(np.float32)
    p[rng.random(base[-1]) < 0.05] = np.nan
    gaps = rng.random(base[-1]) < 0.2
    o = np.concatenate([np.cumsum(1 + gaps[a:b]) for a, b in zip(base[:-1], base[1:])] + [np.zeros(0)]).astype(np.int32)
    return p, base, o


@pytest.mark.parametrize("mode", ["consecutive", "cumulative"])
@pytest.mark.parametrize("strike", [1, 2, 3])
def test_monotone_in_the_threshold(mode, strike):
    thr = np.linspace(0, 1, 17).astype(np.float32)
    for seed in range(3):
        p, base, o = _random_case(seed)
        for ordn in (None, o):
            first = ref.alarm_sweep(p, base, thr, strike, mode, ordn).astype(np.int64)
            alarm = first >= 0
            assert (alarm[:, 1:] <= alarm[:, :-1]).all()             # the alarm set shrinks
            both = alarm[:, 1:]                                      # then the earlier one fired too
            assert (first[:, 1:][both] >= first[:, :-1][both]).all()  # and no later than this one
            assert not alarm[:, -1].any()                            # nothing exceeds 1.0
            rc = ref.recording_counts(first, np.arange(len(base) - 1) % 2, np.diff(base))
            assert (np.diff(rc[:, 1]) <= 0).all()                    # so the false-positive count cannot rise


def test_strike_one_is_alike_in_both_modes():
    thr = np.linspace(0, 1, 9).astype(np.float32)
    for seed in range(3):
        p, base, o = _random_case(seed)
        a = ref.alarm_sweep(p, base, thr, 1, "consecutive", o)
        assert np.array_equal(a, ref.alarm_sweep(p, base, thr, 1, "cumulative"))
        assert np.array_equal(a, ref.alarm_sweep(p, base, thr, 1, "consecutive"))


# ------------------------------------------------------------------ host helpers
def test_multiplicities_repeat_for_a_seed():
    m = ce.multiplicities(13, 50, seed=3)
    assert m.shape == (50, 13) and m.dtype == np.int32 and (m.sum(1) == 13).all() and m.min() == 0
    assert np.array_equal(m, ce.multiplicities(13, 50, seed=3)) and np.array_equal(m, ref.multiplicities(13, 50, 3))
    assert not np.array_equal(m, ce.multiplicities(13, 50, seed=4))
    assert ce.multiplicities(0, 5).shape == (5, 0) and ce.multiplicities(4, 0).shape == (0, 4)


def test_window_ordinals_and_defaults():
    rec_all = np.array([0, 0, 0, 2, 2, 2, 2, 3])
    kept = np.array([0, 2, 3, 4, 6, 7])
    assert ce.window_ordinals(rec_all, kept).tolist() == [0, 2, 0, 1, 3, 0] == ref.ordinals(rec_all, kept).tolist()
    assert ce.window_ordinals(np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0,)
    t = ce.default_thresholds()
    assert t.dtype == np.float32 and t.shape == (401,) and t[0] == 0 and t[-1] == 1 and (np.diff(t) > 0).all()
    assert ce.COLUMNS == ("guid", "epoch_num", "prob_class_0", "prob_class_1", "predicted_class", "true_label")


def test_check_args_accepts_and_normalises():
    lab, strike, mode, tf, th, thr, bins, nb, seed = ce.check_args(3, [0, 1, 1], 2, "cumulative", 0.25, 0.5, [0, 0.5, 1],
                                                                   [0, 10, 20], 5, 1)
    assert lab.dtype == np.uint8 and lab.tolist() == [0, 1, 1] and (strike, mode, tf, th, nb, seed) == (2, 1, 0.25, 0.5,
                                                                                                       5, 1)
    assert thr.dtype == np.float32 and thr.tolist() == [0, 0.5, 1] and bins.dtype == np.float64
    assert ce.check_args(2, np.array([True, False]))[0].tolist() == [1, 0]
    assert ce.check_args(0)[5].shape == (401,)


@pytest.mark.parametrize("kw", [
    dict(labels=[0, 1]), dict(labels=[[0, 1, 1]]), dict(labels=[0, 1, 2]), dict(labels=[0.5, 0, 1]),
    dict(strike=0), dict(strike=1.5), dict(strike=True), dict(mode="either"), dict(mode=0),
    dict(target_fpr=0.0), dict(target_fpr=1.0), dict(target_fpr=float("nan")),
    dict(threshold=float("nan")), dict(threshold=float("inf")),
    dict(thresholds=[]), dict(thresholds=[[0.1, 0.2]]), dict(thresholds=[0.1, float("nan")]),
    dict(thresholds=[0.5, 0.4]), dict(thresholds=[0.1, float("inf")]),
    dict(epoch_bins=[1.0]), dict(epoch_bins=[0, 0]), dict(epoch_bins=[2, 1]), dict(epoch_bins=[[0, 1]]),
    dict(epoch_bins=[0, float("nan")]), dict(n_boot=-1), dict(n_boot=2.5), dict(seed=-1),
])
def test_check_args_refuses(kw):
    with pytest.raises(ValueError):
        ce.check_args(3, **kw)


# ------------------------------------------------------------------ the C ABI, before any device work
def test_entry_points_refuse_bad_sizes_and_null_pointers():
    """VT_ERR_ARG (ValueError) for a bad size or a null pointer, VT_OK for an empty output: both are
    decided before any device work, so neither needs a GPU."""
    from vaeteb import _lib
    lib = _lib.lib()
    assert lib.fns["vt_cls_scan_span"]() >= 256 and lib.fns["vt_cls_stage_chunk"]() >= 256
    one = 4096                                                        # stands for a non-null pointer; never read
    bad = [
        ("vt_cls_alarm_sweep", (one, 4, one, 2, None, one, 3, 0, 0, one, None)),          # strike 0
        ("vt_cls_alarm_sweep", (one, 4, one, 2, None, one, 3, 2, 2, one, None)),          # mode 2
        ("vt_cls_alarm_sweep", (one, -1, one, 2, None, one, 3, 2, 0, one, None)),         # W < 0
        ("vt_cls_alarm_sweep", (one, 2 ** 31, one, 2, None, one, 3, 2, 0, one, None)),    # W too large
        ("vt_cls_alarm_sweep", (None, 4, one, 2, None, one, 3, 2, 0, one, None)),         # p null
        ("vt_cls_alarm_sweep", (one, 4, None, 2, None, one, 3, 2, 0, one, None)),         # rec_base null
        ("vt_cls_alarm_sweep", (one, 4, one, 2, None, None, 3, 2, 0, one, None)),         # thr null
        ("vt_cls_alarm_sweep", (one, 4, one, 2, None, one, 3, 2, 0, None, None)),         # first null
        ("vt_cls_confusion", (one, one, None, 4, -1, one, 3, one, None)),                 # G < 0
        ("vt_cls_confusion", (one, one, None, 4, 65536, one, 3, one, None)),              # G too large
        ("vt_cls_confusion", (one, None, None, 4, 1, one, 3, one, None)),                 # label null
        ("vt_cls_confusion", (one, one, None, 4, 1, None, 3, one, None)),                 # thr null
        ("vt_cls_confusion", (one, one, None, 4, 1, one, 3, None, None)),                 # counts null
        ("vt_cls_auc_ranks", (one, one, -1, one, None, None, 1, None, 1, 0, one, None)),  # W < 0
        ("vt_cls_auc_ranks", (one, None, 4, one, None, None, 1, None, 1, 0, one, None)),  # order null
        ("vt_cls_auc_ranks", (one, one, 4, one, None, None, 1, one, 1, 3, one, None)),    # mult without rec
        ("vt_cls_auc_ranks", (one, one, 4, one, None, None, 1, None, 1, 0, None, None)),  # out null
        ("vt_cls_auc_ranks", (one, one, 4, one, None, None, 1, None, -1, 0, one, None)),  # Bt < 0
    ]
    for name, args in bad:
        with pytest.raises(ValueError):
            _lib.call(name, *args)
    for name, args in [("vt_cls_alarm_sweep", (None, 0, None, 0, None, None, 5, 1, 0, None, None)),      # R = 0
                       ("vt_cls_alarm_sweep", (None, 0, None, 3, None, None, 0, 1, 0, None, None)),      # T = 0
                       ("vt_cls_confusion", (None, None, None, 0, 0, None, 5, None, None)),              # G = 0
                       ("vt_cls_confusion", (None, None, None, 0, 2, None, 0, None, None)),              # T = 0
                       ("vt_cls_auc_ranks", (None, None, 0, None, None, None, 0, None, 1, 0, None, None)),   # G = 0
                       ("vt_cls_auc_ranks", (None, None, 0, None, None, None, 1, None, 0, 0, None, None))]:  # Bt = 0
        assert _lib.call(name, *args) == 0
