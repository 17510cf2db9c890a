"""The classifier-evaluation statistics on the GPU (vaeteb.clseval, csrc/clseval.hip) against the naive
numpy reference (tests/clseval_ref.py).  Every kernel output is an integer table, so every comparison
is np.array_equal; the float64 AUCs and metrics are formed from those integers by the same
expressions on both sides and are compared exactly too.

* vt_cls_alarm_sweep: recordings of 0, 1, 7, 300 and 3 kept windows, p in multiples of 1/8 (so that
  p == thr occurs and must not fire) with a few NaN, T in {1, 65, 401}, strike in {1, 2, 3, 8}, both
  modes, with and without ordinals that hold gaps; a recording of more than two staging chunks with a
  run laid across a chunk border; W = 0.
* vt_cls_confusion: the same p, G in {1, 3} with windows in no group; more windows than one
  workgroup's slab (the atomic path); W = 0.
* vt_cls_auc_ranks: W in {1, 2, 255, 256, 257, 2 span + 3} with p from 5 values (tie groups straddle
  every span border), all p distinct, a single class, multiplicities 0..5, Bt in {1, 7}, G in {1, 3},
  NaN p; W = 0.
* Each kernel twice into buffers holding different garbage: equal bits.
* ClassifierScorer end to end on the fixture shape of tests/test_gpu_timeline.py.
"""
import numpy as np
import pytest
import torch

import clseval_ref as ref

pytestmark = pytest.mark.gpu

N_R = [0, 1, 7, 300, 3]


def _thr(T):
    return {1: np.array([0.5], np.float32), 65: np.linspace(0, 1, 65).astype(np.float32)}.get(
        T, np.linspace(0, 1, 401).astype(np.float32))


def _case(seed, n_r=N_R, nan=0.03):
    """p (W,) in multiples of 1/8 with some NaN, the CSR of the recordings, ordinals with gaps."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = np.concatenate([[0], np.cumsum(n_r)]).astype(np.int64)
    W = int(base[-1])
    p = (rng.integers(0, 9, W) / 8).astype(np.float32)
    p[rng.random(W) < nan] = np.nan
    gaps = rng.random(W) < 0.15
    o = np.concatenate([np.cumsum(1 + gaps[a:b]) for a, b in zip(base[:-1], base[1:])] + [np.zeros(0)])
    return p, base, o.astype(np.int32)


def _garbage(shape, dtype, fill):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


# ------------------------------------------------------------------ alarm sweep
@pytest.mark.parametrize("strike", [1, 2, 3, 8])
@pytest.mark.parametrize("T", [1, 65, 401])
def test_alarm_sweep_vs_reference(T, strike):
    from vaeteb import clseval as ce
    p, base, o = _case(100 + T)
    thr = _thr(T)
    assert np.isnan(p).any() and (p[:, None] == thr[None, :]).any() and (np.diff(o) > 1).any()
    pd = torch.from_numpy(p).cuda()
    some = False
    for mode in ("consecutive", "cumulative"):
        for ordn in (None, o):
            got = ce.alarm_sweep(pd, base, thr, strike, mode, ordn)
            assert got.dtype == torch.int32 and got.shape == (len(N_R), T)
            want = ref.alarm_sweep(p, base, thr, strike, mode, ordn)
            assert np.array_equal(got.cpu().numpy(), want), (mode, ordn is not None)
            assert (want[0] == -1).all()                              # the recording without windows
            some |= bool((want >= 0).any())
            if mode == "consecutive" and ordn is not None and strike in (2, 3) and T > 1:
                assert not np.array_equal(want, ref.alarm_sweep(p, base, thr, strike, mode))   # the gaps matter
    assert some


def test_alarm_sweep_recording_longer_than_the_staging_chunk():
    from vaeteb import _lib
    from vaeteb import clseval as ce
    chunk = _lib.lib().fns["vt_cls_stage_chunk"]()
    n_r = [3, 2 * chunk + 5, 2]
    base = np.concatenate([[0], np.cumsum(n_r)]).astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(9))
    thr = _thr(65)
    # (a) eight firing windows laid across the first chunk border of the long recording, nothing else
    p = np.zeros(base[-1], np.float32)
    p[3 + chunk - 3:3 + chunk + 5] = 1.0
    pd = torch.from_numpy(p).cuda()
    for strike, mode, at in ((8, "consecutive", chunk + 4), (3, "consecutive", chunk - 1), (8, "cumulative", chunk + 4),
                             (5, "cumulative", chunk + 1), (9, "consecutive", -1)):
        got = ce.alarm_sweep(pd, base, thr, strike, mode).cpu().numpy()
        assert np.array_equal(got, ref.alarm_sweep(p, base, thr, strike, mode)), (strike, mode)
        assert got[1, 0] == at and got[1, -1] == -1 and (got[0] == -1).all()
    # (b) sparse random firing: the first run of 8 (or the 40th firing window) comes chunks later
    p = np.where(rng.random(base[-1]) < 0.4, 1.0, 0.25).astype(np.float32)
    o = np.concatenate([np.arange(n) + (np.arange(n) >= n // 2) for n in n_r]).astype(np.int32)
    pd = torch.from_numpy(p).cuda()
    late = False
    for strike, mode in ((8, "consecutive"), (40, "cumulative"), (700, "cumulative")):
        for ordn in (None, o):
            got = ce.alarm_sweep(pd, base, thr, strike, mode, ordn).cpu().numpy()
            assert np.array_equal(got, ref.alarm_sweep(p, base, thr, strike, mode, ordn)), (strike, mode)
            late |= bool((got[1] >= chunk).any())
    assert late


def test_alarm_sweep_without_windows():
    from vaeteb import clseval as ce
    first = ce.alarm_sweep(torch.zeros(0, device="cuda"), np.zeros(4, np.int64), _thr(65), 2, "consecutive",
                           out=_garbage((3, 65), torch.int32, 77))
    assert (first == -1).all()
    assert ce.alarm_sweep(torch.zeros(0, device="cuda"), np.zeros(1, np.int64), _thr(65)).shape == (0, 65)
    with pytest.raises(ValueError):
        ce.alarm_sweep(torch.zeros(4, device="cuda"), np.array([0, 3]), _thr(1))       # the CSR stops short
    with pytest.raises(ValueError):
        ce.alarm_sweep(torch.zeros(4, device="cuda"), np.array([0, 4]), _thr(1), ordinal=np.zeros(3, np.int32))


# ------------------------------------------------------------------ confusion
def _groups(rng, W, G):
    return rng.integers(-1, G + 1, W).astype(np.int32)               # -1 and G: in no group


@pytest.mark.parametrize("T", [1, 65, 401])
@pytest.mark.parametrize("G", [1, 3])
def test_confusion_vs_reference(G, T):
    from vaeteb import clseval as ce
    p, base, _ = _case(200 + T)
    rng = np.random.Generator(np.random.PCG64(G))
    lab = rng.integers(0, 2, len(p)).astype(np.uint8)
    grp = _groups(rng, len(p), G)
    thr = _thr(T)
    pd = torch.from_numpy(p).cuda()
    got = ce.confusion(pd, lab, thr, grp, G)
    assert got.dtype == torch.int32 and got.shape == (G, T, 4)
    want = ref.confusion(p, lab, thr, grp, G)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.sum(2).max() < len(p) and (want.sum(2)[:, 0] == want.sum(2)[:, -1]).all()   # some windows in no group
    if G == 1:
        assert np.array_equal(ce.confusion(pd, lab, thr).cpu().numpy(), ref.confusion(p, lab, thr))


def test_confusion_more_windows_than_a_slab_and_none():
    from vaeteb import clseval as ce
    n = 2 * 8192 + 7                                                  # three slabs: integer atomics into zeros
    p, _, _ = _case(5, [n])
    rng = np.random.Generator(np.random.PCG64(6))
    lab = rng.integers(0, 2, n).astype(np.uint8)
    grp = _groups(rng, n, 3)
    thr = _thr(65)
    got = ce.confusion(torch.from_numpy(p).cuda(), lab, thr, grp, 3, out=_garbage((3, 65, 4), torch.int32, -5))
    assert np.array_equal(got.cpu().numpy(), ref.confusion(p, lab, thr, grp, 3))
    none = ce.confusion(torch.zeros(0, device="cuda"), np.zeros(0, np.uint8), thr, None, 2,
                        out=_garbage((2, 65, 4), torch.int32, 9))
    assert (none == 0).all()


# ------------------------------------------------------------------ AUC
def _span():
    from vaeteb import _lib
    return _lib.lib().fns["vt_cls_scan_span"]()


def _auc_case(seed, W, distinct=False, nan=2, R=9):
    """nan: how many p are NaN (they sort last: two leave the last span border inside the top tie group)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = rng.permutation(W).astype(np.float32) / max(W, 1) if distinct else (rng.integers(0, 5, W) / 4).astype(np.float32)
    if W > 2 and nan:
        p[rng.choice(W, nan, replace=False)] = np.nan
    lab = rng.integers(0, 2, W).astype(np.uint8)
    rec = np.sort(rng.integers(0, R, W)).astype(np.int32)
    return p, lab, rec


@pytest.mark.parametrize("Bt", [1, 7])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("W", [1, 2, 255, 256, 257, "2span+3"])
def test_auc_ranks_vs_pair_count(W, G, Bt):
    from vaeteb import clseval as ce
    span = _span()
    W = 2 * span + 3 if W == "2span+3" else W
    R = 9
    p, lab, rec = _auc_case(300 + W, W, R=R)
    rng = np.random.Generator(np.random.PCG64(W + G + Bt))
    grp = _groups(rng, W, G) if G > 1 else None
    mult = rng.integers(0, 6, (Bt, R)).astype(np.int32)
    mult[0, 0] = 0
    pd = torch.from_numpy(p).cuda()
    got = ce.auc_ranks(pd, lab, rec=rec, group=grp, G=G, mult=mult)
    assert got.dtype == torch.int64 and got.shape == (Bt, G, 4)
    want = ref.auc_ranks(p, lab, rec, grp, G, mult)
    assert np.array_equal(got.cpu().numpy(), want)
    if W > 2 * span:                                                  # a tie group lies across each span border
        ps = np.sort(p)
        assert ps[span - 1] == ps[span] and ps[2 * span - 1] == ps[2 * span] and want[..., 1].max() > 0
    if Bt == 1:                                                       # without multiplicities: every weight 1
        assert np.array_equal(ce.auc_ranks(pd, lab, group=grp, G=G).cpu().numpy(), ref.auc_ranks(p, lab, None, grp, G))
    a, b = ce.auc_from_ranks(got.cpu().numpy()), ce.auc_from_ranks(want)
    assert np.array_equal(a, b, equal_nan=True)


def test_auc_ranks_distinct_single_class_and_none():
    from vaeteb import clseval as ce
    span = _span()
    W = span + 300
    p, lab, rec = _auc_case(1, W, distinct=True, nan=0)
    got = ce.auc_ranks(torch.from_numpy(p).cuda(), lab).cpu().numpy()
    assert np.array_equal(got, ref.auc_ranks(p, lab)) and got[0, 0, 1] == 0           # no ties at all
    assert ce.auc_from_ranks(got)[0, 0] == ref.auc(p, lab)
    one = np.ones(W, np.uint8)
    got = ce.auc_ranks(torch.from_numpy(p).cuda(), one).cpu().numpy()
    assert got[0, 0].tolist() == [0, 0, W, 0] and np.isnan(ce.auc_from_ranks(got)[0, 0])
    got = ce.auc_ranks(torch.from_numpy(p).cuda(), 1 - one).cpu().numpy()
    assert got[0, 0].tolist() == [0, 0, 0, W]
    none = ce.auc_ranks(torch.zeros(0, device="cuda"), np.zeros(0, np.uint8), G=2, out=_garbage((1, 2, 4), torch.int64, 3))
    assert (none == 0).all()
    # -0.0 and 0.0 are one tie group (==), whatever their bits
    pz = np.array([-0.0, 0.0, 0.0, -0.0, 0.5], np.float32)
    lz = np.array([1, 0, 1, 0, 0], np.uint8)
    assert ce.auc_ranks(torch.from_numpy(pz).cuda(), lz).cpu().numpy()[0, 0].tolist() == [0, 4, 2, 3]


# ------------------------------------------------------------------ determinism
def test_two_runs_into_different_garbage_give_equal_bits():
    from vaeteb import clseval as ce
    span = _span()
    p, base, o = _case(7, [0, 1, 7, 2500, 3])
    W = len(p)
    rng = np.random.Generator(np.random.PCG64(8))
    lab, grp = rng.integers(0, 2, W).astype(np.uint8), _groups(rng, W, 3)
    rec = np.repeat(np.arange(5), np.diff(base)).astype(np.int32)
    mult = rng.integers(0, 6, (7, 5)).astype(np.int32)
    thr = _thr(65)
    pd = torch.from_numpy(p).cuda()
    assert W > 2 * span
    runs = []
    for fill in (0x5A5A5A5A, -1):
        f = ce.alarm_sweep(pd, base, thr, 3, "consecutive", o, out=_garbage((5, 65), torch.int32, fill & 0x7FFFFFFF))
        c = ce.confusion(pd, lab, thr, grp, 3, out=_garbage((3, 65, 4), torch.int32, fill & 0x7FFFFFFF))
        r = ce.auc_ranks(pd, lab, rec=rec, group=grp, G=3, mult=mult, out=_garbage((7, 3, 4), torch.int64, fill))
        runs.append((f.clone(), c.clone(), r.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert np.array_equal(runs[0][0].cpu().numpy(), ref.alarm_sweep(p, base, thr, 3, "consecutive", o))
    assert np.array_equal(runs[0][1].cpu().numpy(), ref.confusion(p, lab, thr, grp, 3))


# ------------------------------------------------------------------ end to end
N, TRIM = 2048, 8
REC_LENGTHS = [2048, 5120, 5120, 1500]
LABELS = [0, 1, 1, 0]


def _recordings():
    """The four recordings of tests/test_gpu_timeline.py with labels: recording 1 holds a constant FHR
    run inside its two middle windows only (the gate drops them), recording 3 is shorter than a window."""
    from vaeteb.windows import Recording
    rng = np.random.Generator(np.random.PCG64(31415))
    out = []
    for i, L in enumerate(REC_LENGTHS):
        t = np.arange(L) / 4.0
        fhr = 140 + 8 * np.sin(2 * np.pi * 0.011 * t + i) + 3 * np.sin(2 * np.pi * 0.17 * t) + 1.5 * rng.standard_normal(L)
        up = 10 + 40 * np.exp(-((t % 180.0) - 90.0) ** 2 / (2 * 22.0 ** 2)) + 0.5 * rng.standard_normal(L)
        x = np.stack([fhr, up]).astype(np.float32)
        if i == 1:
            x[0, 2300:2700] = x[0, 2300]
        out.append(Recording(x, f"rec_{i}", domain_start=1000.0 * (i + 1), bg_label=bool(LABELS[i])))
    return out


@pytest.fixture(scope="module")
def e2e():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from golden_util import det_fill_
    from vaeteb.classifier import SeqVaeTebClassifier
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.windows import QualityGate, RecordingWindows
    fe = FrontEnd(FrontEndPlan(6, 1, 16, N, device="cuda"), load_stats(6, 1, 16, 4096), trim=TRIM)
    assert fe.S_out == 112
    m = det_fill_(SeqVaeTebClassifier(sequence_length=112, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                                      cross_phase_channels=fe.C_x)).cuda()
    recs = _recordings()
    big = 10 ** 9
    gate = QualityGate(max_flat_fhr=300, max_flat_up=big, total_flat_fhr=big, total_flat_up=big)
    rw = RecordingWindows(recs, N=N, overlap=0.5, gate=gate, batch_size=256, device="cuda")
    m.train()
    torch.cuda.synchronize()
    rng0 = torch.cuda.get_rng_state()
    ev = m.evaluate_recordings(fe, rw)
    torch.cuda.synchronize()
    rng1 = torch.cuda.get_rng_state()
    return dict(fe=fe, m=m, rw=rw, ev=ev, rng=(rng0, rng1), training_after=m.training)


def _check_against_reference(ev, rw, strike, mode, target_fpr, n_boot, seed, bins=None, threshold=None,
                             break_on_gap=True):
    """Everything the evaluation derives from its own p, against the numpy reference applied to that p."""
    from vaeteb import clseval as ce
    p = ev.windows.p.cpu().numpy()
    rec, epoch = ev.windows.rec, ev.windows.epoch
    R = len(REC_LENGTHS)
    n_r = np.bincount(rec, minlength=R)
    base = np.concatenate([[0], np.cumsum(n_r)])
    labels = np.asarray(LABELS)
    thr = np.linspace(0, 1, 401).astype(np.float32)
    o = ref.ordinals(rw.rec, rw.kept) if break_on_gap else None
    assert np.array_equal(ev.thresholds.cpu().numpy(), thr)
    first = ref.alarm_sweep(p, base, thr, strike, mode, o)
    assert np.array_equal(ev.first.cpu().numpy(), first)
    rc = ref.recording_counts(first, labels, n_r)
    assert np.array_equal(ev.rec_counts.cpu().numpy(), rc)
    if threshold is None:
        ti, th = ref.select_threshold(thr, rc, target_fpr)
        assert ev.threshold == th and ev.threshold_index == ti
        col = first[:, ti]
    else:
        assert ev.threshold == threshold
        col = ref.alarm_sweep(p, base, np.array([threshold], np.float32), strike, mode, o)[:, 0]
    assert np.array_equal(ev.alarm, col >= 0) and ev.alarm.dtype == np.bool_
    want_epoch = np.array([epoch[base[r] + col[r]] if col[r] >= 0 else np.nan for r in range(R)])
    assert np.array_equal(ev.alarm_epoch, want_epoch, equal_nan=True) and ev.alarm_epoch.dtype == np.float64
    wlab = labels[rec].astype(np.uint8)
    assert np.array_equal(ev.windows.label, wlab)
    G = 1 if bins is None else len(bins) - 1
    grp = None if bins is None else np.digitize(epoch, bins) - 1
    counts = ref.confusion(p, wlab, thr, grp, G)
    assert np.array_equal(ev.counts.cpu().numpy(), counts)
    got = ev.metrics()
    at = counts[:, int(np.searchsorted(thr, np.float32(ev.threshold)))] if np.float32(ev.threshold) in thr else \
        ref.confusion(p, wlab, np.array([ev.threshold], np.float32), grp, G)[:, 0]
    assert np.array_equal(got["counts"], at)
    for g in range(G):
        want = ref.metrics(at[g])
        for k in ce.METRICS:
            assert got[k][g] == want[k] or (np.isnan(got[k][g]) and np.isnan(want[k])), (g, k)
    a = ref.auc(p, wlab)
    assert ev.auc == a or (np.isnan(ev.auc) and np.isnan(a))
    ag = np.array([ref.auc(p, wlab, None if grp is None else (grp == g).astype(np.int64)) for g in range(G)])
    assert np.array_equal(ev.auc_groups, ag, equal_nan=True)
    mult = ref.multiplicities(R, n_boot, seed)
    boot = np.array([ref.auc(p, wlab, mult[b][rec]) for b in range(n_boot)])
    assert ev.auc_boot.dtype == np.float64 and np.array_equal(ev.auc_boot, boot, equal_nan=True)
    valid = ~np.isnan(boot)
    assert ev.n_valid == int(valid.sum())
    if valid.any():
        assert ev.auc_ci == tuple(np.percentile(boot[valid], [2.5, 97.5]).tolist())
    return p


def test_end_to_end_default_evaluation(e2e):
    from vaeteb.timeline import stitch
    ev, rw, fe, m = e2e["ev"], e2e["rw"], e2e["fe"], e2e["m"]
    assert rw.rec[rw.kept].tolist() == [0, 1, 1, 2, 2, 2, 2] and ref.ordinals(rw.rec, rw.kept).tolist() == [0, 0, 3, 0,
                                                                                                           1, 2, 3]
    assert e2e["training_after"] is False and torch.equal(e2e["rng"][0], e2e["rng"][1])
    # (a) the window probabilities are the model's own, on the same batches, on the posterior mean
    w0 = 0
    with torch.no_grad():
        for b in rw:
            f = fe(b.x)
            nb = b.x.shape[0]
            out = m(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], eps=torch.zeros(nb, 112, 32, device="cuda"))
            assert torch.equal(ev.windows.p[w0:w0 + nb], out["probabilities"][:, 1])
            assert torch.equal(ev.windows.p0[w0:w0 + nb], out["probabilities"][:, 0])
            w0 += nb
    assert w0 == 7 and ev.windows.p.dtype == torch.float32 and ev.windows.p.shape == (7,)
    # (b) the statistics against the reference applied to the returned p
    p = _check_against_reference(ev, rw, 2, "consecutive", 0.3, 1000, 0)
    assert np.isfinite(p).all() and ev.first.shape == (4, 401) and ev.counts.shape == (1, 401, 4)
    # recording 1's two kept windows are not neighbours: with strike 2 the gap keeps it silent
    assert (ev.first[1] == -1).all() and (ev.first[0] == -1).all()
    # (c) prob[i] is the stitch of the broadcast p; the recording without windows is NaN throughout
    so, _ = ev.layout.window_offsets(ev.windows.rec, ev.windows.start, fe)
    want, count = stitch(ev.windows.p[:, None].expand(7, 112).contiguous(), so, ev.layout.n_steps)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(torch.cat(ev.prob)), bits(want)) and torch.equal(torch.cat(ev.coverage_steps), count)
    assert [len(t) for t in ev.prob] == [128, 320, 320, 93]
    assert ev.unscored == [3] and torch.isnan(ev.prob[3]).all() and ev.coverage_steps[3].max().item() == 0
    assert (ev.first[3] == -1).all() and not ev.alarm[3] and np.isnan(ev.alarm_epoch[3])
    assert torch.isnan(ev.prob[1][120:200]).all() and ev.coverage_steps[2].max().item() == 2
    one = ev.coverage_steps[2] == 1
    assert one.any() and torch.equal(ev.prob[0][TRIM:120], ev.windows.p[0].expand(112))
    # (d) rows: the reference's CSV columns
    rows = ev.rows()
    pr = ev.windows.p.cpu().numpy()
    assert len(rows) == 7 and list(rows[0]) == ["guid", "epoch_num", "prob_class_0", "prob_class_1", "predicted_class",
                                                "true_label"]
    assert [r["guid"] for r in rows] == ["rec_0", "rec_1", "rec_1"] + ["rec_2"] * 4
    assert [r["true_label"] for r in rows] == [0, 1, 1, 1, 1, 1, 1]
    assert [r["epoch_num"] for r in rows] == [1000.0, 2000.0, 2000.0 + 3072, 3000.0, 3000.0 + 1024, 3000.0 + 2048,
                                              3000.0 + 3072]
    assert all(r["prob_class_1"] == float(pr[i]) and r["predicted_class"] == int(pr[i] > np.float32(ev.threshold))
               for i, r in enumerate(rows))
    assert m.__dict__["_classifier_scorer"].frontend is fe              # kept for the next call


def test_end_to_end_other_settings(e2e):
    rw, fe, m = e2e["rw"], e2e["fe"], e2e["m"]
    # epochs 1000 | 2000 | 3000 4024 | 5072 5048 6072 | none: the first window is in no group, the last group empty
    bins = [1500.0, 2500.0, 4500.0, 7000.0, 9000.0]
    ev = m.evaluate_recordings(fe, rw, strike=1, mode="cumulative", target_fpr=0.5, epoch_bins=bins, n_boot=40, seed=5)
    assert torch.equal(ev.windows.p, e2e["ev"].windows.p)             # scoring does not depend on the settings
    _check_against_reference(ev, rw, 1, "cumulative", 0.5, 40, 5, bins=bins)
    assert ev.counts.shape == (4, 401, 4) and ev.counts[3].sum().item() == 0 and ev.auc_groups.shape == (4,)
    # an operating point off the grid, no gap rule, explicit labels equal to the default
    th = 0.50125
    ev = m.evaluate_recordings(fe, rw, labels=LABELS, strike=2, threshold=th, break_on_gap=False, n_boot=0)
    _check_against_reference(ev, rw, 2, "consecutive", 0.3, 0, 0, threshold=th, break_on_gap=False)
    assert ev.threshold_index is None and ev.auc_boot.shape == (0,) and ev.n_valid == 0 and np.isnan(ev.auc_ci[0])
    # sampling draws noise: the random stream moves
    torch.cuda.synchronize()
    before = torch.cuda.get_rng_state()
    ev = m.evaluate_recordings(fe, rw, sample=True, n_boot=0)
    torch.cuda.synchronize()
    assert not torch.equal(before, torch.cuda.get_rng_state()) and torch.isfinite(ev.windows.p).all()
    # refused on the host, before any launch
    with pytest.raises(ValueError):
        m.evaluate_recordings(fe, rw, labels=[1, 1, 1, 1])                # no scored negative recording
    with pytest.raises(ValueError):
        m.evaluate_recordings(fe, rw, labels=[1, 1, 1, 0])                # the only negative has no kept window
    with pytest.raises(ValueError):
        m.evaluate_recordings(fe, rw, strike=0)
