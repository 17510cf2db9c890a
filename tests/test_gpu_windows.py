"""vaeteb.windows on the device: vt_window_flat_stats against the reference's recorded
find_flat_regions results (tests/golden/flat_regions_cases.npz) and against the numpy
restatement of tests/windows_util.py (pinned to that fixture by tests/test_windows_cpu.py),
vt_window_gather against slicing, the QualityGate thresholds, and recordings -> windows ->
gate -> FrontEnd.raw -> a file CombinedHDF5Dataset loads.  Everything is integer or bit
equality: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from windows_util import fixture_cases, flat_stats_np

pytestmark = pytest.mark.gpu

JUNK = np.float32(7.125)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _walk(rng, n, start=100.0):
    """n float32 samples, multiples of 0.25, no two consecutive ones equal (nowhere flat)."""
    steps = rng.choice(np.array([-0.5, -0.25, 0.25, 0.5]), size=n)
    return (start + np.cumsum(steps)).astype(np.float32)


def _pack(rows):
    """One buffer holding the rows with neighbour bait: the element just before a row equals
    the row's first sample and the element just after equals its last, so a kernel that looks
    one element outside a row sees a flat difference there.  Row 0 starts at element 0, the
    last row ends at the buffer's last element, and row k starts at an offset = k (mod 4)."""
    parts, offs, pos = [], [], 0
    for k, r in enumerate(rows):
        r = np.asarray(r, np.float32)
        if k:
            pad = (k % 4 - (pos + 1)) % 4
            parts += [np.full(pad, JUNK, np.float32), r[:1]]
            pos += pad + 1
        offs.append(pos)
        parts.append(r)
        pos += len(r)
        if k < len(rows) - 1:
            parts.append(r[-1:])
            pos += 1
    return np.concatenate(parts), np.array(offs, np.int64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_fixture_cases_equal_reference():
    _need_gpu()
    from vaeteb.windows import flat_stats
    cases = fixture_cases()
    base, offs = _pack([s for s, *_ in cases][::6])          # the 6 parameter sets share a signal
    dev = torch.from_numpy(base).cuda()
    got = torch.cat([flat_stats(dev, offs[i // 6:i // 6 + 1], len(s), tol, ml)
                     for i, (s, tol, ml, _) in enumerate(cases)]).cpu().numpy()
    exp = np.stack([e for *_, e in cases])
    bad = np.nonzero((got != exp).any(1))[0]
    assert bad.size == 0, [(len(cases[i][0]), cases[i][1], cases[i][2], got[i], exp[i]) for i in bad[:5]]


def _shape_rows(rng, N, ml):
    """Rows of length N where the kernel can go wrong (each nowhere flat outside what is planted)."""
    rows = [_walk(rng, N)]
    rows.append(np.full(N, 3.25, np.float32))                                # entirely flat
    r = _walk(rng, N); r[max(0, N - 7):] = 55.0; rows.append(r)              # a run that ends at the last sample
    r = _walk(rng, N); r[:min(N, 5)] = 55.0; rows.append(r)                  # and one from the first sample
    if N > 70:
        r = _walk(rng, N); r[60:71] = 55.0; rows.append(r)                   # samples 60..70: across a tile boundary
        r = _walk(rng, N); r[2:63] = 55.0; rows.append(r)                    # ends at lane 62 / 63 / 64
        r = _walk(rng, N); r[2:64] = 55.0; rows.append(r)
        r = _walk(rng, N); r[2:65] = 55.0; rows.append(r)
    if N >= 2 * ml + 3 and ml >= 2:
        r = _walk(rng, N); r[1:ml] = 55.0; r[ml + 1:2 * ml + 1] = 66.0; rows.append(r)   # ml - 1 and ml samples
    if N >= 12:
        r = _walk(rng, N); r[1:11] = 55.0; r[5] = np.nan; rows.append(r)     # NaN inside a run
        r = _walk(rng, N); r[1:11] = 55.0; r[5] = np.inf; rows.append(r)
        r = _walk(rng, N); r[1:11] = np.inf; rows.append(r)                  # inf - inf: not flat
    if N == 5760:
        r = _walk(rng, N); r[100:581] = 55.0; r[1000:2201] = 66.0; r[5000:] = 77.0; rows.append(r)
    return rows


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 128, 129, 5760])
def test_shapes_against_restatement(N):
    _need_gpu()
    from vaeteb.windows import flat_stats
    res = {}
    for ml in (1, 2, 20):
        rows = _shape_rows(np.random.default_rng(N), N, 20)   # the same rows for every min_length
        base, offs = _pack(rows)
        got = flat_stats(torch.from_numpy(base).cuda(), offs, N, 1e-9, ml).cpu().numpy()
        exp = np.array([flat_stats_np(r, 1e-9, ml) for r in rows])
        assert (got == exp).all(), (N, ml, got.tolist(), exp.tolist())
        res[ml] = got
    assert (res[1] == res[2]).all()                            # a region has at least 2 samples
    flat = res[1][1]
    assert flat.tolist() == ([N, N, 1] if N >= 2 else [0, 0, 0])
    if N >= 20:
        assert res[20][1].tolist() == [N, N, 1]


@pytest.mark.parametrize("rows", [1, 5, 7])
def test_overlapping_rows_and_odd_offsets(rows):
    _need_gpu()
    from vaeteb.windows import flat_stats, gather
    N, hop = 129, 65                                           # offsets 0, 65, 130, 195, ... = 0, 1, 2, 3 (mod 4)
    rng = np.random.default_rng(rows)
    x = _walk(rng, hop * (rows - 1) + N)
    for a in range(20, len(x) - 30, 90):
        x[a:a + 25] = 55.0                                     # runs that the overlapping rows share and cut
    offs = np.arange(rows, dtype=np.int64) * hop
    assert offs[-1] + N == len(x)
    dev = torch.from_numpy(x).cuda()
    for ml in (1, 20):
        got = flat_stats(dev, offs, N, 1e-9, ml).cpu().numpy()
        exp = np.array([flat_stats_np(x[o:o + N], 1e-9, ml) for o in offs])
        assert (got == exp).all(), (ml, got.tolist(), exp.tolist())
    # offsets given as a device tensor take the same path
    got = flat_stats(dev, torch.from_numpy(offs).cuda(), N, 1e-9, 1).cpu().numpy()
    assert (got == np.array([flat_stats_np(x[o:o + N], 1e-9, 1) for o in offs])).all()
    assert (_bits(gather(dev, offs, N).cpu().numpy()) == _bits(np.stack([x[o:o + N] for o in offs]))).all()


@pytest.mark.parametrize("N", [1, 2, 64, 65, 257])
def test_neighbour_bait(N):
    """Rows that are nowhere flat, each with a copy of its first sample just before it and of
    its last sample just after it: with min_length 1 the answer is all zeros, and one look
    outside a row makes a region of 2 samples."""
    _need_gpu()
    from vaeteb.windows import flat_stats
    rng = np.random.default_rng(100 + N)
    rows = [_walk(rng, N, 100.0 + 10 * k) for k in range(7)]
    base, offs = _pack(rows)
    assert offs[0] == 0 and offs[-1] + N == len(base)
    assert sorted(set((offs % 4).tolist())) == [0, 1, 2, 3]
    for k in range(1, 7):
        assert base[offs[k] - 1] == rows[k][0] and base[offs[k - 1] + N] == rows[k - 1][-1]
    got = flat_stats(torch.from_numpy(base).cuda(), offs, N, 1e-9, 1).cpu().numpy()
    assert (got == 0).all(), got.tolist()
    # with a run inside, still only that run
    if N >= 64:
        for r in rows:
            r[10:40] = 55.0
        base, offs = _pack(rows)
        got = flat_stats(torch.from_numpy(base).cuda(), offs, N, 1e-9, 1).cpu().numpy()
        assert (got == np.array([30, 30, 1])).all(), got.tolist()


@pytest.mark.parametrize("N,aligned", [(1, False), (3, False), (64, True), (64, False), (1030, True), (1030, False),
                                       (5760, True), (5760, False)])
def test_gather_is_bit_exact(N, aligned):
    _need_gpu()
    from vaeteb.windows import gather
    rng = np.random.default_rng(N)
    rows = 7
    span = (N + 3) // 4 * 4 + 8
    base = rng.integers(0, 2 ** 32, size=rows * span, dtype=np.uint32).view(np.float32)   # any bits, NaN payloads too
    offs = np.arange(rows, dtype=np.int64) * span + (0 if aligned else np.arange(rows) % 4)
    offs[-1] = len(base) - N                                   # the last row ends at the buffer's last element
    offs = offs[[3, 0, 6, 1, 5, 2, 4]]                         # any order
    dev = torch.from_numpy(base).cuda()
    got = gather(dev, offs, N)
    assert got.shape == (rows, N) and got.dtype == torch.float32
    exp = torch.stack([dev[o:o + N] for o in offs.tolist()])   # torch slicing on the device
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))
    assert (got.cpu().numpy().view(np.int32) == np.stack([base[o:o + N] for o in offs]).view(np.int32)).all()


def test_offsets_are_bounds_checked_on_the_host():
    _need_gpu()
    from vaeteb.windows import flat_stats, gather
    dev = torch.zeros(100, device="cuda")
    for fn in (lambda o: flat_stats(dev, o, 64), lambda o: gather(dev, o, 64)):
        with pytest.raises(ValueError):
            fn(np.array([37]))                                 # 37 + 64 > 100
        with pytest.raises(ValueError):
            fn(np.array([-1]))
        with pytest.raises(ValueError):
            fn(torch.tensor([0, 40], device="cuda"))
    assert flat_stats(dev, np.array([36]), 64, 1e-9, 20).cpu().tolist() == [[64, 64, 1]]
    assert flat_stats(dev, np.zeros(0, np.int64), 64).shape == (0, 3)
    assert gather(dev, np.zeros(0, np.int64), 64).shape == (0, 64)


# ---------------------------------------------------------------------------- the gate
GATE_N = 5760


def _gate_recordings():
    """One window per recording (L = N), each on one side of one threshold."""
    from vaeteb.windows import Recording
    rng = np.random.default_rng(7)
    S = GATE_N // 16

    def rec(name, fhr_runs=(), up_runs=(), ones=None):
        x = np.stack([_walk(rng, GATE_N), _walk(rng, GATE_N, 20.0)])
        for ch, runs in ((0, fhr_runs), (1, up_runs)):
            a = 50
            for n in runs:
                x[ch, a:a + n] = 5000.0 + a                   # far from the walk: neighbours differ
                a += n + 30
        w = None
        if ones is not None:
            w = np.zeros(S, np.float32)
            w[rng.permutation(S)[:ones]] = 1.0
        return Recording(x, name, weight=w)

    # name, recording, the rules that reject it
    return [("clean", rec("clean"), ()),
            ("fhr480", rec("fhr480", fhr_runs=[480]), ()),
            ("fhr481", rec("fhr481", fhr_runs=[481]), ("max_flat_fhr",)),
            ("up1200", rec("up1200", up_runs=[1200]), ()),
            ("up1201", rec("up1201", up_runs=[1201]), ("max_flat_up", "total_flat_up")),
            ("fhr_tot1200", rec("fhr_tot1200", fhr_runs=[400, 400, 400]), ()),
            ("fhr_tot1201", rec("fhr_tot1201", fhr_runs=[400, 401, 400]), ("total_flat_fhr",)),
            ("up_tot1200", rec("up_tot1200", up_runs=[400, 400, 400]), ()),
            ("up_tot1201", rec("up_tot1201", up_runs=[401, 400, 400]), ("total_flat_up",)),
            ("short_runs", rec("short_runs", fhr_runs=[19] * 80), ()),           # 1520 flat samples, none qualifies
            ("w0.9", rec("w0.9", ones=324), ()),                                 # 324 / 360 = 0.9: not < 0.9
            ("w<0.9", rec("w<0.9", ones=323), ("weight",)),
            ("w_and_flat", rec("w_and_flat", fhr_runs=[600], ones=100), ("max_flat_fhr", "weight"))]


def test_quality_gate_thresholds_masks_and_report():
    _need_gpu()
    from vaeteb.windows import RULES, QualityGate, RecordingWindows
    cases = _gate_recordings()
    rw = RecordingWindows([r for _, r, _ in cases], N=GATE_N, overlap=0.5, gate=QualityGate(), batch_size=4)
    W = len(cases)
    assert rw.n_windows == W and rw.start.tolist() == [0] * W and rw.rec.tolist() == list(range(W))
    # the kernel's statistics equal the host's on every row
    exp = np.array([[flat_stats_np(r.x[c].numpy(), 1e-9, 20) for c in (0, 1)] for _, r, _ in cases])
    assert (rw.stats.cpu().numpy() == exp).all()
    assert exp[1, 0].tolist() == [480, 480, 1] and exp[6, 0].tolist() == [401, 1201, 3]
    assert exp[9, 0].tolist() == [0, 0, 0]
    # every rule as the reference states it
    masks = {k: rw.result.masks[k].cpu().numpy() for k in RULES}
    for i, (name, _, rules) in enumerate(cases):
        assert {k for k in RULES if masks[k][i]} == set(rules), name
        assert bool(rw.result.keep[i]) == (not rules), name
    assert rw.weight_mean.dtype == torch.float64
    assert rw.weight_mean[10].item() == 0.9 and rw.weight_mean[11].item() < 0.9 and rw.weight_mean[0].item() == 1.0
    # report and masks agree
    kept = [i for i, (_, _, rules) in enumerate(cases) if not rules]
    assert rw.kept.tolist() == kept
    assert rw.report["windows"] == W and rw.report["kept"] == len(kept) and rw.report["rejected"] == W - len(kept)
    for k in RULES:
        assert rw.report[k] == int(masks[k].sum()) == sum(k in rules for _, _, rules in cases)
    # the batches carry the kept windows, in order, bit for bit
    guids = [g for b in rw for g in b.guid]
    assert guids == [cases[i][0] for i in kept] and len(rw) == 2
    xs = torch.cat([b.x for b in rw]).cpu().numpy()
    assert (_bits(xs) == _bits(np.stack([cases[i][1].x.numpy() for i in kept]))).all()


def test_weights_need_aligned_starts():
    _need_gpu()
    from vaeteb.windows import Recording, RecordingWindows
    r = Recording(np.zeros((2, 160), np.float32), "a", weight=np.ones(10))
    with pytest.raises(ValueError):
        RecordingWindows([r], N=40, overlap=0.5)               # hop 20: not a multiple of 16
    rw = RecordingWindows([r], N=64, overlap=0.5)
    assert rw.start.tolist() == [0, 32, 64, 96] and rw.weight_mean.tolist() == [1.0] * 4


def test_no_windows():
    """A recording shorter than N gives no window; nothing to launch, nothing to iterate."""
    _need_gpu()
    from vaeteb.windows import Recording, RecordingWindows
    for recs in ([], [Recording(np.zeros((2, 100), np.float32), "short", weight=np.ones(6))]):
        rw = RecordingWindows(recs, N=128)
        assert rw.n_windows == 0 and rw.n_kept == 0 and len(rw) == 0 and list(rw) == []
        assert rw.stats.shape == (0, 2, 3) and rw.report["windows"] == 0 and rw.report["kept"] == 0


# ---------------------------------------------------------------------------- end to end
def test_recordings_to_dataset_end_to_end(tmp_path):
    _need_gpu()
    from vaeteb import synthetic
    from vaeteb.data import CombinedHDF5Dataset
    from vaeteb.frontend import FrontEnd, FrontEndPlan
    from vaeteb.windows import QualityGate, Recording, RecordingWindows, window_starts, write_dataset
    N, S = 4096, 256
    w = synthetic.batch(500, 5, N)
    a = np.concatenate(list(w[:3]), axis=-1)[:, :10240].copy()
    b = np.concatenate(list(w[3:]), axis=-1)[:, :6144].copy()
    a[0, 3000:3600] = a[0, 3000]                               # a 600-sample FHR dropout
    wb = np.ones(6144 // 16, np.float32)
    wb[[5, 130, 200, 300]] = 0.0
    recs = [Recording(a, "rec_a"), Recording(b, "rec_b", weight=wb, domain_start=-44640.0, target=2.0, cs_label=True)]
    fe = FrontEnd(FrontEndPlan(11, 4, 16, N, device="cuda"))
    rw = RecordingWindows(recs, N=N, overlap=0.5, gate=QualityGate(), batch_size=3)

    # the kept set, computed on the host
    gate = lambda x: (flat_stats_np(x[0])[0] > 480 or flat_stats_np(x[1])[0] > 1200 or
                      flat_stats_np(x[0])[1] > 1200 or flat_stats_np(x[1])[1] > 1200)
    host = []
    for ri, r in enumerate((a, b)):
        for s0 in window_starts(r.shape[1], N, 0.5):
            wm = 1.0 if ri == 0 else float(wb[s0 // 16:s0 // 16 + S].astype(np.float64).mean())
            if not gate(r[:, s0:s0 + N]) and not wm < 0.9:
                host.append((ri, int(s0)))
    assert host == [(0, 4096), (0, 6144), (1, 0), (1, 2048)]
    assert [(int(r), int(s)) for r, s in zip(rw.rec[rw.kept], rw.start[rw.kept])] == host
    assert rw.report["windows"] == 6 and rw.report["max_flat_fhr"] == 2 and rw.report["kept"] == 4

    # batches: the torch-sliced windows bit for bit, and the same features from them
    sliced = torch.stack([torch.from_numpy((a, b)[r][:, s:s + N]) for r, s in host]).cuda()
    batches = list(rw)
    assert [len(bt.rec) for bt in batches] == [3, 1]
    got_x = torch.cat([bt.x for bt in batches])
    assert torch.equal(got_x.view(torch.int32), sliced.view(torch.int32))
    assert [g for bt in batches for g in bt.guid] == ["rec_a", "rec_a", "rec_b", "rec_b"]
    assert np.concatenate([bt.epoch for bt in batches]).tolist() == [4096.0, 6144.0, -44640.0, -42592.0]
    ref = {k: v.clone() for k, v in fe.raw(sliced).items()}
    got = {k: v.clone() for k, v in fe.raw(got_x).items()}
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    # the batches feed fit_stats directly
    stats = fe.fit_stats(bt.x for bt in rw)
    assert np.asarray(stats["fhr_st_mean"]).size == 43 and np.isfinite(np.asarray(stats["fhr_st_mean"])).all()

    # the file CombinedHDF5Dataset loads
    path = str(tmp_path / "train.npz")
    assert write_dataset(path, rw, fe) == 4
    with pytest.raises(ValueError):
        write_dataset(str(tmp_path / "train.h5"), rw, fe)
    ds = CombinedHDF5Dataset([path], cache_size=0, pin_memory=False)
    assert len(ds) == 4
    st, pairs = ref["fhr_st"].cpu(), ref["pairs"].cpu()
    for i, (ri, s0) in enumerate(host):
        smp = ds[i]
        assert torch.equal(smp.fhr, sliced[i, 0].cpu()) and torch.equal(smp.up, sliced[i, 1].cpu())
        assert smp.fhr_st.shape == (S, 43) and smp.fhr_ph.shape == (S, 44) and smp.fhr_up_ph.shape == (S, 130)
        assert torch.equal(smp.fhr_st, st[i].T) and torch.equal(smp.fhr_ph, pairs[i, :44].T)
        assert torch.equal(smp.fhr_up_ph, pairs[i, 44:].T)
        assert smp.guid == ("rec_a", "rec_b")[ri]
        assert float(smp.epoch) == (0.0, -44640.0)[ri] + s0
        assert smp.cs_label is (ri == 1) and smp.bg_label is False
        wexp = np.ones(S, np.float32) if ri == 0 else wb[s0 // 16:s0 // 16 + S]
        assert (smp.weight.numpy() == wexp).all()
        assert (smp.target.numpy() == (0.0 if ri == 0 else 2.0) * wexp).all()
    only_b = CombinedHDF5Dataset([path], allowed_guids=["rec_b"], cs_label=True, cache_size=0, pin_memory=False)
    assert len(only_b) == 2
