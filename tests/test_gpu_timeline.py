"""Windows stitched into recording timelines on the GPU (vaeteb.timeline, csrc/timeline.hip).

Bounds:
* vt_timeline_accumulate + vt_timeline_finish vs the float64 restatement (tests/timeline_util.py
  stitch_np): per position (m + 3) 2^-24 sum w|v| / sum w with m covering windows — one rounding of
  the window value, m products, m - 1 sums, one quotient, one spare.  count exact; positions no window
  covers hold the fill; singly covered positions of a plain mean are the input bits.
* Any split of an ascending window list into consecutive calls, and a second run: equal bits.
* vt_timeline_finish with a scale and a shift: the bits of torch's (acc / wacc) * scale + shift.
* overlap_mean vs SeqVaeTeb.get_predictions on the device: equal NaN masks, values within twice the
  bound (ATen's nanmean has its own float32 order), within the bound of the restatement.
* vt_timeline_metrics vs float64 numpy over the covered positions: the bounds tests/test_gpu_eval.py
  holds vt_recon_metrics_rows to (rows drawn the same way, recon = y + 0.7 noise): mse and
  1 - vaf_unclamped 1e-6 relative, snr 1e-5 dB, vaf == clamp(vaf_unclamped); covered fraction exact.
* RecordingScorer end to end: see test_end_to_end_* (four synthetic recordings, one with two gated
  windows and a hole, one shorter than a window).
"""
import numpy as np
import pytest
import torch

from timeline_util import DB, masked_metrics_np, metrics64, overlap_mean_np, stitch_np

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits(t):
    return t.contiguous().view(torch.int32)


def _check_case(vals, off, lengths, total, blend, fill=float("nan"), what=""):
    """stitch on the device against stitch_np: bound, exact count, fill where uncovered."""
    from vaeteb.timeline import stitch
    out, count = stitch(torch.from_numpy(vals).cuda(), off, total, lengths=lengths, blend=blend, fill=fill)
    ref, rcount, bound = stitch_np(vals, off, lengths, total, blend)
    out, count = out.cpu().numpy(), count.cpu().numpy()
    assert out.dtype == np.float32 and count.dtype == np.int32 and out.shape == (total,)
    assert np.array_equal(count, rcount), what
    cov = rcount > 0
    err = np.abs(out[cov].astype(np.float64) - ref[cov])
    assert (err <= bound[cov]).all(), (what, float((err / np.maximum(bound[cov], 1e-300)).max()))
    if np.isnan(fill):
        assert np.isnan(out[~cov]).all(), what
    else:
        assert (out[~cov] == np.float32(fill)).all(), what
    return out, rcount


# ------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_stitch_vs_float64(n):
    """hops 1 (up to n-fold coverage), n // 2 (the product's half overlap), n (abutting), n + 5 (gaps);
    the windows start 3 positions in and the timeline ends 4 past the last one."""
    rng = np.random.Generator(np.random.PCG64(n))
    for inner in (1, 3, 32):
        for W in (1, 2, 7):
            vals = rng.standard_normal((W, n, inner) if inner > 1 else (W, n)).astype(np.float32)
            for hop in sorted({1, max(n // 2, 1), n, n + 5}):
                off = 3 + hop * np.arange(W)
                total = int(off[-1]) + n + 4
                for blend in ("mean", "taper"):
                    _check_case(vals, off, None, total, blend, what=f"n={n} inner={inner} W={W} hop={hop} {blend}")


@pytest.mark.parametrize("inner", [1, 32])
@pytest.mark.parametrize("blend", ["mean", "taper"])
def test_stitch_duplicates_gaps_lengths_and_fill(inner, blend):
    """One table with a duplicated offset, two 'recordings' separated by positions nothing touches and
    lengths that clip the last window of each; coverage runs from 0 to 4."""
    n = 64
    off = np.array([5, 5, 20, 37, 90, 230, 262, 294])
    lengths = np.array([64, 64, 64, 64, 30, 64, 64, 16], np.int32)
    total = 330
    rng = np.random.Generator(np.random.PCG64(11 + inner))
    vals = rng.standard_normal((8, n, inner) if inner > 1 else (8, n)).astype(np.float32)
    for fill in (float("nan"), -7.5):
        out, count = _check_case(vals, off, lengths, total, blend, fill=fill, what=f"fill={fill}")
        assert count.min() == 0 and count.max() >= 3
        assert (count[120:230] == 0).all() and (count[:5] == 0).all() and (count[326:] == 0).all()
    # without lengths the same table must run past the end: refused on the host
    from vaeteb.timeline import stitch
    with pytest.raises(ValueError):
        stitch(torch.from_numpy(vals).cuda(), off, total, blend=blend)


def test_single_cover_is_the_input_bits():
    from vaeteb.timeline import stitch
    n, W, hop = 65, 5, 40
    gen = torch.Generator().manual_seed(3)
    vals = torch.randn(W, n, generator=gen)
    off = hop * np.arange(W)
    total = int(off[-1]) + n
    out, count = stitch(vals.cuda(), off, total)
    out, count = out.cpu(), count.cpu()
    src = torch.full((total,), float("nan"))
    for j in range(W):
        src[off[j]:off[j] + n] = vals[j]           # singly covered positions keep their one writer
    single = count == 1
    assert single.sum() == total - 4 * (n - hop) and (count[~single] == 2).all()
    assert torch.equal(bits(out[single]), bits(src[single]))


# ------------------------------------------------------------------ split invariance, determinism
@pytest.mark.parametrize("inner", [1, 32])
@pytest.mark.parametrize("blend", ["mean", "taper"])
def test_split_invariance_and_determinism(inner, blend):
    from vaeteb.timeline import TimelineState
    W, n, hop = 7, 64, 32
    gen = torch.Generator().manual_seed(17 + inner)
    vals = torch.randn((W, n, inner) if inner > 1 else (W, n), generator=gen).cuda()
    off = 10 + hop * np.arange(W)
    total = int(off[-1]) + n + 10

    def run(cuts):
        st = TimelineState(total, blend)
        for a, b in zip(cuts[:-1], cuts[1:]):
            st.accumulate(vals[a:b], off[a:b])
        out, count = st.finish(fill=-1.0)
        return st.acc, st.wacc, count, out

    one = run([0, W])
    assert one[2].max().item() == 2 and one[2].min().item() == 0
    for other in [run([0, W])] + [run([0, k, W]) for k in range(1, W)] + [run(list(range(W + 1)))]:
        for a, b in zip(one, other):
            assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ finish
def test_finish_is_quotient_product_sum():
    from vaeteb import _lib
    from vaeteb.timeline import TimelineState
    W, n, hop = 9, 300, 100
    gen = torch.Generator().manual_seed(5)
    vals = (torch.randn(W, n, generator=gen) * 3 + 0.5).cuda()
    off = hop * np.arange(W)
    total = int(off[-1]) + n + 3                    # 3 uncovered positions, total not a multiple of 4
    st = TimelineState(total, "taper").accumulate(vals, off)
    std, mean = 17.31259, 139.4703
    out, count = st.finish(scale=std + 1e-8, shift=mean)
    cov = count > 0
    assert int(count.max()) == 3 and int((~cov).sum()) == 3
    want = (st.acc / st.wacc) * (std + 1e-8) + mean
    assert torch.equal(bits(out[cov]), bits(want[cov])) and torch.isnan(out[~cov]).all()
    plain, _ = st.finish()
    assert torch.equal(bits(plain[cov]), bits((st.acc / st.wacc)[cov]))
    # bases off the 16-byte grid take the scalar path: the same bits
    pad = lambda t: torch.cat([t.new_zeros(1), t])[1:]
    a, w, c = pad(st.acc), pad(st.wacc), pad(st.count)
    o = torch.empty(total + 1, device="cuda")[1:]
    assert a.data_ptr() % 16 == 4 and o.data_ptr() % 16 == 4
    _lib.call("vt_timeline_finish", a.data_ptr(), w.data_ptr(), c.data_ptr(), total, float("nan"), std + 1e-8, mean,
              o.data_ptr(), _lib.stream())
    assert torch.equal(bits(o), bits(out))


# ------------------------------------------------------------------ overlap_mean
@pytest.mark.parametrize("shape,stride,new_C", [((2, 5, 7), 2, 12), ((2, 5, 7), 3, 8), ((2, 5, 7), 9, 40),
                                                ((2, 20, 48), 16, 320)])
def test_overlap_mean_vs_get_predictions(shape, stride, new_C):
    from vaeteb.model import SeqVaeTeb
    from vaeteb.timeline import overlap_mean
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(stride + new_C))
    got = overlap_mean(x.cuda(), stride, new_C)
    want = SeqVaeTeb.get_predictions(x.cuda(), stride, new_C)[1]
    ref, count, bound = overlap_mean_np(x.numpy(), stride, new_C)
    assert got.shape == want.shape == (shape[0], new_C) and got.dtype == torch.float32
    got, want = got.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
    cov = count > 0
    assert np.array_equal(np.isnan(got), ~cov) and np.array_equal(np.isnan(want), ~cov)
    assert (np.abs(got - ref)[cov] <= bound[cov]).all()
    assert (np.abs(got - want)[cov] <= 2 * bound[cov]).all()
    if shape == (2, 20, 48):
        assert count.max() == 3 and cov.all()       # 48-sample rows every 16: triple coverage, none clipped away


# ------------------------------------------------------------------ metrics kernel
LENGTHS = [1, 63, 255, 256, 257, 1200]


def _metrics(y, recon, count, base):
    from vaeteb import _lib
    R = len(base) - 1
    out = torch.empty((R, 5), device="cuda")
    b = torch.as_tensor(np.asarray(base, np.int64)).cuda()
    _lib.call("vt_timeline_metrics", _lib.ptr(y), _lib.ptr(recon), _lib.ptr(count), _lib.ptr(b), R, _lib.ptr(out),
              _lib.stream())
    return out


def _assert_metric_bounds(out, ref, what):
    """out (R, 5) float32 from the kernel, ref (R, 5) float64; rows of NaN must be NaN in both."""
    o = out.double().cpu().numpy()
    nan = np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(o[:, :4]), np.repeat(nan[:, None], 4, 1)), what
    assert np.array_equal(o[:, 4], ref[:, 4].astype(np.float32).astype(np.float64)), what      # covered fraction exact
    o, r = o[~nan], ref[~nan]
    e_mse = np.abs(o[:, 1] - r[:, 1]) / np.maximum(r[:, 1], 1e-300)
    e_vu = np.abs((1 - o[:, 3]) - (1 - r[:, 3])) / np.maximum(np.abs(1 - r[:, 3]), 1e-300)
    e_snr = np.abs(o[:, 2] - r[:, 2])
    print(f"{what}: mse rel {e_mse.max():.2e}  (1 - vaf_unclamped) rel {e_vu.max():.2e}  snr abs {e_snr.max():.2e} dB")
    assert (e_mse <= 1e-6).all() and (e_vu <= 1e-6).all() and (e_snr <= 1e-5).all(), what
    ok = ~torch.isnan(out[:, 0])
    assert torch.equal(out[ok, 0], out[ok, 3].clamp(0.0, 1.0)), what


def test_metrics_kernel_vs_float64():
    from vaeteb.evaluate import recon_metrics
    base = np.concatenate([[0], np.cumsum(LENGTHS)])
    total = int(base[-1])
    rng = np.random.Generator(np.random.PCG64(2024))
    y = rng.standard_normal(total).astype(np.float32)
    pr = (y + np.float32(0.7) * rng.standard_normal(total).astype(np.float32)).astype(np.float32)
    yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(pr).cuda()
    full = np.ones(total, np.int32)
    gap = full.copy()
    for r in range(1, 6):                           # a hole in the middle of every recording but the first
        a, b = base[r], base[r + 1]
        gap[a + (b - a) // 3:a + 2 * (b - a) // 3] = 0
    none = np.where(np.arange(total) >= base[5], 0, 3).astype(np.int32)     # the last recording uncovered
    none[base[2] + 7] = 0
    for name, count in (("all covered", full), ("gap in the middle", gap), ("one recording uncovered", none)):
        cd = torch.from_numpy(count).cuda()
        out = _metrics(yd, pd, cd, base)
        ref = masked_metrics_np(y, pr, count, base)
        _assert_metric_bounds(out, ref, name)
        assert out[0, 0].item() == 0 and out[0, 3].item() == 0          # L = 1: no variance, vaf 0
        assert torch.equal(bits(out), bits(_metrics(yd, pd, cd, base))), name                 # deterministic
    o = _metrics(yd, pd, torch.from_numpy(none).cuda(), base).cpu().numpy()
    assert np.isnan(o[5, :4]).all() and o[5, 4] == 0 and o[4, 4] == 1 and o[2, 4] == np.float32(254 / 255)
    # a fully covered recording against the row kernel of vaeteb.evaluate
    out = _metrics(yd, pd, torch.from_numpy(full).cuda(), base)
    for r in range(6):
        a, b = int(base[r]), int(base[r + 1])
        row = torch.stack(recon_metrics(yd[a:b][None].contiguous(), pd[a:b][None].contiguous()), -1).view(1, 4)
        rv = row.double().cpu().numpy()
        _assert_metric_bounds(out[r:r + 1], np.concatenate([rv, [[1.0]]], 1), f"recording {r} vs recon_metrics")
    # an empty recording between two others
    out = _metrics(yd, pd, torch.from_numpy(full).cuda(), [0, 64, 64, 320]).cpu().numpy()
    assert np.isnan(out[1, :4]).all() and out[1, 4] == 0 and out[0, 4] == 1 and out[2, 4] == 1


# ------------------------------------------------------------------ end to end
N, HOP, TRIM = 2048, 1024, 8
REC_LENGTHS = [2048, 5120, 5120, 1500]


def _recordings():
    """Four recordings from one seeded generator; recording 1 holds a constant FHR run over samples
    2300..2699, inside its two middle windows only."""
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
        out.append(Recording(x, f"rec_{i}", domain_start=1000.0 * (i + 1)))
    return out


@pytest.fixture(scope="module")
def e2e():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from golden_util import det_fill_
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.model import SeqVaeTeb
    from vaeteb.timeline import RecordingScorer
    from vaeteb.windows import QualityGate, RecordingWindows
    fe = FrontEnd(FrontEndPlan(6, 1, 16, N, device="cuda"), load_stats(6, 1, 16, 4096), trim=TRIM)
    assert fe.S_out == 112 and fe.N_out == 1792 and fe.plan.S * fe.plan.step == N
    m = det_fill_(SeqVaeTeb(sequence_length=112, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                            cross_phase_channels=fe.C_x)).cuda()
    recs = _recordings()
    big = 10 ** 9
    gate = QualityGate(max_flat_fhr=300, max_flat_up=big, total_flat_fhr=big, total_flat_up=big)
    win = lambda bs: RecordingWindows(recs, N=N, overlap=0.5, gate=gate, batch_size=bs, device="cuda")
    rw = win(256)
    scorer = RecordingScorer(m, fe)
    m.train()
    torch.cuda.synchronize()
    rng0 = torch.cuda.get_rng_state()
    res = scorer(rw, keep_windows=True)
    torch.cuda.synchronize()
    rng1 = torch.cuda.get_rng_state()
    return dict(fe=fe, m=m, recs=recs, rw=rw, win=win, scorer=scorer, res=res, rng=(rng0, rng1),
                training_after=m.training)


def test_end_to_end_preconditions(e2e):
    rw, res = e2e["rw"], e2e["res"]
    assert rw.report["windows"] == 9 and rw.report["rejected"] == 2 and rw.report["max_flat_fhr"] == 2
    assert rw.rec[rw.kept].tolist() == [0, 1, 1, 2, 2, 2, 2] and rw.start[rw.kept].tolist() == [0, 0, 3072, 0, 1024,
                                                                                               2048, 3072]
    assert 3 not in rw.rec                                              # recording 3 has no window
    cs = [c.cpu().numpy() for c in res.coverage_steps]
    assert [len(c) for c in cs] == [128, 320, 320, 93] and [len(t) for t in res.recon] == REC_LENGTHS
    assert cs[2].max() == 2                                              # some step is covered twice
    inner = cs[1][TRIM:320 - TRIM]
    assert inner[0] == 1 and inner[-1] == 1 and (inner == 0).any()       # a hole inside recording 1
    assert (cs[1][120:200] == 0).all() and cs[3].max() == 0 and res.coverage[3].max().item() == 0
    assert torch.isnan(res.te[3]).all() and torch.isnan(res.recon[3]).all()
    assert res.te[0].shape == (128,) and torch.isnan(res.te[0][:TRIM]).all() and torch.isfinite(res.te[0][TRIM:120]).all()


def test_end_to_end_timelines_are_the_stitch_of_the_windows(e2e):
    """(a) te / recon against the float64 stitch of the scorer's own per-window kl / mu_pr, metrics
    against the restatement on the stitched arrays."""
    res, fe, recs = e2e["res"], e2e["fe"], e2e["recs"]
    lay, w = res.layout, res.windows
    so, no = lay.window_offsets(w.rec, w.start, fe)
    assert so.tolist() == [8, 128 + 8, 128 + 192 + 8, 448 + 8, 448 + 72, 448 + 136, 448 + 200]
    kl, mu = w.kl.cpu().numpy(), w.mu_pr.cpu().numpy()
    assert kl.shape == (7, 112, 32) and mu.shape == (7, 1792)
    for got, cnt, vals, off, total in ((res.te_packed, res.coverage_steps, kl, so, lay.n_steps),
                                       (res.recon_packed, res.coverage, mu, no, lay.n_samples)):
        ref, count, bound = stitch_np(vals, off, None, total)
        got = got.cpu().numpy()
        assert np.array_equal(torch.cat(cnt).cpu().numpy(), count)
        cov = count > 0
        assert np.isnan(got[~cov]).all() and (np.abs(got[cov] - ref[cov]) <= bound[cov]).all()
    fm, fs = fe.stats["fhr"]
    y = np.concatenate([(r.x[0].numpy() - np.float32(fm)) / (np.float32(fs) + np.float32(1e-8)) for r in recs])
    assert y.dtype == np.float32
    ref = masked_metrics_np(y, res.recon_packed.cpu().numpy(), torch.cat(res.coverage).cpu().numpy(), lay.sample_base)
    assert res.metrics.shape == (4, 5)
    _assert_metric_bounds(res.metrics, ref, "recording metrics")
    frac = res.metrics[:, 4].cpu().numpy()
    assert frac[0] == np.float32(1792 / 2048) and frac[1] == np.float32(2 * 1792 / 5120) and frac[3] == 0
    assert frac[2] == np.float32((5120 - 256) / 5120)


def _propagated(y, ref_mu, got_mu):
    """Allowed |d mse|, |d vaf_unclamped|, |d snr| between the metric kernels' values of got_mu and of
    ref_mu (one row each), from the measured delta = got_mu - ref_mu (tests/test_gpu_eval.py module
    docstring): |d mse|, |d var_res| <= (2 |delta| |res| + |delta|^2) / n, plus the kernels' own 1e-6
    / 1e-5 dB on either side and the float32 rounding of two outputs."""
    y, ref_mu, got_mu = (np.asarray(a, np.float64) for a in (y, ref_mu, got_mu))
    n = y.shape[-1]
    nd, nr = np.linalg.norm(got_mu - ref_mu), np.linalg.norm(y - ref_mu)
    d = (2 * nd * nr + nd ** 2) / n
    _, mse, _, vu = metrics64(y.astype(np.float32), ref_mu.astype(np.float32))
    assert d < 0.5 * mse
    return (d + 2e-6 * mse, d / y.var() + 2e-6 * abs(1 - vu) + 1.2e-7 * max(1.0, abs(vu)),
            DB * d / (mse - d) + 2e-5)


def test_end_to_end_windows_match_the_per_window_loop(e2e):
    """(b) each kept window alone through the public API: kl / te bit-equal (row-independent encoders
    and latent kernel, as tests/test_gpu_eval.py asserts for chunking), mu_pr within the forward-output
    bound 5e-5 rel-L2, the metrics within what that deviation allows."""
    from vaeteb.windows import gather
    res, fe, m, rw = e2e["res"], e2e["fe"], e2e["m"], e2e["rw"]
    w = res.windows
    eps = torch.zeros(1, 1, 112, 32, device="cuda")
    for i, k in enumerate(rw.kept):
        x = gather(rw.buffer, rw.row_off_host[k], N).view(1, 2, N)
        f = fe(x)
        r = m.reconstruction_metrics(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], eps=eps, elementwise=True,
                                     return_mu=True)
        assert torch.equal(r.kl.view(112, 32), w.kl[i]) and torch.equal(r.te.view(()), w.te[i]), i
        e = rel(w.mu_pr[i], r.mu_pr.view(-1))
        assert e < 5e-5, (i, e)
        a_mse, a_vu, a_snr = _propagated(f["fhr"].view(-1).cpu().numpy(), r.mu_pr.view(-1).cpu().numpy(),
                                         w.mu_pr[i].cpu().numpy())
        assert abs(w.mse[i].item() - r.mse.item()) <= a_mse, i
        assert abs(w.vaf_unclamped[i].item() - r.vaf_unclamped.item()) <= a_vu, i
        assert abs(w.vaf[i].item() - r.vaf.item()) <= a_vu, i
        assert abs(w.snr[i].item() - r.snr.item()) <= a_snr, i


def test_end_to_end_batch_size_does_not_move_te(e2e):
    """(c) batch_size 1, 3 and 256."""
    res, m, fe = e2e["res"], e2e["m"], e2e["fe"]
    for bs in (1, 3):
        r = m.score_recordings(fe, e2e["win"](bs))
        assert torch.equal(bits(r.te_packed), bits(res.te_packed)), bs
        assert torch.equal(torch.cat(r.coverage_steps), torch.cat(res.coverage_steps))
        assert torch.equal(torch.cat(r.coverage), torch.cat(res.coverage))
        assert torch.equal(r.windows.te, res.windows.te)
        cov = torch.cat(res.coverage) > 0
        e = rel(r.recon_packed[cov], res.recon_packed[cov])
        print(f"batch_size {bs}: recon rel-L2 vs batch_size 256 {e:.2e}")
        assert e < 5e-5, (bs, e)
        assert r.windows.kl is None and r.windows.mu_pr is None
    assert m.__dict__["_recording_scorer"].frontend is fe              # kept for the next call


def test_end_to_end_denormalised_rows_and_side_effects(e2e):
    """(d) recon_raw, (e) rows(), (f) eval mode and the random stream."""
    res, fe, rw = e2e["res"], e2e["fe"], e2e["rw"]
    fm, fs = fe.stats["fhr"]
    scale, shift = res.denorm
    assert scale == float(np.float32(fs) + np.float32(1e-8)) and shift == float(np.float32(fm))
    cov = torch.cat(res.coverage) > 0
    want = res.recon_packed * scale + shift
    assert torch.equal(bits(res.recon_raw_packed[cov]), bits(want[cov])) and torch.isnan(res.recon_raw_packed[~cov]).all()
    assert [t.shape[0] for t in res.recon_raw] == REC_LENGTHS
    rows = res.rows()
    assert len(rows) == 7 and [r["guid"] for r in rows] == ["rec_0", "rec_1", "rec_1"] + ["rec_2"] * 4
    assert [r["epoch"] for r in rows] == [1000.0, 2000.0, 2000.0 + 3072, 3000.0, 3000.0 + 1024, 3000.0 + 2048,
                                          3000.0 + 3072]
    te = res.windows.te.cpu().numpy()
    assert all(r["te"] == float(te[i]) for i, r in enumerate(rows)) and set(rows[0]) == {"guid", "epoch", "te", "vaf",
                                                                                         "mse", "snr"}
    assert e2e["training_after"] is False
    assert torch.equal(e2e["rng"][0], e2e["rng"][1])
    # without denormalize there is no raw timeline; sampling moves the stream and the reconstruction
    r = e2e["scorer"](rw, denormalize=False)
    assert r.recon_raw is None and torch.equal(bits(r.recon_packed), bits(res.recon_packed))
    torch.cuda.synchronize()
    before = torch.cuda.get_rng_state()
    r = e2e["scorer"](rw, sample=True)
    torch.cuda.synchronize()
    assert not torch.equal(before, torch.cuda.get_rng_state())
    assert torch.equal(bits(r.te_packed), bits(res.te_packed))           # the KL does not see the noise
    assert not torch.equal(bits(r.recon_packed), bits(res.recon_packed))
