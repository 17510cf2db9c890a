"""The host side of the surrogate test (vaeteb.tenull): plans, argument errors, and the numpy
restatement's counts (tests/tenull_ref.py) against a loop over every single comparison.  No GPU."""
import numpy as np
import pytest
import torch

import tenull_ref as R
from vaeteb.tenull import SurrogatePlan, TeSignificanceResult, surrogate_plan

KINDS = ("shift", "block", "swap")
SHAPES = [(3, 7, 4096), (2, 1, 5760)]


# ------------------------------------------------------------------ plans
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,K,N", SHAPES)
def test_plan_properties(kind, B, K, N):
    p = surrogate_plan(kind, B, K, N, seed=3)
    nblk = N // 240
    assert p.src.shape == p.shift.shape == (B, K + 1) and p.src.dtype == p.shift.dtype == np.int32
    assert p.block_len == 240 and p.K == K
    # column 0: the observed row
    assert np.array_equal(p.src[:, 0], np.arange(B)) and not p.shift[:, 0].any()
    if kind == "block":
        assert p.perm.shape == (B, K + 1, nblk) and p.perm.dtype == np.int32
        assert np.array_equal(p.perm[:, 0], np.tile(np.arange(nblk), (B, 1)))
        for b in range(B):
            for k in range(1, K + 1):
                assert sorted(p.perm[b, k]) == list(range(nblk)), (b, k)
                assert not np.array_equal(p.perm[b, k], np.arange(nblk)), (b, k)
    else:
        assert p.perm is None
    sh = p.shift[:, 1:]
    if kind == "shift":
        assert sh.min() >= 240 and sh.max() <= N - 240       # the guard band
    else:
        assert sh.min() >= 0 and sh.max() < N
    if kind == "swap":
        assert (p.src[:, 1:] != np.arange(B)[:, None]).all()
        assert p.src.min() >= 0 and p.src.max() < B
    else:
        assert (p.src == np.arange(B)[:, None]).all()
    # equal seeds, equal plans; another seed, another plan
    q, o = surrogate_plan(kind, B, K, N, seed=3), surrogate_plan(kind, B, K, N, seed=4)
    assert np.array_equal(p.src, q.src) and np.array_equal(p.shift, q.shift)
    assert (p.perm is None and q.perm is None) or np.array_equal(p.perm, q.perm)
    assert not (np.array_equal(p.src, o.src) and np.array_equal(p.shift, o.shift)
                and (p.perm is None or np.array_equal(p.perm, o.perm)))


def test_guard_band_and_block_length_arguments():
    p = surrogate_plan("shift", 2, 50, 1000, seed=0, min_shift=400)
    assert p.shift[:, 1:].min() >= 400 and p.shift[:, 1:].max() <= 600
    p = surrogate_plan("shift", 1, 5, 480, seed=0)             # a single admissible shift
    assert (p.shift[:, 1:] == 240).all()
    p = surrogate_plan("block", 2, 3, 1000, seed=0, block_len=300)
    assert p.perm.shape == (2, 4, 3) and p.block_len == 300


def test_materialised_rows_follow_the_definition():
    """tests/tenull_ref.materialise against the formula applied one sample at a time."""
    rng = np.random.default_rng(0)
    B, K, N, bl = 2, 3, 50, 8
    x = rng.standard_normal((B, 2, N)).astype(np.float32)
    p = surrogate_plan("block", B, K, N, seed=1, min_shift=0, block_len=bl)
    p.src[1, 2] = 0                                            # a row of another recording too
    got = R.materialise(x, p)
    nblk = N // bl
    for b in range(B):
        for k in range(K + 1):
            for i in range(N):
                j = (i - int(p.shift[b, k])) % N
                mj = int(p.perm[b, k, j // bl]) * bl + j % bl if j < nblk * bl else j
                assert got[b, k, i] == x[p.src[b, k], 1, mj]
    assert np.array_equal(got[:, 0], x[:, 1])
    # without a permutation a row is a roll
    q = SurrogatePlan(p.src, p.shift, None, bl).validate(B, N)
    assert np.array_equal(R.materialise(x, q)[1, 1], np.roll(x[1, 1], int(p.shift[1, 1])))


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("kw", [
    dict(kind="shift", K=0), dict(kind="shift", K=4096), dict(kind="shift", min_shift=2049),
    dict(kind="block", block_len=0), dict(kind="block", block_len=4097), dict(kind="block", block_len=2049),
    dict(kind="swap", B=1), dict(kind="fourier"), dict(kind="shift", min_shift=-1),
])
def test_generated_plan_errors(kw):
    a = dict(kind="shift", B=3, K=7, N=4096, seed=0)
    a.update(kw)
    with pytest.raises(ValueError):
        surrogate_plan(a.pop("kind"), a.pop("B"), a.pop("K"), a.pop("N"), a.pop("seed"), **a)


def test_the_largest_plan_is_accepted():
    assert surrogate_plan("shift", 1, 4095, 4096, seed=0).K == 4095


def _hand(B=3, K1=4, nblk=17, perm=True, block_len=240):
    src = np.tile(np.arange(B)[:, None], (1, K1))
    shift = np.tile(np.arange(K1) * 5, (B, 1))
    pm = np.tile(np.arange(nblk), (B, K1, 1)) if perm else None
    return src, shift, pm, block_len


def test_hand_made_plan_errors():
    B, N = 3, 4096
    SurrogatePlan(*_hand()).validate(B, N)
    SurrogatePlan(*_hand(perm=False)).validate(B, N)
    bad = []
    src, shift, pm, bl = _hand()
    bad.append(SurrogatePlan(src[:, :1], shift[:, :1], pm[:, :1], bl))                      # K < 1
    big = 4097
    bad.append(SurrogatePlan(np.tile(np.arange(B)[:, None], (1, big)), np.zeros((B, big), int)))   # K + 1 > 4096
    bad.append(SurrogatePlan(src, shift, pm, 0))                                            # block_len < 1
    bad.append(SurrogatePlan(src, shift, None, N + 1))                                      # block_len > N
    s2 = src.copy(); s2[1, 0] = 2
    bad.append(SurrogatePlan(s2, shift, pm, bl))                                            # column 0: src
    h2 = shift.copy(); h2[0, 0] = N
    bad.append(SurrogatePlan(src, h2, pm, bl))                                              # column 0: shift
    p2 = pm.copy(); p2[2, 0, :2] = [1, 0]
    bad.append(SurrogatePlan(src, shift, p2, bl))                                           # column 0: perm
    for v in (-1, B):
        s3 = src.copy(); s3[0, 2] = v
        bad.append(SurrogatePlan(s3, shift, pm, bl))                                        # src outside [0, B)
    p3 = pm.copy(); p3[1, 2, 0] = 1
    bad.append(SurrogatePlan(src, shift, p3, bl))                                           # not a permutation
    p4 = pm.copy(); p4[1, 2, 0] = 17
    bad.append(SurrogatePlan(src, shift, p4, bl))
    bad.append(SurrogatePlan(src, shift, pm[:, :, :16], bl))                                # perm of another length
    bad.append(SurrogatePlan(src, shift[:, :3], pm, bl))                                    # shapes
    for i, p in enumerate(bad):
        with pytest.raises(ValueError):
            p.validate(B, N)
            pytest.fail(f"case {i} was accepted")
    with pytest.raises(ValueError):
        SurrogatePlan(src, shift.astype(np.int64) + 2 ** 31)                                # not 32-bit


def test_te_significance_checks_before_any_launch():
    """The argument checks come before the first kernel: no GPU is needed to see them."""
    from vaeteb.tenull import TeSignificance

    class _Plan:
        N, device = 4096, "cpu"

    class _Fe:
        plan, C_x, S_out = _Plan(), 0, 256

    with pytest.raises(ValueError):
        TeSignificance(None, _Fe())                                                         # no cross pairs
    with pytest.raises(ValueError):
        TeSignificance(None, _Fe(), rows_per_launch=0)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Sizes and null pointers are checked before any device work."""
    from vaeteb import _lib
    ok = dict(x=1, B=2, stride=8192, N=4096, n_pad=8192, pad_left=2048, mode=0, src=1, shift=1, perm=None, bl=240,
              row0=0, rows=4, tw=1, xhat=1)
    for bad in (dict(n_pad=8000), dict(n_pad=2048), dict(B=0), dict(stride=100), dict(bl=0), dict(bl=4097),
                dict(row0=-1), dict(rows=0), dict(src=None), dict(shift=None), dict(x=None), dict(xhat=None),
                dict(mode=3)):
        a = dict(ok, **bad)
        with pytest.raises(ValueError):
            _lib.call("vt_fe_spectrum_surrogate", a["x"], a["B"], a["stride"], a["N"], a["n_pad"], a["pad_left"],
                      a["mode"], a["src"], a["shift"], a["perm"], a["bl"], a["row0"], a["rows"], a["tw"], a["xhat"],
                      None)
    for args in ((None, 1, 1, 1, 1, 3, 16, 32, 1, 1), (1, 1, 1, 1, 0, 3, 16, 32, 1, 1), (1, 1, 1, 1, 1, 0, 16, 32, 1, 1),
                 (1, 1, 1, 1, 1, 3, 0, 32, 1, 1), (1, 1, 1, 1, 1, 3, 16, 0, 1, 1), (1, 1, 1, 1, 1, 3, 16, 32, None, 1),
                 (1, 1, 1, 1, 1, 3, 16, 32, 1, None)):
        with pytest.raises(ValueError):
            _lib.call("vt_te_kl_steps", *args, None)
    for args in ((1, 1, 0, 5, 16), (1, 1, 2, 1, 16), (1, 1, 2, 4097, 16), (1, 1, 2, 5, 0), (None, 1, 2, 5, 16),
                 (1, None, 2, 5, 16)):
        with pytest.raises(ValueError):
            _lib.call("vt_tenull_stats", *args, 1, 1, 1, 1, 1, 1, 1, None)
    with pytest.raises(ValueError):
        _lib.call("vt_tenull_stats", 1, 1, 2, 5, 16, 1, 1, 1, 1, 1, 1, None, None)


# ------------------------------------------------------------------ counts
quantised = R.quantised


def brute(ts, te):
    B, K1, S = ts.shape
    c, sc, mc = np.zeros(B, np.int64), np.zeros((B, S), np.int64), np.zeros((B, S), np.int64)
    for b in range(B):
        for k in range(1, K1):
            if te[b, k] >= te[b, 0]:
                c[b] += 1
            mx = max(float(v) for v in ts[b, k])
            for s in range(S):
                if ts[b, k, s] >= ts[b, 0, s]:
                    sc[b, s] += 1
                if mx >= ts[b, 0, s]:
                    mc[b, s] += 1
    return c, sc, mc


def _result(ts, te, st):
    t = torch.from_numpy
    return TeSignificanceResult(t(te[:, 0]), t(te[:, 1:]), t(ts[:, 0]), t(ts[:, 1:]), t(st["step_surr_mean"]),
                                t(st["count_ge"]), t(st["step_count_ge"]), t(st["max_count_ge"]),
                                t(st["surr_mean"]), t(st["surr_sd"]), t(st["group_sums"]))


@pytest.mark.parametrize("K1", [2, 3, 65])
@pytest.mark.parametrize("S", [1, 64, 65])
def test_ref_counts_against_brute_force(K1, S):
    B, K = 4, K1 - 1
    ts, te = quantised(B, K1, S, seed=K1 * 100 + S)
    st = R.stats(ts, te)
    c, sc, mc = brute(ts, te)
    assert np.array_equal(st["count_ge"], c) and np.array_equal(st["step_count_ge"], sc)
    assert np.array_equal(st["max_count_ge"], mc)
    # >= against >: the ties are there and they count
    strict = sum(int(te[b, k] > te[b, 0]) for b in range(B) for k in range(1, K1))
    if K1 == 65:
        assert c.sum() > strict
    assert (sc <= mc).all()                                    # the maximum is at least the step
    # moments
    assert np.allclose(st["surr_mean"], te[:, 1:].astype(np.float64).mean(1), rtol=1e-12, atol=0)
    if K > 1:
        assert np.allclose(st["surr_sd"], te[:, 1:].astype(np.float64).std(1, ddof=1), rtol=1e-12, atol=1e-300)
    else:
        assert np.isnan(st["surr_sd"]).all()
    assert np.allclose(st["step_surr_mean"], ts[:, 1:].astype(np.float64).mean(1), rtol=1e-6, atol=1e-7)
    # p-values of the result object
    r = _result(ts, te, st)
    for p, cnt in ((r.p, c), (r.p_steps, sc), (r.p_steps_fwer, mc)):
        p = p.numpy()
        assert p.dtype == np.float64 and (p >= 1.0 / (K + 1)).all() and (p <= 1.0).all()
        assert np.array_equal(p, (1.0 + cnt) / (K + 1))
    assert np.array_equal(r.p.numpy(), R.p_value(c, K))
    g = te.astype(np.float64).sum(0)
    assert np.allclose(r.group_sums.numpy(), g, rtol=1e-12, atol=0)
    want = (1 + sum(1 for k in range(1, K1) if g[k] >= g[0])) / (K + 1)
    assert float(r.group_p()) == want == R.group_p(st["group_sums"])
    assert np.allclose(r.te_effective.numpy(), te[:, 0].astype(np.float64) - st["surr_mean"], rtol=0, atol=0)
    if K > 1:
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.allclose(r.z.numpy(), (te[:, 0] - st["surr_mean"]) / st["surr_sd"], equal_nan=True)


def test_a_nan_never_counts_in_the_reference():
    ts, te = quantised(2, 5, 7, seed=9)
    ts[0, 2, 3] = np.nan
    te[1, 3] = np.nan
    st = R.stats(ts, te)
    clean_ts, clean_te = ts.copy(), te.copy()
    clean_ts[0, 2, 3] = -np.inf                                # never >= anything here, never the maximum
    clean_te[1, 3] = -np.inf
    ref = R.stats(clean_ts, clean_te)
    for f in ("count_ge", "step_count_ge", "max_count_ge"):
        assert np.array_equal(st[f], ref[f]), f
    ts[1, 0, 0] = np.nan                                       # a NaN observation: nothing counts
    st = R.stats(ts, te)
    assert st["step_count_ge"][1, 0] == 0 and st["max_count_ge"][1, 0] == 0


def test_merge_of_two_halves_is_the_whole():
    ts, te = quantised(6, 9, 11, seed=5)
    whole = _result(ts, te, R.stats(ts, te))
    a, b = (_result(ts[s], te[s], R.stats(ts[s], te[s])) for s in (slice(0, 2), slice(2, 6)))
    m = a.merge(b)
    for f in ("count_ge", "step_count_ge", "max_count_ge", "te", "te_surr", "te_steps", "te_steps_surr"):
        assert torch.equal(getattr(m, f), getattr(whole, f)), f
    assert torch.equal(m.p, whole.p) and torch.equal(m.p_steps_fwer, whole.p_steps_fwer)
    assert np.allclose(m.group_sums.numpy(), whole.group_sums.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(m.surr_mean.numpy(), whole.surr_mean.numpy(), rtol=0, atol=0)
    assert float(m.group_p()) == float(whole.group_p())
    other = _result(ts[:, :5], te[:, :5], R.stats(ts[:, :5], te[:, :5]))
    with pytest.raises(ValueError):
        whole.merge(other)
