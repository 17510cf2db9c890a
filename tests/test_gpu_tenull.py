"""The surrogate test of the transfer entropy (vaeteb.tenull, csrc/tenull.hip,
vt_fe_spectrum_surrogate) on the GPU against its numpy restatement (tests/tenull_ref.py) and against
the literal loop: every surrogate batch materialised and run through ShiftSweep at shift 0.

Bounds:
* surrogate spectra: equality with vt_fe_spectrum on the materialised rows (the same values enter the
  same FFT).
* vt_te_kl_steps vs float64: 1e-6 relative on every ts and te, what tests/test_gpu_te_shift.py holds
  vt_te_kl_rows to; te vs vt_te_kl_rows on the same inputs: one float32 ulp (both round a double sum
  of the same fp32 terms, taken in another order).
* vt_tenull_stats: the integers exactly; the float64 moments and group sums 1e-12 relative (sums of
  at most 4095 float32 values in double: 4095 * 2^-53 = 5e-13); step_surr_mean 1e-6.
* end to end: te one ulp off the loop's vt_te_kl_rows, te_steps 1e-6 relative off kl.mean(-1); the
  integers are those of tenull_ref.stats on the device's own ts / te; chunking changes no bit.
No test asserts that a p-value is small or large: with det_fill_ weights that is a property of the
inputs, not of the code.
"""
import numpy as np
import pytest
import torch

import tenull_ref as R

pytestmark = pytest.mark.gpu

KINDS = ("shift", "block", "swap")


def _ulp_close(a, b):
    """|a - b| <= one float32 ulp of b, elementwise (numpy float32 arrays)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)).all()


def _max_rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(a - ref) / np.abs(ref)).max())


def _materialise(x, plan):
    """(B, K+1, N) on the device by torch indexing with tenull_ref's index rows."""
    B, _, N = x.shape
    K1 = plan.K + 1
    idx = np.stack([R.surrogate_index(N, plan.shift[b, k], None if plan.perm is None else plan.perm[b, k],
                                      plan.block_len) for b in range(B) for k in range(K1)])
    rows = x[torch.from_numpy(plan.src.reshape(-1).astype(np.int64)).cuda(), 1]          # (B*K1, N)
    return torch.gather(rows, 1, torch.from_numpy(idx).cuda()).view(B, K1, N)


# ------------------------------------------------------------------ 1. spectra
def _plan_fe(name):
    from vaeteb.frontend import FrontEndPlan
    return {"j11_n4096": lambda: FrontEndPlan(11, 4, 16, 4096, device="cuda"),
            "j11_n5760": lambda: FrontEndPlan(11, 4, 16, 5760, device="cuda"),
            "j6_n2048": lambda: FrontEndPlan(6, 1, 16, 2048, device="cuda")}[name]()


def _windows(B, N, seed=2000):
    from vaeteb import synthetic
    return torch.from_numpy(synthetic.batch(seed, B, N)).cuda().contiguous()


def _surrogate_spectra(p, x, plan, row0=0, rows=None):
    from vaeteb import _lib
    from vaeteb.frontend import _i32
    B, N = x.shape[0], p.N
    rows = B * (plan.K + 1) - row0 if rows is None else rows
    src, shift = _i32(plan.src, "cuda"), _i32(plan.shift, "cuda")
    perm = None if plan.perm is None else _i32(plan.perm, "cuda")
    out = torch.full((rows + 1, p.n_pad, 2), 7.0, device="cuda")        # one guard row behind the output
    _lib.call("vt_fe_spectrum_surrogate", x.data_ptr() + 4 * N, B, 2 * N, N, p.n_pad, p.pad_left, 0, _lib.ptr(src),
              _lib.ptr(shift), _lib.ptr(perm), int(plan.block_len), row0, rows, _lib.ptr(p.t_tw), _lib.ptr(out),
              _lib.stream())
    assert (out[rows] == 7.0).all()
    return out[:rows]


def _plain_spectra(p, u):
    from vaeteb import _lib
    u = u.reshape(-1, p.N).contiguous()
    out = torch.empty((u.shape[0], p.n_pad, 2), device="cuda")
    _lib.call("vt_fe_spectrum", _lib.ptr(u), u.shape[0], p.N, p.n_pad, p.pad_left, 0, _lib.ptr(p.t_tw), _lib.ptr(out),
              _lib.stream())
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", ["j11_n4096", "j11_n5760", "j6_n2048"])
def test_surrogate_spectrum_bit_equal(cfg, kind):
    from vaeteb.tenull import surrogate_plan
    p = _plan_fe(cfg)
    B, K1 = 3, 5
    x = _windows(B, p.N)
    plan = surrogate_plan(kind, B, K1 - 1, p.N, seed=11)
    got, ref = _surrogate_spectra(p, x, plan), _plain_spectra(p, _materialise(x, plan))
    assert torch.equal(got, ref)
    assert torch.isfinite(got).all() and not torch.equal(got[0], got[1])     # the surrogate is really applied
    assert torch.equal(got[::K1], _plain_spectra(p, x[:, 1]))                 # column 0: the observed channel


def _hand_plan(N, block_len, perm, seed=5):
    from vaeteb.tenull import SurrogatePlan
    B, shifts = 3, [0, -1, N, N + 7, -3 * N - 2]
    rng = np.random.default_rng(seed)
    src = np.tile(np.arange(B)[:, None], (1, len(shifts)))
    src[0, 3], src[2, 1] = 2, 0
    pm = None
    if perm:
        nblk = N // block_len
        pm = np.stack([np.stack([np.arange(nblk) if k == 0 else rng.permutation(nblk) for k in range(len(shifts))])
                       for _ in range(B)])
    return SurrogatePlan(src, np.tile(shifts, (B, 1)), pm, block_len).validate(B, N)


@pytest.mark.parametrize("block_len,perm", [(240, True), (4096, True), (1, True), (240, False)])
def test_surrogate_spectrum_hand_made_plans(block_len, perm):
    """Shifts of any sign and magnitude; 17 blocks and a 16-sample tail that stays in place; one block;
    blocks of one sample; no permutation."""
    p = _plan_fe("j11_n4096")
    x = _windows(3, p.N, seed=2001)
    plan = _hand_plan(p.N, block_len, perm)
    u = _materialise(x, plan)
    if block_len == 240 and perm:
        # the tail is not permuted: undo the row's roll and its last 16 samples are the source's
        for b, k in ((0, 1), (1, 3), (2, 4)):
            back = torch.roll(u[b, k], -int(plan.shift[b, k]) % p.N)
            assert torch.equal(back[4080:], x[int(plan.src[b, k]), 1, 4080:])
            assert not torch.equal(back[:4080], x[int(plan.src[b, k]), 1, :4080])
    if block_len == 4096:
        assert torch.equal(u[1, 2], x[1, 1])                                   # shift N, one block: the identity
    got = _surrogate_spectra(p, x, plan)
    assert torch.equal(got, _plain_spectra(p, u))
    if not perm:                                                               # the rolled kernel's rows
        assert torch.equal(got[1 * 5 + 4], _plain_spectra(p, torch.roll(x[1, 1], (-3 * p.N - 2) % p.N)[None])[0])


def test_surrogate_spectrum_from_a_row_offset_inside_a_recording():
    from vaeteb.tenull import surrogate_plan
    p = _plan_fe("j11_n4096")
    B, K1 = 3, 5
    x = _windows(B, p.N)
    for kind in ("swap", "block"):
        plan = surrogate_plan(kind, B, K1 - 1, p.N, seed=12)
        whole = _surrogate_spectra(p, x, plan)
        part = _surrogate_spectra(p, x, plan, row0=K1 + 2, rows=6)             # rows 7 .. 12: recordings 1 and 2
        assert torch.equal(part, whole[K1 + 2:K1 + 8])


# ------------------------------------------------------------------ 2. KL per step
def _kl_steps(mu_c, lv_q, mu_y, lv_p, B, K):
    from vaeteb import _lib
    R_, S, L = mu_c.shape
    assert R_ == B * K
    ts = torch.full((R_ + 1, S), 7.0, device="cuda")
    te = torch.full((R_ + 1,), 7.0, device="cuda")
    _lib.call("vt_te_kl_steps", _lib.ptr(mu_c), _lib.ptr(lv_q), _lib.ptr(mu_y), _lib.ptr(lv_p), B, K, S, L,
              _lib.ptr(ts), _lib.ptr(te), _lib.stream())
    assert (ts[R_] == 7.0).all() and te[R_] == 7.0
    return ts[:R_], te[:R_]


@pytest.mark.parametrize("S,L", [(1, 1), (3, 5), (2, 32), (16, 32), (300, 32), (7, 64)])
def test_te_kl_steps_vs_float64(S, L):
    """ts / te relative error against float64 as printed; the bound is 1e-6 on every element."""
    from vaeteb import _lib
    B, K1 = 2, 3
    gen = torch.Generator().manual_seed(1000 * S + L)
    mu_c, lv_q = torch.randn(B * K1, S, L, generator=gen), torch.randn(B * K1, S, L, generator=gen)
    mu_y, lv_p = torch.randn(B, S, L, generator=gen), torch.randn(B, S, L, generator=gen)
    d = [t.cuda() for t in (mu_c, lv_q, mu_y, lv_p)]
    ts, te = _kl_steps(*d, B, K1)
    ref_ts, ref_te = R.kl_steps(mu_c.numpy(), lv_q.numpy(), mu_y.numpy(), lv_p.numpy(), K1)
    e_ts, e_te = _max_rel(ts.cpu().numpy(), ref_ts), _max_rel(te.cpu().numpy(), ref_te)
    print(f"S={S} L={L}: ts max rel {e_ts:.3e}, te max rel {e_te:.3e}")
    assert ts.shape == (B * K1, S) and te.shape == (B * K1,)
    assert e_ts <= 1e-6 and e_te <= 1e-6
    # against vt_te_kl_rows on the same inputs
    te_rows = torch.empty(B * K1, device="cuda")
    _lib.call("vt_te_kl_rows", _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), B, K1, S * L,
              _lib.ptr(te_rows), None, _lib.stream())
    assert _ulp_close(te.cpu().numpy(), te_rows.cpu().numpy())
    # the prior is read at row r // K1: another prior for recording 1 moves its rows only
    my2, lp2 = d[2].clone(), d[3].clone()
    my2[1] += 0.5
    lp2[1] -= 0.25
    ts2, te2 = _kl_steps(d[0], d[1], my2, lp2, B, K1)
    assert torch.equal(ts2[:K1], ts[:K1]) and torch.equal(te2[:K1], te[:K1])
    assert (te2[K1:] != te[K1:]).all() and (ts2[K1:] != ts[K1:]).any(dim=1).all()
    # the same bits on a second run, and when the rows are split over calls
    ts3, te3 = _kl_steps(*d, B, K1)
    assert torch.equal(ts3, ts) and torch.equal(te3, te)
    halves = [_kl_steps(d[0][b * K1:(b + 1) * K1].contiguous(), d[1][b * K1:(b + 1) * K1].contiguous(),
                        d[2][b:b + 1].contiguous(), d[3][b:b + 1].contiguous(), 1, K1) for b in range(B)]
    assert torch.equal(torch.cat([h[0] for h in halves]), ts) and torch.equal(torch.cat([h[1] for h in halves]), te)
    a = _kl_steps(d[0][K1:K1 + 2].contiguous(), d[1][K1:K1 + 2].contiguous(), d[2][1:2].contiguous(),
                  d[3][1:2].contiguous(), 1, 2)                                # inside recording 1
    assert torch.equal(a[0], ts[K1:K1 + 2]) and torch.equal(a[1], te[K1:K1 + 2])


# ------------------------------------------------------------------ 3. rank statistics
def _stats(ts, te):
    from vaeteb.tenull import rank_statistics
    r = rank_statistics(torch.from_numpy(ts).cuda(), torch.from_numpy(te).cuda())
    torch.cuda.synchronize()
    return r


def _check_stats(r, ref, K):
    for f in ("count_ge", "step_count_ge", "max_count_ge"):
        got = getattr(r, f).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, ref[f]), f
    for f in ("surr_mean", "surr_sd", "group_sums"):
        got = getattr(r, f).cpu().numpy()
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, ref[f], rtol=1e-12, atol=0, equal_nan=True, err_msg=f)
    np.testing.assert_allclose(r.step_surr_mean.cpu().numpy(), ref["step_surr_mean"], rtol=1e-6, atol=0,
                               equal_nan=True)
    for p, c in ((r.p, ref["count_ge"]), (r.p_steps, ref["step_count_ge"]), (r.p_steps_fwer, ref["max_count_ge"])):
        assert p.dtype == torch.float64 and p.is_cuda
        assert np.array_equal(p.cpu().numpy(), R.p_value(c, K))
    assert float(r.group_p()) == R.group_p(ref["group_sums"]) or np.isnan(ref["group_sums"]).any()


@pytest.mark.parametrize("S", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("K1", [2, 3, 64, 65, 257, 4096])
def test_tenull_stats_exact_integers(K1, S):
    B = 3
    ts, te = R.quantised(B, K1, S, seed=K1 * 1000 + S)
    ts[1, K1 - 1, S // 2] = np.nan                             # in a surrogate row: it must not count
    ref = R.stats(ts, te)
    r = _stats(ts, te)
    _check_stats(r, ref, K1 - 1)
    # >= and not >: the tied inputs make the two differ
    if K1 >= 64:
        assert (ref["step_count_ge"] > (ts[:, 1:] > ts[:, :1]).sum(1)).any()
    # the NaN counted nowhere: the counts are those of the same inputs with -inf in its place
    clean = ts.copy()
    clean[1, K1 - 1, S // 2] = -np.inf
    r2 = _stats(clean, te)
    for f in ("count_ge", "step_count_ge", "max_count_ge"):
        assert torch.equal(getattr(r, f), getattr(r2, f)), f


def test_tenull_stats_nan_in_the_row_means_and_the_observation():
    ts, te = R.quantised(3, 9, 70, seed=4)
    te[0, 4] = np.nan                                          # a surrogate's mean
    ts[2, 0, 5] = np.nan                                       # an observed step: nothing is >= a NaN
    ref = R.stats(ts, te)
    r = _stats(ts, te)
    _check_stats(r, ref, 8)
    assert int(r.step_count_ge[2, 5]) == 0 and int(r.max_count_ge[2, 5]) == 0
    assert torch.isnan(r.surr_mean[0]) and torch.isfinite(r.surr_mean[1:]).all()


def test_tenull_stats_single_surrogate():
    ts, te = R.quantised(3, 2, 65, seed=6)
    r = _stats(ts, te)
    _check_stats(r, R.stats(ts, te), 1)
    assert torch.isnan(r.surr_sd).all() and torch.isnan(r.z).all()
    for f in ("surr_mean", "group_sums", "step_surr_mean", "te_effective", "p", "p_steps", "p_steps_fwer"):
        assert torch.isfinite(getattr(r, f)).all(), f
    assert set(np.unique(r.p.cpu().numpy())) <= {0.5, 1.0}


# ------------------------------------------------------------------ 4.-6. end to end
def _model(fe, golden):
    from golden_util import det_fill_
    from vaeteb.model import SeqVaeTeb
    m = det_fill_(SeqVaeTeb(sequence_length=16, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                            cross_phase_channels=fe.C_x))
    sd = m.state_dict()
    for i, k in enumerate(list(golden["bn_names"])):
        sd[k].copy_(torch.from_numpy(golden[f"bn_{i}"]))
    return m.cuda()


FIELDS = ("te", "te_surr", "te_steps", "te_steps_surr", "step_surr_mean", "count_ge", "step_count_ge",
          "max_count_ge", "surr_mean", "surr_sd", "group_sums")


@pytest.fixture(scope="module")
def fx(golden):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.te import ShiftSweep
    from vaeteb.tenull import TeSignificance, surrogate_plan
    g, gi = golden("te_shift_j11_n4096"), golden("te_shift_j11_n4096_in")
    fe = FrontEnd(FrontEndPlan(11, 4, 16, 4096, device="cuda"), load_stats(11, 4, 16, 4096))
    x = torch.from_numpy(gi["x"]).cuda()
    m = _model(fe, g)
    sig, sweep = TeSignificance(m, fe), ShiftSweep(m, fe)
    B, K = x.shape[0], 4
    out = {}
    for kind in KINDS:
        plan = surrogate_plan(kind, B, K, fe.plan.N, seed=21)
        m.train()
        torch.cuda.manual_seed(99)
        rng0 = torch.cuda.get_rng_state()
        r = sig(x, plan=plan)
        torch.cuda.synchronize()
        rng1, training = torch.cuda.get_rng_state(), m.training
        u = _materialise(x, plan)
        te, kl = [], []
        for k in range(K + 1):                                  # the literal loop, one surrogate batch at a time
            xk = x.clone()
            xk[:, 1] = u[:, k]
            s = sweep(xk, [0], elementwise=True)
            te.append(s.te[:, 0])
            kl.append(s.kl[:, 0])
        out[kind] = dict(plan=plan, r=r, loop_te=torch.stack(te, 1), loop_kl=torch.stack(kl, 1), rng0=rng0, rng1=rng1,
                         training=training)
    return dict(fe=fe, x=x, m=m, sig=sig, sweep=sweep, K=K, out=out)


@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end_against_the_literal_loop(fx, kind):
    o, K = fx["out"][kind], fx["K"]
    r, B, S = o["r"], fx["x"].shape[0], fx["fe"].S_out
    assert r.te.shape == (B,) and r.te_surr.shape == (B, K) and r.te.dtype == torch.float32
    assert r.te_steps.shape == r.p_steps.shape == r.p_steps_fwer.shape == (B, S)
    assert r.p.shape == r.z.shape == r.te_effective.shape == (B,) and r.group_sums.shape == (K + 1,)
    te_all = torch.cat([r.te[:, None], r.te_surr], 1).cpu().numpy()
    ts_all = torch.cat([r.te_steps[:, None], r.te_steps_surr], 1).cpu().numpy()
    loop_te, loop_ts = o["loop_te"].cpu().numpy(), o["loop_kl"].mean(-1).cpu().numpy()
    e = _max_rel(ts_all, loop_ts)
    print(f"{kind}: te_steps vs kl.mean(-1) max rel {e:.3e}; te bit-equal {np.array_equal(te_all, loop_te)}")
    assert np.isfinite(te_all).all() and _ulp_close(te_all, loop_te)
    assert e <= 1e-6
    # column 0 is ShiftSweep(x, [0])
    assert _ulp_close(r.te.cpu().numpy(), fx["sweep"](fx["x"], [0]).te[:, 0].cpu().numpy())
    # the surrogates are not the observed row
    assert (te_all[:, 1:] != te_all[:, :1]).all()
    # the integers, from the device's own ts / te
    ref = R.stats(ts_all, te_all)
    _check_stats(r, ref, K)
    assert torch.equal(r.te_effective, r.te.double() - r.surr_mean) and torch.equal(r.z, r.te_effective / r.surr_sd)


@pytest.mark.parametrize("kind", ["swap", "block"])
def test_chunking_does_not_change_a_bit(fx, kind):
    from vaeteb.tenull import TeSignificance
    o = fx["out"][kind]
    for rows in (256, 5, 3, 2):        # all at once, a recording per chunk, inside a recording (3 + 2; 2 + 2 + 1)
        r = TeSignificance(fx["m"], fx["fe"], rows_per_launch=rows)(fx["x"], plan=o["plan"])
        for f in FIELDS:
            assert torch.equal(getattr(r, f), getattr(o["r"], f)), (rows, f)


def test_side_effects(fx):
    from vaeteb.tenull import surrogate_plan
    for kind in KINDS:
        o = fx["out"][kind]
        assert torch.equal(o["rng0"], o["rng1"])                # the device generator is not touched
        assert o["training"] is False                           # left in eval mode
        assert not o["r"].te.requires_grad
    m, fe, x = fx["m"], fx["fe"], fx["x"]
    a = fx["sig"](x, kind="shift", n_surrogates=3, seed=7)
    b = fx["sig"](x, kind="shift", n_surrogates=3, seed=7)
    c = m.te_significance(fe, x, kind="shift", n_surrogates=3, seed=7)
    d = fx["sig"](x, plan=surrogate_plan("shift", x.shape[0], 3, fe.plan.N, 7))
    for f in FIELDS:
        for other in (b, c, d):
            assert torch.equal(getattr(a, f), getattr(other, f)), f
    m.te_significance(fe, x, kind="shift", n_surrogates=1, seed=7)
    assert m.__dict__["_te_significance"].frontend is fe        # kept for the next call
    with pytest.raises(ValueError):
        fx["sig"](x[:, :, :4000], kind="shift", n_surrogates=3)
    with pytest.raises(ValueError):
        fx["sig"](x[:1], kind="swap", n_surrogates=3)
