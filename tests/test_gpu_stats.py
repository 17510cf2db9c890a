"""Dataset statistics on the device (csrc/stats.hip, vaeteb/stats.py) against the reference's
fp64 sums (tests/golden/stats_accum_b5.npz, tools/gen_golden_stats.py) and against a numpy
fp64 restatement of the per-element rule.

Bounds (derived, not measured): a reordered fp64 sum of n <= 2e3 terms errs by at most about
n * 2^-53 * sum|t| ~ 2e-13 * sum|t|, and the double log / asinh (<= 3 / <= 5 ulp) add about
6e-16 relative per term; 1e-12 * sum|t| (sum t^2 for the squares) leaves a margin over both.
sum|t|, not |sum t|: asinh channels sum to near zero.  Finalised fp32 means / variances may
differ from the reference's by one ulp (two nearly equal fp64 values can round apart).  The
cases with more terms per channel (up to 1.3e4: the raw rows of the end-to-end case) keep the
same 1e-12: neither side sums them serially.  A kernel thread adds at most 32 * 1024 / 256 =
128 terms, then 6 butterfly levels, 3 wave sums and one add per chunk; numpy sums pairwise
over blocks of 128.  Either error is below (140 + chunks) * 2^-53 * sum|t| < 3e-14 * sum|t|."""
import numpy as np
import pytest
import torch

from vaeteb import _lib, synthetic
from vaeteb.frontend import FrontEnd, FrontEndPlan
from vaeteb.stats import StatsAccumulator, channel_kinds, chunking, default_fields, finalize_state

pytestmark = pytest.mark.gpu

MULTI = ("fhr_st", "fhr_ph", "fhr_up_ph")
SINGLE = ("fhr", "up")
REL = 1e-12


def np_state(x, kinds, eps=1e-6):
    """count, sum, sum_sq, sum|t|, sum t^2 per channel of x (B, C, S) float32, in fp64."""
    x = np.asarray(x).astype(np.float64)
    C = x.shape[1]
    cnt, s, q, a = np.zeros(C, np.int64), np.zeros(C), np.zeros(C), np.zeros(C)
    with np.errstate(all="ignore"):
        for c in range(C):
            v = x[:, c].ravel()
            m = np.isfinite(v)
            t = np.log(np.maximum(v, 0.0) + eps) if kinds[c] == 1 else np.arcsinh(v) if kinds[c] == 2 else v
            t = t[m & np.isfinite(t)]
            cnt[c], s[c], q[c], a[c] = t.size, t.sum(), (t * t).sum(), np.abs(t).sum()
    return cnt, s, q, a


def check_state(got, want, what=""):
    cnt, s, q = (np.asarray(g) for g in got)
    rc, rs, rq, ra = want
    print(what, "max |dsum| / sum|t|:", np.max(np.abs(s - rs) / np.maximum(ra, 1e-300)),
          "max |dsq| / sum t^2:", np.max(np.abs(q - rq) / np.maximum(rq, 1e-300)))
    assert np.array_equal(cnt, rc), what
    assert np.all(np.abs(s - rs) <= REL * ra), what
    assert np.all(np.abs(q - rq) <= REL * rq), what


def ulp_apart(a, b):
    """Distance in fp32 ulps (both finite, same sign or zero)."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    key = lambda v: np.where(v.view(np.int32) < 0, -(v.view(np.int32) & 0x7fffffff), v.view(np.int32)).astype(np.int64)
    return np.abs(key(a) - key(b))


def messy(rng, shape):
    """Signed values over nine decades with NaN, +inf and -inf sprinkled in."""
    x = rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-6, 3, shape)
    u = rng.random(shape)
    x[u < 0.02] = np.nan
    x[(u >= 0.02) & (u < 0.03)] = np.inf
    x[(u >= 0.03) & (u < 0.04)] = -np.inf
    return x.astype(np.float32)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def accum_view(buf, c_off, C, s0, S_len, kinds, state, work):
    """vt_stats_accum on channels [c_off, c_off + C) and steps [s0, s0 + S_len) of buf (B, in_C, in_S)."""
    B, in_C, in_S = buf.shape
    cnt, s, q = state
    _lib.call("vt_stats_accum", buf[:, c_off:].data_ptr(), B, C, in_C, in_S, s0, S_len,
              None if kinds is None else kinds.data_ptr(), 1e-6, cnt.data_ptr(), s.data_ptr(), q.data_ptr(),
              work.data_ptr(), work.numel() * 8, _lib.stream())


def new_state(C):
    return (torch.zeros(C, dtype=torch.int64, device="cuda"), torch.zeros(C, dtype=torch.float64, device="cuda"),
            torch.zeros(C, dtype=torch.float64, device="cuda"))


def host(state):
    return tuple(t.cpu().numpy() for t in state)


def workspace(B, C, S_len):
    import ctypes
    n = ctypes.c_int64()
    _lib.call("vt_stats_workspace_bytes", B, C, S_len, ctypes.byref(n))
    return torch.full((n.value // 8,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("stats_accum_b5")


def fixture_accumulator(fx):
    acc = StatsAccumulator(default_fields(), "cuda", trim=3, step=16)
    for lo, hi in ((0, 3), (3, 5)):
        for f in SINGLE + MULTI:
            acc.update(f, dev(fx[f"in_{f}"][lo:hi]))
    return acc


# ------------------------------------------------------------------ 1. the reference fixture
def test_kernel_matches_reference_sums(fx):
    acc = fixture_accumulator(fx)
    st = acc.host_state()
    for f in SINGLE + MULTI:
        x = fx[f"in_{f}"]
        kinds = channel_kinds(f, x.shape[1]) if f in MULTI else [0]
        x = x[:, :, 3:-3] if f in MULTI else x[:, None, 48:-48]
        _, _, own_q, own_a = np_state(x, kinds)
        check_state(st[f], (fx[f"ref_{f}_count"], fx[f"ref_{f}_sum"], fx[f"ref_{f}_sum_squares"], own_a), f)
        # the restatement's own sum of squares is the scale of the second bound
        assert np.all(np.abs(st[f][2] - fx[f"ref_{f}_sum_squares"]) <= REL * own_q), f


def test_finalised_statistics_match_reference(fx):
    acc = fixture_accumulator(fx)
    out = acc.finalize()
    for f in MULTI:
        assert out[f + "_mean"].dtype == np.float32 and out[f + "_variance"].dtype == np.float32
        assert np.array_equal(out[f + "_count"], fx[f"ref_{f}_count"])
        assert ulp_apart(out[f + "_mean"], fx[f"ref_{f}_mean"]).max() <= 1, f
        assert ulp_apart(out[f + "_variance"], fx[f"ref_{f}_variance"]).max() <= 1, f
    for f in SINGLE:
        assert isinstance(out[f + "_mean"], float) and out[f + "_count"] == int(fx[f"ref_{f}_count"][0])
        assert ulp_apart(out[f + "_mean"], fx[f"ref_{f}_mean"]).max() <= 1, f
        assert ulp_apart(out[f + "_variance"], fx[f"ref_{f}_variance"]).max() <= 1, f
    dead = int(np.nonzero(fx["ref_fhr_ph_count"] == 0)[0][0])
    assert out["fhr_ph_count"][dead] == 0 and out["fhr_ph_mean"][dead] == 0 and out["fhr_ph_variance"][dead] == 0
    assert acc.n_windows == 5


# ------------------------------------------------------------------ 2. layout and tiling edges
@pytest.mark.parametrize("S_len", [18, 70])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 43, 130])
def test_channel_subview_and_step_window(C, B, S_len):
    rng = np.random.default_rng(1000 * C + 10 * B + S_len)
    c_off, s0 = 2, 4
    x = messy(rng, (B, C + 5, S_len + 7))
    kinds = (np.arange(C) % 3).astype(np.int32)
    state = new_state(C)
    accum_view(dev(x), c_off, C, s0, S_len, dev(kinds), state, workspace(B, C, S_len))
    check_state(host(state), np_state(x[:, c_off:c_off + C, s0:s0 + S_len], kinds)[:4])


def test_many_row_chunks_per_channel():
    rows, _ = chunking()
    B, C, S_len = 2 * rows + 5, 2, 18   # 3 partials per channel, the last one short
    rng = np.random.default_rng(7)
    x = messy(rng, (B, C + 1, S_len + 2))
    kinds = np.array([2, 1], np.int32)
    state = new_state(C)
    accum_view(dev(x), 1, C, 1, S_len, dev(kinds), state, workspace(B, C, S_len))
    check_state(host(state), np_state(x[:, 1:1 + C, 1:1 + S_len], kinds)[:4])


def test_raw_rows_span_column_chunks():
    _, cols = chunking()
    rows, N, stride = 3, 2 * cols + 70, 2 * cols + 300   # 3 column chunks, the last one short
    rng = np.random.default_rng(8)
    x = (140.0 + 20.0 * rng.standard_normal((rows, stride))).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    x[1, 100] = np.inf
    xd = dev(x)
    cnt, s, q = new_state(1)
    w = workspace(rows, 1, N)
    _lib.call("vt_stats_accum_raw", xd.data_ptr() + 4 * 50, rows, stride, N, cnt.data_ptr(), s.data_ptr(),
              q.data_ptr(), w.data_ptr(), w.numel() * 8, _lib.stream())
    check_state(host((cnt, s, q)), np_state(x[:, None, 50:50 + N], [0])[:4])


# ------------------------------------------------------------------ 3. accumulation
def test_two_updates_equal_one_and_rejected_call_leaves_state():
    rng = np.random.default_rng(3)
    x = messy(rng, (6, 43, 24))
    kinds = channel_kinds("fhr_st", 43)
    fields = {"fhr_st": (43, kinds)}
    whole, halves = StatsAccumulator(fields, "cuda", trim=3), StatsAccumulator(fields, "cuda", trim=3)
    whole.update("fhr_st", dev(x))
    halves.update("fhr_st", dev(x[:3]))
    halves.update("fhr_st", dev(x[3:]))
    want = np_state(x[:, :, 3:-3], kinds)
    hw, hh = whole.host_state()["fhr_st"], halves.host_state()["fhr_st"]
    check_state(hw, want[:4], "whole")
    check_state(hh, want[:4], "halves")
    assert np.array_equal(hw[0], hh[0])
    # validation failures: the wrong channel count (Python), then a short workspace (C ABI)
    with pytest.raises(ValueError):
        halves.update("fhr_st", dev(x[:, :40]))
    cnt, s, q = halves.state("fhr_st")
    w = workspace(6, 43, 18)
    with pytest.raises(ValueError):
        _lib.call("vt_stats_accum", dev(x).data_ptr(), 6, 43, 43, 24, 3, 18, None, 1e-6, cnt.data_ptr(), s.data_ptr(),
                  q.data_ptr(), w.data_ptr(), w.numel() * 8 - 8, _lib.stream())
    with pytest.raises(ValueError):
        _lib.call("vt_stats_accum", dev(x).data_ptr(), 6, 43, 43, 24, 8, 18, None, 1e-6, cnt.data_ptr(), s.data_ptr(),
                  q.data_ptr(), w.data_ptr(), w.numel() * 8, _lib.stream())
    after = halves.host_state()["fhr_st"]
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(after, hh))
    assert halves.windows["fhr_st"] == 6


def test_merge_adds_states():
    rng = np.random.default_rng(4)
    x = messy(rng, (4, 44, 20))
    fields = {"fhr_ph": (44, channel_kinds("fhr_ph", 44))}
    a, b, whole = (StatsAccumulator(fields, "cuda") for _ in range(3))
    a.update("fhr_ph", dev(x[:2]))
    b.update("fhr_ph", dev(x[2:]))
    whole.update("fhr_ph", dev(x))
    a.merge(b)
    want = np_state(x, fields["fhr_ph"][1])
    check_state(a.host_state()["fhr_ph"], want[:4], "merged")
    assert np.array_equal(a.host_state()["fhr_ph"][0], whole.host_state()["fhr_ph"][0]) and a.n_windows == 4


# ------------------------------------------------------------------ 4. determinism
def test_bitwise_repeatable_whatever_the_workspace_holds(fx):
    rows, _ = chunking()
    rng = np.random.default_rng(5)
    big = dev(messy(rng, (2 * rows + 3, 130, 24)))
    runs = []
    acc = StatsAccumulator(default_fields(), "cuda", trim=3, step=16)
    for fill in (None, "ff", "nan"):   # first run: whatever the allocator returned
        acc.reset()
        for w in acc._work.values():
            if fill == "ff":
                w.view(torch.uint8).fill_(0xFF)
            elif fill == "nan":
                w.fill_(float("nan"))
        for lo, hi in ((0, 3), (3, 5)):
            for f in SINGLE + MULTI:
                acc.update(f, dev(fx[f"in_{f}"][lo:hi]))
        acc.update("fhr_up_ph", big)
        runs.append((acc._count.cpu().numpy().copy(), acc._sums.cpu().numpy().copy()))
    for r in runs[1:]:
        assert np.array_equal(runs[0][0], r[0])
        assert np.array_equal(runs[0][1].view(np.int64), r[1].view(np.int64))
    assert np.isfinite(runs[0][1]).all() and runs[0][0].min() >= 0


# ------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def plan():
    return FrontEndPlan(11, 4, 16, 4096)


def test_fit_stats_on_the_front_ends_own_buffers(plan, tmp_path):
    trim = 30
    batches = [dev(synthetic.batch(0, 2, 4096)), dev(synthetic.batch(2, 2, 4096))]
    fe = FrontEnd(plan, stats=None, trim=trim)
    with pytest.raises(RuntimeError):
        fe(batches[0])
    got = fe.fit_stats(batches)

    # the numpy restatement on the same raw features, copied to the host
    probe = FrontEnd(plan, stats=None, trim=trim)
    feats = {f: [] for f in SINGLE + MULTI}
    for x in batches:
        r = probe.raw(x)
        torch.cuda.synchronize()
        feats["fhr_st"].append(r["fhr_st"].cpu().numpy()[:, :, trim:-trim])
        pr = r["pairs"].cpu().numpy()[:, :, trim:-trim]
        feats["fhr_ph"].append(pr[:, :probe.C_ph])
        feats["fhr_up_ph"].append(pr[:, probe.C_ph:])
        xh = x.cpu().numpy()[:, :, None, trim * 16:-trim * 16]
        feats["fhr"].append(xh[:, 0])
        feats["up"].append(xh[:, 1])
    state = fe.stats_accumulator.host_state()
    for f in SINGLE + MULTI:
        x = np.concatenate(feats[f])
        kinds = channel_kinds(f, x.shape[1])
        want = np_state(x, kinds)
        check_state(state[f], want[:4], f)
        mean, var = finalize_state(*want[:3], single=f in SINGLE)
        assert ulp_apart(got[f + "_mean"], mean).max() <= 1, f
        assert ulp_apart(got[f + "_variance"], var).max() <= 1, f
    assert state["fhr_st"][0].min() == 4 * (plan.S - 2 * trim) and state["fhr"][0][0] == 4 * (4096 - 32 * trim)

    # a side stream for the cross pairs changes no bit
    fe_side = FrontEnd(plan, stats=None, trim=trim)
    got_side = fe_side.fit_stats(batches, side=torch.cuda.Stream())
    assert got.keys() == got_side.keys()
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(got_side[k])), k
    st_side = fe_side.stats_accumulator.host_state()
    for f in SINGLE + MULTI:
        assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(state[f], st_side[f])), f

    # fe(x) now runs, and the saved file gives the same normalised batch bit for bit
    path = str(tmp_path / "stats_fit.npz")
    fe.stats_accumulator.save(path)
    saved = dict(np.load(path, allow_pickle=False))
    assert int(saved["n_windows"]) == 4
    y = fe(batches[0])
    z = FrontEnd(plan, saved, trim=trim)(batches[0])
    for k in y:
        assert torch.isfinite(y[k]).all(), k
        assert torch.equal(y[k], z[k]), k


def test_training_step_on_fitted_statistics(plan):
    """fit_stats replaces the shipped synthetic statistics: raw windows -> fe(x) -> Trainer.step."""
    from vaeteb.model import SeqVaeTeb
    from vaeteb.train import Trainer
    x = dev(synthetic.batch(0, 4, 4096))
    fe = FrontEnd(plan)
    fe.fit_stats([x[:2], x[2:]])
    torch.manual_seed(0)
    m = SeqVaeTeb(sequence_length=plan.S, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                  cross_phase_channels=fe.C_x).cuda()
    tr = Trainer(m, lr=1e-3, frontend=fe)
    eps = torch.randn(4, plan.S, 32, generator=torch.Generator().manual_seed(1)).cuda()
    L = tr.step({"x": x}, eps=eps)
    assert np.isfinite(L["total_loss"].item())


def test_calculator_facade_on_feature_dicts_and_windows(fx, plan):
    from vaeteb.stats import DatasetStatsCalculator
    calc = DatasetStatsCalculator(trim_minutes=0.2, device="cuda")
    fields = SINGLE + MULTI
    res = calc.calculate_stats({f: fx[f"in_{f}"][lo:hi] for f in fields} for lo, hi in ((0, 3), (3, 5)))
    assert list(res) == calc.stats_fields
    for f in MULTI:
        assert np.array_equal(res[f]["channel_counts"], fx[f"ref_{f}_count"])
        assert res[f]["count"] == int(fx[f"ref_{f}_count"].sum()) and res[f]["n_channels"] == fx[f"in_{f}"].shape[1]
        assert ulp_apart(res[f]["mean"], fx[f"ref_{f}_mean"]).max() <= 1
        assert ulp_apart(res[f]["variance"], fx[f"ref_{f}_variance"]).max() <= 1
        assert res[f]["shape"] == (fx[f"in_{f}"].shape[1], 18)
    assert res["fhr_st"]["regular_channels"] == [0] and res["fhr_st"]["log_channels"] == list(range(1, 43))
    assert res["fhr_ph"]["asinh_channels"] == list(range(44))
    for f in SINGLE:
        assert res[f]["count"] == int(fx[f"ref_{f}_count"][0]) and res[f]["shape"] == (288,)
        assert ulp_apart(res[f]["mean"], fx[f"ref_{f}_mean"]).max() <= 1
    # window batches through the online front-end: the same statistics as fit_stats
    x = dev(synthetic.batch(0, 2, 4096))
    fe = FrontEnd(plan, trim=30)
    want = fe.fit_stats([x])
    res = DatasetStatsCalculator(trim_minutes=2, device="cuda").calculate_stats([x], frontend=FrontEnd(plan, trim=30))
    for f in MULTI:
        assert np.array_equal(res[f]["mean"], want[f + "_mean"])
        assert res[f]["shape"] == (len(want[f + "_mean"]), 196)
    assert res["fhr"]["mean"] == want["fhr_mean"] and res["up"]["variance"] == want["up_variance"]


# ------------------------------------------------------------------ 6. stream capture
def test_update_is_capturable(fx):
    fields = {"fhr_up_ph": default_fields()["fhr_up_ph"], "fhr": None}
    xs, xr = dev(fx["in_fhr_up_ph"]), dev(fx["in_fhr"])
    eager, graphed = (StatsAccumulator(fields, "cuda", trim=3, step=16) for _ in range(2))
    eager.update("fhr_up_ph", xs)
    eager.update("fhr", xr)
    # size the workspaces first: nothing is allocated while capturing
    graphed.update("fhr_up_ph", xs)
    graphed.update("fhr", xr)
    graphed.reset()
    torch.cuda.synchronize()
    work = {k: v.data_ptr() for k, v in graphed._work.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update("fhr_up_ph", xs)
        graphed.update("fhr", xr)
    assert work == {k: v.data_ptr() for k, v in graphed._work.items()}
    torch.cuda.synchronize()
    assert int(graphed._count.sum()) == 0   # capture enqueues, it does not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed._count, eager._count)
    assert torch.equal(graphed._sums.view(torch.int64), eager._sums.view(torch.int64))
    assert int(eager._count.sum()) > 0
