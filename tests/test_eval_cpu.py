"""The evaluation sweep (vaeteb.evaluate), the parts that need no GPU: the self-consistency of the
reference fixture tests/golden/eval_gain_s16_b3.npz (tools/gen_golden_eval.py) through the model
oracle, the condition the fixture was built to meet, the reference's float32 numpy metrics against a
float64 evaluation of the same rows, the argument validation of the three new C entry points, and
the host-side pieces (EvalSweepResult.means, the gain list).

Bounds:
* model oracle: mu_pr rel-L2 < 1e-5, te np.allclose(rtol=1e-5, atol=1e-6): what tests/test_oracle.py
  holds the same oracle to against the reference's own goldens (test_transfer_entropy; the fixture
  holds each row's mean, and a mean of values each within that bound is within it).
* float64 metrics vs the reference's float32 numpy lines: np.var / np.mean of 256 float32 values
  (pairwise float32 sums) carry a few float32 roundings, <= 2e-6 relative on var_res, var_y, mse and
  sig; vaf = 1 - var_res/var_y then moves by <= 4e-6 (1 - vaf), plus one float32 rounding of a
  value below 1 (6e-8) where numpy keeps the difference in float32, and snr by
  10/ln(10) * 4e-6 < 2e-5 dB.
"""
import numpy as np
import pytest
import torch

from golden_util import det_fill_
from oracle import model_ref as M
from vaeteb import _lib
from vaeteb import evaluate as E

GAINS = [0.0, 0.001, 0.01, 1.0, 2.0, -1.0]
DISTINCT = [0, 1, 2, 3, 5]      # {0, 0.001, 0.01, 1, -1}: gain 2 is the near-invariant case


@pytest.fixture(scope="module")
def g(golden):
    d = golden("eval_gain_s16_b3")
    assert list(d["gains"]) == GAINS
    assert d["mu_pr"].shape == (3, 6, 256) and d["eps"].shape == (3, 16, 32) and d["y_raw"].shape == (3, 256)
    for k in ("te", "vaf", "mse", "snr", "vaf_unclamped"):
        assert d[k].shape == (3, 6), k
    return d


def test_fixture_through_the_model_oracle(g):
    m = det_fill_(M.SeqVaeTebRef(16))
    sd = m.state_dict()
    names = list(g["bn_names"])
    assert any(k.startswith("decoder.") for k in names)       # the decoder's buffers are stored too
    assert sorted(names) == sorted(k for k in sd if k.endswith("running_mean") or k.endswith("running_var"))
    for i, k in enumerate(names):
        sd[k].copy_(torch.from_numpy(g[f"bn_{i}"]))
    m.eval()
    T = torch.from_numpy
    with torch.no_grad():
        for k, gain in enumerate(GAINS):
            xs = T(g["x_ph"]) * float(gain)
            mu = m(T(g["y_st"]), T(g["y_ph"]), xs, T(g["eps"]))["mu_pr"].double().numpy()
            ref = g["mu_pr"][:, k].astype(np.float64)
            err = np.linalg.norm(mu - ref) / np.linalg.norm(ref)
            te = m.measure_transfer_entropy(T(g["y_st"]), T(g["y_ph"]), xs).mean(dim=(1, 2)).numpy()
            print(f"gain {gain}: mu_pr rel-L2 {err:.2e}, te max rel {np.abs(te / g['te'][:, k] - 1).max():.2e}")
            assert err < 1e-5, (gain, err)
            assert np.allclose(te, g["te"][:, k], rtol=1e-5, atol=1e-6), gain


def test_fixture_condition(g):
    """Every row's reference VAF is strictly inside the clamp, and rows of different gains really
    differ (a sweep that ignored the gain cannot pass)."""
    vu = g["vaf_unclamped"]
    assert ((vu > 0.05) & (vu < 0.95)).all(), vu
    assert np.array_equal(g["vaf"], vu)
    mu = g["mu_pr"].astype(np.float64)
    for b in range(3):
        for i in DISTINCT:
            for j in DISTINCT:
                if i < j:
                    d = np.linalg.norm(mu[b, i] - mu[b, j]) / np.linalg.norm(mu[b, j])
                    assert d > 1e-2, (b, GAINS[i], GAINS[j], d)


def metrics64(y, pr):
    """The metric definitions in float64 on float32 rows, the residual formed in float32:
    (vaf, mse, snr_db, vaf_unclamped), shaped like pr's leading dimensions; y broadcasts over K."""
    y = np.asarray(y, np.float32)
    pr = np.asarray(pr, np.float32)
    yb = y[:, None, :] if pr.ndim == 3 else y
    res = (yb - pr).astype(np.float64)
    y64 = np.broadcast_to(yb.astype(np.float64), res.shape)
    var_y, var_r = y64.var(-1), res.var(-1)
    mse, sig = (res ** 2).mean(-1), (y64 ** 2).mean(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        vu = np.where(var_y > 1e-12, 1.0 - var_r / np.where(var_y > 1e-12, var_y, 1.0), 0.0)
        snr = np.where(mse > 1e-12, 10.0 * np.log10(sig / np.where(mse > 1e-12, mse, 1.0)), 100.0)
    return np.clip(vu, 0.0, 1.0), mse, snr, vu


def test_stored_metrics_are_the_definitions_in_float64(g):
    vaf, mse, snr, vu = metrics64(g["y_raw"], g["mu_pr"])
    assert np.all(np.abs(mse - g["mse"]) <= 2e-6 * mse)
    assert np.all(np.abs(vu - g["vaf_unclamped"]) <= 4e-6 * (1 - vu) + 6e-8)
    assert np.all(np.abs(vaf - g["vaf"]) <= 4e-6 * (1 - vu) + 6e-8)
    assert np.all(np.abs(snr - g["snr"]) <= 2e-5)


def test_eval_entry_points_reject_bad_arguments_without_a_gpu():
    """Validation comes before any device work (the pattern of
    test_new_entry_points_reject_bad_arguments_without_a_gpu): empty sizes, K <= 0, B*K >= 2^31, null
    required pointers; the nullable outputs are accepted up to the launch."""
    P = 0x1000   # never dereferenced: every call below fails validation first
    ok_scale = dict(x=P, B=2, K=5, n=2080, g=P, out=P)

    def scale(**kw):
        a = dict(ok_scale, **kw)
        _lib.call("vt_eval_scale_rows", a["x"], a["B"], a["K"], a["n"], a["g"], a["out"], None)
    for bad in (dict(B=0), dict(B=-1), dict(K=0), dict(K=-3), dict(n=0), dict(x=None), dict(g=None), dict(out=None),
                dict(B=1 << 30, K=2), dict(B=1 << 40, K=1)):
        with pytest.raises(ValueError):
            scale(**bad)

    ok_lat = dict(mc=P, lq=P, my=P, lp=P, eps=P, B=2, K=4, n=512, z=P, mp=None, te=P, kl=None)

    def latent(**kw):
        a = dict(ok_lat, **kw)
        _lib.call("vt_te_latent_rows", a["mc"], a["lq"], a["my"], a["lp"], a["eps"], a["B"], a["K"], a["n"], a["z"],
                  a["mp"], a["te"], a["kl"], None)
    for bad in (dict(B=0), dict(K=0), dict(K=-2), dict(n=0), dict(mc=None), dict(lq=None), dict(my=None),
                dict(lp=None), dict(eps=None), dict(z=None), dict(te=None), dict(B=1 << 30, K=2)):
        with pytest.raises(ValueError):
            latent(**bad)

    ok_met = dict(y=P, pr=P, B=2, K=4, n=4800, out=P)

    def met(**kw):
        a = dict(ok_met, **kw)
        _lib.call("vt_recon_metrics_rows", a["y"], a["pr"], a["B"], a["K"], a["n"], a["out"], None)
    for bad in (dict(B=0), dict(K=0), dict(K=-1), dict(n=0), dict(n=-5), dict(y=None), dict(pr=None), dict(out=None),
                dict(B=1 << 30, K=2)):
        with pytest.raises(ValueError):
            met(**bad)


def test_means_are_per_gain_means_over_recordings():
    """ref/model/graph_model.py:1862-1864: sums over the samples divided by their count, per gain."""
    rng = np.random.default_rng(3)
    a = {k: torch.from_numpy(rng.standard_normal((5, 3)).astype(np.float32))
         for k in ("te", "vaf", "mse", "snr", "vaf_unclamped")}
    r = E.EvalSweepResult(np.array([0.0, 1.0, 2.0]), **a)
    assert r.mu_pr is None and r.kl is None
    mean = r.means()
    assert sorted(mean) == sorted(a)
    for k, v in a.items():
        assert mean[k].shape == (3,)
        assert np.allclose(mean[k].numpy(), v.numpy().sum(0) / 5, rtol=1e-6, atol=1e-7), k


def test_gain_lists():
    assert E.DEFAULT_GAINS == (0.0, 0.5, 1.0, 1.5, 2.0) and E.ABLATION_GAINS == (1.0, 0.0)
    for ok in (E.DEFAULT_GAINS, [1], (1.0, 0.0), np.array([0.001, -1.0]), range(3)):
        got = E.check_gains(ok)
        assert got.dtype == np.float64 and got.ndim == 1 and list(got) == [float(v) for v in ok]
    for bad in ([], (), [[1.0, 2.0]], [float("nan")], [1.0, float("inf")], [1e39]):
        with pytest.raises(ValueError):
            E.check_gains(bad)
    with pytest.raises(ValueError):
        E.GainSweep(None, rows_per_launch=0)
    s = E.GainSweep(None, rows_per_launch=6)
    assert s._chunks(3, 6) == [(0, 1, 0, 6), (1, 1, 0, 6), (2, 1, 0, 6)]
    assert s._chunks(3, 2) == [(0, 3, 0, 2)]
    s = E.GainSweep(None, rows_per_launch=4)
    assert s._chunks(2, 6) == [(0, 1, 0, 4), (0, 1, 4, 2), (1, 1, 0, 4), (1, 1, 4, 2)]
