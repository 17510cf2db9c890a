"""The predictive distribution without a GPU: the float64 reference of the definitions
(tests/predictive_ref.py) against closed forms, and the package side (vaeteb.predictive imports, its
argument errors come before any device call, the new prototypes are bound and validate their sizes
on the host)."""
import math

import numpy as np
import pytest
import torch

import predictive_ref as R


def _case(seed, B, K, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.standard_normal((B, n))
    mu = y[:, None] + 0.6 * rng.standard_normal((B, K, n))
    lv = rng.uniform(-2.5, 2.5, (B, K, n))
    return rng, y, mu, lv


# ------------------------------------------------------------------ the reference against closed forms
def test_single_draw_is_the_gaussian_formula():
    rng, y, mu, lv = _case(1, 2, 1, 50)
    logw = rng.standard_normal((2, 1))
    r = R.predictive(y, mu, lv, logw)
    nll = 0.5 * (math.log(2 * math.pi) + lv[:, 0] + (y - mu[:, 0]) ** 2 / np.exp(lv[:, 0]))
    np.testing.assert_allclose(r["nll_mixture"], nll.mean(-1), rtol=1e-13)
    np.testing.assert_allclose(r["nll_moment"], nll.mean(-1), rtol=1e-13)       # one component: v = exp(lv)
    np.testing.assert_allclose(r["iwae"], r["elbo"], rtol=1e-13)
    np.testing.assert_allclose(r["elbo"], -nll.sum(-1) + logw[:, 0], rtol=1e-13)
    assert (r["var_epistemic"] == 0).all()
    np.testing.assert_allclose(r["sharpness"], np.exp(0.5 * lv[:, 0]).mean(-1), rtol=1e-13)


def test_iwae_is_at_least_the_elbo():
    for K in (2, 7, 16):
        rng, y, mu, lv = _case(10 + K, 3, K, 40)
        logw = rng.standard_normal((3, K))
        r = R.predictive(y, mu, lv, logw)
        assert (r["iwae"] >= r["elbo"]).all() and (r["iwae"] > r["elbo"] + 1e-9).any()
        assert (r["iwae"] <= (r["ll"] + logw).max(-1)).all()          # and never above the best draw


def test_law_of_total_variance_on_a_hand_case():
    """Two components N(-1, 1) and N(3, 4) with equal weight: mean 1, E[var] = 2.5, var of the
    means = 4, mixture variance = E[x^2] - 1 = ((1 + 1) + (4 + 9)) / 2 - 1 = 6.5."""
    mu = np.array([[[-1.0], [3.0]]])
    lv = np.log(np.array([[[1.0], [4.0]]]))
    r = R.predictive(np.zeros((1, 1)), mu, lv)
    assert r["mean"][0, 0] == 1.0
    assert abs(r["var_aleatoric"][0, 0] - 2.5) < 1e-15 and r["var_epistemic"][0, 0] == 4.0
    second_moment = 0.5 * ((1.0 + 1.0) + (4.0 + 9.0))
    assert abs(r["var_aleatoric"][0, 0] + r["var_epistemic"][0, 0] - (second_moment - 1.0)) < 1e-14
    # density and CDF of that mixture at 0
    pdf = 0.5 * (math.exp(-0.5) / math.sqrt(2 * math.pi) + math.exp(-9 / 8) / math.sqrt(8 * math.pi))
    assert abs(r["logdens"][0, 0] - math.log(pdf)) < 1e-14
    cdf = 0.5 * (0.5 * math.erfc(-1 / math.sqrt(2)) + 0.5 * math.erfc(1.5 / math.sqrt(2)))
    assert abs(r["pit"][0, 0] - cdf) < 1e-15


def test_pit_is_uniform_when_y_comes_from_the_mixture():
    rng = np.random.Generator(np.random.PCG64(5))
    K, n, bins = 5, 20000, 20
    mu = rng.standard_normal((1, K, n))
    lv = rng.uniform(-2.5, 2.5, (1, K, n))
    pick = rng.integers(0, K, n)
    i = np.arange(n)
    y = (mu[0, pick, i] + np.exp(0.5 * lv[0, pick, i]) * rng.standard_normal(n))[None]
    r = R.predictive(y, mu, lv, bins=bins, levels=(0.5, 0.9))
    assert r["pit_hist"].sum() == n
    chi2 = ((r["pit_hist"][0] - n / bins) ** 2 / (n / bins)).sum()
    assert chi2 < 60.0, chi2                      # 19 degrees of freedom: mean 19, 60 is beyond 1e-5
    assert abs(r["coverage"][0, 0] - 0.5) < 0.02 and abs(r["coverage"][0, 1] - 0.9) < 0.02


def test_logdens_survives_a_draw_far_below_the_others():
    y = np.zeros((1, 3))
    mu = np.zeros((1, 3, 3))
    lv = np.zeros((1, 3, 3))
    mu[0, 1] = 60.0                               # l = -1800.9: exp underflows against the others
    r = R.predictive(y, mu, lv)
    assert (r["l"][0, 0] - r["l"][0, 1] > 745).all()
    want = math.log(2.0) - 0.5 * math.log(2 * math.pi) - math.log(3.0)      # two equal maxima
    assert np.isfinite(r["logdens"]).all() and np.abs(r["logdens"] - want).max() < 1e-15
    mu[0, 2] = -70.0                              # one maximum: max - log K
    r = R.predictive(y, mu, lv)
    assert np.abs(r["logdens"] - (-0.5 * math.log(2 * math.pi) - math.log(3.0))).max() < 1e-15
    assert R.lse(np.array([[-np.inf, -np.inf]]), 1)[0] == -np.inf


def test_pit_of_one_goes_in_the_last_bin_and_edges_are_found():
    r = R.predictive(np.array([[100.0, 0.0]]), np.zeros((1, 1, 2)), np.zeros((1, 1, 2)), bins=4, levels=(0.5,))
    assert r["pit"][0, 0] == 1.0 and list(r["pit_hist"][0]) == [0, 0, 1, 1]
    assert r["coverage"][0, 0] == 0.5             # pit 0.5 is inside every central interval, 1.0 in none
    assert R.near_edge(r["pit"], 4, (0.5,)) == 1  # 0.5 is a bin edge


def test_logw_is_log_p_minus_log_q():
    rng = np.random.Generator(np.random.PCG64(9))
    B, K, m = 2, 3, 11
    mu_q, mu_p = rng.standard_normal((B, m)), rng.standard_normal((B, m))
    lv_q, lv_p = rng.uniform(-2, 2, (B, m)), rng.uniform(-2, 2, (B, m))
    eps = rng.standard_normal((B, K, m))
    z = mu_q[:, None] + eps * np.exp(0.5 * lv_q)[:, None]
    w, mag = R.logw(lv_q, lv_p, eps, z, mu_p)
    logn = lambda x, mu, lv: -0.5 * (math.log(2 * math.pi) + lv + (x - mu) ** 2 / np.exp(lv))
    want = (logn(z, mu_p[:, None], lv_p[:, None]) - logn(z, mu_q[:, None], lv_q[:, None])).sum(-1)
    np.testing.assert_allclose(w, want, rtol=0, atol=1e-12 * mag.max())
    assert (mag >= np.abs(w)).all()


# ------------------------------------------------------------------ the package side
def test_module_imports_and_documents_its_result():
    from vaeteb import predictive as P
    assert P.Predictive and P.PredictiveResult and P.DEFAULT_LEVELS == (0.5, 0.9, 0.95)
    for name in ("mean", "var_aleatoric", "var_epistemic", "nll_mixture", "nll_moment", "sharpness", "pit_hist",
                 "coverage", "elbo", "iwae", "ll", "logw", "vaf", "mse", "snr", "vaf_unclamped", "mu_pr", "logvar_pr"):
        assert name in P.PredictiveResult.__slots__ and name in P.PredictiveResult.__doc__, name
    r = P.PredictiveResult(var_aleatoric=torch.full((1, 2), 3.0), var_epistemic=torch.full((1, 2), 1.0))
    assert torch.equal(r.sd, torch.full((1, 2), 2.0)) and r.elbo is None
    from vaeteb.model import SeqVaeTeb
    assert callable(SeqVaeTeb.predictive)


class _NoDevice:
    """Stands for the model where an argument error must come first: touching it is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def _fields(B=2, S=16):
    return [torch.zeros(B, S, c) for c in (43, 44, 130)] + [torch.zeros(B, 16 * S)]


def test_argument_errors_come_before_any_device_call():
    from vaeteb.predictive import Predictive
    with pytest.raises(ValueError, match="rows_per_launch"):
        Predictive(_NoDevice(), rows_per_launch=0)
    p = Predictive(_NoDevice())
    f = _fields()
    with pytest.raises(ValueError, match="device tensor"):              # CPU tensors
        p(*f)
    with pytest.raises(ValueError, match="source"):
        p(*f, source="likelihood")
    with pytest.raises(ValueError, match="n_samples"):                  # K > 64
        p(*f, n_samples=65)
    with pytest.raises(ValueError, match="n_samples"):
        p(*f, n_samples=-1)
    with pytest.raises(ValueError, match="rows_per_launch"):            # K > rows_per_launch
        Predictive(_NoDevice(), rows_per_launch=8)(*f, n_samples=9)
    for bad in ((0.0,), (1.0,), (0.5, 1.5), (-0.1,), (float("nan"),)):
        with pytest.raises(ValueError, match="levels"):
            p(*f, levels=bad)
    with pytest.raises(ValueError, match="levels"):
        p(*f, levels=[0.1 * i for i in range(1, 10)])                   # more than 8
    with pytest.raises(ValueError, match="bins"):
        p(*f, bins=0)
    with pytest.raises(ValueError, match="bins"):
        p(*f, bins=257)
    with pytest.raises(ValueError, match="device tensor"):              # wrong rank, still before the model
        p(f[0], f[1], f[2], torch.zeros(2, 16, 16, 1, 1))
    with pytest.raises(ValueError, match="device tensor"):              # wrong dtype
        p(f[0].double(), f[1], f[2], f[3])
    with pytest.raises(ValueError, match="device tensor"):              # recordings disagree
        p(f[0][:1], f[1], f[2], f[3])


def test_model_entry_needs_the_fields_or_the_frontend():
    from vaeteb.model import SeqVaeTeb
    m = SeqVaeTeb(sequence_length=16)
    f = _fields()
    with pytest.raises(ValueError):
        m.predictive(f[0], f[1], f[2])
    with pytest.raises(ValueError):
        m.predictive(*f, frontend=object())
    with pytest.raises(ValueError, match="device tensor"):
        m.predictive(*f, n_samples=4)
    assert m.training                                                    # refused before eval() was set


def test_prototypes_are_bound_and_validate_on_the_host():
    from vaeteb import _lib
    protos = _lib.parse_header()
    assert protos["vt_pred_tile"] == ("int", [])
    assert len(protos["vt_pred_draw_rows"][1]) == 11
    assert len(protos["vt_pred_mixture_rows"][1]) == 16 and protos["vt_pred_mixture_rows"][1][7] == "double*"
    assert len(protos["vt_pred_finish"][1]) == 12 and protos["vt_pred_finish"][1][9] == "int*"
    fns = _lib.lib().fns
    T = fns["vt_pred_tile"]()
    assert T >= 64 and T % 4 == 0
    p = 16                                   # any non-null address: validation returns before it is used
    draw = lambda **k: _lib.call("vt_pred_draw_rows", *[{**dict(mu=p, lv=p, eps=p, mu_p=None, lv_p=None, B=2, K=3,
                                                                 m=8, z=p, logw=p, st=None), **k}[a] for a in
                                                        ("mu", "lv", "eps", "mu_p", "lv_p", "B", "K", "m", "z", "logw",
                                                         "st")])
    for bad in (dict(B=0), dict(K=0), dict(m=0), dict(mu=None), dict(eps=None), dict(z=None), dict(logw=None),
                dict(mu_p=p), dict(lv_p=p), dict(B=1 << 30, K=4)):
        with pytest.raises(ValueError):
            draw(**bad)
    mix = lambda **k: _lib.call("vt_pred_mixture_rows", *[{**dict(y=p, mu=p, lv=p, B=2, K=3, n=100, bins=20, lev=p,
                                                                   nl=3, mean=p, va=p, ve=p, pit=None, ld=None, ws=p,
                                                                   st=None), **k}[a] for a in
                                                          ("y", "mu", "lv", "B", "K", "n", "bins", "lev", "nl", "mean",
                                                           "va", "ve", "pit", "ld", "ws", "st")])
    for bad in (dict(K=65), dict(K=0), dict(B=0), dict(B=65536), dict(n=0), dict(bins=0), dict(bins=257), dict(nl=9),
                dict(nl=-1), dict(y=None), dict(mu=None), dict(lv=None), dict(mean=None), dict(va=None), dict(ve=None),
                dict(ws=None), dict(lev=None)):
        with pytest.raises(ValueError):
            mix(**bad)
    fin = lambda **k: _lib.call("vt_pred_finish", *[{**dict(ws=p, logw=None, B=2, K=3, n=100, bins=20, nl=3, out=p,
                                                             ll=p, hist=p, cov=p, st=None), **k}[a] for a in
                                                    ("ws", "logw", "B", "K", "n", "bins", "nl", "out", "ll", "hist",
                                                     "cov", "st")])
    for bad in (dict(K=65), dict(B=0), dict(n=0), dict(bins=0), dict(nl=9), dict(ws=None), dict(out=None),
                dict(ll=None), dict(hist=None), dict(cov=None)):
        with pytest.raises(ValueError):
            fin(**bad)
    with pytest.raises(ValueError, match=r"K must be in 1\.\.64, got 65"):
        mix(K=65)
