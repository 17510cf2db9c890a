"""Transfer entropy vs shift, the parts that need no GPU: the reference's shift grid, the
self-consistency of the reference fixture tests/golden/te_shift_j11_n4096*.npz
(tools/gen_golden_te_shift.py) through the two oracles, and the argument validation of the three
new C entry points.

Bounds are the ones tests/test_oracle.py holds the same oracles to against their own goldens:

* front-end oracle (test_phase_frontend): the cross-phase channels' error distribution, measured
  against a float64 evaluation on the cancellation-free scale ||lowpass(|a_i| |a_j|)||, may be at
  most twice the reference's own fp32 error (max and median over the channels).  The fixture holds
  the reference's *normalised* fp32 features only, so (a) the float64 yardstick is the oracle's own
  float64 front-end, which test_phase_frontend pins to the reference's float64 run at 1e-10, and
  (b) the reference's raw features are recovered by inverting the normalisation in float64
  (sinh(z (sigma + 1e-8) + mu): the rounding of z is part of the reference's own error).
  Direct agreement of two fp32 front-ends is not attainable (non-integer phase powers make
  atan2's branch cut a discontinuity; see the comment in test_phase_frontend), which is why that
  test, and this one, compare error distributions.
* model oracle (test_transfer_entropy): np.allclose(rtol=1e-5, atol=1e-6) on the elementwise KL;
  the fixture holds each row's mean, and a mean of values each within that bound is within it.
"""
import numpy as np
import pytest
import torch

from golden_util import det_fill_
from oracle import frontend_ref as F
from oracle import model_ref as M
from vaeteb import _lib
from vaeteb.te import left_shifts


def test_left_shifts_are_the_reference_grid():
    """ref/model/graph_model.py:1283-1287."""
    ref = (np.arange(-60, 1, 1) * 4.0).astype(int)
    got = left_shifts()
    assert got.dtype == ref.dtype and np.array_equal(got, ref) and len(got) == 61
    for mx, step, sr in ((60, 1, 4.0), (30, 2, 4.0), (7, 3, 2.5), (0, 1, 4.0), (12.9, 1.7, 4.0)):
        ref = (np.arange(-int(mx), 0 + 1, int(step)) * sr).astype(int)
        assert np.array_equal(left_shifts(mx, step, sr), ref), (mx, step, sr)


@pytest.fixture(scope="module")
def fixture(golden):
    g, gi = golden("te_shift_j11_n4096"), golden("te_shift_j11_n4096_in")
    assert g["x_ph"].shape == (2, 4, 256, 130) and g["te"].shape == (2, 4)
    assert list(g["shifts"]) == [0, -1, 7, -240] and gi["x"].shape == (2, 2, 4096)
    return g, gi


def test_fixture_features_through_the_frontend_oracle(fixture):
    g, gi = fixture
    from vaeteb.frontend import load_stats
    st = load_stats(11, 4, 16, 4096)
    x, shifts = gi["x"], g["shifts"]
    rolled = np.stack([np.stack([x[b, 0], np.roll(x[b, 1], int(s))]) for b in range(2) for s in shifts])
    fe, fe64 = F.PhaseFrontEnd(11, 4, 16, 4096), F.PhaseFrontEnd(11, 4, 16, 4096, dtype=np.float64)
    _, cm = fe.masks()
    assert int(cm.sum()) == 130
    out = fe.forward(rolled, compute_phase=False, compute_cross_phase=True, pair_subset=cm)["cross_phase_corr"]
    out64 = fe64.forward(rolled, compute_phase=False, compute_cross_phase=True, pair_subset=cm)["cross_phase_corr"]
    # the reference's raw features from its normalised ones (rows (b, k), channels first)
    mean = np.asarray(st["fhr_up_ph_mean"], np.float32).astype(np.float64)
    std = np.sqrt(np.asarray(st["fhr_up_ph_variance"], np.float32)).astype(np.float32).astype(np.float64)
    z = g["x_ph"].reshape(8, 256, 130).transpose(0, 2, 1).astype(np.float64)
    ref = np.sinh(z * (std[None, :, None] + 1e-8) + mean[None, :, None])
    a64 = fe64.analytic(rolled[:, [0, 1]])
    ii, jj = fe64.i_idx[cm], fe64.j_idx[cm]
    scale = np.sqrt((fe64._lowpass(np.abs(a64[:, 0][:, ii]) * np.abs(a64[:, 1][:, jj]) + 0j, 256) ** 2).sum(-1))
    err = np.sqrt(((out - out64) ** 2).sum(-1)) / scale
    ref_err = np.sqrt(((ref - out64) ** 2).sum(-1)) / scale
    print(f"front-end oracle err max {err.max():.3e} median {np.median(err):.3e}; "
          f"reference err max {ref_err.max():.3e} median {np.median(ref_err):.3e}")
    assert err.max() <= 2 * ref_err.max() + 1e-5
    assert np.median(err) <= 2 * np.median(ref_err) + 1e-6
    # the normalisation oracle on the oracle's own features: the channels no branch flip hit (the
    # median channel) land on the fixture to the normalisation oracle's own bound (test_normalize)
    zo = F.normalize(out, "fhr_up_ph", st["fhr_up_ph_mean"], st["fhr_up_ph_variance"])
    zr = g["x_ph"].reshape(8, 256, 130).transpose(0, 2, 1)
    assert np.isfinite(zo).all()
    print("normalised features: median abs difference", np.median(np.abs(zo - zr)))


def test_fixture_te_through_the_model_oracle(fixture):
    g, gi = fixture
    # S enters the decoder's head width only; the encoders (all the transfer entropy uses) are
    # length-agnostic, so the small model carries the same det_fill_ encoder weights
    m = det_fill_(M.SeqVaeTebRef(16))
    sd = m.state_dict()
    names = list(g["bn_names"])
    assert len(names) == 18 and not any(k.startswith("decoder.") for k in names)
    for i, k in enumerate(names):
        sd[k].copy_(torch.from_numpy(g[f"bn_{i}"]))
    T = torch.from_numpy
    te = np.zeros((2, 4))
    for b in range(2):
        for k in range(4):
            kl = m.measure_transfer_entropy(T(gi["y_st"][b:b + 1]), T(gi["y_ph"][b:b + 1]),
                                            T(np.ascontiguousarray(g["x_ph"][b:b + 1, k])))
            assert kl.shape == (1, 256, 32)
            te[b, k] = kl.mean().item()
    assert not m.training
    print("model oracle te rel err", np.abs(te - g["te"]).max() / np.abs(g["te"]).max())
    assert np.allclose(te, g["te"], rtol=1e-5, atol=1e-6)
    assert list(te.argmin(1)) == list(g["te"].argmin(1))


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    """Validation comes before any device work (the pattern of test_argument_errors_map_to_value_error):
    empty sizes, K <= 0, null pointers, a non-power-of-two n_pad."""
    P = 0x1000   # never dereferenced: every call below fails validation first
    ok_spec = dict(x=P, B=2, stride=8192, N=4096, n_pad=8192, pad_left=2048, pad_mode=0, shifts=P, K=4, tw=P, xhat=P)

    def spectrum(**kw):
        a = dict(ok_spec, **kw)
        _lib.call("vt_fe_spectrum_rolled", a["x"], a["B"], a["stride"], a["N"], a["n_pad"], a["pad_left"],
                  a["pad_mode"], a["shifts"], a["K"], a["tw"], a["xhat"], None)
    for bad in (dict(B=0), dict(K=0), dict(K=-3), dict(n_pad=8000), dict(x=None), dict(shifts=None), dict(tw=None),
                dict(xhat=None), dict(N=0), dict(stride=100), dict(pad_mode=3)):
        with pytest.raises(ValueError):
            spectrum(**bad)

    ok_pairs = dict(ai=P, nsi=70, aj=P, nsj=30, B=2, K=4, N=4096, n_pad=8192, pad_left=2048, n_pairs=130, si=P, sj=P,
                    pw=P, tw=P, phi=P, dec=16, start=128, S=256, pad_mode=0, out=P)

    def pairs(**kw):
        a = dict(ok_pairs, **kw)
        _lib.call("vt_fe_pairs_split", a["ai"], a["nsi"], a["aj"], a["nsj"], a["B"], a["K"], a["N"], a["n_pad"],
                  a["pad_left"], a["n_pairs"], a["si"], a["sj"], a["pw"], a["tw"], a["phi"], a["dec"], a["start"],
                  a["S"], a["pad_mode"], a["out"], None)
    for bad in (dict(B=0), dict(K=0), dict(K=-1), dict(n_pairs=0), dict(n_pad=6000), dict(ai=None), dict(aj=None),
                dict(si=None), dict(sj=None), dict(pw=None), dict(phi=None), dict(out=None), dict(dec=3),
                dict(nsi=0), dict(nsj=0), dict(pad_mode=5), dict(start=400)):
        with pytest.raises(ValueError):
            pairs(**bad)

    ok_kl = dict(mc=P, lq=P, my=P, lp=P, B=2, K=4, n=8192, te=P, kl=None)

    def kl_rows(**kw):
        a = dict(ok_kl, **kw)
        _lib.call("vt_te_kl_rows", a["mc"], a["lq"], a["my"], a["lp"], a["B"], a["K"], a["n"], a["te"], a["kl"], None)
    for bad in (dict(B=0), dict(K=0), dict(K=-2), dict(n=0), dict(mc=None), dict(lq=None), dict(my=None),
                dict(lp=None), dict(te=None)):
        with pytest.raises(ValueError):
            kl_rows(**bad)
