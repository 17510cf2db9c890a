"""The K-draw predictive distribution (vaeteb.predictive.Predictive; csrc/predictive.hip) on the GPU:
the three kernels against the float64 definitions (tests/predictive_ref.py) on the same float32
inputs, and Predictive end to end against the literal loop of K forwards on the same GPU model and
against the reference's forward (oracle.model_ref on the CPU).

Kernel bounds (got vs predictive_ref; every measured maximum is printed):
* z of vt_pred_draw_rows: bit-equal vt_te_latent_rows's z for mu_c = mu expanded over K, mu_y = 0.
* row sums: |ll - ref| <= 1e-6 * 1/2 sum_i (log 2pi + |lv| + d^2 e^-lv);
  |logw - ref| <= 1e-6 * 1/2 sum_j (|lv_q| + |lv_p| + eps^2 + (z - mu_p)^2 e^-lv_p): the 1e-6 the KL
  and metrics kernels are held to, applied to magnitudes so that cancellation cannot hide an error.
* nll_mixture: 1e-6 * mean_i max_k (term magnitude of l_ki) (LSE is 1-Lipschitz in the max norm).
* elbo, iwae: the largest of the bounds of the rows that enter them.
* mean: 2^-23 * mean_k |mu|.  var_aleatoric: 5e-7 relative (float32 expf within 2 ulp, plus the
  output rounding).  var_epistemic: 5e-7 relative where it exceeds 1e-10 * mean_k mu^2, >= 0 everywhere.
* nll_moment, sharpness: 2e-6 of their magnitude sums.
* pit: 1e-6 absolute (float32 argument, |t phi(t)| <= 0.25, output rounding); logdens (per sample,
  this file's own bound): 1e-6 * max_k term magnitude, as nll_mixture before its mean.
* pit_hist, coverage: counts.  A PIT the reference puts within 2e-6 of a bin edge or of
  1/2 +- level/2 may fall either side, so each test first asserts that the reference has no such
  sample for its seed (the seeds were chosen for that on the CPU), then requires equal counts.

The sample tile of vt_pred_mixture_rows is T = 1024 (vt_pred_tile, asserted): n covers 1, the wave
and workgroup sizes +-1, T - 1, T, T + 1, 2 T + 3 and the model's 4800; odd n with B = 3 puts rows
off the 16-byte grid (the scalar path), even n on it (float4).

End to end (S = 16 model of tests/test_gpu_eval.py, B = 3, K = 5): z and the encoder pieces bit-equal
the loop's; mu_pr / logvar_pr on the terms of test_sweep_matches_the_loop_fp32 (the decoder sees 15
rows here and 3 per forward in the loop): asserted equal; every result field within the kernel
bounds of predictive_ref on the loop's own mu_pr / logvar_pr; against the reference's forward
5e-5 rel-L2 per draw (the project's forward-output bound).
"""
import math

import numpy as np
import pytest
import torch

import predictive_ref as R

pytestmark = pytest.mark.gpu

T_TILE = 1024
LEVELS = (0.5, 0.9, 0.95)
NS = [1, 63, 64, 255, 256, 257, 1023, T_TILE - 1, T_TILE, T_TILE + 1, 2 * T_TILE + 3, 4800]
CASES = sorted({(n, 7, 3 if n % 2 else 1) for n in NS} | {(2 * T_TILE + 3, K, 3) for K in (1, 2, 7, 16, 64)}
               | {(257, 16, 1), (4800, 16, 3), (64, 2, 3)})
# seeds moved off a PIT within 2e-6 of an edge (found on the CPU; the tests assert there is none)
RESEED = {(1024, 7, 1): 1, (1025, 7, 3): 1, (4800, 7, 1): 1, (4800, 16, 3): 8}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def inputs(n, K, B, extra=0):
    """Seeded float32 y (B, n), mu = y + noise, lv uniform in [-2.5, 2.5] (the range of fw_logvar_pr
    in tests/golden/model_s16_b4.npz), logw (B, K)."""
    seed = 100000 * K + 10 * n + B + RESEED.get((n, K, B), 0) + extra
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.standard_normal((B, n)).astype(np.float32)
    mu = (y[:, None] + np.float32(0.6) * rng.standard_normal((B, K, n)).astype(np.float32)).astype(np.float32)
    lv = rng.uniform(-2.5, 2.5, (B, K, n)).astype(np.float32)
    logw = rng.standard_normal((B, K)).astype(np.float32)
    return y, mu, lv, logw


def run(y, mu, lv, logw=None, bins=20, levels=LEVELS, ws_fill=None, want_pit=True):
    """vt_pred_mixture_rows + vt_pred_finish on device tensors y (B, n), mu / lv (B, K, n)."""
    from vaeteb import _lib
    B, K, n = mu.shape
    P, st = _lib.ptr, _lib.stream()
    tile = _lib.lib().fns["vt_pred_tile"]()
    assert tile == T_TILE
    tiles, nl = -(-n // tile), len(levels)
    lev = torch.tensor(levels, dtype=torch.float64, device="cuda")
    new = lambda *s, dtype=torch.float32: torch.full(s, float("nan") if dtype != torch.int32 else -7, dtype=dtype,
                                                     device="cuda")
    o = dict(mean=new(B, n), var_aleatoric=new(B, n), var_epistemic=new(B, n), pit=new(B, n) if want_pit else None,
             logdens=new(B, n) if want_pit else None, out=new(B, 5), ll=new(B, K),
             pit_hist=new(B, bins, dtype=torch.int32), coverage=new(B, nl))
    ws = torch.empty(B * tiles * (K + 3 + bins + nl), dtype=torch.float64, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    _lib.call("vt_pred_mixture_rows", P(y), P(mu), P(lv), B, K, n, bins, P(lev), nl, P(o["mean"]),
              P(o["var_aleatoric"]), P(o["var_epistemic"]), P(o["pit"]), P(o["logdens"]), P(ws), st)
    _lib.call("vt_pred_finish", P(ws), P(logw), B, K, n, bins, nl, P(o["out"]), P(o["ll"]), P(o["pit_hist"]),
              P(o["coverage"]), st)
    for i, k in enumerate(("nll_mixture", "nll_moment", "sharpness", "elbo", "iwae")):
        o[k] = o["out"][:, i].clone()
    return o


def assert_bounds(got, ref, mu, what, row_bound=None):
    """got: name -> tensor (run()'s dict or a PredictiveResult's fields), ref: R.predictive(...) of the
    same float32 inputs; mu the (B, K, n) float32 means.  row_bound (B, K): the allowed error of the
    rows that enter elbo / iwae (default: ll's own)."""
    G = lambda k: got[k].double().cpu().numpy()
    mu = np.asarray(mu, np.float64)
    n = mu.shape[-1]
    worst = {}

    def within(name, err, allowed):
        ratio = np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), np.where(err > 0, np.inf, 0.0))
        worst[name] = f"{np.max(err):.2e} ({np.max(ratio):.2f} of the bound)"
        assert (err <= allowed).all(), (what, name, float(np.max(err)), float(np.max(ratio)))

    ll_bound = 1e-6 * ref["ll_mag"]
    within("ll", np.abs(G("ll") - ref["ll"]), ll_bound)
    within("nll_mixture", np.abs(G("nll_mixture") - ref["nll_mixture"]), 1e-6 * ref["mix_mag"])
    rb = (ll_bound if row_bound is None else row_bound).max(-1)
    if got.get("elbo") is not None:
        within("elbo", np.abs(G("elbo") - ref["elbo"]), rb)
        within("iwae", np.abs(G("iwae") - ref["iwae"]), rb)
    within("mean", np.abs(G("mean") - ref["mean"]), 2.0 ** -23 * np.abs(mu).mean(1))
    within("var_aleatoric", np.abs(G("var_aleatoric") - ref["var_aleatoric"]), 5e-7 * ref["var_aleatoric"])
    ve, rve = G("var_epistemic"), ref["var_epistemic"]
    assert (ve >= 0).all(), what
    big = rve > 1e-10 * (mu ** 2).mean(1)
    within("var_epistemic", np.where(big, np.abs(ve - rve), 0.0), 5e-7 * rve)
    within("nll_moment", np.abs(G("nll_moment") - ref["nll_moment"]), 2e-6 * ref["moment_mag"])
    within("sharpness", np.abs(G("sharpness") - ref["sharpness"]), 2e-6 * ref["sharp_mag"])
    if got.get("pit") is not None:
        within("pit", np.abs(G("pit") - ref["pit"]), np.full_like(ref["pit"], 1e-6))
        within("logdens", np.abs(G("logdens") - ref["logdens"]), 1e-6 * ref["l_mag_max"])
    bins, levels = got["pit_hist"].shape[-1], got["levels"]
    assert R.near_edge(ref["pit"], bins, levels) == 0, (what, "a reference PIT lies within 2e-6 of an edge")
    assert (G("pit_hist") == ref["pit_hist"]).all(), what
    assert (G("pit_hist").sum(-1) == n).all()
    ref_cnt = np.rint(ref["coverage"] * n)
    assert (np.rint(G("coverage") * n) == ref_cnt).all(), what
    assert np.abs(G("coverage") - ref_cnt / n).max(initial=0.0) <= 6e-8, what
    print(f"{what}: " + "  ".join(f"{k} {v}" for k, v in worst.items()))


def reference(y, mu, lv, logw=None, bins=20, levels=LEVELS):
    ref = R.predictive(y, mu, lv, logw, bins=bins, levels=levels)
    ref["l_mag_max"] = R.log_terms(y, mu, lv)[1].max(1)
    return ref


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ------------------------------------------------------------------ the draw kernel
@pytest.mark.parametrize("B,K,m", [(1, 1, 96), (3, 5, 512), (3, 2, 513), (2, 7, 9600)])
def test_draw_rows_z_bit_equal_and_logw(B, K, m):
    from vaeteb import _lib
    P, st = _lib.ptr, _lib.stream()
    gen = torch.Generator().manual_seed(1000 * m + 10 * B + K)
    mu, mu_p = torch.randn(B, m, generator=gen).cuda(), torch.randn(B, m, generator=gen).cuda()
    lv = (torch.rand(B, m, generator=gen) * 8 - 6).cuda()
    lv_p = (torch.rand(B, m, generator=gen) * 8 - 6).cuda()
    eps = torch.randn(B * K, m, generator=gen).cuda()
    z, logw = torch.full((B * K, m), float("nan"), device="cuda"), torch.full((B * K,), float("nan"), device="cuda")
    _lib.call("vt_pred_draw_rows", P(mu), P(lv), P(eps), P(mu_p), P(lv_p), B, K, m, P(z), P(logw), st)
    # vt_te_latent_rows with mu_c = mu expanded over K and mu_y = 0
    mu_x, lv_x = (t.repeat_interleave(K, 0).contiguous() for t in (mu, lv))
    z0, te, zero = torch.empty_like(z), torch.empty(B * K, device="cuda"), torch.zeros_like(mu)
    _lib.call("vt_te_latent_rows", P(mu_x), P(lv_x), P(zero), P(lv_p), P(eps), B, K, m, P(z0), None, P(te), None, st)
    assert torch.equal(z, z0)
    ref, mag = R.logw(lv.cpu().numpy(), lv_p.cpu().numpy(), eps.view(B, K, m).cpu().numpy(),
                      z.view(B, K, m).cpu().numpy(), mu_p.cpu().numpy())
    err = np.abs(logw.view(B, K).double().cpu().numpy() - ref)
    print(f"logw B={B} K={K} m={m}: max err {err.max():.2e}, {(err / (1e-6 * mag)).max():.2f} of the bound")
    assert (err <= 1e-6 * mag).all()
    # without the prior: the same z, logw written as 0
    z1, w1 = torch.full_like(z, float("nan")), torch.full_like(logw, float("nan"))
    _lib.call("vt_pred_draw_rows", P(mu), P(lv), P(eps), None, None, B, K, m, P(z1), P(w1), st)
    assert torch.equal(z1, z) and (w1 == 0).all()
    # two calls, and the recordings one at a time
    z2, w2 = torch.empty_like(z), torch.empty_like(logw)
    for b in range(B):
        part = [t.clone() for t in (mu[b:b + 1], lv[b:b + 1], eps[b * K:(b + 1) * K], mu_p[b:b + 1], lv_p[b:b + 1])]
        _lib.call("vt_pred_draw_rows", *[P(t) for t in part], 1, K, m, z2.data_ptr() + 4 * b * K * m,
                  w2.data_ptr() + 4 * b * K, st)
    assert torch.equal(z2, z) and torch.equal(w2, logw)


# ------------------------------------------------------------------ the mixture and finish kernels
@pytest.mark.parametrize("n,K,B", CASES)
def test_mixture_kernels_vs_float64(n, K, B):
    y, mu, lv, logw = inputs(n, K, B)
    ref = reference(y, mu, lv, logw)
    yd, md, ld, wd = dev(y, mu, lv, logw)
    if B > 1 and n % 4:
        assert md.view(B * K, n)[1].data_ptr() % 16                          # rows off the 16-byte grid
    got = run(yd, md, ld, wd)
    got["levels"] = LEVELS
    assert_bounds(got, ref, mu, f"n={n} K={K} B={B}")
    if K > 1:
        assert (got["iwae"] >= got["elbo"]).all()
    # the nullable outputs change nothing else
    g2 = run(yd, md, ld, wd, want_pit=False)
    for k in ("mean", "var_aleatoric", "var_epistemic", "out", "ll", "pit_hist", "coverage"):
        assert torch.equal(g2[k], got[k]), k


def test_mixture_misaligned_bases_write_nothing_outside():
    """Inputs and outputs one float off the 16-byte grid at even n (every row misaligned alike): the
    scalar path gives the float4 path's bits, and nothing outside the output rows is written."""
    from vaeteb import _lib
    n, K, B = 2 * T_TILE + 4, 3, 2
    y, mu, lv, _ = inputs(n, K, B)
    yd, md, ld = dev(y, mu, lv)
    a = run(yd, md, ld)
    shift = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    ys, ms, ls = shift(yd), shift(md), shift(ld)
    assert ys.data_ptr() % 16 == 4 and ms.data_ptr() % 16 == 4
    P, st = _lib.ptr, _lib.stream()
    pad = torch.full((5, B * n + 9), float("nan"), device="cuda")
    outs = [pad[i, 1:1 + B * n].view(B, n) for i in range(5)]
    lev = torch.tensor(LEVELS, dtype=torch.float64, device="cuda")
    ws = torch.empty(B * 3 * (K + 3 + 20 + 3), dtype=torch.float64, device="cuda")
    _lib.call("vt_pred_mixture_rows", ys.data_ptr(), ms.data_ptr(), ls.data_ptr(), B, K, n, 20, P(lev), 3,
              *[o.data_ptr() for o in outs], P(ws), st)
    for o, k in zip(outs, ("mean", "var_aleatoric", "var_epistemic", "pit", "logdens")):
        assert torch.equal(o, a[k]), k
    assert torch.isnan(pad[:, 0]).all() and torch.isnan(pad[:, 1 + B * n:]).all()


def test_mixture_edge_rows():
    """Recording 0: lv = -20; 1: lv = +10; 2: y == mu exactly for every draw; 3: all draws identical;
    4: one draw's l more than 745 below the others; then a NaN in one recording's mu."""
    n, K, B, bins = 257, 4, 5, 7
    y, mu, lv, logw = inputs(n, K, B, extra=3)
    mu[0] = y[0, None] + np.float32(1e-4) * (mu[0] - y[0, None])
    lv[0] = -20.0
    lv[1] = 10.0
    mu[2] = y[2, None]
    mu[3], lv[3] = mu[3, :1], lv[3, :1]
    mu[4, 1], lv[4, 1] = y[4] + np.float32(60.0), 0.0
    ref = reference(y, mu, lv, logw, bins=bins)
    assert (ref["l"][4, [0, 2, 3]].min(0) - ref["l"][4, 1] > 745).all()
    yd, md, ld, wd = dev(y, mu, lv, logw)
    got = run(yd, md, ld, wd, bins=bins)
    got["levels"] = LEVELS
    assert_bounds(got, ref, mu, "edge rows")
    for k in ("mean", "var_aleatoric", "var_epistemic", "pit", "logdens", "ll", "out"):
        assert torch.isfinite(got[k]).all(), k
    assert (got["var_epistemic"][2] == 0).all() and (got["var_epistemic"][3] == 0).all()
    assert (got["pit"][2] == 0.5).all() and torch.equal(got["mean"][2], yd[2]) and torch.equal(got["mean"][3], md[3, 0])
    # identical draws: the mixture is its single component
    one = run(yd[3:4].contiguous(), md[3:4, :1].contiguous(), ld[3:4, :1].contiguous(), None, bins=bins)
    r1 = reference(y[3:4], mu[3:4, :1], lv[3:4, :1], bins=bins)
    assert abs(one["nll_mixture"].item() - got["nll_mixture"][3].item()) <= 2e-6 * r1["mix_mag"][0]
    assert abs(got["nll_mixture"][3].item() - r1["nll_mixture"][0]) <= 1e-6 * r1["mix_mag"][0]
    assert torch.equal(one["pit_hist"][0], got["pit_hist"][3]) and torch.equal(one["mean"][0], got["mean"][3])
    # the far draw does not enter: max - log K over the three others
    r3 = reference(y[4:5], mu[4:5, [0, 2, 3]], lv[4:5, [0, 2, 3]], bins=bins)
    want = r3["logdens"][0] + math.log(3.0) - math.log(4.0)
    assert np.abs(got["logdens"][4].double().cpu().numpy() - want).max() <= 1e-6 * ref["l_mag_max"][4].max()
    # a NaN in recording 1 stays in recording 1
    mu_nan = mu.copy()
    mu_nan[1, 2, 5] = np.nan
    nd = dev(mu_nan)[0]
    bad = run(yd, nd, ld, wd, bins=bins)
    for k in ("mean", "var_aleatoric", "var_epistemic", "pit", "logdens", "ll", "out", "pit_hist", "coverage"):
        keep = [0, 2, 3, 4]
        assert torch.equal(bad[k][keep].contiguous().view(torch.int32), got[k][keep].contiguous().view(torch.int32)), k
    assert torch.isnan(bad["out"][1]).all()            # nll_mixture, nll_moment, sharpness, elbo, iwae
    assert torch.isnan(bad["ll"][1, 2]) and torch.isfinite(bad["ll"][1, [0, 1, 3]]).all()
    for k in ("mean", "var_epistemic", "pit", "logdens"):
        assert torch.isnan(bad[k][1, 5]) and torch.isfinite(bad[k][1, :5]).all() and torch.isfinite(bad[k][1, 6:]).all(), k
    assert bad["pit_hist"][1].sum().item() == n - 1    # a NaN PIT is counted nowhere


def test_mixture_deterministic_workspace_blind_and_split_invariant():
    n, K, B = 2 * T_TILE + 3, 7, 3
    y, mu, lv, logw = inputs(n, K, B)
    yd, md, ld, wd = dev(y, mu, lv, logw)
    names = ("mean", "var_aleatoric", "var_epistemic", "pit", "logdens", "out", "ll", "pit_hist", "coverage")
    bits = lambda t: t.contiguous().view(torch.int32)
    a, b, c = run(yd, md, ld, wd), run(yd, md, ld, wd), run(yd, md, ld, wd, ws_fill=float("nan"))
    for k in names:
        assert torch.equal(bits(a[k]), bits(b[k])) and torch.equal(bits(a[k]), bits(c[k])), k
    parts = [run(yd[i:i + 1].clone(), md[i:i + 1].clone(), ld[i:i + 1].clone(), wd[i:i + 1].clone()) for i in range(B)]
    for k in names:
        assert torch.equal(bits(torch.cat([p[k] for p in parts])), bits(a[k])), k


# ------------------------------------------------------------------ end to end
B_E, K_E, S_E, L_E = 3, 5, 16, 32


def _model(g, **prec):
    """det_fill_ weights and the fixture's BatchNorm running buffers (decoder included)."""
    from golden_util import det_fill_
    from vaeteb.model import SeqVaeTeb
    m = det_fill_(SeqVaeTeb(sequence_length=S_E, **prec))
    sd = m.state_dict()
    for i, k in enumerate(list(g["bn_names"])):
        sd[k].copy_(torch.from_numpy(g[f"bn_{i}"]))
    return m.cuda()


def _loop(m, y_st, y_ph, x_ph, eps):
    """The literal alternative: K eval-mode forwards."""
    m.eval()
    with torch.no_grad():
        return [m(y_st, y_ph, x_ph, eps=eps[:, k].contiguous()) for k in range(eps.shape[1])]


def _fields_of(r):
    d = {k: getattr(r, k) for k in r.__slots__}
    return d


def _check_against_ref_of(r, fws, y_raw, eps, what):
    """Every field of the result against predictive_ref on the loop's own mu_pr / logvar_pr."""
    mu = torch.stack([fw["mu_pr"] for fw in fws], 1).cpu().numpy()
    lv = torch.stack([fw["logvar_pr"] for fw in fws], 1).cpu().numpy()
    B, K = mu.shape[:2]
    wref, wmag = R.logw(fws[0]["logvar_post"].reshape(B, -1).cpu().numpy(), fws[0]["logvar_prior"].reshape(B, -1).cpu().numpy(),
                        eps.reshape(B, K, -1).cpu().numpy(), r.z.reshape(B, K, -1).cpu().numpy(),
                        fws[0]["mu_prior"].reshape(B, -1).cpu().numpy())
    err = np.abs(r.logw.double().cpu().numpy() - wref)
    print(f"{what}: logw max err {err.max():.2e}, {(err / (1e-6 * wmag)).max():.2f} of the bound")
    assert (err <= 1e-6 * wmag).all()
    ref = reference(y_raw.cpu().numpy(), mu, lv, wref, bins=r.bins, levels=tuple(r.levels))
    assert_bounds(_fields_of(r), ref, mu, what, row_bound=1e-6 * (ref["ll_mag"] + wmag))


@pytest.fixture(scope="module")
def px(golden):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb.predictive import Predictive
    g = golden("eval_gain_s16_b3")
    Tn = lambda k: torch.from_numpy(g[k]).cuda()
    args = (Tn("y_st"), Tn("y_ph"), Tn("x_ph"), Tn("y_raw"))
    eps = torch.randn(B_E, K_E, S_E, L_E, generator=torch.Generator().manual_seed(4242)).cuda()
    m = _model(g)
    pred = Predictive(m)
    m.train()
    res = pred(*args, n_samples=K_E, eps=eps, return_samples=True, return_pit=True)
    training_after = m.training
    fws = _loop(m, *args[:3], eps)
    return dict(g=g, m=m, pred=pred, args=args, eps=eps, res=res, fws=fws, training_after=training_after)


def test_predictive_matches_the_loop_fp32(px):
    """z and the encoder pieces bit-equal; mu_pr / logvar_pr: the decoder runs on B*K = 15 rows here and
    on B = 3 rows per forward in the loop; its heads are bit-reproducible across such row counts
    (tests/test_gpu_eval.py), so they are asserted EQUAL, and every field is then checked against the
    float64 definitions of the loop's own outputs."""
    from vaeteb.evaluate import recon_metrics
    r, fws, (y_st, y_ph, x_ph, y_raw), eps = px["res"], px["fws"], px["args"], px["eps"]
    assert r.mean.shape == (3, 256) and r.ll.shape == (3, 5) and r.pit_hist.shape == (3, 20)
    assert r.pit_hist.dtype == torch.int32 and r.coverage.shape == (3, 3) and r.mu_pr.shape == (3, 5, 256)
    assert r.z.shape == (3, 5, 16, 32) and r.nll_mixture.shape == (3,) and r.iwae.shape == (3,)
    for k in range(K_E):
        assert torch.equal(r.z[:, k], fws[k]["z"]), k
        assert torch.equal(r.z_mu, fws[k]["mu_post"]) and torch.equal(r.z_logvar, fws[k]["logvar_post"])
    mu_loop = torch.stack([fw["mu_pr"] for fw in fws], 1)
    lv_loop = torch.stack([fw["logvar_pr"] for fw in fws], 1)
    print(f"vs the loop: mu_pr rel-L2 {rel(r.mu_pr, mu_loop):.2e}, logvar_pr rel-L2 {rel(r.logvar_pr, lv_loop):.2e}")
    assert torch.equal(r.mu_pr, mu_loop) and torch.equal(r.logvar_pr, lv_loop)
    _check_against_ref_of(r, fws, y_raw, eps, "vs the loop")
    for name, t in zip(("vaf", "mse", "snr", "vaf_unclamped"), recon_metrics(y_raw, r.mean)):
        assert torch.equal(getattr(r, name), t) and t.shape == (3,), name
    assert torch.equal(r.sd, (r.var_aleatoric + r.var_epistemic).sqrt())
    mean = r.means()
    assert mean["coverage"].shape == (3,) and abs(mean["pit_hist"].sum().item() - 1) < 1e-6
    assert (r.iwae >= r.elbo).all() and (r.var_epistemic > 0).any()


def test_predictive_matches_the_reference_forward(px):
    """oracle.model_ref on the CPU with the same weights, BatchNorm buffers and eps."""
    from golden_util import det_fill_
    from oracle import model_ref as M
    g, r, eps = px["g"], px["res"], px["eps"].cpu()
    ref = det_fill_(M.SeqVaeTebRef(S_E))
    sd = ref.state_dict()
    for i, k in enumerate(list(g["bn_names"])):
        sd[k].copy_(torch.from_numpy(g[f"bn_{i}"]))
    ref.eval()
    Tn = lambda k: torch.from_numpy(g[k])
    mus = []
    with torch.no_grad():
        for k in range(K_E):
            fw = ref(Tn("y_st"), Tn("y_ph"), Tn("x_ph"), eps[:, k].contiguous())
            e_mu, e_lv = rel(r.mu_pr[:, k], fw["mu_pr"]), rel(r.logvar_pr[:, k], fw["logvar_pr"])
            print(f"draw {k}: mu_pr rel-L2 {e_mu:.2e}, logvar_pr rel-L2 {e_lv:.2e} vs the reference")
            assert e_mu < 5e-5 and e_lv < 5e-5, (k, e_mu, e_lv)
            mus.append(fw["mu_pr"].double())
    mus = torch.stack(mus, 1)
    err = (r.mean.double().cpu() - mus.mean(1)).norm().item()
    allowed = 5e-5 * max(mus[:, k].norm().item() for k in range(K_E))
    print(f"mean vs the reference's: {err:.2e} (allowed {allowed:.2e})")
    assert err <= allowed


def test_plug_in_predictive_and_the_training_nll(px):
    m, pred, (y_st, y_ph, x_ph, y_raw) = px["m"], px["pred"], px["args"]
    zero = torch.zeros(B_E, 1, S_E, L_E, device="cuda")
    a = pred(y_st, y_ph, x_ph, y_raw, n_samples=1, eps=zero, return_samples=True, return_pit=True)
    p = pred(y_st, y_ph, x_ph, y_raw, n_samples=0, return_samples=True, return_pit=True)
    assert p.iwae is None and p.elbo is None and a.iwae is not None
    assert torch.equal(p.z[:, 0], p.z_mu) and (p.logw == 0).all()
    for k in ("z", "mu_pr", "logvar_pr", "mean", "var_aleatoric", "var_epistemic", "pit", "logdens", "ll",
              "nll_mixture", "nll_moment", "sharpness", "pit_hist", "coverage", "vaf", "mse", "snr"):
        assert torch.equal(getattr(a, k), getattr(p, k)), k
    assert (a.var_epistemic == 0).all() and torch.equal(a.mean, a.mu_pr[:, 0])
    with pytest.raises(ValueError):
        pred(y_st, y_ph, x_ph, y_raw, n_samples=0, eps=zero)
    # K = 1: rows of nll_mixture - 1/2 log 2pi average to compute_loss's nll_loss of the same forward
    eps1 = px["eps"][:, :1].contiguous()
    r1 = pred(y_st, y_ph, x_ph, y_raw, n_samples=1, eps=eps1)
    with torch.no_grad():
        fw = m(y_st, y_ph, x_ph, eps=eps1[:, 0].contiguous())
        nll = m.compute_loss(fw, y_st, y_ph, y_raw)["nll_loss"].double().item()
    mine = (r1.nll_mixture.double() - 0.5 * math.log(2 * math.pi)).mean().item()
    print(f"nll_loss {nll:.8f} vs mean(nll_mixture) - log(2 pi)/2 {mine:.8f}: rel {abs(mine / nll - 1):.2e}")
    assert abs(mine - nll) <= 1e-6 * abs(nll)
    assert torch.allclose(r1.iwae, r1.elbo, rtol=0, atol=0)


def test_prior_source(px):
    from vaeteb import _lib
    m, pred, (y_st, y_ph, x_ph, y_raw), eps = px["m"], px["pred"], px["args"], px["eps"]
    r = pred(y_st, y_ph, x_ph, y_raw, n_samples=K_E, eps=eps, source="prior", return_samples=True, return_pit=True)
    fw = px["fws"][0]
    assert torch.equal(r.z_mu, fw["mu_prior"]) and torch.equal(r.z_logvar, fw["logvar_prior"])
    P, n = _lib.ptr, S_E * L_E
    mu_x, lv_x = (t.repeat_interleave(K_E, 0).contiguous() for t in (r.z_mu, r.z_logvar))
    z0, te = torch.empty(B_E * K_E, S_E, L_E, device="cuda"), torch.empty(B_E * K_E, device="cuda")
    zero = torch.zeros_like(r.z_mu)
    _lib.call("vt_te_latent_rows", P(mu_x), P(lv_x), P(zero), P(r.z_logvar), P(eps), B_E, K_E, n, P(z0), None, P(te),
              None, _lib.stream())
    assert torch.equal(r.z.view(B_E * K_E, S_E, L_E), z0)
    assert (r.logw == 0).all() and r.source == "prior"
    assert rel(r.mu_pr, px["res"].mu_pr) > 1e-3          # other draws than the posterior's
    blind = pred(y_st, y_ph, torch.zeros_like(x_ph), y_raw, n_samples=K_E, eps=eps, source="prior",
                 return_samples=True, return_pit=True)
    for k in r.__slots__:
        a, b = getattr(r, k), getattr(blind, k)
        if torch.is_tensor(a):
            assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), k
    # elbo is then the mean log-likelihood of the draws, iwae their log-mean-exp
    assert torch.allclose(r.elbo, r.ll.double().mean(1).float(), rtol=1e-6)


def test_noise_comes_from_one_draw(px):
    pred, args = px["pred"], px["args"]
    torch.cuda.manual_seed(99)
    a = pred(*args, n_samples=K_E, return_samples=True)
    torch.cuda.synchronize()
    state_a = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(99)
    eps = torch.randn((B_E, K_E, S_E, L_E), device="cuda")
    torch.cuda.synchronize()
    state_one = torch.cuda.get_rng_state()
    b = pred(*args, n_samples=K_E, eps=eps, return_samples=True)
    assert torch.equal(state_a, state_one)
    for k in ("z", "mu_pr", "mean", "var_epistemic", "nll_mixture", "iwae", "elbo", "logw", "pit_hist"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    pred(*args, n_samples=0)
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), state_one)


@pytest.mark.parametrize("rows", [K_E, 2 * K_E + 1])
def test_chunking(px, rows):
    """rows_per_launch K: one recording per chunk; 2 K + 1: two, then one; the fixture (256) ran all 15
    rows at once.  z and logw do not move a bit; mu_pr / logvar_pr on the same terms as against the
    loop: equal, and with them everything the mixture kernels compute."""
    from vaeteb.predictive import Predictive
    res = px["res"]
    r = Predictive(px["m"], rows_per_launch=rows)(*px["args"], n_samples=K_E, eps=px["eps"], return_samples=True,
                                                  return_pit=True)
    assert torch.equal(r.z, res.z) and torch.equal(r.logw, res.logw)
    print(f"rows_per_launch {rows}: mu_pr rel-L2 {rel(r.mu_pr, res.mu_pr):.2e}")
    assert torch.equal(r.mu_pr, res.mu_pr) and torch.equal(r.logvar_pr, res.logvar_pr)
    for k in ("mean", "var_aleatoric", "var_epistemic", "pit", "logdens", "ll", "nll_mixture", "nll_moment",
              "sharpness", "elbo", "iwae", "pit_hist", "coverage", "vaf", "mse", "snr", "vaf_unclamped"):
        assert torch.equal(getattr(r, k), getattr(res, k)), k
    with pytest.raises(ValueError):
        Predictive(px["m"], rows_per_launch=K_E - 1)(*px["args"], n_samples=K_E, eps=px["eps"])


def test_side_effects_and_shape_errors(px):
    assert px["training_after"] is False
    r, pred, (y_st, y_ph, x_ph, y_raw), eps = px["res"], px["pred"], px["args"], px["eps"]
    assert not any(t.requires_grad for t in (getattr(r, k) for k in r.__slots__) if torch.is_tensor(t))
    lean = pred(y_st, y_ph, x_ph, y_raw, n_samples=K_E, eps=eps)
    assert lean.mu_pr is None and lean.z is None and lean.pit is None and lean.logdens is None
    assert torch.equal(lean.nll_mixture, r.nll_mixture) and torch.equal(lean.pit_hist, r.pit_hist)
    other = pred(y_st, y_ph, x_ph, y_raw, n_samples=K_E, eps=eps, bins=7, levels=(0.8,))
    assert other.pit_hist.shape == (3, 7) and other.coverage.shape == (3, 1) and (other.pit_hist.sum(1) == 256).all()
    assert torch.equal(other.iwae, r.iwae)
    with pytest.raises(ValueError):
        pred(y_st, y_ph, x_ph, y_raw[:, :-1], n_samples=K_E, eps=eps)
    with pytest.raises(ValueError):
        pred(y_st[:, :-1], y_ph, x_ph, y_raw, n_samples=K_E, eps=eps)
    with pytest.raises(ValueError):
        pred(y_st, y_ph, x_ph, y_raw, n_samples=K_E - 1, eps=eps)
    with pytest.raises(ValueError):
        pred(y_st, y_ph, x_ph, y_raw, n_samples=K_E, eps=eps.cpu())


def test_frontend_entry_equals_the_field_entry():
    from vaeteb import synthetic
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.model import SeqVaeTeb
    fe = FrontEnd(FrontEndPlan(11, 4, 16, 4096, device="cuda"), load_stats(11, 4, 16, 4096))
    torch.manual_seed(0)
    m = SeqVaeTeb(sequence_length=fe.S_out, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                  cross_phase_channels=fe.C_x).cuda()
    x = torch.from_numpy(synthetic.batch(4000, 2, 4096)).cuda()
    eps = torch.randn(2, 3, fe.S_out, 32, generator=torch.Generator().manual_seed(1)).cuda()
    a = m.predictive(frontend=fe, x=x, n_samples=3, eps=eps, return_samples=True)
    f = {k: v.clone() for k, v in fe(x).items()}
    b = m.predictive(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], n_samples=3, eps=eps, return_samples=True)
    for k in ("mean", "var_aleatoric", "var_epistemic", "nll_mixture", "nll_moment", "sharpness", "elbo", "iwae",
              "ll", "logw", "pit_hist", "coverage", "vaf", "mu_pr", "logvar_pr"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.mean.shape == (2, 16 * fe.S_out) and torch.isfinite(a.iwae).all() and torch.isfinite(a.nll_mixture).all()
    assert not m.training and m.__dict__["_predictive"] is not None
    with pytest.raises(ValueError):
        m.predictive(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], frontend=fe, x=x)
    with pytest.raises(ValueError):
        m.predictive(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"])


def test_predictive_at_the_bench_precisions(px):
    g, (y_st, y_ph, x_ph, y_raw), eps = px["g"], px["args"], px["eps"]
    m = _model(g, conv_precision="bf16", mlp_precision="bf16", head_precision="bf16", lstm_precision="16-mixed")
    r = m.predictive(y_st, y_ph, x_ph, y_raw, n_samples=K_E, eps=eps, return_samples=True, return_pit=True)
    fws = _loop(m, y_st, y_ph, x_ph, eps)
    for k in range(K_E):
        assert torch.equal(r.z[:, k], fws[k]["z"]), k
    assert torch.equal(r.z_mu, fws[0]["mu_post"]) and torch.equal(r.z_logvar, fws[0]["logvar_post"])
    mu_loop = torch.stack([fw["mu_pr"] for fw in fws], 1)
    print(f"16-bit: mu_pr vs loop rel-L2 {rel(r.mu_pr, mu_loop):.2e}, bit-equal {torch.equal(r.mu_pr, mu_loop)}")
    # the mixture outputs against the definitions on this mode's own decoder outputs
    own = [dict(fw, mu_pr=r.mu_pr[:, k], logvar_pr=r.logvar_pr[:, k]) for k, fw in enumerate(fws)]
    _check_against_ref_of(r, own, y_raw, eps, "16-bit")
    assert not m.training
