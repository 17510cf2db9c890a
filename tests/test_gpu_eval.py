"""The batched evaluation sweep (vaeteb.evaluate: GainSweep, recon_metrics; csrc/evalm.hip) on the
GPU: the three row kernels against float64 numpy / the kernels they extend, the sweep against the
reference's own values (tests/golden/eval_gain_s16_b3.npz, tools/gen_golden_eval.py) and against the
literal loop over the public API (per gain: model(y_st, y_ph, x_ph * g), then
measure_transfer_entropy, metrics per sample), which is how the reference runs it
(ref/model/graph_model.py:1832-1854).

Bounds:
* vt_recon_metrics_rows vs float64 numpy of the same float32 rows (residual formed in float32):
  mse and 1 - vaf_unclamped to 1e-6 relative (what tests/test_gpu_elbo_optim.py holds the KL kernel
  to), snr_db to 1e-5 dB absolute (10/ln 10 times the ratio's 2e-6).  The outputs are float32, so
  the rows are drawn with var_res / var_y of order 1 (pr = y + 0.7 noise): the float32 rounding of
  vaf_unclamped, 6e-8 |vaf|, is then far below 1e-6 (1 - vaf).
* vt_eval_scale_rows: equality with the broadcast float32 product.
* vt_te_latent_rows: z, mu_post bit-equal vt_elbo_latent_fwd's, te, kl bit-equal vt_te_kl_rows's.
* GainSweep vs the reference fixture: mu_pr rel-L2 < 5e-5 (the project's forward-output bound,
  tests/test_gpu_model.py:226), te rel < 5e-5 (:258).  Metrics: with delta = mu_pr - ref per row and
  res = y - ref, |d var_res| and |d mse| <= (2 |delta| |res| + |delta|^2) / n (centring is a
  projection, so the same bound serves the variance), hence |d vaf| <= that / var_y and
  |d snr| <= 10/ln 10 * d mse / (mse - d mse); added: the kernel bounds above and the reference's own
  float32 np.var / np.mean, 2e-6 relative each (tests/test_eval_cpu.py).
* GainSweep vs the loop on the same GPU model: the encoders and the latent kernel are
  row-independent in eval mode, so the posterior pieces, z, te and kl are asserted bit-equal (te / kl
  through vt_te_kl_rows on the loop's pieces; the loop's own KL is ATen's expression and float32
  mean, held to 5e-5 as in tests/test_gpu_te_shift.py).  mu_pr: see
  test_sweep_matches_the_loop_fp32.
* 16-bit run: pieces bit-equal; mu_pr against the loop in the same mode within the 16-bit forward
  bound of tests/test_gpu_parity_s256.py (test_s256_bf16_step_within_reference_autocast_spread:
  2 x the reference's own bf16 spread of mu_pr, tests/golden/model_s256_b2_amp.npz).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAINS = [0.0, 0.001, 0.01, 1.0, 2.0, -1.0]
DB = 10.0 / np.log(10.0)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def metrics64(y, pr):
    """The metric definitions in float64 on float32 rows, the residual formed in float32:
    (vaf, mse, snr_db, vaf_unclamped, var_y), shaped like pr's leading dimensions."""
    y, pr = np.asarray(y, np.float32), np.asarray(pr, np.float32)
    yb = y[:, None, :] if pr.ndim == 3 else y
    res = (yb - pr).astype(np.float64)
    y64 = np.broadcast_to(yb.astype(np.float64), res.shape)
    var_y, var_r = y64.var(-1), res.var(-1)
    mse, sig = (res ** 2).mean(-1), (y64 ** 2).mean(-1)
    ok_v, ok_m = var_y > 1e-12, mse > 1e-12
    vu = np.where(ok_v, 1.0 - var_r / np.where(ok_v, var_y, 1.0), 0.0)
    snr = np.where(ok_m, DB * np.log(np.where(ok_m, sig / np.where(ok_m, mse, 1.0), 1.0)), 100.0)
    return np.clip(vu, 0.0, 1.0), mse, snr, vu, var_y


def _metrics(y, pr, B, K):
    """vt_recon_metrics_rows on device tensors y (B, n), pr (B*K, n) -> (B*K, 4)."""
    from vaeteb import _lib
    out = torch.empty((B * K, 4), device="cuda")
    _lib.call("vt_recon_metrics_rows", _lib.ptr(y), _lib.ptr(pr), B, K, y.shape[-1], _lib.ptr(out), _lib.stream())
    return out


def _assert_kernel_bounds(out, ref, what):
    """out (rows, 4) float32 from the kernel, ref = metrics64(...) flattened over the rows."""
    vaf, mse, snr, vu = (out[:, i].double().cpu().numpy() for i in range(4))
    rvaf, rmse, rsnr, rvu, _ = (np.asarray(a, np.float64).reshape(-1) for a in ref)
    e_mse = np.abs(mse - rmse) / np.maximum(rmse, 1e-300)
    e_vu = np.abs((1 - vu) - (1 - rvu)) / np.maximum(np.abs(1 - rvu), 1e-300)
    e_snr = np.abs(snr - rsnr)
    print(f"{what}: mse rel {e_mse.max():.2e}  (1 - vaf_unclamped) rel {e_vu.max():.2e}  snr abs {e_snr.max():.2e} dB")
    assert (np.abs(mse - rmse) <= 1e-6 * rmse).all(), what
    assert (np.abs((1 - vu) - (1 - rvu)) <= 1e-6 * np.abs(1 - rvu)).all(), what
    assert (e_snr <= 1e-5).all(), what
    assert torch.equal(out[:, 0], out[:, 3].clamp(0.0, 1.0)), what


# ------------------------------------------------------------------ metrics kernel
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 4800])
def test_metrics_kernel_vs_float64(n):
    from vaeteb.evaluate import recon_metrics
    for (B, K) in ((1, 1), (3, 1), (2, 3)):
        rng = np.random.Generator(np.random.PCG64(1000 * n + 10 * B + K))
        y = rng.standard_normal((B, n)).astype(np.float32)
        pr = (y[:, None, :] + np.float32(0.7) * rng.standard_normal((B, K, n)).astype(np.float32)).astype(np.float32)
        yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(pr).cuda()
        out = _metrics(yd, pd.view(B * K, n), B, K)
        ref = metrics64(y, pr)
        _assert_kernel_bounds(out, ref, f"n={n} B={B} K={K}")
        if n == 1:      # a single sample has no variance: vaf 0 by the var_y threshold
            assert (out[:, 0] == 0).all() and (out[:, 3] == 0).all()
        # the public wrapper is the same kernel: (B, K, n) and, for K = 1, (B, n)
        w = recon_metrics(yd, pd)
        assert all(t.shape == (B, K) for t in w)
        assert torch.equal(torch.stack(w, -1).reshape(B * K, 4), out)
        if K == 1:
            w2 = recon_metrics(yd.unsqueeze(-1), pd[:, 0])
            assert all(t.shape == (B,) for t in w2) and torch.equal(torch.stack(w2, -1), out)


def test_metrics_kernel_edge_rows():
    n = 257
    rng = np.random.Generator(np.random.PCG64(77))
    base = rng.standard_normal((5, n)).astype(np.float32)
    noise = rng.standard_normal((5, n)).astype(np.float32)
    y = base.copy()
    pr = (base + np.float32(0.7) * noise).astype(np.float32)
    y[0] = 2.5                                      # constant ground truth
    pr[1] = y[1]                                    # perfect reconstruction
    pr[2] = np.float32(3.0) * y[2]                  # residual -2 y: unclamped 1 - 4
    y[3] = np.float32(1e4) + base[3]                # large mean, unit spread
    pr[3] = (y[3] + np.float32(0.7) * noise[3]).astype(np.float32)
    out = _metrics(torch.from_numpy(y).cuda(), torch.from_numpy(pr).cuda(), 5, 1)
    o = out.cpu().numpy()
    assert o[0, 0] == 0 and o[0, 3] == 0                                   # var_y = 0
    assert o[1, 0] == 1 and o[1, 3] == 1 and o[1, 1] == 0 and o[1, 2] == 100
    assert abs(o[2, 3] + 3.0) <= 4e-6 and o[2, 0] == 0
    assert 0.2 < o[3, 0] < 0.8 and 0.2 < o[4, 0] < 0.8
    keep = [2, 3, 4]                                # rows 0 / 1 are exact values, checked above
    ref = [np.asarray(a)[keep] for a in metrics64(y, pr)]
    _assert_kernel_bounds(out[keep], ref, "edge rows (3y, offset 1e4, plain)")


def test_metrics_kernel_deterministic_and_split_invariant():
    B, K, n = 2, 3, 255
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(B, n, generator=gen).cuda()
    pr = (y.cpu()[:, None] + torch.randn(B, K, n, generator=gen)).view(B * K, n).cuda()
    one = _metrics(y, pr, B, K)
    assert torch.equal(one, _metrics(y, pr, B, K))
    halves = [_metrics(y[b:b + 1].contiguous(), pr[b * K:(b + 1) * K].contiguous(), 1, K) for b in range(B)]
    assert torch.equal(torch.cat(halves), one)
    inside = [_metrics(y[:1].contiguous(), pr[:2].contiguous(), 1, 2), _metrics(y[:1].contiguous(), pr[2:3].contiguous(), 1, 1)]
    assert torch.equal(torch.cat(inside), one[:3])


# ------------------------------------------------------------------ scale kernel
@pytest.mark.parametrize("n", [1, 7, 2080, 2082])
@pytest.mark.parametrize("misalign", [(0, 0), (1, 0), (0, 1), (3, 2)])
def test_scale_rows_is_the_ieee_product(n, misalign):
    """2080 = 16 * 130 (float4 rows), 2082 (every other row 16-byte aligned), 1 and 7 (tails only);
    source / destination base pointers off the 16-byte grid by `misalign` floats."""
    from vaeteb import _lib
    B, gains = 3, torch.tensor([0.0, -1.0, 0.001, 1.5], device="cuda")
    K = gains.numel()
    gen = torch.Generator().manual_seed(n)
    xs = torch.randn(B * n + 8, generator=gen).cuda()
    os_ = torch.full((B * K * n + 8,), float("nan"), device="cuda")
    x = xs[misalign[0]:misalign[0] + B * n].view(B, n)
    out = os_[misalign[1]:misalign[1] + B * K * n].view(B, K, n)
    assert x.data_ptr() % 16 == 4 * misalign[0] and out.data_ptr() % 16 == 4 * misalign[1]
    _lib.call("vt_eval_scale_rows", x.data_ptr(), B, K, n, _lib.ptr(gains), out.data_ptr(), _lib.stream())
    want = x[:, None] * gains[None, :, None]
    assert torch.equal(out, want)
    assert torch.equal(out.contiguous().view(torch.int32), want.contiguous().view(torch.int32))   # signed zeros too
    # nothing outside the destination rows was written
    assert torch.isnan(os_[:misalign[1]]).all() and torch.isnan(os_[misalign[1] + B * K * n:]).all()


# ------------------------------------------------------------------ latent kernel
@pytest.mark.parametrize("S,K", [(3, 1), (3, 3), (16, 1), (16, 3)])
def test_te_latent_rows_bit_equal_the_kernels_it_extends(S, K):
    """Row sizes S * 32 = 96 (less than one workgroup) and 512 (two elements per thread)."""
    from vaeteb import _lib
    B, L = 2, 32
    n = S * L
    gen = torch.Generator().manual_seed(100 * S + K)
    mu_c, mu_y = torch.randn(B * K, S, L, generator=gen).cuda(), torch.randn(B, S, L, generator=gen).cuda()
    lv_q = (torch.rand(B * K, S, L, generator=gen) * 12 - 6).cuda()
    lv_p = (torch.rand(B, S, L, generator=gen) * 12 - 6).cuda()
    eps = torch.randn(B * K, S, L, generator=gen).cuda()
    P, st = _lib.ptr, _lib.stream()
    z, mp, kl = (torch.empty_like(mu_c) for _ in range(3))
    te = torch.empty(B * K, device="cuda")
    _lib.call("vt_te_latent_rows", P(mu_c), P(lv_q), P(mu_y), P(lv_p), P(eps), B, K, n, P(z), P(mp), P(te), P(kl), st)
    # vt_elbo_latent_fwd on the prior expanded to one row per (recording, gain)
    mu_y_x, lv_p_x = (t.repeat_interleave(K, 0).contiguous() for t in (mu_y, lv_p))
    z0, mp0, kl0 = torch.empty_like(mu_c), torch.empty_like(mu_c), torch.empty(1, device="cuda")
    ws = torch.empty(_lib.lib().fns["vt_elbo_workspace_floats"](), device="cuda")
    _lib.call("vt_elbo_latent_fwd", P(mu_c), P(lv_q), P(mu_y_x), P(lv_p_x), P(eps), B * K * S, L, P(z0), P(mp0),
              P(kl0), P(ws), st)
    assert torch.equal(z, z0) and torch.equal(mp, mp0)
    te1, kl1 = torch.empty(B * K, device="cuda"), torch.empty_like(mu_c)
    _lib.call("vt_te_kl_rows", P(mu_c), P(lv_q), P(mu_y), P(lv_p), B, K, n, P(te1), P(kl1), st)
    assert torch.equal(te, te1) and torch.equal(kl, kl1)
    # the nullable outputs change nothing else
    z2, te2 = torch.empty_like(mu_c), torch.empty(B * K, device="cuda")
    _lib.call("vt_te_latent_rows", P(mu_c), P(lv_q), P(mu_y), P(lv_p), P(eps), B, K, n, P(z2), None, P(te2), None, st)
    assert torch.equal(z2, z) and torch.equal(te2, te)


# ------------------------------------------------------------------ the sweep
def _model(g, **prec):
    """det_fill_ weights and the fixture's BatchNorm running buffers (decoder included)."""
    from golden_util import det_fill_
    from vaeteb.model import SeqVaeTeb
    m = det_fill_(SeqVaeTeb(sequence_length=16, **prec))
    sd = m.state_dict()
    for i, k in enumerate(list(g["bn_names"])):
        sd[k].copy_(torch.from_numpy(g[f"bn_{i}"]))
    return m.cuda()


def _loop(m, y_st, y_ph, x_ph, gains, eps=None):
    """The literal loop (ref/model/graph_model.py:1832-1836) and, per gain, the encoder pieces
    (mu_c, lv_q, mu_y, lv_p) as encode() computes them (they draw no noise)."""
    m.eval()
    fws, kls, pieces = [], [], []
    with torch.no_grad():
        for k, g in enumerate(gains):
            xs = x_ph * float(g)
            fws.append(m(y_st, y_ph, xs, eps=None if eps is None else eps[:, k].contiguous()))
            if eps is None:
                kls.append(m.measure_transfer_entropy(y_st, y_ph, xs, reduce_mean=False))
            mu_y, lv_full = m.target_encoder(y_st, y_ph)
            lv_p, c_lv = torch.split(lv_full, m.latent_dim_target, dim=-1)
            mu_c, lv_q = m.conditional_encoder(m.source_encoder(xs), c_lv)
            pieces.append((mu_c.contiguous(), lv_q.contiguous(), mu_y.contiguous(), lv_p.contiguous()))
    return fws, kls, pieces


def _assert_pieces_reproduced(res, pieces):
    """The loop's per-gain pieces (B rows each) through vt_te_kl_rows give the sweep's te and kl
    exactly: the sweep's posterior and prior pieces are the loop's, bit for bit."""
    from vaeteb import _lib
    for k, (mu_c, lv_q, mu_y, lv_p) in enumerate(pieces):
        B, n = mu_c.shape[0], mu_c[0].numel()
        te, kl = torch.empty(B, device="cuda"), torch.empty_like(mu_c)
        _lib.call("vt_te_kl_rows", _lib.ptr(mu_c), _lib.ptr(lv_q), _lib.ptr(mu_y), _lib.ptr(lv_p), B, 1, n,
                  _lib.ptr(te), _lib.ptr(kl), _lib.stream())
        assert torch.equal(te, res.te[:, k]), k
        assert torch.equal(kl, res.kl[:, k]), k


def _propagated(y, ref_mu, got_mu):
    """Allowed |d mse|, |d vaf|, |d snr| (each (B, K)) for the kernel's metrics of got_mu against the
    reference's float32 numpy metrics of ref_mu (ref/model/graph_model.py:1619-1645), from the
    measured deviation delta = got_mu - ref_mu (module docstring)."""
    y, ref_mu, got_mu = (np.asarray(a, np.float64) for a in (y, ref_mu, got_mu))
    n = y.shape[-1]
    nd = np.linalg.norm(got_mu - ref_mu, axis=-1)
    nr = np.linalg.norm(y[:, None] - ref_mu, axis=-1)
    d = (2 * nd * nr + nd ** 2) / n
    _, mse, _, vu, var_y = metrics64(y, ref_mu)
    assert (d < 0.5 * mse).all()
    own = 2e-6
    a_mse = d + (1e-6 + own) * mse
    a_vaf = d / var_y + (1e-6 + 2 * own) * (1 - vu) + 1.2e-7      # 1.2e-7: two float32 values below 1
    a_snr = DB * d / (mse - d) + 1e-5 + DB * 2 * own
    return a_mse, a_vaf, a_snr


def _assert_metrics_within(res, ref, allowed, what):
    a_mse, a_vaf, a_snr = allowed
    for name, a in (("mse", a_mse), ("vaf", a_vaf), ("vaf_unclamped", a_vaf), ("snr", a_snr)):
        got = getattr(res, name).double().cpu().numpy()
        err = np.abs(got - np.asarray(ref[name], np.float64))
        print(f"{what}: {name} max err {err.max():.3e} (allowed there {a.reshape(-1)[err.argmax()]:.3e})")
        assert (err <= a).all(), (what, name, err.max())


@pytest.fixture(scope="module")
def fx(golden):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb.evaluate import GainSweep
    g = golden("eval_gain_s16_b3")
    assert list(g["gains"]) == GAINS
    T = lambda k: torch.from_numpy(g[k]).cuda()
    y_st, y_ph, x_ph, y_raw = T("y_st"), T("y_ph"), T("x_ph"), T("y_raw")
    B, K = 3, len(GAINS)
    eps = T("eps")[:, None].expand(B, K, 16, 32).contiguous()      # the fixture's one eps for every gain
    m = _model(g)
    sweep = GainSweep(m)
    m.train()
    res = sweep(y_st, y_ph, x_ph, y_raw, GAINS, eps=eps, elementwise=True, return_mu=True)
    training_after = m.training
    # the generator's noise: loop, then sweep, from the same seed
    torch.cuda.manual_seed(1234)
    fws, kls, pieces = _loop(m, y_st, y_ph, x_ph, GAINS)
    torch.cuda.synchronize()
    rng_loop = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(1234)
    res_rng = sweep(y_st, y_ph, x_ph, y_raw, GAINS, elementwise=True, return_mu=True)
    z_rng = sweep._bufs["z"].clone()                                # one chunk: every row's z, (B*K, S, L)
    torch.cuda.synchronize()
    rng_sweep = torch.cuda.get_rng_state()
    return dict(g=g, m=m, sweep=sweep, args=(y_st, y_ph, x_ph, y_raw), eps=eps, res=res, res_rng=res_rng,
                z_rng=z_rng, fws=fws, kls=kls, pieces=pieces, rng_loop=rng_loop, rng_sweep=rng_sweep,
                training_after=training_after)


def test_sweep_matches_the_reference_fixture(fx):
    g, res = fx["g"], fx["res"]
    assert res.te.shape == (3, 6) and res.mu_pr.shape == (3, 6, 256) and res.kl.shape == (3, 6, 16, 32)
    assert list(res.gains) == GAINS and res.te.is_cuda and res.vaf.is_cuda and not res.mu_pr.requires_grad
    for k, gain in enumerate(GAINS):
        e = rel(res.mu_pr[:, k], torch.from_numpy(g["mu_pr"][:, k]))
        print(f"gain {gain}: mu_pr rel-L2 vs reference {e:.2e}")
        assert e < 5e-5, (gain, e)
    e_te = np.abs(res.te.cpu().numpy().astype(np.float64) / g["te"] - 1)
    print("te max rel vs reference", e_te.max())
    assert (e_te < 5e-5).all()
    allowed = _propagated(g["y_raw"], g["mu_pr"], res.mu_pr.cpu().numpy())
    _assert_metrics_within(res, g, allowed, "vs reference")
    # inside the clamp on every row, as the fixture was built
    assert torch.equal(res.vaf, res.vaf_unclamped)
    mean = res.means()
    assert mean["te"].shape == (6,) and torch.allclose(mean["vaf"], res.vaf.mean(0))
    # rows of different gains differ as the reference's do (the gain is really applied)
    assert rel(res.mu_pr[:, 0], res.mu_pr[:, 3]) > 0.3 and rel(res.mu_pr[:, 5], res.mu_pr[:, 3]) > 0.3


def test_sweep_matches_the_loop_fp32(fx):
    """Same model, same seed.  Bit-equal: the device random state afterwards, the noise and the
    encoder pieces of every row (z, and te / kl through vt_te_kl_rows).  mu_pr: the decoder runs on
    B*K = 18 rows in the sweep and on B = 3 rows per forward in the loop, and its heads turned out
    bit-reproducible across these row counts (measured on the MI355X: equal), so mu_pr and with it
    the four metrics are asserted EQUAL to the loop's, not merely within the forward-output bound."""
    from vaeteb.evaluate import recon_metrics
    res, fws, y_raw = fx["res_rng"], fx["fws"], fx["args"][3]
    assert torch.equal(fx["rng_sweep"], fx["rng_loop"])
    _assert_pieces_reproduced(res, fx["pieces"])
    z = fx["z_rng"].view(3, 6, 16, 32)
    mu_loop = torch.stack([fw["mu_pr"] for fw in fws], 1)
    for k in range(6):
        assert torch.equal(z[:, k], fws[k]["z"]), k
    print("mu_pr vs the loop's: rel-L2", rel(res.mu_pr, mu_loop))
    assert torch.equal(res.mu_pr, mu_loop)
    # the loop's own KL (ATen expression, float32 mean)
    te_loop = torch.stack([k.mean(dim=(1, 2)) for k in fx["kls"]], 1)
    assert ((res.te - te_loop).abs() / te_loop.abs()).max().item() < 5e-5
    assert rel(res.kl, torch.stack(fx["kls"], 1)) < 5e-5
    # metrics of the loop's mu_pr: by recon_metrics and by numpy
    names = ("vaf", "mse", "snr", "vaf_unclamped")
    by_kernel = dict(zip(names, recon_metrics(y_raw, mu_loop)))
    ref64 = metrics64(y_raw.cpu().numpy(), mu_loop.cpu().numpy())
    _assert_kernel_bounds(torch.stack([by_kernel[k] for k in names], -1).view(18, 4), ref64, "loop mu_pr")
    for k in names:
        assert torch.equal(getattr(res, k), by_kernel[k]), k


def test_side_effects(fx):
    assert fx["training_after"] is False             # left in eval mode, as measure_transfer_entropy leaves it
    for r in (fx["res"], fx["res_rng"]):
        assert not any(t.requires_grad for t in (r.te, r.vaf, r.mse, r.snr, r.vaf_unclamped, r.mu_pr, r.kl))
    r = fx["sweep"](*fx["args"], GAINS, eps=fx["eps"])
    assert r.mu_pr is None and r.kl is None and torch.equal(r.te, fx["res"].te) and torch.equal(r.mse, fx["res"].mse)


def test_up_ablation_second_column_is_the_zeroed_forward(fx):
    m, (y_st, y_ph, x_ph, y_raw) = fx["m"], fx["args"]
    eps = fx["eps"][:, :2].contiguous()
    r = m.up_ablation(y_st, y_ph, x_ph, y_raw, eps=eps, elementwise=True, return_mu=True)
    assert list(r.gains) == [1.0, 0.0] and r.te.shape == (3, 2)
    fws, _, pieces = _loop(m, y_st, y_ph, x_ph, [1.0], eps=eps[:, :1])
    with torch.no_grad():
        fw0 = m(y_st, y_ph, torch.zeros_like(x_ph), eps=eps[:, 1].contiguous())
        mu_y, lv_full = m.target_encoder(y_st, y_ph)
        lv_p, c_lv = torch.split(lv_full, m.latent_dim_target, dim=-1)
        mu_c, lv_q = m.conditional_encoder(m.source_encoder(torch.zeros_like(x_ph)), c_lv)
    _assert_pieces_reproduced(r, pieces + [(mu_c.contiguous(), lv_q.contiguous(), mu_y.contiguous(), lv_p.contiguous())])
    mu = torch.stack([fws[0]["mu_pr"], fw0["mu_pr"]], 1)
    print("ablation mu_pr vs the forwards': rel-L2", rel(r.mu_pr, mu))
    assert torch.equal(r.mu_pr, mu)                  # on the same terms as against the loop: equal
    # the intact column is the fixture sweep's gain-1 column, the zeroed one its gain-0 column
    assert torch.equal(r.te[:, 0], fx["res"].te[:, 3]) and torch.equal(r.te[:, 1], fx["res"].te[:, 0])
    one = m.reconstruction_metrics(y_st, y_ph, x_ph, y_raw, eps=eps[:, :1].contiguous())
    assert one.te.shape == (3, 1) and torch.equal(one.te[:, 0], r.te[:, 0])


@pytest.mark.parametrize("rows", [4, 6])
def test_chunking(fx, rows):
    """rows_per_launch 4: chunks inside a recording (4 + 2 gains); 6: one recording per chunk; the
    fixture sweep (256) ran all 18 rows at once.  te / kl do not move a bit; mu_pr and the metrics on
    the same terms as against the loop: equal (the decoder heads see another row count)."""
    from vaeteb.evaluate import GainSweep
    res = fx["res"]
    r = GainSweep(fx["m"], rows_per_launch=rows)(*fx["args"], GAINS, eps=fx["eps"], elementwise=True, return_mu=True)
    assert torch.equal(r.te, res.te) and torch.equal(r.kl, res.kl)
    print(f"rows_per_launch {rows}: mu_pr rel-L2 {rel(r.mu_pr, res.mu_pr):.2e}")
    assert torch.equal(r.mu_pr, res.mu_pr)
    for k in ("vaf", "mse", "snr", "vaf_unclamped"):
        assert torch.equal(getattr(r, k), getattr(res, k)), k


def test_sweep_is_capturable_no_host_sync(fx):
    """One call with explicit eps under stream capture: any host synchronisation or .item() inside the
    call would fail the capture.  The replay reproduces the eager call."""
    sweep, args, eps, res = fx["sweep"], fx["args"], fx["eps"], fx["res"]
    sweep(*args, GAINS, eps=eps)                      # buffers and the gain table exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = sweep(*args, GAINS, eps=eps)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(r.te, res.te) and torch.equal(r.mse, res.mse) and torch.equal(r.vaf, res.vaf)
    assert torch.equal(r.snr, res.snr)


def test_frontend_entry_equals_the_field_entry():
    from vaeteb import synthetic
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.model import SeqVaeTeb
    fe = FrontEnd(FrontEndPlan(11, 4, 16, 4096, device="cuda"), load_stats(11, 4, 16, 4096))
    torch.manual_seed(0)
    m = SeqVaeTeb(sequence_length=fe.S_out, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                  cross_phase_channels=fe.C_x).cuda()
    x = torch.from_numpy(synthetic.batch(4000, 2, 4096)).cuda()
    eps = torch.randn(2, 2, fe.S_out, 32, generator=torch.Generator().manual_seed(1)).cuda()
    a = m.up_ablation(frontend=fe, x=x, eps=eps, return_mu=True)
    f = {k: v.clone() for k, v in fe(x).items()}
    b = m.up_ablation(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], eps=eps, return_mu=True)
    for k in ("te", "vaf", "mse", "snr", "vaf_unclamped", "mu_pr"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.te.shape == (2, 2) and torch.isfinite(a.te).all() and torch.isfinite(a.snr).all()
    assert not m.training
    with pytest.raises(ValueError):
        m.up_ablation(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], frontend=fe, x=x)
    with pytest.raises(ValueError):
        m.up_gain_sweep(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"])


def test_sweep_at_the_bench_precisions(fx, golden):
    g, (y_st, y_ph, x_ph, y_raw), eps = fx["g"], fx["args"], fx["eps"]
    ga = golden("model_s256_b2_amp")
    spread = max(float(ga[f"{mode}_fwrel_mu_pr"]) for mode in ("cpu_bf16", "emu_bf16"))
    m = _model(g, conv_precision="bf16", mlp_precision="bf16", head_precision="bf16", lstm_precision="16-mixed")
    r = m.up_gain_sweep(y_st, y_ph, x_ph, y_raw, gains=GAINS, eps=eps, elementwise=True, return_mu=True)
    fws, _, pieces = _loop(m, y_st, y_ph, x_ph, GAINS, eps=eps)
    assert torch.isfinite(r.te).all() and torch.isfinite(r.mu_pr).all() and torch.isfinite(r.snr).all()
    _assert_pieces_reproduced(r, pieces)
    mu_loop = torch.stack([fw["mu_pr"] for fw in fws], 1)
    e = rel(r.mu_pr, mu_loop)
    print(f"16-bit: mu_pr vs loop rel-L2 {e:.2e} (bound 2 x {spread:.2e}), bit-equal {torch.equal(r.mu_pr, mu_loop)}")
    assert e <= 2 * spread
    assert not m.training
