"""The batched transfer-entropy-vs-shift sweep (vaeteb.te.ShiftSweep, ref/model/graph_model.py:
1210-1458) on the GPU against the literal loop over the existing public API — FrontEnd.__call__ on
the rolled window, SeqVaeTeb.measure_transfer_entropy, one (recording, shift) at a time — and
against the reference's own values (tests/golden/te_shift_j11_n4096*.npz).

Bounds:
* features: equality.  A sweep row runs the per-item code of the front-end's kernels on the same
  values (the rolled gather feeds the same FFT, the split pair kernels share the item body).
* vt_te_kl_rows vs float64: 1e-6 relative, what tests/test_gpu_elbo_optim.py holds k_latent_fwd's KL
  to (there a scalar; here the row means each, and the elementwise tensor in the relative L2 norm).
* transfer entropy vs the loop: the encoders are row-independent in eval mode, and the sweep's
  posterior / prior pieces are asserted bit-equal to the loop's (through the same KL kernel).  The
  loop's own KL is ATen's elementwise expression and fp32 mean, vt_te_kl_rows is k_latent_fwd's
  contracted expression and a double sum, so te / kl against measure_transfer_entropy itself are
  held to the project's transfer-entropy bound, rel < 5e-5 (tests/test_gpu_model.py:258).
* vs the reference fixture: max(5e-5 |te|, 1.5 x the loop's error on the same inputs).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIX_SHIFTS = [0, -1, 7, -240]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _roll_up(x, shift):
    xr = x.clone()
    xr[:, 1] = torch.roll(x[:, 1], int(shift), dims=-1)
    return xr


def _model(fe, golden=None, **prec):
    """det_fill_ weights (sequence_length only sizes the decoder head, which the transfer entropy
    never runs) and, with `golden`, the fixture's BatchNorm running buffers."""
    from golden_util import det_fill_
    from vaeteb.model import SeqVaeTeb
    m = det_fill_(SeqVaeTeb(sequence_length=16, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                            cross_phase_channels=fe.C_x, **prec))
    if golden is not None:
        sd = m.state_dict()
        for i, k in enumerate(list(golden["bn_names"])):
            sd[k].copy_(torch.from_numpy(golden[f"bn_{i}"]))
    return m.cuda()


def _loop(m, fe, x, shifts):
    """The literal loop: (te (B, K), kl (B, K, S, L), pieces per row)."""
    te, kl, pieces = [], [], []
    for b in range(x.shape[0]):
        for s in shifts:
            f = fe(_roll_up(x[b:b + 1], s))
            k = m.measure_transfer_entropy(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], reduce_mean=False)
            kl.append(k[0])
            te.append(k.mean())
            with torch.no_grad():   # what encode() runs (eval mode by now), kept before mu_c + mu_y
                mu_y, lv_full = m.target_encoder(f["fhr_st"], f["fhr_ph"])
                lv_p, c_lv = torch.split(lv_full, m.latent_dim_target, dim=-1)
                mu_c, lv_q = m.conditional_encoder(m.source_encoder(f["fhr_up_ph"]), c_lv)
                pieces.append((mu_c, lv_q, mu_y, lv_p.contiguous()))
    B, K = x.shape[0], len(shifts)
    return torch.stack(te).view(B, K), torch.stack(kl).view(B, K, *kl[0].shape), pieces


def _kl_rows(mu_c, lv_q, mu_y, lv_p, B, K, elementwise=True):
    from vaeteb import _lib
    n = mu_c[0].numel()
    te = torch.empty(B * K, device="cuda")
    kl = torch.empty_like(mu_c) if elementwise else None
    _lib.call("vt_te_kl_rows", _lib.ptr(mu_c), _lib.ptr(lv_q), _lib.ptr(mu_y), _lib.ptr(lv_p), B, K, n,
              _lib.ptr(te), _lib.ptr(kl), _lib.stream())
    return te, kl


def _assert_rows_reproduced(res, pieces):
    """The encoders' outputs of each sweep row are the loop's, bit for bit: the loop's batch-1 pieces
    through the same KL kernel, one row at a time, give the sweep's numbers exactly."""
    rows = res.te.numel()
    for r, (mu_c, lv_q, mu_y, lv_p) in enumerate(pieces):
        te_r, kl_r = _kl_rows(mu_c.contiguous(), lv_q.contiguous(), mu_y.contiguous(), lv_p.contiguous(), 1, 1)
        assert torch.equal(kl_r[0], res.kl.view(rows, *kl_r.shape[1:])[r]), r
        assert torch.equal(te_r[0], res.te.view(-1)[r]), r


@pytest.fixture(scope="module")
def fx(golden):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.te import ShiftSweep
    g, gi = golden("te_shift_j11_n4096"), golden("te_shift_j11_n4096_in")
    assert list(g["shifts"]) == FIX_SHIFTS
    fe = FrontEnd(FrontEndPlan(11, 4, 16, 4096, device="cuda"), load_stats(11, 4, 16, 4096))
    x = torch.from_numpy(gi["x"]).cuda()
    m = _model(fe, g)
    sweep = ShiftSweep(m, fe)
    torch.cuda.manual_seed(1234)
    m.train()
    loop_te, loop_kl, pieces = _loop(m, fe, x, FIX_SHIFTS)
    torch.cuda.synchronize()
    # encode() above draws nothing; measure_transfer_entropy drew one noise tensor per row
    rng_loop = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(1234)
    m.train()
    res = sweep(x, FIX_SHIFTS, elementwise=True, return_features=True)
    torch.cuda.synchronize()
    rng_sweep = torch.cuda.get_rng_state()
    return dict(g=g, fe=fe, x=x, m=m, sweep=sweep, res=res, loop_te=loop_te, loop_kl=loop_kl, pieces=pieces,
                rng_loop=rng_loop, rng_sweep=rng_sweep, training_after=m.training)


# ------------------------------------------------------------------ features
@pytest.mark.parametrize("cfg", ["j11_half_image", "j11_n5760_full_image", "j6_generic"])
def test_sweep_features_bit_equal_frontend_on_rolled_windows(fx, cfg):
    from vaeteb import synthetic
    from vaeteb.frontend import FrontEnd, FrontEndPlan, load_stats
    from vaeteb.te import ShiftSweep
    if cfg == "j11_half_image":
        fe, x, shifts = fx["fe"], fx["x"], FIX_SHIFTS + [-4097]
        assert fe.plan.n_pad == 8192 and fe.plan.pad_left == 2048
        m = fx["m"]
    elif cfg == "j11_n5760_full_image":
        fe = FrontEnd(FrontEndPlan(11, 4, 16, 5760, device="cuda"), load_stats(11, 4, 16, 4096), trim=30)
        assert fe.plan.n_pad == 8192 and fe.S_out == 300
        x, shifts = torch.from_numpy(synthetic.batch(2000, 1, 5760)).cuda(), [-240, 7]
        m = _model(fe)
    else:
        # (6, 1, 16, 4096) pads to 8192 as well; the same bank on 2048-point windows (n_pad 4096) is the
        # nearest plan that takes the generic k_fe_pairs / k_fe_wavelet path (the channel statistics
        # depend on (J, Q, T) only).  -4097 = -1 mod 2048 too.
        fe = FrontEnd(FrontEndPlan(6, 1, 16, 2048, device="cuda"), load_stats(6, 1, 16, 4096))
        assert fe.plan.n_pad != 8192
        x, shifts = fx["x"][:, :, :2048].contiguous(), FIX_SHIFTS + [-4097]
        m = _model(fe)
    res = ShiftSweep(m, fe)(x, shifts, return_features=True)
    B, K = x.shape[0], len(shifts)
    assert res.x_ph.shape == (B, K, fe.S_out, fe.C_x) and res.kl is None and res.te.shape == (B, K)
    for k, s in enumerate(shifts):
        ref = fe(_roll_up(x, s))["fhr_up_ph"]
        assert torch.equal(res.x_ph[:, k], ref), (cfg, s, (res.x_ph[:, k] - ref).abs().max().item())
    if -4097 in shifts:
        assert torch.equal(res.x_ph[:, shifts.index(-4097)], res.x_ph[:, shifts.index(-1)])
    # shifts that differ (mod N) give different features: the roll is really applied
    assert not torch.equal(res.x_ph[:, 0], res.x_ph[:, 1])
    assert torch.isfinite(res.te).all()


# ------------------------------------------------------------------ KL kernel
def test_te_kl_rows_vs_float64_deterministic_and_split_invariant():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb.model import SeqVaeTeb
    B, K, S, L = 2, 3, 16, 32
    gen = torch.Generator().manual_seed(11)
    mu_c, mu_y = torch.randn(B * K, S, L, generator=gen), torch.randn(B, S, L, generator=gen)
    lv_q = torch.rand(B * K, S, L, generator=gen) * 20 - 10
    lv_p = torch.rand(B, S, L, generator=gen) * 20 - 10
    d = [t.cuda() for t in (mu_c, lv_q, mu_y, lv_p)]
    te, kl = _kl_rows(*d, B, K)
    ex = lambda t: t.double().repeat_interleave(K, 0)            # prior row r // K
    ref = SeqVaeTeb.kld_elementwise(ex(mu_y), ex(lv_p), mu_c.double() + ex(mu_y), lv_q.double())
    ref_te = ref.mean(dim=(1, 2))
    print("kl rel L2", rel(kl, ref), "te rel", ((te.cpu().double() - ref_te).abs() / ref_te.abs()).max().item())
    assert rel(kl, ref) <= 1e-6
    assert ((te.cpu().double() - ref_te).abs() <= 1e-6 * ref_te.abs()).all()
    te2, kl2 = _kl_rows(*d, B, K)
    assert torch.equal(te, te2) and torch.equal(kl, kl2)
    te_only, _ = _kl_rows(*d, B, K, elementwise=False)
    assert torch.equal(te, te_only)
    # two calls of one recording each: the same row means
    halves = [_kl_rows(d[0][b * K:(b + 1) * K].contiguous(), d[1][b * K:(b + 1) * K].contiguous(),
                       d[2][b:b + 1].contiguous(), d[3][b:b + 1].contiguous(), 1, K)[0] for b in range(B)]
    assert torch.equal(torch.cat(halves), te)
    # ... and a split inside a recording
    a = _kl_rows(d[0][:2].contiguous(), d[1][:2].contiguous(), d[2][:1].contiguous(), d[3][:1].contiguous(), 1, 2)[0]
    assert torch.equal(a, te[:2])


# ------------------------------------------------------------------ TE
def test_sweep_matches_the_loop_fp32(fx):
    res, m = fx["res"], fx["m"]
    B, K = 2, len(FIX_SHIFTS)
    assert res.te.shape == (B, K) and res.te.dtype == torch.float32 and res.te.is_cuda
    assert res.kl.shape == fx["loop_kl"].shape and list(res.shifts) == FIX_SHIFTS
    _assert_rows_reproduced(res, fx["pieces"])
    # against measure_transfer_entropy's own (ATen) KL and mean
    e_te = ((res.te - fx["loop_te"]).abs() / fx["loop_te"].abs()).max().item()
    print("te vs loop: max rel", e_te, "kl vs loop: rel L2", rel(res.kl, fx["loop_kl"]),
          "bit-equal te:", torch.equal(res.te, fx["loop_te"]))
    assert e_te < 5e-5
    assert rel(res.kl, fx["loop_kl"]) < 5e-5
    assert torch.equal(res.argmin.cpu(), torch.from_numpy(fx["loop_te"].cpu().numpy().argmin(1)))
    assert res.argmin.shape == (B,)


def test_sweep_matches_the_reference_fixture(fx):
    ref = torch.from_numpy(fx["g"]["te"]).double()
    te, loop = fx["res"].te.cpu().double(), fx["loop_te"].cpu().double()
    err, err_loop = (te - ref).abs(), (loop - ref).abs()
    allowed = torch.maximum(5e-5 * ref.abs(), 1.5 * err_loop)
    print("sweep rel err vs reference", (err / ref.abs()).numpy(), "loop rel err", (err_loop / ref.abs()).numpy())
    assert (err <= allowed).all()


def test_chunking_does_not_change_a_bit(fx):
    from vaeteb.te import ShiftSweep
    res = fx["res"]
    for rows in (3, 4, 5):      # inside a recording (3 + 1), one recording per chunk (4, 5)
        r = ShiftSweep(fx["m"], fx["fe"], rows_per_launch=rows)(fx["x"], FIX_SHIFTS, elementwise=True,
                                                                return_features=True)
        assert torch.equal(r.te, res.te) and torch.equal(r.kl, res.kl) and torch.equal(r.x_ph, res.x_ph), rows
        assert torch.equal(r.argmin, res.argmin)


def test_sweep_at_the_bench_precisions(fx):
    fe, x = fx["fe"], fx["x"]
    m = _model(fe, fx["g"], conv_precision="bf16", mlp_precision="bf16", head_precision="bf16",
               lstm_precision="16-mixed")
    res = m.transfer_entropy_vs_shift(fe, x, FIX_SHIFTS, elementwise=True)
    loop_te, loop_kl, pieces = _loop(m, fe, x, FIX_SHIFTS)
    assert torch.isfinite(res.te).all() and torch.isfinite(res.kl).all()
    _assert_rows_reproduced(res, pieces)
    e_te = ((res.te - loop_te).abs() / loop_te.abs()).max().item()
    print("16-bit: te vs loop max rel", e_te, "kl rel L2", rel(res.kl, loop_kl))
    assert e_te < 5e-5
    assert rel(res.kl, loop_kl) < 5e-5
    assert torch.equal(res.argmin.cpu(), torch.from_numpy(loop_te.cpu().numpy().argmin(1)))


def test_side_effects_match_the_loop(fx):
    res = fx["res"]
    assert fx["training_after"] is False                       # left in eval mode, as the reference
    assert not res.te.requires_grad and not res.kl.requires_grad and not res.x_ph.requires_grad
    assert torch.equal(fx["rng_sweep"], fx["rng_loop"])       # one noise draw per (recording, shift) row


def test_frontend_path_untouched_by_a_sweep(fx):
    fe, x = fx["fe"], fx["x"]
    before = {k: v.clone() for k, v in fe(x).items()}
    fx["sweep"](x, FIX_SHIFTS, elementwise=True, return_features=True)
    after = fe(x)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_default_shifts_through_the_model_method(fx):
    """The reference's 61 left shifts on one recording: K > the fixture's, more rows than recordings."""
    from vaeteb.te import left_shifts
    r = fx["m"].transfer_entropy_vs_shift(fx["fe"], fx["x"][:1])
    assert r.te.shape == (1, 61) and np.array_equal(r.shifts, left_shifts()) and torch.isfinite(r.te).all()
    # shift 0 is the grid's last column and the fixture sweep's first: a row does not depend on its batch
    assert torch.equal(r.te[0, -1], fx["res"].te[0, 0])
