"""vt_layernorm_fwd / vt_layernorm_bwd (csrc/norm.hip) at every width, row count and pointer
alignment where their launchers change kernel, against the per-row fp64 formulas of
tests/norm_ref.py.  Forward + backward go through ops.layer_norm_act; the C entry points are
called directly where a case needs the raw arguments (accumulate_params, ws_floats, NULL xhat).

Forward dispatch: C <= 32 / 64 / 128 / 256: k_ln_fwd16<2 / 4 / 8 / 16> (16 lanes per row, 16 rows
per workgroup); 1024 <= C <= 4096 with C % 4 == 0 and 16-byte aligned x, y, xhat, gamma, beta:
k_ln_fwd_wide<V4>, V4 = ceil(C / 1024); everything else the wave-per-row k_ln_fwd.
Backward dispatch: C <= 256: k_ln_bwd16<2 / 4 / 8 / 16> + k_colred16 (16 columns per workgroup,
its 16-loads-in-flight loop runs from 256 partial rows on); C <= 512: k_ln_bwd<8> +
k_reduce_parts; wider: k_ln_bwd_wide (a workgroup per row) + k_reduce_parts over the R rows.
Partial rows of the two narrow paths: blocks = min(ceil(R / 64), 1024, ws_floats / 2C),
rows_per_block = ceil(R / blocks), blocks = ceil(R / rows_per_block).

Bounds: test_layernorm_act's rel-L2 1e-5 for y (and the saved xhat / rstd), 2e-5 for dx, dgamma,
dbeta.  ReLU: dy is zeroed where the reference pre-activation is within 1e-4 of the kink.

measured on MI355X, worst over all cases (bound): y 8.6e-8, xhat 5.8e-8, rstd 4.1e-8, misaligned
against aligned y 1.0e-7 (1e-5); dx 9.5e-8, dgamma 1.5e-7, dbeta 3.2e-7 (2e-5); rows of mean 1000:
y / kappa 7.0e-8, dx / kappa 7.0e-8, dgamma 3.4e-5, dbeta 2.2e-5 (2e-5 kappa = 2e-2).
"""
import pytest
import torch

import norm_ref as NR

pytestmark = pytest.mark.gpu

B_Y, B_G = 1e-5, 2e-5
EPS = 1e-5
LN_ACTS = ("none", "relu", "gelu")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb import ops as o
    return o


@pytest.fixture(scope="module")
def L(ops):
    from vaeteb import _lib
    return _lib


def _gen(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *s: torch.randn(*s, device="cuda", generator=g)


def _data(R, C, seed, mu=1.0, sigma=3.0):
    rn = _gen(seed)
    return dict(x=rn(R, C) * sigma + mu, dy=rn(R, C), gamma=1 + 0.1 * rn(C), beta=0.1 * rn(C))


def _hold(what, tag, got, ref, bound):
    v = NR.rel(got, ref)
    print(f"MEASURE ln_{what} {v:.3e} (bound {bound:.2e}) {tag}")
    assert v <= bound, (what, tag, v, bound)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _reference(d, act):
    """fp64 forward / backward (on the device for the large cases), dy masked at the ReLU kinks in place."""
    R, C = d["x"].shape
    dev = "cuda" if R * C > (1 << 18) else "cpu"
    r = {k: v.to(dev) for k, v in d.items()}
    f = NR.ln_fwd(r["x"], r["gamma"], r["beta"], act, EPS)
    m = NR.kink_mask(f["z"], act)
    share = m.float().mean().item()
    print(f"MEASURE ln_kink_share {share:.3e} R={R} C={C}")
    assert share <= max(1e-3, 1.5 / m.numel()), share     # one element of a tiny case is more than 1e-3 of it
    d["dy"][m.to("cuda")] = 0
    return f, NR.ln_bwd(d["dy"].to(dev), r["x"], r["gamma"], r["beta"], act, EPS)


def _check_op(ops, R, C, act, seed=0):
    tag = f"R={R} C={C} {act}"
    d = _data(R, C, seed + 131 * C + R)
    f, b = _reference(d, act)
    x, g, be = (d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = ops.layer_norm_act(x, g, be, act)
    (y * d["dy"]).sum().backward()
    torch.cuda.synchronize()
    _hold("y", tag, y.detach(), f["y"], B_Y)
    _hold("dx", tag, x.grad, b["dx"], B_G)
    _hold("dgamma", tag, g.grad, b["dgamma"], B_G)
    _hold("dbeta", tag, be.grad, b["dbeta"], B_G)


def _fwd(L, x, g, b, act, y, xhat, rstd):
    R, C = x.shape
    L.call("vt_layernorm_fwd", L.ptr(x), R, C, L.ptr(g), L.ptr(b), NR.ACT[act], EPS, L.ptr(y), L.ptr(xhat), L.ptr(rstd),
           L.stream())


def _bwd(L, dy, xhat, rstd, g, b, act, dx, dg, db, acc, ws, ws_floats=None):
    R, C = dy.shape
    L.call("vt_layernorm_bwd", L.ptr(dy), L.ptr(xhat), L.ptr(rstd), R, C, L.ptr(g), L.ptr(b), NR.ACT[act], L.ptr(dx),
           L.ptr(dg), L.ptr(db), acc, L.ptr(ws), ws.numel() if ws_floats is None else ws_floats, L.stream())


def _poisoned(n):
    return torch.full((n,), float("nan"), device="cuda")


# ------------------------------------------------------------------ widths
# R = 100: 7 forward workgroups of 16 rows (the last with 4), 2 backward workgroups of 50 rows
NARROW = (1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 511, 512, 513, 1000, 1023)
# R = 5: 1024 -> V4 1; 1028, 2048 -> 2; 3072 -> 3; 4092, 4096 -> 4 (1028, 4092: a partial last vector);
# 1026 (C % 4 != 0) and 4100, 5000 (past 4 V4) take the wave-per-row kernel; all take the wide backward
WIDE = (1024, 1026, 1028, 2048, 3072, 4092, 4096, 4100, 5000)


@pytest.mark.parametrize("act", LN_ACTS)
@pytest.mark.parametrize("C", NARROW + WIDE)
def test_widths(ops, C, act):
    _check_op(ops, 100 if C < 1024 else 5, C, act)


# ------------------------------------------------------------------ rows
# R: (partial workgroups, rows per workgroup) of the two narrow backward paths
ROWS = {
    1: (1, 1), 15: (1, 15), 17: (1, 17),     # less than / one more than a 16-row pass
    16385: (257, 64),      # k_colred16: one round of its 16-loads-in-flight loop (256 rows) + a one-row tail
    70001: (1015, 69),     # the 1024-workgroup cap: ceil(70001 / 1024) = 69 rows, not a multiple of 16
}


@pytest.mark.parametrize("R", sorted(ROWS))
@pytest.mark.parametrize("C", [33, 64, 256, 300])
def test_rows(ops, R, C):
    blocks = min((R + 63) // 64, 1024)
    rpb = (R + blocks - 1) // blocks
    assert ((R + rpb - 1) // rpb, rpb) == ROWS[R]
    _check_op(ops, R, C, "relu", seed=1)


# ------------------------------------------------------------------ misaligned wide rows
@pytest.mark.parametrize("which", ["x", "y", "xhat", "all"])
def test_misaligned_wide_rows_fall_back(L, which):
    """C = 1024, R = 3 with x / y / xhat one float into a larger buffer: the launcher takes the
    scalar wave-per-row kernel instead of the float4 one.  Both are two-pass, in different orders:
    each is held to the fp64 bounds, no bits required."""
    R, C = 3, 1024
    d = _data(R, C, 7)
    f = NR.ln_fwd(d["x"].cpu(), d["gamma"].cpu(), d["beta"].cpu(), "gelu", EPS)
    res = []
    for off in (0, 1):
        view = lambda k: torch.full((R * C + 4,), -7.5, device="cuda")[o(k):o(k) + R * C].view(R, C)
        o = lambda k: off if which in (k, "all") else 0
        x, y, xhat = view("x"), view("y"), view("xhat")
        x.copy_(d["x"])
        rstd = torch.empty(R, device="cuda")
        assert x.data_ptr() % 16 == 4 * o("x") and y.data_ptr() % 16 == 4 * o("y")
        _fwd(L, x, d["gamma"], d["beta"], "gelu", y, xhat, rstd)
        torch.cuda.synchronize()
        tag = f"C=1024 R=3 {which} offset {off}"
        _hold("y", tag, y, f["y"], B_Y)
        _hold("xhat", tag, xhat, f["xhat"], B_Y)
        _hold("rstd", tag, rstd, f["rstd"], B_Y)
        res.append(y.clone())
    _hold("y_vs_aligned", f"C=1024 R=3 {which}", res[1], res[0].double(), B_Y)


# ------------------------------------------------------------------ accumulate_params
@pytest.mark.parametrize("R,C", [(100, 64), (100, 300), (5, 1024)])
def test_accumulate_params(L, R, C):
    """Prefill + fresh column sums as one fp32 add on the three backward paths; dx unchanged."""
    d = _data(R, C, 9)
    y, xhat, rstd = torch.empty_like(d["x"]), torch.empty_like(d["x"]), torch.empty(R, device="cuda")
    _fwd(L, d["x"], d["gamma"], d["beta"], "gelu", y, xhat, rstd)
    rn = _gen(10)
    pg, pb = 5 * rn(C), 5 * rn(C)
    out = []
    for acc in (0, 1):
        dx = torch.empty_like(d["x"])
        dg, db = (pg.clone(), pb.clone()) if acc else (torch.empty(C, device="cuda"), torch.empty(C, device="cuda"))
        _bwd(L, d["dy"], xhat, rstd, d["gamma"], d["beta"], "gelu", dx, dg, db, acc, _poisoned(1 << 20))
        out.append((dx, dg, db))
    torch.cuda.synchronize()
    (dx0, dg0, db0), (dx1, dg1, db1) = out
    assert _bits_equal(dx0, dx1) and _bits_equal(dg1, pg + dg0) and _bits_equal(db1, pb + db0)


# ------------------------------------------------------------------ workspace
@pytest.mark.parametrize("C", [64, 300])
def test_minimum_workspace_one_block(L, C):
    """2 C floats admit one workgroup, which walks all R = 100 rows (7 or 25 adds per lane, below
    the 16-row-per-lane chains of the natural launch at large R): the same bounds; one float
    less is refused with nothing written."""
    R = 100
    tag = f"R={R} C={C} one block"
    d = _data(R, C, 11)
    _, b = _reference(d, "relu")
    y, xhat, rstd = torch.empty_like(d["x"]), torch.empty_like(d["x"]), torch.empty(R, device="cuda")
    _fwd(L, d["x"], d["gamma"], d["beta"], "relu", y, xhat, rstd)
    sent = lambda *s: torch.full(s, -7.5, device="cuda")
    dx, dg, db, ws = sent(R, C), sent(C), sent(C), _poisoned(1 << 16)
    with pytest.raises(ValueError):
        _bwd(L, d["dy"], xhat, rstd, d["gamma"], d["beta"], "relu", dx, dg, db, 0, ws, 2 * C - 1)
    torch.cuda.synchronize()
    assert all(bool((t == -7.5).all()) for t in (dx, dg, db)) and bool(torch.isnan(ws).all())
    _bwd(L, d["dy"], xhat, rstd, d["gamma"], d["beta"], "relu", dx, dg, db, 0, ws, 2 * C)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[2 * C:]).all())
    _hold("dx", tag, dx, b["dx"], B_G)
    _hold("dgamma", tag, dg, b["dgamma"], B_G)
    _hold("dbeta", tag, db, b["dbeta"], B_G)


def test_wide_workspace_below_2RC_raises(L):
    R, C = 5, 1024
    d = _data(R, C, 12)
    y, xhat, rstd = torch.empty_like(d["x"]), torch.empty_like(d["x"]), torch.empty(R, device="cuda")
    _fwd(L, d["x"], d["gamma"], d["beta"], "none", y, xhat, rstd)
    sent = lambda *s: torch.full(s, -7.5, device="cuda")
    dx, dg, db, ws = sent(R, C), sent(C), sent(C), _poisoned(2 * R * C)
    with pytest.raises(ValueError):
        _bwd(L, d["dy"], xhat, rstd, d["gamma"], d["beta"], "none", dx, dg, db, 0, ws, 2 * R * C - 1)
    torch.cuda.synchronize()
    assert all(bool((t == -7.5).all()) for t in (dx, dg, db)) and bool(torch.isnan(ws).all())
    _bwd(L, d["dy"], xhat, rstd, d["gamma"], d["beta"], "none", dx, dg, db, 0, ws, 2 * R * C)
    b = NR.ln_bwd(d["dy"].cpu(), d["x"].cpu(), d["gamma"].cpu(), d["beta"].cpu(), "none", EPS)
    _hold("dx", "wide, exact workspace", dx, b["dx"], B_G)
    _hold("dgamma", "wide, exact workspace", dg, b["dgamma"], B_G)


# ------------------------------------------------------------------ saved state
@pytest.mark.parametrize("R,C", [(100, 17), (100, 64), (100, 300), (5, 1024), (5, 4096), (5, 5000)])
def test_saved_state_and_null_outputs(L, R, C):
    """xhat and rstd against the reference; with xhat = NULL and rstd = NULL the forward still
    runs (a NULL xhat is 16-byte aligned: the wide kernel stays selected) and y has the same bits."""
    tag = f"R={R} C={C}"
    d = _data(R, C, 13)
    f = NR.ln_fwd(d["x"].cpu(), d["gamma"].cpu(), d["beta"].cpu(), "relu", EPS)
    y, xhat, rstd = torch.empty_like(d["x"]), torch.empty_like(d["x"]), torch.empty(R, device="cuda")
    _fwd(L, d["x"], d["gamma"], d["beta"], "relu", y, xhat, rstd)
    y2 = torch.empty_like(y)
    _fwd(L, d["x"], d["gamma"], d["beta"], "relu", y2, None, None)
    torch.cuda.synchronize()
    _hold("y", tag, y, f["y"], B_Y)
    _hold("xhat", tag, xhat, f["xhat"], B_Y)
    _hold("rstd", tag, rstd, f["rstd"], B_Y)
    assert _bits_equal(y, y2)


# ------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("R,C", [(100, 64), (5, 4096)])
def test_conditioning_mean_1000(ops, R, C, act):
    """Rows with mean 1000 and spread 1: per row the bounds times kappa_r = 1 + |mean_r| rstd_r
    (a row mean known to fp32's 6e-8 relative is known to 6e-5 absolute, which xhat sees); a
    one-pass variance would lose the spread entirely.  Smooth activations, as a ReLU here
    would test the side of the kink, not the conditioning."""
    tag = f"R={R} C={C} {act} mu=1000"
    d = _data(R, C, 14, mu=1000.0, sigma=1.0)
    f, b = _reference(d, act)
    x, g, be = (d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = ops.layer_norm_act(x, g, be, act)
    (y * d["dy"]).sum().backward()
    torch.cuda.synchronize()
    xr = d["x"].cpu().double()
    kappa = 1 + xr.mean(1).abs() * f["rstd"]
    for name, got, ref, bound in (("y", y.detach(), f["y"], B_Y), ("dx", x.grad, b["dx"], B_G)):
        e = (got.cpu().double() - ref).norm(dim=1) / ref.norm(dim=1)
        worst = (e / kappa).max().item()
        print(f"MEASURE ln_{name}/kappa {worst:.3e} (bound {bound:.2e}) {tag}")
        assert worst <= bound, (name, worst)
    _hold("dgamma/kappa", tag, g.grad, b["dgamma"], B_G * kappa.max().item())
    _hold("dbeta/kappa", tag, be.grad, b["dbeta"], B_G * kappa.max().item())
