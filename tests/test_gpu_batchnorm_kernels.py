"""The BatchNorm entry points of csrc/norm.hip, each called through the C ABI (launcher + kernel)
and compared with the plain fp64 formulas of tests/norm_ref.py at the row / channel counts where
the launchers change what they do.

Structure of a column pass (bn_blocks, col_partial_fin; mirrored by _bn_blocks below, which the
cases assert their commented block / group counts against):
    blocks = min(ceil(M / 256), cap),  cap = 512 (BN_FOLD_BLOCKS) for C <= 128, else 2048
    rpb    = ceil4(ceil(M / blocks)),  blocks = ceil(M / rpb)
    C <= 128: in-kernel finalize, arrival groups of BN_GB = 64 blocks (one group: single stage;
              more: the last group to finish sums the group sums); C > 128: k_bn_finalize.
    In a block Tp = colp_threads(C) threads are active; 4 Tp / C thread groups per channel are
    combined in LDS, by a wave per channel when 4 Tp / C >= 256 (C <= 4), else by one thread.

Conventions: the workspace is NaN before every call (a finaliser reading a partial nobody wrote
shows up), 1 << 20 floats unless the case is about the workspace; x = randn sigma_c + mu_c with
|mu_c| in [1, 3] (either sign) and sigma_c in [0.5, 2], so every block's partial is a visible share
of its sum and a mean's condition number sum|x| / |sum x| stays below ~3 (a mean near zero would
be judged by its cancellation, not by the reduction); gamma = 1 + 0.1 randn, beta = 0.1 randn;
non-trivial running statistics on entry; the backward is fed the kernel's own fp32 mean / rstd
and judged against the from-scratch fp64 backward.  ReLU: dy is zeroed, for the reference and the
kernel alike, where the reference pre-activation is within 1e-4 of the kink (asserted <= 1e-3 of
the elements).

Bounds (rel-L2; the single-op bounds of test_conv_bn_act, not tuned to these kernels):
    y 1e-5;  dx, dgamma, dbeta 5e-5;  mean, rstd, run_mean, run_var 1e-6 (over channels).
A lane's sequential fp32 chain is about rpb C / (4 Tp) + 4 Tp / C adds (_chain), everything after
it is in double: at most 48 adds for C >= 32, where a random walk of sqrt(48) 2^-24 = 4e-7 sits
under 1e-6, and up to 205 at C = 5 (one thread adds 204 LDS partials), where the walk relative to
the final sum is 2^-24 sqrt(n / 3) = 5e-7 (the early adds act on small running sums) and is
averaged over the blocks besides: the natural launches all keep 1e-6.  Where the workspace forces
fewer, longer blocks the statistics bound is scaled by sqrt(chain / 48) (_stat_bound), the same
headroom over the same error model.

measured on MI355X, worst over all cases (bound): mean 2.6e-7, rstd 1.3e-7, run_mean 2.7e-7,
run_var 2.7e-7 (1e-6; the 2.6e-7 is the one-block workspace case, 1.1e-7 elsewhere); y 6.5e-7
(1e-5); dx 6.0e-7, dgamma 8.4e-7, dbeta 5.0e-7 (5e-5); mu = 1000: y / kappa 5.6e-8, dx / kappa
4.7e-8, dgamma 4.7e-5, dbeta 1.6e-5 (5e-5 kappa = 5e-2); apply 9.7e-8, eval 8.3e-8, act fwd 6.0e-8
(1e-5), act bwd 1.1e-7 (5e-5); masked ReLU kinks at most 1.8e-4 of a case's elements (1e-3).
The whole module runs in about 4 s, the 237 MB case of the separate finaliser in 0.05 s.
"""
import math

import pytest
import torch

import norm_ref as NR

pytestmark = pytest.mark.gpu

B_Y, B_G, B_S = 1e-5, 5e-5, 1e-6
EPS = 1e-5
WS_FLOATS = 1 << 20
ACTS = ("none", "relu", "gelu", "tanh")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb import _lib
    return _lib


# ------------------------------------------------------------------ the launcher's arithmetic
BN_GB, BN_FOLD_BLOCKS, NT = 64, 512, 256


def _bn_blocks(M, C, ws_floats=WS_FLOATS):
    """(blocks, rows per block, arrival groups or 0 with the separate finaliser): bn_blocks."""
    need = lambda b: ((2 * C * b + 1) & ~1) + 4 * C * ((b + BN_GB - 1) // BN_GB)
    blocks = min((M + 255) // 256, BN_FOLD_BLOCKS if C <= 128 else 2048)
    while blocks > 1 and need(blocks) > ws_floats:
        blocks = min(blocks * 15 // 16, blocks - 1)
    if need(blocks) > ws_floats:
        return 0, 0, 0
    rpb = ((M + blocks - 1) // blocks + 3) // 4 * 4
    blocks = (M + rpb - 1) // rpb
    return blocks, rpb, ((blocks + BN_GB - 1) // BN_GB if C <= 128 else 0)


def _colp_threads(C):
    P = C // (4 if C % 4 == 0 else 2 if C % 2 == 0 else 1)
    return NT // P * P


def _chain(M, C, ws_floats=WS_FLOATS):
    """Longest sequential fp32 add chain of a column pass: a thread's rows, then the LDS combine."""
    _, rpb, _ = _bn_blocks(M, C, ws_floats)
    Tp = _colp_threads(C)
    groups = 4 * Tp // C
    return math.ceil(rpb * C / (4 * Tp)) + (math.ceil(groups / 64) + 6 if groups >= 256 else groups)


def _stat_bound(M, C, ws_floats):
    return B_S * max(1.0, math.sqrt(_chain(M, C, ws_floats) / 48.0))


# ------------------------------------------------------------------ data and kernel runs
def _gen(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (lambda *s: torch.randn(*s, device="cuda", generator=g),
            lambda *s: torch.rand(*s, device="cuda", generator=g))


def _data(M, C, seed, mu=None, sigma=None):
    rn, ru = _gen(seed)
    full = lambda v: torch.full((C,), float(v), device="cuda")
    mu_c = (1 + 2 * ru(C)) * (2 * (ru(C) < 0.5).float() - 1) if mu is None else full(mu)
    sg_c = 0.5 + 1.5 * ru(C) if sigma is None else full(sigma)
    x = rn(M, C) * sg_c + mu_c
    return dict(x=x, dy=rn(M, C), gamma=1 + 0.1 * rn(C), beta=0.1 * rn(C), rm=0.3 * rn(C), rv=0.5 + ru(C))


def _poisoned(n=WS_FLOATS):
    return torch.full((n,), float("nan"), device="cuda")


def _k_fwd(L, d, act, mom=0.9, ws=None, ws_floats=None):
    x = d["x"]
    M, C = x.shape
    ws = _poisoned() if ws is None else ws
    o = dict(y=torch.empty_like(x), mean=torch.empty(C, device="cuda"), rstd=torch.empty(C, device="cuda"),
             rm=d["rm"].clone(), rv=d["rv"].clone())
    L.call("vt_batchnorm_fwd", L.ptr(x), M, C, L.ptr(d["gamma"]), L.ptr(d["beta"]), NR.ACT[act], EPS, mom, L.ptr(o["y"]),
           L.ptr(o["mean"]), L.ptr(o["rstd"]), L.ptr(o["rm"]), L.ptr(o["rv"]), L.ptr(ws),
           ws.numel() if ws_floats is None else ws_floats, L.stream())
    return o


def _k_bwd(L, d, dy, mean, rstd, act, ws=None, ws_floats=None, acc=0, dg=None, db=None):
    x = d["x"]
    M, C = x.shape
    ws = _poisoned() if ws is None else ws
    o = dict(dx=torch.empty_like(x), dgamma=torch.empty(C, device="cuda") if dg is None else dg,
             dbeta=torch.empty(C, device="cuda") if db is None else db)
    L.call("vt_batchnorm_bwd", L.ptr(dy), L.ptr(x), M, C, L.ptr(mean), L.ptr(rstd), L.ptr(d["gamma"]), L.ptr(d["beta"]),
           NR.ACT[act], L.ptr(o["dx"]), L.ptr(o["dgamma"]), L.ptr(o["dbeta"]), acc, L.ptr(ws),
           ws.numel() if ws_floats is None else ws_floats, L.stream())
    return o


def _k_coef(L, d, dy, mean, rstd, act, ws=None, acc=0, dg=None, db=None):
    x = d["x"]
    M, C = x.shape
    ws = _poisoned() if ws is None else ws
    o = dict(bnp=torch.full((6 * C,), float("nan"), device="cuda"),
             dgamma=torch.empty(C, device="cuda") if dg is None else dg,
             dbeta=torch.empty(C, device="cuda") if db is None else db)
    L.call("vt_batchnorm_bwd_coef", L.ptr(dy), L.ptr(x), M, C, L.ptr(mean), L.ptr(rstd), L.ptr(d["gamma"]),
           L.ptr(d["beta"]), NR.ACT[act], L.ptr(o["dgamma"]), L.ptr(o["dbeta"]), acc, L.ptr(o["bnp"]), L.ptr(ws),
           ws.numel(), L.stream())
    return o


def _ref_dev(M, C):
    """Small cases take their reference on the CPU, the large ones with torch on the device."""
    return "cuda" if M * C > (1 << 18) else "cpu"


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _hold(what, tag, got, ref, bound):
    v = NR.rel(got, ref)
    print(f"MEASURE {what} {v:.3e} (bound {bound:.2e}) {tag}")
    assert v <= bound, (what, tag, v, bound)


def _mask_kinks(d, z, act, tag):
    """Zero dy (in place: the kernel run and the reference share it) at the ReLU kinks."""
    m = NR.kink_mask(z, act).to(d["dy"].device)
    share = m.float().mean().item()
    print(f"MEASURE kink_share {share:.3e} (bound 1.00e-03) {tag}")
    assert share <= 1e-3, (tag, share)
    d["dy"][m] = 0


def _check_fwd_bwd(L, M, C, act, mom=0.9, seed=0, ws_floats=None, stat_bound=B_S):
    tag = f"M={M} C={C} {act}"
    d = _data(M, C, seed + 1000 * C + M)
    dev = _ref_dev(M, C)
    r = _to(d, dev)
    fr = NR.bn_fwd(r["x"], r["gamma"], r["beta"], act, EPS, r["rm"], r["rv"], mom)
    _mask_kinks(d, fr["z"], act, tag)
    br = NR.bn_bwd(d["dy"].to(dev), r["x"], r["gamma"], r["beta"], act, EPS)
    ws = _poisoned()
    f = _k_fwd(L, d, act, mom, ws, ws_floats)
    ws.fill_(float("nan"))
    b = _k_bwd(L, d, d["dy"], f["mean"], f["rstd"], act, ws, None if ws_floats is None else ws_floats + 2 * C)
    torch.cuda.synchronize()
    _hold("mean", tag, f["mean"], fr["mean"], stat_bound)
    _hold("rstd", tag, f["rstd"], fr["rstd"], stat_bound)
    _hold("run_mean", tag, f["rm"], fr["run_mean"], stat_bound)
    _hold("run_var", tag, f["rv"], fr["run_var"], stat_bound)
    _hold("y", tag, f["y"], fr["y"], B_Y)
    _hold("dx", tag, b["dx"], br["dx"], B_G)
    _hold("dgamma", tag, b["dgamma"], br["dgamma"], B_G)
    _hold("dbeta", tag, b["dbeta"], br["dbeta"], B_G)


# ------------------------------------------------------------------ 1. rows x channels sweep
# M: (blocks, arrival groups) for C <= 128
SWEEP_M = {
    1: (1, 1),          # var = 0, rstd = 1 / sqrt(eps), running variance takes the M = 1 branch
    3: (1, 1),          # fewer than four elements at C = 1: scalar tail only
    5: (1, 1),          # one float4 + a scalar tail at C = 1
    257: (2, 1),        # rpb 132
    4099: (17, 1),      # rpb 244; M C not a multiple of 4 for odd C
    16384: (64, 1),     # rpb 256: one full group, single-stage finalize
    16385: (65, 2),     # rpb 256: a second group with one member
    131072: (512, 8),   # rpb 256: 8 groups, exactly at the BN_FOLD_BLOCKS cap
    131073: (505, 8),   # cap binding: 513 -> 512, rpb 260, 505 blocks, last group 57 members
}
# C: 1, 2, 3, 4 take the wave-per-channel LDS combine (4 Tp / C = 1024, 512, 340, 256 >= 256); odd C
# leave threads idle (Tp = 255 at 3 and 5, 252 at 7, 253 at 11, 174 at 87, 254 at 127); 128 is the last
# in-kernel-finalize width (256 finalize threads)
SWEEP_C = (1, 2, 3, 4, 5, 7, 11, 16, 87, 127, 128)
SWEEP = sorted({(M, C) for M in SWEEP_M for C in (1, 3, 16)} | {(M, C) for M in (4099, 16385) for C in SWEEP_C}
               | {(131073, 128)})


@pytest.mark.parametrize("M,C", SWEEP)
def test_fwd_bwd_relu(L, M, C):
    blocks, _, groups = _bn_blocks(M, C)
    assert (blocks, groups) == SWEEP_M[M]
    _check_fwd_bwd(L, M, C, "relu")


@pytest.mark.parametrize("act", ["tanh", "none"])
@pytest.mark.parametrize("M,C", [(1, 1), (5, 3), (4099, 7), (16385, 16), (16385, 87), (131073, 3)])
def test_fwd_bwd_tanh_none(L, M, C, act):
    _check_fwd_bwd(L, M, C, act, seed=1)


def test_fwd_momentum_01(L):
    _check_fwd_bwd(L, 16385, 11, "relu", mom=0.1, seed=2)


# ------------------------------------------------------------------ 2. separate finaliser
# C > 128: cap 2048, k_bn_finalize (one workgroup per channel, thread t sums partials t, t + 256, ...)
FIN = [
    (4099, 129, 17), (4099, 130, 17), (4099, 255, 17), (4099, 256, 17),   # 17 partials: 239 threads idle
    (70001, 129, 274),      # rpb 256, 274 partials: threads 0..17 sum two
    (458760, 129, 1793),    # rpb 256, 1793 partials: thread 0 runs the eight-way unrolled loop once
]


@pytest.mark.parametrize("M,C,blocks", FIN)
def test_fwd_bwd_separate_finaliser(L, M, C, blocks):
    """(458760, 129) is 237 MB per tensor, its fp64 reference taken on the device (0.05 s on MI355X)."""
    assert _bn_blocks(M, C)[::2] == (blocks, 0)
    _check_fwd_bwd(L, M, C, "relu")


# ------------------------------------------------------------------ 3. conditioning
@pytest.mark.parametrize("act", ["tanh", "none"])
def test_conditioning_mean_1000(L, act):
    """mu_c = 1000, sigma_c = 1: the statistics keep their bounds (two-pass variance; a one-pass
    E[x^2] - E[x]^2 in fp32 would lose var = 1 under 1e6 entirely), and y, dx, dgamma, dbeta keep
    theirs times kappa_c = 1 + |mu_c| rstd_c per channel: a mean known to 1e-6 relative is known
    to 1e-3 absolute, which is what xhat = (x - mean) rstd sees.  Smooth activations: a ReLU
    here would test which side of the kink 1e-3 of slack falls on, not the conditioning."""
    M, C = 16385, 16
    tag = f"M={M} C={C} {act} mu=1000"
    d = _data(M, C, 77, mu=1000.0, sigma=1.0)
    fr = NR.bn_fwd(d["x"], d["gamma"], d["beta"], act, EPS, d["rm"], d["rv"], 0.9)
    br = NR.bn_bwd(d["dy"], d["x"], d["gamma"], d["beta"], act, EPS)
    f = _k_fwd(L, d, act)
    b = _k_bwd(L, d, d["dy"], f["mean"], f["rstd"], act)
    torch.cuda.synchronize()
    for k, rk in (("mean", "mean"), ("rstd", "rstd"), ("rm", "run_mean"), ("rv", "run_var")):
        _hold(rk, tag, f[k], fr[rk], B_S)
    kappa = 1 + fr["mean"].abs() * fr["rstd"]
    for name, got, ref, bound in (("y", f["y"], fr["y"], B_Y), ("dx", b["dx"], br["dx"], B_G)):
        e = (got.double() - ref).norm(dim=0) / ref.norm(dim=0)
        worst = (e / kappa).max().item()
        print(f"MEASURE {name}/kappa {worst:.3e} (bound {bound:.2e}) {tag}")
        assert worst <= bound, (name, worst)
    _hold("dgamma/kappa", tag, b["dgamma"].double() / kappa, br["dgamma"] / kappa, B_G * kappa.max().item())
    _hold("dbeta/kappa", tag, b["dbeta"].double() / kappa, br["dbeta"] / kappa, B_G * kappa.max().item())


# ------------------------------------------------------------------ 4. workspace behaviour
@pytest.mark.parametrize("M,C", [(4099, 16), (4099, 129)])
def test_minimum_workspace_one_block(L, M, C):
    """6 C floats (forward) / 8 C (backward: + the fresh sums at the end of ws) admit exactly one
    block, which loops over all rows: chain = ceil(4100 C / (4 Tp)) + 4 Tp / C = 65 + 64 = 129
    adds at C = 16 (statistics bound 1e-6 sqrt(129 / 48) = 1.64e-6) and 1025 + 4 at C = 129
    (Tp = 129: 4.63e-6); y, dx, dgamma, dbeta keep their bounds."""
    assert _bn_blocks(M, C, 6 * C)[0] == 1 and _bn_blocks(M, C, 6 * C - 1)[0] == 0
    assert _chain(M, C, 6 * C) == {16: 129, 129: 1029}[C]
    _check_fwd_bwd(L, M, C, "relu", seed=3, ws_floats=6 * C, stat_bound=_stat_bound(M, C, 6 * C))


@pytest.mark.parametrize("C", [16, 129])
def test_workspace_one_float_short_raises_and_writes_nothing(L, C):
    M = 4099
    d = _data(M, C, 5)
    sent = lambda *s: torch.full(s, -7.5, device="cuda")
    ws = _poisoned()
    y, mean, rstd, rm, rv = sent(M, C), sent(C), sent(C), d["rm"].clone(), d["rv"].clone()
    with pytest.raises(ValueError):
        L.call("vt_batchnorm_fwd", L.ptr(d["x"]), M, C, L.ptr(d["gamma"]), L.ptr(d["beta"]), 1, EPS, 0.9, L.ptr(y),
               L.ptr(mean), L.ptr(rstd), L.ptr(rm), L.ptr(rv), L.ptr(ws), 6 * C - 1, L.stream())
    dx, dg, db = sent(M, C), sent(C), sent(C)
    with pytest.raises(ValueError):
        L.call("vt_batchnorm_bwd", L.ptr(d["dy"]), L.ptr(d["x"]), M, C, L.ptr(d["rm"]), L.ptr(d["rv"]), L.ptr(d["gamma"]),
               L.ptr(d["beta"]), 1, L.ptr(dx), L.ptr(dg), L.ptr(db), 0, L.ptr(ws), 8 * C - 1, L.stream())
    bnp = sent(6 * C)
    with pytest.raises(ValueError):
        L.call("vt_batchnorm_bwd_coef", L.ptr(d["dy"]), L.ptr(d["x"]), M, C, L.ptr(d["rm"]), L.ptr(d["rv"]),
               L.ptr(d["gamma"]), L.ptr(d["beta"]), 1, L.ptr(dg), L.ptr(db), 0, L.ptr(bnp), L.ptr(ws), 6 * C - 1, L.stream())
    torch.cuda.synchronize()
    for t in (y, mean, rstd, dx, dg, db, bnp):
        assert bool((t == -7.5).all())
    assert _bits_equal(rm, d["rm"]) and _bits_equal(rv, d["rv"]) and bool(torch.isnan(ws).all())


def test_workspace_for_half_the_blocks(L):
    """M = 16385, C = 16: 65 blocks by nature; 1088 floats (need(32) = 2 C 32 + 4 C) stop the
    15/16 shrink at 30 blocks (need(33) = 1120, need(30) = 1024), rpb 548, one group.  Another
    summation order, so bounds, not bits: chain = ceil(548 16 / 1024) + 64 = 73."""
    M, C, wsf = 16385, 16, 1088
    assert _bn_blocks(M, C, wsf) == (30, 548, 1) and _chain(M, C, wsf) == 73
    _check_fwd_bwd(L, M, C, "relu", seed=4, ws_floats=wsf, stat_bound=_stat_bound(M, C, wsf))


# ------------------------------------------------------------------ 5. stale workspace state
def _fwd_bwd_all(L, d, ws):
    f = _k_fwd(L, d, "relu", ws=ws)
    b = _k_bwd(L, d, d["dy"], f["mean"], f["rstd"], "relu", ws=ws)
    return [f[k] for k in ("y", "mean", "rstd", "rm", "rv")] + [b[k] for k in ("dx", "dgamma", "dbeta")]


@pytest.mark.parametrize("side_stream", [False, True])
def test_stale_workspace_is_never_read(L, side_stream):
    """A 505-block, 8-group call (M = 131073) leaves partials and group sums in ws; the 17-block
    call that follows on the same ws equals, bit for bit, the same call on a NaN workspace."""
    big, small = _data(131073, 16, 11), _data(4099, 16, 12)
    ws = _poisoned()
    torch.cuda.synchronize()
    st = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        _fwd_bwd_all(L, big, ws)
        got = _fwd_bwd_all(L, small, ws)
        ws.fill_(float("nan"))
        exp = _fwd_bwd_all(L, small, ws)
    torch.cuda.synchronize()
    for a, e in zip(got, exp):
        assert not torch.isnan(a).any() and _bits_equal(a, e)


# ------------------------------------------------------------------ 6. arrival-counter pool wrap
def test_arrival_counter_pool_wraps(L):
    """M = 16385, C = 4: 65 blocks, 2 groups -> 3 counters per column pass, 2 passes per call.
    6000 calls draw 36000 counters from the 32768 of the pool's eager half: the pool wraps once,
    and since 32768 = 3 * 10922 + 2 the run starting at counter 32766 does not fit, which takes
    arrive_slots' retry.  Outputs of call 1 and of every 500th call are the same bits."""
    M, C = 16385, 4
    assert _bn_blocks(M, C)[::2] == (65, 2)
    d = _data(M, C, 21)
    ws = _poisoned()
    y, mean, rstd = torch.empty_like(d["x"]), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    args = (L.ptr(d["x"]), M, C, L.ptr(d["gamma"]), L.ptr(d["beta"]), 1, EPS, 0.9, L.ptr(y), L.ptr(mean), L.ptr(rstd),
            None, None, L.ptr(ws), ws.numel(), L.stream())
    snaps = []
    for i in range(1, 6001):
        L.call("vt_batchnorm_fwd", *args)
        if i == 1 or i % 500 == 0:
            snaps.append((y.clone(), mean.clone(), rstd.clone()))
    torch.cuda.synchronize()
    r = NR.bn_fwd(d["x"].cpu(), d["gamma"].cpu(), d["beta"].cpu(), "relu", EPS)
    assert NR.rel(snaps[0][0], r["y"]) <= B_Y and NR.rel(snaps[0][1], r["mean"]) <= B_S
    for s in snaps[1:]:
        assert all(_bits_equal(a, e) for a, e in zip(s, snaps[0]))


# ------------------------------------------------------------------ 7. accumulate_params
@pytest.mark.parametrize("C", [16, 129])
def test_accumulate_params(L, C):
    """dgamma / dbeta pre-filled: prefill + fresh sum as ONE fp32 add, for vt_batchnorm_bwd and
    vt_batchnorm_bwd_coef; dx is the non-accumulating call's (it uses the fresh sums)."""
    M = 4099
    d = _data(M, C, 31)
    f = _k_fwd(L, d, "relu")
    fresh = _k_bwd(L, d, d["dy"], f["mean"], f["rstd"], "relu")
    rn, _ = _gen(32)
    pg, pb = 5 * rn(C), 5 * rn(C)
    acc = _k_bwd(L, d, d["dy"], f["mean"], f["rstd"], "relu", acc=1, dg=pg.clone(), db=pb.clone())
    cf = _k_coef(L, d, d["dy"], f["mean"], f["rstd"], "relu", acc=1, dg=pg.clone(), db=pb.clone())
    torch.cuda.synchronize()
    assert _bits_equal(acc["dx"], fresh["dx"])
    for o in (acc, cf):
        assert _bits_equal(o["dgamma"], pg + fresh["dgamma"]) and _bits_equal(o["dbeta"], pb + fresh["dbeta"])
    assert _bits_equal(cf["bnp"][4 * C:5 * C], fresh["dgamma"]) and _bits_equal(cf["bnp"][5 * C:], fresh["dbeta"])


# ------------------------------------------------------------------ 8. vt_batchnorm_bwd_coef
@pytest.mark.parametrize("M", [4099, 16385])
@pytest.mark.parametrize("C", [3, 87, 128, 129])
def test_bwd_coef(L, M, C):
    """bnp = [mean | rstd | gamma | beta | dgamma_now | dbeta_now]: the inputs bit for bit, the
    sums those of vt_batchnorm_bwd bit for bit (same M, C, ws: 17 / 65 blocks) and within the bound."""
    tag = f"coef M={M} C={C}"
    d = _data(M, C, 41)
    r = _to(d, "cpu")
    _mask_kinks(d, NR.bn_fwd(r["x"], r["gamma"], r["beta"], "relu", EPS)["z"], "relu", tag)
    br = NR.bn_bwd(d["dy"].cpu(), r["x"], r["gamma"], r["beta"], "relu", EPS)
    f = _k_fwd(L, d, "relu")
    b = _k_bwd(L, d, d["dy"], f["mean"], f["rstd"], "relu")
    c = _k_coef(L, d, d["dy"], f["mean"], f["rstd"], "relu")
    torch.cuda.synchronize()
    bnp = c["bnp"].view(6, C)
    for i, t in enumerate((f["mean"], f["rstd"], d["gamma"], d["beta"], b["dgamma"], b["dbeta"])):
        assert _bits_equal(bnp[i], t), i
    assert _bits_equal(c["dgamma"], b["dgamma"]) and _bits_equal(c["dbeta"], b["dbeta"])
    _hold("dgamma", tag, bnp[4], br["dgamma"], B_G)
    _hold("dbeta", tag, bnp[5], br["dbeta"], B_G)


# ------------------------------------------------------------------ 9. element-wise kernels
# (M, C): n = M C <= 3; exactly one workgroup's 4096 elements; 4096 +- 1; several workgroups with
# n % 4 != 0 (and the C > 256 parameter staging loop at 257, 1000, 1024; chan4's modulo branch at C < 4)
ELEM = [(1, 1), (1, 2), (1, 3), (3, 1),
        (4096, 1), (2048, 2), (1024, 4), (16, 256), (4, 1024),
        (4095, 1), (4097, 1), (1365, 3), (819, 5), (585, 7),
        (4099, 2), (2731, 3), (2049, 4), (1639, 5), (1171, 7), (101, 87), (37, 256), (33, 257), (9, 1000), (5, 1024)]


def _elem_params(C, seed):
    rn, ru = _gen(seed)
    return dict(mean=2 * rn(C), rstd=0.5 + ru(C), var=0.25 + ru(C), gamma=1 + 0.1 * rn(C), beta=0.1 * rn(C))


@pytest.mark.parametrize("act", ACTS)
def test_batchnorm_apply(L, act):
    for M, C in ELEM:
        rn, _ = _gen(M + C)
        x, p = 2 * rn(M, C) + 1, _elem_params(C, C)
        y = torch.full((M * C + 8,), -7.5, device="cuda")
        L.call("vt_batchnorm_apply", L.ptr(x), M, C, L.ptr(p["mean"]), L.ptr(p["rstd"]), L.ptr(p["gamma"]),
               L.ptr(p["beta"]), NR.ACT[act], L.ptr(y), L.stream())
        ref, _ = NR.bn_apply(x.cpu(), p["mean"].cpu(), p["rstd"].cpu(), p["gamma"].cpu(), p["beta"].cpu(), act)
        assert bool((y[M * C:] == -7.5).all()), (M, C)
        _hold("apply_y", f"M={M} C={C} {act}", y[:M * C].view(M, C), ref, B_Y)


def test_batchnorm_apply_rejects_more_than_1024_channels(L):
    C = 1025
    x, p = torch.zeros(2, C, device="cuda"), _elem_params(C, 1)
    y = torch.full((2, C), -7.5, device="cuda")
    with pytest.raises(ValueError):
        L.call("vt_batchnorm_apply", L.ptr(x), 2, C, L.ptr(p["mean"]), L.ptr(p["rstd"]), L.ptr(p["gamma"]),
               L.ptr(p["beta"]), 1, L.ptr(y), L.stream())
    assert bool((y == -7.5).all())


@pytest.mark.parametrize("act", ACTS)
def test_batchnorm_eval(L, act):
    for M, C in ELEM + [(3, 1025), (5, 4096)]:     # no channel limit: one thread per element
        rn, _ = _gen(M + C + 1)
        x, p = 2 * rn(M, C) + 1, _elem_params(C, C + 1)
        y = torch.full((M * C + 8,), -7.5, device="cuda")
        L.call("vt_batchnorm_eval", L.ptr(x), M, C, L.ptr(p["mean"]), L.ptr(p["var"]), EPS, L.ptr(p["gamma"]),
               L.ptr(p["beta"]), NR.ACT[act], L.ptr(y), L.stream())
        rstd = 1.0 / torch.sqrt(p["var"].cpu().double() + EPS)
        ref, _ = NR.bn_apply(x.cpu(), p["mean"].cpu(), rstd, p["gamma"].cpu(), p["beta"].cpu(), act)
        assert bool((y[M * C:] == -7.5).all()), (M, C)
        _hold("eval_y", f"M={M} C={C} {act}", y[:M * C].view(M, C), ref, B_Y)


@pytest.mark.parametrize("act", ACTS)
def test_act_fwd_bwd(L, act):
    """One thread per element, 256 per workgroup: n around one and several workgroups."""
    for n in (1, 3, 255, 256, 257, 4095, 4096, 4097, 8787):
        rn, _ = _gen(n)
        x, dy = 1.5 * rn(n), rn(n)
        dy[NR.kink_mask(x.double(), act)] = 0
        y, dx = torch.full((n + 8,), -7.5, device="cuda"), torch.full((n + 8,), -7.5, device="cuda")
        L.call("vt_act_fwd", L.ptr(x), n, NR.ACT[act], L.ptr(y), L.stream())
        L.call("vt_act_bwd", L.ptr(dy), L.ptr(x), n, NR.ACT[act], L.ptr(dx), L.stream())
        xr = x.cpu().double()
        assert bool((y[n:] == -7.5).all()) and bool((dx[n:] == -7.5).all()), n
        _hold("act_y", f"n={n} {act}", y[:n], NR.act_f(xr, act), B_Y)
        _hold("act_dx", f"n={n} {act}", dx[:n], dy.cpu().double() * NR.act_d(xr, act), B_G)


# ------------------------------------------------------------------ 10. synchronised BatchNorm, one process
@pytest.mark.parametrize("split", ["one_row", "third"])
@pytest.mark.parametrize("M", [4099, 16385])
@pytest.mark.parametrize("C", [3, 87, 129])
def test_syncbn_two_parts_equal_full_batch(L, C, M, split):
    """The rows in two unequal parts (each its own allocation, as two ranks hold them), the
    [2C + 1] double sums added with torch in place of the all-reduce: statistics, running
    statistics (unbiased with the total count), y, dx and the per-part dgamma / dbeta
    (which = 2 on the local sums) against the full-batch fp64 reference."""
    tag = f"syncbn M={M} C={C} {split}"
    d = _data(M, C, 51)
    r = _to(d, "cpu")
    fr = NR.bn_fwd(r["x"], r["gamma"], r["beta"], "relu", EPS, r["rm"], r["rv"], 0.9)
    _mask_kinks(d, fr["z"], "relu", tag)
    br = NR.bn_bwd(d["dy"].cpu(), r["x"], r["gamma"], r["beta"], "relu", EPS)
    m0 = 1 if split == "one_row" else M // 3
    parts = [(d["x"][:m0].clone(), d["dy"][:m0].clone()), (d["x"][m0:].clone(), d["dy"][m0:].clone())]
    g, b, act = d["gamma"], d["beta"], 1
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = d["rm"].clone(), d["rv"].clone()
    ws = _poisoned()

    def sums(which):
        out = []
        for x, dy in parts:
            s = torch.full((2 * C + 1,), float("nan"), dtype=torch.float64, device="cuda")
            ws.fill_(float("nan"))
            L.call("vt_syncbn_sums", L.ptr(x), L.ptr(dy) if which == 2 else None, x.shape[0], C, which, L.ptr(mean),
                   L.ptr(rstd) if which == 2 else None, L.ptr(g) if which == 2 else None,
                   L.ptr(b) if which == 2 else None, act if which == 2 else 0, L.ptr(s), L.ptr(ws), ws.numel(), L.stream())
            out.append(s)
        return out

    s0 = sums(0)
    tot = s0[0] + s0[1]
    L.call("vt_syncbn_stats", L.ptr(tot), C, 0, EPS, 0.9, L.ptr(mean), None, None, None, None, None, 0, L.stream())
    s1 = sums(1)
    tot = s1[0] + s1[1]
    assert tot[2 * C].item() == M
    L.call("vt_syncbn_stats", L.ptr(tot), C, 1, EPS, 0.9, L.ptr(mean), L.ptr(rstd), L.ptr(rm), L.ptr(rv), None, None, 0,
           L.stream())
    ys = []
    for x, _ in parts:
        y = torch.empty_like(x)
        L.call("vt_batchnorm_apply", L.ptr(x), x.shape[0], C, L.ptr(mean), L.ptr(rstd), L.ptr(g), L.ptr(b), act,
               L.ptr(y), L.stream())
        ys.append(y)
    s2 = sums(2)
    pgrads = []
    for s in s2:
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        L.call("vt_syncbn_stats", L.ptr(s), C, 2, 0.0, 0.0, None, None, None, None, L.ptr(dg), L.ptr(db), 0, L.stream())
        pgrads.append((dg, db))
    tot = s2[0] + s2[1]
    dxs = []
    for x, dy in parts:
        dx, w2 = torch.empty_like(x), torch.full((2 * C,), float("nan"), device="cuda")
        L.call("vt_syncbn_bwd_dx", L.ptr(dy), L.ptr(x), x.shape[0], C, L.ptr(mean), L.ptr(rstd), L.ptr(g), L.ptr(b), act,
               L.ptr(tot), L.ptr(dx), L.ptr(w2), L.stream())
        dxs.append(dx)
    torch.cuda.synchronize()
    _hold("mean", tag, mean, fr["mean"], B_S)
    _hold("rstd", tag, rstd, fr["rstd"], B_S)
    _hold("run_mean", tag, rm, fr["run_mean"], B_S)
    _hold("run_var", tag, rv, fr["run_var"], B_S)
    _hold("y", tag, torch.cat(ys), fr["y"], B_Y)
    _hold("dx", tag, torch.cat(dxs), br["dx"], B_G)
    xhat = (r["x"].double() - fr["mean"]) * fr["rstd"]
    dz = d["dy"].cpu().double() * NR.act_d(fr["z"], "relu")
    for (lo, hi), (dg, db) in zip(((0, m0), (m0, M)), pgrads):
        _hold("dgamma", f"{tag} rows {lo}:{hi}", dg, (dz * xhat)[lo:hi].sum(0), B_G)
        _hold("dbeta", f"{tag} rows {lo}:{hi}", db, dz[lo:hi].sum(0), B_G)


# ------------------------------------------------------------------ 11. the dropout variants
@pytest.mark.parametrize("Lrows", [64, 0])
def test_dropout_variants_against_reference(L, Lrows):
    """vt_batchnorm_fwd_dropout / _bwd_dropout at M = 16448 (257 samples of 64 rows: 65 blocks,
    2 groups), C = 12, p = 0.3, against mask scale BN_ref(x) and the reference backward of the
    masked dy; the mask is vt_dropout_apply's on a tensor of ones (Lrows = 0: element-wise)."""
    M, C, p, seed = 257 * 64, 12, 0.3, 99
    assert _bn_blocks(M, C)[::2] == (65, 2)
    tag = f"dropout M={M} C={C} L={Lrows}"
    d = _data(M, C, 61)
    r = _to(d, "cpu")
    fr = NR.bn_fwd(r["x"], r["gamma"], r["beta"], "relu", EPS, r["rm"], r["rv"], 0.9)
    _mask_kinks(d, fr["z"], "relu", tag)
    ones, keep = torch.ones(M, C, device="cuda"), torch.empty(M, C, device="cuda")
    L.call("vt_dropout_apply", L.ptr(ones), M * C, C, Lrows, p, seed, None, L.ptr(keep), L.stream())
    scale = 1.0 / (1.0 - p)
    keep = (keep.cpu().double() / keep.max().item())
    assert set(keep.unique().tolist()) == {0.0, 1.0} and abs(keep.mean().item() - 0.7) < 0.1
    br = NR.bn_bwd(d["dy"].cpu().double() * keep * scale, r["x"], r["gamma"], r["beta"], "relu", EPS)
    ws = _poisoned()
    y, dx = torch.empty_like(d["x"]), torch.empty_like(d["x"])
    mean, rstd, dg, db = (torch.empty(C, device="cuda") for _ in range(4))
    rm, rv = d["rm"].clone(), d["rv"].clone()
    L.call("vt_batchnorm_fwd_dropout", L.ptr(d["x"]), M, C, L.ptr(d["gamma"]), L.ptr(d["beta"]), 1, EPS, 0.9, L.ptr(y),
           L.ptr(mean), L.ptr(rstd), L.ptr(rm), L.ptr(rv), Lrows, p, seed, None, L.ptr(ws), ws.numel(), L.stream())
    ws.fill_(float("nan"))
    L.call("vt_batchnorm_bwd_dropout", L.ptr(d["dy"]), L.ptr(d["x"]), M, C, L.ptr(mean), L.ptr(rstd), L.ptr(d["gamma"]),
           L.ptr(d["beta"]), 1, Lrows, p, seed, None, L.ptr(dx), L.ptr(dg), L.ptr(db), 0, L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    _hold("mean", tag, mean, fr["mean"], B_S)
    _hold("rstd", tag, rstd, fr["rstd"], B_S)
    _hold("run_mean", tag, rm, fr["run_mean"], B_S)
    _hold("run_var", tag, rv, fr["run_var"], B_S)
    _hold("y", tag, y, keep * scale * fr["y"], B_Y)
    _hold("dx", tag, dx, br["dx"], B_G)
    _hold("dgamma", tag, dg, br["dgamma"], B_G)
    _hold("dbeta", tag, db, br["dbeta"], B_G)


# ------------------------------------------------------------------ pointer alignment
def test_misaligned_activation_pointers_are_rejected(L):
    """x, y, dy, dx one float off 16-byte alignment: ValueError before any launch (the float4
    kernels are never started on such a pointer), nothing written."""
    M, C = 64, 8
    n = M * C
    base = {k: torch.full((n + 4,), -7.5, device="cuda") for k in ("x", "dy", "y", "dx")}
    v = torch.zeros(C, device="cuda")
    o = torch.ones(C, device="cuda")
    ws = _poisoned(4096)
    sums = torch.zeros(2 * C + 1, dtype=torch.float64, device="cuda")
    bnp = torch.zeros(6 * C, device="cuda")
    pv, po, pw = L.ptr(v), L.ptr(o), L.ptr(ws)

    def calls(P):
        st = L.stream()
        return {
            "vt_batchnorm_fwd": ("xy", (P["x"], M, C, po, pv, 1, EPS, 0.9, P["y"], pv, po, None, None, pw, 4096, st)),
            "vt_batchnorm_fwd_dropout": ("xy", (P["x"], M, C, po, pv, 1, EPS, 0.9, P["y"], pv, po, None, None, 8, 0.3, 1,
                                                None, pw, 4096, st)),
            "vt_batchnorm_bwd": ("dxy", (P["dy"], P["x"], M, C, pv, po, po, pv, 1, P["dx"], pv, pv, 0, pw, 4096, st)),
            "vt_batchnorm_bwd_dropout": ("dxy", (P["dy"], P["x"], M, C, pv, po, po, pv, 1, 8, 0.3, 1, None, P["dx"], pv, pv,
                                                 0, pw, 4096, st)),
            "vt_batchnorm_bwd_coef": ("dx", (P["dy"], P["x"], M, C, pv, po, po, pv, 1, pv, pv, 0, L.ptr(bnp), pw, 4096, st)),
            "vt_batchnorm_apply": ("xy", (P["x"], M, C, pv, po, po, pv, 1, P["y"], st)),
            "vt_syncbn_sums": ("dx", (P["x"], P["dy"], M, C, 2, pv, po, po, pv, 1, L.ptr(sums), pw, 4096, st)),
            "vt_syncbn_bwd_dx": ("dxy", (P["dy"], P["x"], M, C, pv, po, po, pv, 1, L.ptr(sums), P["dx"], pw, st)),
        }

    names = {"xy": ("x", "y"), "dx": ("dy", "x"), "dxy": ("dy", "x", "dx")}
    aligned = {k: t.data_ptr() for k, t in base.items()}
    assert all(a % 16 == 0 for a in aligned.values())
    for fn, (kind, _) in calls(aligned).items():
        for off in names[kind]:
            P = dict(aligned)
            P[off] += 4                     # a view one float into the buffer
            with pytest.raises(ValueError, match="16-byte aligned"):
                L.call(fn, *calls(P)[fn][1])
    torch.cuda.synchronize()
    assert all(bool((t == -7.5).all()) for t in base.values()) and bool(torch.isnan(ws).all())
