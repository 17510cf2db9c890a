"""Is a transfer-entropy value different from what an unrelated uterine-pressure channel would give?
A surrogate test: the estimator of vaeteb.te is run again on up channels whose timing relation to the
heart rate is destroyed while their own statistics are kept, and the observed value is ranked among
those results.  The KL between a learned posterior and prior is positive for any input, so the rank,
not the value, is what a reader can hold a number against.  The reference has no such test: its shift
analysis sweeps 0 .. -60 s and takes an argmin (ref/model/graph_model.py:1414).

A SurrogatePlan gives every (recording b, variant k) row, k = 0 .. K, a source recording, a circular
shift and a permutation of blocks of block_len samples; the row's up channel is

    u[i] = x[src[b,k], 1, m((i - shift[b,k]) mod N)]
    m(j) = perm[b,k, j // block_len] * block_len + j % block_len   for j < (N // block_len) * block_len
    m(j) = j                                                        otherwise (the tail stays in place)

and variant 0 is always the identity, the observed channel.  surrogate_plan draws the three usual kinds:

    "shift"   the recording's own channel rolled by min_shift .. N - min_shift samples: the guard band
              (default 240 samples, 60 s at 4 Hz, the range vaeteb.te.left_shifts() searches for the
              real coupling) keeps the null away from the lags under test
    "block"   its own channel with its block_len-sample blocks (default one minute) in a random order
              that is not the identity, then rolled by any amount: a large roll of a quasi-periodic
              contraction pattern can land back in phase, shuffled blocks cannot
    "swap"    the channel of another recording of the batch, rolled by any amount

The pass is ShiftSweep's (vaeteb/te.py), the heart-rate side once per recording and everything that
depends on the up channel once per row, with two other kernels at its ends:

    frontend(x)                fhr_st, fhr_ph and the fhr analytic signals        B rows, once
    vt_fe_spectrum_surrogate   padded spectra of the surrogate up channels        B*(K+1) rows
    ShiftSweep._posterior_rows wavelets, cross pairs, normalise, both encoders    B*(K+1) rows
    vt_te_kl_steps             ts[b, k, s] mean KL of step s, te[b, k] of the row B*(K+1) rows
    vt_tenull_stats            the ranks below, exact integers                    B workgroups, once

    count_ge[b]         #{k >= 1 : te[b,k] >= te[b,0]}          p      = (1 + count_ge) / (K + 1)
    step_count_ge[b,s]  #{k >= 1 : ts[b,k,s] >= ts[b,0,s]}      p_steps, the same per step
    max_count_ge[b,s]   #{k >= 1 : max_s' ts[b,k,s'] >= ts[b,0,s]}   p_steps_fwer: against the maximum over
                        the window's steps, so that the chance of any false step in a window is controlled
    group_sums[k]       sum_b te[b,k]      group_p = (1 + #{k >= 1 : G_k >= G_0}) / (K + 1): surrogate k
                        is an independent draw per recording, so the sums are exchangeable under the null

The smallest attainable p is 1 / (K + 1).  Comparisons are float32 >=; a NaN never counts.  The KL draws
no noise and this analysis has no reference loop whose random stream it would mirror, so the device
generator is left untouched.  No host synchronisation: the plan is uploaded once per call and the
p-values are formed on the device from the integers.

Not here: phase-randomised (Fourier) surrogates (the window length is not a power of two and the padded
spectrum is not the window's), cluster-based corrections, plots, and per-step p-values stitched across
overlapping windows (vaeteb.timeline.stitch takes te_steps as it is; a stitched p needs its own null).
"""
import numpy as np
import torch

from . import _lib
from . import model as _model
from .frontend import _i32
from .te import ShiftSweep

KINDS = ("shift", "block", "swap")
MAX_VARIANTS = 4096                                  # K + 1: vt_tenull_stats keeps a recording's rows in LDS


class SurrogatePlan:
    """src, shift int32 (B, K+1); perm int32 (B, K+1, N // block_len) or None; block_len.  A hand-made
    plan is checked by validate(B, N) exactly as a generated one before it is used."""

    __slots__ = ("src", "shift", "perm", "block_len")

    def __init__(self, src, shift, perm=None, block_len=240):
        self.src = np.ascontiguousarray(src, dtype=np.int32)
        sh = np.asarray(shift)
        if sh.size and (sh.min() < -2 ** 31 or sh.max() >= 2 ** 31):
            raise ValueError("shifts must fit 32-bit integers")
        self.shift = np.ascontiguousarray(sh, dtype=np.int32)
        self.perm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        self.block_len = block_len

    @property
    def K(self):
        return self.src.shape[1] - 1

    def validate(self, B, N):
        """ValueError unless this is a plan for B recordings of N samples.  Returns self."""
        B, N = int(B), int(N)
        bl = self.block_len
        if isinstance(bl, bool) or not isinstance(bl, (int, np.integer)) or bl < 1 or bl > N:
            raise ValueError(f"block_len must be an integer in [1, {N}], got {bl!r}")
        if self.src.ndim != 2 or self.src.shape[0] != B or self.shift.shape != self.src.shape:
            raise ValueError(f"src and shift must both be ({B}, K + 1), got {self.src.shape} and {self.shift.shape}")
        K1 = self.src.shape[1]
        if K1 < 2:
            raise ValueError("a plan needs at least one surrogate (K >= 1)")
        if K1 > MAX_VARIANTS:
            raise ValueError(f"K + 1 = {K1} variants exceed {MAX_VARIANTS}")
        if self.src.min() < 0 or self.src.max() >= B:
            raise ValueError(f"src must lie in [0, {B})")
        nblk = N // int(bl)
        if self.perm is not None:
            if self.perm.shape != (B, K1, nblk):
                raise ValueError(f"perm must be ({B}, {K1}, {nblk}) for block_len {bl}, got {self.perm.shape}")
            if not np.array_equal(np.sort(self.perm, axis=-1),
                                  np.broadcast_to(np.arange(nblk, dtype=np.int32), self.perm.shape)):
                raise ValueError("every perm row must be a permutation of the blocks")
        ident = np.array_equal(self.src[:, 0], np.arange(B)) and not self.shift[:, 0].any() and (
            self.perm is None or np.array_equal(self.perm[:, 0], np.broadcast_to(np.arange(nblk), (B, nblk))))
        if not ident:
            raise ValueError("column 0 of a plan is the observed row: src = b, shift = 0, identity permutation")
        return self


def surrogate_plan(kind, B, K, N, seed, *, min_shift=240, block_len=240):
    """The SurrogatePlan of K surrogates per recording of the given kind (module docstring) for B
    recordings of N samples, drawn from numpy.random.default_rng(seed): equal arguments, equal plan."""
    for name, v in (("B", B), ("K", K), ("N", N), ("min_shift", min_shift), ("block_len", block_len)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    B, K, N, min_shift, block_len = int(B), int(K), int(N), int(min_shift), int(block_len)
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if B < 1 or N < 2:
        raise ValueError(f"B >= 1 and N >= 2 are required, got B = {B}, N = {N}")
    if K < 1:
        raise ValueError(f"at least one surrogate is required, got K = {K}")
    if K + 1 > MAX_VARIANTS:
        raise ValueError(f"K + 1 = {K + 1} variants exceed {MAX_VARIANTS}")
    if min_shift < 0 or 2 * min_shift > N:
        raise ValueError(f"min_shift = {min_shift} leaves no shift in [min_shift, N - min_shift] at N = {N}")
    if block_len < 1 or block_len > N:
        raise ValueError(f"block_len must lie in [1, {N}], got {block_len}")
    nblk = N // block_len
    if kind == "block" and nblk < 2:
        raise ValueError(f"block surrogates need at least two blocks, N // block_len = {nblk}")
    if kind == "swap" and B < 2:
        raise ValueError("swap surrogates need at least two recordings")
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(B, dtype=np.int32)[:, None], K + 1, axis=1)
    shift = np.zeros((B, K + 1), np.int32)
    perm = None
    if kind == "shift":
        shift[:, 1:] = rng.integers(min_shift, N - min_shift + 1, size=(B, K))
    elif kind == "block":
        perm = np.broadcast_to(np.arange(nblk, dtype=np.int32), (B, K + 1, nblk)).copy()
        for b in range(B):
            for k in range(1, K + 1):
                p = rng.permutation(nblk)
                while np.array_equal(p, np.arange(nblk)):
                    p = rng.permutation(nblk)
                perm[b, k] = p
        shift[:, 1:] = rng.integers(0, N, size=(B, K))
    else:
        other = rng.integers(0, B - 1, size=(B, K))
        src[:, 1:] = other + (other >= np.arange(B)[:, None])
        shift[:, 1:] = rng.integers(0, N, size=(B, K))
    return SurrogatePlan(src, shift, perm, block_len).validate(B, N)


class TeSignificanceResult:
    """te (B,) and te_surr (B, K) float32; te_steps (B, S_out) and te_steps_surr (B, K, S_out) float32
    (the observed row and its surrogates per step) and step_surr_mean (B, S_out) float32; count_ge (B,), step_count_ge, max_count_ge (B, S_out) int32;
    surr_mean, surr_sd (B,) and group_sums (K + 1,) float64; the p-values, z and te_effective are
    formed from these where the tensors live (no synchronisation)."""

    __slots__ = ("te", "te_surr", "te_steps", "te_steps_surr", "step_surr_mean", "count_ge", "step_count_ge", "max_count_ge",
                 "surr_mean", "surr_sd", "group_sums")

    def __init__(self, te, te_surr, te_steps, te_steps_surr, step_surr_mean, count_ge, step_count_ge, max_count_ge,
                 surr_mean, surr_sd, group_sums):
        self.te, self.te_surr, self.te_steps, self.te_steps_surr = te, te_surr, te_steps, te_steps_surr
        self.step_surr_mean = step_surr_mean
        self.count_ge, self.step_count_ge, self.max_count_ge = count_ge, step_count_ge, max_count_ge
        self.surr_mean, self.surr_sd, self.group_sums = surr_mean, surr_sd, group_sums

    @property
    def K(self):
        return self.te_surr.shape[1]

    def _p(self, count):
        # a tensor divisor: the correctly rounded quotient (a Python scalar may be applied as a reciprocal)
        return (count.double() + 1.0) / torch.full((), self.K + 1, dtype=torch.float64, device=count.device)

    @property
    def p(self):
        """(B,) float64: (1 + count_ge) / (K + 1), at least 1 / (K + 1)."""
        return self._p(self.count_ge)

    @property
    def p_steps(self):
        """(B, S_out) float64: every step ranked among the same step of its surrogates."""
        return self._p(self.step_count_ge)

    @property
    def p_steps_fwer(self):
        """(B, S_out) float64: every step ranked among the surrogates' maxima over the window's steps;
        controls the family-wise error rate within a window."""
        return self._p(self.max_count_ge)

    @property
    def te_effective(self):
        """(B,) float64: the observed value less the surrogates' mean."""
        return self.te.double() - self.surr_mean

    @property
    def z(self):
        """(B,) float64: te_effective in units of the surrogates' sd (NaN for K = 1)."""
        return self.te_effective / self.surr_sd

    def group_p(self):
        """float64 scalar tensor: (1 + #{k >= 1 : G_k >= G_0}) / (K + 1) over the pooled recordings."""
        g = self.group_sums
        return self._p((g[1:] >= g[0]).sum())

    def merge(self, other):
        """The result over both sets of recordings (the same K): per-recording fields concatenated,
        group_sums added."""
        if other.K != self.K:
            raise ValueError(f"results with K = {self.K} and K = {other.K} do not merge")
        cat = {f: torch.cat([getattr(self, f), getattr(other, f)]) for f in self.__slots__ if f != "group_sums"}
        return TeSignificanceResult(group_sums=self.group_sums + other.group_sums, **cat)


class TeSignificance:
    """sig = TeSignificance(model, frontend); r = sig(x, kind="block", n_surrogates=199, seed=0) or
    sig(x, plan=a SurrogatePlan), x (B, 2, N) float32 on the device.  Returns a TeSignificanceResult.

    rows_per_launch bounds the (recording, variant) rows of one pass through the kernels and is cut as
    ShiftSweep cuts it (whole recordings, or inside one recording when K + 1 is larger); every row's
    result depends on that row and its recording only, so the chunking does not change a bit.  The
    model is left in eval mode; the device generator is not touched."""

    def __init__(self, model, frontend, rows_per_launch=256):
        self.sweep = ShiftSweep(model, frontend, rows_per_launch)
        self.model, self.frontend, self.rows_per_launch = model, frontend, int(rows_per_launch)

    @torch.no_grad()
    def __call__(self, x, kind="block", n_surrogates=199, seed=0, plan=None, min_shift=240, block_len=240):
        sw, fe, m = self.sweep, self.frontend, self.model
        p = fe.plan
        if x.dim() != 3 or x.shape[1] != 2 or x.shape[2] != p.N or x.dtype != torch.float32:
            raise ValueError(f"expected float32 (B, 2, {p.N}) windows, got {x.dtype} {tuple(x.shape)}")
        B, N = x.shape[0], p.N
        if plan is None:
            plan = surrogate_plan(kind, B, n_surrogates, N, seed, min_shift=min_shift, block_len=block_len)
        else:
            plan.validate(B, N)
        x = x.contiguous()
        K1, S = plan.K + 1, fe.S_out
        dev = p.device
        src, shift = _i32(plan.src, dev), _i32(plan.shift, dev)
        perm = None if plan.perm is None else _i32(plan.perm, dev)
        feats = fe(x)                                   # fhr side, once; leaves the fhr analytic signals
        an_fhr = fe._bufs["analytic"]                   # (B, n_slots, N, 2)
        m.eval()
        if getattr(m, "h16_format", None):
            _lib.set_h16(m.h16_format == "fp16")
        st = _lib.stream()
        prev = dict(_model._PAR)
        _model._PAR["on"], _model._PAR["next"] = bool(m.concurrent_encoders), 1
        try:
            mu_y, lv_full = m.target_encoder(feats["fhr_st"], feats["fhr_ph"])
            lv_p, c_lv = torch.split(lv_full, m.latent_dim_target, dim=-1)
            mu_y, lv_p = mu_y.contiguous(), lv_p.contiguous()
            L = mu_y.shape[-1]
            te = torch.empty((B, K1), device=dev)
            ts = torch.empty((B, K1, S), device=dev)
            for (b0, nb, k0, nk) in sw._chunks(B, K1):
                R, r0 = nb * nk, b0 * K1 + k0
                xhat = sw._buf("xhat", (R, p.n_pad, 2))
                _lib.call("vt_fe_spectrum_surrogate", x.data_ptr() + 4 * N, B, 2 * N, N, p.n_pad, p.pad_left, 0,
                          _lib.ptr(src), _lib.ptr(shift), _lib.ptr(perm), int(plan.block_len), r0, R,
                          _lib.ptr(p.t_tw), _lib.ptr(xhat), st)
                mu_c, lv_q = sw._posterior_rows(xhat, an_fhr, c_lv, b0, nb, nk)
                _lib.call("vt_te_kl_steps", _lib.ptr(mu_c), _lib.ptr(lv_q), mu_y.data_ptr() + 4 * b0 * S * L,
                          lv_p.data_ptr() + 4 * b0 * S * L, nb, nk, S, L, ts.data_ptr() + 4 * r0 * S,
                          te.data_ptr() + 4 * r0, st)
        finally:
            _model._PAR.update(prev)
        return rank_statistics(ts, te)


def rank_statistics(ts, te):
    """The TeSignificanceResult of ts (B, K + 1, S) and te (B, K + 1), float32 on the device, variant 0
    the observed row: one vt_tenull_stats call."""
    if ts.dim() != 3 or te.shape != ts.shape[:2] or ts.dtype != torch.float32 or te.dtype != torch.float32:
        raise ValueError(f"expected float32 ts (B, K + 1, S) and te (B, K + 1), got {tuple(ts.shape)}, {tuple(te.shape)}")
    B, K1, S = ts.shape
    if B < 1 or S < 1 or K1 < 2 or K1 > MAX_VARIANTS:
        raise ValueError(f"B >= 1, S >= 1 and 2 <= K + 1 <= {MAX_VARIANTS} are required, got {tuple(ts.shape)}")
    ts, te = ts.contiguous(), te.contiguous()
    dev = ts.device
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    count, step_count, max_count = i32(B), i32(B, S), i32(B, S)
    mean, sd, group = f64(B), f64(B), f64(K1)
    step_mean = torch.empty((B, S), device=dev)
    _lib.call("vt_tenull_stats", _lib.ptr(ts), _lib.ptr(te), B, K1, S, _lib.ptr(count), _lib.ptr(step_count),
              _lib.ptr(max_count), _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(step_mean), _lib.ptr(group), _lib.stream())
    return TeSignificanceResult(te[:, 0], te[:, 1:], ts[:, 0], ts[:, 1:], step_mean, count, step_count, max_count,
                                mean, sd, group)
