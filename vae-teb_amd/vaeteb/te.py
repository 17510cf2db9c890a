"""Transfer entropy against a circular shift of the source channel, batched over
(recording, shift) — the reference's run_transfer_entropy_shift_analysis
(ref/model/graph_model.py:1210-1458) without its per-shift, batch-1 loop.

For every recording the reference rolls the up channel by each shift (:1443-1458), re-runs the
cross-phase front-end (:1328-1336), normalises (:1340-1350) and calls
measure_transfer_entropy(reduce_mean=False).mean() (:1368-1371).  Only the up spectrum, the up
analytic signals, the cross pairs, the source encoder and the conditional encoder depend on the
shift; `ShiftSweep` runs the fhr side once per recording and everything else once per
(recording, shift) row, rows batched:

    frontend(x)              fhr_st, fhr_ph and the fhr analytic signals     B rows, once
    vt_fe_spectrum_rolled    padded spectra of the rolled up channel         B*K rows
    vt_fe_wavelet (C = 1)    up analytic signals the cross pairs use         B*K rows
    vt_fe_pairs_split        cross pairs, fhr operand per recording          B*K rows
    vt_fe_normalize_window   asinh + z-score + trim -> x_ph                  B*K rows
    target encoder           prior (mu_y, logvar_y), c_logvar                B rows, once
    source + conditional     posterior pieces                                B*K rows
    vt_te_kl_rows            te[b, k] = mean KL, optional elementwise KL     B*K rows

Not ported: the reference's plots and its HDF5 dataset iteration (callers bring the windows).
"""
import numpy as np
import torch

from . import _lib
from . import model as _model
from .frontend import _i32, launch_wavelet


def left_shifts(max_left_shift_seconds=60, step_seconds=1, sampling_rate=4.0):
    """The reference's shift_samples (ref/model/graph_model.py:1283-1287): left shifts only,
    -max_left_shift_seconds .. 0 s in step_seconds steps, in samples."""
    shift_seconds = np.arange(-int(max_left_shift_seconds), 0 + 1, int(step_seconds))
    return (shift_seconds * sampling_rate).astype(int)


class ShiftSweepResult:
    """te (B, K) float32 on the device; shifts (the K integers, numpy); argmin (B,) index of each
    recording's minimum (first minimum on ties, as np.argmin at ref/model/graph_model.py:1414);
    x_ph (B, K, S_out, C_x) and kl (B, K, S_out, L) when requested, else None."""

    __slots__ = ("te", "shifts", "argmin", "x_ph", "kl")

    def __init__(self, te, shifts, argmin, x_ph=None, kl=None):
        self.te, self.shifts, self.argmin, self.x_ph, self.kl = te, shifts, argmin, x_ph, kl


class ShiftSweep:
    """sweep = ShiftSweep(model, frontend); r = sweep(x, shifts) with x (B, 2, N) on the device.

    rows_per_launch bounds the (recording, shift) rows of one pass through the kernels (the work
    buffers are sized by it); chunks are cut at whole recordings when a recording's K shifts fit,
    inside one recording otherwise.  Every row's result depends on that row and its recording only,
    so the chunking does not change a bit.  No host synchronisation; the model is left in eval mode
    (as measure_transfer_entropy leaves it) and one noise draw per row is consumed from the device
    generator, as the reference's loop of forwards consumes it."""

    def __init__(self, model, frontend, rows_per_launch=256):
        if rows_per_launch < 1:
            raise ValueError(f"rows_per_launch must be positive, got {rows_per_launch}")
        if not frontend.C_x:
            raise ValueError("the front-end selects no cross pairs")
        self.model, self.frontend, self.rows_per_launch = model, frontend, int(rows_per_launch)
        p, fe = frontend.plan, frontend
        # the (1, f) filters of the cross pairs as a one-channel wavelet table: channel 0 of the
        # rolled spectra, slots in ascending filter order (FrontEndPlan.tables' order), no S1
        fj = sorted({int(p.j_idx[k]) for k in fe.cross_pairs})
        slot = {f: s for s, f in enumerate(fj)}
        dev = p.device
        self.up_tab = dict(n_slots=len(fj), n_items=len(fj),
                           items=_i32(np.array([(0, f, slot[f], -1, 0) for f in fj]).reshape(-1, 5), dev))
        self.slot_j = _i32([slot[int(p.j_idx[k])] for k in fe.cross_pairs], dev)
        self.slot_i = fe.tab["slot_i"][fe.C_ph:]
        self.power = fe.tab["power"][fe.C_ph:]
        self._bufs = {}
        self._shifts = {}

    def _buf(self, name, shape):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape):
            b = self._bufs[name] = torch.empty(shape, dtype=torch.float32, device=self.frontend.plan.device)
        return b

    def _shifts_dev(self, shifts):
        key = tuple(int(s) for s in shifts)
        if not key:
            raise ValueError("no shifts")
        if any(not -2 ** 31 <= s < 2 ** 31 for s in key):
            raise ValueError("shifts must fit 32-bit integers")
        t = self._shifts.get(key)
        if t is None:
            if len(self._shifts) >= 16:
                self._shifts.clear()
            t = self._shifts[key] = (_i32(key, self.frontend.plan.device), np.array(key, dtype=np.int64))
        return t

    def _chunks(self, B, K):
        """(b0, nb, k0, nk): nb whole recordings from b0 (k0 = 0, nk = K), or shifts
        [k0, k0 + nk) of the one recording b0."""
        R = self.rows_per_launch
        if K <= R:
            per = R // K
            return [(b0, min(per, B - b0), 0, K) for b0 in range(0, B, per)]
        return [(b, 1, k0, min(R, K - k0)) for b in range(B) for k0 in range(0, K, R)]

    def _posterior_rows(self, xhat, an_fhr, c_lv, b0, nb, nk, x_ph=None):
        """The posterior pieces (mu_c, lv_q), each (nb * nk, S, L), of the rows whose padded up spectra
        are xhat (nb * nk, n_pad, 2): row i belongs to recording b0 + i // nk, whose fhr analytic
        signals (an_fhr, all recordings) and c_logvar (c_lv, all recordings) it reads.  The up analytic
        signals, the cross pairs, the normalised window (into x_ph when given, else a work buffer),
        the source encoder and the conditional encoder; called inside the model's _PAR setting."""
        fe, m = self.frontend, self.model
        p = fe.plan
        N, S, C_x, R = p.N, fe.S_out, fe.C_x, nb * nk
        n_slots_i = fe.tab["n_slots"]
        k_, mean_, std_ = fe.stats["fhr_up_ph"]
        st = _lib.stream()
        an_up = self._buf("analytic_up", (R, self.up_tab["n_slots"], N, 2))
        launch_wavelet(p, xhat, R, 1, self.up_tab, an_up, None, 0)
        pairs = self._buf("pairs", (R, C_x, p.pair_len))
        _lib.call("vt_fe_pairs_split", an_fhr.data_ptr() + 8 * b0 * n_slots_i * N, n_slots_i,
                  _lib.ptr(an_up), self.up_tab["n_slots"], nb, nk, N, p.n_pad, p.pad_left, C_x,
                  _lib.ptr(self.slot_i), _lib.ptr(self.slot_j), _lib.ptr(self.power), _lib.ptr(p.t_tw),
                  _lib.ptr(p.t_phi_crop), p.dec, p.pair_start, p.pair_len, 0, _lib.ptr(pairs), st)
        if x_ph is None:
            x_ph = self._buf("x_ph", (R, S, C_x))
        _lib.call("vt_fe_normalize_window", _lib.ptr(pairs), R, C_x, C_x, p.S, fe.trim, S, _lib.ptr(k_),
                  _lib.ptr(mean_), _lib.ptr(std_), 1e-6, _lib.ptr(x_ph), C_x, 0, st)
        mu_x = m.source_encoder(x_ph)
        c_rep = c_lv[b0:b0 + nb].unsqueeze(1).expand(nb, nk, S, c_lv.shape[-1]).reshape(R, S, -1)
        return m.conditional_encoder(mu_x, c_rep)

    @torch.no_grad()
    def __call__(self, x, shifts, elementwise=False, return_features=False):
        fe, m = self.frontend, self.model
        p = fe.plan
        if x.dim() != 3 or x.shape[1] != 2 or x.shape[2] != p.N or x.dtype != torch.float32:
            raise ValueError(f"expected float32 (B, 2, {p.N}) windows, got {x.dtype} {tuple(x.shape)}")
        sh_dev, sh_host = self._shifts_dev(shifts)
        x = x.contiguous()
        B, K, N = x.shape[0], len(sh_host), p.N
        S, C_x = fe.S_out, fe.C_x
        feats = fe(x)                                   # fhr side, once; leaves the fhr analytic signals
        an_fhr = fe._bufs["analytic"]                   # (B, n_slots, N, 2)
        m.eval()
        if getattr(m, "h16_format", None):
            _lib.set_h16(m.h16_format == "fp16")
        x_ph_all = torch.empty((B, K, S, C_x), device=p.device) if return_features else None
        st = _lib.stream()
        prev = dict(_model._PAR)
        _model._PAR["on"], _model._PAR["next"] = bool(m.concurrent_encoders), 1
        try:
            mu_y, lv_full = m.target_encoder(feats["fhr_st"], feats["fhr_ph"])
            lv_p, c_lv = torch.split(lv_full, m.latent_dim_target, dim=-1)
            mu_y, lv_p = mu_y.contiguous(), lv_p.contiguous()
            L = mu_y.shape[-1]
            te = torch.empty((B, K), device=p.device)
            kl = torch.empty((B, K, S, L), device=p.device) if elementwise else None
            for (b0, nb, k0, nk) in self._chunks(B, K):
                R, r0 = nb * nk, b0 * K + k0
                xhat = self._buf("xhat", (R, p.n_pad, 2))
                _lib.call("vt_fe_spectrum_rolled", x.data_ptr() + 4 * ((b0 * 2 + 1) * N), nb, 2 * N, N, p.n_pad,
                          p.pad_left, 0, sh_dev.data_ptr() + 4 * k0, nk, _lib.ptr(p.t_tw), _lib.ptr(xhat), st)
                x_ph = (x_ph_all.view(B * K, S, C_x)[r0:r0 + R] if return_features else None)
                mu_c, lv_q = self._posterior_rows(xhat, an_fhr, c_lv, b0, nb, nk, x_ph)
                _lib.call("vt_te_kl_rows", _lib.ptr(mu_c), _lib.ptr(lv_q), mu_y.data_ptr() + 4 * b0 * S * L,
                          lv_p.data_ptr() + 4 * b0 * S * L, nb, nk, S * L, te.data_ptr() + 4 * r0,
                          kl.data_ptr() + 4 * r0 * S * L if elementwise else None, st)
        finally:
            _model._PAR.update(prev)
        _advance_noise(B * K, (1, S, L), p.device)
        return ShiftSweepResult(te, sh_host, torch.argmin(te, dim=1), x_ph_all, kl)


def _advance_noise(rows, shape, device):
    """Consume from the device generator what `rows` calls of torch.randn(shape) consume (the
    reparameterisation draw of each of the reference's forwards, vae_teb_model.py:1046-1050, made and
    discarded by measure_transfer_entropy): one draw measures the Philox offset a draw of this shape
    takes, the rest is added to the offset (the same state as `rows` draws, without `rows` launches).
    Generators without an offset interface get the draws themselves."""
    idx = torch.device(device).index
    gen = torch.cuda.default_generators[torch.cuda.current_device() if idx is None else idx]
    if hasattr(gen, "get_offset") and hasattr(gen, "set_offset") and not torch.cuda.is_current_stream_capturing():
        o0 = gen.get_offset()
        torch.randn(shape, device=device)
        o1 = gen.get_offset()
        gen.set_offset(o0 + rows * (o1 - o0))
    else:
        for _ in range(rows):
            torch.randn(shape, device=device)
