"""The reference's evaluation analyses that scale the UP features, batched over (recording, gain):

    run_metrics_histogram_analysis   ref/model/graph_model.py:1510-1680   gains (1,)
    run_up_ablation_analysis         :1682-1777                           gains (1, 0)
    run_up_gain_sweep_analysis       :1779-1870                           gains [0, .5, 1, 1.5, 2]

All three are one computation: for each recording and each multiplicative gain g on the normalised
fhr_up_ph features, an eval-mode forward on x_ph * float(g) (:1833-1835), the per-sample mean of
measure_transfer_entropy(reduce_mean=False) (:1836-1839, :1598-1602), and VAF / MSE / SNR of mu_pr
against the normalised raw FHR (:1619-1645, :1842-1851).  The reference computes the metrics one
sample at a time in numpy on the host, runs every encoder twice per gain (forward, then
measure_transfer_entropy) and the target encoder again for every gain.  `GainSweep` runs the target
encoder once per recording and everything else once per (recording, gain) row, rows batched, with
nothing leaving the device:

    target encoder           prior (mu_y, logvar_y), c_logvar                   B rows, once
    vt_eval_scale_rows       x_ph * gain                                        B*K rows
    source + conditional     posterior pieces (c_logvar expanded per row)       B*K rows
    vt_te_latent_rows        te[b, k] = mean KL, z = mu_post + eps*exp(lv/2)    B*K rows
    decoder                  mu_pr                                              B*K rows
    vt_recon_metrics_rows    vaf, mse, snr_db, vaf_unclamped                    B*K rows

`recon_metrics` is the metrics kernel alone, for any forward's output.

Not ported: the reference's plots (plot_metrics_histograms, plot_te_gain_sweep), its pickle file of
the metric lists, the GUID selection and the dataset iteration (callers bring the batches).
"""
import numpy as np
import torch

from . import _lib
from . import model as _model
from .te import _advance_noise

DEFAULT_GAINS = (0.0, 0.5, 1.0, 1.5, 2.0)      # ref/model/graph_model.py:1802
ABLATION_GAINS = (1.0, 0.0)                    # intact, then UP zeroed (:1682-1777)


def check_gains(gains):
    """The gain list as float64 numpy (K,): at least one gain, all finite.  Each is applied as the
    reference applies float(g) to a float32 tensor: rounded to float32, then the IEEE product."""
    g = np.asarray(list(gains) if not isinstance(gains, np.ndarray) else gains, dtype=np.float64)
    if g.ndim != 1 or g.size == 0:
        raise ValueError(f"gains must be a non-empty 1-D list, got shape {g.shape}")
    with np.errstate(over="ignore"):
        g32 = g.astype(np.float32)
    if not np.isfinite(g).all() or not np.isfinite(g32).all():
        raise ValueError(f"gains must be finite in float32, got {g.tolist()}")
    return g


def recon_metrics(y_raw, mu_pr):
    """(vaf, mse, snr, vaf_unclamped) of the reconstruction mu_pr (B, n) or (B, K, n) against the
    ground truth y_raw (B, n) (or (B, n, 1)), float32 device tensors shaped like mu_pr's leading
    dimensions (vt_recon_metrics_rows; ref/model/graph_model.py:1619-1645: population variances,
    vaf clamped to [0, 1] and 0 when var(y) <= 1e-12, snr in dB and 100 when mse <= 1e-12).  No
    host synchronisation."""
    if y_raw.dim() == 3 and y_raw.size(-1) == 1:
        y_raw = y_raw.squeeze(-1)
    if y_raw.dim() != 2 or mu_pr.dim() not in (2, 3) or mu_pr.shape[0] != y_raw.shape[0] \
            or mu_pr.shape[-1] != y_raw.shape[-1]:
        raise ValueError(f"expected y_raw (B, n) and mu_pr (B, n) or (B, K, n), got {tuple(y_raw.shape)} and "
                         f"{tuple(mu_pr.shape)}")
    if y_raw.dtype != torch.float32 or mu_pr.dtype != torch.float32:
        raise ValueError(f"expected float32 tensors, got {y_raw.dtype} and {mu_pr.dtype}")
    if not (y_raw.is_cuda and mu_pr.is_cuda):
        raise ValueError("recon_metrics runs on the device: both tensors must be on the GPU")
    B, n = y_raw.shape
    K = mu_pr.shape[1] if mu_pr.dim() == 3 else 1
    y_raw, mu_pr = y_raw.contiguous(), mu_pr.contiguous()
    out = torch.empty((B * K, 4), device=mu_pr.device)
    _lib.call("vt_recon_metrics_rows", _lib.ptr(y_raw), _lib.ptr(mu_pr), B, K, n, _lib.ptr(out), _lib.stream())
    return _split_metrics(out, mu_pr.shape[:-1])


def _split_metrics(out, lead):
    m = out.t().contiguous()
    return tuple(m[i].view(*lead) for i in range(4))


class EvalSweepResult:
    """gains (the K gains, float64 numpy); te, vaf, mse, snr, vaf_unclamped (B, K) float32 on the
    device; mu_pr (B, K, n) and kl (B, K, S, L) when requested, else None."""

    __slots__ = ("gains", "te", "vaf", "mse", "snr", "vaf_unclamped", "mu_pr", "kl")

    def __init__(self, gains, te, vaf, mse, snr, vaf_unclamped, mu_pr=None, kl=None):
        self.gains, self.te, self.vaf, self.mse, self.snr = gains, te, vaf, mse, snr
        self.vaf_unclamped, self.mu_pr, self.kl = vaf_unclamped, mu_pr, kl

    def means(self):
        """Per-gain means over the recordings, (K,) tensors under the metric names: the reference's
        kld_means (here "te") and vaf_means (ref/model/graph_model.py:1862-1864), and the same for
        mse, snr and vaf_unclamped."""
        return {k: getattr(self, k).mean(dim=0) for k in ("te", "vaf", "mse", "snr", "vaf_unclamped")}


class GainSweep:
    """sweep = GainSweep(model); r = sweep(y_st, y_ph, x_ph, y_raw, gains) with the normalised
    fields y_st (B, S, C_st), y_ph (B, S, C_ph), x_ph (B, S, C_x) and y_raw (B, 16 S) on the device.

    rows_per_launch bounds the (recording, gain) rows of one pass through the kernels (the work
    buffers are sized by it); chunks are cut at whole recordings when a recording's K gains fit,
    inside one recording otherwise.  Every row's result depends on that row and its recording only.
    No host synchronisation; the model is left in eval mode (as measure_transfer_entropy leaves it).

    Noise.  eps (B, K, S, L) is used as given.  With eps=None the device generator is used as the
    reference's gain loop over one batch of B uses it (ref/model/graph_model.py:1832-1836): for each
    gain in order, one torch.randn((B, S, L)) is drawn for that gain's rows (the forward's
    reparameterisation draw), then the generator is advanced by one more draw of that shape (the one
    measure_transfer_entropy's forward makes and discards).  The noise of row (b, k) is what that
    loop gives it, and the device's random stream ends where the loop's ends."""

    def __init__(self, model, rows_per_launch=256):
        if rows_per_launch < 1:
            raise ValueError(f"rows_per_launch must be positive, got {rows_per_launch}")
        self.model, self.rows_per_launch = model, int(rows_per_launch)
        self._bufs = {}
        self._gains = {}

    def _buf(self, name, shape, device):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != device:
            b = self._bufs[name] = torch.empty(shape, dtype=torch.float32, device=device)
        return b

    def _gains_dev(self, gains, device):
        host = check_gains(gains)
        key = (tuple(host.tolist()), str(device))
        t = self._gains.get(key)
        if t is None:
            if len(self._gains) >= 16:
                self._gains.clear()
            t = self._gains[key] = torch.tensor(host, dtype=torch.float32, device=device)
        return t, host

    def _chunks(self, B, K):
        """(b0, nb, k0, nk): nb whole recordings from b0 (k0 = 0, nk = K), or gains
        [k0, k0 + nk) of the one recording b0."""
        R = self.rows_per_launch
        if K <= R:
            per = R // K
            return [(b0, min(per, B - b0), 0, K) for b0 in range(0, B, per)]
        return [(b, 1, k0, min(R, K - k0)) for b in range(B) for k0 in range(0, K, R)]

    @torch.no_grad()
    def __call__(self, y_st, y_ph, x_ph, y_raw, gains=DEFAULT_GAINS, eps=None, elementwise=False, return_mu=False):
        m = self.model
        if y_raw.dim() == 3 and y_raw.size(-1) == 1:
            y_raw = y_raw.squeeze(-1)
        for name, t, nd in (("y_st", y_st, 3), ("y_ph", y_ph, 3), ("x_ph", x_ph, 3), ("y_raw", y_raw, 2)):
            if t.dim() != nd or t.dtype != torch.float32 or not t.is_cuda or t.shape[0] != x_ph.shape[0]:
                raise ValueError(f"{name}: expected a float32 device tensor of {nd} dimensions and "
                                 f"{x_ph.shape[0]} recordings, got {t.dtype} {tuple(t.shape)} on {t.device}")
        B, S, C_x = x_ph.shape
        L, n = m.latent_dim_z, 16 * m.decoder.sequence_length
        if y_st.shape[1] != S or y_ph.shape[1] != S or S != m.decoder.sequence_length or y_raw.shape[1] != n:
            raise ValueError(f"the model decodes {m.decoder.sequence_length} steps to {n} samples; got y_st "
                             f"{tuple(y_st.shape)}, y_ph {tuple(y_ph.shape)}, x_ph {tuple(x_ph.shape)}, y_raw "
                             f"{tuple(y_raw.shape)}")
        dev = x_ph.device
        g_dev, g_host = self._gains_dev(gains, dev)
        K = len(g_host)
        if eps is not None and (tuple(eps.shape) != (B, K, S, L) or eps.dtype != torch.float32 or eps.device != dev):
            raise ValueError(f"eps: expected float32 {(B, K, S, L)} on {dev}, got {eps.dtype} {tuple(eps.shape)} "
                             f"on {eps.device}")
        y_st, y_ph, x_ph, y_raw = y_st.contiguous(), y_ph.contiguous(), x_ph.contiguous(), y_raw.contiguous()
        m.eval()
        if getattr(m, "h16_format", None):
            _lib.set_h16(m.h16_format == "fp16")
        if eps is None:
            eps = torch.empty((B, K, S, L), device=dev)
            for k in range(K):
                eps[:, k] = torch.randn((B, S, L), device=dev)    # the forward's draw for gain k
                _advance_noise(1, (B, S, L), dev)                 # measure_transfer_entropy's discarded draw
        else:
            eps = eps.contiguous()
        st = _lib.stream()
        prev = dict(_model._PAR)
        _model._PAR["on"], _model._PAR["next"] = bool(m.concurrent_encoders), 1
        try:
            mu_y, lv_full = m.target_encoder(y_st, y_ph)
            lv_p, c_lv = torch.split(lv_full, m.latent_dim_target, dim=-1)
            mu_y, lv_p = mu_y.contiguous(), lv_p.contiguous()
            te = torch.empty((B, K), device=dev)
            met = torch.empty((B * K, 4), device=dev)
            kl = torch.empty((B, K, S, L), device=dev) if elementwise else None
            mu_all = torch.empty((B, K, n), device=dev) if return_mu else None
            for (b0, nb, k0, nk) in self._chunks(B, K):
                R, r0 = nb * nk, b0 * K + k0
                xs = self._buf("x_scaled", (R, S, C_x), dev)
                _lib.call("vt_eval_scale_rows", x_ph.data_ptr() + 4 * b0 * S * C_x, nb, nk, S * C_x,
                          g_dev.data_ptr() + 4 * k0, _lib.ptr(xs), st)
                mu_x = m.source_encoder(xs)
                c_rep = c_lv[b0:b0 + nb].unsqueeze(1).expand(nb, nk, S, c_lv.shape[-1]).reshape(R, S, -1)
                mu_c, lv_q = m.conditional_encoder(mu_x, c_rep)
                z = self._buf("z", (R, S, L), dev)
                _lib.call("vt_te_latent_rows", _lib.ptr(mu_c), _lib.ptr(lv_q), mu_y.data_ptr() + 4 * b0 * S * L,
                          lv_p.data_ptr() + 4 * b0 * S * L, eps.data_ptr() + 4 * r0 * S * L, nb, nk, S * L,
                          _lib.ptr(z), None, te.data_ptr() + 4 * r0,
                          kl.data_ptr() + 4 * r0 * S * L if elementwise else None, st)
                mu_pr = m.decoder(z)[1]
                if return_mu:
                    mu_all.view(B * K, n)[r0:r0 + R].copy_(mu_pr)
                _lib.call("vt_recon_metrics_rows", y_raw.data_ptr() + 4 * b0 * n, _lib.ptr(mu_pr), nb, nk, n,
                          met.data_ptr() + 16 * r0, st)
        finally:
            _model._PAR.update(prev)
        vaf, mse, snr, vaf_u = _split_metrics(met, (B, K))
        return EvalSweepResult(g_host, te, vaf, mse, snr, vaf_u, mu_all, kl)
