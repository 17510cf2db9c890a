"""The model's predictive distribution from K latent draws per recording: how sure it is (aleatoric
and epistemic variance), whether that sureness is justified (PIT histogram, interval coverage,
sharpness) and a held-out likelihood (ELBO and the importance-weighted bound), batched over
(recording, draw) with nothing leaving the device.  The reference trains the decoder's logvar_pr
with a Gaussian NLL (ref/model/vae_teb_model.py:932-979) and never reads it again; there is no
reference counterpart of these analyses, so the definitions below are the contract.

Recording b, sample i < n = 16 S, draw k < K; the decoder gives mu_ki, lv_ki; d_ki = y_i - mu_ki.

    l_ki            = -1/2 (log 2pi + lv_ki + d_ki^2 exp(-lv_ki))
    mean_i          = 1/K sum_k mu_ki
    var_aleatoric_i = 1/K sum_k exp(lv_ki)
    var_epistemic_i = 1/K sum_k (mu_ki - mean_i)^2        never negative, exactly 0 when the draws coincide
    logdens_i       = LSE_k l_ki - log K                  log density of the K-component mixture at y_i
    pit_i           = 1/K sum_k Phi(d_ki exp(-lv_ki / 2)) the mixture CDF at y_i
    ll_bk           = sum_i l_ki

per recording, with v = var_aleatoric + var_epistemic:

    nll_mixture     = -1/n sum_i logdens_i
    nll_moment      = 1/n sum_i 1/2 (log 2pi + log v_i + (y_i - mean_i)^2 / v_i)
    sharpness       = 1/n sum_i sqrt(v_i)
    pit_hist[j]     = #{i : min(bins - 1, floor(pit_i bins)) = j}        int32; a PIT of 1.0 in the last bin
    coverage[level] = 1/n #{i : |pit_i - 1/2| <= level / 2}
    elbo            = 1/K sum_k (ll_bk + logw_bk)
    iwae            = LSE_k (ll_bk + logw_bk) - log K

source="posterior": z_k = mu_post + eps_k exp(logvar_post / 2) and, over the S L latent elements,
logw_bk = 1/2 sum_j [lv_q - lv_p + eps_kj^2 - (z_kj - mu_p)^2 exp(-lv_p)] = log p(z|y) - log q(z|x,y)
(the q quadratic written with eps, which is exact).  source="prior": z_k = mu_prior + eps_k
exp(logvar_prior / 2) and logw = 0; elbo and iwae are then the Monte-Carlo expected and marginal
log-likelihood under the prior: what the model predicts without the UP channel's information (the
source and conditional encoders do not run).  A sample whose PIT is NaN is counted in no bin and no
coverage level.

The log 2pi is part of every likelihood here and is absent from the training nll_loss: for K = 1,
nll_mixture - 1/2 log 2pi of a row is that row's share of compute_loss's nll_loss (their mean over
the rows is the batch's nll_loss).

    encoders               mu, logvar of the latent (posterior or prior)            B rows, once
    vt_pred_draw_rows      z = mu + eps exp(logvar / 2), logw                        B*K rows
    decoder                mu_pr, logvar_pr                                          B*K rows
    vt_pred_mixture_rows   per-sample bands, logdens, pit; per-tile partial sums     (tiles, B) workgroups
    vt_pred_finish         per-recording scalars, ll, histogram, coverage            B workgroups, once
    vt_recon_metrics_rows  vaf, mse, snr, vaf_unclamped of the predictive mean       B rows

Not here: stitching the bands into recording timelines (mean and var_* are (B, n), which
vaeteb.timeline.stitch takes), plots, the mixture's CRPS (O(K^2)) and gradients.
"""
import numpy as np
import torch

from . import _lib
from . import model as _model
from .evaluate import recon_metrics

DEFAULT_LEVELS = (0.5, 0.9, 0.95)
MAX_DRAWS, MAX_BINS, MAX_LEVELS = 64, 256, 8        # csrc/predictive.hip
SOURCES = ("posterior", "prior")


def check_levels(levels):
    """The central-interval levels as float64 numpy (n_levels,): at most MAX_LEVELS, each in (0, 1)."""
    lv = np.asarray(list(levels), dtype=np.float64)
    if lv.ndim != 1 or lv.size > MAX_LEVELS:
        raise ValueError(f"levels must be a 1-D list of at most {MAX_LEVELS}, got shape {lv.shape}")
    if not ((lv > 0) & (lv < 1)).all():
        raise ValueError(f"levels must lie in (0, 1), got {lv.tolist()}")
    return lv


class PredictiveResult:
    """B recordings, K draws, n = 16 S samples; float32 device tensors unless noted.

    mean, var_aleatoric, var_epistemic (B, n); nll_mixture, nll_moment, sharpness (B,); elbo, iwae
    (B,), None for the plug-in predictive (n_samples=0); ll, logw (B, K); pit_hist (B, bins) int32;
    coverage (B, n_levels); levels (float64 numpy), bins, source; vaf, mse, snr, vaf_unclamped (B,)
    of the predictive mean (vaeteb.evaluate.recon_metrics); z_mu, z_logvar (B, S, L) the latent
    distribution the draws came from; pit, logdens (B, n) with return_pit, else None; z (B, K, S, L),
    mu_pr, logvar_pr (B, K, n) with return_samples, else None."""

    __slots__ = ("mean", "var_aleatoric", "var_epistemic", "nll_mixture", "nll_moment", "sharpness", "elbo", "iwae",
                 "ll", "logw", "pit_hist", "coverage", "levels", "bins", "source", "vaf", "mse", "snr",
                 "vaf_unclamped", "z_mu", "z_logvar", "pit", "logdens", "z", "mu_pr", "logvar_pr")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    @property
    def sd(self):
        """The predictive standard deviation sqrt(var_aleatoric + var_epistemic), (B, n)."""
        return (self.var_aleatoric + self.var_epistemic).sqrt()

    def means(self):
        """Means over the recordings under the result's names: scalars for nll_mixture, nll_moment,
        sharpness, vaf, mse, snr, vaf_unclamped (and elbo, iwae when present), (n_levels,) for
        coverage; pit_hist: the pooled histogram as fractions, (bins,)."""
        names = ["nll_mixture", "nll_moment", "sharpness", "vaf", "mse", "snr", "vaf_unclamped", "coverage"]
        names += [k for k in ("elbo", "iwae") if getattr(self, k) is not None]
        out = {k: getattr(self, k).mean(dim=0) for k in names}
        h = self.pit_hist.sum(dim=0).to(torch.float32)
        out["pit_hist"] = h / h.sum().clamp_min(1.0)
        return out


class Predictive:
    """pred = Predictive(model); r = pred(y_st, y_ph, x_ph, y_raw, n_samples=16) with the normalised
    fields y_st (B, S, C_st), y_ph (B, S, C_ph), x_ph (B, S, C_x) and y_raw (B, 16 S) on the device.

    rows_per_launch bounds the (recording, draw) rows of one pass through the decoder and the mixture
    kernel (the work buffers are sized by it); chunks are whole recordings, rows_per_launch // K at a
    time, so a recording's K rows are reduced in one workgroup pass.  Every recording's result depends
    on that recording only.  No host synchronisation; the model is left in eval mode.

    n_samples=0 is the plug-in predictive: K = 1, z = the latent mean, no noise is drawn, elbo and
    iwae are None.  source: "posterior" (default) or "prior".

    Noise.  eps (B, K, S, L) is used as given.  With eps=None one torch.randn((B, K, S, L)) is drawn
    from the device generator and nothing else, so the device's random stream ends where that single
    draw ends (and is untouched for n_samples=0)."""

    def __init__(self, model, rows_per_launch=256):
        if rows_per_launch < 1:
            raise ValueError(f"rows_per_launch must be positive, got {rows_per_launch}")
        self.model, self.rows_per_launch = model, int(rows_per_launch)
        self._bufs = {}
        self._levels = {}

    def _buf(self, name, shape, device, dtype=torch.float32):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != device:
            b = self._bufs[name] = torch.empty(shape, dtype=dtype, device=device)
        return b

    def _levels_dev(self, host, device):
        key = (tuple(host.tolist()), str(device))
        t = self._levels.get(key)
        if t is None:
            if len(self._levels) >= 16:
                self._levels.clear()
            t = self._levels[key] = torch.tensor(host, dtype=torch.float64, device=device)
        return t

    @torch.no_grad()
    def __call__(self, y_st, y_ph, x_ph, y_raw, n_samples=16, eps=None, source="posterior", bins=20,
                 levels=DEFAULT_LEVELS, return_samples=False, return_pit=False):
        m = self.model
        n_samples, bins = int(n_samples), int(bins)
        if source not in SOURCES:
            raise ValueError(f"source must be one of {SOURCES}, got {source!r}")
        if n_samples < 0 or n_samples > MAX_DRAWS:
            raise ValueError(f"n_samples must be in 0..{MAX_DRAWS}, got {n_samples}")
        K = max(n_samples, 1)
        if K > self.rows_per_launch:
            raise ValueError(f"a recording's {K} draws do not fit rows_per_launch = {self.rows_per_launch}")
        if bins < 1 or bins > MAX_BINS:
            raise ValueError(f"bins must be in 1..{MAX_BINS}, got {bins}")
        lv_host = check_levels(levels)
        if y_raw.dim() == 3 and y_raw.size(-1) == 1:
            y_raw = y_raw.squeeze(-1)
        for name, t, nd in (("y_st", y_st, 3), ("y_ph", y_ph, 3), ("x_ph", x_ph, 3), ("y_raw", y_raw, 2)):
            if t.dim() != nd or t.dtype != torch.float32 or not t.is_cuda or t.shape[0] != x_ph.shape[0]:
                raise ValueError(f"{name}: expected a float32 device tensor of {nd} dimensions and "
                                 f"{x_ph.shape[0]} recordings, got {t.dtype} {tuple(t.shape)} on {t.device}")
        B, S, _ = x_ph.shape
        L, n = m.latent_dim_z, 16 * m.decoder.sequence_length
        if y_st.shape[1] != S or y_ph.shape[1] != S or S != m.decoder.sequence_length or y_raw.shape[1] != n:
            raise ValueError(f"the model decodes {m.decoder.sequence_length} steps to {n} samples; got y_st "
                             f"{tuple(y_st.shape)}, y_ph {tuple(y_ph.shape)}, x_ph {tuple(x_ph.shape)}, y_raw "
                             f"{tuple(y_raw.shape)}")
        dev = x_ph.device
        if eps is not None and n_samples == 0:
            raise ValueError("n_samples=0 draws no noise: eps must be None")
        if eps is not None and (tuple(eps.shape) != (B, K, S, L) or eps.dtype != torch.float32 or eps.device != dev):
            raise ValueError(f"eps: expected float32 {(B, K, S, L)} on {dev}, got {eps.dtype} {tuple(eps.shape)} "
                             f"on {eps.device}")
        y_st, y_ph, x_ph, y_raw = y_st.contiguous(), y_ph.contiguous(), x_ph.contiguous(), y_raw.contiguous()
        m.eval()
        if getattr(m, "h16_format", None):
            _lib.set_h16(m.h16_format == "fp16")
        if n_samples > 0:
            eps = torch.randn((B, K, S, L), device=dev) if eps is None else eps.contiguous()
        lv_dev = self._levels_dev(lv_host, dev)
        n_lv = len(lv_host)
        tiles = -(-n // _lib.lib().fns["vt_pred_tile"]())
        stride = K + 3 + bins + n_lv
        P, st = _lib.ptr, _lib.stream()
        prev = dict(_model._PAR)
        _model._PAR["on"], _model._PAR["next"] = bool(m.concurrent_encoders), 1
        try:
            if source == "prior":
                mu_y, lv_full = m.target_encoder(y_st, y_ph)
                z_mu, z_lv = mu_y.contiguous(), torch.split(lv_full, m.latent_dim_target, dim=-1)[0].contiguous()
                mu_p = lv_p = None
            else:
                mu_p, lv_p, z_mu, z_lv = (t.contiguous() for t in m.encode(y_st, y_ph, x_ph))
            new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
            mean, var_a, var_e = new(B, n), new(B, n), new(B, n)
            pit, logdens = (new(B, n), new(B, n)) if return_pit else (None, None)
            logw = new(B, K)
            z_all = new(B, K, S, L) if return_samples else None
            mu_all, lv_all = (new(B, K, n), new(B, K, n)) if return_samples else (None, None)
            ws = self._buf("ws", (B * tiles * stride,), dev, torch.float64)
            per = self.rows_per_launch // K
            for b0 in range(0, B, per):
                nb = min(per, B - b0)
                R, r0 = nb * K, b0 * K
                if n_samples == 0:
                    z = z_mu[b0:b0 + nb]
                    logw[b0:b0 + nb].zero_()
                else:
                    z = self._buf("z", (R, S, L), dev)
                    off = 4 * b0 * S * L
                    _lib.call("vt_pred_draw_rows", z_mu.data_ptr() + off, z_lv.data_ptr() + off,
                              eps.data_ptr() + 4 * r0 * S * L, None if mu_p is None else mu_p.data_ptr() + off,
                              None if lv_p is None else lv_p.data_ptr() + off, nb, K, S * L, P(z),
                              logw.data_ptr() + 4 * r0, st)
                _, mu_pr, lv_pr = m.decoder(z)
                mu_pr, lv_pr = mu_pr.contiguous(), lv_pr.contiguous()
                if return_samples:
                    z_all.view(B * K, S, L)[r0:r0 + R].copy_(z)
                    mu_all.view(B * K, n)[r0:r0 + R].copy_(mu_pr)
                    lv_all.view(B * K, n)[r0:r0 + R].copy_(lv_pr)
                o = 4 * b0 * n
                _lib.call("vt_pred_mixture_rows", y_raw.data_ptr() + o, P(mu_pr), P(lv_pr), nb, K, n, bins, P(lv_dev),
                          n_lv, mean.data_ptr() + o, var_a.data_ptr() + o, var_e.data_ptr() + o,
                          pit.data_ptr() + o if return_pit else None, logdens.data_ptr() + o if return_pit else None,
                          ws.data_ptr() + 8 * b0 * tiles * stride, st)
            out, ll = new(B, 5), new(B, K)
            hist, cov = new(B, bins, dtype=torch.int32), new(B, n_lv)
            _lib.call("vt_pred_finish", P(ws), P(logw), B, K, n, bins, n_lv, P(out), P(ll), P(hist),
                      P(cov) if n_lv else None, st)
        finally:
            _model._PAR.update(prev)
        s = out.t().contiguous()
        vaf, mse, snr, vaf_u = recon_metrics(y_raw, mean)
        return PredictiveResult(
            mean=mean, var_aleatoric=var_a, var_epistemic=var_e, nll_mixture=s[0], nll_moment=s[1], sharpness=s[2],
            elbo=s[3] if n_samples else None, iwae=s[4] if n_samples else None, ll=ll, logw=logw, pit_hist=hist,
            coverage=cov, levels=lv_host, bins=bins, source=source, vaf=vaf, mse=mse, snr=snr, vaf_unclamped=vaf_u,
            z_mu=z_mu, z_logvar=z_lv, pit=pit, logdens=logdens, z=z_all, mu_pr=mu_all, logvar_pr=lv_all)
