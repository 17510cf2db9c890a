"""From gated windows to per-recording timelines, on the device: the stage after the per-window
analyses (vaeteb.evaluate, vaeteb.te), which all end at the window.

    RecordingWindows -> FrontEnd -> GainSweep (gain 1) -> stitched TE / reconstruction timelines
                     -> per-recording VAF / MSE / SNR over the covered samples

What is the reference's:
  * the overlap-average itself.  SeqVaeTeb.get_predictions (ref/model/vae_teb_model.py:1228-1246)
    places N overlapping rows on a (B, N, new_C) NaN canvas in a Python loop and takes nanmean over
    it; `overlap_mean` gives that mean through the same kernels, without the canvas;
  * the per-window numbers (transfer entropy as the mean KL, VAF / MSE / SNR of mu_pr against the
    normalised FHR: ref/model/graph_model.py:1598-1645), denormalize_signal_data (:83-85) and the
    (guid, epoch, ...) shape of its result rows.
What is ours: stitching the windows of a recording into one timeline (which window covers which
step, what happens where the quality gate dropped a window, how the dataset trim shifts everything).
The reference scores windows only and never does it.

Layout.  Every recording r of L_r samples owns L_r // step positions of a packed step timeline and
L_r positions of a packed sample timeline (TimelineLayout.step_base / sample_base are the running
sums).  A window that starts at sample `start` of recording `rec`, trimmed by the front-end's `trim`
steps at each end, covers the positions from

    step_base[rec] + start // step + trim          (S_out steps)
    sample_base[rec] + start + step * trim         (N_out samples)

Kernels (csrc/timeline.hip): vt_timeline_accumulate adds a batch of windows into the running sums
acc / wacc / count of a timeline, gathering through the ascending offset table — no atomics, the
same bits for every batch split; vt_timeline_finish divides (and denormalises); vt_timeline_metrics
is the metrics kernel of vaeteb.evaluate over the covered positions of each recording.
"""
import math

import numpy as np
import torch

from . import _lib

BLENDS = {"mean": 0, "taper": 1}


def _blend(blend):
    if blend not in BLENDS:
        raise ValueError(f"blend must be one of {sorted(BLENDS)}, got {blend!r}")
    return BLENDS[blend]


def check_offsets(dst_off, n, total, lengths=None):
    """The host tables of one accumulate call, checked before any launch: dst_off (W,) int64
    ascending (duplicates allowed) and >= 0, lengths (W,) int32 with 0 <= len <= n (None: all n),
    dst_off + len <= total.  Returns (dst_off, lengths) as contiguous numpy arrays."""
    off = np.ascontiguousarray(dst_off, dtype=np.int64).reshape(-1)
    n, total = int(n), int(total)
    if n < 1 or total < 0:
        raise ValueError(f"window length {n} < 1 or total {total} < 0")
    ln = None
    if lengths is not None:
        ln = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if ln.shape != off.shape:
            raise ValueError(f"{ln.shape[0]} lengths for {off.shape[0]} offsets")
        if ln.size and (ln.min() < 0 or ln.max() > n):
            raise ValueError(f"lengths must lie in [0, {n}], got [{ln.min()}, {ln.max()}]")
    if off.size:
        if np.any(np.diff(off) < 0):
            raise ValueError("window offsets must be ascending")
        end = off + (n if ln is None else ln.astype(np.int64))
        if off[0] < 0 or end.max() > total:
            raise ValueError(f"window offsets [{off[0]}, {off[-1]}] + lengths (up to {n}) leave the timeline of "
                             f"{total} positions")
    return off, ln


class TimelineLayout:
    """Host tables of the packed timelines of `recordings` (objects with a length L in samples, or
    the lengths themselves): step_base (R+1,) the running sum of L_r // step, sample_base (R+1,) the
    running sum of L_r."""

    def __init__(self, recordings, step=16):
        self.step = int(step)
        if self.step < 1:
            raise ValueError(f"step {step} < 1")
        self.lengths = np.array([int(getattr(r, "L", r)) for r in recordings], np.int64)
        if np.any(self.lengths < 0):
            raise ValueError("negative recording length")
        self.step_base = np.zeros(len(self.lengths) + 1, np.int64)
        np.cumsum(self.lengths // self.step, out=self.step_base[1:])
        self.sample_base = np.zeros(len(self.lengths) + 1, np.int64)
        np.cumsum(self.lengths, out=self.sample_base[1:])

    @property
    def n_steps(self):
        return int(self.step_base[-1])

    @property
    def n_samples(self):
        return int(self.sample_base[-1])

    def _tables(self, rec, start):
        rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1)
        start = np.ascontiguousarray(start, dtype=np.int64).reshape(-1)
        if rec.shape != start.shape:
            raise ValueError(f"{rec.shape[0]} recording indices for {start.shape[0]} starts")
        if rec.size and (rec.min() < 0 or rec.max() >= len(self.lengths)):
            raise ValueError(f"recording index outside [0, {len(self.lengths)})")
        if np.any(start % self.step):
            raise ValueError(f"every window start must be a multiple of {self.step} samples")
        return rec, start

    def step_offsets(self, rec, start, trim=0):
        """step_base[rec] + start // step + trim, int64 (W,)."""
        rec, start = self._tables(rec, start)
        return self.step_base[rec] + start // self.step + int(trim)

    def sample_offsets(self, rec, start, trim=0):
        """sample_base[rec] + start + step * trim, int64 (W,)."""
        rec, start = self._tables(rec, start)
        return self.sample_base[rec] + start + self.step * int(trim)

    def window_offsets(self, rec, start, frontend):
        """(step offsets, sample offsets) of windows run through `frontend` (its plan's N, S and step,
        its trim), checked against both timelines: ascending and inside them."""
        p = frontend.plan
        if p.step != self.step:
            raise ValueError(f"the front-end decimates by {p.step}, the layout by {self.step}")
        if p.S * p.step != p.N:
            raise ValueError(f"the front-end gives {p.S} steps of {p.step} samples for windows of {p.N}: the step "
                             f"and sample timelines would not line up")
        so = self.step_offsets(rec, start, frontend.trim)
        no = self.sample_offsets(rec, start, frontend.trim)
        check_offsets(so, frontend.S_out, self.n_steps)
        check_offsets(no, frontend.N_out, self.n_samples)
        return so, no


class TimelineState:
    """The running sums of one packed timeline on the device: acc, wacc (float32) and count (int32),
    `total` positions, zero at the start.  accumulate() adds windows (ascending over all calls);
    finish() gives the timeline."""

    def __init__(self, total, blend="mean", device="cuda"):
        self.total, self.blend = int(total), blend
        self._blend = _blend(blend)
        if self.total < 0:
            raise ValueError(f"total {total} < 0")
        self.device = torch.device(device)
        self.acc = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.wacc = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.count = torch.zeros(self.total, dtype=torch.int32, device=self.device)

    def accumulate(self, values, dst_off, lengths=None):
        """values (W, n) or (W, n, inner) float32 on the device; dst_off / lengths host tables
        (checked here), or device tensors that the caller has checked (check_offsets)."""
        if not isinstance(dst_off, torch.Tensor):
            off, ln = check_offsets(dst_off, values.shape[1] if values.dim() >= 2 else 1, self.total, lengths)
            dst_off = torch.from_numpy(off)
            lengths = None if ln is None else torch.from_numpy(ln)
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or not values.is_cuda \
                or values.dim() not in (2, 3):
            raise ValueError("values must be a float32 device tensor (W, n) or (W, n, inner)")
        W, n = values.shape[0], values.shape[1]
        inner = values.shape[2] if values.dim() == 3 else 1
        if dst_off.numel() != W or (lengths is not None and lengths.numel() != W):
            raise ValueError(f"{dst_off.numel()} offsets for {W} windows")
        values = values.contiguous()
        off = dst_off.to(device=values.device, dtype=torch.int64).contiguous()
        ln = None if lengths is None else lengths.to(device=values.device, dtype=torch.int32).contiguous()
        _lib.call("vt_timeline_accumulate", _lib.ptr(values), W, n, inner, _lib.ptr(off), _lib.ptr(ln), self._blend,
                  _lib.ptr(self.acc), _lib.ptr(self.wacc), _lib.ptr(self.count), self.total, _lib.stream())
        return self

    def finish(self, fill=math.nan, scale=1.0, shift=0.0):
        """(out, count): out[p] = (acc[p] / wacc[p]) * scale + shift where count[p] > 0, else fill."""
        out = torch.empty(self.total, dtype=torch.float32, device=self.device)
        _lib.call("vt_timeline_finish", _lib.ptr(self.acc), _lib.ptr(self.wacc), _lib.ptr(self.count), self.total,
                  float(fill), float(scale), float(shift), _lib.ptr(out), _lib.stream())
        return out, self.count


def stitch(values, dst_off, total, lengths=None, blend="mean", fill=math.nan, scale=1.0, shift=0.0, state=None):
    """Overlap-average of windows on a packed timeline of `total` positions.

    values (W, n) float32 on the device, or (W, n, inner): the mean over the inner axis (formed in
    double, rounded once) is the window's value.  Window w covers positions
    [dst_off[w], dst_off[w] + lengths[w]) (lengths None: n).  blend "mean": every window weighs 1;
    "taper": window sample i weighs min(i + 1, n - i).  Returns (out, count): the weighted mean
    times scale plus shift (float32 quotient, product, sum) and the int32 number of windows per
    position; `fill` where no window covers.  The offsets are checked on the host before any launch
    (ValueError: descending, negative, or past `total`).

    With state= (a TimelineState) the windows are only added to it and the state is returned;
    state.finish(fill, scale, shift) gives the output after the last batch.  Batches must continue
    the ascending order; any split of an ascending window list gives the bits of the single call."""
    n = values.shape[1] if getattr(values, "ndim", 0) >= 2 else 1
    off, ln = check_offsets(dst_off, n, total if state is None else state.total, lengths)
    if not isinstance(values, torch.Tensor) or not values.is_cuda:
        raise ValueError("values must be a float32 device tensor (W, n) or (W, n, inner)")
    if state is not None:
        if state.total != int(total) or state._blend != _blend(blend):
            raise ValueError("state was made for another total or blend")
        return state.accumulate(values, torch.from_numpy(off), None if ln is None else torch.from_numpy(ln))
    st = TimelineState(total, blend, values.device)
    st.accumulate(values, torch.from_numpy(off), None if ln is None else torch.from_numpy(ln))
    return st.finish(fill, scale, shift)


def overlap_rows(N, C, stride=16, new_C=4800):
    """Host tables of get_predictions' placement for one sample: row i < kept goes to i * stride with
    len = clamp(new_C - i * stride, 0, C); rows starting at or past new_C are dropped (the
    reference's break).  Returns (kept, offsets (kept,), lengths (kept,))."""
    N, C, stride, new_C = int(N), int(C), int(stride), int(new_C)
    if stride < 0 or new_C < 0 or C < 1 or N < 0:
        raise ValueError(f"N={N} C={C} stride={stride} new_C={new_C}")
    i = np.arange(N, dtype=np.int64)
    keep = i * stride < new_C
    kept = int(keep.sum())                       # a prefix: i * stride is non-decreasing
    off = i[:kept] * stride
    return kept, off, np.clip(new_C - off, 0, C).astype(np.int32)


def overlap_mean(x, stride=16, new_C=4800):
    """SeqVaeTeb.get_predictions(x, stride, new_C)[1] for x (B, N, C) float32 on the device, without
    the (B, N, new_C) canvas: (B, new_C), NaN where no row reaches.  One difference: a NaN inside x
    propagates into the positions it covers, where nanmean would skip it."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("x must be a float32 device tensor (B, N, C)")
    B, N, C = x.shape
    kept, off, ln = overlap_rows(N, C, stride, new_C)
    total = B * int(new_C)
    if B == 0 or kept == 0:
        return torch.full((B, int(new_C)), math.nan, dtype=torch.float32, device=x.device)
    offs = (np.arange(B, dtype=np.int64)[:, None] * int(new_C) + off[None, :]).reshape(-1)
    out, _ = stitch(x[:, :kept].reshape(B * kept, C), offs, total, lengths=np.tile(ln, B))
    return out.view(B, int(new_C))


class WindowScores:
    """The kept windows of a scored RecordingWindows: host rec / start / epoch (arrays) and guid
    (list); device (W,) te, vaf, mse, snr, vaf_unclamped — the per-window values of
    SeqVaeTeb.reconstruction_metrics, the reference's per-sample numbers; kl (W, S, L) and mu_pr
    (W, n) when kept, else None."""

    def __init__(self, rec, start, epoch, guid, te, vaf, mse, snr, vaf_unclamped, kl=None, mu_pr=None):
        self.rec, self.start, self.epoch, self.guid = rec, start, epoch, guid
        self.te, self.vaf, self.mse, self.snr, self.vaf_unclamped = te, vaf, mse, snr, vaf_unclamped
        self.kl, self.mu_pr = kl, mu_pr

    def __len__(self):
        return len(self.guid)


class RecordingTimelines:
    """Per recording i, views into the packed device buffers: te[i] (L_i // 16,) the mean KL over the
    latent per step, NaN where no kept window covers the step; recon[i] (L_i,) the normalised
    reconstruction; recon_raw[i] the same in bpm (None without denormalize); coverage_steps[i],
    coverage[i] the int32 numbers of windows per step / sample.  metrics (R, 5): vaf, mse, snr_db,
    vaf_unclamped of recon against the normalised FHR over the covered samples, and the covered
    fraction.  windows: a WindowScores.  layout: the TimelineLayout; denorm: the (scale, shift) of
    recon_raw = recon * scale + shift."""

    def __init__(self, layout, te, recon, recon_raw, count_steps, count, metrics, windows, denorm):
        self.layout, self.metrics, self.windows, self.denorm = layout, metrics, windows, denorm
        self.te_packed, self.recon_packed, self.recon_raw_packed = te, recon, recon_raw
        sb, nb = layout.step_base, layout.sample_base
        R = len(layout.lengths)
        cut = lambda t, b: [t[int(b[i]):int(b[i + 1])] for i in range(R)]
        self.te, self.coverage_steps = cut(te, sb), cut(count_steps, sb)
        self.recon, self.coverage = cut(recon, nb), cut(count, nb)
        self.recon_raw = cut(recon_raw, nb) if recon_raw is not None else None

    def rows(self):
        """One dict per kept window: guid, epoch, te, vaf, mse, snr (the (guid, epoch_num, ...) table of
        the reference's result files).  One host read."""
        w = self.windows
        if not len(w):
            return []
        v = torch.stack([w.te, w.vaf, w.mse, w.snr], 1).cpu().numpy()
        return [dict(guid=g, epoch=float(e), te=float(r[0]), vaf=float(r[1]), mse=float(r[2]), snr=float(r[3]))
                for g, e, r in zip(w.guid, w.epoch, v)]


class RecordingScorer:
    """scorer = RecordingScorer(model, frontend); r = scorer(windows) with a RecordingWindows.

    Per batch of kept windows (ascending, as RecordingWindows yields them): frontend(b.x), then
    GainSweep at the single gain 1 (elementwise KL and mu_pr kept), kl (b, S, L) added to the step
    timeline with the mean over the latent, mu_pr (b, 16 S) added to the sample timeline.  After the
    last batch both timelines are finished, the recordings' FHR is normalised as the front-end
    normalises a window's (vt_normalize_raw, the front-end's fhr statistics) and the per-recording
    metrics are taken over the covered samples.  Each window is scored independently; nothing is
    carried from one window to the next.

    Noise.  The sweep is always given its eps, so it makes no discarded draws.  sample=False: zeros
    (z = mu_post) — reproducible, the device's random stream untouched, and the result independent
    of batch_size (te bit for bit; recon as far as the decoder heads are row-count independent).
    sample=True: one torch.randn((b, 1, S, L)) per batch, so the noise a window gets depends on
    batch_size.

    No host synchronisation apart from building the offset tables from the host arrays that
    RecordingWindows already holds.  The model is left in eval mode."""

    def __init__(self, model, frontend, rows_per_launch=256):
        from .evaluate import GainSweep
        self.model, self.frontend = model, frontend
        self.sweep = GainSweep(model, rows_per_launch)
        self._zeros = None

    def _eps(self, b, S, L, dev, sample):
        if sample:
            return torch.randn((b, 1, S, L), device=dev)
        z = self._zeros
        if z is None or z.shape[0] < b or tuple(z.shape[1:]) != (1, S, L) or z.device != dev:
            z = self._zeros = torch.zeros((b, 1, S, L), device=dev)
        return z[:b]

    @torch.no_grad()
    def __call__(self, windows, sample=False, blend="mean", denormalize=True, keep_windows=False):
        fe, m = self.frontend, self.model
        p = fe.plan
        if fe.stats is None:
            raise RuntimeError("FrontEnd needs normalisation statistics (set_stats)")
        if p.N != windows.N:
            raise ValueError(f"front-end built for N = {p.N}, windows are N = {windows.N}")
        _blend(blend)
        layout = TimelineLayout(windows.recordings, step=p.step)
        rec, start = windows.rec[windows.kept], windows.start[windows.kept]
        step_off, samp_off = layout.window_offsets(rec, start, fe)
        dev = windows.buffer.device
        W, S, n, L = len(rec), fe.S_out, fe.N_out, m.latent_dim_z
        step_dev, samp_dev = torch.from_numpy(step_off).to(dev), torch.from_numpy(samp_off).to(dev)
        te_state = TimelineState(layout.n_steps, blend, dev)
        rc_state = TimelineState(layout.n_samples, blend, dev)
        per = torch.empty((5, W), device=dev)                       # te, vaf, mse, snr, vaf_unclamped
        kl_all = torch.empty((W, S, L), device=dev) if keep_windows else None
        mu_all = torch.empty((W, n), device=dev) if keep_windows else None
        epoch, guid = [], []
        m.eval()
        w0 = 0
        for b in windows:
            nb = b.x.shape[0]
            f = fe(b.x)
            r = self.sweep(f["fhr_st"], f["fhr_ph"], f["fhr_up_ph"], f["fhr"], gains=(1.0,),
                           eps=self._eps(nb, S, L, dev, sample), elementwise=True, return_mu=True)
            kl, mu = r.kl.view(nb, S, L), r.mu_pr.view(nb, n)
            te_state.accumulate(kl, step_dev[w0:w0 + nb])
            rc_state.accumulate(mu, samp_dev[w0:w0 + nb])
            for i, t in enumerate((r.te, r.vaf, r.mse, r.snr, r.vaf_unclamped)):
                per[i, w0:w0 + nb].copy_(t.reshape(nb))
            if keep_windows:
                kl_all[w0:w0 + nb].copy_(kl)
                mu_all[w0:w0 + nb].copy_(mu)
            epoch.append(b.epoch)
            guid.extend(b.guid)
            w0 += nb
        assert w0 == W, (w0, W)
        te, count_steps = te_state.finish()
        recon, count = rc_state.finish()
        fm, fs = fe.stats["fhr"]
        scale, shift = float(np.float32(fs) + np.float32(1e-8)), float(np.float32(fm))
        recon_raw = rc_state.finish(scale=scale, shift=shift)[0] if denormalize else None
        R, total = len(layout.lengths), layout.n_samples
        metrics = torch.empty((R, 5), device=dev)
        if R and total:
            # channel 0 of every recording, packed as the sample timeline is, then normalised
            rb = np.zeros(R + 1, np.int64)
            np.cumsum(2 * layout.lengths, out=rb[1:])
            if total >= 2 ** 31:
                raise ValueError(f"{total} samples in all: vt_normalize_raw takes rows below 2^31")
            raw = torch.cat([windows.buffer[int(rb[i]):int(rb[i]) + int(layout.lengths[i])] for i in range(R)])
            y = torch.empty_like(raw)
            _lib.call("vt_normalize_raw", _lib.ptr(raw), 1, total, total, fm, fs, _lib.ptr(y), _lib.stream())
            base = torch.from_numpy(layout.sample_base).to(dev)
            _lib.call("vt_timeline_metrics", _lib.ptr(y), _lib.ptr(recon), _lib.ptr(count), _lib.ptr(base), R,
                      _lib.ptr(metrics), _lib.stream())
        elif R:
            metrics[:, :4] = math.nan
            metrics[:, 4] = 0.0
        ws = WindowScores(rec, start, np.concatenate(epoch) if epoch else np.zeros(0, np.float64), guid,
                          per[0], per[1], per[2], per[3], per[4], kl_all, mu_all)
        return RecordingTimelines(layout, te, recon, recon_raw, count_steps, count, metrics, ws, (scale, shift))
