"""From recordings to training windows, on the device: the counterpart of
create_hdf5_dataset_from_records_list (ref/hdf5_dataset/create_hdf5_dataset.py:352-508)
without its external record reader.

    recordings (2, L) -> overlapping windows -> signal-dropout gate -> FrontEnd.raw
                      -> one .npz file CombinedHDF5Dataset opens

What is the reference's:
  * the gate: find_flat_regions (:46-81) with tolerance 1e-9 and min_length 20 on both
    channels, the thresholds of :474-477 and the sample-weight rule of :458 — as one HIP
    launch over every window of every recording (vt_window_flat_stats) with the thresholds
    applied on the device to the kernel's output;
  * the channel order of st_input (:418: channel 0 FHR, channel 1 UP) and the two front-end
    calls (:421-441, FrontEnd.raw);
  * the file fields and layouts of create_initial_hdf5 / append_sample
    (ref/hdf5_dataset/hdf5_dataset.py:140-281) and target = target * weight (:498).
What is ours: the window placement (window_starts).  The reference places its blocks inside
EarlyMaestraMimoAdaptor.prepare_data, an external package that is not part of it.
Not ported: that reader, the plots, and HDF5 output (no h5py here; the .npz file holds the
same fields and CombinedHDF5Dataset reads both).
"""
import numpy as np
import torch

from . import _lib

STEP = 16   # raw samples per decimated step (out_dec_factor=16, ref :390): weights and targets live at this rate
RULES = ("max_flat_fhr", "max_flat_up", "total_flat_fhr", "total_flat_up", "weight")


def window_starts(L, N, overlap=0.5, tail="drop"):
    """Start samples of the N-sample windows of an L-sample recording (int64 array).

    hop = N - int(N * overlap) (>= 1); starts are 0, hop, 2 hop, ... while start + N <= L.
    tail="drop" leaves the samples after the last full hop out; tail="align" adds one last
    window at L - N when the last window does not already end at L.  Empty when L < N.

    These semantics are this package's own: the reference places its windows inside an
    external reader (EarlyMaestraMimoAdaptor.prepare_data, overlap_percentage=0.5), which is
    not available to compare against."""
    L, N = int(L), int(N)
    if N < 1:
        raise ValueError(f"window length {N} < 1")
    if tail not in ("drop", "align"):
        raise ValueError(f"tail must be 'drop' or 'align', got {tail!r}")
    hop = N - int(N * overlap)
    if hop < 1 or hop > N:
        raise ValueError(f"overlap {overlap} gives hop {hop} for N = {N} (need 1 <= hop <= N)")
    if L < N:
        return np.zeros(0, np.int64)
    starts = np.arange(0, L - N + 1, hop, dtype=np.int64)
    if tail == "align" and starts[-1] + N != L:
        starts = np.append(starts, np.int64(L - N))
    return starts


def _base_and_offsets(x, row_off, N):
    """The flat float32 device buffer and the bounds-checked int64 device offsets.  Host offsets
    (array-like) are checked on the host and uploaded; a device tensor costs one host read."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("x must be a float32 tensor on the device")
    if not x.is_contiguous():
        raise RuntimeError("Tensors must be contiguous.")
    N = int(N)
    if isinstance(row_off, torch.Tensor):
        off = row_off.to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
        lo, hi = (int(off.min()), int(off.max())) if off.numel() else (0, 0)
    else:
        host = np.ascontiguousarray(row_off, dtype=np.int64).reshape(-1)
        lo, hi = (int(host.min()), int(host.max())) if host.size else (0, 0)
        off = torch.from_numpy(host).to(x.device)
    if off.numel() and (lo < 0 or hi + max(N, 0) > x.numel()):
        raise ValueError(f"row offsets [{lo}, {hi}] + {N} leave the buffer of {x.numel()} elements")
    return x, off


def flat_stats(x, row_off, N, tolerance=1e-9, min_length=20):
    """(rows, 3) int32 device tensor {longest, total, count} of the qualifying flat regions of
    each row x.flatten()[row_off[r] : row_off[r] + N] (vt_window_flat_stats: find_flat_regions,
    ref create_hdf5_dataset.py:46-81, + the lengths of :462-472)."""
    x, off = _base_and_offsets(x, row_off, N)
    out = torch.empty((off.numel(), 3), dtype=torch.int32, device=x.device)
    _lib.call("vt_window_flat_stats", _lib.ptr(x), _lib.ptr(off), off.numel(), int(N), float(tolerance),
              int(min_length), _lib.ptr(out), _lib.stream())
    return out


def gather(x, row_off, N):
    """(rows, N) float32 device tensor: the rows copied bit for bit (vt_window_gather)."""
    x, off = _base_and_offsets(x, row_off, N)
    out = torch.empty((off.numel(), int(N)), dtype=torch.float32, device=x.device)
    _lib.call("vt_window_gather", _lib.ptr(x), _lib.ptr(off), off.numel(), int(N), _lib.ptr(out), _lib.stream())
    return out


class GateResult:
    """keep (W,) bool and the per-rule rejection masks {rule: (W,) bool}, on the device."""

    def __init__(self, keep, masks):
        self.keep, self.masks = keep, masks

    def counts(self):
        """{'windows', 'kept', 'rejected', one count per rule} as Python ints (one host read)."""
        names = list(self.masks)
        v = torch.stack([self.keep.sum()] + [self.masks[k].sum() for k in names]).tolist()
        W = int(self.keep.numel())
        out = {"windows": W, "kept": int(v[0]), "rejected": W - int(v[0])}
        out.update({k: int(c) for k, c in zip(names, v[1:])})
        return out


class QualityGate:
    """The window acceptance rules of ref create_hdf5_dataset.py:458-479 on the device.

    A window is rejected iff its longest FHR flat region > max_flat_fhr, its longest UP flat
    region > max_flat_up, its total FHR / UP flat length > total_flat_fhr / total_flat_up
    (:474-477; flat regions from find_flat_regions(tolerance, min_length), :462-463), or the
    mean of its sample weights < min_weight (:458).  A window can break several rules; each
    rule's mask is kept."""

    def __init__(self, max_flat_fhr=480, max_flat_up=1200, total_flat_fhr=1200, total_flat_up=1200, min_weight=0.90,
                 tolerance=1e-9, min_length=20):
        self.max_flat_fhr, self.max_flat_up = max_flat_fhr, max_flat_up
        self.total_flat_fhr, self.total_flat_up = total_flat_fhr, total_flat_up
        self.min_weight, self.tolerance, self.min_length = min_weight, tolerance, min_length

    def stats(self, x, row_off, N):
        """flat_stats with this gate's tolerance and min_length."""
        return flat_stats(x, row_off, N, self.tolerance, self.min_length)

    def __call__(self, stats, weight_mean=None):
        """stats: (W, 2, 3) int32 device tensor (window, channel {fhr, up}, {longest, total,
        count}); weight_mean: optional (W,) float64 device tensor.  -> GateResult."""
        if stats.dim() != 3 or stats.shape[1:] != (2, 3):
            raise ValueError(f"expected (W, 2, 3) flat statistics, got {tuple(stats.shape)}")
        masks = {"max_flat_fhr": stats[:, 0, 0] > self.max_flat_fhr,
                 "max_flat_up": stats[:, 1, 0] > self.max_flat_up,
                 "total_flat_fhr": stats[:, 0, 1] > self.total_flat_fhr,
                 "total_flat_up": stats[:, 1, 1] > self.total_flat_up}
        if weight_mean is None:
            masks["weight"] = torch.zeros_like(masks["max_flat_fhr"])
        else:
            masks["weight"] = weight_mean.to(torch.float64) < self.min_weight
        reject = masks["weight"].clone()
        for k in RULES[:4]:
            reject |= masks[k]
        return GateResult(~reject, masks)


class Recording:
    """One recording: x (2, L) float32, channel 0 FHR and channel 1 UP at 4 Hz (the st_input
    order of ref create_hdf5_dataset.py:418); guid its name (:455-456, :500).

    weight: optional (L // 16,) sample weights at the decimated rate, as the reference
    stores them (:416); target: optional scalar or (L // 16,) array, written as
    target * weight (:498); domain_start: the epoch of sample 0 (a window's epoch is
    domain_start + its start sample, :501); cs_label / bg_label: the file's labels."""

    def __init__(self, x, guid, weight=None, domain_start=0.0, target=None, cs_label=False, bg_label=False):
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if x.dim() != 2 or x.shape[0] != 2:
            raise ValueError(f"expected a (2, L) recording, got {tuple(x.shape)}")
        self.x = x.to(torch.float32)
        self.L = int(x.shape[1])
        self.guid = str(guid)
        self.domain_start = float(domain_start)
        self.cs_label, self.bg_label = bool(cs_label), bool(bg_label)
        steps = self.L // STEP
        self.weight = None
        if weight is not None:
            self.weight = np.ascontiguousarray(torch.as_tensor(weight).cpu().numpy(), dtype=np.float32).reshape(-1)
            if self.weight.shape[0] != steps:
                raise ValueError(f"{self.guid}: {self.weight.shape[0]} weights for {steps} steps (L // {STEP})")
        self.target = None
        if target is not None:
            t = np.asarray(torch.as_tensor(target).cpu().numpy(), dtype=np.float32)
            if t.ndim and t.reshape(-1).shape[0] != steps:
                raise ValueError(f"{self.guid}: {t.size} targets for {steps} steps (L // {STEP})")
            self.target = np.ascontiguousarray(np.broadcast_to(t.reshape(-1) if t.ndim else t, (steps,)))


class WindowBatch(dict):
    """One batch of kept windows: x (B, 2, N) on the device; rec (index into the
    recordings), start (sample) and epoch (domain_start + start) as host arrays; guid a list."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(name) from e


class RecordingWindows:
    """Every window of every recording, gated on the device, iterated in batches.

    The recordings are packed into one device buffer; one vt_window_flat_stats launch gives the
    flat-region statistics of all (window, channel) rows; `gate` is applied to them on the
    device; iterating yields WindowBatch objects whose x is the
    (B, 2, N) batch of FrontEnd.raw / fit_stats / DatasetStatsCalculator.calculate_stats,
    gathered from the packed buffer by vt_window_gather.  `report` holds the counts
    (windows, kept, rejected, one per rule); `result` the GateResult; `stats` the (W, 2, 3)
    kernel output; `rec` / `start` the host tables of all windows, `kept` the kept indices."""

    def __init__(self, recordings, N=5760, overlap=0.5, tail="drop", gate=QualityGate(), batch_size=256,
                 device="cuda"):
        self.recordings = list(recordings)
        self.N, self.batch_size, self.gate = int(N), int(batch_size), gate
        self.device = torch.device(device)
        if self.batch_size < 1:
            raise ValueError(f"batch_size {batch_size} < 1")
        recs = self.recordings
        rec_base = np.zeros(len(recs) + 1, np.int64)     # element offset of each recording in the buffer
        np.cumsum(np.array([2 * r.L for r in recs], np.int64), out=rec_base[1:])
        starts = [window_starts(r.L, self.N, overlap, tail) for r in recs]
        self.rec = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(starts)] + [np.zeros(0, np.int64)])
        self.start = np.concatenate(starts + [np.zeros(0, np.int64)])
        W = int(self.start.shape[0])
        lens = np.array([r.L for r in recs], np.int64)
        fhr_off = rec_base[self.rec] + self.start if W else np.zeros(0, np.int64)
        self.row_off_host = np.stack([fhr_off, fhr_off + (lens[self.rec] if W else 0)], axis=1)   # (W, 2)
        if recs:
            self.buffer = torch.cat([r.x.to(self.device).reshape(-1) for r in recs])
        else:
            self.buffer = torch.zeros(0, dtype=torch.float32, device=self.device)
        self.row_off = torch.from_numpy(self.row_off_host).to(self.device)
        self.stats = gate.stats(self.buffer, self.row_off_host, self.N).view(W, 2, 3)
        self.weight_mean = self._weight_means()
        self.result = gate(self.stats, self.weight_mean)
        self.report = self.result.counts()
        self.kept = torch.nonzero(self.result.keep).reshape(-1).cpu().numpy()

    def _weight_means(self):
        """(W,) float64 device tensor: mean weight over each window's N // 16 steps, an fp64 sum
        (difference of an fp64 running sum) over their number; None when no recording has weights."""
        recs = self.recordings
        if not any(r.weight is not None for r in recs) or not len(self.start):
            return None
        if self.N % STEP or np.any(self.start % STEP):
            raise ValueError(f"sample weights need N and every window start to be multiples of {STEP}")
        S = self.N // STEP
        w = [r.weight if r.weight is not None else np.ones(r.L // STEP, np.float32) for r in recs]
        base = np.zeros(len(recs) + 1, np.int64)
        np.cumsum(np.array([len(a) for a in w], np.int64), out=base[1:])
        run = torch.zeros(int(base[-1]) + 1, dtype=torch.float64, device=self.device)
        run[1:] = torch.cumsum(torch.from_numpy(np.concatenate(w)).to(self.device, torch.float64), 0)
        a = torch.from_numpy(base[self.rec] + self.start // STEP).to(self.device)
        return (run[a + S] - run[a]) / S

    @property
    def n_windows(self):
        return int(self.start.shape[0])

    @property
    def n_kept(self):
        return int(self.kept.shape[0])

    def __len__(self):
        return (self.n_kept + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for b0 in range(0, self.n_kept, self.batch_size):
            idx = self.kept[b0:b0 + self.batch_size]
            x = gather(self.buffer, self.row_off_host[idx], self.N).view(len(idx), 2, self.N)
            rec, start = self.rec[idx], self.start[idx]
            yield WindowBatch(x=x, rec=rec, start=start, guid=[self.recordings[i].guid for i in rec],
                              epoch=np.array([self.recordings[i].domain_start for i in rec], np.float64) + start)


def write_dataset(path, windows, frontend):
    """Write the kept windows of `windows` (a RecordingWindows) as one .npz file with the
    fields and per-sample layouts of create_initial_hdf5 / append_sample
    (ref/hdf5_dataset/hdf5_dataset.py:140-281), which CombinedHDF5Dataset opens:
    fhr, up (n, N); fhr_st (n, 43, S), fhr_ph (n, 44, S), fhr_up_ph (n, 130, S) — the raw,
    UN-normalised features of frontend.raw in file layout (C, S), as GpuNormalizer expects;
    target, weight (n, S): zeros / ones when the recording has none, else target * weight
    (ref create_hdf5_dataset.py:498) and the window's weights; epoch f4; cs_label, bg_label
    u1; guid a fixed-width byte-string array (the reader loads with allow_pickle=False).
    HDF5 output is out of scope (h5py is not a dependency).  Returns the number of samples."""
    path = str(path)
    if not path.endswith(".npz"):
        raise ValueError(f"write_dataset writes .npz files (HDF5 output is not supported), got {path}")
    p = frontend.plan
    if p.N != windows.N:
        raise ValueError(f"front-end built for N = {p.N}, windows are N = {windows.N}")
    S, C_ph = p.S, frontend.C_ph
    cols = {k: [] for k in ("fhr", "up", "fhr_st", "fhr_ph", "fhr_up_ph", "target", "weight", "epoch", "cs_label",
                            "bg_label", "guid")}
    for b in windows:
        r = frontend.raw(b.x)
        x = b.x.cpu().numpy()
        cols["fhr"].append(x[:, 0])
        cols["up"].append(x[:, 1])
        cols["fhr_st"].append(r["fhr_st"].cpu().numpy())
        pairs = r["pairs"].cpu().numpy()
        cols["fhr_ph"].append(pairs[:, :C_ph])
        cols["fhr_up_ph"].append(pairs[:, C_ph:])
        weight, target = np.ones((len(b.rec), S), np.float32), np.zeros((len(b.rec), S), np.float32)
        for i, (ri, s0) in enumerate(zip(b.rec, b.start)):
            rec = windows.recordings[ri]
            if rec.weight is not None or rec.target is not None:
                if S * STEP != windows.N or s0 % STEP:
                    raise ValueError(f"weights / targets need {STEP}-sample steps: N = {windows.N}, S = {S}, "
                                     f"start = {s0}")
                a = int(s0) // STEP
                if rec.weight is not None:
                    weight[i] = rec.weight[a:a + S]
                if rec.target is not None:
                    target[i] = rec.target[a:a + S] * weight[i]
        cols["weight"].append(weight)
        cols["target"].append(target)
        cols["epoch"].append(b.epoch.astype(np.float32))
        cols["cs_label"].append(np.array([windows.recordings[i].cs_label for i in b.rec], np.uint8))
        cols["bg_label"].append(np.array([windows.recordings[i].bg_label for i in b.rec], np.uint8))
        cols["guid"].extend(g.encode("utf-8") for g in b.guid)
    empty = {"fhr": (0, p.N), "up": (0, p.N), "fhr_st": (0, frontend.C_st, S), "fhr_ph": (0, C_ph, S),
             "fhr_up_ph": (0, frontend.C_x, S), "target": (0, S), "weight": (0, S), "epoch": (0,), "cs_label": (0,),
             "bg_label": (0,)}
    out = {}
    for k, shape in empty.items():
        dt = np.uint8 if k in ("cs_label", "bg_label") else np.float32
        out[k] = np.concatenate(cols[k]).astype(dt, copy=False) if cols[k] else np.zeros(shape, dt)
    out["guid"] = np.array(cols["guid"], dtype="S") if cols["guid"] else np.zeros(0, "S1")
    np.savez(path, **out)
    return int(out["fhr"].shape[0])
