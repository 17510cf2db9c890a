"""Normalisation statistics of a dataset, accumulated on the device from the online front-end.

The reference computes them offline (ref/hdf5_dataset/calculate_dataset_stats.py:14-444) from
features its CPU front-end wrote to HDF5.  Here the raw features `FrontEnd.raw()` leaves on the
device are reduced in one fused, deterministic pass (csrc/stats.hip: vt_stats_accum /
vt_stats_accum_raw) to the same per-channel fp64 {count, sum, sum of squares}, and finalised
on the host with the reference's formula:

    acc = StatsAccumulator.for_frontend(fe)
    for x in windows:                    # (B, 2, N) float32 on the device
        acc.update_windows(fe, x)
    fe.set_stats(acc.finalize())         # or: fe.fit_stats(windows)
    acc.save("stats_mine.npz")           # FrontEnd(plan, dict(np.load(...))) reads it back

`finalize_state` is plain numpy, so the formula can be checked without a GPU.
"""
import numpy as np

SINGLE_FIELDS = ("fhr", "up")
KIND_REGULAR, KIND_LOG, KIND_ASINH = 0, 1, 2


def finalize_state(count, sum_, sum_sq, single=False):
    """(mean, variance) from accumulated fp64 sums: _finalize_stats
    (calculate_dataset_stats.py:223-273).  mean = sum / count, variance =
    max(0, sum_sq / count - mean^2); a channel without data gives 0 and 0.  Multi-channel
    results are float32 arrays, single-channel results Python floats."""
    count = np.asarray(count, np.int64).reshape(-1)
    s = np.asarray(sum_, np.float64).reshape(-1)
    q = np.asarray(sum_sq, np.float64).reshape(-1)
    safe = np.where(count > 0, count, 1)
    mean = s / safe
    var = q / safe - mean ** 2
    mean[count == 0] = 0
    var[count == 0] = 0
    var[var < 0] = 0
    if single:
        return float(mean[0]), float(var[0])
    return mean.astype(np.float32), var.astype(np.float32)


def channel_kinds(field, n_channels):
    """The reference's transform per channel (calculate_dataset_stats.py:50-60): fhr_st channel 0
    regular and the others log, fhr_ph / fhr_up_ph all asinh, anything else regular."""
    k = np.zeros(n_channels, np.int32)
    if field == "fhr_st":
        k[1:] = KIND_LOG
    elif field in ("fhr_ph", "fhr_up_ph"):
        k[:] = KIND_ASINH
    return k


def default_fields(C_st=43, C_ph=44, C_x=130):
    return {"fhr": None, "up": None, "fhr_st": (C_st, channel_kinds("fhr_st", C_st)),
            "fhr_ph": (C_ph, channel_kinds("fhr_ph", C_ph)), "fhr_up_ph": (C_x, channel_kinds("fhr_up_ph", C_x))}


def chunking():
    """(rows, cols) of the batch-row x step chunk one partial of the kernel covers."""
    import ctypes
    from . import _lib
    r, c = ctypes.c_int(), ctypes.c_int()
    _lib.call("vt_stats_chunking", ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


class StatsAccumulator:
    """Device-resident {count int64, sum fp64, sum_sq fp64} per field and channel.

    fields: name -> (C, kinds) for a (B, C, S) feature field, None for a single-channel raw
    field ((B, N) rows); default: the reference's five fields at J=11, Q=4.
    trim: decimated steps dropped at each end of a feature field; raw rows lose trim * step
    samples at each end (calculate_dataset_stats.py:343-351)."""

    def __init__(self, fields=None, device="cuda", trim=0, step=16, log_eps=1e-6):
        import torch
        self.device = torch.device(device)
        self.trim, self.step, self.log_eps = int(trim), int(step), float(log_eps)
        fields = default_fields() if fields is None else fields
        self.fields, self._slice, self._kind, self._work, self.windows = {}, {}, {}, {}, {}
        n = 0
        for name, spec in fields.items():
            C = 1 if spec is None else int(spec[0])
            self.fields[name] = None if spec is None else (C, np.asarray(spec[1], np.int32).reshape(-1))
            if spec is not None:
                if self.fields[name][1].shape[0] != C:
                    raise ValueError(f"{name}: {self.fields[name][1].shape[0]} kinds for {C} channels")
                self._kind[name] = torch.as_tensor(self.fields[name][1], device=self.device)
            self._slice[name] = slice(n, n + C)
            self.windows[name] = 0
            n += C
        # one allocation per dtype; a field's state is a contiguous slice of each
        self._count = torch.zeros(n, dtype=torch.int64, device=self.device)
        self._sums = torch.zeros((2, n), dtype=torch.float64, device=self.device)

    @classmethod
    def for_frontend(cls, frontend, log_eps=1e-6):
        return cls(default_fields(frontend.C_st, frontend.C_ph, frontend.C_x), frontend.plan.device,
                   trim=frontend.trim, step=frontend.plan.step, log_eps=log_eps)

    # ------------------------------------------------------------------ state
    def state(self, field):
        """(count, sum, sum_sq) device views of one field."""
        sl = self._slice[field]
        return self._count[sl], self._sums[0, sl], self._sums[1, sl]

    def reset(self):
        self._count.zero_()
        self._sums.zero_()
        self.windows = {k: 0 for k in self.windows}

    @property
    def n_windows(self):
        return max(self.windows.values()) if self.windows else 0

    def _workspace(self, field, B, C, S_len):
        import ctypes
        import torch
        from . import _lib
        need = ctypes.c_int64()
        _lib.call("vt_stats_workspace_bytes", B, C, S_len, ctypes.byref(need))
        w = self._work.get(field)
        if w is None or w.numel() * 8 < need.value:
            w = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=self.device)
            self._work[field] = w
        return w

    # ---------------------------------------------------------------- updates
    def update(self, field, tensor, in_C=None, trim=None):
        """Accumulate a (B, C, S) float32 feature tensor in the reference's stored layout, or
        (B, N) raw rows for a single-channel field, on the current stream.  in_C: the channel
        count of the buffer `tensor` is a channel sub-view of (e.g. pairs[:, C_ph:])."""
        import torch
        from . import _lib
        if field not in self.fields:
            raise KeyError(field)
        t = torch.as_tensor(tensor)
        if t.dtype != torch.float32 or t.device.type != self.device.type:
            t = t.to(device=self.device, dtype=torch.float32)
        trim = self.trim if trim is None else int(trim)
        cnt, s, q = self.state(field)
        spec = self.fields[field]
        if spec is None:
            if t.dim() != 2:
                raise ValueError(f"{field}: expected (B, N) rows, got {tuple(t.shape)}")
            if t.stride(1) != 1:
                t = t.contiguous()
            B, N = t.shape
            cut = trim * self.step
            if B == 0:
                return
            if 2 * cut >= N:
                raise ValueError(f"{field}: trim of {cut} samples at each end leaves nothing of {N}")
            stride = t.stride(0) if B > 1 else N
            w = self._workspace(field, B, 1, N - 2 * cut)
            _lib.call("vt_stats_accum_raw", t.data_ptr() + 4 * cut, B, stride, N - 2 * cut, cnt.data_ptr(),
                      s.data_ptr(), q.data_ptr(), w.data_ptr(), w.numel() * 8, _lib.stream())
        else:
            C, _ = spec
            if t.dim() != 3 or t.shape[1] != C:
                raise ValueError(f"{field}: expected (B, {C}, S) features, got {tuple(t.shape)}")
            B, _, S = t.shape
            if B == 0 or C == 0:
                return
            if in_C is None:
                t, in_C = t.contiguous(), C
            elif in_C < C or t.stride(2) != 1 or t.stride(1) != S or (B > 1 and t.stride(0) != in_C * S):
                raise ValueError(f"{field}: not a channel sub-view of a (B, {in_C}, {S}) buffer")
            if 2 * trim >= S:
                raise ValueError(f"{field}: trim of {trim} steps at each end leaves nothing of {S}")
            w = self._workspace(field, B, C, S - 2 * trim)
            _lib.call("vt_stats_accum", t.data_ptr(), B, C, in_C, S, trim, S - 2 * trim,
                      self._kind[field].data_ptr(), self.log_eps, cnt.data_ptr(), s.data_ptr(), q.data_ptr(),
                      w.data_ptr(), w.numel() * 8, _lib.stream())
        self.windows[field] += int(B)

    def update_windows(self, frontend, x, side=None):
        """frontend.raw(x, side) and all five fields from its buffers; with a side stream the
        cross pairs are reduced there, and the current stream joins it before returning."""
        import torch
        from . import _lib
        r = frontend.raw(x, side)
        trim = frontend.trim
        if frontend.plan.step != self.step:
            raise ValueError(f"front-end decimates by {frontend.plan.step}, accumulator by {self.step}")
        pairs, C_ph, C_x = r["pairs"], frontend.C_ph, frontend.C_x
        if "fhr_st" in self.fields:
            self.update("fhr_st", r["fhr_st"], trim=trim)
        if "fhr_ph" in self.fields and C_ph:
            self.update("fhr_ph", pairs[:, :C_ph], in_C=pairs.shape[1], trim=trim)
        if "fhr_up_ph" in self.fields and C_x:
            if "cross" in r:
                with torch.cuda.stream(side):
                    self.update("fhr_up_ph", r["cross"], trim=trim)
                _lib.wait_for(torch.cuda.current_stream(), side)
            else:
                self.update("fhr_up_ph", pairs[:, C_ph:], in_C=pairs.shape[1], trim=trim)
        for ch, f in enumerate(SINGLE_FIELDS):
            if f in self.fields:
                self.update(f, x[:, ch], trim=trim)

    # ------------------------------------------------------------ combination
    def _check_same(self, other):
        if list(self._slice.items()) != list(other._slice.items()):
            raise ValueError("accumulators hold different fields")

    def merge(self, other):
        """Add another accumulator's state (same fields) to this one."""
        self._check_same(other)
        self._count += other._count.to(self.device)
        self._sums += other._sums.to(self.device)
        for k in self.windows:
            self.windows[k] += other.windows[k]
        return self

    def all_reduce(self, group=None):
        """One SUM all-reduce of the packed state over the ranks of a sharded dataset.  The
        counts travel as fp64 (exact below 2^53 elements per channel)."""
        import torch
        import torch.distributed as dist
        n = self._count.numel()
        packed = torch.cat([self._count.double(), self._sums.reshape(-1),
                            torch.tensor([float(self.windows[k]) for k in self.windows], dtype=torch.float64,
                                         device=self.device)])
        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
        self._count.copy_(packed[:n].round().long())
        self._sums.copy_(packed[n:3 * n].reshape(2, n))
        for k, v in zip(self.windows, packed[3 * n:].tolist()):   # host sync: the window counts
            self.windows[k] = int(round(v))
        return self

    # --------------------------------------------------------------- results
    def host_state(self):
        """{field: (count, sum, sum_sq)} as numpy arrays (synchronises)."""
        cnt, sums = self._count.cpu().numpy(), self._sums.cpu().numpy()
        return {f: (cnt[sl].copy(), sums[0, sl].copy(), sums[1, sl].copy()) for f, sl in self._slice.items()}

    def finalize(self):
        """The '<field>_mean' / '<field>_variance' / '<field>_count' mapping FrontEnd.set_stats,
        GpuNormalizer and data.load_stats_file's consumers read.  The only host sync."""
        out = {}
        for f, (cnt, s, q) in self.host_state().items():
            single = self.fields[f] is None
            out[f + "_mean"], out[f + "_variance"] = finalize_state(cnt, s, q, single)
            out[f + "_count"] = int(cnt[0]) if single else cnt
        return out

    def save(self, path):
        """Write the stats_*.npz layout of vaeteb/data (n_windows and the finalize() keys)."""
        st = self.finalize()
        np.savez(path, n_windows=self.n_windows, **{k: np.asarray(v) for k, v in st.items()})
        return st


class DatasetStatsCalculator:
    """The reference's calculator (calculate_dataset_stats.py:14-444: constructor, attributes,
    calculate_stats and its nested result) on the device accumulator."""

    def __init__(self, trim_minutes=None, device=None):
        self.stats_fields = ["fhr", "up", "fhr_st", "fhr_ph", "fhr_up_ph"]
        self.trim_minutes = trim_minutes
        self.device = "cuda" if device is None else device
        if trim_minutes is not None:
            self.trim_samples_raw = int(4 * 60 * trim_minutes)
            self.trim_samples_decimated = self.trim_samples_raw // 16
        else:
            self.trim_samples_raw = 0
            self.trim_samples_decimated = 0
        self.log_norm_channels_config = {"fhr_st": "all_except_0"}
        self.asinh_norm_channels_config = {"fhr_ph": "all", "fhr_up_ph": "all"}
        self.accumulator = None

    def _kinds(self, field, C):
        k = np.zeros(C, np.int32)
        a = self.asinh_norm_channels_config.get(field, [])
        k[list(range(C)) if a == "all" else list(a)] = KIND_ASINH
        lg = self.log_norm_channels_config.get(field, [])
        k[list(range(1, C)) if lg == "all_except_0" else list(lg)] = KIND_LOG   # log takes precedence
        return k

    def _h5_batches(self, paths, batch_size):
        import h5py
        for path in paths:
            with h5py.File(path, "r") as f:
                n = f[self.stats_fields[0]].shape[0]
                for a in range(0, n, batch_size):
                    yield {k: np.asarray(f[k][a:min(a + batch_size, n)]) for k in self.stats_fields if k in f}

    def calculate_stats(self, batches, batch_size=100, frontend=None, side=None):
        """batches: an iterable of feature dicts {field: (B, C, S) or (B, N)} (arrays or
        tensors, untrimmed, the reference's stored layout), of (B, 2, N) window batches (run
        through `frontend`; default the J=11, Q=4, T=16 front-end for that N), or the
        reference's list of HDF5 paths when h5py is importable."""
        import torch
        batches = list(batches) if isinstance(batches, (list, tuple)) else batches
        if isinstance(batches, list) and batches and all(isinstance(b, str) for b in batches):
            batches = self._h5_batches(batches, batch_size)
        acc, shapes = None, {}
        for b in batches:
            if isinstance(b, dict):
                if acc is None:
                    fields = {}
                    for k in self.stats_fields:
                        if k in b:
                            C = None if k in SINGLE_FIELDS else int(b[k].shape[1])
                            fields[k] = None if C is None else (C, self._kinds(k, C))
                            cut = self.trim_samples_raw if C is None else self.trim_samples_decimated
                            shapes[k] = tuple(b[k].shape[1:-1]) + (int(b[k].shape[-1]) - 2 * cut,)
                    acc = StatsAccumulator(fields, self.device, trim=self.trim_samples_decimated, step=16)
                for k in acc.fields:
                    acc.update(k, b[k])
            else:
                x = torch.as_tensor(b).to(device=self.device, dtype=torch.float32)
                if frontend is None:
                    from .frontend import FrontEnd, FrontEndPlan
                    frontend = FrontEnd(FrontEndPlan(11, 4, 16, x.shape[-1], device=self.device),
                                        trim=self.trim_samples_decimated)
                if acc is None:
                    fe = frontend
                    fields = default_fields(fe.C_st, fe.C_ph, fe.C_x)
                    for k, spec in fields.items():
                        if spec is not None:
                            fields[k] = (spec[0], self._kinds(k, spec[0]))
                    acc = StatsAccumulator(fields, self.device, trim=fe.trim, step=fe.plan.step)
                    for k, spec in fields.items():
                        shapes[k] = (fe.N_out,) if spec is None else (spec[0], fe.S_out)
                acc.update_windows(frontend, x, side)
        if acc is None:
            raise ValueError("No batches to compute statistics from")
        self.accumulator = acc
        flat, host, stats = acc.finalize(), acc.host_state(), {}
        for k, spec in acc.fields.items():
            cnt, s, q = host[k]
            st = {"mean": flat[k + "_mean"], "variance": flat[k + "_variance"], "shape": shapes[k]}
            if spec is None:
                st.update(count=int(cnt[0]), sum=float(s[0]), sum_squares=float(q[0]))
            else:
                kinds = spec[1]
                st.update(count=int(cnt.sum()), sum=s, sum_squares=q, channel_counts=cnt, n_channels=spec[0],
                          regular_channels=[int(c) for c in np.nonzero(kinds == KIND_REGULAR)[0]],
                          log_channels=[int(c) for c in np.nonzero(kinds == KIND_LOG)[0]],
                          asinh_channels=[int(c) for c in np.nonzero(kinds == KIND_ASINH)[0]], log_epsilon=1e-6)
            stats[k] = st
        return stats
