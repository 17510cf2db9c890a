#!/usr/bin/env python3
"""Time the signal-dropout gate of vaeteb.windows for a batch of recordings on the device
against the reference's host loop, in the same run.

Device: one vt_window_flat_stats launch over every (window, channel) row of every recording
plus the QualityGate thresholds, recordings already packed in HBM (device events around
`--reps` repetitions after a warm-up), and separately the whole RecordingWindows
construction (packing upload + launch + gate + the kept list back on the host).
Host: the loop of find_flat_regions (ref/hdf5_dataset/create_hdf5_dataset.py:46-81) restated
here over numpy float32 samples, one interpreter iteration per sample, followed by the length
arithmetic of :462-472 — timed on the first `--host-windows` windows (both channels) and
reported per window; its results are compared with the kernel's on those windows.

Reported, not gated.  Usage:  python tools/windows_micro.py [--recordings 64] [--length 57600]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vae-teb_amd"))
from vaeteb import _lib, synthetic  # noqa: E402
from vaeteb.windows import QualityGate, Recording, RecordingWindows  # noqa: E402


def host_flat_stats(signal, tolerance=1e-9, min_length=20):
    """The reference's per-sample loop, then (max, total, count) of the region lengths."""
    lengths, start = [], None
    for i in range(1, len(signal)):
        if abs(signal[i] - signal[i - 1]) <= tolerance:
            if start is None:
                start = i - 1
        elif start is not None:
            if i - start >= min_length:
                lengths.append(i - start)
            start = None
    if start is not None and len(signal) - start >= min_length:
        lengths.append(len(signal) - start)
    return max(lengths, default=0), sum(lengths), len(lengths)


def recordings(count, length, n=5760):
    """Synthetic recordings (windows of vaeteb.synthetic laid end to end) with dropouts."""
    rng = np.random.default_rng(0)
    per = -(-length // n)
    out = []
    for r in range(count):
        x = np.concatenate(list(synthetic.batch(r * per, per, n)), axis=-1)[:, :length].copy()
        for _ in range(int(rng.integers(0, 4))):
            a, m = int(rng.integers(0, length - 1500)), int(rng.integers(20, 1500))
            ch = int(rng.integers(0, 2))
            x[ch, a:a + m] = x[ch, a]
        out.append(Recording(x, f"rec_{r}"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--length", type=int, default=57600, help="samples per recording (57600 = 4 h at 4 Hz)")
    ap.add_argument("--window", type=int, default=5760)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-windows", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    recs = recordings(a.recordings, a.length, a.window)
    gate = QualityGate()

    t0 = time.perf_counter()
    rw = RecordingWindows(recs, N=a.window, overlap=0.5, gate=gate)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rw = RecordingWindows(recs, N=a.window, overlap=0.5, gate=gate)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3

    W = rw.n_windows
    off, out = rw.row_off.reshape(-1), torch.empty((2 * W, 3), dtype=torch.int32, device=rw.device)

    def run():   # the launch + the thresholds, no host read in between
        _lib.call("vt_window_flat_stats", _lib.ptr(rw.buffer), _lib.ptr(off), 2 * W, a.window, gate.tolerance,
                  gate.min_length, _lib.ptr(out), _lib.stream())
        return gate(out.view(W, 2, 3), rw.weight_mean)

    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        res = run()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.reps

    hw = min(a.host_windows, W)
    rows = [(w, c) for w in range(hw) for c in (0, 1)]
    sig = [recs[rw.rec[w]].x[c, rw.start[w]:rw.start[w] + a.window].numpy() for w, c in rows]
    t0 = time.perf_counter()
    host = [host_flat_stats(s, gate.tolerance, gate.min_length) for s in sig]
    host_ms_per_window = (time.perf_counter() - t0) * 1e3 / hw
    got = rw.stats.cpu().numpy()[:hw].reshape(-1, 3)
    assert (got == np.array(host)).all(), "kernel and host loop disagree"
    assert torch.equal(res.keep, rw.result.keep)

    print(json.dumps({
        "recordings": a.recordings, "length": a.length, "window": a.window, "overlap": 0.5, "windows": W,
        "rows": 2 * W, "kept": rw.report["kept"],
        "device_gate_ms": round(dev_ms, 4), "device_gate_us_per_window": round(dev_ms * 1e3 / W, 4),
        "device_gate_read_GBps": round(2 * W * a.window * 4 / (dev_ms * 1e-3) / 1e9, 1),
        "recording_windows_build_ms": round(build_ms, 3), "recording_windows_first_build_ms": round(first_ms, 3),
        "host_loop_ms_per_window": round(host_ms_per_window, 3), "host_loop_windows_timed": hw,
        "host_loop_ms_all_windows_extrapolated": round(host_ms_per_window * W, 1),
        "host_over_device": round(host_ms_per_window * W / dev_ms, 1)}))


if __name__ == "__main__":
    main()
