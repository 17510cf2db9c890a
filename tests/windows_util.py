"""Shared by tests/test_windows_cpu.py and tests/test_gpu_windows.py: a numpy run-length
restatement of the reference's flat-region statistics (find_flat_regions,
ref/hdf5_dataset/create_hdf5_dataset.py:46-81, + the length arithmetic of :462-472).  The CPU
test pins it to the reference's recorded results (tests/golden/flat_regions_cases.npz); the GPU
tests then use it as the expected value for shapes the fixture does not hold."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_regions_cases.npz")


def flat_stats_np(x, tolerance=1e-9, min_length=20):
    """(longest, total, count) of the flat regions of >= min_length samples of the 1-D signal x.
    The fp32 difference is compared with the double tolerance."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        flat = np.abs(x[1:] - x[:-1]).astype(np.float64) <= tolerance      # NaN, inf - inf: not flat
    edge = np.diff(np.concatenate([[0], flat.astype(np.int8), [0]]))
    first, last = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]      # diff indices [first, last)
    lens = last - first + 1                                                # m flat diffs = m + 1 samples
    lens = lens[lens >= min_length]
    return (int(lens.max()) if lens.size else 0, int(lens.sum()), int(lens.size))


def fixture_cases():
    """[(signal, tolerance, min_length, expected (3,))] of the reference fixture."""
    g = np.load(FIXTURE, allow_pickle=False)
    out = []
    for i, L in enumerate(g["lengths"]):
        for p, (tol, ml) in enumerate(zip(g["tolerance"], g["min_length"])):
            out.append((g["signals"][i, :L], float(tol), int(ml), g["expected"][i, p]))
    return out
