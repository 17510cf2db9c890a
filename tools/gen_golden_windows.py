#!/usr/bin/env python3
"""Generate tests/golden/flat_regions_cases.npz from the REFERENCE's own find_flat_regions
(ref/hdf5_dataset/create_hdf5_dataset.py:46-81; build container only, as tools/gen_golden.py,
whose helpers it uses).

The reference module's imports (early_maestra, h5py, sklearn, ...) are absent, so the function
definition is taken from the file's source with `ast` at generation time and executed
unchanged; nothing of it is stored.  For every signal and every (tolerance, min_length) the
fixture holds what the gate derives from the function's regions (:466-472): the longest
length, the total length and the number of regions.

Signals: float32, values multiples of 0.25 (so no difference lies near either tolerance),
with planted constant segments (also at the first and the last sample and across the
multiples of 64), near-constant segments that step by 2^-11 (flat at tolerance 1e-3, not at
1e-9; exact in float32 at these magnitudes), and NaN / +-inf inside constant segments
(two infinities side by side give inf - inf = NaN: not flat).  ~40 signals of lengths 1..300
plus one of 5760 with dropouts around the gate's thresholds.

Stored (data only): signals (n, 5760) zero-padded, lengths (n,), tolerance (P,),
min_length (P,), expected (n, P, 3) = {max, total, count}.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_windows.py
"""
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (reference paths, extract_functions, save)

NAME = "flat_regions_cases.npz"
LENGTHS = [1, 2, 3, 4, 19, 20, 21, 22, 40, 62, 63, 64, 65, 66, 83, 100, 126, 127, 128, 129, 130, 150, 171, 190, 191,
           192, 193, 194, 200, 222, 233, 250, 255, 256, 257, 258, 270, 287, 299, 300]
PARAMS = [(tol, ml) for tol in (1e-9, 1e-3) for ml in (1, 3, 20)]
LMAX = 5760


def plant(x, rng, a, n, kind):
    """A segment of n samples from a: 'const', 'ramp' (steps of 2^-11) or a constant segment
    with a NaN / inf / inf pair inside."""
    n = max(1, min(n, len(x) - a))
    v = np.float32(rng.integers(400, 720) * 0.25)
    x[a:a + n] = v
    if kind == "ramp":
        x[a:a + n] = v + np.arange(n, dtype=np.float32) * np.float32(2.0 ** -11)
    elif kind in ("nan", "inf", "infpair") and n >= 3:
        k = a + int(rng.integers(1, n - 1))
        if kind == "nan":
            x[k] = np.nan
        elif kind == "inf":
            x[k] = np.inf if rng.integers(2) else -np.inf
        else:
            x[k:min(k + 2, a + n)] = np.inf


def signal(L, rng, segments):
    x = (rng.integers(400, 720, size=L) * 0.25).astype(np.float32)
    for a, n, kind in segments:
        if a < L:
            plant(x, rng, a, n, kind)
    return x


def short_signal(L, rng):
    kinds = ["const", "const", "ramp", "nan", "inf", "infpair"]
    segs = []
    for _ in range(int(rng.integers(1, 5))):
        segs.append((int(rng.integers(0, max(1, L))), int(rng.integers(2, 70)), kinds[int(rng.integers(len(kinds)))]))
    if L >= 4 and rng.integers(2):
        n = int(rng.integers(2, min(L, 40)))
        segs.append((L - n, n, "const"))            # a run that ends at the last sample
    if L >= 4 and rng.integers(3) == 0:
        segs.append((0, int(rng.integers(2, min(L, 40))), "const"))   # and one that starts at the first
    if L > 70 and rng.integers(2):
        segs.append((60, 11, "const"))              # samples 60..70: across the first tile boundary
    return signal(L, rng, segs)


def main():
    fn = G.extract_functions(os.path.join(G.REF, "hdf5_dataset/create_hdf5_dataset.py"), ["find_flat_regions"],
                             {})["find_flat_regions"]
    rng = np.random.Generator(np.random.PCG64(20251020))
    sigs = [short_signal(L, rng) for L in LENGTHS]
    sigs.append(signal(LMAX, rng, [(0, 19, "const"), (100, 20, "const"), (200, 480, "const"), (1000, 481, "const"),
                                   (1600, 1201, "const"), (3000, 300, "ramp"), (3500, 640, "nan"),
                                   (4300, 200, "infpair"), (4600, 64, "const"), (4700, 65, "inf"),
                                   (LMAX - 700, 700, "const")]))
    n = len(sigs)
    padded = np.zeros((n, LMAX), np.float32)
    lengths = np.array([len(s) for s in sigs], np.int32)
    expected = np.zeros((n, len(PARAMS), 3), np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # inf - inf inside the reference loop
        for i, s in enumerate(sigs):
            padded[i, :len(s)] = s
            for p, (tol, ml) in enumerate(PARAMS):
                lens = [e - a + 1 for a, e in fn(s, tolerance=tol, min_length=ml)]
                expected[i, p] = (max(lens, default=0), sum(lens), len(lens))
    G.save(NAME, signals=padded, lengths=lengths, tolerance=np.array([t for t, _ in PARAMS], np.float64),
           min_length=np.array([m for _, m in PARAMS], np.int32), expected=expected)
    assert os.path.getsize(os.path.join(G.OUT, NAME)) < 200_000
    print("cases:", n * len(PARAMS), "non-trivial:", int((expected[:, :, 2] > 0).sum()),
          "tolerance matters in:", int((expected[:, 0] != expected[:, 3]).any(-1).sum()), "signals")


if __name__ == "__main__":
    main()
