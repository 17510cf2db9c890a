#!/usr/bin/env python3
"""Generate tests/golden/stats_accum_b5.npz from the REFERENCE statistics code (build
container only; see tools/gen_golden.py for the mechanism).

The reference's calculator module imports h5py, so the definitions of _initialize_stats,
_update_single_channel_stats, _update_multi_channel_stats and _finalize_stats
(ref/hdf5_dataset/calculate_dataset_stats.py:62-273) are extracted with `ast` and executed
unchanged on small seeded inputs, trimmed the way calculate_stats trims them (:343-351), in
two updates (windows 0-2, then 3-4).  The fixture holds the inputs and the reference's fp64
channel_counts / sum / sum_squares and final mean / variance — data only.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_stats.py
"""
import os
import sys
import types
import typing
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, extract_functions, save  # noqa: E402

TRIM_MINUTES = 0.2
SHAPES = {"fhr_st": (5, 43, 24), "fhr_ph": (5, 44, 24), "fhr_up_ph": (5, 130, 24), "fhr": (5, 384), "up": (5, 384)}
DEAD_PH_CHANNEL = 7          # fhr_ph channel that is NaN throughout: count 0
NEG_LOG_CHANNELS = (5, 17)   # fhr_st log channels with negative entries: clamp to 0 -> log(1e-6), counted


def make_inputs(seed=20240611):
    rng = np.random.default_rng(seed)
    x = {}
    x["fhr_st"] = 10.0 ** rng.uniform(-9, 2, SHAPES["fhr_st"])
    for c in NEG_LOG_CHANNELS:
        neg = rng.random(SHAPES["fhr_st"][::2]) < 0.3
        x["fhr_st"][:, c][neg] *= -1.0
    for f in ("fhr_ph", "fhr_up_ph"):
        x[f] = rng.choice([-1.0, 1.0], SHAPES[f]) * 10.0 ** rng.uniform(-6, 3, SHAPES[f])
    x["fhr"] = 140.0 + 20.0 * rng.standard_normal(SHAPES["fhr"])
    x["up"] = 30.0 + 15.0 * rng.standard_normal(SHAPES["up"])
    for f in x:   # non-finite entries in every field
        u = rng.random(x[f].shape)
        x[f][u < 0.02] = np.nan
        x[f][(u >= 0.02) & (u < 0.03)] = np.inf
        x[f][(u >= 0.03) & (u < 0.04)] = -np.inf
    x["fhr_ph"][:, DEAD_PH_CHANNEL] = np.nan
    return {f: v.astype(np.float32) for f, v in x.items()}


def main():
    fn = extract_functions(os.path.join(REF, "hdf5_dataset/calculate_dataset_stats.py"),
                           ["_initialize_stats", "_update_single_channel_stats", "_update_multi_channel_stats",
                            "_finalize_stats"],
                           {"torch": torch, "np": np, "warnings": warnings, **vars(typing)})
    raw_cut = int(4 * 60 * TRIM_MINUTES)
    dec_cut = raw_cut // 16
    assert (raw_cut, dec_cut) == (48, 3)
    self_ = types.SimpleNamespace(device="cpu", stats_fields=["fhr", "up", "fhr_st", "fhr_ph", "fhr_up_ph"],
                                  log_norm_channels_config={"fhr_st": "all_except_0"},
                                  asinh_norm_channels_config={"fhr_ph": "all", "fhr_up_ph": "all"})
    x = make_inputs()
    cut = {f: raw_cut if f in ("fhr", "up") else dec_cut for f in x}
    trimmed = {f: v[..., cut[f]:v.shape[-1] - cut[f]] for f, v in x.items()}
    stats = fn["_initialize_stats"](self_, {f: v.shape[1:] for f, v in trimmed.items()})
    for lo, hi in ((0, 3), (3, 5)):
        for f in self_.stats_fields:
            upd = "_update_single_channel_stats" if f in ("fhr", "up") else "_update_multi_channel_stats"
            fn[upd](self_, stats[f], trimmed[f][lo:hi])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fn["_finalize_stats"](self_, stats)

    out = {"trim_minutes": np.float64(TRIM_MINUTES)}
    for f, st in stats.items():
        single = f in ("fhr", "up")
        cnt = np.asarray([st["count"]], np.int64) if single else st["channel_counts"].numpy()
        mean = np.asarray(st["mean"], np.float64 if single else np.float32).reshape(-1)
        var = np.asarray(st["variance"], np.float64 if single else np.float32).reshape(-1)
        assert not np.isfinite(trimmed[f]).all() and np.isnan(trimmed[f]).any() and np.isposinf(trimmed[f]).any() \
            and np.isneginf(trimmed[f]).any(), f
        live = cnt > 0
        ratio = (mean[live].astype(np.float64) ** 2 / var[live]).max()
        assert ratio <= 100, (f, ratio)   # the E[t^2] - mean^2 cancellation stays benign
        print(f"{f}: counts {cnt.min()}..{cnt.max()}, max mean^2/variance {ratio:.3g}")
        out.update({f"in_{f}": x[f], f"ref_{f}_count": cnt,
                    f"ref_{f}_sum": st["sum"].numpy().astype(np.float64).reshape(-1),
                    f"ref_{f}_sum_squares": st["sum_squares"].numpy().astype(np.float64).reshape(-1),
                    f"ref_{f}_mean": mean, f"ref_{f}_variance": var})
    assert out["ref_fhr_ph_count"][DEAD_PH_CHANNEL] == 0
    for c in NEG_LOG_CHANNELS:
        assert (trimmed["fhr_st"][:, c] < 0).any()
    save("stats_accum_b5.npz", **out)


if __name__ == "__main__":
    main()
