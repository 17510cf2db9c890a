"""Dataset statistics, host side: the finalisation formula against the reference fixture
(tests/golden/stats_accum_b5.npz, tools/gen_golden_stats.py), the calculator facade's trim
attributes, and the argument validation of the vt_stats_* entry points (no GPU needed:
validation precedes any device work)."""
import ctypes

import numpy as np
import pytest

from vaeteb import _lib
from vaeteb.stats import DatasetStatsCalculator, channel_kinds, finalize_state

MULTI = ("fhr_st", "fhr_ph", "fhr_up_ph")
SINGLE = ("fhr", "up")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("stats_accum_b5")


@pytest.mark.parametrize("field", MULTI)
def test_finalize_multi_channel_bit_equal(fx, field):
    mean, var = finalize_state(fx[f"ref_{field}_count"], fx[f"ref_{field}_sum"], fx[f"ref_{field}_sum_squares"])
    assert mean.dtype == np.float32 and var.dtype == np.float32
    assert np.array_equal(mean.view(np.int32), fx[f"ref_{field}_mean"].view(np.int32))
    assert np.array_equal(var.view(np.int32), fx[f"ref_{field}_variance"].view(np.int32))


@pytest.mark.parametrize("field", SINGLE)
def test_finalize_single_channel(fx, field):
    mean, var = finalize_state(fx[f"ref_{field}_count"], fx[f"ref_{field}_sum"], fx[f"ref_{field}_sum_squares"],
                               single=True)
    assert isinstance(mean, float) and isinstance(var, float)
    assert mean == float(fx[f"ref_{field}_mean"][0]) and var == float(fx[f"ref_{field}_variance"][0])


def test_finalize_empty_channel_and_variance_clamp(fx):
    cnt = fx["ref_fhr_ph_count"]
    dead = np.nonzero(cnt == 0)[0]
    assert dead.size == 1   # the fixture's all-NaN channel
    mean, var = finalize_state(cnt, fx["ref_fhr_ph_sum"], fx["ref_fhr_ph_sum_squares"])
    assert mean[dead[0]] == 0 and var[dead[0]] == 0
    # sum_sq / n - mean^2 slightly negative by rounding: clamped to 0, the mean kept
    mean, var = finalize_state([4, 0, 2], [8.0, 0.0, 2.0], [16.0 - 1e-9, 0.0, 10.0])
    assert mean.tolist() == [2.0, 0.0, 1.0] and var.tolist() == [0.0, 0.0, 4.0]
    assert finalize_state([4], [8.0], [16.0 - 1e-9], single=True) == (2.0, 0.0)
    assert finalize_state([0], [0.0], [0.0], single=True) == (0.0, 0.0)


def test_calculator_has_the_reference_trim_attributes():
    c = DatasetStatsCalculator(trim_minutes=0.2, device="cpu")
    assert c.stats_fields == ["fhr", "up", "fhr_st", "fhr_ph", "fhr_up_ph"]
    assert c.trim_samples_raw == 48 and c.trim_samples_decimated == 3
    assert c.log_norm_channels_config == {"fhr_st": "all_except_0"}
    assert c.asinh_norm_channels_config == {"fhr_ph": "all", "fhr_up_ph": "all"}
    assert c._kinds("fhr_st", 43).tolist() == channel_kinds("fhr_st", 43).tolist() == [0] + [1] * 42
    assert c._kinds("fhr_ph", 44).tolist() == [2] * 44
    c = DatasetStatsCalculator()
    assert c.trim_samples_raw == 0 and c.trim_samples_decimated == 0
    c = DatasetStatsCalculator(trim_minutes=2)
    assert c.trim_samples_raw == 480 and c.trim_samples_decimated == 30


def test_all_reduce_packs_and_unpacks_the_whole_state(tmp_path):
    """One rank (gloo): the SUM all-reduce of the packed state must give the state back — counts
    exact through their fp64 transport, sums bit for bit, window counts kept."""
    import torch
    import torch.distributed as dist
    from vaeteb.stats import StatsAccumulator
    acc = StatsAccumulator({"fhr": None, "fhr_st": (3, channel_kinds("fhr_st", 3))}, "cpu")
    acc._count += torch.tensor([2 ** 40 + 1, 7, 0, 90])
    acc._sums += torch.tensor([[1.0 / 3, -2.5e-7, 0.0, 1e300], [1e-300, 3.0, 0.0, 2.0 / 3]], dtype=torch.float64)
    acc.windows.update(fhr=11, fhr_st=12)
    cnt, sums = acc._count.clone(), acc._sums.clone()
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        acc.all_reduce()
    finally:
        if own:
            dist.destroy_process_group()
    assert torch.equal(acc._count, cnt) and torch.equal(acc._sums.view(torch.int64), sums.view(torch.int64))
    assert acc.windows == {"fhr": 11, "fhr_st": 12} and acc.n_windows == 12
    other = StatsAccumulator({"fhr": None, "fhr_st": (3, channel_kinds("fhr_st", 3))}, "cpu")
    other.merge(acc).merge(acc)
    assert torch.equal(other._count, 2 * cnt) and torch.equal(other._sums, 2 * sums) and other.n_windows == 24
    with pytest.raises(ValueError):
        other.merge(StatsAccumulator({"fhr": None}, "cpu"))


def test_workspace_query_follows_the_chunking():
    r, c = ctypes.c_int(), ctypes.c_int()
    _lib.call("vt_stats_chunking", ctypes.byref(r), ctypes.byref(c))
    rows, cols = r.value, c.value
    assert rows > 0 and cols > 0
    n = ctypes.c_int64()
    for B, C, S in ((1, 1, 1), (rows, 7, cols), (rows + 1, 7, cols), (rows, 7, cols + 1), (3 * rows, 130, 18)):
        _lib.call("vt_stats_workspace_bytes", B, C, S, ctypes.byref(n))
        assert n.value == 24 * C * (-(-B // rows)) * (-(-S // cols))
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            _lib.call("vt_stats_workspace_bytes", *bad, ctypes.byref(n))
    with pytest.raises(ValueError):
        _lib.call("vt_stats_workspace_bytes", 1 << 40, 1 << 20, 1, ctypes.byref(n))   # more than one grid


def test_accum_rejects_bad_arguments_before_device_work():
    # never dereferenced: every call below fails validation
    p = 4096
    ok = dict(B=2, C=3, in_C=5, in_S=24, s0=3, S_len=18)

    def accum(work_bytes=1 << 20, in_=p, count=p, sum_=p, sq=p, work=p, log_eps=1e-6, **kw):
        a = dict(ok, **kw)
        _lib.call("vt_stats_accum", in_, a["B"], a["C"], a["in_C"], a["in_S"], a["s0"], a["S_len"], None, log_eps,
                  count, sum_, sq, work, work_bytes, None)

    for kw in (dict(B=0), dict(C=0), dict(S_len=0), dict(in_C=2), dict(s0=-1), dict(s0=7), dict(S_len=22),
               dict(in_=None), dict(count=None), dict(sum_=None), dict(sq=None), dict(work=None),
               dict(work_bytes=24 * 3 - 1), dict(work=p + 4), dict(log_eps=-1.0)):
        with pytest.raises(ValueError):
            accum(**kw)
    for args in ((p, 0, 8192, 4096), (p, 2, 8192, 0), (p, 2, 100, 101), (None, 2, 8192, 4096)):
        with pytest.raises(ValueError):
            _lib.call("vt_stats_accum_raw", *args, p, p, p, p, 1 << 20, None)
    with pytest.raises(ValueError):
        _lib.call("vt_stats_accum_raw", p, 2, 8192, 4096, p, p, p, p, 24 * 4 - 1, None)   # 4 column chunks
