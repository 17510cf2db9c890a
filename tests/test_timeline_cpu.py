"""vaeteb.timeline without a GPU: the host tables (TimelineLayout, check_offsets, overlap_rows), the
float64 restatements the GPU tests use as expected values (tests/timeline_util.py) on hand cases and
against SeqVaeTeb.get_predictions on CPU tensors, and the three prototypes in the header."""
import numpy as np
import pytest
import torch

from timeline_util import masked_metrics_np, metrics64, overlap_mean_np, stitch_np, taper_weights


class _Plan:
    def __init__(self, N, S, step=16):
        self.N, self.S, self.step = N, S, step


class _FE:
    """The attributes of a FrontEnd that TimelineLayout.window_offsets reads."""

    def __init__(self, N, S, trim, step=16):
        self.plan, self.trim = _Plan(N, S, step), trim
        self.S_out, self.N_out = S - 2 * trim, N - 2 * trim * step


def test_layout_offsets_hand_cases():
    from vaeteb.timeline import TimelineLayout
    lay = TimelineLayout([5760 * 2, 5760], step=16)
    assert lay.step_base.tolist() == [0, 720, 1080] and lay.sample_base.tolist() == [0, 11520, 17280]
    rec, start = [0, 0, 0, 1], [0, 2880, 5760, 0]
    assert lay.step_offsets(rec, start, trim=30).tolist() == [30, 210, 390, 720 + 30]
    assert lay.sample_offsets(rec, start, trim=30).tolist() == [480, 3360, 6240, 11520 + 480]
    so, no = lay.window_offsets(rec, start, _FE(5760, 360, 30))
    assert so.tolist() == [30, 210, 390, 750] and no.tolist() == [480, 3360, 6240, 12000]
    # objects with a length, and a recording shorter than the window: it owns positions, no window
    class Rec:
        def __init__(self, L):
            self.L = L
    lay = TimelineLayout([Rec(5760), Rec(1500), Rec(5775)], step=16)
    assert lay.step_base.tolist() == [0, 360, 360 + 93, 360 + 93 + 360]
    assert lay.sample_base.tolist() == [0, 5760, 7260, 13035]
    assert lay.step_offsets([0, 2], [0, 0], trim=30).tolist() == [30, 483]
    assert lay.n_steps == 813 and lay.n_samples == 13035
    empty = lay.step_offsets([], [])
    assert empty.shape == (0,) and empty.dtype == np.int64


def test_layout_rejects_what_does_not_line_up():
    from vaeteb.timeline import TimelineLayout
    lay = TimelineLayout([11520, 5760])
    with pytest.raises(ValueError, match="multiple of 16"):
        lay.step_offsets([0, 0], [0, 2881])
    with pytest.raises(ValueError, match="multiple of 16"):
        lay.sample_offsets([0], [8])
    with pytest.raises(ValueError, match="line up"):
        lay.window_offsets([0], [0], _FE(5760, 359, 30))          # S * step != N
    with pytest.raises(ValueError):
        lay.window_offsets([0], [0], _FE(5760, 720, 30, step=8))  # another decimation
    with pytest.raises(ValueError):
        lay.step_offsets([2], [0])                                # no such recording
    with pytest.raises(ValueError, match="ascending"):
        lay.window_offsets([1, 0], [0, 0], _FE(5760, 360, 30))
    with pytest.raises(ValueError, match="leave the timeline"):
        lay.window_offsets([1], [2880], _FE(5760, 360, 30))       # runs past the last recording


def test_offsets_are_checked_before_any_launch():
    """No GPU here: a launch would fail differently; these raise from the host check."""
    from vaeteb.timeline import check_offsets, overlap_mean, stitch
    with pytest.raises(ValueError, match="ascending"):
        check_offsets([2, 0], 4, 6)
    with pytest.raises(ValueError, match="leave the timeline"):
        check_offsets([0, 3], 4, 6)
    with pytest.raises(ValueError, match="leave the timeline"):
        check_offsets([-1, 0], 4, 6)
    with pytest.raises(ValueError, match="lengths"):
        check_offsets([0, 2], 4, 6, lengths=[4, 5])
    with pytest.raises(ValueError, match="lengths"):
        check_offsets([0, 2], 4, 6, lengths=[4])
    off, ln = check_offsets([0, 3], 4, 6, lengths=[4, 3])          # the clipped last window fits
    assert off.dtype == np.int64 and ln.dtype == np.int32 and off.tolist() == [0, 3]
    assert check_offsets([1, 1, 2], 4, 6)[1] is None                # duplicates are legal
    vals = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="ascending"):
        stitch(vals, [2, 0], 6)
    with pytest.raises(ValueError, match="leave the timeline"):
        stitch(vals, [0, 3], 6)
    with pytest.raises(ValueError, match="device"):
        stitch(vals, [0, 2], 6)                                     # valid tables, host tensor
    with pytest.raises(ValueError, match="device"):
        overlap_mean(torch.zeros(2, 5, 7))


def test_overlap_rows_tables():
    from vaeteb.timeline import overlap_rows
    kept, off, ln = overlap_rows(5, 7, stride=2, new_C=12)          # the last rows are clipped
    assert kept == 5 and off.tolist() == [0, 2, 4, 6, 8] and ln.tolist() == [7, 7, 7, 6, 4]
    kept, off, ln = overlap_rows(5, 7, stride=3, new_C=8)           # rows 3 and 4 start at or past new_C
    assert kept == 3 and off.tolist() == [0, 3, 6] and ln.tolist() == [7, 5, 2]
    kept, off, ln = overlap_rows(300, 64, stride=16, new_C=4800)    # the product's shape: row 299 keeps 16
    assert kept == 300 and off[-1] == 4784 and ln[-1] == 16
    assert overlap_rows(4, 7, stride=0, new_C=5)[1].tolist() == [0, 0, 0, 0]


def test_restatement_hand_case_mean():
    a, b = np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([10.0, 20.0, 30.0, 40.0], np.float32)
    out, count, bound = stitch_np(np.stack([a, b]), [0, 2], None, 7)
    want = [a[0], a[1], (a[2] + b[0]) / 2, (a[3] + b[1]) / 2, b[2], b[3]]
    assert out[:6].tolist() == want and np.isnan(out[6])
    assert count.tolist() == [1, 1, 2, 2, 1, 1, 0]
    # (m + 3) 2^-24 sum w|v| / sum w
    assert bound[0] == 4 * 2.0 ** -24 * 1.0 and bound[2] == 5 * 2.0 ** -24 * 6.5 and bound[6] == 0
    # lengths clip a window, the inner axis is averaged
    out, count, _ = stitch_np(np.stack([a, b]), [0, 2], [4, 1], 6)
    assert out[:4].tolist() == [1.0, 2.0, 6.5, 4.0] and np.isnan(out[4:]).all() and count.tolist() == [1, 1, 2, 1, 0, 0]
    v3 = np.stack([np.stack([a, a + 2], -1), np.stack([b, b + 2], -1)])          # (2, 4, 2): means a + 1, b + 1
    out3, _, _ = stitch_np(v3, [0, 2], None, 6)
    assert out3.tolist() == [2.0, 3.0, 7.5, 13.0, 31.0, 41.0]


def test_restatement_hand_case_taper():
    assert taper_weights(4).tolist() == [1, 2, 2, 1] and taper_weights(5).tolist() == [1, 2, 3, 2, 1]
    assert taper_weights(1).tolist() == [1]
    a, b = np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([10.0, 20.0, 30.0, 40.0], np.float32)
    out, count, _ = stitch_np(np.stack([a, b]), [0, 2], None, 6, blend="taper")
    # position 2: a's weight 2, b's weight 1; position 3: a's 1, b's 2; single cover: the value itself
    assert out.tolist() == [1.0, 2.0, (2 * 3.0 + 10.0) / 3, (4.0 + 2 * 20.0) / 3, 30.0, 40.0]
    assert count.tolist() == [1, 1, 2, 2, 1, 1]
    # the ramp runs over the full n: a window clipped to 2 samples keeps weights 1, 2
    out, _, _ = stitch_np(np.stack([a, b]), [0, 1], [4, 2], 5, blend="taper")
    assert out[:4].tolist() == [1.0, (2 * 2.0 + 10.0) / 3, (2 * 3.0 + 2 * 20.0) / 4, 4.0] and np.isnan(out[4])


PAIRS = [(2, 12), (3, 8), (9, 40)]     # last rows clipped; rows dropped; stride > C leaves NaN gaps


@pytest.mark.parametrize("stride,new_C", PAIRS)
def test_restatement_equals_get_predictions(stride, new_C):
    from vaeteb.model import SeqVaeTeb
    from vaeteb.timeline import overlap_rows
    x = torch.randn(2, 5, 7, generator=torch.Generator().manual_seed(stride))
    want = SeqVaeTeb.get_predictions(x, stride, new_C)[1].numpy()
    out, count, bound = overlap_mean_np(x.numpy(), stride, new_C)
    assert out.shape == want.shape == (2, new_C)
    assert np.array_equal(np.isnan(out), np.isnan(want))
    cov = count > 0                                  # want is a float32 mean: the kernel's own bound serves
    assert (np.abs(out - want)[cov] <= bound[cov]).all()
    assert np.array_equal(count > 0, ~np.isnan(want))
    # the conditions the three pairs stand for
    kept, off, ln = overlap_rows(5, 7, stride, new_C)
    if (stride, new_C) == (2, 12):
        assert kept == 5 and ln.min() < 7 and not np.isnan(want).any()
    elif (stride, new_C) == (3, 8):
        assert kept < 5
    else:
        assert stride > 7 and np.isnan(want).any() and not np.isnan(want).all()
    assert (bound[count > 0] > 0).all()


def test_masked_metrics_restatement():
    rng = np.random.default_rng(3)
    y = rng.standard_normal(40).astype(np.float32)
    pr = (y + np.float32(0.7) * rng.standard_normal(40).astype(np.float32)).astype(np.float32)
    count = np.ones(40, np.int32)
    count[5:9] = 0            # a gap in recording 0
    count[30:] = 0            # recording 2 uncovered
    out = masked_metrics_np(y, pr, count, [0, 20, 30, 40, 40])
    cov = count[:20] > 0
    assert out[0, :4].tolist() == list(metrics64(y[:20][cov], pr[:20][cov])) and out[0, 4] == 16 / 20
    assert out[1, :4].tolist() == list(metrics64(y[20:30], pr[20:30])) and out[1, 4] == 1.0
    assert np.isnan(out[2, :4]).all() and out[2, 4] == 0 and np.isnan(out[3, :4]).all() and out[3, 4] == 0
    vaf, mse, snr, vu = metrics64(y[20:30], pr[20:30])
    res = (y[20:30] - pr[20:30]).astype(np.float64)
    assert mse == (res ** 2).mean() and vu == 1 - res.var() / y[20:30].astype(np.float64).var()
    assert metrics64(y[:1], pr[:1])[0] == 0.0 and metrics64(y[:4], y[:4])[2] == 100.0


def test_header_declares_the_timeline_entry_points():
    from vaeteb import _lib
    protos = _lib.parse_header()
    assert protos["vt_timeline_accumulate"] == ("int", ["float*", "int64_t", "int", "int", "int64_t*", "int*", "int",
                                                         "float*", "float*", "int*", "int64_t", "void*"])
    assert protos["vt_timeline_finish"] == ("int", ["float*", "float*", "int*", "int64_t", "float", "float", "float",
                                                     "float*", "void*"])
    assert protos["vt_timeline_metrics"] == ("int", ["float*", "float*", "int*", "int64_t*", "int64_t", "float*",
                                                      "void*"])


def test_argument_errors_before_device_work():
    from vaeteb import _lib
    for bad in (dict(n=0), dict(inner=0), dict(W=-1), dict(total=-1), dict(blend=2)):
        a = dict(W=1, n=4, inner=1, blend=0, total=8)
        a.update(bad)
        with pytest.raises(ValueError):
            _lib.call("vt_timeline_accumulate", None, a["W"], a["n"], a["inner"], None, None, a["blend"], None, None,
                      None, a["total"], None)
    assert _lib.call("vt_timeline_accumulate", None, 0, 4, 1, None, None, 0, None, None, None, 8, None) == 0   # W == 0
    with pytest.raises(ValueError):
        _lib.call("vt_timeline_accumulate", None, 1, 4, 1, None, None, 0, None, None, None, 8, None)           # null
    with pytest.raises(ValueError):
        _lib.call("vt_timeline_finish", None, None, None, -1, 0.0, 1.0, 0.0, None, None)
    assert _lib.call("vt_timeline_finish", None, None, None, 0, 0.0, 1.0, 0.0, None, None) == 0
    with pytest.raises(ValueError):
        _lib.call("vt_timeline_metrics", None, None, None, None, -1, None, None)
    assert _lib.call("vt_timeline_metrics", None, None, None, None, 0, None, None) == 0
