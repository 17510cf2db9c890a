"""vaeteb.windows without a device: window placement, the reference fixture of the flat-region
gate against the tests' numpy restatement, argument validation of the two entry points and
their export (no GPU needed: nothing here launches a kernel)."""
import ctypes

import numpy as np
import pytest

from vaeteb import _lib
from vaeteb.windows import QualityGate, Recording, window_starts
from windows_util import fixture_cases, flat_stats_np


def test_window_starts():
    assert window_starts(10, 4, 0.5, "drop").tolist() == [0, 2, 4, 6]
    assert window_starts(10, 4, 0.5, "align").tolist() == [0, 2, 4, 6]
    assert window_starts(11, 4, 0.5, "drop").tolist() == [0, 2, 4, 6]
    assert window_starts(11, 4, 0.5, "align").tolist() == [0, 2, 4, 6, 7]
    for tail in ("drop", "align"):
        s = window_starts(3, 4, 0.5, tail)
        assert s.shape == (0,) and s.dtype == np.int64
    assert window_starts(12, 4, 0.0).tolist() == [0, 4, 8]                 # overlap 0: hop N
    assert window_starts(4, 4).tolist() == [0]
    assert window_starts(5760 * 2, 5760).tolist() == [0, 2880, 5760]
    assert window_starts(10, 5, 0.5).tolist() == [0, 3]                    # hop = 5 - int(2.5) = 3
    assert window_starts(10, 5, 0.5, "align").tolist() == [0, 3, 5]


def test_window_starts_rejects_bad_arguments():
    with pytest.raises(ValueError):
        window_starts(10, 4, 1.0)          # hop 0
    with pytest.raises(ValueError):
        window_starts(10, 0)
    with pytest.raises(ValueError):
        window_starts(10, 4, tail="pad")


def test_restatement_equals_reference_fixture():
    cases = fixture_cases()
    assert len(cases) >= 240
    lengths = {len(s) for s, *_ in cases}
    assert {1, 2, 63, 64, 65, 5760} <= lengths
    assert any(np.isnan(s).any() for s, *_ in cases) and any(np.isinf(s).any() for s, *_ in cases)
    bad = [(len(s), tol, ml, flat_stats_np(s, tol, ml), tuple(e)) for s, tol, ml, e in cases
           if flat_stats_np(s, tol, ml) != tuple(int(v) for v in e)]
    assert not bad, bad[:5]
    # the fixture exercises the parameters: some signal separates the tolerances, some the min_lengths
    by = {}
    for s, tol, ml, e in cases:
        by.setdefault(s.tobytes(), {})[(tol, ml)] = tuple(int(v) for v in e)
    assert any(v[(1e-9, 20)] != v[(1e-3, 20)] for v in by.values())
    assert any(v[(1e-9, 3)] != v[(1e-9, 20)] for v in by.values())
    assert all(v[(1e-9, 1)][0] >= v[(1e-9, 3)][0] for v in by.values())


def test_restatement_small_cases():
    assert flat_stats_np([1.0], 1e-9, 1) == (0, 0, 0)
    assert flat_stats_np([1.0, 1.0], 1e-9, 2) == (2, 2, 1)
    assert flat_stats_np([1.0, 1.0], 1e-9, 3) == (0, 0, 0)
    assert flat_stats_np([1, 1, 2, 3, 3, 3], 1e-9, 1) == (3, 5, 2)
    assert flat_stats_np([1, 1, np.nan, np.nan, 1, 1], 1e-9, 1) == (2, 4, 2)
    assert flat_stats_np([np.inf, np.inf, np.inf], 1e-9, 1) == (0, 0, 0)


def test_argument_errors_map_to_value_error():
    # validated before any device work, so this is safe without a GPU (as tests/test_abi.py)
    with pytest.raises(ValueError):
        _lib.call("vt_window_flat_stats", None, None, 0, 0, 1e-9, 20, None, None)        # N = 0
    with pytest.raises(ValueError):
        _lib.call("vt_window_flat_stats", None, None, 0, 64, 1e-9, 0, None, None)        # min_length = 0
    with pytest.raises(ValueError):
        _lib.call("vt_window_flat_stats", None, None, -1, 64, 1e-9, 20, None, None)      # rows < 0
    with pytest.raises(ValueError):
        _lib.call("vt_window_flat_stats", None, None, 3, 64, 1e-9, 20, None, None)       # null with rows > 0
    with pytest.raises(ValueError):
        _lib.call("vt_window_gather", None, None, 0, 0, None, None)                      # N = 0
    with pytest.raises(ValueError):
        _lib.call("vt_window_gather", None, None, -1, 64, None, None)
    with pytest.raises(ValueError):
        _lib.call("vt_window_gather", None, None, 2, 64, None, None)
    # rows == 0 is a no-op, not an error
    assert _lib.call("vt_window_flat_stats", None, None, 0, 64, 1e-9, 20, None, None) == 0
    assert _lib.call("vt_window_gather", None, None, 0, 64, None, None) == 0


def test_symbols_exported():
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("vt_window_flat_stats", 8), ("vt_window_gather", 6)):
        assert name in protos and len(protos[name][1]) == nargs
        assert hasattr(dll, name)
        assert name in _lib.lib().fns


def test_recording_and_gate_validate_on_the_host():
    r = Recording(np.zeros((2, 64), np.float32), "a", weight=np.ones(4), target=2.0)
    assert r.L == 64 and r.target.shape == (4,) and r.target.dtype == np.float32 and r.weight.dtype == np.float32
    with pytest.raises(ValueError):
        Recording(np.zeros((3, 64), np.float32), "a")
    with pytest.raises(ValueError):
        Recording(np.zeros((2, 64), np.float32), "a", weight=np.ones(5))
    g = QualityGate()
    assert (g.max_flat_fhr, g.max_flat_up, g.total_flat_fhr, g.total_flat_up) == (480, 1200, 1200, 1200)
    assert (g.min_weight, g.tolerance, g.min_length) == (0.90, 1e-9, 20)
