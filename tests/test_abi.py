"""The C-ABI library loads on the host and exports every symbol declared in
include/vaeteb.h (no GPU needed: no compute calls here)."""
import ctypes
import os

from vaeteb import _lib


def test_header_parses_and_all_symbols_exported():
    protos = _lib.parse_header()
    assert len(protos) >= 20
    dll = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in protos if not hasattr(dll, n)]
    assert not missing, missing


def test_bound_library_reports_version_and_errors():
    lib = _lib.lib()
    assert lib.fns["vt_abi_version"]() >= 1
    assert isinstance(lib.last_error(), str)


def test_argument_errors_map_to_value_error():
    import pytest
    # shape validation happens before any device work, so this is safe without a GPU
    with pytest.raises(ValueError):
        _lib.call("vt_fe_spectrum", None, 0, 4096, 8192, 2048, 0, None, None, None)
    with pytest.raises(ValueError):
        _lib.call("vt_fft", None, None, 1, 12, 0, None, 1, None)   # not a power of two


def test_library_is_in_tree():
    assert os.path.commonpath([_lib.LIB_PATH, os.path.dirname(os.path.dirname(__file__))])


def test_documented_switches_are_read_by_the_package():
    """Every VAETEB_* name that INTEGRATION.md, include/vaeteb.h or a file under tools/ mentions is
    read somewhere in the package's sources (a .hip / .cpp / .h / .py file under vae-teb_amd/), so
    that documents and tools cannot go on naming a switch that no longer exists.  The header's own
    include guard is no switch."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = re.compile(r"VAETEB_[A-Z0-9_]+")
    header = open(os.path.join(root, "include", "vaeteb.h")).read()
    guards = set(re.findall(r"^#\s*(?:ifndef|define)\s+(VAETEB_[A-Z0-9_]+)\s*$", header, re.M))
    docs = [os.path.join(root, "INTEGRATION.md"), os.path.join(root, "include", "vaeteb.h")]
    for d, _, files in os.walk(os.path.join(root, "tools")):
        docs += [os.path.join(d, f) for f in files]
    named = {}
    for path in docs:
        with open(path, errors="replace") as fh:
            for n in name.findall(fh.read()):
                named.setdefault(n, os.path.relpath(path, root))
    read = set()
    for d, _, files in os.walk(os.path.join(root, "vae-teb_amd")):
        for f in files:
            if f.endswith((".hip", ".cpp", ".h", ".py")):
                with open(os.path.join(d, f), errors="replace") as fh:
                    read.update(name.findall(fh.read()))
    stale = {n: where for n, where in named.items() if n not in read and n not in guards}
    assert len(named) >= 20 and read, (len(named), len(read))
    assert not stale, stale
