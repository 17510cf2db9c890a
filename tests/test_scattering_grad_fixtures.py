"""The Scattering1D gradient fixtures (tools/gen_golden_scat_grad.py; the
reference's kymatio torch frontend under torch autograd, fp64 and fp32): every
file loads, shapes agree, and the reference's own fp32 gradient is within 1e-6
per-sample rel-L2 of its fp64 gradient -- so the bound of
tests/test_gpu_scattering_grad.py is about our kernels, not about the fixture."""
import numpy as np
import pytest

CFGS = {  # cfg -> (J, Q, T, N, order, B)
    "a": (2, 1, 4, 64, 2, 3),
    "b": (3, 1, 8, 100, 1, 3),
    "c": (4, 4, 16, 256, 2, 3),
    "d": (6, 16, 64, 512, 2, 2),
    "e": (4, 1, 16, 12000, 2, 2),
}


def rowrel(a, b):
    """Per-sample relative L2 error of a against b over the last axis."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a - b) ** 2).sum(-1) / (b ** 2).sum(-1))


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_fixture(golden, cfg):
    J, Q, T, N, order, B = CFGS[cfg]
    d = golden("scat_grad_" + cfg)
    x, w, S64, g64, g32 = d["x"], d["w"], d["S64"], d["g64"], d["g32"]
    assert x.dtype == np.float32 and w.dtype == np.float32 and g64.dtype == np.float64 and g32.dtype == np.float32
    assert x.shape == (B, N) and g64.shape == x.shape and g32.shape == x.shape
    assert S64.ndim == 3 and S64.shape[0] == B and w.shape == S64.shape
    assert np.isfinite(g64).all() and np.isfinite(g32).all()
    r = rowrel(g32, g64)
    assert r.max() < 1e-6, r
    if cfg == "a":   # the zero row: every modulus is 0 there, the gradient flows through order 0 only
        assert not x[0].any() and np.abs(g64[0]).max() > 0
    if cfg == "d":
        assert d["x0"].shape == x.shape and d["gq64"].shape == x.shape and d["gq32"].shape == x.shape
        rq = rowrel(d["gq32"], d["gq64"])
        assert rq.max() < 1e-6, rq


def test_paths_match_bank():
    """The fixtures' channel counts are those of the project's own filter bank."""
    from vaeteb.filter_bank import build_bank, padding
    import os
    for cfg, (J, Q, T, N, order, B) in CFGS.items():
        pd = padding(N, J, Q, T)
        b = build_bank(pd.J_pad, J, Q, T)
        C = 1 + len(b.xi1)
        if order == 2:
            C += sum(int(j2) > int(j1) for j1 in b.j1 for j2 in b.j2)
        S64 = np.load(os.path.join(os.path.dirname(__file__), "golden", f"scat_grad_{cfg}.npz"))["S64"]
        assert S64.shape[1] == C, (cfg, S64.shape, C)
