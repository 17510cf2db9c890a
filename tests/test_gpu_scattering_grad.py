"""Gradients through Scattering1D and the torch_hip plugin ops on the GPU
(csrc/scatter_bwd.hip), against the reference's kymatio torch frontend under
torch autograd in fp64 (fixtures tests/golden/scat_grad_<cfg>.npz, written by
tools/gen_golden_scat_grad.py) and against torch fp64 CPU autograd of the same
formulas for the single ops.

Bound of the gradient tests: e.max() <= 2 * r.max() + 2e-6 per-sample rel-L2,
with r the reference's own fp32-vs-fp64 gradient error on the same input.
2 * r is the rule of test_scattering1d_vs_reference_golden for this FFT engine;
the floor is that test's 1e-6 doubled, since the gradient runs the forward
chain and then its adjoint: twice the arithmetic depth."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CFGS = {  # cfg -> (J, Q, T, N, order, B); what each reaches: tools/gen_golden_scat_grad.py
    "a": (2, 1, 4, 64, 2, 3),        # one level; x[0] = 0: the zero-modulus subgradient
    "b": (3, 1, 8, 100, 1, 3),       # non-power-of-two N; _fused_ok(): the grad run must leave the fused path
    "c": (4, 4, 16, 256, 2, 3),      # level rows 512 / 256 / 128 / 64: both branches of fold_row
    "d": (6, 16, 64, 512, 2, 2),     # kymatio's known-answer configuration: many children per parent
    "e": (4, 1, 16, 12000, 2, 2),    # rows 16384 (four-step), 8192 (composed backward), 4096 (largest fused)
}


def rowrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a - b) ** 2).sum(-1) / (b ** 2).sum(-1))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sc(cfg, cascade=True):
    from vaeteb.scattering import Scattering1D
    J, Q, T, N, order, B = CFGS[cfg]
    sc = Scattering1D(J=J, shape=N, Q=Q, max_order=order, T=T)
    sc.cascade = cascade
    return sc


def _fixture(cfg):
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", f"scat_grad_{cfg}.npz"))


@functools.lru_cache(maxsize=None)
def _run(cfg, cascade):
    """(S, dsum(w S)/dx) of one fixture on one path, computed once for the tests that share it."""
    d = _fixture(cfg)
    sc = _sc(cfg, cascade)
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    S, S2 = sc(x)
    assert S is S2 and S.requires_grad
    (torch.from_numpy(d["w"]).cuda() * S).sum().backward()
    return S.detach().cpu().numpy(), x.grad.cpu().numpy()


@pytest.mark.parametrize("cascade", [True, False])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_grad_vs_reference(cfg, cascade):
    d = _fixture(cfg)
    S, g = _run(cfg, cascade)
    assert S.shape == d["S64"].shape and g.shape == d["g64"].shape
    e, r = rowrel(g, d["g64"]), rowrel(d["g32"], d["g64"])
    print(f"scat_grad {cfg} cascade={cascade}: e.max {e.max():.3e} r.max {r.max():.3e}")
    assert e.max() <= 2 * r.max() + 2e-6, (cfg, cascade, e, r)
    if cfg == "d":   # quadratic loss 0.5 ||S(x) - S(x0)||^2: the cotangent is itself computed
        sc = _sc(cfg, cascade)
        with torch.no_grad():
            T = sc(torch.from_numpy(d["x0"]).cuda())[0]
        x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
        (0.5 * ((sc(x)[0] - T) ** 2).sum()).backward()
        e, r = rowrel(x.grad.cpu().numpy(), d["gq64"]), rowrel(d["gq32"], d["gq64"])
        print(f"scat_grad {cfg} cascade={cascade} quadratic: e.max {e.max():.3e} r.max {r.max():.3e}")
        assert e.max() <= 2 * r.max() + 2e-6, (cfg, cascade, e, r)


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_forward_unchanged_under_grad(cfg):
    d = _fixture(cfg)
    sc = _sc(cfg)
    x = torch.from_numpy(d["x"]).cuda()
    S_grad, _ = _run(cfg, True)
    with torch.no_grad():
        S0 = sc(x)[0]
    assert not S0.requires_grad
    if cfg == "b":
        # without grad the fused first-order kernels still serve this configuration ...
        assert sc._fused_ok() and sc._cascade is None
        e, r = rowrel(S0.cpu().numpy(), d["S64"]), rowrel(d["S32"], d["S64"])
        assert e.max() <= 2 * r.max() + 1e-6, (e, r)
        # ... and under grad it ran the cascade: the bits of the cascade's own no-grad launches
        from vaeteb.scattering import _Cascade
        S0 = _Cascade(sc, x.device)(x)
        e = rowrel(S_grad, d["S64"])
        assert e.max() <= 2 * r.max() + 1e-6, (e, r)
    else:
        assert not sc._fused_ok()
    assert np.array_equal(S0.cpu().numpy(), S_grad)


def test_list_and_unaveraged_outputs_under_grad():
    """out_type='list' and average=False run the generic core: differentiable through the plugin ops."""
    from vaeteb.scattering import Scattering1D
    d = _fixture("c")
    J, Q, T, N, order, B = CFGS["c"]
    w = torch.from_numpy(d["w"]).cuda()
    sc = Scattering1D(J=J, shape=N, Q=Q, max_order=order, T=T, out_type="list")
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    S, _ = sc(x)
    assert len(S) == w.shape[1] and all(o["coef"].requires_grad for o in S)
    sum((w[:, i] * o["coef"]).sum() for i, o in enumerate(S)).backward()
    _, g_arr = _run("c", False)      # the same coefficients as one array, same cotangent
    assert rowrel(x.grad.cpu().numpy(), g_arr).max() < 1e-6
    # average=False: U1 / U2 themselves (no low-pass); every coefficient is |.| >= 0, so the sum is an l1 norm
    sc = Scattering1D(J=J, shape=N, Q=Q, max_order=order, T=T, out_type="list", average=False)
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    S, _ = sc(x)
    sum(o["coef"].sum() for o in S[1:]).backward()
    g = x.grad.cpu().numpy()
    assert np.isfinite(g).all() and (np.abs(g).max(-1) > 0).all()
    # the l1 norm is 1-homogeneous in x: <x, grad> = value (Euler), to fp32 accuracy
    val = sum(o["coef"].sum() for o in S[1:]).item()
    assert abs((g.astype(np.float64) * d["x"]).sum() - val) <= 1e-5 * abs(val)


# ------------------------------------------------------------------ plugin ops
def _c(t):
    return torch.view_as_complex(t.contiguous())


def _r(t):
    return torch.view_as_real(t)


def _op_grad(op, ref, x, seed=0):
    """(gradient through the HIP op, gradient of the fp64 CPU formula) under one random cotangent."""
    xg = x.clone().cuda().requires_grad_(True)
    y = op(xg)
    assert y.requires_grad
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    (w.float().cuda() * y).sum().backward()
    x64 = x.double().requires_grad_(True)
    y64 = ref(x64)
    assert y64.shape == y.shape
    (w.float().double() * y64).sum().backward()
    return xg.grad.cpu().double(), x64.grad


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("n,tol", [(256, 2e-6), (16384, 3e-6)])   # vt_fft (LDS) and vt_fft_large (four-step)
def test_plugin_fft_family_grads(n, tol):
    from vaeteb.scattering import TorchHipBackend1D as bk
    gen = torch.Generator().manual_seed(n)
    xc = torch.randn(3, n, 2, generator=gen)
    xr = torch.randn(3, n, 1, generator=gen)
    cases = [
        ("fft", bk.fft, lambda t: _r(torch.fft.fft(_c(t))), xc),
        ("ifft", bk.ifft, lambda t: _r(torch.fft.ifft(_c(t))), xc),
        ("rfft", bk.rfft, lambda t: _r(torch.fft.fft(torch.complex(t[..., 0], torch.zeros_like(t[..., 0])))), xr),
        ("irfft", bk.irfft, lambda t: torch.fft.ifft(_c(t)).real[..., None], xc),
    ]
    for name, op, ref, x in cases:
        g, g64 = _op_grad(op, ref, x)
        e = _rel(g, g64)
        print(f"plugin grad {name} n={n}: rel-L2 {e:.3e}")
        assert e < tol, (name, n, e)


def test_plugin_op_grads():
    from vaeteb.scattering import TorchHipBackend1D as bk
    gen = torch.Generator().manual_seed(7)
    A = torch.randn(2, 3, 16, 2, generator=gen)
    Br = torch.randn(16, 1, generator=gen)
    Bc = torch.randn(16, 2, generator=gen)
    g, g64 = _op_grad(lambda t: bk.cdgmm(t, Br.cuda()), lambda t: _r(_c(t) * Br[..., 0].double()), A)
    assert torch.allclose(g, g64, atol=1e-6), (g - g64).abs().max()
    g, g64 = _op_grad(lambda t: bk.cdgmm(t, Bc.cuda()), lambda t: _r(_c(t) * _c(Bc.double())), A)
    assert torch.allclose(g, g64, atol=1e-6), (g - g64).abs().max()
    with pytest.raises(RuntimeError, match="not differentiable in the filter"):
        bk.cdgmm(A.cuda().requires_grad_(True), Bc.cuda().requires_grad_(True))
    with pytest.raises(RuntimeError, match="not differentiable in the filter"):
        bk.cdgmm(A.cuda(), Br.cuda().requires_grad_(True))

    for N, k in [(64, 1), (64, 4), (64, 64), (16, 4)]:      # k = 1, 4, the whole row, and k = L
        x = torch.randn(2, 3, N, 2, generator=gen)
        g, g64 = _op_grad(lambda t: bk.subsample_fourier(t, k),
                          lambda t: _r(_c(t).reshape(2, 3, k, N // k).mean(-2)), x)
        assert torch.allclose(g, g64, atol=1e-6), (N, k, (g - g64).abs().max())

    for pl, pr in [(7, 5), (15, 15), (0, 3)]:               # the issue's case, the largest pads, no left pad
        x = torch.randn(3, 5, 16, generator=gen)
        g, g64 = _op_grad(lambda t: bk.pad(t, pl, pr), lambda t: F.pad(t, (pl, pr), mode="reflect")[..., None], x)
        assert torch.allclose(g, g64, atol=1e-6), (pl, pr, (g - g64).abs().max())


def test_plugin_ops_without_grad_cut_no_graph():
    """No input requiring grad: plain tensors out (the launches of the forward-only plugin)."""
    from vaeteb.scattering import TorchHipBackend1D as bk
    x = torch.randn(2, 16, 2, device="cuda")
    for y in (bk.fft(x), bk.ifft(x), bk.irfft(x), bk.subsample_fourier(x, 2), bk.pad(x[..., 0].contiguous(), 3, 2),
              bk.cdgmm(x, torch.randn(16, 1, device="cuda")), bk.rfft(x[..., :1].contiguous())):
        assert not y.requires_grad and y.grad_fn is None
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        assert torch.equal(bk.fft(xg), bk.fft(x)) and bk.fft(xg).grad_fn is None


# ------------------------------------------------------------------ properties
def test_backward_bitwise_reproducible():
    d = _fixture("d")
    sc = _sc("d")
    x6 = np.concatenate([d["x"], d["x0"], 0.5 * (d["x"] + d["x0"])]).astype(np.float32)     # (6, N)
    C, S = d["S64"].shape[1:]
    w6 = torch.randn(6, C, S, generator=torch.Generator().manual_seed(3)).cuda()

    def grad(shape):
        x = torch.from_numpy(x6).reshape(shape).cuda().requires_grad_(True)
        S_ = sc(x)[0]
        assert S_.shape == tuple(shape[:-1]) + (C, S)
        (w6.reshape(S_.shape) * S_).sum().backward()
        return x.grad.cpu().numpy()

    g1, g2 = grad((6, 512)), grad((6, 512))
    assert np.array_equal(g1, g2)
    g3 = grad((2, 3, 512))
    assert g3.shape == (2, 3, 512) and np.array_equal(g3.reshape(6, 512), g1)


@pytest.mark.parametrize("cascade", [True, False])
def test_double_backward_raises(cascade):
    d = _fixture("a")
    sc = _sc("a", cascade)
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    g, = torch.autograd.grad((sc(x)[0] ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
