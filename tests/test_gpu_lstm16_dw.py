"""The 16-bit LSTM's gate-gradient hand-off and batched weight gradient on MI355X.

vt_lstm16_pair_bwd / vt_lstm16_quad_bwd can emit each layer's gate gradients as the bf16 image
the recurrence itself works on ([B S][4H], column 4 u + g = gate g of unit u) instead of fp32
[B S][4H] by gate row; vt_lstm16_bwd_weight_multi (csrc/skdw16.hip k_sk_dw16m + k_sk_sum16) forms
the parameter gradients of up to four layers from either format in one launch.  Everything here
is a bitwise statement — the image is the rounded fp32 gradient, the weight gradients do not
depend on the format, the batching or the entry point — except the kernel's own accuracy, which
keeps test_gpu_lstm16.test_lstm16_weight_grad_bf16's criterion: rel-L2 <= 1e-5 to the fp64 sum of
the bf16-rounded operands (fp32 accumulation order only).

Row partition: a layer's workgroups depend on B S alone (ceil(B S / 256) of them, at most 128,
each a whole number of 32-row chunks), so no workgroup is ever empty; the "fewer rows than
workgroups" situation shows up as a workgroup whose only chunk is mostly rows past the range
(B S = 2) and as a last workgroup shorter than the others (B S = 111, 2400).
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64
GUARD = 4096   # elements before and after a buffer under test


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vaeteb import ops as o
    return o


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def P(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def to_image(dg):
    """fp32 dgates [..., 4H] by gate row -> the bf16 image (column 4 u + g)"""
    s = dg.shape
    return dg.view(*s[:-1], 4, H).transpose(-1, -2).reshape(s).bfloat16().contiguous()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


SENT = 0x5A5A


class Guarded:
    """A bf16 buffer of n elements between two guard regions, all filled with a sentinel"""

    def __init__(self, n):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int16, device="cuda")
        self.t = self.raw[GUARD: GUARD + n].view(torch.bfloat16)

    def guards_ok(self):
        return bool((self.raw[:GUARD] == SENT).all() and (self.raw[GUARD + self.n:] == SENT).all())


def _forward(In, B, S, nl, seed):
    """nl (2 or 4) layers' forward through the pair kernels: parameters and saved state"""
    from vaeteb import _lib
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(In, H, nl, batch_first=True)
    prm = [p.detach().cuda().contiguous() for p in ref.parameters()]
    x = torch.randn(B, S, In, device="cuda")
    hs, cs, gs = ([torch.empty(B, S, w, device="cuda") for _ in range(nl)] for w in (H, H, 4 * H))
    inp = x
    for l in range(0, nl, 2):
        a, b = prm[4 * l: 4 * l + 4], prm[4 * l + 4: 4 * l + 8]
        _lib.call("vt_lstm16_pair_fwd", P(inp), inp.shape[-1], P(a[0]), P(a[2]), P(a[1]), P(a[3]), P(b[0]), P(b[2]),
                  P(b[1]), P(b[3]), B, S, H, P(hs[l]), P(cs[l]), P(gs[l]), P(hs[l + 1]), P(cs[l + 1]), P(gs[l + 1]),
                  _st())
        inp = hs[l + 1]
    dh = torch.randn(B, S, H, device="cuda")
    return prm, x, hs, cs, gs, dh


def _backward(kind, prm, cs, gs, dh, In, B, S, mask):
    """pair (layers 1, 0) or quad backward; dgates of layer l as the image where bit l of mask is
    set.  Returns (dgates tensors, their guard holders, dx, dmid)."""
    from vaeteb import _lib
    nl = 2 if kind == "pair" else 4
    hold = [Guarded(B * S * 4 * H) if (mask >> l) & 1 else None for l in range(nl)]
    dg = [hold[l].t.view(B, S, 4 * H) if hold[l] else torch.full((B, S, 4 * H), float("nan"), device="cuda")
          for l in range(nl)]
    dx = torch.full((B, S, In), float("nan"), device="cuda")
    dmid = None
    if kind == "pair":
        _lib.call("vt_lstm16_pair_bwd", P(dh), P(gs[1]), P(cs[1]), P(prm[5]), P(prm[4]), P(gs[0]), P(cs[0]), P(prm[1]),
                  P(prm[0]), In, B, S, H, P(dg[1]), P(dg[0]), P(dx), _st(), mask)
    else:
        dmid = torch.full((B, S, H), float("nan"), device="cuda")
        wv = (ctypes.c_void_p * 8)(*[P(prm[4 * k + i]) for k in range(4) for i in (0, 1)])
        gv = (ctypes.c_void_p * 8)(*[P(t) for k in range(4) for t in (gs[k], cs[k])])
        dv = (ctypes.c_void_p * 4)(*[P(t) for t in dg])
        _lib.call("vt_lstm16_quad_bwd", P(dh), ctypes.addressof(wv), ctypes.addressof(gv), In, B, S, H,
                  ctypes.addressof(dv), P(dmid), P(dx), _st(), mask)
    torch.cuda.synchronize()
    return dg, hold, dx, dmid


@pytest.mark.parametrize("kind,In,B,S", [("pair", 20, 3, 37), ("pair", 32, 5, 33), ("pair", 64, 4, 16),
                                         ("pair", 20, 2, 1), ("pair", 8, 4, 33), ("quad", 32, 6, 40),
                                         ("quad", 32, 64, 17)])
def test_image_is_rounded_fp32_gradient(ops, kind, In, B, S):
    """The bf16 image == dgates.bfloat16() with columns permuted k' = 4 u + g, bit for bit, for
    every layer of the pair and of the quad backward (B = 6: the pairs unchained; B = 64: the
    chained launch); dx and dmid do not depend on the format; nothing is written outside the
    image's [0, B S) rows (ragged batches, S not a multiple of the 16-step chunk, S = 1)."""
    nl = 2 if kind == "pair" else 4
    prm, x, hs, cs, gs, dh = _forward(In, B, S, nl, 100 + In + B + S)
    full = (1 << nl) - 1
    dg32, _, dx32, dm32 = _backward(kind, prm, cs, gs, dh, In, B, S, 0)
    dg16, hold, dx16, dm16 = _backward(kind, prm, cs, gs, dh, In, B, S, full)
    for l in range(nl):
        assert torch.isfinite(dg32[l]).all()
        assert torch.equal(bits(dg16[l]), bits(to_image(dg32[l]))), l
        assert hold[l].guards_ok(), l
    assert torch.equal(bits(dx16), bits(dx32)) and torch.isfinite(dx32).all()
    if kind == "quad":
        assert torch.equal(bits(dm16), bits(dm32))
        # mixed formats in one launch: layers 0 and 3 fp32, 1 and 2 as images
        dgm, holdm, dxm, _ = _backward(kind, prm, cs, gs, dh, In, B, S, 0b0110)
        for l in range(nl):
            want = dg16[l] if l in (1, 2) else dg32[l]
            assert torch.equal(bits(dgm[l]), bits(want)), l
            assert holdm[l] is None or holdm[l].guards_ok()
        assert torch.equal(bits(dxm), bits(dx32))


# ------------------------------------------------------------------ weight gradients
def _operands(In, B, S, seed):
    torch.manual_seed(seed)
    dg = torch.randn(B, S, 4 * H, device="cuda")
    x = torch.randn(B, S, In, device="cuda")
    h = torch.randn(B, S, H, device="cuda")
    return dg, x, h


def _outs(In, fill=float("nan")):
    return [torch.full(s, fill, device="cuda") for s in ((4 * H, In), (4 * H, H), (4 * H,), (4 * H,))]


_WS = {}


def _ws():
    if "ws" not in _WS:
        _WS["ws"] = torch.empty(32 << 20, device="cuda")
    return _WS["ws"]


def _multi(layers, B, S, outs, acc):
    """layers: [(dg tensor fp32 or bf16 image, x, h)]; outs: per layer 4 tensors; acc: per layer"""
    from vaeteb import _lib
    n = len(layers)
    dv = (ctypes.c_void_p * n)(*[P(e[0]) for e in layers])
    fv = (ctypes.c_int * n)(*[int(e[0].dtype == torch.bfloat16) for e in layers])
    xv = (ctypes.c_void_p * n)(*[P(e[1]) for e in layers])
    iv = (ctypes.c_int * n)(*[e[1].shape[-1] for e in layers])
    hv = (ctypes.c_void_p * n)(*[P(e[2]) for e in layers])
    gv = (ctypes.c_void_p * (4 * n))(*[P(t) for o in outs for t in o])
    av = (ctypes.c_int * n)(*acc)
    ws = _ws()
    _lib.call("vt_lstm16_bwd_weight_multi", n, ctypes.addressof(dv), ctypes.addressof(fv), ctypes.addressof(xv),
              ctypes.addressof(iv), ctypes.addressof(hv), B, S, H, ctypes.addressof(gv), ctypes.addressof(av), P(ws),
              ws.numel(), _st())
    torch.cuda.synchronize()


def _ref64(dg, x, h):
    b16 = lambda t: t.cpu().bfloat16().double()
    hp = torch.cat([torch.zeros_like(h[:, :1]), h[:, :-1]], 1)
    g16 = b16(dg)
    return [torch.einsum("bsg,bsi->gi", g16, b16(x)), torch.einsum("bsg,bsi->gi", g16, b16(hp)), g16.sum((0, 1)),
            g16.sum((0, 1))]


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B,S", [(2, 1), (3, 37), (8, 300)])
@pytest.mark.parametrize("In", [8, 20, 32, 64])
def test_weight_grad_from_image(ops, In, B, S, acc):
    """vt_lstm16_bwd_weight_multi fed the image == fed the fp32 dgates, bit for bit, and within
    rel-L2 1e-5 of the fp64 sum of the bf16-rounded operands: B S = 2 (less than a chunk), 111
    (not a multiple of 32 or 64, t = 0 rows mid-chunk), 2400 (10 workgroups of 8 chunks, the last
    one shorter); accumulate = 0 overwrites NaN-filled outputs, accumulate = 1 adds to them."""
    dg, x, h = _operands(In, B, S, 7 * In + S)
    img = Guarded(B * S * 4 * H)
    img.t.copy_(to_image(dg).view(-1))
    res = []
    torch.manual_seed(1)
    base = [torch.randn_like(t) for t in _outs(In)]
    for d in (dg, img.t.view(B, S, 4 * H)):
        o = [b.clone() for b in base] if acc else _outs(In)
        _multi([(d, x, h)], B, S, [o], [acc])
        res.append(o)
    assert img.guards_ok()
    for a, b in zip(res[0], res[1]):
        assert torch.equal(bits(a), bits(b))
    if acc:   # base + the accumulate = 0 result (checked against fp64 in the acc = 0 case), in fp32
        o0 = _outs(In)
        _multi([(dg, x, h)], B, S, [o0], [0])
        for a, z, b0 in zip(res[0], o0, base):
            assert torch.equal(bits(a), bits(b0 + z))
    else:
        for a, r in zip(res[0], _ref64(dg, x, h)):
            assert rel(a, r) <= 1e-5, rel(a, r)


def _four_layers(B, S):
    ins = (20, 64, 64, 64)
    ops_ = [_operands(In, B, S, 31 + 5 * k) for k, In in enumerate(ins)]
    return ins, ops_


@pytest.mark.parametrize("B,S", [(3, 37), (8, 300)])
def test_batching_does_not_change_bits(ops, B, S):
    """Four layers (In 20, 64, 64, 64) in one call == each in a call of its own ==
    vt_lstm16_layer_bwd_weight, bit for bit; also one fp32 layer with two image layers in one
    call (nl = 3), and in another order.  The one-call result repeated: the same bits."""
    from vaeteb import _lib
    ins, L = _four_layers(B, S)
    imgs = [to_image(dg) for dg, _, _ in L]
    one = [_outs(In) for In in ins]
    _multi([(imgs[k], L[k][1], L[k][2]) for k in range(4)], B, S, one, [0] * 4)
    again = [_outs(In) for In in ins]
    _multi([(imgs[k], L[k][1], L[k][2]) for k in range(4)], B, S, again, [0] * 4)
    single = [_outs(In) for In in ins]
    for k in range(4):
        _multi([(imgs[k], L[k][1], L[k][2])], B, S, [single[k]], [0])
    layer = [_outs(In) for In in ins]
    ws = _ws()
    for k in range(4):
        _lib.call("vt_lstm16_layer_bwd_weight", P(L[k][0]), P(L[k][1]), ins[k], P(L[k][2]), B, S, H,
                  *[P(t) for t in layer[k]], 0, P(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    mixed = [_outs(ins[k]) for k in (1, 0, 2)]   # fp32 In = 64 first, then the In = 20 and In = 64 images
    _multi([(L[1][0], L[1][1], L[1][2]), (imgs[0], L[0][1], L[0][2]), (imgs[2], L[2][1], L[2][2])], B, S, mixed,
           [0] * 3)
    for k in range(4):
        for j in range(4):
            assert torch.isfinite(one[k][j]).all()
            assert torch.equal(bits(one[k][j]), bits(again[k][j])), (k, j)
            assert torch.equal(bits(one[k][j]), bits(single[k][j])), (k, j)
            assert torch.equal(bits(one[k][j]), bits(layer[k][j])), (k, j)
    for m, k in enumerate((1, 0, 2)):
        for j in range(4):
            assert torch.equal(bits(mixed[m][j]), bits(one[k][j])), (k, j)


# ------------------------------------------------------------------------- fallback
def test_unsupported_shape_keeps_fp32_dgates(ops, monkeypatch):
    """In = 30 (not a multiple of 4): vt_lstm16_dg16_ok says no, the batched entry runs such a
    layer on the exact-fp32 kernel (== vt_lstm_layer_bwd_weight on an explicit h_{t-1}, bit for
    bit) beside a bf16 layer, refuses an image for it, and ops.lstm(half=True) runs with the
    same gradients whichever hand-off format is configured."""
    from vaeteb import _lib
    ok = _lib.lib().fns["vt_lstm16_dg16_ok"]
    assert ok(30) == 0 and ok(68) == 0 and ok(32) == 1 and ok(20) == 1 and ok(64) == 1 and ok(8) == 1
    B, S = 3, 37
    dg, x, h = _operands(30, B, S, 3)
    dg2, x2, h2 = _operands(64, B, S, 4)
    hp = torch.cat([torch.zeros_like(h[:, :1]), h[:, :-1]], 1).contiguous()
    o, o2 = _outs(30), _outs(64)
    _multi([(dg, x, h), (to_image(dg2), x2, h2)], B, S, [o, o2], [0, 0])
    e, e2 = _outs(30), _outs(64)
    ws = _ws()
    _lib.call("vt_lstm_layer_bwd_weight", P(dg), P(x), 30, P(hp), B, S, H, *[P(t) for t in e], 0, P(ws), ws.numel(),
              _st())
    _multi([(dg2, x2, h2)], B, S, [e2], [0])
    torch.cuda.synchronize()
    for a, b in zip(o + o2, e + e2):
        assert torch.equal(bits(a), bits(b))
    with pytest.raises(ValueError):
        _multi([(to_image(dg), x, h)], B, S, [_outs(30)], [0])
    torch.manual_seed(9)
    ref = torch.nn.LSTM(30, H, 3, batch_first=True)
    prm = [p.detach().cuda() for p in ref.parameters()]
    xin = torch.randn(B, S, 30, device="cuda")
    gy = torch.randn(B, S, H, device="cuda")
    res = []
    for f in (1, 0):
        monkeypatch.setattr(ops, "LSTM_DG16", f)
        pd = [p.clone().requires_grad_() for p in prm]
        xd = xin.clone().requires_grad_()
        y = ops.lstm(xd, pd, half=True)
        y.backward(gy)
        torch.cuda.synchronize()
        res.append([y.detach(), xd.grad] + [p.grad for p in pd])
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b))


_CHILD = """
import sys, torch
sys.path.insert(0, {pkg!r})
from vaeteb import ops, _lib
In, B, S, nl = {In}, {B}, {S}, {nl}
torch.manual_seed(5 + In + S + B)
ref = torch.nn.LSTM(In, 64, nl, batch_first=True)
params = [p.detach().cuda() for p in ref.parameters()]
x = torch.randn(B, S, In, device="cuda")
gy = torch.randn(B, S, 64, device="cuda")
real_call = ops.call
def run(pair):
    ops.LSTM_PAIR = pair
    called = []
    ops.call = lambda name, *a: (called.append(name), real_call(name, *a))[1]
    pd = [p.clone().requires_grad_() for p in params]
    xd = x.clone().requires_grad_()
    y = ops.lstm(xd, pd, half=True)
    y.backward(gy)
    torch.cuda.synchronize()
    ops.call = real_call
    return [y.detach().cpu(), xd.grad.cpu()] + [p.grad.cpu() for p in pd], called
out, called = run(1)
ok16 = _lib.lib().fns["vt_lstm16_dg16_ok"](In)
if {per_layer}:
    out0, called0 = run(0)
    assert "vt_lstm16_pair_bwd" not in called0 and "vt_lstm16_quad_bwd" not in called0
    assert all(torch.equal(a, b) for a, b in zip(out, out0))
torch.save(dict(out=out, multi=called.count("vt_lstm16_bwd_weight_multi"),
                quad=called.count("vt_lstm16_quad_bwd"), ok16=ok16), {dst!r})
print("ok")
"""


def _child(tmp_path, name, env, In, B, S, nl, per_layer):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vae-teb_amd")
    dst = str(tmp_path / f"{name}.pt")
    code = _CHILD.format(pkg=pkg, In=In, B=B, S=S, nl=nl, per_layer=per_layer, dst=dst)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    return torch.load(dst)


def test_exact_fp32_switch_matches_per_layer_path(ops, tmp_path):
    """VAETEB_L16_DW16=0 in a fresh process: no layer qualifies for the image, and ops.lstm
    through the quad launch and the batched entry == the same process's per-layer path, bit for
    bit (the exact-fp32 kernel either way)."""
    r = _child(tmp_path, "dw16off", {"VAETEB_L16_DW16": "0"}, 20, 6, 40, 4, 1)
    assert r["ok16"] == 0 and r["multi"] == 1 and r["quad"] == 1


@pytest.mark.parametrize("In,B,S", [(20, 6, 40), (32, 64, 17)])
def test_autograd_end_to_end_format_switch(ops, tmp_path, In, B, S):
    """ops.lstm with four layers in fresh processes, VAETEB_L16_DG16=1 against =0: y, x.grad and
    every parameter gradient bit-equal (the same kernel and partition; only the dG format
    differs), one vt_lstm16_bwd_weight_multi call per backward."""
    r1 = _child(tmp_path, "dg16on", {"VAETEB_L16_DG16": "1"}, In, B, S, 4, 0)
    r0 = _child(tmp_path, "dg16off", {"VAETEB_L16_DG16": "0"}, In, B, S, 4, 0)
    assert r1["multi"] == 1 and r0["multi"] == 1 and r1["quad"] == 1 and r0["quad"] == 1 and r1["ok16"] == 1
    for k, (a, b) in enumerate(zip(r1["out"], r0["out"])):
        assert torch.isfinite(a).all() and torch.equal(a, b), k
