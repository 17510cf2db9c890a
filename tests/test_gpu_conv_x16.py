"""Staged 16-bit hand-off between conv blocks (model.ConvStack / ops.ConvBNActF x16 / y16;
vt_conv1d_bn_fwd_bf16_x16, vt_conv1d_bwd_weight_bf16_x16): a block writes y = act(BN(conv))
once as the next block's MFMA operand rows — 16-bit, channel stride ceil8(C), the x2 upsample
applied — and the consumer's forward and weight gradient copy those rows into their LDS windows
instead of re-forming them from the fp32 y.  The operand bits are the same by construction, so
a block pair run both ways must agree BIT FOR BIT in the consumer's pre-BN conv output, its
BatchNorm mean and rstd, its weight gradient and the input gradient it returns: no tolerance.

Shapes: the smallest at which each index path can go wrong, B = 3 — causal K 3 / 5 / 7; reflect
without upsample at L = 70 (64-row chunks) and L = 300 (256-row chunks where dY has <= 32
channels), both with a ragged last chunk and a split boundary inside a sample; reflect with the
x2 upsample at L = 8 (the shortest with L_up > pad) and L = 37 (odd row count, chunks starting on
odd upsampled rows); one fp16 case.  The staged rows' pad channels must be zero, and the consumer
must not use anything outside them: it runs on rows that sit between NaN guard bands, its
compared outputs in allocations of their own.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
CASES = (
    # (cin, cout, k, causal, up, L, fmt)
    [(c, c, k, True, False, 40, "bf16") for c in (16, 32) for k in (3, 5, 7)] +
    [(a, b, k, False, False, L, "bf16") for a, b, k in ((55, 44, 5), (22, 11, 3), (11, 1, 3)) for L in (70, 300)] +
    [(a, b, k, False, True, L, "bf16") for a, b, k in ((77, 66, 9), (33, 22, 3)) for L in (8, 37)] +
    [(33, 22, 3, False, True, 37, "fp16")]
)


def _params(cin, cout, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)
    w = ((r(cout, cin, k) - 0.5) * (2.0 / (cin * k) ** 0.5)).requires_grad_(True)
    gam = (0.5 + r(cout)).requires_grad_(True)
    bet = (0.6 * r(cout) - 0.3).requires_grad_(True)
    return w, gam, bet, torch.zeros(cout, device="cuda"), torch.ones(cout, device="cuda")


def _pair(cin, cout, k, causal, up, L, fmt, staged):
    """Producer block (8 -> cin, K 3) then the consumer (cin -> cout): the consumer's pre-BN output,
    statistics, weight gradient and returned input gradient (+ the staged rows)."""
    from vaeteb import ops
    mode = 0 if causal else 1
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = torch.randn(B, L, 8, device="cuda", generator=g)
    gy = torch.randn(B, L * (2 if up else 1), cout, device="cuda", generator=g)
    p0, p1 = _params(8, cin, 3, 2), _params(cin, cout, k, 3)
    rows = None
    if staged:
        h, rows = ops.conv_bn_act(x0, *p0, mode=mode, up=False, bf16=fmt, y16=up)
        assert h.shape == (B, L, cin) and rows.shape == (B, L * (2 if up else 1), (cin + 7) // 8 * 8)
        # the consumer reads a copy of the rows between NaN guard bands (128 bytes each side)
        buf = torch.full((rows.numel() + 128,), float("nan"), dtype=rows.dtype, device="cuda")
        buf[64:64 + rows.numel()] = rows.reshape(-1)
        y = ops.conv_bn_act(h, *p1, mode=mode, up=up, bf16=fmt, x16=buf[64:64 + rows.numel()].view(rows.shape))
    else:
        h = ops.conv_bn_act(x0, *p0, mode=mode, up=False, bf16=fmt)
        y = ops.conv_bn_act(h, *p1, mode=mode, up=up, bf16=fmt)
    h.retain_grad()
    _, conv, mean, rstd = y.grad_fn.saved_tensors[:4]
    y.backward(gy)
    torch.cuda.synchronize()
    return {"conv": conv, "mean": mean, "rstd": rstd, "y": y.detach(), "dW": p1[0].grad, "dx": h.grad,
            "dgamma": p1[1].grad, "dW0": p0[0].grad}, rows


@pytest.mark.parametrize("cin,cout,k,causal,up,L,fmt", CASES)
def test_staged_handoff_bitwise(cin, cout, k, causal, up, L, fmt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ref, _ = _pair(cin, cout, k, causal, up, L, fmt, staged=False)
    got, rows = _pair(cin, cout, k, causal, up, L, fmt, staged=True)
    assert rows.dtype == (torch.float16 if fmt == "fp16" else torch.bfloat16)
    assert not rows[..., cin:].any(), "pad channels of the staged rows"
    assert torch.isfinite(rows.float()).all() and rows.float().abs().sum() > 0
    for key in ref:
        assert ref[key].shape == got[key].shape, key
        d = (ref[key] - got[key]).abs().max().item()
        print(f"{key}: max |diff| {d:.3e}")
    bad = [key for key in ref if not torch.equal(ref[key], got[key])]
    assert not bad, bad
    assert torch.isfinite(got["dW"]).all() and torch.isfinite(got["dx"]).all()
