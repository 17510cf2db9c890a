#!/usr/bin/env python3
"""Time the surrogate test of the transfer entropy (vaeteb.tenull.TeSignificance) end to end against
the literal alternative kept on the device: for every variant k the surrogate batch is materialised
with torch.gather (the block permutation and the roll as one index), run through
ShiftSweep(x_k, [0], elementwise=True), averaged over the latent with .mean(-1), and the ranks are
formed with torch comparisons.  Both paths give the same te and the same integers, checked in the
same run.  Workload: B windows of 5760 samples (trim 30, 300 steps), kind="block", K = 199, the
bench's precisions (conv / mlp / head bf16, lstm 16-mixed).

HIP events around whole calls, both variants warmed at the timed shapes, alternated within each
repeat, median and min-max over the repeats.  The three new kernels are also timed alone at the
workload's shapes (the rows of one chunk for the two row kernels), with the bytes their
code requests ("moved": gathers and second passes included, wherever they are served from) against
the bytes that have to cross at least once ("compulsory").  One JSON line per section.

Usage:  python tools/tenull_micro.py [--B 64] [--K 199] [--repeats 5] [--kind block]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-teb_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vaeteb import _lib, synthetic  # noqa: E402
from vaeteb.frontend import FrontEnd, FrontEndPlan, _i32, load_stats  # noqa: E402
from vaeteb.model import SeqVaeTeb  # noqa: E402
from vaeteb.te import ShiftSweep  # noqa: E402
from vaeteb.tenull import TeSignificance, rank_statistics, surrogate_plan  # noqa: E402


def plan_index(plan, N):
    """(B, K+1, N) int64 on the device: the source sample of every surrogate sample."""
    B, K1 = plan.src.shape
    j = (np.arange(N)[None, None, :] - plan.shift[:, :, None].astype(np.int64)) % N
    if plan.perm is not None:
        bl = int(plan.block_len)
        nblk = N // bl
        blk = np.minimum(j // bl, nblk - 1)
        moved = np.take_along_axis(plan.perm.astype(np.int64), blk, axis=2) * bl + j % bl
        j = np.where(j < nblk * bl, moved, j)
    return torch.from_numpy(j).cuda()


def literal(sweep, x, plan, idx):
    src = torch.from_numpy(plan.src.astype(np.int64)).cuda()
    te, ts = [], []
    for k in range(plan.src.shape[1]):
        xk = x.clone()
        xk[:, 1] = torch.gather(x[src[:, k], 1], 1, idx[:, k])
        r = sweep(xk, [0], elementwise=True)
        te.append(r.te[:, 0])
        ts.append(r.kl[:, 0].mean(-1))
    te, ts = torch.stack(te, 1), torch.stack(ts, 1)
    count = (te[:, 1:] >= te[:, :1]).sum(1)
    step = (ts[:, 1:] >= ts[:, :1]).sum(1)
    mx = (ts[:, 1:].max(-1).values[:, :, None] >= ts[:, :1]).sum(1)
    return te, ts, count, step, mx


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def med(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)]}


def kernel_times(fn, repeats, calls=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return [timed(lambda: [fn() for _ in range(calls)])[0] / calls for _ in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--K", type=int, default=199)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kind", default="block")
    ap.add_argument("--rows-per-launch", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tenull_micro needs a GPU: nothing is measured without one")
    if a.repeats < 5:
        raise SystemExit("at least 5 repeats")
    N, B, K1 = 5760, a.B, a.K + 1
    fe = FrontEnd(FrontEndPlan(11, 4, 16, N, device="cuda"), load_stats(11, 4, 16, 4096), trim=30)
    p = fe.plan
    torch.manual_seed(0)
    model = SeqVaeTeb(sequence_length=fe.S_out, scattering_channels=fe.C_st, phase_channels=fe.C_ph,
                      cross_phase_channels=fe.C_x, conv_precision="bf16", mlp_precision="bf16",
                      head_precision="bf16", lstm_precision="16-mixed").cuda()
    x = torch.from_numpy(synthetic.batch(0, B, N)).cuda()
    plan = surrogate_plan(a.kind, B, a.K, N, seed=0)
    idx = plan_index(plan, N)
    sig, sweep = TeSignificance(model, fe, a.rows_per_launch), ShiftSweep(model, fe, a.rows_per_launch)
    for _ in range(2):                          # warm-up of both variants at the timed shapes
        r = sig(x, plan=plan)
        lit = literal(sweep, x, plan, idx)
        torch.cuda.synchronize()
        print("warm-up pass done", file=sys.stderr, flush=True)
    te_new = torch.cat([r.te[:, None], r.te_surr], 1)
    ts_new = torch.cat([r.te_steps[:, None], r.te_steps_surr], 1)
    # the literal path's integers come from its own fp32 .mean(-1); the new path's from its double sums:
    # where the two ts differ in the last bit a tie can fall the other way, so the integers are also
    # recomputed with the same torch comparisons on the new path's ts / te, which must match exactly
    same = {"te_bit_equal": bool(torch.equal(te_new, lit[0])),
            "te_max_rel_diff": ((te_new - lit[0]).abs() / lit[0].abs()).max().item(),
            "ts_max_rel_diff": ((ts_new - lit[1]).abs() / lit[1].abs()).max().item(),
            "count_ge_equal_literal": bool(torch.equal(r.count_ge.long(), lit[2])),
            "step_count_ge_differing_literal": int((r.step_count_ge.long() != lit[3]).sum()),
            "max_count_ge_differing_literal": int((r.max_count_ge.long() != lit[4]).sum()),
            "integers_equal_torch_on_own_ts": bool(
                torch.equal(r.count_ge.long(), (te_new[:, 1:] >= te_new[:, :1]).sum(1))
                and torch.equal(r.step_count_ge.long(), (ts_new[:, 1:] >= ts_new[:, :1]).sum(1))
                and torch.equal(r.max_count_ge.long(),
                                (ts_new[:, 1:].max(-1).values[:, :, None] >= ts_new[:, :1]).sum(1)))}
    tn, tl = [], []
    for _ in range(a.repeats):                  # alternated: drift hits both alike
        tn.append(timed(lambda: sig(x, plan=plan))[0])
        tl.append(timed(lambda: literal(sweep, x, plan, idx))[0])
    print(json.dumps({"section": "end_to_end", "N": N, "B": B, "K": a.K, "kind": a.kind, "rows": B * K1,
                      "rows_per_launch": a.rows_per_launch, "tenull": med(tn), "literal": med(tl),
                      "literal_over_tenull": round(statistics.median(tl) / statistics.median(tn), 2),
                      "repeats": a.repeats, **same}), flush=True)

    # ---- the three new kernels alone
    S, L, st = fe.S_out, model.latent_dim_target, _lib.stream()
    chunks = sig.sweep._chunks(B, K1)
    R = chunks[0][1] * chunks[0][3]                # the rows of one pass through the row kernels
    src, shift, perm = _i32(plan.src, "cuda"), _i32(plan.shift, "cuda"), (
        None if plan.perm is None else _i32(plan.perm, "cuda"))
    xhat = torch.empty((R, p.n_pad, 2), device="cuda")
    t = kernel_times(lambda: _lib.call("vt_fe_spectrum_surrogate", x.data_ptr() + 4 * N, B, 2 * N, N, p.n_pad,
                                       p.pad_left, 0, _lib.ptr(src), _lib.ptr(shift), _lib.ptr(perm),
                                       int(plan.block_len), 0, R, _lib.ptr(p.t_tw), _lib.ptr(xhat), st), a.repeats)
    nblk = N // int(plan.block_len)
    moved = R * (4 * p.n_pad + (4 * p.n_pad if perm is not None else 0) + 8 * p.n_pad + 8)
    comp = R * (8 * p.n_pad + 8 + (4 * nblk if perm is not None else 0)) + 4 * N * min(B, R)
    print(json.dumps({"section": "vt_fe_spectrum_surrogate", "rows": R, **med(t), "bytes_moved": moved,
                      "bytes_compulsory": comp, "compulsory_GBps": round(comp / statistics.median(t) / 1e6, 1),
                      "calls_per_significance_call": len(chunks)}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    mu_c, lv_q = torch.randn(R, S, L, device="cuda", generator=g), torch.randn(R, S, L, device="cuda", generator=g)
    nb = max(1, R // K1)
    kk = R // nb
    mu_y, lv_p = torch.randn(nb, S, L, device="cuda", generator=g), torch.randn(nb, S, L, device="cuda", generator=g)
    ts, te = torch.empty((nb * kk, S), device="cuda"), torch.empty(nb * kk, device="cuda")
    t = kernel_times(lambda: _lib.call("vt_te_kl_steps", _lib.ptr(mu_c), _lib.ptr(lv_q), _lib.ptr(mu_y),
                                       _lib.ptr(lv_p), nb, kk, S, L, _lib.ptr(ts), _lib.ptr(te), st), a.repeats)
    rows = nb * kk
    moved = rows * (16 * S * L + 4 * S + 4)
    comp = rows * (8 * S * L + 4 * S + 4) + nb * 8 * S * L
    print(json.dumps({"section": "vt_te_kl_steps", "rows": rows, "S": S, "L": L, **med(t), "bytes_moved": moved,
                      "bytes_compulsory": comp, "compulsory_GBps": round(comp / statistics.median(t) / 1e6, 1),
                      "elementwise_tensor_bytes_not_written": rows * 4 * S * L,
                      "calls_per_significance_call": len(chunks)}), flush=True)
    ts_all, te_all = ts_new.contiguous(), te_new.contiguous()
    t = kernel_times(lambda: rank_statistics(ts_all, te_all), a.repeats)
    moved = 2 * ts_all.numel() * 4 + te_all.numel() * 8 + B * (20 + 12 * S) + 8 * K1
    comp = ts_all.numel() * 4 + te_all.numel() * 4 + B * (20 + 12 * S) + 8 * K1
    print(json.dumps({"section": "vt_tenull_stats (with its output allocations)", "B": B, "K1": K1, "S": S, **med(t),
                      "bytes_moved": moved, "bytes_compulsory": comp,
                      "compulsory_GBps": round(comp / statistics.median(t) / 1e6, 1),
                      "calls_per_significance_call": 1}), flush=True)


if __name__ == "__main__":
    main()
