#!/usr/bin/env python3
"""Generate tests/golden/eval_gain_s16_b3.npz from the REFERENCE code (build container only, as
tools/gen_golden.py, whose helpers it uses).

The reference's UP gain sweep (ref/model/graph_model.py:1779-1870; gain 1 alone is its metrics
histogram analysis :1510-1680, gains {1, 0} its UP ablation :1682-1777) on three synthetic recordings
at S = 16 (n = 256): the reference SeqVaeTeb with det_fill_ weights, one train-mode forward to move
the BatchNorm running buffers, then eval(); reparameterize replaced by the stored eps (as
run_ref_step); for every gain g the forward on x_ph * float(g) (:1833-1835) and
measure_transfer_entropy(reduce_mean=False).mean() per sample (:1836-1839, :1602); VAF / MSE / SNR
by the reference's literal numpy lines (:1619-1645).

Gains [0, 0.001, 0.01, 1, 2, -1], not the reference's default [0, .5, 1, 1.5, 2]: the source encoder
starts Linear -> LayerNorm, so it is almost invariant to a positive scale (gains 0.5 and 2 move mu_pr
by ~1e-5 rel-L2 against gain 1, below every tolerance of the tests), and a sweep that ignored the gain
would pass on the default list.  Gain 2 stays to cover that near-invariant case.

y_raw[b] = mu_pr[b, gain 1] + a_b * std(mu_pr[b, gain 1]) * noise, a = (0.3, 0.6, 1.0): every row's
VAF then lies strictly inside (0, 1) and the clamp of :1627 is never active.

Asserted here (and re-checked by tests/test_eval_cpu.py on the stored values): every one of the 18
rows has vaf_unclamped in (0.05, 0.95); rows of different gains among {0, 0.001, 0.01, 1, -1} differ
in mu_pr by more than 1e-2 rel-L2.

One eps (B, S, 32) serves every gain, so the rows of one recording differ by the gain alone.

Stored (data only): gains, the inputs y_st / y_ph / x_ph, eps (B, S, 32), y_raw, the reference's
mu_pr (B, K, n), te / vaf / mse / snr / vaf_unclamped (B, K), and all BatchNorm running buffers
(decoder included) after the train-mode forward.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_eval.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (sets the reference import paths)

GAINS = [0.0, 0.001, 0.01, 1.0, 2.0, -1.0]
DISTINCT = [0, 1, 2, 3, 5]          # indices of {0, 0.001, 0.01, 1, -1}
B, S, L = 3, 16, 32
A = (0.3, 0.6, 1.0)
NAME = "eval_gain_s16_b3.npz"


def ref_metrics(gt, pr):
    """The float32 numpy operations of ref/model/graph_model.py:1619-1645 on one sample (np.var and
    np.mean of float32 rows, the same thresholds), plus the VAF before its clamp."""
    res = gt - pr
    vy = np.var(gt)
    vu = 1.0 - np.var(res) / vy if vy > 1e-12 else 0.0
    mse = np.mean((gt - pr) ** 2)
    noise = np.mean(res ** 2)
    snr = 10.0 * np.log10(np.mean(gt ** 2) / noise) if noise > 1e-12 else 100.0
    return max(0.0, min(1.0, vu)), mse, snr, vu


def main():
    rng = np.random.Generator(np.random.PCG64(7100))
    K, n = len(GAINS), 16 * S
    y_st = rng.standard_normal((B, S, 43)).astype(np.float32)
    y_ph = rng.standard_normal((B, S, 44)).astype(np.float32)
    x_ph = rng.standard_normal((B, S, 130)).astype(np.float32)
    eps = rng.standard_normal((B, S, L)).astype(np.float32)
    noise = rng.standard_normal((B, n)).astype(np.float32)
    T = torch.from_numpy

    model = G.build_ref_model(S)
    cur = {}
    model.reparameterize = lambda mu, lv: mu + cur["eps"] * torch.exp(0.5 * lv)
    model.train()
    cur["eps"] = T(eps)
    with torch.no_grad():
        model(T(y_st), T(y_ph), T(x_ph))                 # updates the BatchNorm running statistics
    model.eval()

    mu_pr = np.zeros((B, K, n), np.float32)
    te = np.zeros((B, K), np.float32)
    with torch.no_grad():
        for k, g in enumerate(GAINS):                    # the loop of :1832-1839
            x_scaled = T(x_ph) * float(g)
            out = model(T(y_st), T(y_ph), x_scaled)
            mu_pr[:, k] = out["mu_pr"].numpy()
            kld = model.measure_transfer_entropy(T(y_st), T(y_ph), x_scaled, reduce_mean=False)
            te[:, k] = kld.mean(dim=(1, 2)).numpy()
    assert not model.training

    base = mu_pr[:, GAINS.index(1.0)]
    y_raw = np.stack([base[b] + np.float32(A[b]) * np.std(base[b]) * noise[b] for b in range(B)]).astype(np.float32)
    m = np.array([[ref_metrics(y_raw[b], mu_pr[b, k]) for k in range(K)] for b in range(B)], dtype=np.float64)
    vaf, mse, snr, vaf_u = (m[..., i] for i in range(4))     # float64 holds the reference's float32 results exactly

    assert ((vaf_u > 0.05) & (vaf_u < 0.95)).all(), vaf_u
    for b in range(B):
        for i in DISTINCT:
            for j in DISTINCT:
                if i < j:
                    d = np.linalg.norm(mu_pr[b, i].astype(np.float64) - mu_pr[b, j]) / np.linalg.norm(mu_pr[b, j])
                    assert d > 1e-2, (b, GAINS[i], GAINS[j], d)
    one = GAINS.index(1.0)
    print("rel-L2 of mu_pr against gain 1, per gain:",
          [float(np.linalg.norm(mu_pr[:, k].astype(np.float64) - mu_pr[:, one]) / np.linalg.norm(mu_pr[:, one]))
           for k in range(K)])
    print("te:", te, "\nvaf:", vaf, "\nmse:", mse, "\nsnr:", snr)

    sd = model.state_dict()
    bn_keys = [k for k in sd if k.endswith("running_mean") or k.endswith("running_var")]
    G.save(NAME, gains=np.array(GAINS, np.float64), y_st=y_st, y_ph=y_ph, x_ph=x_ph, eps=eps, y_raw=y_raw,
           mu_pr=mu_pr, te=te, vaf=vaf, mse=mse, snr=snr, vaf_unclamped=vaf_u, bn_names=np.array(bn_keys),
           **{f"bn_{i}": sd[k].numpy() for i, k in enumerate(bn_keys)})
    assert os.path.getsize(os.path.join(G.OUT, NAME)) < (1 << 20)


if __name__ == "__main__":
    main()
