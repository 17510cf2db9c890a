#!/usr/bin/env python3
"""Generate tests/golden/te_shift_j11_n4096.npz (+ its inputs, te_shift_j11_n4096_in.npz) from the
REFERENCE code (build container only, as tools/gen_golden.py, whose helpers it uses).

The reference's transfer-entropy-vs-shift analysis (ref/model/graph_model.py:1210-1458) on two
synthetic recordings and four shifts: for each (recording, shift) the up channel is rolled with
np.roll (:1443-1458), the reference's KymatioPhaseScattering1D computes the cross-phase features
(:1328-1336), cross_mask selects the 130 channels, normalize_tensor_data applies the shipped
statistics (:1340-1350, channels first as the dataset calls it, then the (C, S) -> (S, C)
transpose of hdf5_dataset.py:758-759), and the reference SeqVaeTeb (S = 256, det_fill_ weights,
after one train-mode forward on the unshifted batch, as gen_te) gives
measure_transfer_entropy(reduce_mean=False).mean() (:1368-1371).  No trim: 4096-point windows.

Stored (data only): shifts, the normalised x_ph (2, 4, 256, 130), te (2, 4) and the encoders'
BatchNorm running buffers after the train-mode forward (the decoder's depend on the reference's
random noise and do not enter the transfer entropy); in the second file the windows x and the
normalised target-side inputs y_st / y_ph the reference model was given.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_te_shift.py [--seed START]
"""
import argparse
import os
import sys
import typing

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (sets the reference import paths)
from vaeteb import synthetic  # noqa: E402

SHIFTS = np.array([0, -1, 7, -240], dtype=np.int64)
J, Q, T, N, S = 11, 4, 16, 4096, 256


def main(start):
    from kymatio_phase_scattering import KymatioPhaseScattering1D
    norm = G.extract_functions(os.path.join(G.REF, "hdf5_dataset/hdf5_dataset.py"), ["normalize_tensor_data"],
                               {"torch": torch, "np": np, **vars(typing)})["normalize_tensor_data"]
    st = np.load(os.path.join(G.ROOT, "vae-teb_amd", "vaeteb", "data", f"stats_j{J}q{Q}t{T}_n{N}.npz"))
    nstats = {k: {"mean": st[k + "_mean"], "variance": st[k + "_variance"]} for k in ("fhr_st", "fhr_ph", "fhr_up_ph")}
    cfg = ({"fhr_st": "all_except_0"}, {"fhr_ph": "all", "fhr_up_ph": "all"}, 1e-6)
    normalise = lambda a, field: norm(a, field, nstats, *cfg).transpose(1, 2).contiguous()

    x = synthetic.batch(start, 2, N)
    m = KymatioPhaseScattering1D(J=J, Q=Q, T=T, shape=N, device=torch.device("cpu"), max_order=1)
    sel = m.get_optimal_coefficients_for_fhr(J, Q, T)
    pm, cm = sel["recommendations"]["use_phase_mask"], sel["recommendations"]["use_cross_mask"]
    xt = torch.from_numpy(x)
    rp = m(x=xt, compute_phase=True, compute_cross_phase=False, scattering_channel=0, phase_channels=[0])
    y_st = normalise(rp["scattering"], "fhr_st")
    y_ph = normalise(rp["phase_corr"][:, pm, :], "fhr_ph")
    x_ph = torch.empty(2, len(SHIFTS), S, int(cm.sum()))
    for b in range(2):
        for k, sh in enumerate(SHIFTS):
            xs = np.stack([x[b, 0], np.roll(x[b, 1], int(sh))])[None]          # _apply_circular_shift
            rc = m(x=torch.from_numpy(xs), compute_phase=False, compute_cross_phase=True, scattering_channel=0,
                   phase_channels=[0, 1])
            x_ph[b, k] = normalise(rc["cross_phase_corr"][:, cm, :], "fhr_up_ph")[0]
    assert y_st.shape == (2, S, 43) and y_ph.shape == (2, S, 44) and x_ph.shape == (2, 4, S, 130)

    model = G.build_ref_model(S)
    model.train()
    with torch.no_grad():
        model(y_st, y_ph, x_ph[:, 0].contiguous())      # updates the BatchNorm running statistics
    te = np.zeros((2, len(SHIFTS)), np.float32)
    for b in range(2):
        for k in range(len(SHIFTS)):
            kld = model.measure_transfer_entropy(y_st=y_st[b:b + 1], y_ph=y_ph[b:b + 1], x_ph=x_ph[b:b + 1, k],
                                                 reduce_mean=False)
            te[b, k] = kld.mean().item()
    assert not model.training
    sd = model.state_dict()
    bn_keys = [k for k in sd if (k.endswith("running_mean") or k.endswith("running_var"))
               and not k.startswith("decoder.")]
    print("te:", te, "argmin:", te.argmin(1))
    # two files: the features alone are ~1.0 MB compressed, just under the committed-file limit
    G.save("te_shift_j11_n4096.npz", shifts=SHIFTS, x_ph=x_ph.numpy(), te=te, bn_names=np.array(bn_keys),
           **{f"bn_{i}": sd[k].numpy() for i, k in enumerate(bn_keys)})
    G.save("te_shift_j11_n4096_in.npz", x=x, seed_start=start, y_st=y_st.numpy(), y_ph=y_ph.numpy())
    for f in ("te_shift_j11_n4096.npz", "te_shift_j11_n4096_in.npz"):
        assert os.path.getsize(os.path.join(G.OUT, f)) < (1 << 20), f


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=3000, help="first synthetic window (vaeteb.synthetic.batch start)")
    main(ap.parse_args().seed)
