"""Writes tests/golden/nfp_small.npz: float64 vectors of the NFP restatement (tests/nfp_ref.py) on five small synthetic
molecules, d = 16, out 8, two layers.  Run from the repository root: python tests/golden/make_golden_nfp.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "gcn-bmp_amd")]
import nfp_ref as NR            # noqa: E402
from bmp import synth           # noqa: E402

store = synth.make_store(5, seed=21, n_lo=2, n_hi=12, n_mean=6)
atoms, adj = NR.nfp_adj(store)
p = NR.make_nfp_params(11, 16, 8, 2)
g, h = NR.nfp_forward(p, atoms, adj)
np.savez_compressed(os.path.join(HERE, "nfp_small.npz"), atoms=atoms, adj=adj, g=g.numpy(), atoms_out=h.numpy(),
                    **{"p:" + k: v.numpy() for k, v in p.items()})
