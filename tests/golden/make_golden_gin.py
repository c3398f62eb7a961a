"""Writes tests/golden/gin_small.npz: float64 vectors of the GIN restatement (tests/gin_ref.py), d = 8, out 4: a 2-atom
molecule, a 5-ring, and a padded batch of 3 (untied 2 layers, concat_hidden).  Run from the repository root:
python tests/golden/make_golden_gin.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "gcn-bmp_amd")]
import gin_ref as GR            # noqa: E402
from bmp import synth           # noqa: E402

two = synth.Molecule(np.array([6, 8], np.int32), np.array([[0, 1, 1]], np.int32))
ring = synth.Molecule(np.array([6, 6, 7, 6, 8], np.int32), np.array([[k, (k + 1) % 5, k % 4] for k in range(5)], np.int32))
batch = synth.make_store(3, seed=21, n_lo=2, n_hi=9, n_mean=5)
p = GR.make_gin_params(11, 8, 4, 2, False, concat_hidden=True)
out = {"p:" + k: v.numpy() for k, v in p.items()}
for name, mols in (("two", [two]), ("ring", [ring]), ("batch", batch)):
    atoms, adj = synth.concat_mols(mols)
    g, h = GR.gin_forward(p, atoms, adj, tying=False, concat_hidden=True)
    out.update({name + ":atoms": atoms, name + ":adj": adj, name + ":g": g.numpy(), name + ":h": h.numpy()})
np.savez_compressed(os.path.join(HERE, "gin_small.npz"), **out)
