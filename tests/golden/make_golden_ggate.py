"""Writes tests/golden/ggnn_gate_small.npz: float64 vectors of the two gated GGNN encoders, d = 8, out 4, on a padded batch of
three molecules: one fuse case (tied, 3 steps) and one gate case (untied message weights, update_tying=False, 2 steps,
concat_hidden); 20 atom types keep the embedding small.  The values are NOT made by tests/ggate_ref.py: this file follows the
reference's reshape / transpose / matmul sequence (models/ggnn_dev_fuse.py:90-131, models/ggnn_dev_gate.py:76-119) in plain
numpy, so that the fixture pins the restatement from a second side.  Run from the repository root:
python tests/golden/make_golden_ggate.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "gcn-bmp_amd")]
import ggate_ref as R           # noqa: E402  (the parameter maker only)
from bmp import synth           # noqa: E402

sig = lambda x: 1.0 / (1.0 + np.exp(-x))


def run(kind, p, atoms, adj, layers, tying, update_tying, concat_hidden):
    lin = lambda x, n: x @ p[n + "/W"].T + p[n + "/b"]
    h = p["embed/W"][atoms]
    h0 = h.copy()
    mb, atom, ch = h.shape
    gs = []
    for step in range(layers):
        li = 0 if tying else step
        m = lin(h, f"message_layers/{li}").reshape(mb, atom, ch, 4)
        m = m.transpose(0, 3, 1, 2).reshape(mb * 4, atom, ch)
        m = np.matmul(adj.reshape(mb * 4, atom, atom), m).reshape(mb, 4, atom, ch).sum(axis=1)
        hf, mf = h.reshape(mb * atom, ch), m.reshape(mb * atom, ch)
        x = np.concatenate((hf, mf), axis=1)
        if kind == "fuse":
            z, r, f = np.tanh(lin(x, "update_layer1")), sig(lin(x, "update_layer2")), sig(lin(x, "update_layer3"))
            out = r * hf + f * z
        else:
            a = sig(lin(x, f"gate_layer/{0 if update_tying else step}"))
            out = (1 - a) * hf + a * mf
        h = out.reshape(mb, atom, ch)
        if concat_hidden:
            gs.append((sig(lin(np.concatenate((h, h0), axis=2), f"i_layers/{step}")) * lin(h, f"j_layers/{step}")).sum(axis=1))
    if concat_hidden:
        return np.concatenate(gs, axis=1), h
    return (sig(lin(np.concatenate((h, h0), axis=2), "i_layers/0")) * lin(h, "j_layers/0")).sum(axis=1), h


atoms, adj = synth.concat_mols(synth.make_store(3, seed=21, n_lo=2, n_hi=9, n_mean=5))
adj = adj.astype(np.float64)
out = {"atoms": atoms, "adj": adj}
for kind, cfg in (("fuse", dict(layers=3, tying=True, update_tying=True, concat_hidden=False)),
                  ("gate", dict(layers=2, tying=False, update_tying=False, concat_hidden=True))):
    p = R.make_params(kind, 31, 8, 4, cfg["layers"], cfg["tying"], cfg["update_tying"], cfg["concat_hidden"], n_atom_types=20)
    pn = {k: v.numpy() for k, v in p.items()}
    g, h = run(kind, pn, atoms.astype(np.int64), adj, **cfg)
    out.update({f"{kind}:p:{k}": v for k, v in pn.items()})
    out.update({f"{kind}:g": g, f"{kind}:h": h})
np.savez_compressed(os.path.join(HERE, "ggnn_gate_small.npz"), **out)
