"""Writes tests/golden/ggnn_edge_small.npz: float64 vectors of the GGNN with message_function='edge_network', d = 8, out 4, on a
padded batch of three molecules: one tied case (3 steps, the plain readout) and one untied case (3 steps, concat_hidden); 20 atom
types keep the embedding small.  The values are NOT made by tests/edge_ref.py: this file follows the reference's reshape /
transpose / matmul sequence (EdgeNetwork.__call__, models/ggnn.py:685-720; GGNN.update and __call__, :215-263, 584-654) and
chainer's StatefulGRU in plain numpy, so that the fixture pins the restatement from a second side.  Run from the repository root:
python tests/golden/make_golden_edge.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "gcn-bmp_amd")]
import edge_ref as R            # noqa: E402  (the parameter maker only)
from bmp import synth           # noqa: E402

sig = lambda x: 1.0 / (1.0 + np.exp(-x))


def edge_network(p, name, h, adj):
    mb, n_et, atoms, _ = adj.shape
    nd = h.shape[2]
    a = adj.transpose(0, 2, 3, 1).reshape(mb * atoms * atoms, n_et)
    out = a @ p[name + "/output_layer/W"].T + p[name + "/output_layer/b"]
    tmp = out.reshape(mb, atoms, atoms, nd, nd)
    big = tmp.transpose(0, 1, 3, 2, 4).reshape(-1, atoms * nd, atoms * nd)
    mul = np.matmul(big, h.reshape(mb, atoms * nd, 1)).reshape(mb * atoms, nd)
    return (mul + np.zeros(nd)).reshape(mb, atoms, nd)


def run(p, atoms, adj, layers, tying, concat_hidden):
    lin = lambda x, n: x @ p[n + "/W"].T + p[n + "/b"]
    h = p["embed/W"][atoms]
    h0 = h.copy()
    mb, atom, ch = h.shape
    state = None                                            # update_layer.reset_state()
    hs, gs = [], []
    for step in range(layers):
        m = edge_network(p, f"message_layers/{0 if tying else step}", h, adj).reshape(mb, atom, ch)
        x = np.concatenate((h.reshape(mb * atom, ch), m.reshape(mb * atom, ch)), axis=1)
        z, hb = lin(x, "update_layer/W_z"), lin(x, "update_layer/W")
        if state is None:                                   # StatefulGRU without a state: no r, no U
            state = sig(z) * np.tanh(hb)
        else:
            r = sig(lin(x, "update_layer/W_r") + lin(state, "update_layer/U_r"))
            z = sig(z + lin(state, "update_layer/U_z"))
            hb = np.tanh(hb + lin(r * state, "update_layer/U"))
            state = (1 - z) * state + z * hb
        h = state.reshape(mb, atom, ch)
        k = step if concat_hidden else 0
        hs.append(h)
        gs.append((sig(lin(np.concatenate((h, h0), axis=2), f"i_layers/{k}")) * lin(h, f"j_layers/{k}")).sum(axis=1))
    return (np.concatenate(gs, axis=1) if concat_hidden else gs[-1]), hs


CONFIGS = (("tied", dict(layers=3, tying=True, concat_hidden=False)), ("untied", dict(layers=3, tying=False, concat_hidden=True)))

if __name__ == "__main__":
    atoms, adj = synth.concat_mols(synth.make_store(3, seed=21, n_lo=2, n_hi=9, n_mean=5))
    adj = adj.astype(np.float64)
    out = {"atoms": atoms, "adj": adj}
    for tag, cfg in CONFIGS:
        p = R.make_params(43, 8, 4, cfg["layers"], cfg["tying"], cfg["concat_hidden"], n_atom_types=20, a_typ=atoms.shape[1])
        pn = {k: v.numpy() for k, v in p.items()}
        g, hs = run(pn, atoms.astype(np.int64), adj, **cfg)
        out.update({f"{tag}:p:{k}": v for k, v in pn.items()})
        out.update({f"{tag}:g": g, f"{tag}:hs": np.stack(hs)})
    np.savez_compressed(os.path.join(HERE, "ggnn_edge_small.npz"), **out)
