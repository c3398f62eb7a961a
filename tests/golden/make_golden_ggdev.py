"""Writes tests/golden/ggnn_dev_small.npz: float64 vectors of the ggnn_dev and self-loop GGNN encoders, d = 8, out 4, on a padded
batch of three molecules: one dev case (tied, 3 steps, the hidden-wide sum) and one loop case (untied, 3 steps, concat_hidden);
20 atom types keep the embedding small.  The values are NOT made by tests/ggdev_ref.py: this file follows the reference's
reshape / transpose / matmul sequence (models/ggnn_dev.py:69-168, models/ggnn_dev_self_loop.py:67-145) and chainer's StatefulGRU
in plain numpy, so that the fixture pins the restatement from a second side.  Run from the repository root:
python tests/golden/make_golden_ggdev.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "gcn-bmp_amd")]
import ggdev_ref as R           # noqa: E402  (the parameter maker only)
from bmp import synth           # noqa: E402

sig = lambda x: 1.0 / (1.0 + np.exp(-x))


def run(kind, p, atoms, adj, layers, tying, concat_hidden):
    lin = lambda x, n: x @ p[n + "/W"].T + p[n + "/b"]
    h = p["embed/W"][atoms]
    h0 = h.copy()
    mb, atom, ch = h.shape
    state = None                                            # update_layer.reset_state()
    hs, gs = [], []
    for step in range(layers):
        li = 0 if tying else step
        m = lin(h, f"message_layers/{li}").reshape(mb, atom, ch, 4)
        m = m.transpose(0, 3, 1, 2).reshape(mb * 4, atom, ch)
        m = np.matmul(adj.reshape(mb * 4, atom, atom), m).reshape(mb, 4, atom, ch).sum(axis=1)
        if kind == "loop":
            m = m + lin(h, f"message_self_loop_layers/{li}")
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
    if concat_hidden:
        return np.concatenate(gs, axis=1), hs, gs
    return (h.sum(axis=1) if kind == "dev" else gs[-1]), hs, gs


CONFIGS = (("dev", dict(layers=3, tying=True, concat_hidden=False)), ("loop", dict(layers=3, tying=False, concat_hidden=True)))

if __name__ == "__main__":
    atoms, adj = synth.concat_mols(synth.make_store(3, seed=21, n_lo=2, n_hi=9, n_mean=5))
    adj = adj.astype(np.float64)
    out = {"atoms": atoms, "adj": adj}
    for kind, cfg in CONFIGS:
        p = R.make_params(kind, 41, 8, 4, cfg["layers"], cfg["tying"], cfg["concat_hidden"], n_atom_types=20)
        pn = {k: v.numpy() for k, v in p.items()}
        g, hs, gs = run(kind, pn, atoms.astype(np.int64), adj, **cfg)
        out.update({f"{kind}:p:{k}": v for k, v in pn.items()})
        out.update({f"{kind}:g": g, f"{kind}:hs": np.stack(hs), f"{kind}:gs": np.stack(gs)})
    np.savez_compressed(os.path.join(HERE, "ggnn_dev_small.npz"), **out)
