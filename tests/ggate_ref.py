"""Dense restatement of the two gated GGNN encoders of the reference, op for op, in the dtype of the parameters it is given
(float64 for reference values): models/ggnn_dev_fuse.py (kind "fuse") and models/ggnn_dev_gate.py (kind "gate").

    h0 = h = embed[atoms]                                                          (mb, A, d)
    per step:  m = ggnn_message(h, adj, message_layers[0 if tying else step])      (oracle.ref_cpu, models/ggnn.py's message)
               x = [h, m] per atom row
               fuse:  z = tanh(W1 x + b1), r = sigmoid(W2 x + b2), f = sigmoid(W3 x + b3);  h = keep * (r * h) + f * z
                      (keep: F.dropout(r * h, 0.05)'s multiplier, 0 or 1 / 0.95; None in evaluation mode)
               gate:  a = sigmoid(Wg_k x + bg_k), k = 0 if update_tying else step;  h = (1 - a) * h + a * m
               h = step_keep * h  (F.dropout(h, dropout_rate), training only)
               concat_hidden: g_list += ggnn_readout(h, h0, step)
    readout = sum over ALL A positions of sigmoid(i([h, h0])) * j(h): padded positions (id 0, no bonds) count everywhere.

Parameter names are the link paths of the reference: embed/W, message_layers/{i}/{W,b}, update_layer{1,2,3}/{W,b} (fuse) or
gate_layer/{k}/{W,b} (gate), i_layers/{k}/{W,b}, j_layers/{k}/{W,b}; the fuse file also constructs update_layer/{W_r,W_z,W,U_r,
U_z,U}/{W,b} (the GRU it no longer calls) and embed_linear/{W,b} (66 -> d, float atom features only): drawn, never read.
"""
import math

import numpy as np
import torch

from oracle import ref_cpu as O
from gin_ref import data          # noqa: F401  (the data sets: "fixture" 13 + 13 instances, "small", "oversized")

FUSE_DROPOUT = 0.05


def make_params(kind, seed, hidden, out, layers, tying, update_tying=True, concat_hidden=False, n_atom_types=117,
                dtype=torch.float64, prefix="", bias=0.3):
    """Fixed draw order: embed, the message layers, the update, the readout layers, then (fuse) the links nobody calls."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    d = hidden
    p = {prefix + "embed/W": r(n_atom_types, d)}
    for i in range(1 if tying else layers):
        p[f"{prefix}message_layers/{i}/W"] = r(4 * d, d) / math.sqrt(d) * 0.5
        p[f"{prefix}message_layers/{i}/b"] = bias * r(4 * d)
    if kind == "fuse":
        for k in (1, 2, 3):
            p[f"{prefix}update_layer{k}/W"] = r(d, 2 * d) / math.sqrt(2 * d)
            p[f"{prefix}update_layer{k}/b"] = bias * r(d)
    else:
        for k in range(1 if update_tying else layers):
            p[f"{prefix}gate_layer/{k}/W"] = r(d, 2 * d) / math.sqrt(2 * d)
            p[f"{prefix}gate_layer/{k}/b"] = bias * r(d)
    for k in range(layers if concat_hidden else 1):
        p[f"{prefix}i_layers/{k}/W"] = r(out, 2 * d) / math.sqrt(2 * d)
        p[f"{prefix}i_layers/{k}/b"] = bias * r(out)
        p[f"{prefix}j_layers/{k}/W"] = r(out, d) / math.sqrt(d)
        p[f"{prefix}j_layers/{k}/b"] = bias * r(out)
    if kind == "fuse":
        for n, k_in in (("W_r", 2 * d), ("W_z", 2 * d), ("W", 2 * d), ("U_r", d), ("U_z", d), ("U", d)):
            p[f"{prefix}update_layer/{n}/W"] = r(d, k_in) / math.sqrt(k_in)
            p[f"{prefix}update_layer/{n}/b"] = bias * r(d)
        p[f"{prefix}embed_linear/W"] = r(d, 66) / math.sqrt(66)
        p[f"{prefix}embed_linear/b"] = bias * r(d)
    return {k: v.to(dtype) for k, v in p.items()}


def forward(kind, params, atoms, adj, layers, tying=True, update_tying=True, concat_hidden=False, keep=None, step_keep=None,
            prefix=""):
    """(g, h).  ``keep`` / ``step_keep``: one (mb, A, d) multiplier per step (the fuse gate's dropout on r * h / the dropout on
    the step's output), or None (evaluation mode)."""
    P = lambda k: params[prefix + k]
    dt = P("embed/W").dtype
    atoms = torch.as_tensor(np.asarray(atoms)).long()
    adj = torch.as_tensor(np.asarray(adj)).to(dt)
    h = P("embed/W")[atoms]
    h0 = h
    mb, A, d = h.shape
    g_list = []
    for step in range(layers):
        li = 0 if tying else step
        m = O.ggnn_message(h, adj, P(f"message_layers/{li}/W"), P(f"message_layers/{li}/b"))
        hf, mf = h.reshape(mb * A, d), m.reshape(mb * A, d)
        x = torch.cat((hf, mf), dim=1)
        if kind == "fuse":
            z = torch.tanh(O.linear(x, P("update_layer1/W"), P("update_layer1/b")))
            r = torch.sigmoid(O.linear(x, P("update_layer2/W"), P("update_layer2/b")))
            f = torch.sigmoid(O.linear(x, P("update_layer3/W"), P("update_layer3/b")))
            rh = r * hf
            if keep is not None:
                rh = rh * keep[step].to(dt).reshape(mb * A, d)
            out = rh + f * z
        else:
            k = 0 if update_tying else step
            a = torch.sigmoid(O.linear(x, P(f"gate_layer/{k}/W"), P(f"gate_layer/{k}/b")))
            out = (1 - a) * hf + a * mf
        h = out.reshape(mb, A, d)
        if step_keep is not None:
            h = h * step_keep[step].to(dt)
        if concat_hidden:
            g_list.append(O.ggnn_readout(h, h0, P(f"i_layers/{step}/W"), P(f"i_layers/{step}/b"),
                                         P(f"j_layers/{step}/W"), P(f"j_layers/{step}/b")))
    if concat_hidden:
        return torch.cat(g_list, dim=1), h
    return O.ggnn_readout(h, h0, P("i_layers/0/W"), P("i_layers/0/b"), P("j_layers/0/W"), P("j_layers/0/b")), h


# name: kind, seed, hidden, out, layers, tying, update_tying, data.  Widths 16 and 24 take the composed operators, 64 and 128 the
# fused kernels; "fixture" has all four bond types, rows lacking a type, pad rows of multiplicity > 1 and three tiles; "oversized"
# one molecule larger than a tile.
CASES = {
    "fuse16": dict(kind="fuse", seed=1, hidden=16, out=16, layers=3, tying=True, update_tying=True, data="fixture"),
    "fuse24": dict(kind="fuse", seed=2, hidden=24, out=12, layers=2, tying=False, update_tying=True, data="fixture"),
    "fuse64": dict(kind="fuse", seed=3, hidden=64, out=32, layers=3, tying=False, update_tying=True, data="fixture"),
    "fuse128": dict(kind="fuse", seed=4, hidden=128, out=64, layers=2, tying=True, update_tying=True, data="fixture"),
    "gate16": dict(kind="gate", seed=5, hidden=16, out=16, layers=3, tying=False, update_tying=True, data="fixture"),
    "gate24": dict(kind="gate", seed=6, hidden=24, out=12, layers=2, tying=True, update_tying=True, data="fixture"),
    "gate64": dict(kind="gate", seed=7, hidden=64, out=32, layers=3, tying=True, update_tying=True, data="fixture"),
    "gate128": dict(kind="gate", seed=8, hidden=128, out=64, layers=2, tying=False, update_tying=True, data="fixture"),
    "gate16u": dict(kind="gate", seed=9, hidden=16, out=8, layers=3, tying=True, update_tying=False, data="fixture"),
    "gate64u": dict(kind="gate", seed=10, hidden=64, out=16, layers=3, tying=False, update_tying=False, data="fixture"),
    "fuse_over16": dict(kind="fuse", seed=11, hidden=16, out=8, layers=2, tying=False, update_tying=True, data="oversized"),
    "fuse_over64": dict(kind="fuse", seed=12, hidden=64, out=16, layers=2, tying=False, update_tying=True, data="oversized"),
    "gate_over16": dict(kind="gate", seed=13, hidden=16, out=8, layers=2, tying=False, update_tying=True, data="oversized"),
    "gate_over64": dict(kind="gate", seed=14, hidden=64, out=16, layers=2, tying=False, update_tying=True, data="oversized"),
    "fuse_small16": dict(kind="fuse", seed=15, hidden=16, out=8, layers=2, tying=False, update_tying=True, data="small"),
    "gate_small64": dict(kind="gate", seed=16, hidden=64, out=16, layers=2, tying=False, update_tying=True, data="small"),
    "fuse_keep16": dict(kind="fuse", seed=17, hidden=16, out=8, layers=2, tying=False, update_tying=True, data="fixture"),
    "fuse_keep64": dict(kind="fuse", seed=18, hidden=64, out=16, layers=2, tying=True, update_tying=True, data="fixture"),
    "fuse_pair16": dict(kind="fuse", seed=19, hidden=16, out=16, layers=2, tying=True, update_tying=True, data="fixture"),
}


def case_params(c, concat_hidden=False, prefix=""):
    return make_params(c["kind"], c["seed"], c["hidden"], c["out"], c["layers"], c["tying"], c["update_tying"], concat_hidden,
                       prefix=prefix)


def case_forward(c, params, atoms, adj, concat_hidden=False, keep=None, prefix=""):
    return forward(c["kind"], params, atoms, adj, c["layers"], c["tying"], c["update_tying"], concat_hidden, keep=keep, prefix=prefix)


def keep_rows(name, hidden, steps, seed, p=FUSE_DROPOUT):
    """``steps`` fuse-gate masks on the packed rows of data set ``name`` ((n_rows, hidden) float32, values 0 or 1 / (1 - p)): the
    pad row of a molecule carries one mask for all its padded positions."""
    g = torch.Generator().manual_seed(seed)
    n = data(name)["pb"].n_rows
    return [(torch.rand(n, hidden, generator=g) >= p).float() * (1.0 / (1.0 - p)) for _ in range(steps)]


def keep_dense(name, rows, side):
    """The row masks at the dense positions of one side: [(mb, A, hidden)] per step."""
    dm = data(name)["pb"].dense_maps[side]
    return [k[dm] for k in rows]
