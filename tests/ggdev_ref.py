"""Dense restatement of the reference's models/ggnn_dev.py (kind "dev") and models/ggnn_dev_self_loop.py = models/ggnn_dev_edge.py
(kind "loop"), op for op, in the dtype of the parameters it is given (float64 for reference values).

    h0 = h = embed[atoms]                                                          (mb, A, d)
    per step:  m = ggnn_message(h, adj, message_layers[l]),  l = 0 if tying else step     (oracle.ref_cpu, models/ggnn.py's message)
               loop:  m = m + linear(h, message_self_loop_layers[l])               (ggnn_dev_self_loop.py:96-97)
               s = stateful_gru([h, m], s)      (first call after reset: z * tanh(W x), no r gate and no U terms)
               h = step_keep * s                (F.dropout(h, dropout_rate), training only; the GRU keeps the un-dropped s)
               g_t = ggnn_readout(h, h0, readout layer t if concat_hidden else 0)
    dev:   returns cat(g_t) with concat_hidden, else sum over ALL A positions of h_T -- (mb, d), NOT out wide
           (ggnn_dev.py:165-168 compute the readout and overwrite it); get_atom_array(t) = h_t, get_g_list() = [g_t]
    loop:  returns cat(g_t) with concat_hidden, else ggnn_readout(h_T, h0, layer 0)
    The readout sums over ALL A positions: padded positions (id 0, no bonds) count everywhere.

Parameter names are the link paths of the reference: embed/W, message_layers/{i}/{W,b}, message_self_loop_layers/{i}/{W,b} (loop),
update_layer/{W_r,W_z,W,U_r,U_z,U}/{W,b}, i_layers/{k}/{W,b}, j_layers/{k}/{W,b}.
"""
import math

import numpy as np
import torch

from oracle import ref_cpu as O
from gin_ref import data, keep_dense          # noqa: F401  (the data sets: "fixture" 13 + 13 instances, "small", "oversized")


def make_params(kind, seed, hidden, out, layers, tying, concat_hidden=False, n_atom_types=117, dtype=torch.float64, prefix="",
                bias=0.3):
    """Fixed draw order: embed, the message layers, (loop) the self-loop layers, the GRU, the readout layers."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    d = hidden
    p = {prefix + "embed/W": r(n_atom_types, d)}
    for i in range(1 if tying else layers):
        p[f"{prefix}message_layers/{i}/W"] = r(4 * d, d) / math.sqrt(d) * 0.5
        p[f"{prefix}message_layers/{i}/b"] = bias * r(4 * d)
    if kind == "loop":
        for i in range(1 if tying else layers):
            p[f"{prefix}message_self_loop_layers/{i}/W"] = r(d, d) / math.sqrt(d) * 0.5
            p[f"{prefix}message_self_loop_layers/{i}/b"] = bias * r(d)
    for n, k_in in (("W_r", 2 * d), ("W_z", 2 * d), ("W", 2 * d), ("U_r", d), ("U_z", d), ("U", d)):
        p[f"{prefix}update_layer/{n}/W"] = r(d, k_in) / math.sqrt(k_in)
        p[f"{prefix}update_layer/{n}/b"] = bias * r(d)
    for k in range(layers if concat_hidden else 1):
        p[f"{prefix}i_layers/{k}/W"] = r(out, 2 * d) / math.sqrt(2 * d)
        p[f"{prefix}i_layers/{k}/b"] = bias * r(out)
        p[f"{prefix}j_layers/{k}/W"] = r(out, d) / math.sqrt(d)
        p[f"{prefix}j_layers/{k}/b"] = bias * r(out)
    return {k: v.to(dtype) for k, v in p.items()}


def forward(kind, params, atoms, adj, layers, tying=True, concat_hidden=False, step_keep=None, prefix=""):
    """(g, [h_t], [g_t]).  ``step_keep``: one (mb, A, d) multiplier per step (the dropout on the step's output), or None
    (evaluation mode)."""
    P = lambda k: params[prefix + k]
    dt = P("embed/W").dtype
    atoms = torch.as_tensor(np.asarray(atoms)).long()
    adj = torch.as_tensor(np.asarray(adj)).to(dt)
    h = P("embed/W")[atoms]
    h0 = h
    mb, A, d = h.shape
    sp = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix + "update_layer/")}
    s = None
    hs, gs = [], []
    for step in range(layers):
        li = 0 if tying else step
        m = O.ggnn_message(h, adj, P(f"message_layers/{li}/W"), P(f"message_layers/{li}/b"))
        if kind == "loop":
            m = m + O.linear(h, P(f"message_self_loop_layers/{li}/W"), P(f"message_self_loop_layers/{li}/b"))
        x = torch.cat((h.reshape(mb * A, d), m.reshape(mb * A, d)), dim=1)
        s = O.stateful_gru(sp, "update_layer", x, s)
        h = s.reshape(mb, A, d)
        if step_keep is not None:
            h = h * step_keep[step].to(dt)
        k = step if concat_hidden else 0
        hs.append(h)
        gs.append(O.ggnn_readout(h, h0, P(f"i_layers/{k}/W"), P(f"i_layers/{k}/b"), P(f"j_layers/{k}/W"), P(f"j_layers/{k}/b")))
    if concat_hidden:
        return torch.cat(gs, dim=1), hs, gs
    if kind == "dev":
        return h.sum(dim=1), hs, gs
    return gs[-1], hs, gs


# name: kind, seed, hidden, out, layers, tying, data.  Self loop: widths 16, 24 and 32 take the composed operators, 64 and 128 the
# fused kernels (1 layer: the first-call kernel alone; 3 layers: the later-call kernel twice); "fixture" has all four bond types, rows
# lacking a type, pad rows of multiplicity > 1 and three tiles; "oversized" one molecule larger than a tile.
CASES = {
    "loop16": dict(kind="loop", seed=1, hidden=16, out=16, layers=3, tying=True, data="fixture"),
    "loop24": dict(kind="loop", seed=2, hidden=24, out=12, layers=2, tying=False, data="fixture"),
    "loop32": dict(kind="loop", seed=3, hidden=32, out=16, layers=2, tying=False, data="fixture"),
    "loop64": dict(kind="loop", seed=4, hidden=64, out=32, layers=3, tying=False, data="fixture"),
    "loop128": dict(kind="loop", seed=5, hidden=128, out=64, layers=2, tying=True, data="fixture"),
    "loop64_1": dict(kind="loop", seed=6, hidden=64, out=16, layers=1, tying=True, data="fixture"),
    "loop128_3": dict(kind="loop", seed=7, hidden=128, out=16, layers=3, tying=False, data="fixture"),
    "loop_over16": dict(kind="loop", seed=8, hidden=16, out=8, layers=2, tying=False, data="oversized"),
    "loop_over64": dict(kind="loop", seed=9, hidden=64, out=16, layers=2, tying=False, data="oversized"),
    "loop_small16": dict(kind="loop", seed=10, hidden=16, out=8, layers=2, tying=False, data="small"),
    "loop_small64": dict(kind="loop", seed=11, hidden=64, out=16, layers=2, tying=True, data="small"),
    "loop_drop64": dict(kind="loop", seed=12, hidden=64, out=16, layers=3, tying=True, data="fixture"),
    "loop_pair16": dict(kind="loop", seed=13, hidden=16, out=16, layers=2, tying=True, data="fixture"),
    "dev16": dict(kind="dev", seed=14, hidden=16, out=8, layers=3, tying=True, data="fixture"),
    "dev64": dict(kind="dev", seed=15, hidden=64, out=16, layers=3, tying=False, data="fixture"),
    "dev128": dict(kind="dev", seed=16, hidden=128, out=32, layers=2, tying=True, data="fixture"),
}


def case_params(c, concat_hidden=False, prefix=""):
    return make_params(c["kind"], c["seed"], c["hidden"], c["out"], c["layers"], c["tying"], concat_hidden, prefix=prefix)


def case_forward(c, params, atoms, adj, concat_hidden=False, step_keep=None, prefix=""):
    return forward(c["kind"], params, atoms, adj, c["layers"], c["tying"], concat_hidden, step_keep=step_keep, prefix=prefix)


def keep_rows(name, hidden, steps, seed, p):
    """``steps`` dropout masks on the packed rows of data set ``name`` ((n_rows, hidden) float32, values 0 or 1 / (1 - p)): the
    pad row of a molecule carries one mask for all its padded positions."""
    g = torch.Generator().manual_seed(seed)
    n = data(name)["pb"].n_rows
    return [(torch.rand(n, hidden, generator=g) >= p).float() * (1.0 / (1.0 - p)) for _ in range(steps)]
