"""Dense restatement of the reference's GGNN with message_function='edge_network' (models/ggnn.py:92-97, 245-248 and EdgeNetwork,
:657-720), in the dtype of the parameters it is given (float64 for reference values, float32 for the error estimate beside
CASES), on top of oracle.ref_cpu's stateful GRU and readout and agg_ref's layer aggregators.

    h0 = h = embed[atoms]                                                          (mb, A, d)
    per step:  m = edge_message(h, adj, message_layers[l]/output_layer),  l = 0 if tying else step
               s = stateful_gru([h, m], s)      (first call after reset: z * tanh(W x), no r gate and no U terms)
               h = step_keep * s                (F.dropout(h, dropout_rate), training only; the GRU keeps the un-dropped s)
    g = readout(h_T, h0) -- cat_t readout_t(h_t, h0) with concat_hidden, layer_aggregation(h_1..h_T) with an aggregator.
    Nothing is masked: padded positions (id 0, no bonds) receive a message (B . S) and count in every sum.

``edge_message_dense`` is EdgeNetwork.__call__ op for op: one d x d matrix per atom PAIR, an (mb A A, d d) tensor -- 13 x 30 x 30
pairs at d = 128 are 1.5 GB in float64 for one step of one side, and autograd keeps every step's.  ``edge_message_closed`` is the
same arithmetic regrouped (the network is affine in the adjacency vector of a pair):

    m_i = sum_e W_e . (sum_j adj[e, i, j] h_j) + B . S,   W_e[p, q] = W[p d + q, e],  B[p, q] = b[p d + q],  S = sum over ALL j of h_j

tests/test_edge_ref.py holds the two to 1e-12 of each other in float64 on every data set below; ``forward`` takes the op-for-op
form while the per-pair tensor has at most DENSE_MAX_ELEMS elements and the closed form above that.

Parameter names are the link paths of the reference: embed/W, message_layers/{i}/output_layer/{W [d d x 4], b [d d]},
message_layers/{i}/hidden_layers/0/{W [edge_hidden x 4], b} (built and never called), update_layer/{W_r,W_z,W,U_r,U_z,U}/{W,b},
i_layers/{k}/{W,b}, j_layers/{k}/{W,b}, attn_dense_layer/{W,b} ('attn').  No bias_add_layer: the reference never gives it a shape.

PARAMETER SCALES.  Chainer's LeCunNormal on output_layer's fan-in of 4 has std 0.5: a message of about 6 |h| at d = 128, which
saturates the GRU, and a saturated gate hides a wrong message.  ``make_params`` draws W with std wscale / sqrt(d) and b with std
bscale / (A_typ sqrt(d)) (S grows with the padded atom count); every case keeps at least half of its last step's update-gate
values inside (0.05, 0.95) in float64 (tests/test_edge_ref.py asserts it).
"""
import math

import numpy as np
import torch

from oracle import ref_cpu as O
import agg_ref as AG
import gin_ref as _G
from gin_ref import keep_dense          # noqa: F401

DENSE_MAX_ELEMS = 1 << 24          # 128 MB in float64, per step and side; autograd keeps two of them


def edge_message_dense(h, adj, W, b):
    """EdgeNetwork.__call__ (models/ggnn.py:685-720) with n_hidden_layers = 0, op for op."""
    mb, n_et, atoms, _ = adj.shape
    d = h.shape[2]
    a = adj.permute(0, 2, 3, 1).reshape(mb * atoms * atoms, n_et)                   # :689-690
    out = O.linear(a, W, b)                                                         # :700
    tmp = out.reshape(mb, atoms, atoms, d, d)                                       # :702
    big = tmp.permute(0, 1, 3, 2, 4).reshape(-1, atoms * d, atoms * d)              # :703-706
    mul = torch.matmul(big, h.reshape(mb, atoms * d, 1)).reshape(mb * atoms, d)     # :710-713
    return (mul + torch.zeros(d, dtype=h.dtype)).reshape(mb, atoms, d)              # :715-718: the bias is a constant zero


def edge_message_closed(h, adj, W, b):
    d = h.shape[2]
    We = W.reshape(d, d, 4)                                                         # [p, q, e]
    agg = torch.einsum("beij,bjq->beiq", adj, h)
    return torch.einsum("pqe,beiq->bip", We, agg) + (h.sum(dim=1) @ b.reshape(d, d).t())[:, None, :]


def make_params(seed, hidden, out, layers, tying, concat_hidden=False, n_atom_types=117, dtype=torch.float64, prefix="", bias=0.3,
                edge_hidden=16, wscale=0.5, bscale=0.5, a_typ=16, aggregator=None):
    """Fixed draw order: embed, the message layers (output_layer W, b, then hidden_layers/0 W, b), the GRU, the readout layers,
    attn_dense_layer."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    d = hidden
    p = {prefix + "embed/W": r(n_atom_types, d)}
    for i in range(1 if tying else layers):
        q = f"{prefix}message_layers/{i}/"
        p[q + "output_layer/W"] = r(d * d, 4) * (wscale / math.sqrt(d))
        p[q + "output_layer/b"] = r(d * d) * (bscale / (a_typ * math.sqrt(d)))
        p[q + "hidden_layers/0/W"] = r(edge_hidden, 4) * 0.5
        p[q + "hidden_layers/0/b"] = bias * r(edge_hidden)
    for n, k_in in (("W_r", 2 * d), ("W_z", 2 * d), ("W", 2 * d), ("U_r", d), ("U_z", d), ("U", d)):
        p[f"{prefix}update_layer/{n}/W"] = r(d, k_in) / math.sqrt(k_in)
        p[f"{prefix}update_layer/{n}/b"] = bias * r(d)
    ro = layers * d if aggregator == "concat" else d
    for k in range(layers if (concat_hidden and not aggregator) else 1):
        p[f"{prefix}i_layers/{k}/W"] = r(out, 2 * ro) / math.sqrt(2 * ro)
        p[f"{prefix}i_layers/{k}/b"] = bias * r(out)
        p[f"{prefix}j_layers/{k}/W"] = r(out, ro) / math.sqrt(ro)
        p[f"{prefix}j_layers/{k}/b"] = bias * r(out)
    if aggregator == "attn":
        p[f"{prefix}attn_dense_layer/W"] = r(layers, layers) / math.sqrt(layers)
        p[f"{prefix}attn_dense_layer/b"] = bias * r(layers)
    return {k: v.to(dtype) for k, v in p.items()}


def update_gate(sp, x, s):
    """z of chainer's StatefulGRU for the input x and the state s (None: the first call after reset)."""
    z = O.linear(x, sp["update_layer/W_z/W"], sp["update_layer/W_z/b"])
    if s is not None:
        z = z + O.linear(s, sp["update_layer/U_z/W"], sp["update_layer/U_z/b"])
    return torch.sigmoid(z)


def forward(params, atoms, adj, layers, tying=True, concat_hidden=False, step_keep=None, prefix="", aggregator=None, message=None,
            gates=None):
    """(g, [h_t]).  ``step_keep``: one (mb, A, d) multiplier per step (the dropout on the step's output), or None (evaluation
    mode).  ``message``: edge_message_dense / edge_message_closed, None = by size (DENSE_MAX_ELEMS).  ``gates`` (a list):
    receives every step's update gate z."""
    P = lambda k: params[prefix + k]
    dt = P("embed/W").dtype
    atoms = torch.as_tensor(np.asarray(atoms)).long()
    adj = torch.as_tensor(np.asarray(adj)).to(dt)
    h = P("embed/W")[atoms]
    h0 = h
    mb, A, d = h.shape
    if message is None:
        message = edge_message_dense if mb * A * A * d * d <= DENSE_MAX_ELEMS else edge_message_closed
    sp = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix + "update_layer/")}
    s = None
    hs, gs = [], []
    for step in range(layers):
        q = f"message_layers/{0 if tying else step}/output_layer/"
        m = message(h, adj, P(q + "W"), P(q + "b"))
        x = torch.cat((h.reshape(mb * A, d), m.reshape(mb * A, d)), dim=1)
        if gates is not None:
            gates.append(update_gate(sp, x, s).detach())
        s = O.stateful_gru(sp, "update_layer", x, s)
        h = s.reshape(mb, A, d)
        if step_keep is not None:
            h = h * step_keep[step].to(dt)
        hs.append(h)
        if concat_hidden and not aggregator:
            gs.append(O.ggnn_readout(h, h0, P(f"i_layers/{step}/W"), P(f"i_layers/{step}/b"), P(f"j_layers/{step}/W"),
                                     P(f"j_layers/{step}/b")))
    if aggregator:
        return AG.layer_aggregation(params, hs, h0, aggregator, prefix), hs
    if concat_hidden:
        return torch.cat(gs, dim=1), hs
    return O.ggnn_readout(h, h0, P("i_layers/0/W"), P("i_layers/0/b"), P("j_layers/0/W"), P("j_layers/0/b")), hs


# ---------------------------------------------------------------------------------------------------------
# data: gin_ref's sets ("fixture" 13 + 13 instances in three tiles, "small", "oversized") and two single-tile sets of the segment sum
# ---------------------------------------------------------------------------------------------------------
_DATA = {}


def data(name):
    if name not in ("many", "full"):
        return _G.data(name)
    if name in _DATA:
        return _DATA[name]
    from bmp import packed, synth
    if name == "many":          # 64 one-atom molecules: 64 segments of 2 rows (atom + pad row) fill the 128 rows of one tile
        store = synth.make_store(64, seed=31, n_lo=1, n_hi=1, n_mean=1)
    else:                       # one molecule of 127 atoms: with its pad row ONE segment that is a whole tile; five small ones beside it
        store = synth.make_store(1, seed=32, n_lo=127, n_hi=127, n_mean=127) + synth.make_store(5, seed=33, n_lo=2, n_hi=12, n_mean=6)
    idx = [np.arange(len(store))]
    pb = packed.pack_from_store(packed.MolStore(store), idx, device="cpu", with_dense_map=True)
    _DATA[name] = dict(store=store, idx=idx, pb=pb, sides=[synth.concat_mols(store)])
    return _DATA[name]


DATA_SETS = ("fixture", "small", "oversized", "many", "full")
A_TYP = {"fixture": 24, "small": 10, "oversized": 150, "many": 1, "full": 127}        # the padded atom counts, roughly


def keep_rows(name, hidden, steps, seed, p):
    """``steps`` dropout masks on the packed rows of data set ``name`` ((n_rows, hidden) float32, values 0 or 1 / (1 - p)): the
    pad row of a molecule carries one mask for all its padded positions."""
    g = torch.Generator().manual_seed(seed)
    n = data(name)["pb"].n_rows
    return [(torch.rand(n, hidden, generator=g) >= p).float() * (1.0 / (1.0 - p)) for _ in range(steps)]


# name: seed, hidden, out, layers, tying, data[, wscale, bscale].  Widths 16, 24 and 32 take the composed operators, 64 and 128 the
# fused kernels (1 layer: the first-call kernels alone; 3 layers: the later-call kernels twice).  Beside each row, as printed by
# ``python tests/edge_ref.py``: the share of the last step's update-gate values inside (0.05, 0.95) in float64, and the float32
# restatement's error against the float64 one, forward (g, atoms) and gradients, relative to the reference's maximum as
# parity_util.close takes it -- the GPU tests' bound is 1e-4, and a row whose error came within a factor 10 of it had its
# parameter scale shrunk (none came nearer than a factor 22).  Per row: gates; f32 forward / gradients.
CASES = {
    "edge16": dict(seed=1, hidden=16, out=16, layers=3, tying=True, data="fixture"),                            # gates 1.00; f32 1.1e-06 / 1.1e-06
    "edge24": dict(seed=2, hidden=24, out=12, layers=2, tying=False, data="fixture"),                           # gates 1.00; f32 6.4e-07 / 8.2e-07
    "edge32": dict(seed=3, hidden=32, out=16, layers=2, tying=False, data="fixture"),                           # gates 1.00; f32 9.5e-07 / 7.6e-07
    "edge64": dict(seed=4, hidden=64, out=32, layers=3, tying=False, data="fixture"),                           # gates 1.00; f32 5.8e-07 / 1.3e-06
    "edge128": dict(seed=5, hidden=128, out=64, layers=2, tying=True, data="fixture"),                          # gates 1.00; f32 6.3e-07 / 1.0e-06
    "edge64_1": dict(seed=6, hidden=64, out=16, layers=1, tying=True, data="fixture"),                          # gates 1.00; f32 1.1e-06 / 7.9e-07
    "edge128_1": dict(seed=17, hidden=128, out=16, layers=1, tying=True, data="fixture"),                       # gates 1.00; f32 6.7e-07 / 7.6e-07
    "edge64_3": dict(seed=18, hidden=64, out=16, layers=3, tying=True, data="fixture"),                         # gates 1.00; f32 5.3e-07 / 8.2e-07
    "edge128_3": dict(seed=7, hidden=128, out=16, layers=3, tying=False, data="fixture"),                       # gates 1.00; f32 6.3e-07 / 8.4e-07
    "edge_many64": dict(seed=19, hidden=64, out=16, layers=2, tying=False, data="many"),                        # gates 1.00; f32 3.2e-07 / 4.8e-07
    "edge_many128": dict(seed=20, hidden=128, out=16, layers=2, tying=True, data="many"),                       # gates 1.00; f32 3.2e-07 / 4.9e-07
    "edge_full64": dict(seed=21, hidden=64, out=16, layers=2, tying=True, data="full"),                         # gates 1.00; f32 4.7e-07 / 3.9e-06
    "edge_full128": dict(seed=22, hidden=128, out=16, layers=2, tying=False, data="full"),                      # gates 1.00; f32 6.5e-07 / 3.9e-06
    "edge_over16": dict(seed=8, hidden=16, out=8, layers=2, tying=False, data="oversized"),                     # gates 1.00; f32 2.3e-07 / 3.5e-06
    "edge_over64": dict(seed=9, hidden=64, out=16, layers=2, tying=False, data="oversized"),                    # gates 1.00; f32 5.3e-07 / 4.5e-06
    "edge_small16": dict(seed=10, hidden=16, out=8, layers=2, tying=False, data="small"),                       # gates 1.00; f32 5.1e-07 / 9.4e-07
    "edge_small64": dict(seed=11, hidden=64, out=16, layers=2, tying=True, data="small"),                       # gates 1.00; f32 7.0e-07 / 4.8e-07
    "edge_drop64": dict(seed=12, hidden=64, out=16, layers=3, tying=True, data="fixture"),                      # gates 1.00; f32 5.5e-07 / 7.1e-07
    "edge_attn64": dict(seed=14, hidden=64, out=16, layers=3, tying=True, data="fixture"),                      # gates 1.00; f32 7.3e-07 / 6.2e-07
    "edge_pair16": dict(seed=13, hidden=16, out=16, layers=2, tying=True, data="fixture"),                      # gates 1.00; f32 1.4e-06 / 9.8e-07
}


def case_params(c, concat_hidden=False, prefix="", aggregator=None, dtype=torch.float64):
    return make_params(c["seed"], c["hidden"], c["out"], c["layers"], c["tying"], concat_hidden, prefix=prefix, dtype=dtype,
                       wscale=c.get("wscale", 0.5), bscale=c.get("bscale", 0.5), a_typ=A_TYP[c["data"]], aggregator=aggregator)


def case_forward(c, params, atoms, adj, concat_hidden=False, step_keep=None, prefix="", aggregator=None, gates=None):
    return forward(params, atoms, adj, c["layers"], c["tying"], concat_hidden, step_keep=step_keep, prefix=prefix,
                   aggregator=aggregator, gates=gates)


def gate_share(c):
    """The share of the last step's update-gate values inside (0.05, 0.95), float64, over all sides of the case's data."""
    p = case_params(c)
    zs = []
    with torch.no_grad():
        for atoms, adj in data(c["data"])["sides"]:
            gates = []
            case_forward(c, p, atoms, adj, gates=gates)
            zs.append(gates[-1].reshape(-1))
    z = torch.cat(zs)
    return ((z > 0.05) & (z < 0.95)).double().mean().item()


def f32_error(c):
    """(forward, gradient) error of this restatement in float32 against itself in float64, each max|x32 - x64| / max|x64| over g,
    the atom states and (gradient) every parameter that is read, for the scalar <g, cg> + 0.1 <h_T, ca>."""
    out = {}
    for dt in (torch.float64, torch.float32):
        p = {k: v.requires_grad_() for k, v in case_params(c, dtype=dt).items()}
        gen = torch.Generator().manual_seed(5)
        s, keep = 0.0, []
        for atoms, adj in data(c["data"])["sides"]:
            g, hs = case_forward(c, p, atoms, adj)
            cg = torch.randn(g.shape, dtype=torch.float64, generator=gen).to(dt)
            ca = torch.randn(hs[-1].shape, dtype=torch.float64, generator=gen).to(dt)
            s = s + (g * cg).sum() + 0.1 * (hs[-1] * ca).sum()
            keep += [g.detach().double(), hs[-1].detach().double()]
        s.backward()
        out[dt] = (keep, {k: v.grad.double() for k, v in p.items() if v.grad is not None})
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()
    fwd = max(rel(a, b) for a, b in zip(out[torch.float32][0], out[torch.float64][0]))
    grd = max(rel(out[torch.float32][1][k], v) for k, v in out[torch.float64][1].items())
    return fwd, grd


if __name__ == "__main__":
    import sys          # (run with the repository root, gcn-bmp_amd and tests on PYTHONPATH)
    for name, c in CASES.items():
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        fwd, grd = f32_error(c)
        print(f'"{name}": gates inside {gate_share(c):.2f}   float32 error forward {fwd:.1e}  gradients {grd:.1e}', flush=True)
