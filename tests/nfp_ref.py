"""Dense float64 restatement of the neural-fingerprint encoder (the reference's models/models/nfp.py), written from its
description, plus the same computation on the PACKED layout (virtual pad row with multiplicity) for the layout tests.

    h = embed[atoms]                                              (mb, A, d)
    deg = column sums of adj, in float32 as given                 (mb, A); class k iff deg == k, k in 1..7
    per layer l:  fv = adj @ h;  h = sigmoid(sum_k where(deg == k, fv, 0) W_lk^T + b_lk)     (every bias on every position)
                  g += sum over ALL A positions of softmax_channels(h Wo_l^T + bo_l)
    returns g (mb, o) and the last h.  Nothing is masked: padded positions (id 0, empty row and column) count everywhere.

Parameter names are the link paths of the reference: embed/W, layers/{l}/graph_linears/{k}/{W,b},
read_out_layers/{l}/output_weight/{W,b}; Linear weights are [out x in].
"""
import math

import numpy as np
import torch

N_DEG = 7


def make_nfp_params(seed, hidden_dim, out_dim, n_layers, n_atom_types=117, dtype=torch.float64, prefix="", bias=0.3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    p = {prefix + "embed/W": r(n_atom_types, hidden_dim)}
    for l in range(n_layers):
        for k in range(N_DEG):
            p[f"{prefix}layers/{l}/graph_linears/{k}/W"] = r(hidden_dim, hidden_dim) / math.sqrt(hidden_dim)
            p[f"{prefix}layers/{l}/graph_linears/{k}/b"] = bias * r(hidden_dim)
        p[f"{prefix}read_out_layers/{l}/output_weight/W"] = r(out_dim, hidden_dim) / math.sqrt(hidden_dim)
        p[f"{prefix}read_out_layers/{l}/output_weight/b"] = bias * r(out_dim)
    return {k: v.to(dtype) for k, v in p.items()}


def n_layers_of(p, prefix=""):
    return 1 + max(int(k[len(prefix):].split("/")[1]) for k in p if k.startswith(prefix + "layers/"))


def nfp_adj(mols, A=None):
    """The stock ``nfp`` preprocessor's batch: atoms (mb, A) int32 and ONE adjacency (mb, A, A) float32 -- 1 per bond
    whatever its type plus the identity on the real atoms, zero padded."""
    A = max(m.n for m in mols) if A is None else A
    atoms = np.zeros((len(mols), A), dtype=np.int32)
    adj = np.zeros((len(mols), A, A), dtype=np.float32)
    for b, m in enumerate(mols):
        atoms[b, :m.n] = m.atoms
        if len(m.bonds):
            adj[b, m.bonds[:, 0], m.bonds[:, 1]] = 1.0
            adj[b, m.bonds[:, 1], m.bonds[:, 0]] = 1.0
        adj[b, np.arange(m.n), np.arange(m.n)] = 1.0
    return atoms, adj


def deg_class(adj):
    """(mb, A) int64: k in 1..7 where the float32 column sum equals k, else 0."""
    deg = torch.as_tensor(adj).to(torch.float32).sum(dim=1)
    cls = torch.zeros(deg.shape, dtype=torch.int64)
    for k in range(1, N_DEG + 1):
        cls[deg == float(k)] = k
    return cls


def nfp_forward(params, atoms, adj, prefix=""):
    p = params
    nl = n_layers_of(p, prefix)
    atoms = torch.as_tensor(atoms).long()
    cls = deg_class(adj)
    dt = p[prefix + "embed/W"].dtype
    adj = torch.as_tensor(adj).to(dt)
    h = p[prefix + "embed/W"][atoms]
    g = 0
    for l in range(nl):
        fv = adj @ h
        pre = 0
        for k in range(N_DEG):
            W, b = p[f"{prefix}layers/{l}/graph_linears/{k}/W"], p[f"{prefix}layers/{l}/graph_linears/{k}/b"]
            fvd = torch.where((cls == k + 1)[:, :, None], fv, torch.zeros_like(fv))
            pre = pre + fvd @ W.t() + b
        h = torch.sigmoid(pre)
        Wo, bo = p[f"{prefix}read_out_layers/{l}/output_weight/W"], p[f"{prefix}read_out_layers/{l}/output_weight/b"]
        g = g + torch.softmax(h @ Wo.t() + bo, dim=2).sum(dim=1)
    return g, h


def nfp_forward_packed(params, pb, nd, prefix=""):
    """The same on a host PackedMolBatch with its derived NFP data ``nd`` (bmp.nfp.nfp_derived): rows instead of
    positions, one pad row per molecule weighted row_w in the readout.  Returns (g (n_mols, o), h (N, d))."""
    p = params
    nl = n_layers_of(p, prefix)
    dt = p[prefix + "embed/W"].dtype
    N = pb.n_rows
    h = p[prefix + "embed/W"][pb.atom_id.long()]
    src = (pb.csr_col >> 2).long()
    dst = torch.repeat_interleave(torch.arange(N), (pb.csr_ptr[1:] - pb.csr_ptr[:-1]).long())
    val = pb.csr_val.to(dt)
    self_w, cls, row_w = nd["self_w"].to(dt), nd["deg_class"].long(), pb.row_w.to(dt)
    live = pb.row_mol.long() >= 0
    mol = pb.row_mol.long()[live]
    g = 0
    for l in range(nl):
        fv = (self_w[:, None] * h).index_add(0, dst, val[:, None] * h[src])
        d = h.shape[1]
        Ws = torch.stack([torch.zeros(d, d, dtype=dt)] + [p[f"{prefix}layers/{l}/graph_linears/{k}/W"].t() for k in range(N_DEG)])
        B = sum(p[f"{prefix}layers/{l}/graph_linears/{k}/b"] for k in range(N_DEG))
        h = torch.sigmoid(torch.einsum("nk,nkc->nc", fv, Ws[cls]) + B)
        Wo, bo = p[f"{prefix}read_out_layers/{l}/output_weight/W"], p[f"{prefix}read_out_layers/{l}/output_weight/b"]
        s = torch.softmax(h @ Wo.t() + bo, dim=1) * row_w[:, None]
        g = g + torch.zeros(pb.n_mols, s.shape[1], dtype=dt).index_add(0, mol, s[live])
    return g, h
