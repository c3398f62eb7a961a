"""Float64 restatement of the rectangular RelGCN layer's kernel contract (csrc/bmp_relgcn_rect.hip, include/bmp.h): the
gather-first forward, the transposed gathers G_e, gda = [G_0 | G_1 | G_2 | G_3 | dpre], o1 = h^T . gda with its slicing, dbE
and cs.  ``adj`` is dense, [4, N, N] with adj[e, dst, src]; WT [4 d_in x d_out] is K-major with type-major blocks.
tests/test_relgcn_rect_build.py checks it against torch autograd of the reference's order (linear, then adjacency:
models/update/relgcn_update.py:24-44); the GPU tests use it as their second reference."""
import torch

_ACT = {"identity": (lambda v: v, lambda y: torch.ones_like(y)),
        "tanh": (torch.tanh, lambda y: 1.0 - y * y)}


def layer_forward(h, adj, WT, bE, WsT, bs, act):
    """(out, wdeg [N x 4]): out = act(h . WsT + bs + sum_e (A_e . WT_e + wdeg_e * bE_e)), A_e = adj_e . h."""
    d_in = h.shape[1]
    wdeg = adj.sum(dim=2).t().contiguous()
    pre = h @ WsT + bs
    for e in range(4):
        pre = pre + (adj[e] @ h) @ WT[e * d_in:(e + 1) * d_in] + wdeg[:, e:e + 1] * bE[e]
    return _ACT[act][0](pre), wdeg


def layer_backward(dout, out, h, wdeg, adj, WT, WsT, act):
    """dict(dh, gda, o1, dbE, cs, dWT, dWsT, dbs) from the kernel's own operands."""
    d_in, d_out = WsT.shape
    dpre = dout * _ACT[act][1](out)
    G = [adj[e].t() @ dpre for e in range(4)]
    dh = dpre @ WsT.t()
    for e in range(4):
        dh = dh + G[e] @ WT[e * d_in:(e + 1) * d_in].t()
    gda = torch.cat(G + [dpre], dim=1)
    o1 = h.t() @ gda
    cs = gda.sum(dim=0)
    return dict(dh=dh, gda=gda, o1=o1, dbE=wdeg.t() @ dpre, cs=cs,
                dWT=o1[:, :4 * d_out].reshape(d_in, 4, d_out).permute(1, 0, 2).reshape(4 * d_in, d_out),
                dWsT=o1[:, 4 * d_out:], dbs=cs[4 * d_out:])


def layer(h, adj, WT, bE, WsT, bs, act, cot):
    """Forward and backward under the cotangent ``cot``: (out, dict(dx, dWT, dbE, dWsT, dbs))."""
    out, wdeg = layer_forward(h, adj, WT, bE, WsT, bs, act)
    b = layer_backward(cot, out, h, wdeg, adj, WT, WsT, act)
    return out, dict(dx=b["dh"], dWT=b["dWT"], dbE=b["dbE"], dWsT=b["dWsT"], dbs=b["dbs"])


def reference_order(h, adj, WT, bE, WsT, bs, act):
    """The reference's order: out = act(h W_s^T + b_s + sum_e adj_e @ (h W_e^T + b_e)), differentiable."""
    d_in = h.shape[1]
    pre = h @ WsT + bs
    for e in range(4):
        pre = pre + adj[e] @ (h @ WT[e * d_in:(e + 1) * d_in] + bE[e])
    return _ACT[act][0](pre)


def molecules_adj(sizes, seed, scale=True):
    """Dense [4, N, N] adjacency of chain molecules of ``sizes`` atoms with cycling bond types and positive random values
    (scale: divided by the source atom's degree, as rescale_adj), block diagonal."""
    N = sum(sizes)
    g = torch.Generator().manual_seed(seed)
    adj = torch.zeros(4, N, N, dtype=torch.float64)
    o = 0
    for n in sizes:
        for i in range(n - 1):
            v = 0.5 + torch.rand((), generator=g, dtype=torch.float64)
            adj[(i + n) % 4, o + i, o + i + 1] = v
            adj[(i + n) % 4, o + i + 1, o + i] = v
        o += n
    if scale:
        deg = adj.sum(dim=(0, 1))
        adj = adj / torch.where(deg != 0, deg, torch.ones_like(deg))[None, None, :]
    return adj
