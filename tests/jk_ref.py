"""Dense restatement of the reference's two jumping-knowledge GGNN encoders, op for op, in the dtype of the parameters it is given
(float64 for reference values): models/ggnn_dev_jknet.py (kind "jknet") and models/ggnn_dev_jk_gru.py (kind "jk_gru").  The dense
(mb, 4, A, A) adjacency, every padded position unmasked, chainer's first-call GRU branch.

    h0 = h = embed[atoms]                                                          (mb, A, d)
    per step:  m = ggnn_message(h, adj, message_layers[0 if tying else step])      (oracle.ref_cpu, models/ggnn.py's message)
       jknet:  h = relu(update_layer[u] [h, m]),  u = 0 if update_tying else step               (ggnn_dev_jknet.py:104-105,139)
       jk_gru: m = m + linear(h, self_loop_layer)   (self_loop; ONE layer)                      (ggnn_dev_jk_gru.py:106-107)
               x = relu(update_layers_0[u] [h, m]),  u = 0 if TYING else step  (the wrong flag) (:80,117)
               s = stateful_gru(x, s)   (first call after reset: z * tanh(W x), no r gate and no U terms);  h = s
               h = step_keep * h  (F.dropout(h, dropout_rate), training only; the GRU keeps the un-dropped s)
               concat_hidden: g_list += ggnn_readout(h, h0, step)
    jknet, without concat_hidden:  y = aggr([h_1 .. h_T]);  g = ggnn_readout(y, h0, 0)                    (:175-183)
       'max'  y = max_t h_t      'mean'  y = mean_t h_t      'concat'  y = cat_t h_t (the readout links take it for T = 1 only)
       'attn' E_t = <H_t, H_T> + <H_t, H_1> over ALL mb * A * d elements of the call, c = softmax_t(E), y = sum_t c_t H_t    (:304-344)
    readout = sum over ALL A positions of sigmoid(i([h, h0])) * j(h): padded positions (id 0, no bonds) count everywhere.

Parameter names are the link paths of the reference: embed/W, message_layers/{i}/{W,b}, update_layer/{k}/{W,b} (jknet) or
update_layers_0/{k}/{W,b}, update_layer/{W_r,W_z,W,U_r,U_z,U}/{W,b}, self_loop_layer/{W,b} (jk_gru), i_layers/{k}/{W,b},
j_layers/{k}/{W,b}.

``scale``: the network up to the readout is positively homogeneous of degree 1 in (embed, every bias of the message and the
update), so scaling those by s scales every h_t by s and the 'attn' energies by s^2 -- the handle that keeps the softmax over the
energies (sums over tens of thousands of elements) away from saturation without making any step degenerate.
"""
import math

import numpy as np
import torch

from oracle import ref_cpu as O
from ggate32_ref import data            # noqa: F401  ("fixture", "small", "oversized" of gin_ref; "blocks" and "dense")


def make_params(kind, seed, hidden, out, layers, tying, update_tying=True, concat_hidden=False, self_loop=False, scale=1.0,
                n_atom_types=117, dtype=torch.float64, prefix="", bias=0.3):
    """Fixed draw order: embed, the message layers, the update layers, (jk_gru) the GRU and the self loop, the readout layers."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    d = hidden
    p = {prefix + "embed/W": scale * r(n_atom_types, d)}
    for i in range(1 if tying else layers):
        p[f"{prefix}message_layers/{i}/W"] = r(4 * d, d) / math.sqrt(d) * 0.5
        p[f"{prefix}message_layers/{i}/b"] = scale * bias * r(4 * d)
    nu = d if kind == "jknet" else 2 * d
    name = "update_layer" if kind == "jknet" else "update_layers_0"
    for k in range(1 if update_tying else layers):
        p[f"{prefix}{name}/{k}/W"] = r(nu, 2 * d) / math.sqrt(2 * d)
        p[f"{prefix}{name}/{k}/b"] = scale * bias * r(nu)
    if kind == "jk_gru":
        for n, k_in in (("W_r", 2 * d), ("W_z", 2 * d), ("W", 2 * d), ("U_r", d), ("U_z", d), ("U", d)):
            p[f"{prefix}update_layer/{n}/W"] = r(d, k_in) / math.sqrt(k_in)
            p[f"{prefix}update_layer/{n}/b"] = bias * r(d)
        if self_loop:
            p[f"{prefix}self_loop_layer/W"] = r(d, d) / math.sqrt(d) * 0.5
            p[f"{prefix}self_loop_layer/b"] = bias * r(d)
    for k in range(layers if concat_hidden else 1):
        p[f"{prefix}i_layers/{k}/W"] = r(out, 2 * d) / math.sqrt(2 * d)
        p[f"{prefix}i_layers/{k}/b"] = bias * r(out)
        p[f"{prefix}j_layers/{k}/W"] = r(out, d) / math.sqrt(d)
        p[f"{prefix}j_layers/{k}/b"] = bias * r(out)
    return {k: v.to(dtype) for k, v in p.items()}


def attn_energies(hs):
    """E [T]: <H_t, H_T> + <H_t, H_1> over all elements (ggnn_dev_jknet.py:314-318, 336-343)."""
    key = torch.stack([h.reshape(-1) for h in hs])                          # (T, mb * A * d)
    return key @ hs[-1].reshape(-1) + key @ hs[0].reshape(-1)


def aggregate(aggr, hs):
    """(y, coefficients [T] or None)."""
    if aggr == "concat":
        return torch.cat(hs, dim=-1), None
    if aggr == "max":                    # F.max's backward as agg_ref restates it: dy to every position equal to the maximum
        from agg_ref import layer_aggregate
        return layer_aggregate(hs, "max-pool"), None
    st = torch.stack(hs, dim=-2)                                             # (mb, A, T, d)
    if aggr == "mean":
        return st.mean(dim=-2), None
    assert aggr == "attn"
    c = torch.softmax(attn_energies(hs), dim=0)
    return sum(c[t] * hs[t] for t in range(len(hs))), c


def forward(kind, params, atoms, adj, layers, tying=True, update_tying=True, concat_hidden=False, aggr=None, self_loop=False,
            step_keep=None, prefix="", pre=None, states=None):
    """(g, atoms the readout read, coefficients or None).  ``step_keep``: one (mb, A, d) multiplier per step (the dropout on the
    step's output), or None (evaluation mode).  ``pre``: a list that receives every relu's pre-activations; ``states``: one that
    receives the step outputs h_1 .. h_T."""
    P = lambda k: params[prefix + k]
    dt = P("embed/W").dtype
    atoms = torch.as_tensor(np.asarray(atoms)).long()
    adj = torch.as_tensor(np.asarray(adj)).to(dt)
    h = P("embed/W")[atoms]
    h0 = h
    mb, A, d = h.shape
    sp = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix + "update_layer/")}
    s = None
    hs, g_list = [], []
    for step in range(layers):
        li = 0 if tying else step
        m = O.ggnn_message(h, adj, P(f"message_layers/{li}/W"), P(f"message_layers/{li}/b"))
        if kind == "jknet":
            u = 0 if update_tying else step
            a = O.linear(torch.cat((h.reshape(mb * A, d), m.reshape(mb * A, d)), dim=1), P(f"update_layer/{u}/W"), P(f"update_layer/{u}/b"))
            if pre is not None:
                pre.append(a.detach())
            h = torch.relu(a).reshape(mb, A, d)
        else:
            if self_loop:
                m = m + O.linear(h, P("self_loop_layer/W"), P("self_loop_layer/b"))
            u = 0 if tying else step                                         # ggnn_dev_jk_gru.py:80
            a = O.linear(torch.cat((h.reshape(mb * A, d), m.reshape(mb * A, d)), dim=1), P(f"update_layers_0/{u}/W"),
                         P(f"update_layers_0/{u}/b"))
            if pre is not None:
                pre.append(a.detach())
            s = O.stateful_gru(sp, "update_layer", torch.relu(a), s)
            h = s.reshape(mb, A, d)
        if step_keep is not None:
            h = h * step_keep[step].to(dt)
        if concat_hidden:
            g_list.append(O.ggnn_readout(h, h0, P(f"i_layers/{step}/W"), P(f"i_layers/{step}/b"),
                                         P(f"j_layers/{step}/W"), P(f"j_layers/{step}/b")))
        hs.append(h)
    if states is not None:
        states.extend(hs)
    if concat_hidden:
        return torch.cat(g_list, dim=1), h, None
    y, c = (h, None) if kind == "jk_gru" else aggregate(aggr, hs)
    return O.ggnn_readout(y, h0, P("i_layers/0/W"), P("i_layers/0/b"), P("j_layers/0/W"), P("j_layers/0/b")), y, c


# name: kind, seed, hidden, out, layers, tying, update_tying, aggr (jknet), loop (jk_gru), scale, data.  Widths 16, 24 and 32 take the
# composed operators, 64 and 128 the fused kernels; "fixture" has all four bond types, rows lacking a type, pad rows of multiplicity
# > 1, three tiles and two batch sides; "oversized" one molecule larger than a tile; "blocks" / "dense": ggate32_ref's docstring.
# The seed of a row is the first >= its starting value that meets the relu kink condition with KINK_FACTOR (``python
# tests/jk_ref.py`` searches and prints); ``scale`` of an 'attn' row keeps its coefficients inside ATTN_COEF_RANGE.
# Beside each row: the kink margin min |pre64| / max |pre32 - pre64| over its relus, then the worst max-norm relative distance of the
# float32 restatement from the float64 one over g, the atom states and every parameter gradient, against F32_BOUND
# (tests/test_jk_ref.py prints both with -s).
KINK_FACTOR = 8.0
ATTN_COEF_RANGE = (0.02, 0.95)
F32_BOUND = 1e-5


def _c(kind, seed, hidden, out, layers, tying, update_tying, data, aggr=None, loop=False, scale=1.0):
    return dict(kind=kind, seed=seed, hidden=hidden, out=out, layers=layers, tying=tying, update_tying=update_tying, data=data,
                aggr=aggr, loop=loop, scale=scale)


CASES = {
    "max64": _c("jknet", 1, 64, 32, 3, True, True, "fixture", aggr="max"),  # 38 x, 8.3e-07
    "mean64": _c("jknet", 2, 64, 32, 3, False, True, "fixture", aggr="mean"),  # 36 x, 7.3e-07
    "attn64": _c("jknet", 3, 64, 32, 3, True, False, "fixture", aggr="attn", scale=0.01),  # 10 x, 1.2e-06
    "attn64u": _c("jknet", 6, 64, 16, 3, False, False, "fixture", aggr="attn", scale=0.01),  # 32 x, 1.3e-06
    "attn128": _c("jknet", 6, 128, 64, 2, True, True, "fixture", aggr="attn", scale=0.01),  # 13 x, 8.2e-07
    "concat64": _c("jknet", 6, 64, 16, 1, True, True, "fixture", aggr="concat"),  # 368 x, 9.3e-07
    "gru64": _c("jk_gru", 7, 64, 32, 3, True, True, "fixture", loop=True),  # 14 x, 8.5e-07
    "gru64u": _c("jk_gru", 11, 64, 16, 3, False, False, "fixture", loop=True),  # 14 x, 1.0e-06
    "gru128": _c("jk_gru", 25, 128, 64, 2, True, True, "fixture"),  # 10 x, 7.7e-07
    "gru64t": _c("jk_gru", 31, 64, 16, 2, True, False, "fixture"),  # 8 x, 1.2e-06
    "attn16": _c("jknet", 10, 16, 16, 3, True, True, "fixture", aggr="attn", scale=0.03),  # 102 x, 1.0e-06
    "mean24": _c("jknet", 11, 24, 12, 2, False, False, "fixture", aggr="mean"),  # 9 x, 1.5e-06
    "gru32": _c("jk_gru", 12, 32, 16, 2, True, True, "fixture", loop=True),  # 80 x, 1.5e-06
    "attn_over64": _c("jknet", 13, 64, 16, 2, False, True, "oversized", aggr="attn", scale=0.01),  # 20 x, 5.3e-06
    "gru_over64": _c("jk_gru", 15, 64, 16, 2, True, True, "oversized", loop=True),  # 27 x, 8.3e-06
    "attn_blocks64": _c("jknet", 15, 64, 16, 2, False, True, "blocks", aggr="attn", scale=0.01),  # 58 x, 1.6e-06
    "gru_blocks64": _c("jk_gru", 16, 64, 16, 2, True, True, "blocks", loop=True),  # 70 x, 1.6e-06
    "max_dense64": _c("jknet", 17, 64, 16, 2, False, True, "dense", aggr="max"),  # 28 x, 5.6e-07
    "gru_dense64": _c("jk_gru", 20, 64, 16, 2, True, True, "dense"),  # 14 x, 7.4e-07
    "attn_small64": _c("jknet", 19, 64, 16, 2, True, True, "small", aggr="attn", scale=0.05),  # 20 x, 5.1e-07
    "gru_small64": _c("jk_gru", 22, 64, 16, 2, True, True, "small", loop=True),  # 60 x, 4.7e-07
    "attn_drop64": _c("jknet", 21, 64, 16, 2, True, True, "fixture", aggr="attn", scale=0.01),  # 29 x, 7.8e-07
    "gru_drop64": _c("jk_gru", 31, 64, 16, 3, True, True, "fixture", loop=True),  # 8 x, 7.8e-07
    "attn_pair64": _c("jknet", 23, 64, 16, 2, True, True, "fixture", aggr="attn", scale=0.01),  # 15 x, 1.7e-06
    "gru_pair64": _c("jk_gru", 24, 64, 16, 2, True, True, "fixture", loop=True),  # 9 x, 9.1e-07
}
DROP_P = 0.25               # the training-dropout cases' ratio (masks 0 or 1 / 0.75)


def case_params(c, concat_hidden=False, prefix=""):
    return make_params(c["kind"], c["seed"], c["hidden"], c["out"], c["layers"], c["tying"], c["update_tying"], concat_hidden,
                       c["loop"], c["scale"], prefix=prefix)


def case_forward(c, params, atoms, adj, concat_hidden=False, step_keep=None, prefix="", pre=None):
    return forward(c["kind"], params, atoms, adj, c["layers"], c["tying"], c["update_tying"], concat_hidden, c["aggr"], c["loop"],
                   step_keep=step_keep, prefix=prefix, pre=pre)


def keep_rows(name, hidden, steps, seed, p=DROP_P):
    """``steps`` dropout masks on the packed rows of data set ``name`` ((n_rows, hidden) float32, values 0 or 1 / (1 - p)): the
    pad row of a molecule carries one mask for all its padded positions."""
    g = torch.Generator().manual_seed(seed)
    n = data(name)["pb"].n_rows
    return [(torch.rand(n, hidden, generator=g) >= p).float() * (1.0 / (1.0 - p)) for _ in range(steps)]


def keep_dense_of(name, rows, side):
    dm = data(name)["pb"].dense_maps[side]
    return [k[dm] for k in rows]


def reference(name, concat=False, keep_seed=None, dtype=torch.float64):
    """The restatement of a case on every side of its data (one encoder call per side), differentiated once:
    dict(p (leaves with .grad), g, atoms [per side], coef [per side], cg, ca, keep (row masks or None))."""
    c = CASES[name]
    d = data(c["data"])
    p = {k: v.to(dtype).requires_grad_() for k, v in case_params(c, concat).items()}
    kr = None if keep_seed is None else keep_rows(c["data"], c["hidden"], c["layers"], keep_seed)
    outs = []
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else keep_dense_of(c["data"], kr, side)
        outs.append(case_forward(c, p, atoms, adj, concat, step_keep=kd))
    g = torch.cat([o[0] for o in outs])
    gen = torch.Generator().manual_seed(5)
    cg = torch.randn(g.shape, dtype=torch.float64, generator=gen)
    ca = [torch.randn(o[1].shape, dtype=torch.float64, generator=gen) for o in outs]
    ((g * cg.to(dtype)).sum() + 0.1 * sum((o[1] * w.to(dtype)).sum() for o, w in zip(outs, ca))).backward()
    return dict(p=p, g=g.detach(), atoms=[o[1].detach() for o in outs], coef=[None if o[2] is None else o[2].detach() for o in outs],
                cg=cg, ca=ca, keep=kr)


def kink_margin(c, keep_seed=None):
    """(min |pre64|, max |pre32 - pre64|) over every relu pre-activation of the case on all its sides."""
    d = data(c["data"])
    p64 = case_params(c)
    p32 = {k: v.float() for k, v in p64.items()}
    kr = None if keep_seed is None else keep_rows(c["data"], c["hidden"], c["layers"], keep_seed)
    lo, err = float("inf"), 0.0
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else keep_dense_of(c["data"], kr, side)
        a, b = [], []
        with torch.no_grad():
            case_forward(c, p64, atoms, adj, step_keep=kd, pre=a)
            case_forward(c, p32, atoms, adj, step_keep=kd, pre=b)
        for x, y in zip(a, b):
            lo = min(lo, x.abs().min().item())
            err = max(err, (y.double() - x).abs().max().item())
    return lo, err


KEEP_SEEDS = {"attn_drop64": 11, "gru_drop64": 12, "attn_pair64": 13, "gru_pair64": 14}       # the cases run with given masks


def kink_ok(c, keep_seed=None):
    lo, err = kink_margin(c, keep_seed)
    return lo >= KINK_FACTOR * err


# ---- one training step of the pair model cut down: encoder -> MLP link predictor on [g1 | g2] (no co-attention) ----
PAIR_HIDDEN_DIMS = (32, 16)


def pair_params(name, dtype=torch.float64):
    c = CASES[name]
    p = case_params(c, prefix="graph_conv/")
    g = torch.Generator().manual_seed(41)
    dims = [2 * c["out"]] + list(PAIR_HIDDEN_DIMS) + [1]
    for i in range(len(dims) - 1):
        key = f"mlp/layers/{i}" if i < len(PAIR_HIDDEN_DIMS) else "mlp/l_out"
        p[key + "/W"] = torch.randn(dims[i + 1], dims[i], dtype=torch.float64, generator=g) / math.sqrt(dims[i])
        p[key + "/b"] = 0.3 * torch.randn(dims[i + 1], dtype=torch.float64, generator=g)
    return {k: v.to(dtype) for k, v in p.items()}


def pair_labels():
    return np.random.RandomState(4).randint(0, 2, (13, 1)).astype(np.int32)


def pair_reference(name, dtype=torch.float64):
    """dict(p, keep, y, loss, grads {name: tensor}) of one training-mode forward and backward of the pair model on "fixture" with
    the masks given."""
    c = CASES[name]
    d = data(c["data"])
    q = {k: v.clone().requires_grad_() for k, v in pair_params(name, dtype).items()}
    kr = keep_rows(c["data"], c["hidden"], c["layers"], KEEP_SEEDS[name])
    g = [case_forward(c, q, *d["sides"][s], step_keep=keep_dense_of(c["data"], kr, s), prefix="graph_conv/")[0] for s in (0, 1)]
    h = torch.cat(g, dim=1)
    for i in range(len(PAIR_HIDDEN_DIMS)):
        h = torch.relu(h @ q[f"mlp/layers/{i}/W"].t() + q[f"mlp/layers/{i}/b"])
    y = h @ q["mlp/l_out/W"].t() + q["mlp/l_out/b"]
    loss = O.sigmoid_cross_entropy(y, torch.from_numpy(pair_labels()))
    names = sorted(q)
    gr = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    grads = {n: (x if x is not None else torch.zeros_like(q[n])) for n, x in zip(names, gr)}
    return dict(p=q, keep=kr, y=y.detach(), loss=loss.detach(), grads=grads)


if __name__ == "__main__":
    import os
    import sys
    HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "gcn-bmp_amd")]
    for name, c in CASES.items():
        ks = KEEP_SEEDS.get(name)
        seed = next(s for s in range(c["seed"], 4000) if kink_ok(dict(c, seed=s), ks))
        lo, err = kink_margin(dict(c, seed=seed), ks)
        line = f'"{name}": seed={seed}  min|pre64| {lo:.3e}  max|pre32-pre64| {err:.3e}  margin {lo / err:.1f}x'
        if c["aggr"] == "attn":
            r = reference(name, keep_seed=ks) if seed == c["seed"] else None
            if r is not None:
                line += "  coef " + " | ".join(" ".join(f"{x:.3f}" for x in co.tolist()) for co in r["coef"])
        print(line, flush=True)
