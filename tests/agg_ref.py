"""Dense float64 restatement of the GGNN layer aggregators (the reference's models/ggnn.py:154-213, 407-579, 637-644),
written from their description on top of oracle.ref_cpu's message / GRU / readout functions, plus the same computation on
the PACKED layout (virtual pad row with multiplicity) for the layout tests.

With ``layer_aggregator`` set the encoder collects the step outputs h_1..h_T (after dropout, if any) and returns

    concat:    g = readout(concat(h_1..h_T, axis=-1), concat([h0] * T, axis=-1))     i_layers/0: (out, 2 T d), j_layers/0: (out, T d)
    max-pool:  g = readout(max_t h_t, h0)
    attn:      z_s = sum_t W[s, t] h_t + b_s  per (molecule, position, channel), W = attn_dense_layer/W (T, T) on the LAYER axis;
               p = softmax_s(z);  g = readout(sum_s p_s h_s, h0)

through readout layer 0.  Nothing is masked: padded positions run through the steps and the aggregator like atoms.

The backward of the max is Chainer's F.max as recalled (third-party behaviour in the manner of SURVEY.md Appendix B, not
verifiable offline): the WHOLE upstream gradient goes to every position equal to the maximum.  Away from exact ties that is
the ordinary derivative.

Parameter names are the link paths of the reference (embed/W, message_layers/{i}/W, update_layer/W_r/W, i_layers/0/W,
attn_dense_layer/W, ...); Linear weights are [out x in].
"""
import torch

from oracle import ref_cpu as O

AGGREGATORS = ("concat", "max-pool", "attn")


class _MaxAllTies(torch.autograd.Function):
    """max over axis 0; backward: dy to every position that equals the maximum."""

    @staticmethod
    def forward(ctx, x):
        y = x.amax(dim=0)
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        return dy.unsqueeze(0) * (x == y.unsqueeze(0)).to(dy.dtype)


def layer_aggregate(h_list, aggregator, W=None, b=None):
    """What the readout reads in h's place: (..., d) [(..., T d) for concat] from the T tensors (..., d)."""
    if aggregator == "concat":
        return torch.cat(list(h_list), dim=-1)
    x = torch.stack(list(h_list), dim=0)                       # (T, ..., d)
    if aggregator == "max-pool":
        return _MaxAllTies.apply(x)
    if aggregator == "attn":
        z = torch.einsum("st,t...->s...", W, x)
        if b is not None:
            z = z + b.reshape((-1,) + (1,) * (x.dim() - 1))
        return (torch.softmax(z, dim=0) * x).sum(dim=0)
    raise ValueError(aggregator)


def _agg_params(p, aggregator, prefix):
    if aggregator != "attn":
        return None, None
    return p[prefix + "attn_dense_layer/W"], p.get(prefix + "attn_dense_layer/b")


def layer_aggregation(p, h_list, h0, aggregator, prefix=""):
    """models/ggnn.py:407-579 on dense (mb, A, d) arrays -> g (mb, out)."""
    y = layer_aggregate(h_list, aggregator, *_agg_params(p, aggregator, prefix))
    y0 = torch.cat([h0] * len(h_list), dim=-1) if aggregator == "concat" else h0
    P = lambda k: p[prefix + k]
    return O.ggnn_readout(y, y0, P("i_layers/0/W"), P("i_layers/0/b"), P("j_layers/0/W"), P("j_layers/0/b"))


def ggnn_agg_forward(p, atom_array, adj, n_layers, aggregator, weight_tying=True, prefix="", dropout_masks=None):
    """models/ggnn.py:584-644 with layer_aggregator set (the loop is oracle.ref_cpu.ggnn_forward's).  ``atom_array``: int
    ids (mb, A) or float features (mb, A, d).  Returns (g, h_list)."""
    P = lambda k: p[prefix + k]
    if atom_array.dtype in (torch.int32, torch.int64):
        h = P("embed/W")[atom_array.long()]
    else:
        h = atom_array
    h0 = h
    mb, atom, ch = h.shape
    s = None
    sp = {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix + "update_layer/")}
    h_list = []
    for step in range(n_layers):
        li = 0 if weight_tying else step
        m = O.ggnn_message(h, adj, P(f"message_layers/{li}/W"), P(f"message_layers/{li}/b"))
        x = torch.cat((h.reshape(mb * atom, ch), m.reshape(mb * atom, ch)), dim=1)
        s = O.stateful_gru(sp, "update_layer", x, s)
        h = s.reshape(mb, atom, ch)
        if dropout_masks is not None:
            h = h * dropout_masks[step]
        h_list.append(h)
    return layer_aggregation(p, h_list, h0, aggregator, prefix), h_list


def ggnn_agg_forward_packed(p, pb, n_layers, aggregator, weight_tying=True, prefix=""):
    """The same on a host PackedMolBatch: rows instead of positions, one pad row per molecule that stands for all its padded
    positions.  The aggregators act per row and channel, so the pad row stays exact and its multiplicity ``row_w`` enters in
    the readout's sum alone.  Returns (g (n_mols, out), h_list of (N, d))."""
    import packed_ref as PR
    P = lambda k: p[prefix + k]
    sp = {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix + "update_layer/")}
    h = P("embed/W")[pb.atom_id.cpu().long()]
    h0 = h
    h_list = []
    for step in range(n_layers):
        li = 0 if weight_tying else step
        m = PR.message(pb, h, P(f"message_layers/{li}/W"), P(f"message_layers/{li}/b"))
        h, _ = PR.gru(sp, "update_layer", h, m, first=(step == 0))
        h_list.append(h)
    y = layer_aggregate(h_list, aggregator, *_agg_params(p, aggregator, prefix))
    y0 = torch.cat([h0] * n_layers, dim=-1) if aggregator == "concat" else h0
    w = pb.row_w.cpu().to(h.dtype)[:, None]
    gi = torch.sigmoid(torch.cat((y, y0), 1) @ P("i_layers/0/W").t() + P("i_layers/0/b"))
    gj = y @ P("j_layers/0/W").t() + P("j_layers/0/b")
    return PR.segment_sum(pb, w * gi * gj), h_list


def make_agg_params(seed, hidden_dim, out_dim, n_layers, aggregator, weight_tying=True, dtype=torch.float64, prefix="",
                    bias_scale=0.3, n_atom_types=O.MAX_ATOMIC_NUM):
    """The link tree of a GGNN with ``layer_aggregator`` (models/ggnn.py:83-213) minus the recurrent links nobody calls:
    oracle.ref_cpu.init_ggnn's draws, the readout layers at the width construct_layer_aggregator gives them, and
    attn_dense_layer = Linear(T, T) for 'attn'."""
    dr = O._Draw(seed, dtype, bias_scale)
    O.init_ggnn(dr, prefix, out_dim, hidden_dim, n_layers, weight_tying=weight_tying, n_atom_types=n_atom_types)
    if aggregator == "concat":
        dr.lin(f"{prefix}i_layers/0", 2 * n_layers * hidden_dim, out_dim)
        dr.lin(f"{prefix}j_layers/0", n_layers * hidden_dim, out_dim)
    if aggregator == "attn":
        dr.lin(f"{prefix}attn_dense_layer", n_layers, n_layers)
    return dr.p


def make_agg_pair_params(seed, hidden_dim, out_dim, n_layers, aggregator, weight_tying=True, sim_method="mlp",
                         mlp_hidden=(32, 16), class_num=1, dtype=torch.float64, bias_scale=0.05):
    """GraphConvPredictorForPair without a co-attention: the aggregated encoder under graph_conv/ and the link predictor under
    mlp/ (oracle.ref_cpu.init_mlp / init_link)."""
    p = make_agg_params(seed, hidden_dim, out_dim, n_layers, aggregator, weight_tying, dtype, "graph_conv/", bias_scale)
    dr = O._Draw(seed + 1, dtype, bias_scale)
    if sim_method == "mlp":
        O.init_mlp(dr, "mlp/", 2 * out_dim, class_num, mlp_hidden)
    else:
        O.init_link(dr, "mlp/", sim_method, out_dim, class_num, mlp_hidden)
    p.update(dr.p)
    return p


def pair_agg_forward(p, a1, j1, a2, j2, n_layers, aggregator, weight_tying=True, sim_method="mlp", mlp_hidden=2):
    """train_ddi_modify.py:66-77 / train_binary.py:91-113 without a co-attention: logits of the pair batch."""
    g1, _ = ggnn_agg_forward(p, a1, j1, n_layers, aggregator, weight_tying, prefix="graph_conv/")
    g2, _ = ggnn_agg_forward(p, a2, j2, n_layers, aggregator, weight_tying, prefix="graph_conv/")
    if sim_method == "mlp":
        return O.mlp_forward(p, torch.cat((g1, g2), dim=-1), mlp_hidden)
    fwd = {"ntn": O.ntn_forward, "hole": O.hole_forward, "symmlp": O.symmlp_forward}[sim_method]
    return fwd(p, g1, g2, mlp_hidden, prefix="mlp/")
