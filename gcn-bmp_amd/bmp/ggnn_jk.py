"""The two jumping-knowledge GGNN encoders of the reference, with the reference's signatures: ``models.ggnn_dev_jknet.GGNN``
(models/ggnn_dev_jknet.py:45-186) as ``JKNetGGNN`` and ``models.ggnn_dev_jk_gru.GGNN`` (models/ggnn_dev_jk_gru.py:20-155) as
``JKGruGGNN``.  The trainers pick an encoder by import (train_ddi_modify_eval2.py:41-43, train_binary.py:39-51).

Both keep models/ggnn.py's embedding, its message (edge type the fastest axis of the 4d output) and its monolithic readout
``sum over ALL positions of sigmoid(i([h, h0])) * j(h)``; the node update is a relu-linear on ``x = [h, m]`` with no gate:

    jknet  (ggnn_dev_jknet.py:104-105,139)   h' = relu(update_layer[u] x),  u = 0 if update_tying else step;  no GRU, no state;
                                             the T step outputs go through the layer aggregator (:175-183) into readout 0
    jk_gru (ggnn_dev_jk_gru.py:79-80,106-117) m' = m + self_loop_layer(h) (ONE GraphLinear(d, d), with self_loop);
                                             x' = relu(update_layers_0[u] [h, m']) (2d wide),  u = 0 if WEIGHT_tying else step (:80
                                             reads the wrong flag);  h' = GRU(2d, d)(x'), stateful: the first call after reset has
                                             no r gate and no U terms, later calls read the GRU's own previous un-dropped output

A step is ``Fn.jk_step``: one fused kernel per tile and direction at hidden_dim 64 / 128 on whole tiles (csrc/bmp_jk.hip) and,
for the (kind, width) Fn.JK_TABLE_DEFAULT holds True for, on a tile table (csrc/bmp_jk_table.hip; the tile-table seam of bmp/
functional.py); the composed operators otherwise (any width that is a multiple of 8, molecules spanning tiles,
training dropout); jk_gru's GRU is the existing GRU operator on the two d-wide halves of x'.

The rows entry of the encoder layout (``encode_rows`` / ``readout_rows``) is bmp.ggnn._StepEncoder's for both classes; jknet's runs
the aggregator too, and takes every aggregator but 'attn' (``layout_reason``): the arithmetic is per row and per channel then, so a
molecule's atom states do not depend on its batch side.

The layer aggregators of jknet (select_aggr, :21-42):
    'max'     :201-212, the existing Fn.LayerAggFn in max mode          'mean'  :215-226, y = (1 / T) sum_t h_t
    'attn'    :297-344, no parameters: E_t = <H_t, H_T> + <H_t, H_1> over ALL mb * A * d elements of one encoder call (one batch
              side, every padded position included), c = softmax_t(E), y = sum_t c_t H_t.  On packed rows the inner products carry
              row_w (the pad row counts with its multiplicity) and are taken per side (pb.side_tiles).
    'concat'  :189-198 feeds a T d-wide array into readout links built for d: valid for n_layers == 1 only (ValueError otherwise)
    'gru', 'bigru'  NStep links outside the tree: NotImplementedError, as bmp/ggnn.py's recurrent aggregators
    None      select_aggr asserts (:22): the constructor fails in the reference, and here

``dropout_rate`` (after every step): identity under ``eval()``; in training the aggregator sees the dropped states (:168-176), jk_gru's
GRU keeps its own un-dropped state, and the zero-padded positions of a molecule are ONE row of the packed layout and share one
mask.

Parameter names follow the reference link tree (embed.W, message_layers.{i}.W/b, update_layer.{k}.W/b [jknet] or
update_layers_0.{k}.W/b, update_layer.{W_r,W_z,W,U_r,U_z,U}.W/b, self_loop_layer.W/b [jk_gru], i_layers.{k}.W/b, j_layers.{k}.W/b),
so a snapshot maps key by key.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fn
from .ggnn import GGNN, GRU, Linear, MAX_ATOMIC_NUM, _StepEncoder

JK_AGGREGATORS = ('concat', 'max', 'mean', 'attn')                  # models/ggnn_dev_jknet.py:23-28, 37-39
JK_RECURRENT_AGGREGATORS = ('gru', 'bigru')                         # :29-36: refused

JK_ATTN_LAYOUT_REASON = (
    "with layer_aggr='attn' the aggregation coefficients are a softmax over inner products taken over ALL atoms and padded positions "
    "of a whole batch side, so a molecule's vector depends on the other molecules of its side and on the padded atom count: one pad "
    "row per tile (the encoder layout), one encoding per distinct molecule (dedup), the layout plan and the recorded step are not "
    "valid for it; use the per-instance batch form")


class _JKBase(_StepEncoder):
    """What the two files share beyond _StepEncoder: the call and the rows entry over the subclass's ``_encode``."""

    _fused = True               # private switch: False takes the composed operators at every width

    def forward(self, atom_array, adj=None):
        """``atom_array`` is the dense int32 (mb, A) array with ``adj`` (mb, 4, A, A), or a PackedMolBatch (then ``adj`` is
        ignored).  Returns (n_mols, out_dim) [(n_mols, n_layers * out_dim) with concat_hidden]."""
        pb, h0, y, g_list = self._encode(atom_array, adj)
        self.atoms = self._packed_atoms(y, pb)                          # (jknet: the aggregated states)
        if self.concat_hidden:                                          # (jknet :178-179: the aggregator is never called)
            return torch.cat(g_list, dim=1)
        return self.readout(y, h0, pb, 0)

    def _rows(self, pb):
        """(jknet: the aggregator's output too, without the readout.)"""
        _, h0, y, _ = self._encode(pb, None)
        return y, h0


class JKNetGGNN(_JKBase):
    """models/ggnn_dev_jknet.py:45-186."""

    FLOAT_ATOMS_CITE = "models/ggnn_dev_jknet.py:158-161"

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 layer_aggr=None, batch_normalization=False, weight_tying=True, update_tying=True):
        if layer_aggr is None:
            raise ValueError("layer_aggr=None: select_aggr asserts a layer aggregator (models/ggnn_dev_jknet.py:22,87)")
        if layer_aggr in JK_RECURRENT_AGGREGATORS:
            raise NotImplementedError(f"layer_aggr={layer_aggr!r} (NStepGRU / NStepBiGRU, models/ggnn_dev_jknet.py:229-294) is outside "
                                      "the tree")
        if layer_aggr not in JK_AGGREGATORS:
            raise ValueError('No such layer aggr named {}'.format(layer_aggr))      # :41
        if layer_aggr == 'concat' and n_layers != 1 and not concat_hidden:
            raise ValueError("layer_aggr='concat' hands the readout an n_layers * hidden_dim wide array where its links take "
                             "hidden_dim (models/ggnn_dev_jknet.py:91,181-183,197): valid for n_layers == 1 only")
        if n_layers > Fn.AGG_MAX_T and layer_aggr != 'concat':
            raise ValueError(f"the layer aggregators take n_layers <= {Fn.AGG_MAX_T}")
        super().__init__(out_dim, hidden_dim, n_layers, n_atom_types, concat_hidden, dropout_rate, batch_normalization, weight_tying)
        self.update_tying, self.layer_aggr = update_tying, layer_aggr
        self.n_update_layer = 1 if update_tying else n_layers
        self.update_layer = nn.ModuleList([Linear(2 * hidden_dim, hidden_dim) for _ in range(self.n_update_layer)])
        self._make_readout()
        if layer_aggr == 'attn':
            self.layout_reason = JK_ATTN_LAYOUT_REASON

    def aggregate(self, hs, pb):
        if self.layer_aggr == 'concat':
            return hs[0] if len(hs) == 1 else torch.cat(hs, dim=1)
        if self.layer_aggr == 'max':
            return Fn.LayerAggFn.apply(Fn.AGG_MODE["max-pool"], None, None, *hs)
        return Fn.JKAggFn.apply(Fn.JK_AGG_MODE[self.layer_aggr], pb, *hs)

    def _encode(self, atom_array, adj):
        """embed + the steps + the aggregator: (pb, h0, what the readout reads [concat_hidden: the last step's states], the
        per-step readouts of concat_hidden)."""
        pb, h = self._embed(atom_array, adj)
        h0 = h
        drop, masks = self._masks(h)
        msgw, updw, hs, g_list = {}, {}, [], []
        for step in range(self.n_layers):
            ui = 0 if self.update_tying else step
            if ui not in updw:
                updw[ui] = (self.update_layer[ui].W.t().contiguous(), self.update_layer[ui].b)
            h = Fn.jk_step(h, *self._message_weights(step, msgw), None, None, *updw[ui], pb, self._fused and not drop)
            if drop:
                h = self._dropped(h, step, masks)
            if self.concat_hidden:
                g_list.append(self.readout(h, h0, pb, step))
            hs.append(h)
        return pb, h0, (h if self.concat_hidden else self.aggregate(hs, pb)), g_list


class JKGruGGNN(_JKBase):
    """models/ggnn_dev_jk_gru.py:20-155."""

    FLOAT_ATOMS_CITE = "models/ggnn_dev_jk_gru.py:135-138"

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 batch_normalization=False, weight_tying=True, update_tying=True, self_loop=False):
        if not weight_tying and update_tying and n_layers > 1:
            raise ValueError("weight_tying=False with update_tying=True: the update index is `0 if weight_tying else step` "
                             "(models/ggnn_dev_jk_gru.py:80) into a list of ONE layer (:33,55-58): step 1 indexes past its end (:117)")
        super().__init__(out_dim, hidden_dim, n_layers, n_atom_types, concat_hidden, dropout_rate, batch_normalization, weight_tying)
        self.update_tying, self.self_loop = update_tying, self_loop
        self.n_update_layer = 1 if update_tying else n_layers
        self.update_layers_0 = nn.ModuleList([Linear(2 * hidden_dim, 2 * hidden_dim) for _ in range(self.n_update_layer)])
        if weight_tying:
            # :80 reads layer 0 at every step: the others are built and never called.  No gradient, so an optimizer with gradient
            # hooks leaves them alone, as Chainer's does (bmp.ggnn.EdgeNetwork.hidden_layers)
            for lin in self.update_layers_0[1:]:
                for p in lin.parameters():
                    p.requires_grad_(False)
        self.update_layer = GRU(2 * hidden_dim, hidden_dim)
        if self_loop:
            self.self_loop_layer = Linear(hidden_dim, hidden_dim)       # :61-62: ONE layer, not one per message layer
        self._make_readout()

    def _encode(self, atom_array, adj):
        """embed + the steps: (pb, h0, the last step's states, the per-step readouts of concat_hidden)."""
        pb, h = self._embed(atom_array, adj)
        h0 = h
        d = self.hidden_dim
        drop, masks = self._masks(h)
        loop = (self.self_loop_layer.W.t().contiguous(), self.self_loop_layer.b) if self.self_loop else (None, None)
        msgw, updw, g_list = {}, {}, []
        state, first_w, state_w = None, None, None
        for step in range(self.n_layers):
            ui = 0 if self.weight_tying else step                       # :80
            if ui not in updw:
                updw[ui] = (self.update_layers_0[ui].W.t().contiguous(), self.update_layers_0[ui].b)
            x = Fn.jk_step(h, *self._message_weights(step, msgw), *loop, *updw[ui], pb, self._fused and not drop)
            xa, xb = x[:, :d].contiguous(), x[:, d:].contiguous()
            if state is None:                                           # the first call after reset_state (:134)
                first_w = self.update_layer.kernel_weights(first=True)
                state = Fn.GRUFn.apply(xa, xb, *first_w, pb, True)
            else:
                if state_w is None:
                    state_w = self.update_layer.kernel_weights_state()
                state = Fn.GRUStateFn.apply(xa, xb, state, *state_w, pb)
            h = self._dropped(state, step, masks) if drop else state
            if self.concat_hidden:
                g_list.append(self.readout(h, h0, pb, step))
        return pb, h0, h, g_list


class ChinGGNN(GGNN):
    """models/chin_ggnn.py:18-139: models/ggnn.py's default path (matrix-multiply message, stateful GRU, graph-level readout) under
    the shorter constructor of that file."""

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 batch_normalization=False, weight_tying=True):
        super().__init__(out_dim, hidden_dim=hidden_dim, n_layers=n_layers, n_atom_types=n_atom_types, concat_hidden=concat_hidden,
                         dropout_rate=dropout_rate, batch_normalization=batch_normalization, weight_tying=weight_tying)
