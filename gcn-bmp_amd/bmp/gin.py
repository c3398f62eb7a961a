"""Graph isomorphism network encoder with the reference's signatures: ``models.gin.GINUpdate`` (models/gin.py:58-128) and
``GIN`` (:131-226), the encoder the multi-label trainer selects with ``--method gin``
(train_ggnn_hole_multi_class_x37.py:226-228; it reads the ``ggnn`` preprocessor's batches, :458-459).

A layer is ``relu(drop(relu((h + adjsum . h) W1^T + b1) W2^T + b2))`` with ``adjsum`` the (mb, 4, A, A) adjacency summed
over its bond types: the bond type does not matter, an entry counts with its value.  Nothing is masked, so the zero-padded
positions of a molecule have no neighbours and share one trajectory -- the packed layout's virtual pad row with multiplicity
``row_w``.  The readout is the modular ``GGNNReadout`` on ``[h, h0]`` (bmp/relgcn.py).

The loop runs ``range(n_message_layers)`` (models/gin.py:215): with ``weight_tying=True`` -- the default, and what the
trainer builds -- exactly ONE layer runs whatever ``n_layers`` says; with ``weight_tying=False`` ``n_layers`` layers run.  The
readout layers that the loop never reaches keep their parameters, so a snapshot maps key by key, and ``concat_hidden=True``
returns ``(mb, n_message_layers * out_dim)``.

``dropout_ratio`` (between the second linear and its relu, :120-123): identity under ``eval()``; in training the zero-padded
positions of a molecule are ONE row of the packed layout and share one mask, where the reference draws a mask per padded
position -- same expectation, not the same random process.

Batch forms: per instance and the fixed-shape batch (``PairBatches(layout="static")``) through ``forward``; the encoder layout,
with or without ``dedup``, through the rows entry ``encode_rows`` / ``readout_rows`` (``rows_reason`` says what it refuses:
``concat_hidden`` with more than one layer running, and training dropout).  At d = 64 / 128 the layers of a table batch run on the
tile-table kernels (csrc/bmp_gin_table.hip, ``Fn.GIN_TABLE_DEFAULT``).

Parameter names follow the reference link tree (embed.W, update_layers.{i}.linear_g1.W/b, update_layers.{i}.linear_g2.W/b,
readout_layers.{k}.i_layer.W/b, readout_layers.{k}.j_layer.W/b).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import functional as Fn
from .ggnn import CONCAT_LAYOUT_REASON, DROPOUT_LAYOUT_REASON, EmbedID, Linear, MAX_ATOMIC_NUM, PackedAtoms, _is_float_atoms, as_packed
from .packed import PackedMolBatch
from .relgcn import GGNNReadout


class GINUpdate(nn.Module):
    """models/gin.py:58-128: two GraphLinear(hidden, hidden) and relu, dropout in front of the second relu."""

    _fused = True               # private switch: False takes the composed operators at every width

    def __init__(self, hidden_dim=16, dropout_ratio=0.5):
        super().__init__()
        if hidden_dim % 8:
            raise ValueError("hidden_dim must be a multiple of 8")
        if not 0.0 <= dropout_ratio < 1.0:
            raise ValueError("dropout_ratio must lie in [0, 1)")
        self.linear_g1 = Linear(hidden_dim, hidden_dim)
        self.linear_g2 = Linear(hidden_dim, hidden_dim)
        self.hidden_dim, self.dropout_ratio = hidden_dim, dropout_ratio

    def forward(self, h, pb: PackedMolBatch, keep=None):
        """``keep`` [n_rows x hidden]: the mask to use (0 or 1 / (1 - p)); None draws one in training mode."""
        if keep is None and self.dropout_ratio > 0.0 and self.training:
            p = self.dropout_ratio
            keep = (torch.rand(h.shape, device=h.device) >= p).to(torch.float32) * (1.0 / (1.0 - p))
        return Fn.gin_layer(h, self.linear_g1.W.t(), self.linear_g1.b, self.linear_g2.W.t(), self.linear_g2.b, keep, pb, self._fused)


class GIN(nn.Module):
    """models/gin.py:131-226."""

    NUM_EDGE_TYPE = 4

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, dropout_ratio=0.5, concat_hidden=False,
                 weight_tying=True, activation="identity"):
        super().__init__()
        if activation not in Fn.ACT:
            raise ValueError(f"activation must be one of {sorted(k for k in Fn.ACT if k)}")
        n_message_layer = 1 if weight_tying else n_layers
        n_readout_layer = n_layers if concat_hidden else 1
        self.embed = EmbedID(out_size=hidden_dim, in_size=n_atom_types)
        self.update_layers = nn.ModuleList([GINUpdate(hidden_dim=hidden_dim, dropout_ratio=dropout_ratio)
                                            for _ in range(n_message_layer)])
        self.readout_layers = nn.ModuleList([
            GGNNReadout(out_dim=out_dim, hidden_dim=hidden_dim, activation=activation, activation_agg=activation,
                        in_dim=2 * hidden_dim) for _ in range(n_readout_layer)])
        self.out_dim, self.hidden_dim, self.n_layers = out_dim, hidden_dim, n_layers
        self.n_message_layers, self.n_readout_layer = n_message_layer, n_readout_layer
        self.dropout_ratio, self.concat_hidden, self.weight_tying = dropout_ratio, concat_hidden, weight_tying
        # width of the molecule vector in units of out_dim (the pair predictor sizes its link predictor with it)
        self.n_concat = n_message_layer if concat_hidden else 1
        self.atoms = None

    def plannable(self) -> bool:
        return False            # no layout plan: FlatAdam / fit leave the encoder to autograd (bmp/dp.py)

    def _batch(self, atom_array, adj):
        """The call's batch, behind the refusals every entry shares (float atom features, a CPU batch)."""
        if _is_float_atoms(atom_array):
            raise NotImplementedError("float atom features (embedding bypass, models/gin.py:207-210) are not supported")
        pb = as_packed(atom_array, adj, self.embed.W.device)
        if not pb.atom_id.is_cuda:
            raise RuntimeError("GIN runs on the GPU only: there is no CPU path (move the model and the batch to the device)")
        return pb

    @property
    def encoder_layout_reason(self):
        """Why ``PairBatches(layout="encoder")`` is refused whatever the mode, if it is (bmp.trainer.PairBatches.check_encoder):
        concat_hidden with more than one layer reads out after every layer.  The trainer's construction -- concat_hidden with tied
        weights -- runs ONE layer and one readout and is served."""
        return CONCAT_LAYOUT_REASON if self.concat_hidden and self.n_concat > 1 else None

    def rows_reason(self):
        """Why ``encode_rows`` refuses this encoder in its present mode; None: it runs.  (encode_rows cannot see ``dedup``, and
        one mask per distinct molecule is not the reference's process: training dropout takes the per-instance batch form or
        layout="static".)"""
        dropout = DROPOUT_LAYOUT_REASON if self.training and self.dropout_ratio > 0.0 else None
        return self.encoder_layout_reason or dropout

    def encode_rows(self, pb):
        """The embedding and the layers WITHOUT the readout: (h, h0) on the rows of ``pb`` -- the entry the pair predictor uses
        for a batch in the encoder layout (bmp/enclayout.py), whose readout runs on the per-instance rows (``readout_rows``).
        A molecule taller than a tile goes through the composed operators, as in ``forward``; there is no ``is_real_node`` here."""
        reason = self.rows_reason()
        if reason:
            raise NotImplementedError("encode_rows: " + reason)
        pb = self._batch(pb, None)
        pb.check_atom_ids(self.embed.W.shape[0])
        h0 = h = Fn.EmbedFn.apply(self.embed.W, pb.atom_id)
        for step in range(self.n_message_layers):                                # :215 -- not range(n_layers)
            h = self.update_layers[0 if self.weight_tying else step](h, pb, None)
        return h, h0

    def readout_rows(self, h, h0, pb):
        """The readout of row tensors that live on ``pb``'s rows (the partner of ``encode_rows``)."""
        return self.readout_layers[0](h, pb, h0, None)

    def forward(self, atom_array, adj=None, is_real_node=None):
        pb = self._batch(atom_array, adj)
        row_w = None
        if is_real_node is not None:
            # mask (mb, A) -> per-row weight: a virtual row carries the sum of its positions' masks
            if pb.dense_map is None:
                raise NotImplementedError("is_real_node needs the dense input form")
            m = torch.as_tensor(np.asarray(is_real_node), dtype=torch.float32, device=pb.device)
            row_w = torch.zeros(pb.n_rows, device=pb.device).index_add_(0, pb.dense_map.reshape(-1), m.reshape(-1))
        pb.check_atom_ids(self.embed.W.shape[0])
        h = Fn.EmbedFn.apply(self.embed.W, pb.atom_id)
        h0 = h
        # (tests inject the training masks: one (n_rows, hidden) tensor per step)
        masks = getattr(self, "_dropout_masks", None) if self.training else None
        g_list = []
        for step in range(self.n_message_layers):                                # :215 -- not range(n_layers)
            li = 0 if self.weight_tying else step
            h = self.update_layers[li](h, pb, None if masks is None else masks[step])
            if self.concat_hidden:
                g_list.append(self.readout_layers[step](h, pb, h0, row_w))
        self.atoms = PackedAtoms(h, pb, 0 if pb.dense_map is not None else None)
        if self.concat_hidden:
            return torch.cat(g_list, dim=1)
        return self.readout_layers[0](h, pb, h0, row_w)

    def get_atom_array(self):
        """Not in the reference: the last layer's atom states, so that GIN composes with every co-attention (as RelGCN's)."""
        assert self.atoms is not None
        return self.atoms
