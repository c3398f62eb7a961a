"""The last two GRU-based GGNN encoders of the reference that a trainer reaches, with the reference's signatures:
``models.ggnn_dev.GGNN`` (models/ggnn_dev.py:20-176; smiles_based_ddi.py:42, train_ddi_modify_eval3.py:49) as ``DevGGNN`` and
``models.ggnn_dev_self_loop.GGNN`` (models/ggnn_dev_self_loop.py:20-145 = models/ggnn_dev_edge.py; train_binary.py:51,
train_ddi_modify_eval2.py:43, train_ddi_modify_eval3.py:50) as ``SelfLoopGGNN``.

Both keep models/ggnn.py's embedding, message (edge type the fastest axis of the 4d output), stateful GRU (first call after
reset: no r gate, no U terms) and readout ``sum over ALL positions of sigmoid(i([h, h0])) * j(h)``.

    DevGGNN       keeps every step's atom states and readout: ``get_atom_array(step=-1)`` and ``get_g_list()``
                  (train_ddi_modify_eval3.py:116-138).  Without ``concat_hidden`` the call returns the SUM over all A padded
                  positions of the last step's h (:165-168 compute the readout and then overwrite it) -- (mb, hidden_dim), not
                  out_dim wide; i_layers / j_layers then receive gradient through get_g_list() only.
    SelfLoopGGNN  adds ``message_self_loop_layers`` (one GraphLinear(d, d) per message layer) to the message:
                  m = m + h W_s[l]^T + b_s[l], l = 0 if weight_tying else step (:96-97).  Padded positions have no bonds and one
                  h, so m = W_s h + b_s there too and the one virtual pad row per molecule stays exact.  A step is
                  ``Fn.loop_step``: one fused kernel per tile and direction at hidden_dim 64 / 128 on whole tiles
                  (csrc/bmp_loop.hip) and, for the widths Fn.LOOP_TABLE_DEFAULT holds True for, on a tile table (csrc/
                  bmp_loop_table.hip; the tile-table seam of bmp/functional.py); the composed operators otherwise.

The rows entry of the encoder layout (``encode_rows`` / ``readout_rows``) is bmp.ggnn._StepEncoder's for both classes.  ``DevGGNN``
keeps only the last step's atom states then: ``get_atom_array()`` / ``get_atom_array(-1)`` return them, any other step and
``get_g_list()`` raise.

``dropout_rate`` (after every step): identity under ``eval()``; in training the step OUTPUT is dropped while the stateful GRU keeps
its own un-dropped state (the separate-state GRU operator), and the zero-padded positions of a molecule are ONE row of the packed
layout and share one mask, where the reference draws a mask per padded position -- same expectation, not the same random process
(INTEGRATION.md).

Parameter names follow the reference link tree (embed.W, message_layers.{i}.W/b, message_self_loop_layers.{i}.W/b,
update_layer.{W_r,W_z,W,U_r,U_z,U}.W/b, i_layers.{k}.W/b, j_layers.{k}.W/b), so a snapshot maps key by key.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fn
from .coarse import SegPoolFn
from .ggnn import GRU, Linear, MAX_ATOMIC_NUM, _StepEncoder, message_kernel_weights

ROWS_ONLY_REASON = ("the last call ran in the encoder layout, where only the last step's atom states exist on the instance rows; "
                    "per-step outputs need the per-instance batch form")


class _DevBase(_StepEncoder):
    """What the two files share beyond _StepEncoder: the step loop (``_step`` is the subclass's) and the GRU's weights."""

    FLOAT_ATOMS_CITE = "models/ggnn_dev.py:140-143, models/ggnn_dev_self_loop.py:125-128"

    def _steps(self, atom_array, adj):
        """embed + the propagation steps: (pb, h0, [h after every step, dropout applied])."""
        pb, h = self._embed(atom_array, adj)
        h0 = h
        drop, masks = self._masks(h)
        ctx = dict(pb=pb, drop=drop, state=None, later=None, state_w=None, msgw={}, cache={})
        hs = []
        for step in range(self.n_layers):
            s = self._step(h, step, ctx)
            if drop:            # the stateful GRU keeps the un-dropped state
                ctx["state"] = s
                h = self._dropped(s, step, masks)
            else:
                h = s
            hs.append(h)
        return pb, h0, hs

    def _rows(self, pb):
        _, h0, hs = self._steps(pb, None)
        return hs[-1], h0

    def _gru_weights(self, step, ctx):
        if step == 0:
            return self.update_layer.kernel_weights(first=True)
        if ctx["later"] is None:
            ctx["later"] = self.update_layer.kernel_weights(first=False)
        return ctx["later"]

    def _state_weights(self, ctx):
        if ctx["state_w"] is None:
            ctx["state_w"] = self.update_layer.kernel_weights_state()
        return ctx["state_w"]

    def _step(self, h, step, ctx):
        raise NotImplementedError


class DevGGNN(_DevBase):
    """models/ggnn_dev.py:20-176."""

    fused = True                # use the fused per-tile step kernel where the width allows, as bmp.ggnn.GGNN

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 batch_normalization=False, weight_tying=True, output_atoms=True):
        super().__init__(out_dim, hidden_dim, n_layers, n_atom_types, concat_hidden, dropout_rate, batch_normalization, weight_tying)
        self.output_atoms = output_atoms
        self.update_layer = GRU(2 * hidden_dim, hidden_dim)
        self._make_readout()
        self.atoms_list, self.g_vec_list = [], []
        self._rows_only = False     # the last call was encode_rows: only the last step's atoms exist

    def _step(self, h, step, ctx):
        """bmp.ggnn.GGNN.forward's step, without the planned path."""
        pb = ctx["pb"]
        WT, bE = self._message_weights(step, ctx["msgw"])
        AT, UcT, b = self._gru_weights(step, ctx)
        if self.fused and Fn.step_supported(self.hidden_dim) and not ctx["drop"] and not pb.oversized:
            return Fn.GGNNStepFn.apply(h, WT, bE, AT, UcT, b, pb, step == 0, ctx["cache"])
        m = Fn.MsgFn.apply(h, WT, bE, None, None, pb, Fn.ACT["identity"])
        if ctx["state"] is not None:
            return Fn.GRUStateFn.apply(h, m, ctx["state"], *self._state_weights(ctx), pb)
        return Fn.GRUFn.apply(h, m, AT, UcT, b, pb, step == 0)

    def forward(self, atom_array, adj=None):
        """``atom_array`` is the dense int32 (mb, A) array with ``adj`` (mb, 4, A, A), or a PackedMolBatch (then ``adj`` is
        ignored).  Returns (n_mols, hidden_dim): the sum of the last step's atom states over ALL A positions (:165-168) --
        with concat_hidden (n_mols, n_layers * out_dim), the concatenated readouts."""
        self.atoms_list, self.g_vec_list = [], []               # :137-138
        self._rows_only = False
        pb, h0, hs = self._steps(atom_array, adj)
        self.atoms_list = [self._packed_atoms(h, pb) for h in hs]
        self.g_vec_list = [self.readout(h, h0, pb, t) for t, h in enumerate(hs)]       # :159-160
        if self.concat_hidden:
            return torch.cat(self.g_vec_list, dim=1)            # (:153-155 compute the same readouts a second time)
        h = hs[-1]
        ones = torch.ones(h.shape[0], 1, dtype=h.dtype, device=h.device)
        return SegPoolFn.apply(ones, h, pb.row_w, pb.mol_row0, pb.mol_nrows)           # the pad row counts with its multiplicity

    def graph_vector_dim(self) -> int:
        """Width of what the call returns per molecule (the pair predictor sizes its link predictor by it)."""
        return self.n_layers * self.out_dim if self.concat_hidden else self.hidden_dim

    def encode_rows(self, pb):
        """_StepEncoder.encode_rows; what the last call kept of its steps is dropped (``set_rows_atoms`` hands over the new atoms)."""
        self.atoms_list, self.g_vec_list = [], []
        self._rows_only = True
        return super().encode_rows(pb)

    def readout_rows(self, h, h0, pb):
        """What the call returns without concat_hidden, of row tensors that live on ``pb``'s rows: the sum of the last step's
        atom states over all A positions (the pad row counts with its multiplicity pb.row_w), not the gated readout."""
        ones = torch.ones(h.shape[0], 1, dtype=h.dtype, device=h.device)
        return SegPoolFn.apply(ones, h, pb.row_w, pb.mol_row0, pb.mol_nrows)

    def set_rows_atoms(self, atoms):
        """The pair predictor's hand-over after ``encode_rows``: the LAST step's atom states on the instance rows -- the only
        step that exists there."""
        self.atoms_list = [atoms]

    def get_atom_array(self, step=-1):
        """:170-172.  Returns that step's PackedAtoms; ``.dense()`` gives (mb, A, hidden_dim).  After a call in the encoder
        layout only the last step (-1 or n_layers - 1) exists."""
        assert len(self.atoms_list) > 0
        if self._rows_only:
            if step not in (-1, self.n_layers - 1):
                raise RuntimeError(f"get_atom_array({step}): " + ROWS_ONLY_REASON)
            return self.atoms_list[0]
        return self.atoms_list[step]

    def get_g_list(self):
        """:174-176: the T readouts readout(h_t, h0, t), each (n_mols, out_dim)."""
        if self._rows_only:
            raise RuntimeError("get_g_list(): " + ROWS_ONLY_REASON)
        assert len(self.g_vec_list) > 0
        return self.g_vec_list


class SelfLoopGGNN(_DevBase):
    """models/ggnn_dev_self_loop.py:20-145 = models/ggnn_dev_edge.py."""

    _fused = True               # private switch: False takes the composed operators at every width

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 batch_normalization=False, weight_tying=True):
        super().__init__(out_dim, hidden_dim, n_layers, n_atom_types, concat_hidden, dropout_rate, batch_normalization, weight_tying)
        self.message_self_loop_layers = nn.ModuleList([Linear(hidden_dim, hidden_dim) for _ in range(self.n_message_layer)])
        self.update_layer = GRU(2 * hidden_dim, hidden_dim)
        self._make_readout()

    def _step(self, h, step, ctx):
        pb, li = ctx["pb"], (0 if self.weight_tying else step)
        if li not in ctx["msgw"]:
            sl = self.message_self_loop_layers[li]
            ctx["msgw"][li] = message_kernel_weights(self.message_layers[li]) + (sl.W.t().contiguous(), sl.b)
        AT, UcT, b = self._gru_weights(step, ctx)
        if ctx["state"] is not None:
            return Fn.loop_step(h, *ctx["msgw"][li], AT, UcT, b, False, pb, False, ctx["state"], self._state_weights(ctx))
        return Fn.loop_step(h, *ctx["msgw"][li], AT, UcT, b, step == 0, pb, self._fused and not ctx["drop"])

    def forward(self, atom_array, adj=None):
        """``atom_array`` is the dense int32 (mb, A) array with ``adj`` (mb, 4, A, A), or a PackedMolBatch (then ``adj`` is
        ignored).  Returns (n_mols, out_dim) [(n_mols, n_layers * out_dim) with concat_hidden]."""
        pb, h0, hs = self._steps(atom_array, adj)
        self.atoms = self._packed_atoms(hs[-1], pb)
        if self.concat_hidden:
            return torch.cat([self.readout(h, h0, pb, t) for t, h in enumerate(hs)], dim=1)
        return self.readout(hs[-1], h0, pb, 0)
