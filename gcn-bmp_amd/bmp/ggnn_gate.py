"""The two GGNN encoders whose node update is a gate instead of the GRU, with the reference's signatures:
``models.ggnn_dev_fuse.GGNN`` (models/ggnn_dev_fuse.py:18-168, the recorded "fuse gate" run of RECORD.txt:404-405) as
``FuseGGNN`` and ``models.ggnn_dev_gate.GGNN`` (models/ggnn_dev_gate.py:20-154) as ``GateGGNN``.  The trainers pick one by
import (train_ddi_modify_eval2.py:41-43, train_binary.py:39-51).

Both keep models/ggnn.py's embedding, its message (edge type the fastest axis of the 4d output) and its monolithic readout
``sum over ALL positions of sigmoid(i([h, h0])) * j(h)``; they differ in the update, per atom row, with ``x = [h, m]``:

    fuse (ggnn_dev_fuse.py:72-88,127):  z = tanh(W1 x + b1), r = sigmoid(W2 x + b2), f = sigmoid(W3 x + b3)
                                        out = dropout(r * h, 0.05) + f * z          (the ratio is hard-wired)
    gate (ggnn_dev_gate.py:112-116):    a = sigmoid(Wg_k x + bg_k), out = (1 - a) * h + a * m,  k = 0 if update_tying else step

The fuse linears are shared by all steps even when the message weights are untied.  A step is ``Fn.gate_step``: one fused
kernel per tile and direction at hidden_dim 64 / 128 (csrc/bmp_gate.hip) and at 32, the recorded width (csrc/bmp_gate_small.hip,
for the kinds Fn.GATE_SMALL_DEFAULT holds True for), on whole tiles; at 32 also on a tile table (Fn.GATE_TABLE_DEFAULT; the
tile-table seam of bmp/functional.py); the composed operators otherwise.  The rows entry of the encoder layout
(``encode_rows`` / ``readout_rows``) is bmp.ggnn._StepEncoder's: ``GateGGNN`` trains there, ``FuseGGNN`` takes it under ``eval()``
(its training dropout needs per-instance rows: ``_mode_reason``).

Dropout (the fuse gate's on ``r * h`` and ``dropout_rate`` on every step's output, :157-158): identity under ``eval()``; in
training the zero-padded positions of a molecule are ONE row of the packed layout and share one mask, where the reference
draws a mask per padded position -- same expectation, not the same random process.

Parameter names follow the reference link tree (embed.W, message_layers.{i}.W/b, update_layer1|2|3.W/b or gate_layer.{k}.W/b,
i_layers.{k}.W/b, j_layers.{k}.W/b).  ``FuseGGNN`` also keeps the links the file constructs and never calls -- ``update_layer``
(the GRU, :55) and ``embed_linear`` (66 -> hidden, :48, reached by float atom features only) -- so a snapshot maps key by key;
their gradients are zero.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fn
from .ggnn import CONCAT_LAYOUT_REASON, DROPOUT_LAYOUT_REASON, GRU, Linear, MAX_ATOMIC_NUM, _StepEncoder     # noqa: F401 (the reasons: re-exported)

FUSE_DROPOUT = 0.05             # models/ggnn_dev_fuse.py:127

FUSE_TRAIN_LAYOUT_REASON = ("the fuse gate's dropout on r * h is active in training, and the encoder layout (dedup above all) "
                            "would give all instances of a molecule one mask; train per-instance or on the static batch, or call "
                            "eval()")


class _GatedGGNN(_StepEncoder):
    """What the two files share beyond _StepEncoder (its readout is :133-141): the step loop."""

    FLOAT_ATOMS_CITE = "models/ggnn_dev_fuse.py:149-150, models/ggnn_dev_gate.py:136-137"
    KIND = None                 # Fn.GATE_KIND of the subclass
    _fused = True               # private switch: False takes the composed operators at every width (32, 64 and 128 included)

    def _update_weights(self, step):
        """(AU [2d x Nu], bU [Nu]) of the step, in Fn.gate_step's layout."""
        raise NotImplementedError

    def forward(self, atom_array, adj=None):
        """``atom_array`` is the dense int32 (mb, A) array with ``adj`` (mb, 4, A, A), or a PackedMolBatch (then ``adj`` is
        ignored).  Returns (n_mols, out_dim) [(n_mols, n_layers * out_dim) with concat_hidden]."""
        g_list = [] if self.concat_hidden else None
        pb, h, h0 = self._steps(atom_array, adj, g_list)
        self.atoms = self._packed_atoms(h, pb)
        if self.concat_hidden:
            return torch.cat(g_list, dim=1)
        return self.readout(h, h0, pb, 0)

    def _steps(self, atom_array, adj=None, g_list=None):
        """The embedding and the propagation steps: (pb, h, h0).  ``g_list`` collects the per-step readouts of concat_hidden."""
        pb, h = self._embed(atom_array, adj)
        h0 = h
        fuse = self.KIND == Fn.GATE_KIND["fuse"]
        # (tests inject the fuse gate's training masks: one (n_rows, hidden) tensor per step)
        _, masks = self._masks(h, self.training and fuse)
        msgw, updw = {}, {}
        for step in range(self.n_layers):
            ui = self._update_index(step)
            if ui not in updw:
                updw[ui] = self._update_weights(ui)
            keep = None
            if fuse and self.training:
                if masks is not None:
                    keep = masks[step]
                else:
                    keep = (torch.rand(h.shape, device=h.device) >= FUSE_DROPOUT).to(torch.float32) * (1.0 / (1.0 - FUSE_DROPOUT))
            h = Fn.gate_step(h, *self._message_weights(step, msgw), *updw[ui], self.KIND, keep, pb, self._fused)
            if self.dropout_rate != 0.0 and self.training:              # :157-158
                h = self._dropped(h, step, None)
            if g_list is not None:
                g_list.append(self.readout(h, h0, pb, step))
        return pb, h, h0

    def _rows(self, pb):
        return self._steps(pb)[1:]

    def _update_index(self, step):
        return 0


class FuseGGNN(_GatedGGNN):
    """models/ggnn_dev_fuse.py:18-168."""

    KIND = Fn.GATE_KIND["fuse"]

    def _mode_reason(self):
        return FUSE_TRAIN_LAYOUT_REASON if self.training else None

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 batch_normalization=False, weight_tying=True):
        super().__init__(out_dim, hidden_dim, n_layers, n_atom_types, concat_hidden, dropout_rate, batch_normalization, weight_tying)
        self.embed_linear = Linear(66, hidden_dim)                      # :48, never reached with atom ids
        self.update_layer = GRU(2 * hidden_dim, hidden_dim)             # :55, constructed and never called (:126)
        self.update_layer1 = Linear(2 * hidden_dim, hidden_dim)         # z
        self.update_layer2 = Linear(2 * hidden_dim, hidden_dim)         # r
        self.update_layer3 = Linear(2 * hidden_dim, hidden_dim)         # f
        self._make_readout()

    def _update_weights(self, step):
        ls = (self.update_layer1, self.update_layer2, self.update_layer3)
        return torch.cat([l.W for l in ls], dim=0).t().contiguous(), torch.cat([l.b for l in ls])


class GateGGNN(_GatedGGNN):
    """models/ggnn_dev_gate.py:20-154."""

    KIND = Fn.GATE_KIND["gate"]

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False, dropout_rate=0.0,
                 batch_normalization=False, weight_tying=True, update_tying=True):
        super().__init__(out_dim, hidden_dim, n_layers, n_atom_types, concat_hidden, dropout_rate, batch_normalization, weight_tying)
        self.update_tying = update_tying
        self.n_update_layer = 1 if update_tying else n_layers
        self.gate_layer = nn.ModuleList([Linear(2 * hidden_dim, hidden_dim) for _ in range(self.n_update_layer)])
        self._make_readout()

    def _update_index(self, step):
        return 0 if self.update_tying else step

    def _update_weights(self, step):
        lin = self.gate_layer[step]
        return lin.W.t().contiguous(), lin.b
