"""Neural-fingerprint encoder with the reference's signatures: ``models.models.nfp.NFPUpdate`` (models/models/nfp.py:15-62),
``NFPReadout`` (:65-91) and ``NFP`` (:94-179), the second encoder ``set_up_predictor`` can build (train_binary.py:274-276;
``--method`` defaults to ``nfp``, :318-319).

The reference hands the model ONE adjacency (mb, A, A): 1 per bond whatever its type plus the identity on the real atoms.  On the
packed layout that is the batch's CSR with the bond types ignored, plus a per-row self-loop weight ``self_w``; the degree
class of a row is the COLUMN sum of that adjacency (:157) compared with 1..7.  Nothing is masked in the reference, so a
padded position leaves every layer as sigmoid(B); the layout's virtual pad row (degree class 0, multiplicity ``row_w``)
reproduces that, as it does for GGNN.

Per-batch derivations (``nfp_derived``): ``self_w`` [N] f32, ``deg_class`` [N] int32 in 0..7, and the row lists by degree
class ``deg_rows`` [7 x N] / ``deg_cnt`` [7].  Device batches get them from csrc/bmp_nfp.hip; the numpy versions below are
pinned against those bit for bit (tests/test_gpu_nfp.py) and serve host batches (CPU tests of the layout).

Batch forms: per instance and the fixed-shape batch (``PairBatches(layout="static")``) through ``forward``; the encoder layout,
with or without ``dedup``, through ``encode_rows`` / ``readout_enc``: layers AND readout run on the encoder rows, and an instance's
padded positions enter its molecule vector as padcount * ``pad_term()`` (tests/test_nfp_table_build.py pins the formula against
the dense restatement in float64).  At d = 64 / 128 the layers and readouts of a table batch run on the tile-table kernels
(csrc/bmp_nfp_table.hip, ``Fn.NFP_TABLE_DEFAULT``).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import functional as Fn
from .ggnn import EmbedID, Linear, MAX_ATOMIC_NUM, PackedAtoms, _is_float_atoms
from .packed import DEFAULT_R, PackedMolBatch, _assemble, _ragged_arange

NUM_DEGREE_TYPE = 7          # max_degree + 1 (nfp.py:26,111): degrees 1..7 have a weight matrix of their own


# ---------------------------------------------------------------------------------------------------------
# batch side
# ---------------------------------------------------------------------------------------------------------
def deg_class_of(deg: np.ndarray) -> np.ndarray:
    """Degree class of float32 column sums: k where the sum equals k in 1..7 exactly, else 0 (nfp.py:159-161)."""
    deg = np.asarray(deg, dtype=np.float32)
    cls = np.zeros(deg.shape, dtype=np.int32)
    for k in range(1, NUM_DEGREE_TYPE + 1):
        cls[deg == np.float32(k)] = k
    return cls


def nfp_rows_host(pb: PackedMolBatch, enc: bool = False):
    """(self_w [N] float32, deg_class [N] int32) of a batch packed from the store, in numpy: the diagonal of the NFP
    adjacency is 1 on the real atoms of every molecule (rows mol_row0 .. mol_row0 + mol_nrows - 2) and 0 on its pad row and
    on dead rows; the degree is self_w plus the row's transposed-CSR values, added in entry order in float32.
    ``enc``: the batch is in the encoder layout (``EncBatch.pb_enc``), where mol_nrows counts real atoms only and row_mol is
    u >= 0 on a real atom, <= -2 on a tile's pad row, -1 on a dead row: self_w is 1 exactly where row_mol >= 0."""
    N = pb.n_rows
    row0 = pb.mol_row0.cpu().numpy().astype(np.int64)
    nrows = pb.mol_nrows.cpu().numpy().astype(np.int64)
    if enc:
        self_w = (pb.row_mol.cpu().numpy() >= 0).astype(np.float32)
    else:
        self_w = np.zeros(N, dtype=np.float32)
        for r0, n in zip(row0, nrows):
            self_w[r0:r0 + n - 1] = 1.0
    ptrT = pb.csrT_ptr.cpu().numpy().astype(np.int64)
    valT = pb.csrT_val.cpu().numpy().astype(np.float32)
    deg = self_w.copy()
    cnt = np.diff(ptrT)
    for j in range(int(cnt.max()) if N else 0):
        sel = np.nonzero(cnt > j)[0]
        deg[sel] = deg[sel] + valT[ptrT[sel] + j]            # float32 adds, one entry of every row at a time
    return self_w, deg_class_of(deg)


def deg_rows_host(deg_class: np.ndarray):
    """(idx [7 x N] int32, cnt [7] int32): idx[k - 1, :cnt[k - 1]] = the rows of class k, ascending (the rest: -1)."""
    N = len(deg_class)
    idx = np.full((NUM_DEGREE_TYPE, N), -1, dtype=np.int32)
    cnt = np.zeros(NUM_DEGREE_TYPE, dtype=np.int32)
    for k in range(1, NUM_DEGREE_TYPE + 1):
        rows = np.nonzero(deg_class == k)[0]
        idx[k - 1, :len(rows)] = rows
        cnt[k - 1] = len(rows)
    return idx, cnt


def nfp_derived(pb: PackedMolBatch, enc: bool = False) -> dict:
    """The batch's NFP data, derived once and kept with the batch (``StaticPairBatch.reset_derived`` forgets it with the
    other derived data): self_w, deg_class, deg_rows [7 x N], deg_cnt [7] and bwd_w [N], the weight whose zeros the layer
    backward leaves without gradient.  A batch made by ``pack_nfp_dense`` brings its self_w / deg_class along as fields of
    the batch (taken from the dense array as given).
    ``enc``: the caller says that ``pb`` is an ``EncBatch.pb_enc`` (``nfp_rows_host``); it is not guessed from the arrays.
    There bwd_w is the liveness weight, 1 where row_mol != -1: the pad rows have row_w == 0 and still carry the gradient
    that a co-attention sends back through ``EncRowsFn``.  On a per-instance batch bwd_w is row_w itself."""
    nd = pb._cache.get("nfp")
    if nd is not None:
        if nd["enc"] != bool(enc):
            raise ValueError("nfp_derived: this batch's NFP data was derived under the other row convention")
        return nd
    N, dev = pb.n_rows, pb.atom_id.device
    given = None if pb.nfp_self_w is None else (pb.nfp_self_w.to(dev), pb.nfp_deg_class.to(dev))
    if enc and (given is not None or pb.row_mol is None):
        raise ValueError("nfp_derived: an encoder-layout batch carries row_mol and no dense self_w / deg_class")
    bwd_w = pb.row_w
    if pb.atom_id.is_cuda:
        from . import _lib
        from ._lib import check, ptr, stream
        L = _lib.lib()
        if given is not None:
            self_w, deg_class = given
        else:
            if pb.row_mol is None:
                raise ValueError("NFP needs the batch's row -> molecule map (row_mol)")
            self_w = torch.empty(N, dtype=torch.float32, device=dev)
            deg_class = torch.empty(N, dtype=torch.int32, device=dev)
            if enc:
                bwd_w = torch.empty(N, dtype=torch.float32, device=dev)
                check(L.bmp_nfp_rows_enc(ptr(pb.csrT_ptr), ptr(pb.csrT_val), ptr(pb.row_mol), N, ptr(self_w), ptr(deg_class),
                                         ptr(bwd_w), stream()), "bmp_nfp_rows_enc")
            else:
                check(L.bmp_nfp_rows(ptr(pb.csrT_ptr), ptr(pb.csrT_val), ptr(pb.row_mol), ptr(pb.mol_row0), ptr(pb.mol_nrows), N,
                                     ptr(self_w), ptr(deg_class), stream()), "bmp_nfp_rows")
        idx = torch.empty(NUM_DEGREE_TYPE * N, dtype=torch.int32, device=dev)
        cnt = torch.empty(NUM_DEGREE_TYPE, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(L.bmp_nfp_deg_rows_ws_ints(N)), 8), dtype=torch.int32, device=dev)
        check(L.bmp_nfp_deg_rows(ptr(deg_class), N, ptr(idx), ptr(cnt), ptr(ws), stream()), "bmp_nfp_deg_rows")
    else:
        if given is not None:
            self_w, deg_class = given
        else:
            sw, dc = nfp_rows_host(pb, enc)
            self_w, deg_class = torch.from_numpy(sw), torch.from_numpy(dc)
            if enc:
                bwd_w = (pb.row_mol != -1).to(torch.float32)
        i, c = deg_rows_host(deg_class.numpy())
        idx, cnt = torch.from_numpy(i.reshape(-1)), torch.from_numpy(c)
    nd = dict(self_w=self_w, deg_class=deg_class, deg_rows=idx, deg_cnt=cnt, bwd_w=bwd_w, enc=bool(enc))
    pb._cache["nfp"] = nd
    return nd


def pad_count(eb) -> torch.Tensor:
    """[I] float32: the padded positions of every instance of an ``EncBatch`` -- row_w at the pad row of its per-instance rows."""
    pb = eb.pb
    return pb.row_w[pb.mol_row0.long() + pb.mol_nrows.long() - 1]


def inst_readout_host(g_real: torch.Tensor, pad: torch.Tensor, eb) -> torch.Tensor:
    """Reference semantics of bmp_nfp_inst_expand (``Fn.NFPInstFn``) on host tensors: g_inst[i] = g_real[uid[i]] + padcount[i]
    * pad, with g_real [U x o] the readout over the REAL atoms of every encoded molecule and pad [o] ``NFP.pad_term()``."""
    return g_real[eb.uid.long()] + pad_count(eb).to(g_real.dtype)[:, None] * pad


def pack_nfp_dense(atom_arrays: Sequence[np.ndarray], adjs: Sequence[np.ndarray], R: int = DEFAULT_R,
                   device="cpu") -> PackedMolBatch:
    """Pack the reference's NFP call form: per side ``atom_array`` (mb, A) int32 and ONE adjacency (mb, A, A) float32.  The
    off-diagonal entries go into the CSR with their values (bond type 0), the diagonal into ``self_w``, and ``deg_class``
    comes from the float32 column sums of the array as given.  A position is merged into the molecule's virtual pad row
    iff its atom id is 0 and its adjacency row AND column are all zero, diagonal included (the shared pad trajectory: it
    leaves each layer as sigmoid(B) and no row reads it); every other position is a row of its own.  Integer-exact."""
    inst_nrows_l, flat_atom_l, flat_w_l, sw_l, dc_l = [], [], [], [], []
    e_dst_l, e_src_l, e_val_l, side_l, dmf = [], [], [], [], []
    flat_base = 0
    for k, (atoms, adj) in enumerate(zip(atom_arrays, adjs)):
        atoms = np.asarray(atoms)
        adj = np.asarray(adj, dtype=np.float32)
        mb, A = atoms.shape
        if adj.shape != (mb, A, A):
            raise ValueError(f"adj shape {adj.shape} does not match atoms {atoms.shape}: NFP takes ONE (mb, A, A) adjacency")
        cls = deg_class_of(adj.sum(axis=1, dtype=np.float32))                      # column sums (nfp.py:157)
        diag = adj[:, np.arange(A), np.arange(A)]
        off = adj.copy()
        off[:, np.arange(A), np.arange(A)] = 0.0
        nzb, nzi, nzj = np.nonzero(off)
        padlike = (atoms == 0) & ~(adj != 0).any(axis=2) & ~(adj != 0).any(axis=1)
        real = ~padlike
        n = real.sum(axis=1).astype(np.int64)
        local = np.cumsum(real, axis=1) - 1
        nrows = n + 1
        o = flat_base + np.cumsum(nrows) - nrows
        dm = np.where(real, o[:, None] + local, (o + n)[:, None])                 # (mb, A) flat row
        tot = int(nrows.sum())
        fa = np.zeros(tot, dtype=np.int32); fw = np.ones(tot, dtype=np.float32)
        sw = np.zeros(tot, dtype=np.float32); dc = np.zeros(tot, dtype=np.int32)
        fa[dm[real] - flat_base] = atoms[real]
        sw[dm[real] - flat_base] = diag[real]
        dc[dm[real] - flat_base] = cls[real]
        fw[o + n - flat_base] = padlike.sum(axis=1).astype(np.float32)
        inst_nrows_l.append(nrows); flat_atom_l.append(fa); flat_w_l.append(fw); sw_l.append(sw); dc_l.append(dc)
        e_dst_l.append(dm[nzb, nzi]); e_src_l.append(dm[nzb, nzj]); e_val_l.append(off[nzb, nzi, nzj])
        side_l.append(np.full(mb, k, dtype=np.int64))
        dmf.append(dm)
        flat_base += tot
    e_dst = np.concatenate(e_dst_l)
    inst_nrows = np.concatenate(inst_nrows_l)
    pb = _assemble(inst_nrows, np.concatenate(flat_atom_l), np.concatenate(flat_w_l), e_dst, np.concatenate(e_src_l),
                   np.zeros(len(e_dst), dtype=np.int64), np.concatenate(e_val_l), np.concatenate(side_l), len(atom_arrays), R,
                   device, dmf)
    # flat row -> packed row: every instance's rows are consecutive from its mol_row0, in flat order
    rowmap = _ragged_arange(pb.mol_row0.cpu().numpy().astype(np.int64), inst_nrows)
    self_w = np.zeros(pb.n_rows, dtype=np.float32); deg_class = np.zeros(pb.n_rows, dtype=np.int32)
    self_w[rowmap] = np.concatenate(sw_l); deg_class[rowmap] = np.concatenate(dc_l)
    pb.nfp_self_w, pb.nfp_deg_class = torch.from_numpy(self_w).to(device), torch.from_numpy(deg_class).to(device)
    return pb


def as_packed_nfp(atom_array, adj, device) -> PackedMolBatch:
    """A packed batch in the first slot, or the reference's dense pair (atom_array (mb, A) int32, adj (mb, A, A) float32)."""
    if isinstance(atom_array, PackedMolBatch):
        return atom_array
    if _is_float_atoms(atom_array):
        raise NotImplementedError("float atom features (embedding bypass, models/models/nfp.py:146-147) are not supported")
    if adj is None:
        raise ValueError("NFP needs the adjacency with the dense atom array")
    a = atom_array.detach().cpu().numpy() if isinstance(atom_array, torch.Tensor) else np.asarray(atom_array)
    j = adj.detach().cpu().numpy() if isinstance(adj, torch.Tensor) else np.asarray(adj)
    return pack_nfp_dense([a.astype(np.int32)], [j.astype(np.float32)], device=device)


# ---------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------
class NFPUpdate(nn.Module):
    """models/models/nfp.py:15-62: seven GraphLinear(in, out), one per degree 1..7; out = sigmoid(sum_k W_k where(deg == k, fv))."""

    _fused = True               # private switch: False takes the row-wise kernels (and the row-wise weight gradient) at every width

    def __init__(self, in_channels, out_channels, max_degree=6):
        super().__init__()
        if max_degree != NUM_DEGREE_TYPE - 1:
            raise NotImplementedError("max_degree must be 6 (seven degree classes)")
        if in_channels % 8 or out_channels % 8:
            raise ValueError("channel counts must be multiples of 8")
        self.graph_linears = nn.ModuleList([Linear(in_channels, out_channels) for _ in range(max_degree + 1)])
        self.max_degree, self.in_channels, self.out_channels = max_degree, in_channels, out_channels

    def bias_sum(self):
        """B: every GraphLinear adds its bias to every row."""
        return torch.stack([lin.b for lin in self.graph_linears]).sum(dim=0)

    def forward(self, h, pb: PackedMolBatch, enc: bool = False):
        """``enc``: ``pb`` is an ``EncBatch.pb_enc`` (``nfp_derived``)."""
        WT = torch.stack([lin.W.t() for lin in self.graph_linears])               # [7 x d_in x d_out]
        return Fn.NFPLayerFn.apply(h, WT, self.bias_sum(), pb, nfp_derived(pb, enc), self._fused)


class NFPReadout(nn.Module):
    """models/models/nfp.py:65-91: softmax over the channels of GraphLinear(h), summed over all positions."""

    _fused = True               # private switch, as NFPUpdate's

    def __init__(self, in_channels, out_size):
        super().__init__()
        if in_channels % 8 or out_size % 4:
            raise ValueError("in_channels must be a multiple of 8 and out_size a multiple of 4")
        self.output_weight = Linear(in_channels, out_size)
        self.in_channels, self.out_size = in_channels, out_size

    def forward(self, h, pb: PackedMolBatch, g_prev: Optional[torch.Tensor] = None):
        return Fn.NFPReadoutFn.apply(h, self.output_weight.W.t(), self.output_weight.b, pb, g_prev, self._fused)



class NFP(nn.Module):
    """models/models/nfp.py:94-179."""

    def __init__(self, out_dim, hidden_dim=16, n_layers=4, max_degree=6, n_atom_types=MAX_ATOMIC_NUM, concat_hidden=False):
        super().__init__()
        if concat_hidden:
            # the reference concatenates 2-d arrays along axis 2 there and cannot run
            raise NotImplementedError("concat_hidden=True calls concat(axis=2) on (mb, out_dim) arrays in the reference "
                                      "(models/models/nfp.py:173) and cannot run there")
        self.embed = EmbedID(out_size=hidden_dim, in_size=n_atom_types)
        self.layers = nn.ModuleList([NFPUpdate(hidden_dim, hidden_dim, max_degree=max_degree) for _ in range(n_layers)])
        self.read_out_layers = nn.ModuleList([NFPReadout(hidden_dim, out_dim) for _ in range(n_layers)])
        self.out_dim, self.hidden_dim, self.max_degree = out_dim, hidden_dim, max_degree
        self.num_degree_type, self.n_layers, self.concat_hidden = max_degree + 1, n_layers, concat_hidden
        self.atoms = None
        self._enc = None        # (g_real, pad term) between encode_rows and readout_enc

    def plannable(self) -> bool:
        return False            # no layout plan: FlatAdam / fit leave the encoder to autograd (bmp/dp.py)

    def forward(self, atom_array, adj=None):
        pb = as_packed_nfp(atom_array, adj, self.embed.W.device)
        if pb.oversized:
            raise NotImplementedError(f"NFP: a molecule of this batch has more than {pb.R - 1} atoms (it spans tiles)")
        if not pb.atom_id.is_cuda:
            raise RuntimeError("NFP runs on the GPU only: there is no CPU path (move the model and the batch to the device)")
        pb.check_atom_ids(self.embed.W.shape[0])
        h = Fn.EmbedFn.apply(self.embed.W, pb.atom_id)
        g = None
        for update, readout in zip(self.layers, self.read_out_layers):           # :163-166
            h = update(h, pb)
            g = readout(h, pb, g)
        self.atoms = PackedAtoms(h, pb, 0 if pb.dense_map is not None else None)
        return g

    def encode_rows(self, pb: PackedMolBatch):
        """The encoder on the rows of an ``EncBatch.pb_enc`` (bmp/enclayout.py), layers AND per-layer readout: returns
        (h_last, None).  The readout there sums over the REAL atoms of every encoded molecule (the pad rows have row_w == 0, no
        molecule owns them); ``readout_enc``, the partner call, adds every instance's padded positions from the parameters alone."""
        if _is_float_atoms(pb):
            raise NotImplementedError("float atom features (embedding bypass, models/models/nfp.py:146-147) are not supported")
        if not isinstance(pb, PackedMolBatch) or pb.mt_row0 is None or pb.row_mol is None:
            raise ValueError("NFP.encode_rows takes the encoder layout of an EncBatch (pb_enc)")
        if not pb.atom_id.is_cuda:
            raise RuntimeError("NFP runs on the GPU only: there is no CPU path (move the model and the batch to the device)")
        pb.check_atom_ids(self.embed.W.shape[0])
        h = Fn.EmbedFn.apply(self.embed.W, pb.atom_id)
        g = None
        for update, readout in zip(self.layers, self.read_out_layers):
            h = update(h, pb, enc=True)
            g = readout(h, pb, g)
        self._enc = (g, self.pad_term())
        return h, None

    def pad_term(self):
        """[o]: what ONE padded position adds to a molecule's readout, summed over the layers.  Atom id 0, an empty adjacency row
        and column and degree class 0 leave layer l as sigmoid(B_l) whatever the molecule and whatever h was before, so its term is
        softmax(sigmoid(B_l) . Wo_l^T + bo_l): a function of the parameters alone, plain torch on o-vectors for all layers at once
        (no BLAS call: a fixed order), differentiable."""
        B = torch.stack([up.bias_sum() for up in self.layers])                                # [L x d]
        Wo = torch.stack([ro.output_weight.W for ro in self.read_out_layers])                 # [L x o x d]
        bo = torch.stack([ro.output_weight.b for ro in self.read_out_layers])                 # [L x o]
        return torch.softmax((Wo * torch.sigmoid(B)[:, None, :]).sum(dim=2) + bo, dim=1).sum(dim=0)

    def readout_enc(self, eb):
        """The molecule vector of every INSTANCE of the ``EncBatch`` whose ``pb_enc`` the last ``encode_rows`` ran on."""
        if self._enc is None:
            raise RuntimeError("NFP.readout_enc follows NFP.encode_rows on the same EncBatch")
        g_real, pad = self._enc
        self._enc = None
        return Fn.NFPInstFn.apply(g_real, pad, eb)

    def get_atom_array(self):
        assert self.atoms is not None
        return self.atoms
