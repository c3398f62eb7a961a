"""Float64 packed restatement of the segment operators of csrc/bmp_seg.hip and of the five coarse co-attention modules
built on them (test infrastructure, not product; plain torch on the CPU, differentiable through autograd).

Every operator works on exactly the tensors its kernel sees: packed rows [N x c], the row multiplicities ``w``, the
molecule ranges ``row0`` / ``nrows`` and ``row_mol`` (the molecule of every row, -1 for a row of no molecule).  A row of no
molecule gives 0 in every per-row output and takes part in no per-molecule sum.  tests/test_seg_ref.py pins the modules
to the dense oracle (oracle/ref_cpu.py) on ``pb.to_dense`` and the operators to hand-computed answers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

Tensor = torch.Tensor
ACT = {"identity": lambda x: x, "tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid}


def _live(row0: Tensor, nrows: Tensor) -> Tuple[Tensor, Tensor]:
    """(row index, molecule index) of every row inside a molecule range, molecule by molecule."""
    r0, nr = row0.long().cpu(), nrows.long().cpu()
    mol = torch.repeat_interleave(torch.arange(r0.numel()), nr)
    idx = torch.repeat_interleave(r0 - (torch.cumsum(nr, 0) - nr), nr) + torch.arange(int(nr.sum()))
    return idx, mol


def row_mol_of(row0: Tensor, nrows: Tensor, N: int) -> Tensor:
    idx, mol = _live(row0, nrows)
    return torch.full((N,), -1, dtype=torch.long).index_put((idx,), mol)


def segpool(A: Tensor, Y: Tensor, w: Tensor, row0: Tensor, nrows: Tensor) -> Tensor:
    """out[m, c] = sum over the molecule's rows of w[r] * A[r, c or 0] * Y[r, c];  A is [N x 1] or [N x o]."""
    N, o = Y.shape
    assert A.shape in ((N, 1), (N, o))
    idx, mol = _live(row0, nrows)
    term = w.to(Y.dtype)[:, None] * A * Y
    return torch.zeros(row0.numel(), o, dtype=Y.dtype).index_add(0, mol, term[idx])


def segsoftmax(s: Tensor, w: Tensor, row0: Tensor, nrows: Tensor) -> Tensor:
    """alpha[r] = exp(s[r]) / sum over the molecule's rows of w * exp(s): the multiplicities count in the denominator only.
    A row of multiplicity 0 stands for no position at all: alpha = 0 there, and it does not enter the sum."""
    idx, mol = _live(row0, nrows)
    M = row0.numel()
    sl, wl = s[idx], w.to(s.dtype)[idx]
    on = wl > 0
    mx = torch.full((M,), -float("inf"), dtype=s.dtype).scatter_reduce(
        0, mol[on], sl.detach()[on], reduce="amax", include_self=True)
    e = torch.where(on, torch.exp(torch.where(on, sl - mx[mol], torch.zeros_like(sl))), torch.zeros_like(sl))
    den = torch.zeros(M, dtype=s.dtype).index_add(0, mol, wl * e)
    return torch.zeros_like(s).index_put((idx,), e / den[mol])


def rowbcast(q: Tensor, row_mol: Tensor) -> Tensor:
    """out[r, :] = q[row_mol[r], :], 0 for a row of no molecule."""
    rm = row_mol.long()
    return torch.where((rm >= 0)[:, None], q[rm.clamp(min=0)], torch.zeros((), dtype=q.dtype))


def rowdot(x: Tensor, u: Tensor, s0: Optional[Tensor], row_mol: Tensor) -> Tensor:
    """s[r] = x[r, :] . u[row_mol[r], :] + s0[row_mol[r]], 0 for a row of no molecule."""
    rm = row_mol.long()
    on, m = rm >= 0, rm.clamp(min=0)
    s = (x * u[m]).sum(dim=1)
    if s0 is not None:
        s = s + s0[m]
    return torch.where(on, s, torch.zeros((), dtype=x.dtype))


def rowcorr(a: Tensor, q: Tensor, row0: Tensor, nrows: Tensor) -> Tensor:
    """e[r, k] = sum_t a[r, t] * q[m, (t + k) mod o] for the rows of molecule m: the direct double sum, no FFT."""
    N, o = a.shape
    k = torch.arange(o)
    rot = (k[None, :] + k[:, None]) % o                      # rot[k, t] = (t + k) mod o
    e = torch.zeros_like(a)
    for m, (r0, nr) in enumerate(zip(row0.tolist(), nrows.tolist())):
        rows = torch.arange(r0, r0 + nr)
        e = e.index_put((rows,), a[r0:r0 + nr] @ q[m][rot].t())
    return e


# ------------------------------------------------------------------------------------------------ the modules
@dataclass
class Side:
    """The atoms one focus of a coarse module attends over: rows and the index tensors of its molecules."""
    X: Tensor
    w: Tensor
    row0: Tensor
    nrows: Tensor
    row_mol: Tensor

    @property
    def M(self) -> int:
        return self.row0.numel()

    def pool(self, A, Y):
        return segpool(A, Y, self.w, self.row0, self.nrows)

    def mean(self):
        """Mean over ALL padded positions of the molecule (the multiplicities are positions)."""
        ones = torch.ones(self.X.shape[0], 1, dtype=self.X.dtype)
        return self.pool(ones, self.X) / self.pool(ones, ones)


def sides_of(pb, X: Tensor, X2: Optional[Tensor] = None, pb2=None) -> Tuple[Side, Side]:
    """The two sides of one two-sided packed batch (rows X), or of two one-sided batches (pb, X) and (pb2, X2)."""
    def one(b, rows, lo, hi):
        r0, nr = b.mol_row0.cpu()[lo:hi], b.mol_nrows.cpu()[lo:hi]
        return Side(rows, b.row_w.cpu().to(rows.dtype), r0, nr, row_mol_of(r0, nr, rows.shape[0]))
    if pb2 is not None:
        return one(pb, X, 0, pb.n_mols), one(pb2, X2, 0, pb2.n_mols)
    assert len(pb.side_mols) == 3
    return one(pb, X, pb.side_mols[0], pb.side_mols[1]), one(pb, X, pb.side_mols[1], pb.side_mols[2])


def _lin(x, W, b=None):
    y = x @ W.t()
    return y if b is None else y + b


def parallel(p: Dict[str, Tensor], s1: Side, g_1, s2: Side, g_2, activation="tanh", weight_tying=True, prefix=""):
    """ParallelCoattention (head 1): gate[r] = act(bilinear(atom, the OTHER molecule's readout)), no softmax."""
    P = lambda k: p[prefix + k]

    def side(s, q, focus):
        li = 0 if weight_tying else focus - 1
        W, V1 = P(f"energy_layers/{li}/W")[:, :, 0], P(f"energy_layers/{li}/V1")[:, 0]
        V2, b = P(f"energy_layers/{li}/V2")[:, 0], P(f"energy_layers/{li}/b")[0]
        u = q @ W.t() + V1                                   # [M x hidden]: x^T W q + x . V1 = x . (W q + V1)
        e = ACT[activation](rowdot(s.X, u, q @ V2 + b, s.row_mol))
        return s.pool(e[:, None], _lin(s.X, P("j_layer/W"), P("j_layer/b")))
    return side(s1, g_2, 1), side(s2, g_1, 2)


def circ(p, s1: Side, g_1, s2: Side, g_2, activation="tanh", prefix=""):
    """CircularParallelCoattention: gate = act(circular correlation of j_layer(atom) with the other readout)."""
    def side(s, q):
        J = _lin(s.X, p[prefix + "j_layer/W"], p[prefix + "j_layer/b"])
        return s.pool(ACT[activation](rowcorr(J, q, s.row0, s.nrows)), J)
    return side(s1, g_2), side(s2, g_1)


def alternating(p, s1: Side, g_1, s2: Side, g_2, prefix=""):
    """AlternatingCoattention, weight_tying=True; the side-2 query is the side-1 output."""
    P = lambda k: p[prefix + k]
    W1, b1 = P("energy_layers_1/0/W"), P("energy_layers_1/0/b")
    W2, b2 = P("energy_layers_2/0/W"), P("energy_layers_2/0/b")
    o = P("j_layer/W").shape[0]

    def side(s, q):
        t = torch.tanh(_lin(s.X, W1[:, o:]) + rowbcast(_lin(q, W1[:, :o], b1), s.row_mol))     # concat((query, key))
        alpha = segsoftmax(_lin(t, W2, b2)[:, 0], s.w, s.row0, s.nrows)
        return s.pool(alpha[:, None], _lin(s.X, P("j_layer/W"), P("j_layer/b")))
    c1 = side(s1, g_2)
    return c1, side(s2, c1)


def global_(p, s1: Side, s2: Side, weight_tying=True, prefix=""):
    """GlobalCoattention: gate = sigmoid(Linear(concat((atom, mean of the other molecule's atoms))))."""
    P = lambda k: p[prefix + k]
    d = P("lt_layer/W").shape[1]

    def side(s, q, focus):
        li = 0 if weight_tying else focus - 1
        W, b = P(f"att_layers/{li}/W"), P(f"att_layers/{li}/b")
        attn = torch.sigmoid(_lin(s.X, W[:, :d]) + rowbcast(_lin(q, W[:, d:], b), s.row_mol))
        return s.pool(attn, _lin(s.X, P("lt_layer/W"), P("lt_layer/b")))
    return side(s1, s2.mean(), 1), side(s2, s1.mean(), 2)


def neural(p, s1: Side, s2: Side, activation="relu", weight_tying=True, prefix="", pre_out=None, energy_out=None):
    """NeuralCoattention: doc = act(Linear(atom)), context = act(Linear(mean of the other)), gate = sigmoid(doc . context).
    ``pre_out``: a list that receives the pre-activations (of the molecules' rows and of the queries) for the kink check;
    ``energy_out``: one that receives doc . context of the molecules' rows (is the gate off its flat ends?)."""
    P = lambda k: p[prefix + k]

    def side(s, q, focus):
        li = 0 if weight_tying else focus - 1
        W, b = P(f"att_layers/{li}/W"), P(f"att_layers/{li}/b")
        pre_q, pre_x = _lin(q, W, b), _lin(s.X, W, b)
        if pre_out is not None:
            pre_out.extend([pre_q.detach(), pre_x.detach()[s.row_mol >= 0]])
        doc = ACT[activation](pre_x)
        energy = rowdot(doc, ACT[activation](pre_q), None, s.row_mol)
        if energy_out is not None:
            energy_out.append(energy[s.row_mol >= 0])
        return s.pool(torch.sigmoid(energy)[:, None], doc)
    return side(s1, s2.mean(), 1), side(s2, s1.mean(), 2)


# ------------------------------------------------------------------------------------ the relu case of Neural
# A float32 kernel may put a relu pre-activation on the other side of 0 than the float64 reference does when it lies
# within the comparison tolerance of 0; the gradient then takes the other branch and no tolerance covers that.  The relu
# case therefore uses parameters whose every pre-activation clears KINK_FACTOR x 1e-4 x max|pre|.  With unit-variance
# pre-activations that cannot hold for ~5e4 of them (the expected number inside the band is above a hundred), so the case
# gives each output column a bias of +-KINK_BIAS standard deviations: a column is then mostly on one side of 0 and a few
# tens of rows cross.  The condition does not depend on the scale of W and b, so both are then scaled by RELU_SCALE, which
# brings doc . context from ~240 (a gate of exactly 1, and a gradient of exactly 0 through it) to ~2.4, where the gate,
# the dot product in front of it and the relu of the query all carry gradient.  About half of the seeds clear the band;
# the case uses RELU_SEED, and tests/test_seg_ref.py asserts the band and the live gate for it.
KINK_FACTOR = 8.0
KINK_BIAS = 3.5
RELU_SCALE = 0.1
RELU_CASE = dict(hidden_dim=72, out_dim=40, weight_tying=False)
RELU_SEED = 3
RELU_SEEDS = (1, 3, 4, 5)          # seeds that cleared the band when the case was set up (0 and 2 did not)


def relu_case_params(seed: int, dtype=torch.float64) -> Dict[str, Tensor]:
    from oracle import ref_cpu as O
    dr = O._Draw(1000 + seed, dtype, 0.2)
    O.init_neural(dr, "", RELU_CASE["hidden_dim"], RELU_CASE["out_dim"], weight_tying=RELU_CASE["weight_tying"])
    sign = torch.tensor([1.0, -1.0], dtype=dtype).repeat(RELU_CASE["out_dim"] // 2)
    return {k: RELU_SCALE * (v + KINK_BIAS * sign if k.endswith("/b") else v) for k, v in dr.p.items()}


def kink_margin(pres) -> Tuple[float, float]:
    """(min |pre|, max |pre|) over a list of pre-activation tensors."""
    flat = torch.cat([t.reshape(-1) for t in pres]).abs()
    return flat.min().item(), flat.max().item()


# ------------------------------------------------------------------------------------------- the shared batch
# Atom counts of the operator and module tests.  With the virtual pad row the molecules have 2, 3, 4, 5, 6, 64, 65, 66, 128,
# 131 and 301 rows: nrows mod 4 takes every value, 64 / 65 / 66 straddle the softmax kernels' 64-row wrap, 128 fills a
# tile, 131 and 301 span two and three tiles and leave tail rows that belong to no molecule.
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 130, 300)
# side-2 partner of every side-1 molecule: equal sizes at 1, 4, 64 and 300 atoms, unequal everywhere else.  Each side holds
# the 300-atom molecule, so that one's pad row has multiplicity 0 on either side and every other pad row more than 1.
PARTNER = (0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 10)


def make_store(sizes=SIZES, seed=0):
    import numpy as np
    from bmp import synth
    rs = np.random.RandomState(seed)
    lone = lambda: synth.Molecule(atoms=np.array([8], np.int32), bonds=np.zeros((0, 3), np.int32))
    return [lone() if n == 1 else synth._make_molecule(rs, n, n, float(n)) for n in sizes]


def fixture_batch(sizes=SIZES, partner=PARTNER, with_dense_map=False):
    """(two-sided batch, side-1-only batch, side-2-only batch), on the CPU."""
    import numpy as np
    from bmp import packed
    ms = packed.MolStore(make_store(sizes))
    i1, i2 = np.arange(len(sizes)), np.asarray(partner)
    pack = lambda sides: packed.pack_from_store(ms, sides, device="cpu", with_dense_map=with_dense_map)
    return pack([i1, i2]), pack([i1]), pack([i2])


def relu_case_inputs(seed: int):
    """(parameters, X) of Neural's relu case on the shared batch; float32 values held in float64, so that the kernel
    starts from the very numbers the kink condition was checked on."""
    pb = fixture_batch()[0]
    X = torch.randn(pb.n_rows, RELU_CASE["hidden_dim"], generator=torch.Generator().manual_seed(500 + seed),
                    dtype=torch.float64)
    return {k: v.float().double() for k, v in relu_case_params(seed).items()}, X.float().double()


def relu_case_margin(seed: int) -> Tuple[float, float]:
    p, X = relu_case_inputs(seed)
    pres = []
    neural(p, *sides_of(fixture_batch()[0], X), activation="relu", weight_tying=RELU_CASE["weight_tying"], pre_out=pres)
    return kink_margin(pres)
