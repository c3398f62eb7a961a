"""The hidden-width-32 cases of the fuse-gate and simple-gate GGNN encoders: tests/ggate_ref.py's restatement (imported, not
copied) with a CASES table of its own, the data set "blocks", and the restatement of the recorded pair model cut down
(fuse-gate encoder, no co-attention, HolE link predictor: RECORD.txt:404-405).

At hidden = 32 on whole tiles the steps run on the wave-local kernels of csrc/bmp_gate_small.hip: one wave per 32-row block of a
128-row tile, and the message product of a bond type is skipped for a wave whose 32 rows hold no bond of that type.  "blocks" is
the one input on which that skip and a wave without any bond can go wrong: ONE tile whose four 32-row blocks are
    block 0   bonds of a single type only (a chain of 31 atoms with double bonds, and its pad row),
    block 1   all four bond types (a chain of 31 atoms whose bonds cycle through the types, and its pad row),
    block 2   molecules and no bond at all (16 single atoms, each with its pad row of multiplicity 30),
    block 3   empty fill past the last molecule (rows of no molecule).
``blocks_property`` reads that back from the packed batch's CSR.

"dense" is one tile whose CSR has more entries than the kernels stage in LDS (FZ_ECAP = 1024, csrc/bmp_tile.h): one molecule of
127 atoms, every atom bonded to its next five along the chain (620 bonds of all four types = 1240 entries per direction), so
both directions gather through the CSR in global memory.  ``dense_property`` reads that back.
"""
import math

import numpy as np
import torch

import link_ref as LR
from gin_ref import data as _gin_data
from ggate_ref import forward, make_params, case_params, case_forward, keep_dense, FUSE_DROPOUT      # noqa: F401

_DATA = {}


def _blocks_store():
    from bmp import synth
    rs = np.random.RandomState(32)
    atoms = lambda n: synth._ATOM_Z[rs.choice(len(synth._ATOM_Z), size=n, p=synth._ATOM_P)].astype(np.int32)
    chain = lambda types: np.asarray([(i, i + 1, t) for i, t in enumerate(types)], dtype=np.int32).reshape(-1, 3)
    mols = [synth.Molecule(atoms(31), chain([1] * 30)),                       # block 0: double bonds only
            synth.Molecule(atoms(31), chain([i % 4 for i in range(30)]))]     # block 1: all four types
    mols += [synth.Molecule(atoms(1), np.zeros((0, 3), np.int32)) for _ in range(16)]      # block 2: no bond at all
    return mols


STAGED_CSR_ENTRIES = 1024      # FZ_ECAP (csrc/bmp_tile.h; tests/test_ggate32_ref.py reads it back from the source)


def _dense_store():
    from bmp import synth
    rs = np.random.RandomState(33)
    n = 127
    atoms = synth._ATOM_Z[rs.choice(len(synth._ATOM_Z), size=n, p=synth._ATOM_P)].astype(np.int32)
    bonds = [(i, i + k, (i + k) % 4) for i in range(n) for k in range(1, 6) if i + k < n]
    return [synth.Molecule(atoms, np.asarray(bonds, dtype=np.int32))]


def dense_property(pb):
    """True iff ``pb`` is one whole tile with more CSR entries, in either direction, than the kernels stage in LDS."""
    return (pb.n_tiles == 1 and not pb.oversized and int(pb.csr_ptr[128]) > STAGED_CSR_ENTRIES
            and int(pb.csrT_ptr[128]) > STAGED_CSR_ENTRIES)


def data(name):
    """gin_ref.data's sets ("fixture", "small", "oversized"), "blocks" and "dense" (module docstring), in the same form."""
    if name not in ("blocks", "dense"):
        return _gin_data(name)
    if name not in _DATA:
        from bmp import packed, synth
        store = _blocks_store() if name == "blocks" else _dense_store()
        idx = [np.arange(len(store))]
        pb = packed.pack_from_store(packed.MolStore(store), idx, device="cpu", with_dense_map=True)
        _DATA[name] = dict(store=store, idx=idx, pb=pb, sides=[synth.concat_mols(store)])
    return _DATA[name]


def block_types(pb, transposed=False):
    """Per 32-row block of the batch: (set of the bond types among its rows' CSR entries, number of its rows that belong to a
    molecule)."""
    ptr = (pb.csrT_ptr if transposed else pb.csr_ptr).cpu().numpy()
    col = (pb.csrT_col if transposed else pb.csr_col).cpu().numpy()
    rm = pb.row_mol.cpu().numpy()
    out = []
    for b in range(pb.n_rows // 32):
        r0, r1 = 32 * b, 32 * b + 32
        out.append((set(int(t) for t in col[ptr[r0]:ptr[r1]] & 3), int((rm[r0:r1] >= 0).sum())))
    return out


def blocks_property(pb):
    """True iff ``pb`` is one tile laid out as the module docstring says, in the CSR and in the transposed CSR."""
    want = [({1}, 32), ({0, 1, 2, 3}, 32), (set(), 32), (set(), 0)]
    w = pb.row_w.cpu().numpy()
    return (pb.n_tiles == 1 and not pb.oversized and block_types(pb) == want and block_types(pb, True) == want
            and bool((w[64:96:2] == 1).all()) and bool((w[65:96:2] == 30).all()))


def keep_rows(name, hidden, steps, seed, p=FUSE_DROPOUT):
    """ggate_ref.keep_rows on this module's data sets."""
    g = torch.Generator().manual_seed(seed)
    n = data(name)["pb"].n_rows
    return [(torch.rand(n, hidden, generator=g) >= p).float() * (1.0 / (1.0 - p)) for _ in range(steps)]


def keep_dense32(name, rows, side):
    dm = data(name)["pb"].dense_maps[side]
    return [k[dm] for k in rows]


# name: kind, seed, hidden, out, layers, tying, update_tying, data.  Beside each row: the worst max-norm relative distance of the
# float32 restatement from the float64 one over g, the atom states and every parameter gradient (tests/test_ggate32_ref.py
# prints it; fuse_pair32: logits, loss and gradients of the pair model), against the bound 1e-4 of parity_util.close.
CASES = {
    "fuse32": dict(kind="fuse", seed=31, hidden=32, out=16, layers=3, tying=False, update_tying=True, data="fixture"),        # 8.3e-7
    "gate32": dict(kind="gate", seed=32, hidden=32, out=16, layers=3, tying=True, update_tying=True, data="fixture"),         # 8.0e-7
    "gate32u": dict(kind="gate", seed=33, hidden=32, out=16, layers=3, tying=True, update_tying=False, data="fixture"),       # 7.6e-7
    "fuse_keep32": dict(kind="fuse", seed=34, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="fixture"),   # 1.1e-6
    "fuse_over32": dict(kind="fuse", seed=35, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="oversized"),  # 5.7e-6
    "gate_over32": dict(kind="gate", seed=36, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="oversized"),  # 6.7e-6
    "fuse_small32": dict(kind="fuse", seed=37, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="small"),    # 4.0e-7
    "fuse_blocks32": dict(kind="fuse", seed=38, hidden=32, out=16, layers=3, tying=False, update_tying=True, data="blocks"),  # 2.5e-6
    "gate_blocks32": dict(kind="gate", seed=39, hidden=32, out=16, layers=3, tying=False, update_tying=False, data="blocks"),  # 1.6e-6
    "fuse_dense32": dict(kind="fuse", seed=42, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="dense"),    # 3.8e-7
    "gate_dense32": dict(kind="gate", seed=43, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="dense"),    # 3.7e-7
    "fuse_pair32": dict(kind="fuse", seed=40, hidden=32, out=16, layers=2, tying=False, update_tying=True, data="fixture"),   # 3.5e-7
}


def reference(name, concat=False, keep_seed=None, dtype=torch.float64):
    """The restatement of a case on every side of its data, differentiated once:
    dict(p (leaves with .grad), g, atoms [per side], cg, ca, keep (row masks or None))."""
    c = CASES[name]
    d = data(c["data"])
    p = {k: v.to(dtype).requires_grad_() for k, v in case_params(c, concat).items()}
    kr = None if keep_seed is None else keep_rows(c["data"], c["hidden"], c["layers"], keep_seed)
    outs = []
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else keep_dense32(c["data"], kr, side)
        outs.append(case_forward(c, p, atoms, adj, concat, keep=kd))
    g = torch.cat([o[0] for o in outs])
    gen = torch.Generator().manual_seed(5)
    cg = torch.randn(g.shape, dtype=torch.float64, generator=gen)
    ca = [torch.randn(o[1].shape, dtype=torch.float64, generator=gen) for o in outs]
    ((g * cg.to(dtype)).sum() + 0.1 * sum((o[1] * w.to(dtype)).sum() for o, w in zip(outs, ca))).backward()
    return dict(p=p, g=g.detach(), atoms=[o[1].detach() for o in outs], cg=cg, ca=ca, keep=kr)


# ---- the recorded pair model, cut down: fuse-gate encoder -> HolE (circular correlation, relu MLP 16 -> 32 -> 16 -> 1) ----
PAIR_CASE, PAIR_KEEP_SEED, PAIR_HIDDEN_DIMS = "fuse_pair32", 13, (32, 16)


def pair_params(dtype=torch.float64):
    """graph_conv/... from the case, mlp/layers/{0,1}/{W,b} and mlp/l_out/{W,b} of the HolE predictor."""
    c = CASES[PAIR_CASE]
    p = case_params(c, prefix="graph_conv/")
    g = torch.Generator().manual_seed(41)
    dims = [c["out"]] + list(PAIR_HIDDEN_DIMS) + [1]
    for i in range(len(dims) - 1):
        key = f"mlp/layers/{i}" if i < len(PAIR_HIDDEN_DIMS) else "mlp/l_out"
        p[key + "/W"] = torch.randn(dims[i + 1], dims[i], dtype=torch.float64, generator=g) / math.sqrt(dims[i])
        p[key + "/b"] = 0.3 * torch.randn(dims[i + 1], dtype=torch.float64, generator=g)
    return {k: v.to(dtype) for k, v in p.items()}


def pair_labels():
    return np.random.RandomState(4).randint(0, 2, (13, 1)).astype(np.int32)


def pair_reference(dtype=torch.float64):
    """dict(p, keep, y, loss, grads {name: tensor}, pre (the relu layers' pre-activations)) of one training-mode forward and
    backward of the pair model on "fixture" with the masks given."""
    from oracle import ref_cpu as O
    c = CASES[PAIR_CASE]
    d = data(c["data"])
    q = {k: v.clone().requires_grad_() for k, v in pair_params(dtype).items()}
    kr = keep_rows(c["data"], c["hidden"], c["layers"], PAIR_KEEP_SEED)
    g = [case_forward(c, q, *d["sides"][s], keep=keep_dense32(c["data"], kr, s), prefix="graph_conv/")[0] for s in (0, 1)]
    h = LR.hole(g[0], g[1])
    pre = []
    for i in range(len(PAIR_HIDDEN_DIMS)):
        a = h @ q[f"mlp/layers/{i}/W"].t() + q[f"mlp/layers/{i}/b"]
        pre.append(a.detach())
        h = torch.relu(a)
    y = h @ q["mlp/l_out/W"].t() + q["mlp/l_out/b"]
    loss = O.sigmoid_cross_entropy(y, torch.from_numpy(pair_labels()))
    names = sorted(q)
    gr = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    grads = {n: (x if x is not None else torch.zeros_like(q[n])) for n, x in zip(names, gr)}
    return dict(p=q, keep=kr, y=y.detach(), loss=loss.detach(), grads=grads, pre=pre)
