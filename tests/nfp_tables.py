"""The molecule store of the NFP table tests (tests/test_nfp_table_build.py, tests/test_gpu_nfp_table.py).  The stores of
tests/table_harness.py do not exercise the degree-class walk: the hand-made store is chains (column sums 2 / 3 / 4), the dense
store 123 hubs of class 0 plus four atoms of classes 6 and 7, the synthetic world has no class 1, 6, 7 and no real class-0 atom.

This store has the atom counts of tests/enc_tables.py (31, 32, 33, 63, 64, 95, 96, 127, 2, 5) -- the plan reads atom counts only,
so the three tables keep their mt_row0 / mt_nblk and their block-boundary cases, which ``table`` asserts -- plus one single-atom
molecule (class 1 by its self loop alone) behind them, which the tables do not index and the second world does.  Its bonds are
stars on a caterpillar: a molecule of 25 atoms or more opens with a spine of six atoms with 8, 6, 5, 4, 3 and 2 bonds (with the
self loop: class 0 -- a centre with seven bonds or more --, 7, 6, 5, 4, 3), one atom without a bond (class 1) and the spine's
eighteen leaves (class 2); a chain hangs the remaining atoms on the last leaf.  ``check_classes`` asserts what the tests need of
it.  No GPU and no GPU helper is imported here."""
import types

import numpy as np

from enc_tables import COUNTS, TABLES, _hand_store

SPINE_BONDS = (8, 6, 5, 4, 3, 2)
SINGLE = len(COUNTS)                                   # the store index of the single-atom molecule
_CACHE = {}


def _molecule(n, rs):
    from bmp import synth
    atoms = synth._ATOM_Z[rs.choice(len(synth._ATOM_Z), size=n, p=synth._ATOM_P)].astype(np.int32)
    bonds = []
    if n >= 25:
        S = len(SPINE_BONDS)
        bonds += [(i, i + 1) for i in range(S - 1)]
        leaf = S + 1                                   # atom S has no bond
        for i, nb in enumerate(SPINE_BONDS):
            for _ in range(nb - (1 if i in (0, S - 1) else 2)):
                bonds.append((i, leaf)); leaf += 1
        assert leaf == 25
        bonds += [(k - 1, k) for k in range(25, n)]
    elif n > 1:
        bonds += [(0, k) for k in range(1, n)]         # a star
    b = np.asarray([(i, j, (i + j) % 4) for i, j in bonds], dtype=np.int32).reshape(-1, 3)
    return synth.Molecule(atoms, b)


def store():
    if "store" not in _CACHE:
        rs = np.random.RandomState(78)
        _CACHE["store"] = [_molecule(n, rs) for n in COUNTS + [1]]
    return _CACHE["store"]


def table(name):
    """Host EncBatch without dedup of one of the three tables of tests/enc_tables.py on this store; its tile table is the
    hand-made store's."""
    if name not in _CACHE:
        from bmp import enclayout, packed
        inst, n_cu = TABLES[name]
        ms, hand = packed.MolStore(store()), packed.MolStore(_hand_store())
        eb = enclayout.encode_from_store(ms, [np.asarray(inst)], dedup=False, n_cu=n_cu)
        pl = enclayout.plan_enc_numpy(hand.n_atoms, hand.nedges, np.asarray(inst), False, n_cu)
        assert eb.pb_enc.mt_row0.tolist() == pl["mt_row0"].tolist() and eb.pb_enc.mt_nblk.tolist() == pl["mt_nblk"].tolist()
        assert eb.enc_row0.tolist() == pl["row0"].tolist() and eb.enc_pad.tolist() == pl["enc_pad"].tolist()
        assert eb.pb_enc.tile_stride == 0 and not eb.pb_enc.oversized and eb.pb_enc.n_rows < 800
        _CACHE[name] = eb
    return _CACHE[name]


def check_classes(pb_enc, nd):
    """What the tests ask of a table on this store: every class 1..7; real atoms of class 0; a 32-row block of four classes or
    more."""
    cls = nd["deg_class"].numpy()
    real = pb_enc.row_mol.numpy() >= 0
    assert set(np.unique(cls[real])) == set(range(8)), np.unique(cls[real])
    assert (cls[~real] == 0).all()
    per_block = [len(set(cls[a:a + 32][real[a:a + 32]])) for a in range(0, pb_enc.n_rows, 32)]
    assert max(per_block) >= 4, per_block


# The two 13-pair worlds in the form of table_harness.world: "hand" is the ten table molecules under the harness's pairs, "single"
# nine molecules, the single-atom one among them, under the pairs of the harness's synthetic world.
WORLDS = {"hand": (list(range(10)), [0, 1, 2, 8, 3, 3, 9, 1, 7, 5, 5, 4, 6], [1, 0, 8, 8, 4, 3, 1, 9, 0, 5, 2, 7, 6]),
          "single": ([SINGLE, 8, 9, 0, 2, 3, 4, 6, 1], [0, 1, 2, 0, 3, 3, 8, 1, 0, 5, 5, 2, 6], [1, 0, 0, 0, 4, 3, 1, 8, 7, 5, 2, 2, 6])}


def world_molecules(which):
    """(the world's molecules, its two sides as indices into them)."""
    mols, I1, I2 = WORLDS[which]
    st = store()
    return [st[k] for k in mols], np.array(I1), np.array(I2)


def world(which, device):
    """table_harness.world's namespace for one of the two worlds, the store on ``device``."""
    if ("world", which) not in _CACHE:
        from bmp import packed
        mols, I1, I2 = world_molecules(which)
        ms = packed.MolStore(mols)
        _CACHE[("world", which)] = types.SimpleNamespace(which="hand" if which == "hand" else "synthetic", store=mols, ms=ms,
                                                         ds=packed.DeviceMolStore(ms, device), I1=I1, I2=I2,
                                                         counts=[m.n for m in mols])
    return _CACHE[("world", which)]
