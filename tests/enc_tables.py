"""The hand-made molecule store and the three tile tables of the encoder-layout tests (tests/table_harness.py hands them to
the GPU tests of the table families; their properties: tests/test_ggdev_enc_build.py).  No GPU and no GPU helper is imported here.

The store has the atom counts 31, 32, 33, 63, 64, 95, 96, 127, 2, 5: with one tile per molecule (n_cu = 256) the pad row falls on
the last row of a one-block tile, on the first row of a second block and on row 127 of a full tile; with n_cu = 2 tiles are shared
and a molecule crosses a 32-row block boundary; with n_cu = 1 seven small molecules share one two-block tile."""
import numpy as np

COUNTS = [31, 32, 33, 63, 64, 95, 96, 127, 2, 5]
TABLES = {"own": (list(range(10)), 256), "shared": (list(range(10)), 2), "seven": ([8, 9, 8, 9, 0, 8, 9], 1)}      # (instances, n_cu)


def _hand_store():
    """Chains whose bonds cycle through the four types, closed into a ring where there are atoms enough (the plan reads the atom
    and bond counts only)."""
    from bmp import synth
    rs = np.random.RandomState(77)
    mols = []
    for n in COUNTS:
        atoms = synth._ATOM_Z[rs.choice(len(synth._ATOM_Z), size=n, p=synth._ATOM_P)].astype(np.int32)
        bonds = [(i, i + 1, (i + n) % 4) for i in range(n - 1)]
        if n > 4:
            bonds += [(0, n - 1, 3), (1, n - 2, 1)]
        mols.append(synth.Molecule(atoms, np.asarray(bonds, dtype=np.int32).reshape(-1, 3)))
    return mols
