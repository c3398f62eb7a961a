"""CPU checks of the tile-table form of the self-loop GGNN step and of the ``encode_rows`` / ``readout_rows`` pair of the two
encoders of bmp/ggnn_dev.py: the new C entries in the header and the ctypes table, the new translation unit's kernels without
scratch, the dispatch switch, the tables of the GPU tests, the refusals of ``encode_rows`` and the layout check of ``PairBatches``."""
import tempfile

import numpy as np
import pytest

from enc_tables import TABLES, _hand_store
from table_build import check_table_entries, enc_batch, lib, resource_usage

NEW = ("bmp_ggnn_loop_step_table_fwd", "bmp_ggnn_loop_step_table_bwd")


def test_new_entries_in_header_and_ctypes_table():
    from bmp import functional as Fn
    check_table_entries(NEW)
    assert Fn.LOOP_TABLE_DEFAULT.keys() == {64, 128} and all(type(v) is bool for v in Fn.LOOP_TABLE_DEFAULT.values())
    assert Fn.LOOP_PATHS.keys() == {"fused", "composed"}
    L = lib().lib()
    assert [bool(L.bmp_ggnn_loop_step_table_supported(d)) for d in (16, 32, 64, 128, 256)] == [False, False, True, True, False]


def test_table_kernels_do_not_spill():
    """The table instances are the eight kernels of their own translation unit: 2 directions x first / later x 2 widths, none
    with scratch, each within the 512 registers a SIMD's lane has for the two waves of a 512-thread workgroup."""
    with tempfile.TemporaryDirectory() as tmp:
        names, scratch, vgpr, agpr, occ, _lds = resource_usage("bmp_loop_table.hip", tmp, "--cuda-device-only")
    assert len(names) == len(scratch) == len(vgpr) == len(agpr) == len(occ) == 8, names
    assert sum("table_fwd" in n for n in names) == 4 and sum("table_bwd" in n for n in names) == 4, names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert all(v + a <= 256 for v, a in zip(vgpr, agpr)), dict(zip(names, zip(vgpr, agpr)))
    assert all(o >= 2 for o in occ), dict(zip(names, occ))       # the 8 waves of a workgroup: two per SIMD


def test_the_three_tables_have_their_properties():
    """What the GPU tests rely on, from the host plan: "own" has every block count and the pad row on row 31 of a one-block tile,
    on row 32 and on row 127 of a full tile, plus two molecule-free tiles; "shared" has tiles of two or three molecules and a
    molecule from tile row 95 across the block boundary at 96; "seven" has seven molecules in one two-block tile and two empty
    one-block tiles.  Every table is under 800 rows."""
    from bmp import enclayout, packed
    ms = packed.MolStore(_hand_store())
    for name, (inst, n_cu) in TABLES.items():
        pl = enclayout.plan_enc_numpy(ms.n_atoms, ms.nedges, np.asarray(inst), False, n_cu)
        nb, r0 = pl["mt_nblk"].tolist(), pl["mt_row0"]
        n, row0, tile, pad = pl["n"], pl["row0"], pl["tile"], pl["enc_pad"]
        per_tile = np.bincount(tile, minlength=len(nb))
        off = row0 - r0[tile]
        assert int(r0[-1]) + 32 * nb[-1] < 800 and min(nb) >= 1 and max(nb) <= 4
        assert (off >= 0).all() and (off + n <= 32 * np.asarray(nb)[tile]).all()      # no molecule straddles its tile
        if name == "own":
            assert nb == [4, 4, 3, 3, 2, 2, 2, 1, 1, 1, 1]
            at = lambda k: int(pad[list(n).index(k)] - r0[tile[list(n).index(k)]])
            assert at(31) == 31 and nb[tile[list(n).index(31)]] == 1
            assert at(32) == 32 and nb[tile[list(n).index(32)]] == 2
            assert at(127) == 127 and nb[tile[list(n).index(127)]] == 4
            assert per_tile.tolist()[-2:] == [0, 0] and (per_tile[:-2] >= 1).all()
        elif name == "shared":
            assert sorted(per_tile[per_tile > 0].tolist()) == [1, 2, 2, 2, 3]
            u = list(n).index(32)
            assert off[u] == 95 and off[u] + n[u] > 96
        else:
            assert nb == [2, 1, 1] and per_tile.tolist() == [7, 0, 0]


def _enc(kind, **kw):
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    return (DevGGNN if kind == "dev" else SelfLoopGGNN)(out_dim=8, hidden_dim=64, n_layers=2, **kw)


def test_encoders_have_the_rows_pair_and_refuse_with_their_reasons():
    from bmp import ggnn_gate as G
    eb = enc_batch()
    for kind in ("dev", "loop"):
        enc = _enc(kind)
        assert callable(enc.encode_rows) and callable(enc.readout_rows)
        assert enc.encoder_layout_reason is None and enc.plannable() is False
        cc = _enc(kind, concat_hidden=True)
        assert cc.encoder_layout_reason == G.CONCAT_LAYOUT_REASON and cc.plannable() is False
        with pytest.raises(NotImplementedError) as e:
            cc.eval().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + G.CONCAT_LAYOUT_REASON and "concat_hidden" in str(e.value)
        with pytest.raises(NotImplementedError) as e:
            _enc(kind, dropout_rate=0.1).train().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + G.DROPOUT_LAYOUT_REASON and "dropout_rate" in str(e.value)
        assert _enc(kind).train().rows_reason() is None and _enc(kind, dropout_rate=0.1).eval().rows_reason() is None


def test_dev_keeps_only_the_last_step_after_encode_rows():
    """After ``encode_rows`` and the predictor's hand-over only the last step's atoms exist: -1 and n_layers - 1 return them, any
    other step and get_g_list() raise instead of returning a wrong step's rows."""
    enc = _enc("dev")
    enc._rows_only = True                                # what encode_rows leaves, without running the steps
    marker = object()
    enc.set_rows_atoms(marker)
    assert enc.get_atom_array() is marker and enc.get_atom_array(-1) is marker and enc.get_atom_array(1) is marker
    for step in (0, -2, 2):
        with pytest.raises(RuntimeError, match="per-instance batch form"):
            enc.get_atom_array(step)
    with pytest.raises(RuntimeError, match="per-instance batch form"):
        enc.get_g_list()


def test_check_encoder_refuses_the_encoder_layout_for_concat_hidden():
    from bmp import ggnn_gate as G
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.trainer import PairBatches
    z = np.zeros(4, dtype=np.int64)
    mk = lambda layout, dedup=False: PairBatches(None, z, z, z, 2, layout=layout, dedup=dedup)
    for kind in ("dev", "loop"):
        model = GraphConvPredictorForPair(_enc(kind, concat_hidden=True), None, build_link_predictor("hole", 16, 1))
        for dedup in (False, True):
            with pytest.raises(NotImplementedError) as e:
                mk("encoder", dedup).check_encoder(model)
            assert str(e.value) == f"PairBatches(layout='encoder', dedup={dedup}): " + G.CONCAT_LAYOUT_REASON
        mk("instance").check_encoder(model)
        mk("static").check_encoder(model)            # forward(pb), not encode_rows: concat_hidden runs there
        plain = GraphConvPredictorForPair(_enc(kind), None, build_link_predictor("hole", 64 if kind == "dev" else 8, 1))
        for layout in ("instance", "encoder", "static"):
            mk(layout).check_encoder(plain)
        mk("encoder", True).check_encoder(plain)
