"""CPU checks of the tile-table form of the d = 32 gate step and of the gated encoders' ``encode_rows`` / ``readout_rows`` pair:
the two new C entries in the header and the ctypes table, the new translation unit's kernels at the three-workgroups-per-CU
design point, the dispatch switch, the three refusals of ``encode_rows`` and the layout check of ``PairBatches``."""
import re
import tempfile

import numpy as np
import pytest

from table_build import CSRC, check_table_entries, enc_batch, resource_usage

NEW = ("bmp_ggnn_gate_step_small_table_fwd", "bmp_ggnn_gate_step_small_table_bwd")


def test_new_entries_in_header_and_ctypes_table():
    from bmp import functional as Fn
    check_table_entries(NEW, whole_of=lambda name: name.replace("_table", ""))
    assert Fn.GATE_TABLE_DEFAULT.keys() == {"fuse", "gate"} and all(type(v) is bool for v in Fn.GATE_TABLE_DEFAULT.values())
    assert Fn.GATE_PATHS.keys() == {"fused", "composed"}


def test_table_kernels_fit_three_workgroups_per_cu():
    """The table instances are the six kernels of their own translation unit: no scratch, and the same LDS and occupancy budget
    as the whole-tile instances."""
    with tempfile.TemporaryDirectory() as tmp:
        names, scratch, _vgpr, _agpr, occ, lds = resource_usage("bmp_gate_small_table.hip", tmp)
    assert len(names) == len(scratch) == len(lds) == len(occ) == 6, names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    ecap = int(re.search(r"#define FZ_ECAP (\d+)", open(CSRC + "/bmp_tile.h").read()).group(1))
    dyn = (2 * 128 * 36 + 128 * 4 + 132 + 2 * ecap + 4) * 4
    assert all(s + dyn <= 160 * 1024 // 3 for s in lds), (dict(zip(names, lds)), dyn)
    assert all(o >= 3 for o in occ), dict(zip(names, occ))


def _enc(kind, **kw):
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    return (FuseGGNN if kind == "fuse" else GateGGNN)(out_dim=8, hidden_dim=32, n_layers=2, **kw)


def test_encoders_have_the_rows_pair_and_refuse_with_their_reasons():
    from bmp import ggnn_gate as G
    eb = enc_batch()
    for kind in ("fuse", "gate"):
        enc = _enc(kind)
        assert callable(enc.encode_rows) and callable(enc.readout_rows)
        assert enc.encoder_layout_reason is None
        with pytest.raises(NotImplementedError) as e:
            _enc(kind, concat_hidden=True).eval().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + G.CONCAT_LAYOUT_REASON and "concat_hidden" in str(e.value)
        with pytest.raises(NotImplementedError) as e:
            _enc(kind, dropout_rate=0.1).train().encode_rows(eb.pb_enc)
        want = G.FUSE_TRAIN_LAYOUT_REASON if kind == "fuse" else G.DROPOUT_LAYOUT_REASON
        assert str(e.value) == "encode_rows: " + want
    with pytest.raises(NotImplementedError) as e:
        _enc("fuse").train().encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + G.FUSE_TRAIN_LAYOUT_REASON and "dropout on r * h" in str(e.value)
    assert "dropout_rate" in G.DROPOUT_LAYOUT_REASON
    # what is allowed: the gate kind in training, both kinds in evaluation mode (dropout_rate is then the identity)
    assert _enc("gate").train().rows_reason() is None
    assert _enc("fuse").eval().rows_reason() is None and _enc("fuse", dropout_rate=0.1).eval().rows_reason() is None
    assert _enc("gate", dropout_rate=0.1).eval().rows_reason() is None


def test_check_encoder_refuses_the_encoder_layout_for_concat_hidden():
    from bmp import ggnn_gate as G
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.trainer import PairBatches
    z = np.zeros(4, dtype=np.int64)
    mk = lambda layout, dedup=False: PairBatches(None, z, z, z, 2, layout=layout, dedup=dedup)
    for kind in ("fuse", "gate"):
        model = GraphConvPredictorForPair(_enc(kind, concat_hidden=True), None, build_link_predictor("hole", 16, 1))
        for dedup in (False, True):
            with pytest.raises(NotImplementedError) as e:
                mk("encoder", dedup).check_encoder(model)
            assert str(e.value) == f"PairBatches(layout='encoder', dedup={dedup}): " + G.CONCAT_LAYOUT_REASON
        mk("instance").check_encoder(model)
        mk("static").check_encoder(model)            # forward(pb), not encode_rows: concat_hidden runs there
        plain = GraphConvPredictorForPair(_enc(kind), None, build_link_predictor("hole", 8, 1))
        for layout in ("instance", "encoder", "static"):
            mk(layout).check_encoder(plain)
        mk("encoder", True).check_encoder(plain)
