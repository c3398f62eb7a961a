"""CPU checks of the tile-table form of the jumping-knowledge step, of the 'mean' aggregator on a row count and of the
``encode_rows`` / ``readout_rows`` pair of the two encoders of bmp/ggnn_jk.py: the new C entries in the header, the ctypes table
and the library, the widths they serve, their argument checks (which return before any launch: no GPU is needed), the new
translation unit's kernels without scratch, the dispatch switch, the refusals of ``encode_rows`` and the layout check of
``PairBatches``."""
import ctypes
import re
import tempfile

import numpy as np
import pytest

from table_build import BAD_TABLES, CSRC, P, bad_id, check_table_entries, enc_batch, header_args, lib, resource_usage

STEP = ("bmp_jk_step_table_supported", "bmp_jk_step_table_fwd", "bmp_jk_step_table_bwd")
MEAN = ("bmp_jk_mean_fwd", "bmp_jk_mean_bwd")


def test_header_and_ctypes_table_declare_the_entry_points():
    _l = lib()
    from bmp import functional as Fn
    for name in STEP + MEAN:
        args = header_args(name)
        assert name in _l.SIGNATURES, name
        assert len(args) == len(_l.SIGNATURES[name][1]), (name, len(args), len(_l.SIGNATURES[name][1]))   # one ctypes entry per argument
    check_table_entries(STEP[1:])
    kern = open(CSRC + "/bmp_kernels.h").read()
    for name in STEP + MEAN:
        assert re.search(r'extern "C" int %s\s*\(' % name, kern), name
    assert set(Fn.JK_TABLE_DEFAULT) == {(k, d) for k in ("jknet", "jk_gru") for d in (64, 128)}
    assert all(type(v) is bool for v in Fn.JK_TABLE_DEFAULT.values())
    assert Fn.JK_PATHS.keys() == {"fused", "composed"} and callable(Fn.jk_table_ok)


def test_library_exports_the_entry_points_and_serves_64_and_128():
    L = lib().lib()
    for name in STEP + MEAN:
        assert hasattr(L, name), name
    assert [d for d in (8, 16, 24, 32, 40, 64, 128, 256) if L.bmp_jk_step_table_supported(d)] == [64, 128]


def _step_fwd(L, ng=1, d=64, r0=P, nb=P, rows=384, stride=0):
    return L.bmp_jk_step_table_fwd(ng, P, 3, d, P, P, P, P, P, None, None, P, P, P, P, r0, nb, rows, stride, None)


def _step_bwd(L, ng=1, d=64, r0=P, nb=P, rows=384, stride=0):
    return L.bmp_jk_step_table_bwd(ng, P, P, 3, d, P, P, P, P, None, P, P, P, r0, nb, rows, stride, None)


@pytest.mark.parametrize("bad", BAD_TABLES + [dict(ng=3), dict(d=32)], ids=bad_id)
def test_step_entries_check_their_arguments_before_any_launch(bad):
    L = lib().lib()
    assert _step_fwd(L, **bad) < -1000
    assert _step_bwd(L, **bad) < -1000


def test_mean_entries_check_their_arguments_before_any_launch():
    L = lib().lib()
    nine = (ctypes.c_void_p * 9)(*([P] * 9))
    assert L.bmp_jk_mean_fwd(nine, 9, 32, 64, P, None) < -1000             # T = 9
    assert L.bmp_jk_mean_bwd(P, 9, 32, 64, nine, None) < -1000
    assert L.bmp_jk_mean_fwd(nine, 0, 32, 64, P, None) < -1000
    assert L.bmp_jk_mean_fwd(nine, 3, 0, 64, P, None) < -1000              # no rows
    assert L.bmp_jk_mean_bwd(P, 3, 32, 62, nine, None) < -1000             # a width that is no multiple of 4
    assert L.bmp_jk_mean_fwd(nine, 3, 32, 64, P + 4, None) < -1000         # y 4 bytes off
    hole = (ctypes.c_void_p * 3)(P, None, P)
    assert L.bmp_jk_mean_fwd(hole, 3, 32, 64, P, None) < -1000 and L.bmp_jk_mean_bwd(P, 3, 32, 64, hole, None) < -1000


def test_table_kernels_do_not_spill():
    """The table instances are the eight step kernels of their own translation unit: 2 directions x Nu = d and 2d x 2 widths,
    none with scratch, each within the 512 registers a SIMD's lane has for the two waves of a 512-thread workgroup; beside
    them the sixteen row-count 'mean' kernels (T = 1..8, two directions)."""
    with tempfile.TemporaryDirectory() as tmp:
        names, scratch, vgpr, agpr, occ, _lds = resource_usage("bmp_jk_table.hip", tmp, "--cuda-device-only")
    assert len(names) == len(scratch) == len(vgpr) == len(agpr) == len(occ) == 8 + 16, names
    assert sum("table_fwd" in n for n in names) == 4 and sum("table_bwd" in n for n in names) == 4, names
    assert sum("k_jk_mean" in n for n in names) == 16, names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    for n, v, a, o in zip(names, vgpr, agpr, occ):
        if "k_jk_step" in n:
            assert v + a <= 256 and o >= 2, (n, v, a, o)       # the 8 waves of a workgroup: two per SIMD


def _jknet(aggr, **kw):
    from bmp.ggnn_jk import JKNetGGNN
    return JKNetGGNN(out_dim=8, hidden_dim=64, n_layers=2, layer_aggr=aggr, **kw)


def _jkgru(**kw):
    from bmp.ggnn_jk import JKGruGGNN
    return JKGruGGNN(out_dim=8, hidden_dim=64, n_layers=2, **kw)


def test_encoders_have_the_rows_pair_and_refuse_with_their_reasons():
    from bmp import ggnn_gate as G
    from bmp.ggnn import _StepEncoder
    from bmp.ggnn_jk import JK_ATTN_LAYOUT_REASON, JKGruGGNN, JKNetGGNN
    eb = enc_batch()
    for make in (lambda **kw: _jknet("max", **kw), lambda **kw: _jknet("mean", **kw), _jkgru, lambda **kw: _jkgru(self_loop=True, **kw)):
        enc = make()
        assert enc.eval().rows_reason() is None and enc.train().rows_reason() is None
        assert enc.encoder_layout_reason is None and enc.layout_reason is None and enc.plannable() is False
        assert type(enc).readout_rows is _StepEncoder.readout_rows
        cc = make(concat_hidden=True)
        assert cc.encoder_layout_reason == G.CONCAT_LAYOUT_REASON and cc.rows_reason() == G.CONCAT_LAYOUT_REASON
        with pytest.raises(NotImplementedError) as e:
            cc.eval().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + G.CONCAT_LAYOUT_REASON and "concat_hidden" in str(e.value)
        dr = make(dropout_rate=0.25)
        assert dr.train().rows_reason() == G.DROPOUT_LAYOUT_REASON and dr.eval().rows_reason() is None
        with pytest.raises(NotImplementedError) as e:
            dr.train().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + G.DROPOUT_LAYOUT_REASON and "dropout_rate" in str(e.value)
    at = _jknet("attn")
    assert at.rows_reason() == JK_ATTN_LAYOUT_REASON and at.layout_reason == JK_ATTN_LAYOUT_REASON
    with pytest.raises(NotImplementedError) as e:
        at.encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + JK_ATTN_LAYOUT_REASON
    assert JKNetGGNN(out_dim=8, hidden_dim=64, n_layers=1, layer_aggr="concat").rows_reason() is None
    assert JKNetGGNN.encode_rows is JKGruGGNN.encode_rows


def test_check_encoder_passes_every_layout_but_for_concat_hidden_and_attn():
    from bmp import ggnn_gate as G
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor, build_pair_predictor
    from bmp.trainer import PairBatches
    z = np.zeros(4, dtype=np.int64)
    mk = lambda layout, dedup=False: PairBatches(None, z, z, z, 2, layout=layout, dedup=dedup)
    models = [build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=2, attn=None, encoder="ggnn-jk-gru"),
              build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=2, attn="nie", encoder="ggnn-jknet", layer_aggr="mean"),
              build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=2, attn=None, encoder="ggnn-jknet", layer_aggr="max")]
    for model in models:
        for layout in ("instance", "encoder", "static"):
            mk(layout).check_encoder(model)
        mk("encoder", True).check_encoder(model)
    for enc in (_jkgru(concat_hidden=True), _jknet("mean", concat_hidden=True)):
        model = GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1))
        for dedup in (False, True):
            with pytest.raises(NotImplementedError) as e:
                mk("encoder", dedup).check_encoder(model)
            assert str(e.value) == f"PairBatches(layout='encoder', dedup={dedup}): " + G.CONCAT_LAYOUT_REASON
        mk("instance").check_encoder(model)
        mk("static").check_encoder(model)            # forward(pb), not encode_rows: concat_hidden runs there
