"""CPU checks of the tile-table form of the GIN layer and of the ``encode_rows`` / ``readout_rows`` pair of bmp/gin.py: the new C
entries in the header, the ctypes table and the library, the widths they serve, their argument checks (which return before any
launch: no GPU is needed), the new translation unit's kernels without scratch beside the four whole-tile kernels, the dispatch
switch, the refusals of ``rows_reason`` and the layout check of ``PairBatches``."""
import re
import tempfile

import numpy as np
import pytest

from table_build import BAD_TABLES, CSRC, P, ROOT, bad_id, check_table_entries, enc_batch, header_args, lib, resource_usage

ENTRIES = ("bmp_gin_layer_table_supported", "bmp_gin_layer_table_fwd", "bmp_gin_layer_table_bwd")


def test_header_and_ctypes_table_declare_the_entry_points():
    _l = lib()
    from bmp import functional as Fn
    header = open(ROOT + "/include/bmp.h").read()
    assert header.count("models/gin.py:89-128") >= 4           # the whole-tile block and each of the three new entries' block
    for name in ENTRIES:
        args = header_args(name)
        assert name in _l.SIGNATURES, name
        assert len(args) == len(_l.SIGNATURES[name][1]), (name, len(args), len(_l.SIGNATURES[name][1]))   # one ctypes entry per argument
    check_table_entries(ENTRIES[1:])
    kern = open(CSRC + "/bmp_kernels.h").read()
    for name in ENTRIES:
        assert re.search(r'extern "C" int %s\s*\(' % name, kern), name
    assert set(Fn.GIN_TABLE_DEFAULT) == {64, 128}
    assert all(type(v) is bool for v in Fn.GIN_TABLE_DEFAULT.values())
    assert Fn.GIN_PATHS.keys() == {"fused", "composed"} and callable(Fn.gin_table_ok)


def test_library_exports_the_entry_points_and_serves_64_and_128():
    L = lib().lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    widths = (8, 16, 24, 32, 40, 64, 128, 256)
    assert [d for d in widths if L.bmp_gin_layer_table_supported(d)] == [64, 128]
    assert all(bool(L.bmp_gin_layer_table_supported(d)) == bool(L.bmp_gin_layer_supported(d)) for d in widths)


def _fwd(L, d=64, r0=P, nb=P, rows=384, stride=0, s=P, t=P, h=P, n_tiles=3):
    return L.bmp_gin_layer_table_fwd(h, n_tiles, d, P, P, P, P, P, P, P, None, s, t, P, r0, nb, rows, stride, None)


def _bwd(L, d=64, r0=P, nb=P, rows=384, stride=0, dp1=P, n_tiles=3, **_):
    return L.bmp_gin_layer_table_bwd(P, P, None, P, n_tiles, d, P, P, P, P, P, P, dp1, P, r0, nb, rows, stride, None)


@pytest.mark.parametrize("bad", BAD_TABLES + [dict(d=32), dict(n_tiles=0)], ids=bad_id)
def test_entries_check_their_arguments_before_any_launch(bad):
    L = lib().lib()
    assert _fwd(L, **bad) < -1000
    assert _bwd(L, **bad) < -1000


def test_forward_takes_s_and_t_both_or_neither_and_aligned():
    L = lib().lib()
    assert _fwd(L, s=None) < -1000 and _fwd(L, t=None) < -1000          # a lone null
    assert _fwd(L, s=P + 4) < -1000 and _fwd(L, h=P + 8) < -1000        # 16-byte alignment, as the whole-tile entry
    assert _bwd(L, dp1=None) < -1000 and _bwd(L, dp1=P + 4) < -1000
    # the whole-tile entry keeps its contract: s and t are required there
    assert L.bmp_gin_layer_tile_fwd(P, 3, 64, P, P, P, P, P, P, P, None, None, None, P, None) < -1000


def test_table_kernels_do_not_spill_and_the_whole_tile_unit_keeps_its_four():
    """The table instances are the four kernels of their own translation unit -- 2 directions x 2 widths --, none with scratch,
    each within the 512 registers a SIMD's lane has for the two waves of a 512-thread workgroup; bmp_gin.hip still yields its
    four whole-tile kernels and no table instance."""
    with tempfile.TemporaryDirectory() as tmp:
        names, scratch, vgpr, agpr, occ, _lds = resource_usage("bmp_gin_table.hip", tmp, "--cuda-device-only")
        whole = resource_usage("bmp_gin.hip", tmp, "--cuda-device-only")
    assert len(names) == len(scratch) == len(vgpr) == len(agpr) == len(occ) == 4, names
    assert sum("k_gin_table_fwd" in n for n in names) == 2 and sum("k_gin_table_bwd" in n for n in names) == 2, names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    for n, v, a, o in zip(names, vgpr, agpr, occ):
        assert v + a <= 256 and o >= 2, (n, v, a, o)           # the 8 waves of a workgroup: two per SIMD
    assert len(whole[0]) == 4 and all("k_gin_tile_" in n for n in whole[0]) and all(s == 0 for s in whole[1]), whole[:2]


def _gin(**kw):
    from bmp.gin import GIN
    return GIN(out_dim=8, hidden_dim=64, **kw)


def test_gin_has_the_rows_entry_and_its_reasons():
    from bmp.ggnn import CONCAT_LAYOUT_REASON, DROPOUT_LAYOUT_REASON
    from bmp.gin import GIN
    for name in ("encode_rows", "readout_rows", "rows_reason"):
        assert callable(getattr(GIN, name, None)), name
    tied = _gin(n_layers=4, concat_hidden=True)                # the trainer's construction: ONE layer and one readout run
    assert tied.weight_tying and tied.n_concat == 1 and tied.dropout_ratio == 0.5
    assert tied.eval().rows_reason() is None and tied.encoder_layout_reason is None and tied.plannable() is False
    assert tied.train().rows_reason() == DROPOUT_LAYOUT_REASON and tied.encoder_layout_reason is None
    untied = _gin(n_layers=3, concat_hidden=True, weight_tying=False, dropout_ratio=0.0)
    assert untied.n_concat == 3
    for enc in (untied.eval(), untied.train()):
        assert enc.rows_reason() == CONCAT_LAYOUT_REASON and enc.encoder_layout_reason == CONCAT_LAYOUT_REASON
    assert _gin(n_layers=1, concat_hidden=True, weight_tying=False).eval().rows_reason() is None       # one layer runs
    drop = _gin(n_layers=3, weight_tying=False, dropout_ratio=0.5)
    assert drop.train().rows_reason() == DROPOUT_LAYOUT_REASON and drop.eval().rows_reason() is None
    assert drop.encoder_layout_reason is None
    plain = _gin(n_layers=3, weight_tying=False, dropout_ratio=0.0)
    assert plain.train().rows_reason() is None and plain.eval().rows_reason() is None


def test_encode_rows_refuses_with_the_reasons_before_it_touches_the_batch():
    from bmp.ggnn import CONCAT_LAYOUT_REASON, DROPOUT_LAYOUT_REASON
    eb = enc_batch()
    with pytest.raises(NotImplementedError) as e:
        _gin(n_layers=3, concat_hidden=True, weight_tying=False).eval().encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + CONCAT_LAYOUT_REASON and "concat_hidden" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        _gin(dropout_ratio=0.5).train().encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + DROPOUT_LAYOUT_REASON
    with pytest.raises(RuntimeError, match="GPU only"):       # a CPU batch: refused as in forward
        _gin().eval().encode_rows(eb.pb_enc)
    with pytest.raises(NotImplementedError, match="float atom features"):
        _gin().eval().encode_rows(np.zeros((2, 3, 16), np.float32))


def test_check_encoder_passes_every_layout_but_for_a_concat_of_several_layers():
    from bmp.ggnn import CONCAT_LAYOUT_REASON
    from bmp.predictor import build_pair_predictor
    from bmp.trainer import PairBatches
    z = np.zeros(4, dtype=np.int64)
    mk = lambda layout, dedup=False: PairBatches(None, z, z, z, 2, layout=layout, dedup=dedup)
    for attn in (None, "nie"):
        model = build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=3, attn=attn, encoder="gin")      # tied: served
        for layout in ("instance", "encoder", "static"):
            mk(layout).check_encoder(model)
        mk("encoder", True).check_encoder(model)
    model = build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=3, attn=None, encoder="gin", weight_tying=False)
    for dedup in (False, True):
        with pytest.raises(NotImplementedError) as e:
            mk("encoder", dedup).check_encoder(model)
        assert str(e.value) == f"PairBatches(layout='encoder', dedup={dedup}): " + CONCAT_LAYOUT_REASON
    mk("instance").check_encoder(model)
    mk("static").check_encoder(model)                # forward(pb), not encode_rows: concat_hidden runs there
