"""CPU checks of the jumping-knowledge GGNN encoders' surface: the C ABI's new symbols, the widths the fused step serves, the
resource usage of csrc/bmp_jk.hip's kernels, the four import aliases with the reference's parameter names and shapes, the
constructor quirks, the pair predictor's wiring and what an 'attn' encoder refuses."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import jk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bmp_jk_step_supported", "bmp_jk_step_tile_fwd", "bmp_jk_step_tile_bwd", "bmp_jk_agg_ws_floats", "bmp_jk_agg_fwd",
           "bmp_jk_agg_bwd")


def test_new_symbols_in_header_ctypes_table_and_library():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib, functional as Fn
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name          # one ctypes entry per declared argument
    assert os.path.exists(os.path.join(ROOT, "gcn-bmp_amd", "csrc", "bmp_jk.hip"))
    assert Fn.JK_PATHS.keys() == {"fused", "composed"}
    assert callable(Fn.jk_step) and issubclass(Fn.JKStepFn, torch.autograd.Function) and issubclass(Fn.JKAggFn, torch.autograd.Function)
    assert set(Fn.JK_STEP_DEFAULT) == {(k, d) for k in ("jknet", "jk_gru") for d in (64, 128)}
    assert Fn.JK_AGG_MODE == {"mean": 0, "attn": 1}


def test_step_supported_widths():
    import __graft_entry__ as g
    g.build()
    from bmp import functional as Fn
    assert [d for d in (8, 16, 24, 32, 40, 64, 128, 256) if Fn.jk_step_supported(d)] == [64, 128]
    from bmp import _lib
    assert _lib.lib().bmp_jk_agg_ws_floats(3, 2) >= 3 * 2 * 2 and _lib.lib().bmp_jk_agg_ws_floats(0, 2) == 0


def test_kernels_have_no_scratch_and_fit_the_lds():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_jk.hip"), "-o", os.path.join(tmp, "jk.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # the step: forward and backward x Nu = d and 2d x d = 64 and 128;  the aggregators: the per-tile inner products (forward
    # and backward) and the backward for T = 1..8 each in two forms, the combine for T = 1..8, the fold and the fill
    step = [n for n in names if "k_jk_step" in n]
    assert len(step) == 8 and len(names) == len(scratch) == len(lds) == 8 + 16 + 16 + 8 + 2, names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    # static LDS plus, for the step kernels, the two [128][d + 4] tiles they are launched with: within the 160 KB of a CU
    for n, b in zip(names, lds):
        dyn = 0
        if "k_jk_step" in n:
            d = int(re.search(r"ILi(\d+)E", n).group(1))
            assert d in (64, 128)
            dyn = 2 * 128 * (d + 4) * 4
        assert b + dyn <= 160 * 1024, (n, b, dyn)
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    for n, o in zip(names, occ):       # eight waves per workgroup on four SIMDs: two per SIMD at least, or no workgroup fits
        if "k_jk_step" in n:
            assert o >= 2, (n, o)


def _names(kind, **kw):
    from bmp.ggnn_jk import JKGruGGNN, JKNetGGNN
    return (JKNetGGNN if kind == "jknet" else JKGruGGNN)(**kw)


@pytest.mark.parametrize("kind", ["jknet", "jk_gru"])
def test_parameter_names_and_shapes_follow_the_reference(kind):
    from bmp.snapshot import load_param_dict, param_dict
    for tying, ut, concat in ((True, True, False), (False, False, True), (True, False, False)):
        kw = dict(out_dim=12, hidden_dim=24, n_layers=3, concat_hidden=concat, weight_tying=tying, update_tying=ut)
        kw.update(dict(layer_aggr="mean") if kind == "jknet" else dict(self_loop=True))
        enc = _names(kind, **kw)
        want = R.make_params(kind, 0, 24, 12, 3, tying, ut, concat, self_loop=True)
        got = param_dict(enc)
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), k
        load_param_dict(enc, want)
        assert all(torch.equal(param_dict(enc)[k], v.float()) for k, v in want.items())
    assert "self_loop_layer.W" not in dict(_names("jk_gru", out_dim=8).named_parameters())
    if kind == "jk_gru":        # built and never read (:80 reads layer 0 when the messages are tied): no gradient
        enc = _names(kind, out_dim=8, n_layers=3, weight_tying=True, update_tying=False)
        req = {n: p.requires_grad for n, p in enc.named_parameters()}
        assert req["update_layers_0.0.W"] and not req["update_layers_0.1.W"] and not req["update_layers_0.2.b"]
        assert all(v for n, v in req.items() if not n.startswith("update_layers_0."))


def test_the_four_import_aliases():
    from models.chin_ggnn import GGNN as Chin
    from models.ggnn_chin import GGNN as Modular
    from models.ggnn_dev_jk_gru import GGNN as JkGru
    from models.ggnn_dev_jknet import GGNN as JkNet
    import bmp.ggnn as G
    import bmp.ggnn_jk as M
    import bmp.relgcn as RG
    assert JkNet is M.JKNetGGNN and JkGru is M.JKGruGGNN and Modular is RG.GGNNModular and issubclass(Chin, G.GGNN)
    assert JkNet.NUM_EDGE_TYPE == JkGru.NUM_EDGE_TYPE == Chin.NUM_EDGE_TYPE == 4
    e = JkNet(out_dim=8, layer_aggr='attn')
    assert (e.hidden_dim, e.n_layers, e.concat_hidden, e.dropout_rate, e.weight_tying, e.update_tying) == (16, 4, False, 0.0, True, True)
    assert tuple(e.update_layer[0].W.shape) == (16, 32) and len(e.update_layer) == 1 and e.plannable() is False
    u = JkGru(out_dim=8, hidden_dim=24, n_layers=2, weight_tying=False, update_tying=False, self_loop=True)
    assert tuple(u.update_layers_0[1].W.shape) == (48, 48) and tuple(u.update_layer.W_r.W.shape) == (24, 48)
    assert tuple(u.self_loop_layer.W.shape) == (24, 24) and len(u.message_layers) == 2 and u.plannable() is False
    c = Chin(out_dim=8, hidden_dim=24, n_layers=3, n_atom_types=50, concat_hidden=True, dropout_rate=0.1, weight_tying=False)
    names = dict(c.named_parameters())
    assert tuple(names["embed.W"].shape) == (50, 24) and len(c.message_layers) == 3 and len(c.i_layers) == 3
    assert c.message_function == 'matrix_multiply' and c.layer_aggregator is None and c.dropout_rate == 0.1
    with pytest.raises(TypeError):
        Chin(out_dim=8, layer_aggregator='attn')                         # the shorter constructor has no such argument
    with pytest.raises(NotImplementedError):
        Chin(out_dim=8, batch_normalization=True)
    m = Modular(out_dim=8, hidden_dim=16, n_layers=2, weight_tying=False, num_edge_type=4)
    assert len(m.update_layers) == 2


def test_constructor_quirks():
    from bmp.ggnn_jk import JKGruGGNN, JKNetGGNN
    with pytest.raises(ValueError, match="select_aggr"):
        JKNetGGNN(out_dim=8)                                             # layer_aggr=None: the reference's constructor asserts
    with pytest.raises(ValueError, match="No such layer aggr"):
        JKNetGGNN(out_dim=8, layer_aggr='max-pool')
    for agg in ('gru', 'bigru'):
        with pytest.raises(NotImplementedError):
            JKNetGGNN(out_dim=8, layer_aggr=agg)
    with pytest.raises(ValueError, match="n_layers == 1"):
        JKNetGGNN(out_dim=8, layer_aggr='concat', n_layers=2)
    JKNetGGNN(out_dim=8, layer_aggr='concat', n_layers=1)
    JKNetGGNN(out_dim=8, layer_aggr='concat', n_layers=3, concat_hidden=True)      # the aggregator is never called there
    with pytest.raises(ValueError):
        JKNetGGNN(out_dim=8, layer_aggr='attn', n_layers=9)
    with pytest.raises(ValueError, match="ggnn_dev_jk_gru.py:80"):
        JKGruGGNN(out_dim=8, weight_tying=False, update_tying=True, n_layers=2)
    JKGruGGNN(out_dim=8, weight_tying=False, update_tying=True, n_layers=1)
    for cls, kw in ((JKNetGGNN, dict(layer_aggr='mean')), (JKGruGGNN, {})):
        with pytest.raises(NotImplementedError):
            cls(out_dim=8, batch_normalization=True, **kw)
        with pytest.raises(ValueError):
            cls(out_dim=8, hidden_dim=12, **kw)
        enc = cls(out_dim=8, **kw)
        with pytest.raises(NotImplementedError, match="float atom features"):
            enc(np.zeros((2, 3, 16), np.float32), np.zeros((2, 4, 3, 3), np.float32))
        with pytest.raises(AssertionError):
            enc.get_atom_array()


def test_pair_predictor_builds_with_the_encoders():
    from bmp.ggnn_jk import JKGruGGNN, JKNetGGNN
    from bmp.predictor import build_pair_predictor
    m = build_pair_predictor(hidden_dim=24, out_dim=16, n_layers=3, attn=None, encoder="ggnn-jknet")
    assert type(m.graph_conv) is JKNetGGNN and m.graph_conv.layer_aggr == 'attn' and m.mlp.layers[0].W.shape[1] == 2 * 16
    assert build_pair_predictor(hidden_dim=24, out_dim=16, attn=None, encoder="ggnn-jknet", layer_aggr="max").graph_conv.layer_aggr == 'max'
    g = build_pair_predictor(hidden_dim=24, out_dim=16, n_layers=3, attn="nie", encoder="ggnn-jk-gru", weight_tying=False)
    assert type(g.graph_conv) is JKGruGGNN and len(g.graph_conv.update_layers_0) == 3 and g.attn is not None
    with pytest.raises(ValueError):
        build_pair_predictor(encoder="ggnn-jk")


def test_attn_encoder_refuses_encoder_layout_dedup_and_the_recorded_step():
    from bmp import packed, synth
    from bmp.ggnn_jk import JK_ATTN_LAYOUT_REASON, JKNetGGNN
    from bmp.predictor import build_pair_predictor
    from bmp.trainer import PairBatches
    assert all(w in JK_ATTN_LAYOUT_REASON for w in ("dedup", "encoder layout", "layout plan", "recorded step", "batch side"))
    store = synth.make_store(6, seed=2, n_lo=2, n_hi=9, n_mean=5)
    pb = packed.pack_from_store(packed.MolStore(store), [np.arange(3), np.arange(3, 6)], device="cpu")
    with pytest.raises(NotImplementedError, match="batch side"):
        JKNetGGNN(out_dim=8, layer_aggr='attn').encode_rows(pb)
    model = build_pair_predictor(hidden_dim=16, out_dim=8, n_layers=2, attn=None, encoder="ggnn-jknet")
    idx, lab = np.arange(3), np.zeros((3, 1), np.int32)
    for kw in (dict(layout="encoder"), dict(layout="encoder", dedup=True), dict(layout="static")):
        with pytest.raises(NotImplementedError, match="batch side"):
            PairBatches(None, idx, idx, lab, 2, **kw).check_encoder(model)
    PairBatches(None, idx, idx, lab, 2).check_encoder(model)                                         # the per-instance form
    assert model.graph_conv.plannable() is False
    assert JKNetGGNN(out_dim=8, layer_aggr='mean').layout_reason is None
