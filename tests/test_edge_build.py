"""CPU checks of the edge-network GGNN's surface: constructor, parameter names and shapes, the snapshot round trip, both import
paths, what the option refuses (layout plan, encoder layout, dedup), the pair predictor's wiring, the C ABI's new symbols, and zero
scratch in the fused kernels."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import edge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enc(**kw):
    from bmp.ggnn import GGNN
    return GGNN(message_function='edge_network', **kw)


def test_constructor_and_refusals():
    from bmp.ggnn import EdgeNetwork, GGNN
    e = _enc(out_dim=8)
    assert (e.hidden_dim, e.n_layers, e.message_function, e.edge_hidden_dim, e.weight_tying) == (16, 4, 'edge_network', 16, True)
    assert len(e.message_layers) == 1 and type(e.message_layers[0]) is EdgeNetwork
    assert len(_enc(out_dim=8, n_layers=3, weight_tying=False).message_layers) == 3
    assert e.plannable() is False and GGNN(out_dim=8, hidden_dim=64).plannable() is True
    assert GGNN(out_dim=8).message_function == 'matrix_multiply'
    with pytest.raises(ValueError):
        GGNN(out_dim=8, message_function='edge_net')                     # models/ggnn.py:250
    with pytest.raises(ValueError):
        _enc(out_dim=8, hidden_dim=12)
    with pytest.raises(NotImplementedError):
        _enc(out_dim=8, readout_function='set2vec')
    for agg in ('concat', 'max-pool', 'attn'):
        assert _enc(out_dim=8, layer_aggregator=agg, n_layers=3).plannable() is False


def test_parameter_names_and_shapes():
    from bmp.snapshot import param_dict
    for tying, concat in ((True, False), (True, True), (False, False), (False, True)):
        enc = _enc(out_dim=12, hidden_dim=24, n_layers=3, concat_hidden=concat, weight_tying=tying, edge_hidden_dim=10)
        want = R.make_params(0, 24, 12, 3, tying, concat_hidden=concat, edge_hidden=10)
        got = param_dict(enc)
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), k
    enc = _enc(out_dim=8, weight_tying=False, n_layers=2)
    names = dict(enc.named_parameters())
    assert {"embed.W", "message_layers.1.output_layer.W", "message_layers.1.output_layer.b", "message_layers.0.hidden_layers.0.W",
            "message_layers.1.hidden_layers.0.b", "update_layer.W_r.W", "i_layers.0.W", "j_layers.0.b"} <= set(names)
    assert tuple(names["message_layers.0.output_layer.W"].shape) == (256, 4)
    assert not any("bias_add_layer" in n for n in names)                 # the reference never gives it a shape
    # built and never called: no gradient, so an optimizer with gradient hooks leaves them alone (as Chainer's does)
    assert all(p.requires_grad != ("hidden_layers" in n) for n, p in names.items())


def test_kernel_weight_layouts():
    """WT[e d + q, p] = output_layer.W[p d + q, e] and BT[q, p] = output_layer.b[p d + q], differentiable views of the parameters."""
    net = _enc(out_dim=8, hidden_dim=8).message_layers[0]
    with torch.no_grad():
        net.output_layer.b.copy_(torch.randn(64))
    WT, BT = net.kernel_weights()
    assert tuple(WT.shape) == (32, 8) and tuple(BT.shape) == (8, 8) and WT.requires_grad and BT.requires_grad
    for e, q, p in ((0, 0, 0), (3, 5, 2), (1, 7, 6)):
        assert WT[e * 8 + q, p] == net.output_layer.W[p * 8 + q, e] and BT[q, p] == net.output_layer.b[p * 8 + q]


def test_snapshot_round_trip(tmp_path):
    from bmp.snapshot import load_param_dict, param_dict
    mk = lambda: _enc(out_dim=8, hidden_dim=16, n_layers=3, concat_hidden=True, weight_tying=False)
    p = R.make_params(3, 16, 8, 3, False, concat_hidden=True)
    enc = mk()
    load_param_dict(enc, p)
    back = param_dict(enc)
    for k, v in p.items():
        assert torch.equal(back[k], v.float()), k
    path = os.path.join(tmp_path, "enc.npz")
    np.savez(path, **{k: v.numpy() for k, v in back.items()})
    enc2 = mk()
    with np.load(path) as z:
        load_param_dict(enc2, {k: z[k] for k in z.files})
    for k, v in param_dict(enc2).items():
        assert torch.equal(v, back[k]), k


def test_both_import_paths():
    from models.ggnn import GGNN as A
    from models.ggnn_att import GGNN as B
    import bmp.ggnn as M
    assert A is M.GGNN and B is M.GGNN
    assert type(A(out_dim=8, message_function='edge_network').message_layers[0]) is M.EdgeNetwork


def test_encoder_layout_and_dedup_are_refused():
    from bmp import packed, synth
    from bmp.ggnn import EDGE_NETWORK_LAYOUT_REASON
    from bmp.predictor import build_pair_predictor
    from bmp.trainer import PairBatches
    store = synth.make_store(6, seed=2, n_lo=2, n_hi=9, n_mean=5)
    pb = packed.pack_from_store(packed.MolStore(store), [np.arange(3), np.arange(3, 6)], device="cpu")
    with pytest.raises(NotImplementedError, match="padded atom count"):
        _enc(out_dim=8).encode_rows(pb)
    assert "dedup" in EDGE_NETWORK_LAYOUT_REASON and "encoder layout" in EDGE_NETWORK_LAYOUT_REASON
    model = build_pair_predictor(hidden_dim=16, out_dim=8, n_layers=2, attn=None, encoder="ggnn-edge")
    idx, lab = np.arange(3), np.zeros((3, 1), np.int32)
    for kw in (dict(layout="encoder"), dict(layout="encoder", dedup=True), dict(layout="static")):
        with pytest.raises(NotImplementedError):
            PairBatches(None, idx, idx, lab, 2, **kw).check_encoder(model)
    PairBatches(None, idx, idx, lab, 2).check_encoder(model)                                         # the per-instance form
    PairBatches(None, idx, idx, lab, 2, layout="encoder", dedup=True).check_encoder(build_pair_predictor(hidden_dim=16, out_dim=8, attn=None))


def test_pair_predictor_builds_with_the_encoder():
    from bmp.ggnn import GGNN
    from bmp.predictor import build_pair_predictor
    m = build_pair_predictor(hidden_dim=24, out_dim=16, n_layers=3, attn=None, encoder="ggnn-edge")
    enc = m.graph_conv
    assert type(enc) is GGNN and enc.message_function == 'edge_network' and enc.weight_tying and enc.n_layers == 3
    assert m.mlp.layers[0].W.shape[1] == 2 * 16
    u = build_pair_predictor(hidden_dim=24, out_dim=16, n_layers=3, attn="nie", encoder="ggnn-edge", weight_tying=False)
    assert u.graph_conv.n_message_layer == 3 and u.attn is not None and u.mlp.layers[0].W.shape[1] == 2 * 16
    with pytest.raises(ValueError):
        build_pair_predictor(encoder="ggnn-edges")


def test_new_symbols_in_header_and_ctypes_table():
    from bmp import _lib, functional as Fn
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    for name in ("bmp_ggnn_edge_step_supported", "bmp_ggnn_edge_step_tile_fwd", "bmp_ggnn_edge_step_tile_bwd"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name          # one ctypes entry per declared argument
    assert os.path.exists(os.path.join(ROOT, "gcn-bmp_amd", "csrc", "bmp_edge.hip"))
    assert Fn.EDGE_PATHS.keys() == {"fused", "composed"}
    assert callable(Fn.edge_step) and callable(Fn.edge_step_supported) and issubclass(Fn.EdgeStepFn, torch.autograd.Function)


def test_edge_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_edge.hip"), "-o", os.path.join(tmp, "edge.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 8, names             # forward and backward x first and later call x d = 64 and 128
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    # and no fewer waves per SIMD than the kernels were written for: (d = 128, d = 64) per kernel
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    floor = {"first_tile_fwd": (2, 5), "later_tile_fwd": (2, 5), "first_tile_bwd": (3, 5), "later_tile_bwd": (2, 3)}
    assert len(occ) == 8, occ
    for n, o in zip(names, occ):
        *kind, d = re.search(r"k_edge_step_(\w+?)ILi(\d+)E", n).groups()
        assert o >= floor["_".join(kind)][d == "64"], (n, o)
