"""CPU checks of the GIN encoder's surface: constructor, parameter names and shapes, the snapshot round trip, the pair
predictor's wiring, the reference's import paths, the C ABI's new symbols, and zero scratch in the fused kernels."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import gin_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_parameter_names_and_shapes():
    from bmp.gin import GIN, GINUpdate
    from bmp.snapshot import param_dict
    u = GINUpdate()
    assert u.hidden_dim == 16 and u.dropout_ratio == 0.5 and tuple(u.linear_g1.W.shape) == (16, 16)
    for tying, concat, n_msg, n_ro in ((True, False, 1, 1), (True, True, 1, 4), (False, False, 4, 1), (False, True, 4, 4)):
        enc = GIN(out_dim=12, hidden_dim=24, n_layers=4, concat_hidden=concat, weight_tying=tying)
        assert (enc.out_dim, enc.hidden_dim, enc.n_layers, enc.n_message_layers) == (12, 24, 4, n_msg)
        assert len(enc.update_layers) == n_msg and len(enc.readout_layers) == n_ro
        want = GR.make_gin_params(0, 24, 12, 4, tying, concat_hidden=concat)
        got = param_dict(enc)
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), k
    names = [n for n, _ in GIN(out_dim=8, weight_tying=False, n_layers=2).named_parameters()]
    assert "embed.W" in names and "update_layers.1.linear_g2.b" in names and "readout_layers.0.j_layer.W" in names
    d = GIN(out_dim=8)
    assert (d.hidden_dim, d.n_layers, d.dropout_ratio, d.concat_hidden, d.weight_tying) == (16, 4, 0.5, False, True)
    with pytest.raises(ValueError):
        GIN(out_dim=8, hidden_dim=12)


def test_snapshot_round_trip(tmp_path):
    from bmp.gin import GIN
    from bmp.snapshot import load_param_dict, param_dict
    p = GR.make_gin_params(3, 16, 8, 3, False, concat_hidden=True)
    enc = GIN(out_dim=8, hidden_dim=16, n_layers=3, concat_hidden=True, weight_tying=False)
    load_param_dict(enc, p)
    back = param_dict(enc)
    for k, v in p.items():
        assert torch.equal(back[k], v.float()), k
    path = os.path.join(tmp_path, "gin.npz")
    np.savez(path, **{k: v.numpy() for k, v in back.items()})
    enc2 = GIN(out_dim=8, hidden_dim=16, n_layers=3, concat_hidden=True, weight_tying=False)
    with np.load(path) as z:
        load_param_dict(enc2, {k: z[k] for k in z.files})
    for k, v in param_dict(enc2).items():
        assert torch.equal(v, back[k]), k


def test_pair_predictor_builds_with_gin():
    from bmp.gin import GIN
    from bmp.predictor import build_pair_predictor
    m = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=3, attn=None, encoder="gin")
    enc = m.graph_conv
    # the trainer's call (train_ggnn_hole_multi_class_x37.py:226-228): dropout 0.5, concat_hidden, tied -> one layer runs
    assert isinstance(enc, GIN) and enc.dropout_ratio == 0.5 and enc.concat_hidden and enc.weight_tying
    assert enc.n_message_layers == 1 and len(enc.readout_layers) == 3
    assert m.mlp.layers[0].W.shape[1] == 2 * 16                       # one readout wide per molecule
    u = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=3, attn=None, encoder="gin", weight_tying=False, dropout_ratio=0.0)
    assert u.graph_conv.n_message_layers == 3 and u.graph_conv.dropout_ratio == 0.0
    assert u.mlp.layers[0].W.shape[1] == 2 * 3 * 16
    assert build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=2, attn="nie", encoder="gin").attn is not None
    with pytest.raises(ValueError):
        build_pair_predictor(encoder="weavenet")


def test_reference_import_paths():
    from models import GIN
    from models.gin import GIN as G2, GINUpdate, GGNNReadout       # noqa: F401
    import bmp.gin
    assert GIN is bmp.gin.GIN and G2 is GIN


def test_float_atom_features_are_refused():
    from bmp.gin import GIN
    with pytest.raises(NotImplementedError):
        GIN(out_dim=8)(np.zeros((2, 3, 16), np.float32), np.zeros((2, 4, 3, 3), np.float32))


def test_new_symbols_in_header_and_ctypes_table():
    from bmp import _lib
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    for name in ("bmp_gin_layer_supported", "bmp_gin_layer_tile_fwd", "bmp_gin_layer_tile_bwd"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "gcn-bmp_amd", "csrc", "bmp_gin.hip"))


def test_gin_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_gin.hip"), "-o", os.path.join(tmp, "gin.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 4, names                     # forward and backward at d = 64 and 128
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
