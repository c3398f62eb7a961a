"""CPU checks of the fuse-gate and simple-gate GGNN encoders' surface: constructors, parameter names and shapes, the snapshot round
trip, the pair predictor's wiring, the reference's import paths, the C ABI's new symbols, and zero scratch in the fused kernels."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import ggate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cls(kind):
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    return FuseGGNN if kind == "fuse" else GateGGNN


def test_constructor_defaults():
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    for cls in (FuseGGNN, GateGGNN):
        d = cls(out_dim=8)
        assert (d.hidden_dim, d.n_layers, d.concat_hidden, d.dropout_rate, d.batch_normalization, d.weight_tying) == \
            (16, 4, False, 0.0, False, True)
        assert tuple(d.embed.W.shape) == (117, 16) and d.n_message_layer == 1 and d.n_readout_layer == 1
        assert d.plannable() is False
        with pytest.raises(ValueError):
            cls(out_dim=8, hidden_dim=12)
        with pytest.raises(ValueError):
            cls(out_dim=8, dropout_rate=1.0)
    g = GateGGNN(out_dim=8)
    assert g.update_tying is True and g.n_update_layer == 1 and len(g.gate_layer) == 1
    assert GateGGNN(out_dim=8, n_layers=3, update_tying=False).n_update_layer == 3


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_parameter_names_and_shapes(kind):
    from bmp.snapshot import param_dict
    for tying, concat, upd in ((True, False, True), (True, True, False), (False, False, False), (False, True, True)):
        kw = dict(update_tying=upd) if kind == "gate" else {}
        enc = _cls(kind)(out_dim=12, hidden_dim=24, n_layers=3, concat_hidden=concat, weight_tying=tying, **kw)
        want = R.make_params(kind, 0, 24, 12, 3, tying, update_tying=upd, concat_hidden=concat)
        got = param_dict(enc)
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), k
    names = [n for n, _ in _cls(kind)(out_dim=8, weight_tying=False, n_layers=2).named_parameters()]
    assert "embed.W" in names and "message_layers.1.b" in names and "i_layers.0.W" in names and "j_layers.0.b" in names
    if kind == "fuse":
        assert {"update_layer1.W", "update_layer2.b", "update_layer3.W", "update_layer.U_r.W", "embed_linear.W"} <= set(names)
        assert tuple(_cls(kind)(out_dim=8).embed_linear.W.shape) == (16, 66)
    else:
        assert "gate_layer.0.W" in names and not any(n.startswith("update_layer") for n in names)


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_snapshot_round_trip(kind, tmp_path):
    from bmp.snapshot import load_param_dict, param_dict
    kw = dict(update_tying=False) if kind == "gate" else {}
    mk = lambda: _cls(kind)(out_dim=8, hidden_dim=16, n_layers=3, concat_hidden=True, weight_tying=False, **kw)
    p = R.make_params(kind, 3, 16, 8, 3, False, update_tying=False, concat_hidden=True)
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


def test_pair_predictor_builds_with_the_gated_encoders():
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    from bmp.predictor import build_pair_predictor
    for name, cls in (("ggnn-fuse", FuseGGNN), ("ggnn-gate", GateGGNN)):
        m = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=3, attn=None, encoder=name)
        enc = m.graph_conv
        assert type(enc) is cls and enc.weight_tying and not enc.concat_hidden and enc.n_layers == 3
        assert m.mlp.layers[0].W.shape[1] == 2 * 16
        u = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=3, attn="nie", encoder=name, weight_tying=False)
        assert u.graph_conv.n_message_layer == 3 and u.attn is not None
    with pytest.raises(ValueError):
        build_pair_predictor(encoder="ggnn-fuze")


def test_reference_import_paths():
    from models.ggnn_dev_fuse import GGNN as F
    from models.ggnn_dev_gate import GGNN as G
    import bmp.ggnn_gate as M
    assert F is M.FuseGGNN and G is M.GateGGNN and F.NUM_EDGE_TYPE == 4


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_float_atom_features_are_refused(kind):
    with pytest.raises(NotImplementedError):
        _cls(kind)(out_dim=8)(np.zeros((2, 3, 16), np.float32), np.zeros((2, 4, 3, 3), np.float32))


def test_new_symbols_in_header_and_ctypes_table():
    from bmp import _lib, functional as Fn
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    for name in ("bmp_ggnn_gate_step_supported", "bmp_ggnn_gate_step_tile_fwd", "bmp_ggnn_gate_step_tile_bwd"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "gcn-bmp_amd", "csrc", "bmp_gate.hip"))
    assert Fn.GATE_PATHS.keys() == {"fused", "composed"} and Fn.GATE_KIND == {"fuse": 0, "gate": 1}


def test_gate_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_gate.hip"), "-o", os.path.join(tmp, "gate.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 8, names                     # two kinds x forward and backward x d = 64 and 128
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    # and no fewer waves per SIMD than the kernels were written for: (d = 128, d = 64) per kernel
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    floor = {"fuse_fwd": (2, 5), "gate_fwd": (3, 5), "fuse_bwd": (3, 7), "gate_bwd": (3, 7)}
    assert len(occ) == 8, occ
    for n, o in zip(names, occ):
        *kind, d = re.search(r"k_(\w+?)_step_tile_(\w+?)ILi(\d+)E", n).groups()
        assert o >= floor["_".join(kind)][d == "64"], (n, o)
