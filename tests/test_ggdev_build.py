"""CPU checks of the ggnn_dev and self-loop GGNN encoders' surface: constructors, parameter names and shapes, the snapshot round
trip, the pair predictor's wiring, the reference's import paths, the C ABI's new symbols, and zero scratch in the fused kernels."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import ggdev_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cls(kind):
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    return DevGGNN if kind == "dev" else SelfLoopGGNN


def test_constructor_defaults_and_refusals():
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    for cls in (DevGGNN, SelfLoopGGNN):
        d = cls(out_dim=8)
        assert (d.hidden_dim, d.n_layers, d.concat_hidden, d.dropout_rate, d.batch_normalization, d.weight_tying) == \
            (16, 4, False, 0.0, False, True)
        assert tuple(d.embed.W.shape) == (117, 16) and d.n_message_layer == 1 and d.n_readout_layer == 1
        assert d.plannable() is False
        with pytest.raises(ValueError):
            cls(out_dim=8, hidden_dim=12)
        with pytest.raises(ValueError):
            cls(out_dim=6)
        with pytest.raises(ValueError):
            cls(out_dim=8, dropout_rate=1.0)
        with pytest.raises(NotImplementedError):
            cls(out_dim=8, batch_normalization=True)
    assert DevGGNN(out_dim=8).output_atoms is True and DevGGNN(out_dim=8, output_atoms=False).output_atoms is False
    with pytest.raises(TypeError):
        SelfLoopGGNN(out_dim=8, output_atoms=True)                      # the file's constructor has no such argument
    s = SelfLoopGGNN(out_dim=8, n_layers=3, weight_tying=False)
    assert len(s.message_self_loop_layers) == 3 and tuple(s.message_self_loop_layers[2].W.shape) == (16, 16)
    assert len(SelfLoopGGNN(out_dim=8, n_layers=3).message_self_loop_layers) == 1


@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_parameter_names_and_shapes(kind):
    from bmp.snapshot import param_dict
    for tying, concat in ((True, False), (True, True), (False, False), (False, True)):
        enc = _cls(kind)(out_dim=12, hidden_dim=24, n_layers=3, concat_hidden=concat, weight_tying=tying)
        want = R.make_params(kind, 0, 24, 12, 3, tying, concat_hidden=concat)
        got = param_dict(enc)
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), k
    names = [n for n, _ in _cls(kind)(out_dim=8, weight_tying=False, n_layers=2).named_parameters()]
    assert {"embed.W", "message_layers.1.b", "update_layer.W_r.W", "update_layer.U.b", "i_layers.0.W", "j_layers.0.b"} <= set(names)
    assert ("message_self_loop_layers.1.W" in names) == (kind == "loop")


@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_snapshot_round_trip(kind, tmp_path):
    from bmp.snapshot import load_param_dict, param_dict
    mk = lambda: _cls(kind)(out_dim=8, hidden_dim=16, n_layers=3, concat_hidden=True, weight_tying=False)
    p = R.make_params(kind, 3, 16, 8, 3, False, concat_hidden=True)
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


def test_pair_predictor_builds_with_both_encoders():
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    from bmp.predictor import build_pair_predictor
    for name, cls in (("ggnn-dev", DevGGNN), ("ggnn-self-loop", SelfLoopGGNN)):
        m = build_pair_predictor(hidden_dim=24, out_dim=16, n_layers=3, attn=None, encoder=name)
        enc = m.graph_conv
        assert type(enc) is cls and enc.weight_tying and not enc.concat_hidden and enc.n_layers == 3
        # without a co-attention ggnn_dev hands over the hidden-wide sum of its atom states, the self-loop form its readout
        assert m.mlp.layers[0].W.shape[1] == 2 * (24 if name == "ggnn-dev" else 16)
        u = build_pair_predictor(hidden_dim=24, out_dim=16, n_layers=3, attn="nie", encoder=name, weight_tying=False)
        assert u.graph_conv.n_message_layer == 3 and u.attn is not None and u.mlp.layers[0].W.shape[1] == 2 * 16
    with pytest.raises(ValueError):
        build_pair_predictor(encoder="ggnn-devel")


def test_reference_import_paths():
    from models.ggnn_dev import GGNN as Dv
    from models.ggnn_dev_self_loop import GGNN as Sl
    from models.ggnn_dev_edge import GGNN as Ed
    import bmp.ggnn_dev as M
    assert Dv is M.DevGGNN and Sl is M.SelfLoopGGNN and Ed is M.SelfLoopGGNN and Dv.NUM_EDGE_TYPE == Sl.NUM_EDGE_TYPE == 4


@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_float_atom_features_are_refused(kind):
    with pytest.raises(NotImplementedError):
        _cls(kind)(out_dim=8)(np.zeros((2, 3, 16), np.float32), np.zeros((2, 4, 3, 3), np.float32))


def test_new_symbols_in_header_and_ctypes_table():
    from bmp import _lib, functional as Fn
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    for name in ("bmp_ggnn_loop_step_supported", "bmp_ggnn_loop_step_tile_fwd", "bmp_ggnn_loop_step_tile_bwd"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "gcn-bmp_amd", "csrc", "bmp_loop.hip"))
    assert Fn.LOOP_PATHS.keys() == {"fused", "composed"}
    assert callable(Fn.loop_step) and callable(Fn.loop_step_supported) and issubclass(Fn.LoopStepFn, torch.autograd.Function)


def test_loop_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_loop.hip"), "-o", os.path.join(tmp, "loop.o"),
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
        *kind, d = re.search(r"k_loop_step_(\w+?)ILi(\d+)E", n).groups()
        assert o >= floor["_".join(kind)][d == "64"], (n, o)
