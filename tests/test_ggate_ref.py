"""Known answers that pin the float64 restatement of the fuse-gate and simple-gate GGNN encoders (tests/ggate_ref.py) to the
reference's models/ggnn_dev_fuse.py and models/ggnn_dev_gate.py: the golden vectors (made by the plain-numpy transcription in
tests/golden/make_golden_ggate.py) and algebraic identities that need no oracle.  No GPU."""
import os

import numpy as np
import torch

import ggate_ref as R
from bmp import synth

D, O = 8, 4


def _batch():
    return synth.concat_mols(synth.make_store(4, seed=3, n_lo=2, n_hi=9, n_mean=5))


def _states(kind, p, atoms, adj, layers, **kw):
    """h after 0 .. layers steps (the restatement run with fewer steps: the loop has no other state)."""
    return [p["embed/W"][torch.as_tensor(atoms).long()]] + [R.forward(kind, p, atoms, adj, n, **kw)[1] for n in range(1, layers + 1)]


def test_golden_vectors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ggnn_gate_small.npz"))
    atoms, adj = z["atoms"], z["adj"]
    assert atoms.shape[0] == 3 and (atoms == 0).any()                   # the batch is padded
    for kind, cfg in (("fuse", dict(layers=3, tying=True, update_tying=True, concat_hidden=False)),
                      ("gate", dict(layers=2, tying=False, update_tying=False, concat_hidden=True))):
        pre = kind + ":p:"
        p = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
        assert sorted(p) == sorted(R.make_params(kind, 0, D, O, cfg["layers"], cfg["tying"], cfg["update_tying"], cfg["concat_hidden"]))
        g, h = R.forward(kind, p, atoms, adj, **cfg)
        assert g.shape == (3, O * (cfg["layers"] if cfg["concat_hidden"] else 1))
        assert np.abs(g.numpy() - z[kind + ":g"]).max() < 1e-12 and np.abs(h.numpy() - z[kind + ":h"]).max() < 1e-12


def test_gate_closed_leaves_h_and_open_gives_m():
    atoms, adj = _batch()
    p = R.make_params("gate", 3, D, O, 2, False)
    p["gate_layer/0/W"] = torch.zeros_like(p["gate_layer/0/W"])
    h0 = p["embed/W"][torch.as_tensor(atoms).long()]
    p["gate_layer/0/b"] = torch.full_like(p["gate_layer/0/b"], -40.0)
    _, h = R.forward("gate", p, atoms, adj, 2, tying=False)
    assert torch.allclose(h, h0, atol=1e-14)                            # sigmoid(-40) = 4e-18
    p["gate_layer/0/b"] = torch.full_like(p["gate_layer/0/b"], 40.0)
    _, h1 = R.forward("gate", p, atoms, adj, 1, tying=False)
    m = R.O.ggnn_message(h0, torch.as_tensor(adj).double(), p["message_layers/0/W"], p["message_layers/0/b"])
    assert torch.allclose(h1, m, atol=1e-13) and (m - h0).abs().max() > 0.1


def test_gate_update_tying_picks_the_layer():
    atoms, adj = _batch()
    p = R.make_params("gate", 4, D, O, 3, True, update_tying=False)
    assert sum(k.startswith("gate_layer/") for k in p) == 6 and sum(k.startswith("message_layers/") for k in p) == 2
    _, h = R.forward("gate", p, atoms, adj, 3, update_tying=False)
    q = dict(p)
    q["gate_layer/2/W"] = p["gate_layer/2/W"] + 1.0                     # only the third step reads it
    hs, hq = _states("gate", p, atoms, adj, 3, update_tying=False), _states("gate", q, atoms, adj, 3, update_tying=False)
    assert torch.equal(hs[2], hq[2]) and not torch.allclose(hs[3], hq[3], atol=1e-3) and torch.equal(hs[3], h)
    _, ht = R.forward("gate", q, atoms, adj, 3, update_tying=True)      # tied: layer 0 at every step, layer 2 unread
    assert torch.equal(ht, R.forward("gate", p, atoms, adj, 3, update_tying=True)[1])


def test_fuse_with_f_closed_is_r_times_h():
    atoms, adj = _batch()
    p = R.make_params("fuse", 5, D, O, 1, True)
    p["update_layer3/W"] = torch.zeros_like(p["update_layer3/W"])
    p["update_layer3/b"] = torch.full_like(p["update_layer3/b"], -40.0)
    h0 = p["embed/W"][torch.as_tensor(atoms).long()]
    m = R.O.ggnn_message(h0, torch.as_tensor(adj).double(), p["message_layers/0/W"], p["message_layers/0/b"])
    r = torch.sigmoid(R.O.linear(torch.cat((h0, m), dim=2), p["update_layer2/W"], p["update_layer2/b"]))
    _, h = R.forward("fuse", p, atoms, adj, 1)
    assert torch.allclose(h, r * h0, atol=1e-14)


def test_fuse_dropout_multiplies_r_h_only_and_eval_has_none():
    atoms, adj = _batch()
    p = R.make_params("fuse", 6, D, O, 1, True)
    gen = torch.Generator().manual_seed(1)
    keep = (torch.rand(atoms.shape + (D,), generator=gen) >= 0.5).double() * 2.0
    _, h_eval = R.forward("fuse", p, atoms, adj, 1)
    _, h_ones = R.forward("fuse", p, atoms, adj, 1, keep=[torch.ones_like(keep)])
    assert torch.equal(h_eval, h_ones)                                  # evaluation mode: the dropout is the identity
    _, h_keep = R.forward("fuse", p, atoms, adj, 1, keep=[keep])
    _, h_zero = R.forward("fuse", p, atoms, adj, 1, keep=[torch.zeros_like(keep)])       # = f * z
    assert torch.allclose(h_keep - h_zero, keep * (h_eval - h_zero), atol=1e-13)
    # the links the file constructs and never calls do not enter
    q = dict(p)
    for k in p:
        if k.startswith("update_layer/") or k.startswith("embed_linear/"):
            q[k] = p[k] + 1.0
    assert torch.equal(R.forward("fuse", q, atoms, adj, 1)[1], h_eval)


def test_fuse_update_is_shared_by_untied_steps_and_padding_counts():
    atoms, adj = _batch()
    p = R.make_params("fuse", 7, D, O, 3, False, concat_hidden=True)
    assert sum(k.startswith("message_layers/") for k in p) == 6 and sum(k.startswith("update_layer1/") for k in p) == 2
    g, _ = R.forward("fuse", p, atoms, adj, 3, tying=False, concat_hidden=True)
    assert g.shape == (4, 3 * O)
    # the readout sums over ALL positions: one more padded position moves every molecule's g by one common vector
    mb, A = atoms.shape
    a = np.zeros((mb, A + 1), np.int32); a[:, :A] = atoms
    j = np.zeros((mb, 4, A + 1, A + 1), np.float32); j[:, :, :A, :A] = adj
    g1, _ = R.forward("fuse", p, a, j, 3, tying=False, concat_hidden=True)
    step = g1 - g
    assert torch.allclose(step, step[0].expand_as(step), atol=1e-12) and step.abs().max() > 1e-3
