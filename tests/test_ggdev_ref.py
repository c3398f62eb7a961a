"""Known answers that pin the float64 restatement of the ggnn_dev and self-loop GGNN encoders (tests/ggdev_ref.py) to the
reference's models/ggnn_dev.py and models/ggnn_dev_self_loop.py: the golden vectors (made by the plain-numpy transcription in
tests/golden/make_golden_ggdev.py) and algebraic identities that need no oracle.  No GPU."""
import os

import numpy as np
import torch

import ggdev_ref as R
from bmp import synth

D, OUT = 8, 4


def _batch():
    return synth.concat_mols(synth.make_store(4, seed=3, n_lo=2, n_hi=9, n_mean=5))


def _one_more_position(atoms, adj):
    mb, A = atoms.shape
    a = np.zeros((mb, A + 1), np.int32); a[:, :A] = atoms
    j = np.zeros((mb, 4, A + 1, A + 1), np.float32); j[:, :, :A, :A] = adj
    return a, j


def test_golden_vectors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ggnn_dev_small.npz"))
    atoms, adj = z["atoms"], z["adj"]
    assert atoms.shape[0] == 3 and (atoms == 0).any()                   # the batch is padded
    for kind, cfg in (("dev", dict(layers=3, tying=True, concat_hidden=False)), ("loop", dict(layers=3, tying=False, concat_hidden=True))):
        pre = kind + ":p:"
        p = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
        assert sorted(p) == sorted(R.make_params(kind, 0, D, OUT, cfg["layers"], cfg["tying"], cfg["concat_hidden"]))
        g, hs, gs = R.forward(kind, p, atoms, adj, **cfg)
        assert g.shape == ((3, D) if kind == "dev" else (3, 3 * OUT))    # dev: hidden wide, not out wide
        assert np.abs(g.numpy() - z[kind + ":g"]).max() < 1e-12
        assert np.abs(torch.stack(hs).numpy() - z[kind + ":hs"]).max() < 1e-12
        assert np.abs(torch.stack(gs).numpy() - z[kind + ":gs"]).max() < 1e-12


def test_zero_self_loop_is_the_plain_ggnn():
    atoms, adj = _batch()
    for tying, concat in ((True, False), (False, True)):
        p = R.make_params("loop", 3, D, OUT, 3, tying, concat)
        for k in p:
            if k.startswith("message_self_loop_layers/"):
                p[k] = torch.zeros_like(p[k])
        g, hs, _ = R.forward("loop", p, atoms, adj, 3, tying, concat)
        go, ho = R.O.ggnn_forward(p, torch.as_tensor(atoms), torch.as_tensor(adj).double(), 3, tying, concat)
        assert torch.equal(g, go) and torch.equal(hs[-1], ho)
    # ... and a self loop that is not zero moves it
    p = R.make_params("loop", 3, D, OUT, 3, True)
    g, _, _ = R.forward("loop", p, atoms, adj, 3)
    go, _ = R.O.ggnn_forward(p, torch.as_tensor(atoms), torch.as_tensor(adj).double(), 3)
    assert (g - go).abs().max() > 1e-2


def test_dev_is_the_plain_ggnn_up_to_what_it_returns():
    atoms, adj = _batch()
    p = R.make_params("dev", 4, D, OUT, 3, False)
    g, hs, gs = R.forward("dev", p, atoms, adj, 3, tying=False)
    go, ho = R.O.ggnn_forward(p, torch.as_tensor(atoms), torch.as_tensor(adj).double(), 3, False)
    assert torch.equal(hs[-1], ho) and torch.equal(gs[-1], go)           # the readout it computes and throws away
    assert g.shape == (4, D) and torch.equal(g, ho.sum(dim=1))
    assert len(hs) == len(gs) == 3 and all(x.shape == (4, OUT) for x in gs)
    pc = R.make_params("dev", 4, D, OUT, 3, False, concat_hidden=True)
    gc, _, gsc = R.forward("dev", pc, atoms, adj, 3, tying=False, concat_hidden=True)
    assert gc.shape == (4, 3 * OUT) and torch.equal(gc, torch.cat(gsc, dim=1))


def test_padding_law():
    """One more padded position moves every molecule's g by one common vector: the pad atom's h_T (dev: the sum runs over ALL
    positions) or its readout term (loop)."""
    atoms, adj = _batch()
    a1, j1 = _one_more_position(atoms, adj)
    assert (atoms == 0).any(axis=1).sum() >= 2                          # (molecules that are padded already)
    for kind in ("dev", "loop"):
        p = R.make_params(kind, 5, D, OUT, 3, True)
        g, _, _ = R.forward(kind, p, atoms, adj, 3)
        g1, hs1, _ = R.forward(kind, p, a1, j1, 3)
        step = g1 - g
        assert torch.allclose(step, step[0].expand_as(step), atol=1e-12) and step.abs().max() > 1e-3
        hp, h0p = hs1[-1][:, -1], p["embed/W"][0].expand(atoms.shape[0], -1)                   # the appended position
        if kind == "dev":
            want = hp
        else:
            want = torch.sigmoid(R.O.linear(torch.cat((hp, h0p), dim=1), p["i_layers/0/W"], p["i_layers/0/b"])) * \
                R.O.linear(hp, p["j_layers/0/W"], p["j_layers/0/b"])
        assert torch.allclose(step, want, atol=1e-12)
        # the pad trajectory of the self-loop form: no bonds, so m = W_s h + b_s
        if kind == "loop":
            e = p["embed/W"][0]
            m = R.O.linear(e, p["message_self_loop_layers/0/W"], p["message_self_loop_layers/0/b"])
            x = torch.cat((e, m))[None]
            s1 = R.O.stateful_gru({k: v for k, v in p.items() if k.startswith("update_layer/")}, "update_layer", x, None)
            assert torch.allclose(R.forward(kind, p, a1, j1, 1)[1][0][0, -1], s1[0], atol=1e-13)


def test_atom_permutation_invariance():
    atoms, adj = _batch()
    A = atoms.shape[1]
    perm = np.random.RandomState(0).permutation(A)
    ap, jp = atoms[:, perm], adj[:, :, perm][:, :, :, perm]
    for kind, concat in (("dev", False), ("dev", True), ("loop", False), ("loop", True)):
        p = R.make_params(kind, 6, D, OUT, 3, False, concat)
        g, hs, _ = R.forward(kind, p, atoms, adj, 3, False, concat)
        gp, hsp, _ = R.forward(kind, p, ap, jp, 3, False, concat)
        assert torch.allclose(g, gp, atol=1e-12)
        assert torch.allclose(hs[-1][:, perm], hsp[-1], atol=1e-12)


def test_first_step_uses_no_u_term():
    atoms, adj = _batch()
    for kind in ("dev", "loop"):
        p = R.make_params(kind, 7, D, OUT, 2, True)
        q = dict(p)
        for n in ("U_r", "U_z", "U"):
            q[f"update_layer/{n}/W"] = p[f"update_layer/{n}/W"] + 1.0
            q[f"update_layer/{n}/b"] = p[f"update_layer/{n}/b"] - 2.0
        q["update_layer/W_r/W"] = p["update_layer/W_r/W"] * 3.0          # the first call has no r gate either
        assert torch.equal(R.forward(kind, p, atoms, adj, 1)[0], R.forward(kind, q, atoms, adj, 1)[0])
        assert (R.forward(kind, p, atoms, adj, 2)[0] - R.forward(kind, q, atoms, adj, 2)[0]).abs().max() > 1e-3


def test_dropout_multiplies_the_output_and_not_the_gru_state():
    atoms, adj = _batch()
    p = R.make_params("loop", 8, D, OUT, 2, True)
    gen = torch.Generator().manual_seed(1)
    keep = [(torch.rand(atoms.shape + (D,), generator=gen) >= 0.5).double() * 2.0 for _ in range(2)]
    _, hs, _ = R.forward("loop", p, atoms, adj, 2)
    _, hk, _ = R.forward("loop", p, atoms, adj, 2, step_keep=keep)
    assert torch.equal(hk[0], hs[0] * keep[0])
    ones = [torch.ones_like(k) for k in keep]
    assert torch.equal(R.forward("loop", p, atoms, adj, 2, step_keep=ones)[1][1], hs[1])
    # a mask of zeros at step 1 hides the state from the message and the GRU's input, not from the GRU itself
    _, hz, _ = R.forward("loop", p, atoms, adj, 2, step_keep=[torch.zeros_like(keep[0]), ones[1]])
    assert hz[0].abs().max() == 0 and (hz[1] - hs[1]).abs().max() > 1e-3
    q = dict(p)
    q["update_layer/U_z/W"] = p["update_layer/U_z/W"] + 1.0
    assert (R.forward("loop", q, atoms, adj, 2, step_keep=[torch.zeros_like(keep[0]), ones[1]])[1][1] - hz[1]).abs().max() > 1e-3
