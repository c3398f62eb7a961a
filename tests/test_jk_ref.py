"""CPU checks of the jumping-knowledge encoders' restatement (tests/jk_ref.py) itself: known answers worked out by hand, the relu kink
condition and the 'attn' coefficient range of every case in its table, and the distance of its float32 form from its float64
form, which bounds what a correct float32 implementation can be asked for."""
import numpy as np
import pytest
import torch

import jk_ref as R


def _mol(n_atoms, bonds, A):
    """(atoms (1, A) int32, adj (1, 4, A, A) float32): ``bonds`` (i, j, type), symmetric; positions >= n_atoms are padding (id 0)."""
    atoms = np.zeros((1, A), np.int32)
    atoms[0, :n_atoms] = [6, 7, 8, 9, 15, 16][:n_atoms]
    adj = np.zeros((1, 4, A, A), np.float32)
    for i, j, t in bonds:
        adj[0, t, i, j] = adj[0, t, j, i] = 1.0
    return atoms, adj


def test_bondless_molecule_is_relu_of_the_h_half():
    """No bond: the adjacency is zero, so the message is zero (its bias passes through the adjacency product too) and
    h' = relu(W[:, :d] h + b)."""
    d = 8
    p = R.make_params("jknet", 1, d, 4, 1, True)
    atoms, adj = _mol(3, [], 5)
    _, y, _ = R.forward("jknet", p, atoms, adj, 1, aggr="concat")
    h0 = p["embed/W"][torch.as_tensor(atoms).long()]
    want = torch.relu(h0 @ p["update_layer/0/W"][:, :d].t() + p["update_layer/0/b"])
    assert torch.allclose(y, want, rtol=0, atol=1e-14)
    # jk_gru's 2d-wide layer, with the self loop: m = W_s h + b_s
    q = R.make_params("jk_gru", 2, d, 4, 1, True, self_loop=True)
    st = []
    R.forward("jk_gru", q, atoms, adj, 1, self_loop=True, states=st)
    e = q["embed/W"][torch.as_tensor(atoms).long()].reshape(-1, d)
    m = e @ q["self_loop_layer/W"].t() + q["self_loop_layer/b"]
    x = torch.relu(torch.cat((e, m), 1) @ q["update_layers_0/0/W"].t() + q["update_layers_0/0/b"])
    lin = lambda n: x @ q[f"update_layer/{n}/W"].t() + q[f"update_layer/{n}/b"]
    want = torch.sigmoid(lin("W_z")) * torch.tanh(lin("W"))              # the first call after reset: no r gate, no U terms
    assert torch.allclose(st[0].reshape(-1, d), want, rtol=0, atol=1e-14)


def test_attn_of_equal_states_is_uniform_and_mean_of_equal_tensors_is_the_tensor():
    h = torch.randn(3, 5, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    for T in (1, 2, 3, 5):
        y, c = R.aggregate("attn", [h] * T)
        assert torch.allclose(c, torch.full((T,), 1.0 / T, dtype=torch.float64), rtol=0, atol=1e-15)
        assert torch.allclose(y, h, rtol=0, atol=1e-14)
        ym, cm = R.aggregate("mean", [h] * T)
        assert cm is None and torch.allclose(ym, h, rtol=0, atol=1e-15)
    a, b = h, 2 * h
    assert torch.equal(R.aggregate("mean", [a, b])[0], 1.5 * h)
    assert torch.equal(R.aggregate("max", [a, b, -h])[0], torch.maximum(torch.maximum(a, b), -h))


def test_attn_energies_by_hand():
    """Two steps: E_1 = <H_1, H_2> + <H_1, H_1>, E_2 = <H_2, H_2> + <H_2, H_1>."""
    g = torch.Generator().manual_seed(1)
    h1, h2 = (torch.randn(2, 3, 4, dtype=torch.float64, generator=g) for _ in range(2))
    E = R.attn_energies([h1, h2])
    assert torch.allclose(E, torch.stack(((h1 * h2).sum() + (h1 * h1).sum(), (h2 * h2).sum() + (h2 * h1).sum())), rtol=1e-14, atol=0)
    y, c = R.aggregate("attn", [h1, h2])
    w = torch.exp(E - E.max())
    assert torch.allclose(c, w / w.sum(), rtol=1e-14, atol=0) and torch.allclose(y, c[0] * h1 + c[1] * h2, rtol=1e-14, atol=0)


def test_one_more_padded_position_adds_the_pad_states_own_inner_products():
    """Every padded position carries the same states p_t (id 0, no bonds), and no other position sees it: padding to A + 1
    changes E_t by exactly <p_t, p_T> + <p_t, p_1>.  The energies -- and with them every molecule's vector -- depend on A."""
    d, T = 8, 3
    p = R.make_params("jknet", 3, d, 4, T, False, update_tying=False, scale=0.3)
    bonds = [(0, 1, 0), (1, 2, 1), (2, 3, 3)]
    E, pad = [], None
    for A in (6, 7):
        atoms, adj = _mol(4, bonds, A)
        st = []
        R.forward("jknet", p, atoms, adj, T, False, False, aggr="attn", states=st)
        E.append(R.attn_energies(st))
        pad = [s[0, -1] for s in st]
        assert all(torch.equal(s[0, 4], s[0, -1]) for s in st)
    want = torch.stack([(pad[t] * pad[-1]).sum() + (pad[t] * pad[0]).sum() for t in range(T)])
    assert want.abs().min() > 1e-6
    assert torch.allclose(E[1] - E[0], want, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("kind,aggr", [("jknet", "attn"), ("jknet", "max"), ("jknet", "mean"), ("jk_gru", None)])
def test_atom_permutation_leaves_g_unchanged(kind, aggr):
    d, T = 8, 2
    p = R.make_params(kind, 4, d, 4, T, True, self_loop=True, scale=0.3)
    atoms, adj = _mol(5, [(0, 1, 0), (1, 2, 1), (2, 3, 2), (3, 4, 3), (0, 4, 0)], 7)
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    g0 = R.forward(kind, p, atoms, adj, T, aggr=aggr, self_loop=True)[0]
    g1 = R.forward(kind, p, atoms[:, perm], adj[:, :, perm][:, :, :, perm], T, aggr=aggr, self_loop=True)[0]
    assert torch.allclose(g0, g1, rtol=1e-12, atol=1e-14)
    assert g0.abs().max() > 1e-3


def test_jk_gru_reads_update_layer_zero_when_messages_are_tied():
    """ggnn_dev_jk_gru.py:80: the index is 0 if weight_tying else step, whatever update_tying says -- layers 1.. are never read."""
    p = R.make_params("jk_gru", 5, 8, 4, 3, True, update_tying=False)
    atoms, adj = _mol(4, [(0, 1, 0), (1, 2, 1)], 5)
    g0 = R.forward("jk_gru", p, atoms, adj, 3, True, False)[0]
    q = dict(p)
    for k in (1, 2):
        q[f"update_layers_0/{k}/W"] = torch.zeros_like(p[f"update_layers_0/{k}/W"])
    assert torch.equal(g0, R.forward("jk_gru", q, atoms, adj, 3, True, False)[0])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_no_preactivation_sits_on_the_relu_kink(name):
    """min |pre| over every relu of the case >= KINK_FACTOR x the float32 restatement's worst error at a pre-activation: an
    implementation with that error takes the same side of every relu (tests/jk_ref.py's table gives the figures)."""
    lo, err = R.kink_margin(R.CASES[name], R.KEEP_SEEDS.get(name))
    print(f"[kink] {name}: min|pre64| {lo:.3e}  max|pre32-pre64| {err:.3e}  margin {lo / err:.1f}x")
    assert R.KINK_FACTOR >= 1.0 and lo >= R.KINK_FACTOR * err, (name, lo, err)


@pytest.mark.parametrize("name", sorted(n for n, c in R.CASES.items() if c["aggr"] == "attn"))
def test_attn_coefficients_are_not_saturated(name):
    """Every coefficient of every side in [0.02, 0.95]: a saturated softmax would hide a wrong energy."""
    r = R.reference(name, keep_seed=R.KEEP_SEEDS.get(name))
    lo, hi = R.ATTN_COEF_RANGE
    assert (lo, hi) == (0.02, 0.95)
    for c in r["coef"]:
        print(f"[coef] {name}: " + " ".join(f"{x:.3f}" for x in c.tolist()))
        assert c.min().item() >= lo and c.max().item() <= hi, (name, c)
        assert abs(c.sum().item() - 1.0) < 1e-12
    if R.CASES[name]["layers"] > 1:       # and not the uniform 1 / T either, which would hide them as well
        assert max((c.max() - c.min()).item() for c in r["coef"]) > 0.05


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float32_restatement_is_within_a_tenth_of_the_parity_bound(name):
    """max-norm relative distance of the float32 restatement from the float64 one over g, the atom states and every parameter
    gradient <= 1e-5, a tenth of parity_util.close's 1e-4."""
    ks = R.KEEP_SEEDS.get(name)
    a, b = R.reference(name, keep_seed=ks), R.reference(name, keep_seed=ks, dtype=torch.float32)
    rel = lambda x, y: ((x.double() - y).abs().max() / max(y.abs().max().item(), 1e-6)).item()
    worst = max([rel(b["g"], a["g"])] + [rel(x, y) for x, y in zip(b["atoms"], a["atoms"])]
                + [rel(b["p"][k].grad, a["p"][k].grad) for k in a["p"] if a["p"][k].grad is not None])
    print(f"[f32] {name}: {worst:.2e}")
    assert R.F32_BOUND == 1e-5 and worst <= R.F32_BOUND, (name, worst)
    assert all((a["p"][k].grad is None) == (b["p"][k].grad is None) for k in a["p"])


def test_data_sets_are_the_shared_ones():
    import ggate32_ref
    import gin_ref
    assert R.data is ggate32_ref.data and R.data("fixture") is gin_ref.data("fixture")
    assert {c["data"] for c in R.CASES.values()} == {"fixture", "small", "oversized", "blocks", "dense"}
    assert ggate32_ref.blocks_property(R.data("blocks")["pb"]) and ggate32_ref.dense_property(R.data("dense")["pb"])
