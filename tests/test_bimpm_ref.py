"""tests/bimpm_ref.py (the packed-row float64 BiMPM with explicit selections the GPU edge tests compare against) pinned to
the dense oracle restatement on CPU: values and gradients with w = 1, row multiplicities as dense copies, w = 0 rows as
deleted rows, forced selections, the zero-norm convention, tau against a float32 evaluation; and the host-side layout
query the GPU tests read the kernel's selections with."""
import ctypes

import pytest
import torch

import bimpm_ref as BR
from oracle import ref_cpu as O

NAMES = ("max_pooling_W", "att_mean_W", "att_max_W")


def _inputs(n1, n2, d, H, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x1, x2 = torch.randn(n1, d, generator=g, dtype=dtype), torch.randn(n2, d, generator=g, dtype=dtype)
    W = [torch.randn(H, d, generator=g, dtype=dtype) * (2.0 / d) ** 0.5 for _ in range(3)]
    c1, c2 = torch.randn(3 * H, generator=g, dtype=dtype), torch.randn(3 * H, generator=g, dtype=dtype)
    return x1, x2, W, c1, c2


def _leaves(*ts):
    return [t.detach().clone().requires_grad_() for t in ts]


def _oracle(x1, x2, W, c1, c2):
    x1, x2, *W = _leaves(x1, x2, *W)
    m1, m2 = O.bimpm_coattention(dict(zip(NAMES, W)), x1[None], x2[None])
    ((m1[0] * c1).sum() + (m2[0] * c2).sum()).backward()
    return m1[0].detach(), m2[0].detach(), [x1.grad, x2.grad] + [w.grad for w in W]


def _ref(x1, x2, w1, w2, W, c1, c2, sel=None):
    x1, x2, *W = _leaves(x1, x2, *W)
    r = BR.bimpm_pair(x1, x2, w1, w2, *W, sel=sel)
    ((r["mol_1"] * c1).sum() + (r["mol_2"] * c2).sum()).backward()
    return r["mol_1"].detach(), r["mol_2"].detach(), [x1.grad, x2.grad] + [w.grad for w in W], r


def _same(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-6)


@pytest.mark.parametrize("n1,n2,d,H", [(1, 1, 8, 3), (1, 6, 5, 1), (7, 1, 16, 4), (5, 4, 32, 8), (13, 9, 12, 5)])
def test_reference_equals_dense_oracle(n1, n2, d, H):
    x1, x2, W, c1, c2 = _inputs(n1, n2, d, H, seed=n1 * 100 + n2)
    m1o, m2o, go = _oracle(x1, x2, W, c1, c2)
    m1, m2, gr, _ = _ref(x1, x2, torch.ones(n1), torch.ones(n2), W, c1, c2)
    _same(m1, m1o); _same(m2, m2o)
    for a, b in zip(gr, go):
        _same(a, b)


@pytest.mark.parametrize("m", [2, 3])
def test_row_multiplicity_is_dense_copies(m):
    n1, n2, d, H = 5, 6, 8, 4
    x1, x2, W, c1, c2 = _inputs(n1, n2, d, H, seed=7)
    w1, w2 = torch.ones(n1), torch.ones(n2)
    w1[2] = m; w2[0] = m
    m1, m2, gr, _ = _ref(x1, x2, w1, w2, W, c1, c2)
    # dense: the copies appended behind the originals
    d1 = torch.cat([x1, x1[2:3].expand(m - 1, d)]); d2 = torch.cat([x2, x2[0:1].expand(m - 1, d)])
    m1o, m2o, go = _oracle(d1, d2, W, c1, c2)
    _same(m1, m1o); _same(m2, m2o)
    g1 = go[0][:n1].clone(); g1[2] += go[0][n1:].sum(0)
    g2 = go[1][:n2].clone(); g2[0] += go[1][n2:].sum(0)
    _same(gr[0], g1); _same(gr[1], g2)
    for a, b in zip(gr[2:], go[2:]):
        _same(a, b)


def test_zero_weight_row_is_a_deleted_row():
    n1, n2, d, H = 6, 5, 8, 3
    x1, x2, W, c1, c2 = _inputs(n1, n2, d, H, seed=11)
    x1[1] = 3.0e4 * torch.sign(x1[1]); x2[4] *= -7.0e3                 # large finite values a maximum would pick
    w1, w2 = torch.ones(n1), torch.ones(n2)
    w1[1] = 0; w2[4] = 0; w1[3] = 2
    m1, m2, gr, r = _ref(x1, x2, w1, w2, W, c1, c2)
    k1, k2 = [0, 2, 3, 4, 5], [0, 1, 2, 3]
    m1d, m2d, gd, _ = _ref(x1[k1], x2[k2], w1[k1], w2[k2], W, c1, c2)
    _same(m1, m1d); _same(m2, m2d)
    assert (gr[0][1] == 0).all() and (gr[1][4] == 0).all()
    _same(gr[0][k1], gd[0]); _same(gr[1][k2], gd[1])
    for a, b in zip(gr[2:], gd[2:]):
        _same(a, b)
    live = torch.tensor([True, False, True, True, True, True])
    assert (r["sel"]["iT1"] != 1).all() and (r["sel"]["i2s"] != 1).all()
    assert (r["sel"]["jT2"][live] != 4).all() and (r["sel"]["j1s"][live] != 4).all()


def test_forcing_own_selections_changes_nothing():
    x1, x2, W, c1, c2 = _inputs(9, 7, 16, 4, seed=3)
    w1, w2 = torch.ones(9), torch.ones(7)
    m1, m2, gr, r = _ref(x1, x2, w1, w2, W, c1, c2)
    m1f, m2f, gf, _ = _ref(x1, x2, w1, w2, W, c1, c2, sel=r["sel"])
    assert torch.equal(m1, m1f) and torch.equal(m2, m2f)
    for a, b in zip(gr, gf):
        assert torch.equal(a, b)
    assert max(BR.selection_gaps(x1, x2, w1, w2, W[0], r["sel"]).values()) == 0.0


def test_forcing_other_selections_moves_the_gradient_to_them():
    """a forced loser gets the maximum's whole gradient and the float64 winner none of it"""
    x1, x2, W, c1, c2 = _inputs(4, 5, 8, 2, seed=5)
    w1, w2 = torch.ones(4), torch.ones(5)
    _, _, _, r = _ref(x1, x2, w1, w2, W, c1, c2)
    sel = {k: v.clone() for k, v in r["sel"].items()}
    sel["j1s"][0, 1] = (sel["j1s"][0, 1] + 1) % 5
    m1f, _, _, _ = _ref(x1, x2, w1, w2, W, c1, c2, sel=sel)
    want = r["scores"]["pool"][0, sel["j1s"][0, 1], 1] - r["scores"]["pool"][0, r["sel"]["j1s"][0, 1], 1]
    _same(m1f[1] - r["mol_1"][1].detach(), want, tol=1e-9)
    gaps = BR.selection_gaps(x1, x2, w1, w2, W[0], sel)
    assert gaps["j1s"] > 1.0 and gaps["jT2"] == 0.0                    # far beyond tau: not a selection float32 may make


def test_exact_ties_take_the_first_index():
    x1, x2, W, c1, c2 = _inputs(4, 6, 8, 3, seed=9)
    x2[4] = x2[1]
    r = BR.bimpm_pair(x1, x2, torch.ones(4), torch.ones(6), *W)
    assert (r["sel"]["j1s"] != 4).all() and (r["sel"]["jT2"] != 4).all()


def test_zero_row_has_finite_gradients():
    x1, x2, W, c1, c2 = _inputs(4, 3, 8, 2, seed=13)
    x1[2] = 0
    w1 = torch.tensor([1.0, 1.0, 2.0, 1.0])
    m1, m2, gr, _ = _ref(x1, x2, w1, torch.ones(3), W, c1, c2)
    for t in [m1, m2] + gr:
        assert torch.isfinite(t).all()
    # derivative 0 of every norm at 0: what is left at the zero row is d att / d x = y / (eps (|y| + eps)) and the like,
    # the limit of the gradient along x -> 0 only in its eps-regularised form; checked against a one-sided difference of
    # the SAME function is not possible (|u| has a kink), so pin the convention itself
    u = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    BR._norm(u).backward()
    assert (u.grad == 0).all()


@pytest.mark.parametrize("n1,n2,d,H", [(9, 13, 32, 8), (40, 33, 128, 16), (60, 50, 64, 4)])
def test_float32_evaluation_stays_within_tau(n1, n2, d, H):
    """selections of this file evaluated in float32 (torch's summation order, not the kernel's: the bound holds for any)
    lie within tau of the float64 maxima, with room: the derivation is a worst case"""
    g = torch.Generator().manual_seed(d + n1)
    x1, x2 = torch.randn(n1, d, generator=g), torch.randn(n2, d, generator=g)          # float32 values, exact in float64
    W = [torch.randn(H, d, generator=g) * (2.0 / d) ** 0.5 for _ in range(3)]
    x2[3] = x2[0] * (1 + 2.0 ** -20)                                                   # a near-tie on purpose
    w1, w2 = torch.ones(n1), torch.ones(n2)
    s32 = BR.bimpm_pair(x1, x2, w1, w2, *W, dtype=torch.float32)["sel"]
    gaps = BR.selection_gaps(x1, x2, w1, w2, W[0], s32)
    assert max(gaps.values()) <= 1.0, gaps
    assert BR.tau_pool(d) == 2 * (2 * d + 16) * 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    return _lib.lib()


@pytest.mark.parametrize("d,H,maxn", [(16, 4, 7), (128, 16, 157), (128, 16, 158), (64, 16, 330), (5, 3, 1)])
@pytest.mark.parametrize("bwd", [0, 1])
def test_workspace_layout_query(lib, d, H, maxn, bwd):
    """host arithmetic only: the stride is what one workgroup's share of the workspace is sized by, the four index arrays lie
    in carve-up order inside it, [maxn x d] and [maxn x H] apart"""
    out = (ctypes.c_size_t * 5)()
    assert lib.bmp_bimpm_ws_layout(d, H, maxn, bwd, out) == 0
    stride, jT2, iT1, j1s, i2s = list(out)
    assert lib.bmp_bimpm_ws_floats(d, H, maxn, 1, bwd) == stride + (3 * H * d if bwd else 0)
    assert lib.bmp_bimpm_ws_floats(d, H, maxn, 700, bwd) == 512 * (stride + (3 * H * d if bwd else 0))
    assert iT1 - jT2 == maxn * d and j1s > iT1 + maxn * d - 1 and i2s - j1s == maxn * H and i2s + maxn * H <= stride
    assert jT2 == 6 * maxn * H + 2 * maxn + maxn * maxn + 2 * maxn + 4 * maxn * d          # nP..nR, nx ny, att, D, M M T T
    assert lib.bmp_bimpm_ws_layout(d, H, maxn, bwd, None) != 0 and lib.bmp_bimpm_ws_layout(d, 0, maxn, bwd, out) != 0
