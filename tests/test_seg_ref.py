"""Pins the float64 packed restatement of the segment operators and the coarse co-attention modules (tests/seg_ref.py):
every module on a packed batch equals the dense oracle on ``pb.to_dense``, ``rowcorr`` equals the oracle's FFT form,
hand-computed answers for the softmax with multiplicities and the pool with a per-row weight, and the relu kink condition
of Neural's relu case.  No GPU."""
import numpy as np
import pytest
import torch

import seg_ref as SR
from oracle import ref_cpu as O

REL = 1e-10
D, OUT = 12, 8


def _rel(got, want):
    return (got - want).abs().max().item() / want.abs().max().item()


@pytest.fixture(scope="module")
def small():
    """Two-sided batch with a dense map: a single-atom molecule, pad rows of multiplicity 11, 9 and 5, and the 12-atom
    molecule on either side, whose pad row has multiplicity 0."""
    pb = SR.fixture_batch(sizes=(1, 3, 7, 7, 12), partner=(4, 2, 1, 0, 3), with_dense_map=True)[0]
    w = pb.row_w[pb.row_mol >= 0]
    assert (w > 1).sum() >= 6 and int(pb.mol_nrows.min()) == 2
    pads = pb.mol_row0.long() + pb.mol_nrows.long() - 1
    assert (pb.row_w[pads] == 0).sum() == 2
    g = torch.Generator().manual_seed(3)
    X = torch.randn(pb.n_rows, D, generator=g, dtype=torch.float64)          # rows of no molecule hold random values too
    g_1 = torch.randn(5, OUT, generator=g, dtype=torch.float64)
    g_2 = torch.randn(5, OUT, generator=g, dtype=torch.float64)
    return pb, X, g_1, g_2


def _draw(init, seed, *a, **kw):
    dr = O._Draw(seed, torch.float64, 0.2)
    init(dr, "", *a, **kw)
    return dr.p


def _check(got, want):
    for k in (0, 1):
        assert got[k].shape == want[k].shape and _rel(got[k], want[k]) <= REL


@pytest.mark.parametrize("tying", [True, False])
@pytest.mark.parametrize("act", ["tanh", "sigmoid", "relu"])
def test_parallel_equals_the_dense_oracle(small, tying, act):
    pb, X, g_1, g_2 = small
    p = _draw(O.init_parallel, 1, D, OUT, 1, weight_tying=tying)
    want = O.parallel_coattention(p, pb.to_dense(X, 0), g_1, pb.to_dense(X, 1), g_2, activation=act, weight_tying=tying)
    _check(SR.parallel(p, *_sg(pb, X, g_1, g_2), activation=act, weight_tying=tying), want)


def _sg(pb, X, g_1, g_2):
    s1, s2 = SR.sides_of(pb, X)
    return s1, g_1, s2, g_2


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_circ_equals_the_dense_oracle(small, act):
    pb, X, g_1, g_2 = small
    p = {k: v for k, v in _draw(O.init_parallel, 2, D, OUT).items() if k.startswith("j_layer/")}
    want = O.circular_parallel_coattention(p, pb.to_dense(X, 0), g_1, pb.to_dense(X, 1), g_2, activation=act)
    _check(SR.circ(p, *_sg(pb, X, g_1, g_2), activation=act), want)


@pytest.mark.parametrize("head", [5, 8])
def test_alternating_equals_the_dense_oracle(small, head):
    pb, X, g_1, g_2 = small
    p = _draw(O.init_alternating, 3, D, OUT, head)
    want = O.alternating_coattention(p, pb.to_dense(X, 0), g_1, pb.to_dense(X, 1), g_2)
    _check(SR.alternating(p, *_sg(pb, X, g_1, g_2)), want)


@pytest.mark.parametrize("tying", [True, False])
def test_global_equals_the_dense_oracle(small, tying):
    pb, X, _, _ = small
    p = _draw(O.init_global, 4, D, OUT, weight_tying=tying)
    want = O.global_coattention(p, pb.to_dense(X, 0), pb.to_dense(X, 1), weight_tying=tying)
    _check(SR.global_(p, *SR.sides_of(pb, X), weight_tying=tying), want)


@pytest.mark.parametrize("tying", [True, False])
@pytest.mark.parametrize("act", ["tanh", "sigmoid", "relu"])
def test_neural_equals_the_dense_oracle(small, tying, act):
    pb, X, _, _ = small
    p = _draw(O.init_neural, 5, D, OUT, weight_tying=tying)
    want = O.neural_coattention(p, pb.to_dense(X, 0), pb.to_dense(X, 1), activation=act, weight_tying=tying)
    _check(SR.neural(p, *SR.sides_of(pb, X), activation=act, weight_tying=tying), want)


def test_two_one_sided_batches_give_the_same_sides(small):
    """sides_of on two one-sided batches addresses the same rows as on the two-sided batch."""
    pb, p1, p2 = SR.fixture_batch(sizes=(1, 3, 7, 7, 12), partner=(4, 2, 1, 0, 3))
    X = torch.randn(pb.n_rows, D, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    a1, a2 = SR.sides_of(pb, X)
    b1, b2 = SR.sides_of(p1, X[:p1.n_rows], X[p1.n_rows:], p2)
    p = _draw(O.init_global, 4, D, OUT)
    for got, want in zip(SR.global_(p, b1, b2), SR.global_(p, a1, a2)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("o", [1, 2, 7, 8, 24])
def test_rowcorr_equals_the_oracles_fft_form(o):
    g = torch.Generator().manual_seed(o)
    row0, nrows = torch.tensor([5, 0]), torch.tensor([3, 4])             # rows 4 and 8.. belong to no molecule
    a = torch.randn(10, o, generator=g, dtype=torch.float64)
    q = torch.randn(2, o, generator=g, dtype=torch.float64)
    e = SR.rowcorr(a, q, row0, nrows)
    rm = SR.row_mol_of(row0, nrows, 10)
    assert rm.tolist() == [1, 1, 1, 1, -1, 0, 0, 0, -1, -1]
    on = rm >= 0
    want = O.circular_correlation(a[on], q[rm[on]])
    assert (e[on] - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
    assert float(e[~on].abs().max()) == 0.0


def test_rowcorr_rotation_direction():
    """e[k] = sum_t a[t] q[(t + k) mod o]: a = e_1 reads q rotated LEFT by one."""
    a = torch.tensor([[0.0, 1.0, 0.0, 0.0]], dtype=torch.float64)
    q = torch.tensor([[10.0, 20.0, 30.0, 40.0]], dtype=torch.float64)
    e = SR.rowcorr(a, q, torch.tensor([0]), torch.tensor([1]))
    assert e.tolist() == [[20.0, 30.0, 40.0, 10.0]]


def test_segsoftmax_known_answer_with_multiplicities():
    """Scores (0, ln 2, ln 3) with multiplicities (1, 1, 4): the denominator is 1 + 2 + 4 * 3 = 15, and alpha is
    exp(s) / 15 on EVERY row -- the multiplicity does not scale a row's own alpha.  A second molecule has a pad row of
    multiplicity 0 with a huge score: alpha 0 there, and the score stays out of the max and the sum.  Row 3 is dead."""
    ln = np.log
    s = torch.tensor([0.0, ln(2.0), ln(3.0), 7.0, ln(5.0), ln(3.0), 900.0], dtype=torch.float64, requires_grad=True)
    w = torch.tensor([1.0, 1.0, 4.0, 0.0, 1.0, 1.0, 0.0])
    row0, nrows = torch.tensor([0, 4]), torch.tensor([3, 3])
    alpha = SR.segsoftmax(s, w, row0, nrows)
    want = torch.tensor([1 / 15, 2 / 15, 3 / 15, 0.0, 5 / 8, 3 / 8, 0.0], dtype=torch.float64)
    assert torch.allclose(alpha, want, atol=1e-15, rtol=0)
    # ds_k = alpha_k (dalpha_k - w_k sum_j alpha_j dalpha_j), with dalpha = (1, 0, 0) on the first molecule
    alpha[0].backward()
    ds = torch.tensor([(1 / 15) * (1 - 1 / 15), (2 / 15) * (-1 / 15), (3 / 15) * (-4 / 15)], dtype=torch.float64)
    assert torch.allclose(s.grad[:3], ds, atol=1e-14, rtol=0)
    assert s.grad[3:].abs().max().item() == 0.0


def test_segpool_known_answer_with_a_per_row_weight():
    """ca == 1: out[m, c] = sum_r w[r] A[r, 0] Y[r, c].  Row 2 belongs to no molecule."""
    A = torch.tensor([[2.0], [3.0], [100.0], [0.5], [1.0]], dtype=torch.float64)
    Y = torch.tensor([[1.0, 10.0], [2.0, 20.0], [7.0, 7.0], [4.0, 40.0], [8.0, 80.0]], dtype=torch.float64)
    w = torch.tensor([1.0, 5.0, 9.0, 1.0, 0.0])
    out = SR.segpool(A, Y, w, torch.tensor([3, 0]), torch.tensor([2, 2]))
    assert out.tolist() == [[2.0, 20.0], [2.0 + 30.0, 20.0 + 300.0]]
    G = torch.tensor([[1.0, 0.5], [1.0, 1.0], [1.0, 1.0], [2.0, 1.0], [1.0, 1.0]], dtype=torch.float64)     # ca == o
    out = SR.segpool(G, Y, w, torch.tensor([3, 0]), torch.tensor([2, 2]))
    assert out.tolist() == [[8.0, 40.0], [1.0 + 10.0, 5.0 + 100.0]]


def test_rowdot_and_rowbcast_leave_dead_rows_zero():
    rm = torch.tensor([1, -1, 0])
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=torch.float64)
    u = torch.tensor([[1.0, 1.0], [2.0, -1.0]], dtype=torch.float64)
    assert SR.rowdot(x, u, None, rm).tolist() == [0.0, 0.0, 11.0]
    assert SR.rowdot(x, u, torch.tensor([0.5, 0.25], dtype=torch.float64), rm).tolist() == [0.25, 0.0, 11.5]
    assert SR.rowbcast(u, rm).tolist() == [[2.0, -1.0], [0.0, 0.0], [1.0, 1.0]]


def test_shared_batch_has_the_shapes_the_gpu_tests_rely_on():
    pb, p1, p2 = SR.fixture_batch()
    nr = sorted(set(pb.mol_nrows.tolist()))
    assert nr == [2, 3, 4, 5, 6, 64, 65, 66, 128, 131, 301] and {n % 4 for n in nr} == {0, 1, 2, 3}
    assert int((pb.row_mol < 0).sum()) > 0 and pb.oversized
    n1 = np.array(SR.SIZES); n2 = n1[list(SR.PARTNER)]
    assert (n1 == n2).sum() >= 3 and (n1 != n2).sum() >= 3
    pads = pb.mol_row0.long() + pb.mol_nrows.long() - 1
    assert (pb.row_w[pads] == 0).sum() == 2 and (pb.row_w[pads] > 1).sum() == 20
    # the one-sided batches hold the rows of the two-sided one, side by side
    assert torch.equal(p1.mol_row0, pb.mol_row0[:11]) and torch.equal(p2.mol_row0 + p1.n_rows, pb.mol_row0[11:])
    assert torch.equal(torch.cat((p1.row_w, p2.row_w)), pb.row_w)


def test_relu_case_clears_the_kink_band():
    seed = SR.RELU_SEED
    lo, hi = SR.relu_case_margin(seed)
    print(f"[kink] neural relu seed {seed}: min |pre| {lo:.3e}, max |pre| {hi:.3e}, band {SR.KINK_FACTOR * 1e-4 * hi:.3e}")
    assert lo >= SR.KINK_FACTOR * 1e-4 * hi, {s: SR.relu_case_margin(s) for s in SR.RELU_SEEDS}
    # the case is not degenerate: both branches of the relu are taken, and some columns take both
    p, X = SR.relu_case_inputs(seed)
    p = {k: v.requires_grad_() for k, v in p.items()}
    pres, en = [], []
    c1, c2 = SR.neural(p, *SR.sides_of(SR.fixture_batch()[0], X), activation="relu", weight_tying=False, pre_out=pres,
                       energy_out=en)
    pos = torch.cat([t.reshape(-1, SR.RELU_CASE["out_dim"]) for t in pres]) > 0
    frac = pos.double().mean(0)
    assert (frac > 0.5).sum() == (frac < 0.5).sum() and int(((frac > 0) & (frac < 1)).sum()) >= 4
    # ... and the gate is off its flat ends on every row, so that the dot product in front of it, the relu of the query
    # and the gate's share of the parameter gradients are compared as numbers and not as 0 against 0
    en = [e.detach() for e in en]
    gate = torch.sigmoid(torch.cat(en))
    slope = gate * (1 - gate)
    print(f"[gate] doc . context {torch.cat(en).min():.2f} .. {torch.cat(en).max():.2f}, sigmoid' min {slope.min():.3e}")
    assert slope.median() > 1e-2 and slope.min() > 1e-3
    # the gradient that reaches the parameters THROUGH the gate alone (the pooled doc held constant)
    total = torch.autograd.grad(c1.sum() + c2.sum(), [p[k] for k in sorted(p)])
    for k, g in zip(sorted(p), total):
        assert g.abs().max() > 0, k
    pq = {k: v.detach().clone().requires_grad_() for k, v in p.items()}
    en3 = []
    SR.neural(pq, *SR.sides_of(SR.fixture_batch()[0], X), activation="relu", weight_tying=False, energy_out=en3)
    through = torch.autograd.grad(torch.sigmoid(torch.cat(en3)).sum(), [pq[k] for k in sorted(pq)])
    for k, g, tot in zip(sorted(pq), through, total):
        assert g.abs().max() > 1e-3 * tot.abs().max(), k
