"""Pins tests/link_ref.py, the float64 restatement of the pair features and its element-wise float32 error bound: known
answers, S against the sum of |terms| written out, the float32 torch restatement inside the bound at every shape of the
GPU tests, and four deliberately wrong restatements outside it -- the evidence that tests/test_gpu_link_edges.py would see
a subtle error in a kernel.  No GPU."""
import itertools

import pytest
import torch

import link_ref as LR

CASES = [(k, s) for k in LR.KINDS for s in LR.SHAPES[k]]


def _worst(got, want, bound):
    return {k: LR.ratio(got[k], want[k], bound[k]) for k in want}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(kind, shape, **kw):
        key = (kind, shape, tuple(sorted(kw.items())))
        if key not in cache:
            x1, x2, p, cy = LR.make_inputs(kind, shape, **kw)
            cache[key] = (x1, x2, p, cy) + LR.reference(kind, x1, x2, p, cy)
        return cache[key]
    return get


def test_hole_is_the_direct_circular_sum_and_rotates_left():
    a = torch.tensor([[0.0, 1.0, 0.0, 0.0]], dtype=torch.float64)
    q = torch.tensor([[10.0, 20.0, 30.0, 40.0]], dtype=torch.float64)
    assert LR.hole(a, q).tolist() == [[20.0, 30.0, 40.0, 10.0]]
    g = torch.Generator().manual_seed(0)
    x1, x2 = torch.randn(3, 7, generator=g, dtype=torch.float64), torch.randn(3, 7, generator=g, dtype=torch.float64)
    want = torch.zeros(3, 7, dtype=torch.float64)
    for k, i in itertools.product(range(7), range(7)):
        want[:, k] += x1[:, i] * x2[:, (i + k) % 7]
    assert torch.allclose(LR.hole(x1, x2), want, atol=1e-14, rtol=0)


def test_known_answers_of_sym_distmult_and_ntn():
    x1 = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    x2 = torch.tensor([[3.0, -4.0]], dtype=torch.float64)
    assert LR.sym(x1, x2).tolist() == [[4.0, -2.0, 3.0, -8.0]]
    W = torch.tensor([[1.0, 0.5], [0.0, 2.0], [-1.0, 0.0]], dtype=torch.float64)                 # [K = 3 x d = 2]
    assert LR.distmult(x1, x2, dict(W=W)).tolist() == [[3.0 - 4.0, -16.0, -3.0]]
    Wn = torch.zeros(2, 2, 1, dtype=torch.float64)
    Wn[0, 1, 0], Wn[1, 0, 0] = 1.0, 10.0                                                          # x1[0] x2[1] + 10 x1[1] x2[0]
    p = dict(W=Wn, V1=torch.tensor([[1.0], [1.0]], dtype=torch.float64), V2=torch.tensor([[0.0], [0.5]], dtype=torch.float64),
             b=torch.tensor([100.0], dtype=torch.float64))
    assert LR.ntn(x1, x2, p).tolist() == [[-4.0 + 60.0 + 3.0 - 2.0 + 100.0]]
    assert LR.ntn(x1, x2, dict(W=Wn, V1=None, V2=p["V2"], b=None)).tolist() == [[-4.0 + 60.0 - 2.0]]


def test_S_is_the_sum_of_the_absolute_terms():
    """NTN at a size where every term can be written out: y's and dW's S of ``reference`` against the explicit sums."""
    x1, x2, p, cy = LR.make_inputs("ntn", (3, 2, 3, 2))
    want, bound = LR.reference("ntn", x1, x2, p, cy)
    a, c, W, V1, V2, b, g = (t.double().abs() for t in (x1, x2, p["W"], p["V1"], p["V2"], p["b"], cy))
    Sy = torch.zeros(3, 2, dtype=torch.float64)
    SW = torch.zeros(2, 3, 2, dtype=torch.float64)
    for bi, o in itertools.product(range(3), range(2)):
        Sy[bi, o] = b[o] + sum(a[bi, i] * V1[i, o] for i in range(2)) + sum(c[bi, j] * V2[j, o] for j in range(3)) \
            + sum(a[bi, i] * W[i, j, o] * c[bi, j] for i in range(2) for j in range(3))
        for i, j in itertools.product(range(2), range(3)):
            SW[i, j, o] += a[bi, i] * c[bi, j] * g[bi, o]
    r = LR.rounds("ntn", x1, x2, p)
    assert r == dict(y=2 + 3 + 2 + 3, dx1=2 + 3 + 2, dx2=2 + 2 + 2, dW=5, dV1=4, dV2=4, db=3)
    assert torch.allclose(bound["y"], r["y"] * LR.U * Sy, rtol=1e-13, atol=0)
    assert torch.allclose(bound["dW"], r["dW"] * LR.U * SW, rtol=1e-13, atol=0)
    assert LR.rounds("hole", torch.zeros(2, 20), torch.zeros(2, 20), {})["y"] == 21


@pytest.mark.parametrize("kind,shape", CASES)
def test_float32_restatement_stays_inside_the_bound(refs, kind, shape):
    x1, x2, p, cy, want, bound = refs(kind, shape)
    got = LR.evaluate(LR.FEATURE[kind], x1, x2, p, cy, dtype=torch.float32)
    worst = _worst(got, want, bound)
    print(f"[bound] {kind} {shape}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert set(got) == set(want) and all(v <= 1.0 for v in worst.values()), worst
    # not vacuous: float32 does differ from float64 somewhere (the 1 x 1 products of two floats are exact in neither)
    assert max(worst.values()) > 0.0


@pytest.mark.parametrize("V1,V2,b", [(True, True, True), (True, False, False), (False, True, True), (False, False, False)])
def test_float32_ntn_without_optional_parameters_stays_inside_the_bound(refs, V1, V2, b):
    x1, x2, p, cy, want, bound = refs("ntn", (33, 16, 16, 8), V1=V1, V2=V2, b=b)
    assert set(want) == {"y", "dx1", "dx2", "dW"} | ({"dV1"} if V1 else set()) | ({"dV2"} if V2 else set()) | ({"db"} if b else set())
    got = LR.evaluate(LR.ntn, x1, x2, p, cy, dtype=torch.float32)
    worst = _worst(got, want, bound)
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- deliberately wrong restatements: each must leave the bound on at least one element ----
def test_hole_with_a_wrong_wrap_in_the_last_column_is_seen(refs):
    shape = (2, 256)
    x1, x2, p, cy, want, bound = refs("hole", shape)
    d = shape[1]
    rot = LR.rotation(d)
    rot[d - 1] = (torch.arange(d) + (d - 1)) % (d - 1)
    got = LR.evaluate(lambda a, c, q: LR.hole(a, c, rot=rot), x1, x2, p, cy, dtype=torch.float32)
    worst = _worst(got, want, bound)
    assert worst["y"] > 1.0, worst
    # ... in that column alone
    assert LR.ratio(got["y"][:, :d - 1], want["y"][:, :d - 1], bound["y"][:, :d - 1]) <= 1.0
    assert worst["dx2"] > 1.0                               # and in the gradient that reads x2 through the same table


def test_ntn_without_V2_is_seen(refs):
    x1, x2, p, cy, want, bound = refs("ntn", (70, 8, 24, 5))
    got = LR.evaluate(LR.ntn, x1, x2, dict(p, V2=None), cy, dtype=torch.float32)
    assert LR.ratio(got["y"], want["y"], bound["y"]) > 1.0
    for k in ("dx1", "dW", "dV1", "db"):                     # V2 enters y and dx2 alone
        assert LR.ratio(got[k], want[k], bound[k]) <= 1.0, k
    assert LR.ratio(got["dx2"], want["dx2"], bound["dx2"]) > 1.0


def test_ntn_dW_without_the_last_row_of_the_batch_is_seen(refs):
    x1, x2, p, cy, want, bound = refs("ntn", (33, 16, 16, 8))
    got = LR.evaluate(LR.ntn, x1[:-1], x2[:-1], p, cy[:-1], dtype=torch.float32)
    assert LR.ratio(got["dW"], want["dW"], bound["dW"]) > 1.0
    full = LR.evaluate(LR.ntn, x1, x2, p, cy, dtype=torch.float32)
    assert LR.ratio(full["dW"], want["dW"], bound["dW"]) <= 1.0


def test_distmult_with_one_weight_of_the_last_column_zeroed_is_seen(refs):
    x1, x2, p, cy, want, bound = refs("distmult", (17, 1024, 8))
    W = p["W"].clone()
    W[5, -1] = 0.0
    got = LR.evaluate(LR.distmult, x1, x2, dict(W=W), cy, dtype=torch.float32)
    assert LR.ratio(got["y"], want["y"], bound["y"]) > 1.0
    assert LR.ratio(got["y"][:, :5], want["y"][:, :5], bound["y"][:, :5]) <= 1.0         # ... in output column 5 alone


def test_ratio_counts_a_wrong_zero_and_a_non_finite_value():
    w = torch.tensor([1.0, 0.0], dtype=torch.float64)
    bnd = torch.tensor([1e-7, 0.0], dtype=torch.float64)
    assert LR.ratio(w.clone(), w, bnd) == 0.0
    assert LR.ratio(torch.tensor([1.0, 1e-30], dtype=torch.float64), w, bnd) == float("inf")
    assert LR.ratio(torch.tensor([float("nan"), 0.0], dtype=torch.float64), w, bnd) == float("inf")
    assert abs(LR.ratio(torch.tensor([1.0 + 5e-8, 0.0], dtype=torch.float64), w, bnd) - 0.5) < 1e-6
