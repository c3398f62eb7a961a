"""The pair-feature kernels of csrc/bmp_link.hip ALONE (bmp.link.PairFeatFn, no MLP tail behind them) against the float64
restatement of tests/link_ref.py, value and every gradient ELEMENT-WISE inside r * 2**-24 * S, at the smallest shape at
which each path of the kernels exists (link_ref.SHAPES); the refusals past PF_MAXD, PF_MAXD / 4 and PF_MAXK; NTN without its
optional parameters; every call twice, bit for bit (the kernels promise fixed summation orders).  Then the link predictors
whose relu-MLP tail lies outside the MLP kernels (bmp.mlp.kernels_take): the feature stays on its kernel, the tail takes the
plain torch ops."""
import pytest
import torch

import link_ref as LR
from parity_util import close, close_bound

pytestmark = pytest.mark.gpu

NAMES = ("dx1", "dx2", "dW", "dV1", "dV2", "db")


def _run(kind, x1, x2, p, cy):
    """{'y', 'dx1', ...} of PairFeatFn.apply on cuda:0, gradients against ``cy``."""
    from bmp.link import PairFeatFn
    dev = torch.device("cuda:0")
    a, c = (t.to(dev).requires_grad_() for t in (x1, x2))
    prm = [None if p.get(k) is None else p[k].to(dev).requires_grad_() for k in LR.PARAMS]
    K = 0 if p.get("W") is None else p["W"].shape[0 if kind == "distmult" else 2]
    y = PairFeatFn.apply(LR.KIND_ID[kind], K, a, c, *prm)
    leaves = [a, c] + [t for t in prm if t is not None]
    grads = torch.autograd.grad(y, leaves, cy.to(dev))
    out = dict(y=y.detach(), dx1=grads[0], dx2=grads[1])
    out.update({"d" + k: g for k, g in zip([k for k, t in zip(LR.PARAMS, prm) if t is not None], grads[2:])})
    return out


def _check(kind, shape, **kw):
    x1, x2, p, cy = LR.make_inputs(kind, shape, **kw)
    want, bound = LR.reference(kind, x1, x2, p, cy)
    got = _run(kind, x1, x2, p, cy)
    assert set(got) == set(want)
    again = _run(kind, x1, x2, p, cy)
    for k in want:
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
    for k in want:
        close_bound(got[k], want[k], bound[k], f"{kind} {shape} {k}")


@pytest.mark.parametrize("shape", LR.SHAPES["sym"])
def test_sym(shape):
    _check("sym", shape)


@pytest.mark.parametrize("shape", LR.SHAPES["hole"])
def test_hole(shape):
    _check("hole", shape)


@pytest.mark.parametrize("shape", LR.SHAPES["distmult"])
def test_distmult(shape):
    _check("distmult", shape)


@pytest.mark.parametrize("shape", LR.SHAPES["ntn"])
def test_ntn(shape):
    _check("ntn", shape)


@pytest.mark.parametrize("V1,V2,b", [(True, True, True), (True, False, False), (False, True, True), (False, False, False)])
def test_ntn_optional_parameters(V1, V2, b):
    """V1, V2 and b are optional in the C ABI: the values without them, and no gradient written for an absent one."""
    from bmp.link import PairFeatFn
    shape = (33, 16, 16, 8)
    _check("ntn", shape, V1=V1, V2=V2, b=b)
    # the Function's backward itself, on a stand-in context: None in the slot of every absent parameter
    x1, x2, p, cy = LR.make_inputs("ntn", shape, V1=V1, V2=V2, b=b)
    dev = torch.device("cuda:0")

    class Ctx:
        def save_for_backward(self, *t):
            self.saved_tensors = t

    ctx = Ctx()
    prm = [None if p[k] is None else p[k].to(dev) for k in LR.PARAMS]
    y = PairFeatFn.forward(ctx, LR.KIND_ID["ntn"], 8, x1.to(dev), x2.to(dev), *prm)
    grads = PairFeatFn.backward(ctx, cy.to(dev))
    assert len(grads) == 8 and grads[0] is None and grads[1] is None
    for g, have in zip(grads[2:], (True, True, True, V1, V2, b)):
        assert (g is not None) == have
    ref = _run("ntn", x1, x2, p, cy)
    assert torch.equal(y, ref["y"])
    for g, k in zip(grads[2:], NAMES):
        if g is not None:
            assert torch.equal(g, ref[k]), k


@pytest.mark.parametrize("kind,shape", [(k, s) for k in LR.REFUSED for s in LR.REFUSED[k]])
def test_shapes_past_the_limits_are_refused_before_a_launch(kind, shape):
    """Tensors of the right size for the refused shape: a refusal that did not happen could not read or write out of bounds.
    The argument check answers before any launch (-1000 - line: ValueError)."""
    from bmp.link import PairFeatFn
    dev = torch.device("cuda:0")
    x1, x2, p, _cy = LR.make_inputs(kind, shape)
    prm = [None if p.get(k) is None else p[k].to(dev) for k in LR.PARAMS]
    K = 0 if p.get("W") is None else p["W"].shape[0 if kind == "distmult" else 2]
    with pytest.raises(ValueError, match="bmp_pairfeat_fwd: argument check failed"):
        PairFeatFn.apply(LR.KIND_ID[kind], K, x1.to(dev), x2.to(dev), *prm)


# ---- link predictors whose tail the MLP kernels do not take ----
def _tail64(h, Ws, bs):
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = torch.relu(h @ W.t() + b)
    return h @ Ws[-1].t() + bs[-1]


@pytest.mark.parametrize("name", ["hole-1024", "symmlp-512", "ntn-wide", "ntn-deep"])
def test_link_predictors_with_a_tail_outside_the_mlp_kernels(name):
    """Constructions that bmp_mlp_fwd refused with an argument-check error: the first layer's weights do not fit beside the
    launch's row buffers (1024 x 33 and 1024 x 33 floats > 24576), a hidden width above 64, five Linear layers.  Values and
    all gradients against float64, at the per-tensor tolerance of the link predictors' composite test (parity_util.close,
    1e-4): relu makes the element-wise polynomial bound inapplicable behind the feature."""
    from bmp.link import HolE, NTN, SymMLP
    from bmp.mlp import kernels_take
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    B = 9
    if name == "hole-1024":
        lp, kind, d1, d2 = HolE(1, (32, 16), fp_dim=1024), "hole", 1024, 1024
        tail, width = list(lp.layers) + [lp.l_out], 1024
    elif name == "symmlp-512":
        lp, kind, d1, d2 = SymMLP(2, (32, 16), fp_dim=512), "sym", 512, 512
        tail, width = list(lp.layers) + [lp.l_out], 1024
    else:
        lp = NTN(16, 16, 1, hidden_dims=(128,) if name == "ntn-wide" else (16, 16, 16, 16))
        kind, d1, d2 = "ntn", 16, 16
        tail, width = list(lp.mlp_layers) + [lp.l_out], 8
    assert not kernels_take([width] + [l.out_size for l in tail])
    lp = lp.to(dev)
    with torch.no_grad():
        for l in tail:
            l.b.copy_(torch.randn_like(l.b) * 0.3)             # (the biases start at 0; the weights keep their LeCun draw)
    x1 = torch.randn(B, d1, device=dev, requires_grad=True)
    x2 = torch.randn(B, d2, device=dev, requires_grad=True)
    y = lp(x1, x2)
    cy = torch.randn_like(y)
    params = list(lp.parameters())
    got = torch.autograd.grad(y, [x1, x2] + params, cy)

    d = lambda t: t.detach().double().cpu().requires_grad_()
    a, c = d(x1), d(x2)
    Ws, bs = [d(l.W) for l in tail], [d(l.b) for l in tail]
    if kind == "ntn":
        E = lp.ntn_layer
        fp = dict(W=d(E.W), V1=d(E.V1), V2=d(E.V2), b=d(E.b))
    else:
        fp = {}
    y64 = _tail64(LR.FEATURE[kind](a, c, fp), Ws, bs)
    by_id = {id(l.W): w for l, w in zip(tail, Ws)}
    by_id.update({id(l.b): b for l, b in zip(tail, bs)})
    if kind == "ntn":
        by_id.update({id(getattr(lp.ntn_layer, k)): fp[k] for k in fp})
    want = torch.autograd.grad(y64, [a, c] + [by_id[id(q)] for q in params], cy.double().cpu())
    close(y, y64, f"{name} y")
    names = ["dx1", "dx2"] + [n for n, _ in lp.named_parameters()]
    for n, g, w in zip(names, got, want):
        close(g, w, f"{name} grad {n}")
