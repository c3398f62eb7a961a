"""Link-predictor tail on the device (bmp_mlp_* / bmp_sce_*) against the plain fp32 torch ops of the same
functions (models/mlp.py:20-45; chainer sigmoid_cross_entropy, train_ddi_modify.py:285)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref_mlp(mlp, x):
    h = x
    for l in mlp.layers:
        h = torch.relu(torch.nn.functional.linear(h, l.W, l.b))
    return torch.nn.functional.linear(h, mlp.l_out.W, mlp.l_out.b)


def _ref_sce(y, t):
    mask = t != -1
    loss = torch.nn.functional.softplus(y) - t.to(y.dtype) * y
    return torch.where(mask, loss, torch.zeros_like(loss)).sum() / mask.sum().clamp(min=1)


@pytest.mark.parametrize("B,o,hidden,C", [(1024, 128, (32, 16), 1), (37, 20, (32, 16), 37), (5, 8, (), 3), (130, 64, (64, 64, 16), 2)])
def test_mlp_and_loss_match_torch(B, o, hidden, C):
    from bmp.mlp import MLP, sigmoid_cross_entropy
    dev = torch.device("cuda:0")
    torch.manual_seed(B + C)
    mlp = MLP(C, hidden, in_dim=2 * o).to(dev)
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    g1 = torch.randn(B, o, device=dev, requires_grad=True)
    g2 = torch.randn(B, o, device=dev, requires_grad=True)
    t = torch.randint(-1, 2, (B, C), device=dev, dtype=torch.int32)
    y = mlp(g1, g2)
    loss = sigmoid_cross_entropy(y, t)
    loss.backward()
    got = [y.detach().clone(), loss.detach().clone(), g1.grad.clone(), g2.grad.clone()] + [p.grad.clone() for p in mlp.parameters()]
    for p in list(mlp.parameters()) + [g1, g2]:
        p.grad = None
    yr = _ref_mlp(mlp, torch.cat((g1, g2), dim=1))
    lr = _ref_sce(yr, t)
    lr.backward()
    want = [yr.detach(), lr.detach(), g1.grad, g2.grad] + [p.grad for p in mlp.parameters()]
    for a, b in zip(got, want):
        scale = max(b.abs().max().item(), 1e-6)
        assert (a - b).abs().max().item() <= 1e-5 * scale + 1e-7, ((a - b).abs().max().item(), scale)


def test_loss_ignores_minus_one_and_empty_mask():
    from bmp.mlp import sigmoid_cross_entropy
    dev = torch.device("cuda:0")
    y = torch.tensor([[0.5], [-2.0], [3.0]], device=dev, requires_grad=True)
    t = torch.tensor([[1], [-1], [0]], device=dev, dtype=torch.int32)
    loss = sigmoid_cross_entropy(y, t)
    loss.backward()
    ref = (torch.nn.functional.softplus(torch.tensor(0.5)) - 0.5 + torch.nn.functional.softplus(torch.tensor(3.0))) / 2
    assert abs(loss.item() - ref.item()) < 1e-6
    assert y.grad[1].item() == 0.0
    y2 = torch.zeros(2, 1, device=dev, requires_grad=True)
    l2 = sigmoid_cross_entropy(y2, torch.full((2, 1), -1, device=dev, dtype=torch.int32))
    l2.backward()
    assert l2.item() == 0.0 and float(y2.grad.abs().sum()) == 0.0


@pytest.mark.parametrize("B,o,hidden,C,gscale", [(1024, 128, (32, 16), 1, 1.0), (37, 20, (32, 16), 37, 1.0), (5, 8, (), 3, -2.5),
                                                  (130, 64, (64, 64, 16), 2, 0.125), (1024, 256, (32, 16), 37, 1.0)])
def test_link_predictor_and_loss_in_one_launch_equal_the_separate_launches(B, o, hidden, C, gscale):
    """MLP.forward_loss (bmp_mlp_sce_fwdbwd + bmp_mlp_bwd_w: the reference's Classifier around the link predictor as one launch
    each way) against MLP.forward + sigmoid_cross_entropy: the same logits, input and parameter gradients bit for bit (the same
    sums in the same order; the scale arrives as a power of two or one), the loss to rounding (its numerators meet in another
    order); and both against the plain torch ops."""
    from bmp.mlp import MLP, sigmoid_cross_entropy
    dev = torch.device("cuda:0")
    torch.manual_seed(B + C)
    mlp = MLP(C, hidden, in_dim=2 * o).to(dev)
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    g1 = torch.randn(B, o, device=dev, requires_grad=True)
    g2 = torch.randn(B, o, device=dev, requires_grad=True)
    t = torch.randint(-1, 2, (B, C), device=dev, dtype=torch.int32)
    res = []
    for fused in (True, False):
        for p in list(mlp.parameters()) + [g1, g2]:
            p.grad = None
        if fused:
            loss, y = mlp.forward_loss(g1, g2, t)
            assert not y.requires_grad
        else:
            y = mlp(g1, g2)
            loss = sigmoid_cross_entropy(y, t)
        (loss * gscale).backward()
        res.append([y.detach().clone(), loss.detach().clone(), g1.grad.clone(), g2.grad.clone()] + [p.grad.clone() for p in mlp.parameters()])
    exact = gscale in (1.0, 0.125)
    for k, (a, b) in enumerate(zip(*res)):
        scale = max(b.abs().max().item(), 1e-6)
        if k == 1 or not exact:
            assert (a - b).abs().max().item() <= 2e-6 * scale, (k, (a - b).abs().max().item(), scale)
        else:
            assert torch.equal(a, b), (k, (a - b).abs().max().item())
    for p in list(mlp.parameters()) + [g1, g2]:
        p.grad = None
    yr = _ref_mlp(mlp, torch.cat((g1, g2), dim=1))
    lr = _ref_sce(yr, t)
    (lr * gscale).backward()
    want = [yr.detach(), lr.detach(), g1.grad, g2.grad] + [p.grad for p in mlp.parameters()]
    for a, b in zip(res[0], want):
        scale = max(b.abs().max().item(), 1e-6)
        assert (a - b).abs().max().item() <= 1e-5 * scale + 1e-7, ((a - b).abs().max().item(), scale)
    # a second pass right behind the first: the launch leaves its ticket word at zero
    loss2, y2 = mlp.forward_loss(g1, g2, t)
    assert torch.equal(loss2, res[0][1]) and torch.equal(y2, res[0][0])


def test_loss_of_a_batch_without_counted_labels_is_zero():
    from bmp.mlp import MLP
    dev = torch.device("cuda:0")
    mlp = MLP(2, (32, 16), in_dim=16).to(dev)
    g1 = torch.randn(9, 8, device=dev, requires_grad=True)
    g2 = torch.randn(9, 8, device=dev, requires_grad=True)
    loss, _y = mlp.forward_loss(g1, g2, torch.full((9, 2), -1, device=dev, dtype=torch.int32))
    loss.backward()
    assert loss.item() == 0.0 and float(g1.grad.abs().sum()) == 0.0 and all(float(p.grad.abs().sum()) == 0.0 for p in mlp.parameters())


def test_classifier_form_of_the_pair_predictor_equals_forward_plus_loss():
    """GraphConvPredictorForPair.forward_loss / FlatAdam.functional_loss (the reference's Classifier call, train_ddi_modify.py:
    284-286) against functional_forward + model.loss on the same batch: the flat gradient bit for bit, the loss to rounding;
    with and without a co-attention, single- and multi-label."""
    import numpy as np
    from bmp import packed, synth
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    dev = torch.device("cuda:0")
    store = synth.make_store(40, seed=3, n_lo=4, n_hi=40, n_mean=16)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev)
    rs = np.random.RandomState(1)
    i1, i2 = rs.randint(0, 40, 96), rs.randint(0, 40, 96)
    for attn, C in (("nie", 1), (None, 5)):
        lab = rs.randint(-1, 2, (96, C)).astype(np.int32)
        pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
        torch.manual_seed(0)
        model = build_pair_predictor(hidden_dim=64, out_dim=64, n_layers=2, attn=attn, head=4, class_num=C).to(dev)
        opt = FlatAdam(model, alpha=1e-3)
        y = opt.functional_forward(pb)
        l0 = model.loss(y, t)
        l0.backward(); opt.collect_grads()
        g0 = opt.grad.clone()
        l1 = opt.functional_loss(pb, t=t)
        l1.backward(); opt.collect_grads()
        assert torch.equal(model.y, y)
        assert abs(l0.item() - l1.item()) <= 2e-6 * abs(l0.item())
        assert torch.equal(opt.grad, g0), (attn, (opt.grad - g0).abs().max().item())
        # a factor on the loss (it reaches the pair kernels as a device scalar), and something else added to the molecule
        # vectors' gradients on the way back (the factor then goes on the head's share alone)
        for extra in (False, True):
            outs = []
            for fused in (False, True):
                if fused:
                    l = opt.functional_loss(pb, t=t)
                else:
                    l = model.loss(opt.functional_forward(pb), t)
                tot = l * 0.3 + (0.01 * (model.g1.sum() + model.g2.square().sum()) if extra else 0.0)
                tot.backward(); opt.collect_grads()
                outs.append(opt.grad.clone())
            scale = outs[0].abs().max().item()
            assert (outs[0] - outs[1]).abs().max().item() <= 3e-6 * scale, (attn, extra, (outs[0] - outs[1]).abs().max().item(), scale)


# ------------------------------------------------------------------------------------------------ the limits
# The tail and the head at MLP_FR = MLP_BR = 8 rows, MLP_MAXW = 64, one and four layers, a single input block, blocks of
# unequal width, and the LDS edges of bmp_mlp_fwd (in * (w1 + 1) <= 24576 floats beside 64 KB of row buffers) and of
# bmp_mlp_sce_fwdbwd (28672 floats of weights beside 48 KB).  Reference: the float64 restatement on the CPU; tolerance: this
# file's 1e-5 of the tensor's maximum (relu rules out an element-wise polynomial bound), recorded through parity_util.close.
def _ref_sce64(y, t):
    """mean over t != -1 of softplus(y) - t y, softplus as logaddexp(0, y): no threshold, accurate in float64 at any y, and
    smooth at y = 0 (its gradient is sigmoid(y) there too, which max(y, 0) + log1p(exp(-|y|)) does not give autograd)."""
    mask = t != -1
    loss = torch.logaddexp(torch.zeros_like(y), y) - t.to(y.dtype) * y
    return torch.where(mask, loss, torch.zeros_like(loss)).sum() / mask.sum().clamp(min=1)


def _ref64(mlp, x1, x2, t, gscale=1.0):
    """[logits, loss, dx1, (dx2,) parameter gradients...] in float64 on the CPU."""
    d = lambda v: v.detach().double().cpu().requires_grad_()
    a = d(x1)
    c = None if x2 is None else d(x2)
    prm = [d(p) for p in mlp.parameters()]
    by = {id(p): q for p, q in zip(mlp.parameters(), prm)}
    h = a if c is None else torch.cat((a, c), dim=1)
    for l in mlp.layers:
        h = torch.relu(h @ by[id(l.W)].t() + by[id(l.b)])
    y = h @ by[id(mlp.l_out.W)].t() + by[id(mlp.l_out.b)]
    loss = _ref_sce64(y, t.cpu())
    ins = [a] + ([] if c is None else [c])
    return [y.detach(), loss.detach()] + list(torch.autograd.grad(loss * gscale, ins + prm))


def _both_ways(B, d1, d2, hidden, C, kernel, head):
    """MLP.forward + sigmoid_cross_entropy, and MLP.forward_loss, against float64.  ``kernel`` / ``head``: whether the shape
    is one the MLP kernels / the one-launch head take -- the test also pins WHICH path answered."""
    from bmp.mlp import MLP, sigmoid_cross_entropy
    from parity_util import close
    dev = torch.device("cuda:0")
    torch.manual_seed(1000 * B + d1 + d2 + C)
    mlp = MLP(C, hidden, in_dim=d1 + d2).to(dev)
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    x1 = torch.randn(B, d1, device=dev, requires_grad=True)
    x2 = torch.randn(B, d2, device=dev, requires_grad=True) if d2 else None
    t = torch.randint(-1, 2, (B, C), device=dev, dtype=torch.int32)
    t[0, 0] = 1                                               # at least one label counts
    want = _ref64(mlp, x1, x2, t)
    ins = [x1] + ([] if x2 is None else [x2])
    names = ["y", "loss", "dx1"] + ([] if x2 is None else ["dx2"]) + [n for n, _ in mlp.named_parameters()]
    assert mlp._kernel_ok() == kernel and mlp.plannable() == kernel and mlp._kernel_ok(head=True) == head
    for fused in (False, True):
        if fused:
            loss, y = mlp.forward_loss(x1, x2, t)
            assert (type(loss.grad_fn).__name__ == "MLPLossFnBackward") == head
        else:
            y = mlp(x1, x2)
            loss = sigmoid_cross_entropy(y, t)
            assert (type(y.grad_fn).__name__ == "MLPFnBackward") == kernel
        got = [y.detach(), loss.detach()] + list(torch.autograd.grad(loss, ins + list(mlp.parameters())))
        for n, g, w in zip(names, got, want):
            close(g, w, f"{'head' if fused else 'tail'} {n}", tol=1e-5)


@pytest.mark.parametrize("B", [1, 7, 8, 9])
def test_rows_around_the_workgroup_of_eight(B):
    _both_ways(B, 8, 8, (32, 16), 3, True, True)


@pytest.mark.parametrize("d1,d2,hidden,C", [(24, 0, (32, 16), 3),            # a single input block: mlp(x)
                                            (5, 11, (32, 16), 3),            # blocks of unequal width
                                            (8, 8, (), 64),                  # one layer, MLP_MAXW logits
                                            (8, 8, (64, 64, 64), 64)])       # MLP_MAXL layers, every one MLP_MAXW wide
def test_input_forms_depth_and_width_limits(d1, d2, hidden, C):
    _both_ways(9, d1, d2, hidden, C, True, True)


@pytest.mark.parametrize("d,w1,kernel", [(512, 23, True),                    # 1024 x 24 = 24576 floats: the last that fits
                                         (384, 31, True),                    # 768 x 32 = 24576
                                         (512, 24, False)])                  # 1024 x 25: the plain ops, the same answers
def test_lds_edge_of_the_forward_launch(d, w1, kernel):
    _both_ways(9, d, d, (w1,), 2, kernel, kernel)


@pytest.mark.parametrize("hidden,C,head", [((63,), 64, True),                # 384 x 64 + 64 x 64 = 28672 floats = 160 KB - 48 KB
                                           ((63, 64), 1, False)])            # + 65: forward + sigmoid_cross_entropy's launches
def test_lds_edge_of_the_one_launch_head(hidden, C, head):
    _both_ways(9, 192, 192, hidden, C, True, head)


def test_first_layer_past_the_forward_launch_takes_the_plain_ops():
    """MLP(1, (64, 16), in_dim=512): 512 x 65 floats do not fit beside the forward launch's row buffers; the module answered
    with an argument-check error of bmp_mlp_fwd."""
    _both_ways(9, 256, 256, (64, 16), 1, False, False)


def test_loss_at_extreme_logits():
    """softplus(y) - t y and its gradient where expf(-y) overflows (y < -88.7) or vanishes, against labels 1, 0 and -1:
    finite, within this file's tolerance of float64, exact zeros where the label is -1.  sigmoid_cross_entropy on the logits;
    forward_loss through a one-layer MLP with W = I, b = 0, whose logits are a copy of its input."""
    from bmp.mlp import MLP, sigmoid_cross_entropy
    from parity_util import close
    dev = torch.device("cuda:0")
    vals = [0.0, 1e-4, -1e-4, 30.0, -30.0, 90.0, -90.0, 200.0, -200.0]
    y0 = torch.tensor(vals, dtype=torch.float32)[:, None].repeat(1, 3)
    t = torch.tensor([1, 0, -1], dtype=torch.int32)[None, :].repeat(len(vals), 1)
    y64 = y0.double().requires_grad_()
    l64 = _ref_sce64(y64, t)
    (dy64,) = torch.autograd.grad(l64, y64)
    assert torch.isfinite(l64) and torch.isfinite(dy64).all()

    y = y0.to(dev).requires_grad_()
    loss = sigmoid_cross_entropy(y, t.to(dev))
    (dy,) = torch.autograd.grad(loss, y)

    mlp = MLP(3, (), in_dim=3).to(dev)
    with torch.no_grad():
        mlp.l_out.W.copy_(torch.eye(3))
        mlp.l_out.b.zero_()
    x = y0.to(dev).requires_grad_()
    loss_h, y_h = mlp.forward_loss(x, None, t.to(dev))
    assert type(loss_h.grad_fn).__name__ == "MLPLossFnBackward" and torch.equal(y_h.cpu(), y0)
    (dx,) = torch.autograd.grad(loss_h, x)
    for tag, l, g in (("sce", loss, dy), ("head", loss_h, dx)):
        assert torch.isfinite(l) and torch.isfinite(g).all(), tag
        close(l, l64.detach(), f"{tag} loss", tol=1e-5)
        close(g, dy64, f"{tag} dy", tol=1e-5)
        assert float(g[:, 2].abs().max()) == 0.0, tag
