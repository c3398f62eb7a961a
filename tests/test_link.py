"""Link predictors NTN / DistMult / SymMLP / HolE (models/mlp.py:48-193).

CPU: known answers of the oracle restatement (the fft route of HolE.circular_correlation against the direct
circular sum; BilinearDiag against the explicit diagonal Bilinear; tiny hand-computed cases).
GPU: the HIP pair-feature kernels + MLP tail against the oracle, values and all gradients."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O


def test_oracle_circular_correlation_is_the_direct_sum():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(3, 7, generator=g, dtype=torch.float64)
    b = torch.randn(3, 7, generator=g, dtype=torch.float64)
    c = O.circular_correlation(a, b)
    want = torch.zeros_like(c)
    for k in range(7):
        for i in range(7):
            want[:, k] += a[:, i] * b[:, (i + k) % 7]
    assert torch.allclose(c, want, atol=1e-12)
    # known answer: correlating with a one-hot shifts
    e = torch.zeros(1, 7, dtype=torch.float64); e[0, 2] = 1.0
    assert torch.allclose(O.circular_correlation(e, b[:1]), torch.roll(b[:1], -2, dims=1), atol=1e-12)


def test_oracle_distmult_is_weighted_elementwise_product():
    dr = O._Draw(3, torch.float64, 0.1)
    O.init_link(dr, "mlp/", "distmult", 6, 2, (5,), feat_dim=4)
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn(4, 6, generator=g, dtype=torch.float64); x2 = torch.randn(4, 6, generator=g, dtype=torch.float64)
    feat = (x1 * x2) @ dr.p["mlp/dm_layer/W"].t()
    want = O.linear(torch.relu(O.linear(feat, dr.p["mlp/mlp_layers/0/W"], dr.p["mlp/mlp_layers/0/b"])),
                    dr.p["mlp/l_out/W"], dr.p["mlp/l_out/b"])
    assert torch.allclose(O.distmult_forward(dr.p, x1, x2, 1), want, atol=1e-12)


def test_oracle_symmlp_swaps():
    dr = O._Draw(4, torch.float64, 0.1)
    O.init_link(dr, "mlp/", "symmlp", 5, 3, (8, 4))
    g = torch.Generator().manual_seed(2)
    x1 = torch.randn(2, 5, generator=g, dtype=torch.float64); x2 = torch.randn(2, 5, generator=g, dtype=torch.float64)
    assert torch.allclose(O.symmlp_forward(dr.p, x1, x2, 2), O.symmlp_forward(dr.p, x2, x1, 2), atol=1e-14)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,fp,C,hidden", [("ntn", 32, 1, (16,)), ("ntn", 128, 3, (32, 16)), ("distmult", 64, 1, (16,)),
                                              ("symmlp", 48, 2, (32, 16)), ("hole", 128, 1, (32, 16)), ("hole", 20, 37, (16,))])
def test_link_predictors_match_oracle(kind, fp, C, hidden):
    from bmp.predictor import build_link_predictor
    from bmp.snapshot import load_param_dict, grad_dict
    dev = torch.device("cuda:0")
    dr = O._Draw(11, torch.float64, 0.1)
    O.init_link(dr, "", kind, fp, C, hidden)
    p = {k: v.requires_grad_() for k, v in dr.p.items()}
    B = 70
    g = torch.Generator().manual_seed(5)
    x1 = torch.randn(B, fp, generator=g, dtype=torch.float64, requires_grad=True)
    x2 = torch.randn(B, fp, generator=g, dtype=torch.float64, requires_grad=True)
    fwd = dict(ntn=O.ntn_forward, distmult=O.distmult_forward, symmlp=O.symmlp_forward, hole=O.hole_forward)[kind]
    y_ref = fwd(p, x1, x2, len(hidden), prefix="")
    cy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    (y_ref * cy).sum().backward()

    lp = build_link_predictor({"distmult": "dist-mult"}.get(kind, kind), fp, C, hidden).to(dev)
    load_param_dict(lp, p)
    a = x1.detach().float().to(dev).requires_grad_()
    b = x2.detach().float().to(dev).requires_grad_()
    y = lp(a, b)
    (y * cy.float().to(dev)).sum().backward()

    from parity_util import close
    close(y, y_ref, "y")
    close(a.grad, x1.grad, "dx1")
    close(b.grad, x2.grad, "dx2")
    for name, gr in grad_dict(lp).items():
        close(gr, p[name].grad, f"grad {name}")


def test_classifier_form_of_the_mlp_on_host_tensors_is_forward_plus_loss():
    """MLP.forward_loss (the reference's Classifier around the link predictor, train_ddi_modify.py:284-286) on host tensors
    takes the plain ops: the same loss and logits as forward + sigmoid_cross_entropy, labels of -1 left out."""
    import torch
    from bmp.mlp import MLP, sigmoid_cross_entropy
    torch.manual_seed(0)
    mlp = MLP(3, (32, 16), in_dim=24)
    g1, g2 = torch.randn(7, 12, requires_grad=True), torch.randn(7, 12, requires_grad=True)
    t = torch.randint(-1, 2, (7, 3), dtype=torch.int32)
    loss, y = mlp.forward_loss(g1, g2, t)
    y0 = mlp(g1, g2)
    assert torch.equal(y, y0) and torch.equal(loss, sigmoid_cross_entropy(y0, t))
    loss.backward()
    assert g1.grad is not None and torch.isfinite(g1.grad).all()


def test_mlp_kernel_predicate_arithmetic():
    """bmp.mlp.kernels_take: layers, widths, and the first layer's weights -- in * (w1 + 1) floats -- beside the 64 KB of row
    buffers of bmp_mlp_fwd in 160 KB of LDS, i.e. at most 24576 floats; head_kernel_takes: all weights within 28672 floats."""
    from bmp.mlp import head_kernel_takes, kernels_take
    assert kernels_take([1024, 23, 2]) and 1024 * 24 == 24576
    assert kernels_take([768, 31, 2]) and 768 * 32 == 24576
    assert not kernels_take([1024, 24, 2])
    assert not kernels_take([512, 64, 16, 1]) and 512 * 65 == 33280
    assert kernels_take([378, 64, 16, 1]) and not kernels_take([379, 64, 16, 1])
    assert kernels_take([1024, 1]) and not kernels_take([1025, 1])
    assert kernels_take([8, 64, 64, 64, 64]) and not kernels_take([8, 65, 1]) and not kernels_take([8, 16, 65])
    assert not kernels_take([8, 16, 16, 16, 16, 1]) and not kernels_take([8]) and not kernels_take([None, 16, 1])
    assert head_kernel_takes([384, 63, 64]) and 4 * (384 * 64 + 64 * 64) == 160 * 1024 - 49152
    assert kernels_take([384, 63, 64, 1]) and not head_kernel_takes([384, 63, 64, 1])
    assert not head_kernel_takes([1024, 24, 2])               # never wider than the tail's own kernels


def test_mlp_predicate_constants_are_the_kernels():
    import os
    import re
    from bmp import mlp as M
    src = open(os.path.join(os.path.dirname(M.__file__), "..", "csrc", "bmp_mlp.hip")).read()
    D = {k: int(v) for k, v in re.findall(r"#define (MLP_[A-Z]+) (\d+)", src)}
    assert (M._MAXL, M._MAXW, M._MAXIN) == (D["MLP_MAXL"], D["MLP_MAXW"], D["MLP_MAXIN"])
    assert M._FWD_ROWS_BYTES == 2 * D["MLP_FR"] * D["MLP_MAXIN"] * 4          # k_mlp_fwd: buf[2][MLP_FR][MLP_MAXIN]
    assert f"wt_bytes + {M._FWD_ROWS_BYTES} <= 160 * 1024" in src and f"wt_bytes + {M._SCE_ROWS_BYTES} <= 160 * 1024" in src
    assert M._LDS_BYTES == 160 * 1024
    # k_mlp_sce's row buffers: xin, hid, dcur and a few words, inside what it reserves
    static = 4 * D["MLP_BR"] * (D["MLP_MAXIN"] + (D["MLP_MAXL"] + 2) * D["MLP_MAXW"]) + 64
    assert static <= M._SCE_ROWS_BYTES


def test_mlp_that_does_not_fit_is_not_plannable_and_takes_the_plain_ops():
    """plannable() is the predicate of forward: a shape bmp_mlp_fwd would refuse is never planned, so the planned path
    records no launch that would be refused; link._tail asks the same predicate."""
    from bmp import link
    from bmp.mlp import MLP
    assert MLP(1, (32, 16), in_dim=256).plannable()
    for m in (MLP(1, (64, 16), in_dim=512), MLP(1, (32, 16), in_dim=1024), MLP(1, (128,), in_dim=16),
              MLP(1, (16, 16, 16, 16), in_dim=16)):
        assert not m.plannable() and not m._kernel_ok() and not m._kernel_ok(head=True)
    lazy = MLP(1, (32, 16))
    assert not lazy.plannable()
    lazy.materialize_input(128)
    assert lazy.plannable()
    # outside the predicate the tail of the link predictors is the plain ops (host tensors serve: no kernel is asked)
    torch.manual_seed(0)
    lp = link.NTN(16, 16, 1, hidden_dims=(128,))
    h = torch.randn(5, 8)
    want = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(h, lp.mlp_layers[0].W, lp.mlp_layers[0].b)),
                                      lp.l_out.W, lp.l_out.b)
    assert torch.equal(link._tail(lp.mlp_layers, lp.l_out, h), want)
