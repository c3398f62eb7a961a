"""Float64 restatement of the four pair features of csrc/bmp_link.hip and an ELEMENT-WISE bound on what a float32
evaluation of them may differ by (test infrastructure, not product; plain torch on the CPU, gradients through autograd).

The features, each as ``f(x1, x2, params)`` with ``params`` a dict of the tensors the kind has (absent or None: not there):
  SYM       [x1 + x2 | x1 * x2]
  HOLE      c[k] = sum_i x1[i] x2[(i + k) % d], the direct sum through an index table (no fft)
  DISTMULT  (x1 * x2) @ W.T                                   W [K x d]
  NTN       einsum('bp,pqo,bq->bo') + x1 @ V1 + x2 @ V2 + b   W [d1 x d2 x K], V1 [d1 x K], V2 [d2 x K], b [K]; V1, V2, b optional

The bound.  Every output, and every gradient against a cotangent ``cy``, is a polynomial with non-negative coefficients in
the inputs, the parameters and ``cy``.  The sum of the absolute values of one element's terms, S, is therefore the same
function (or its autograd gradient) at the absolute values of all of them.  A float32 evaluation in which every term passes
through at most r roundings differs from the exact value by at most  r * 2**-24 * S  to first order, whatever the order of
the sums; FMA contraction only removes roundings.  r per kind and output, counted on the kernels as written (a product
rounds once, an addition into an accumulator rounds once, the first addition to a zero accumulator is counted although it
is exact):

  SYM       y    1          one addition, or one product                                          k_pf_sym_fwd
            dx   2          gp * x (1), gs + . (1)                                                k_pf_sym_bwd
  HOLE      y    d + 1      a[i] * b[j] (1), d additions into acc                                 k_pf_hole_fwd
            dx   d + 1      gg[k] * b[jp] (1), d additions into s1 (s2 alike)                     k_pf_hole_bwd
  DISTMULT  y    d + 2      pr = x1 * x2 (1), W * pr (1), d additions                             k_pf_dm_fwd
            dx   K + 2      g * W (1), K additions into dp, dp * x (1)                            k_pf_dm_bwd_x
            dW   B + 2      g * x1 (1), . * x2 (1), B additions                                   k_pf_dm_bwd_w
  NTN       y    d1 + d2 + 2 (+ d2 with V2)   w * c (1), d2 additions into t (which starts from V1), a * t (1), d1 additions
                            into y (which starts from b), then d2 additions of the V2 terms       k_pf_ntn_fwd
            dx1  K + d2 + 2 w * gg (1), K additions into t, t * c (1), d2 additions into acc (which holds the V1 sum:
                            1 + K roundings, then the same d2 additions: shorter)                 k_pf_ntn_bwd_x
            dx2  K + d1 + 2 the same with p for q
            dW   B + 2      sx1 * sx2 (1), . * sg (1), one addition per row; the small path (d2 * K <= 128) adds the even and
                            the odd rows apart and the two sums once: ceil(B / 2) + 1 <= B        k_pf_ntn_bwd_w
            dV1  B + 1      sx1 * sg (1), B additions;  dV2 alike
            db   B          B additions
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

Tensor = torch.Tensor
U = 2.0 ** -24
KINDS = ("sym", "hole", "distmult", "ntn")
KIND_ID = dict(sym=0, hole=1, distmult=2, ntn=3)              # bmp.link.SYM / HOLE / DISTMULT / NTN_KIND
PARAMS = ("W", "V1", "V2", "b")

# The shapes of tests/test_gpu_link_edges.py, the smallest at which each path of the kernels exists.
# sym (B, d); hole (B, d); distmult (B, d, K); ntn (B, d1, d2, K)
SHAPES = {
    "sym": [(1, 1), (17, 48), (2049, 256)],                   # 2049 x 256 > 2048 x 256: the grid-stride loops wrap
    "hole": [(1, 1), (3, 2), (3, 20), (2, 256), (2, 257), (2, 1024)],      # 257: a thread's second column; 1024: PF_MAXD
    "distmult": [(1, 1, 1), (15, 64, 8), (16, 64, 8), (17, 1024, 8), (33, 48, 20), (2049, 256, 3)],
    "ntn": [(1, 1, 1, 1), (31, 16, 16, 8), (32, 16, 16, 8), (33, 16, 16, 8),       # small path, nW = 128, odd chunk / PF_WR
            (70, 16, 17, 8),                                  # nW = 136: first size on the general path
            (70, 24, 8, 16), (70, 8, 24, 5),                  # d1 > d2; d2 > d1 (workgroups p >= d1 own dV2 rows alone)
            (5, 256, 256, 16)],                               # nW = 4096: all MAXO = 16 outputs per thread
}
# refused before a launch: PF_MAXD, PF_MAXD / 4, PF_MAXK
REFUSED = {
    "hole": [(2, 1025)],
    "distmult": [(2, 1025, 3)],
    "ntn": [(2, 257, 16, 8), (2, 16, 257, 8), (2, 16, 16, 17)],
}


# ------------------------------------------------------------------------------------------------ the features
def sym(x1: Tensor, x2: Tensor, p=None) -> Tensor:
    return torch.cat((x1 + x2, x1 * x2), dim=1)


def rotation(d: int) -> Tensor:
    """rot[k, i] = (i + k) % d"""
    k = torch.arange(d)
    return (k[None, :] + k[:, None]) % d


def hole(x1: Tensor, x2: Tensor, p=None, rot: Optional[Tensor] = None) -> Tensor:
    rot = rotation(x1.shape[1]) if rot is None else rot
    return torch.einsum("bi,bki->bk", x1, x2[:, rot])


def distmult(x1: Tensor, x2: Tensor, p) -> Tensor:
    return (x1 * x2) @ p["W"].t()


def ntn(x1: Tensor, x2: Tensor, p) -> Tensor:
    y = torch.einsum("bp,pqo,bq->bo", x1, p["W"], x2)
    if p.get("V1") is not None:
        y = y + x1 @ p["V1"]
    if p.get("V2") is not None:
        y = y + x2 @ p["V2"]
    if p.get("b") is not None:
        y = y + p["b"]
    return y


FEATURE = dict(sym=sym, hole=hole, distmult=distmult, ntn=ntn)


def rounds(kind: str, x1: Tensor, x2: Tensor, p: Dict[str, Optional[Tensor]]) -> Dict[str, int]:
    """r of the module docstring, per output name."""
    B, d1 = x1.shape
    d2 = x2.shape[1]
    if kind == "sym":
        return dict(y=1, dx1=2, dx2=2)
    if kind == "hole":
        return dict(y=d1 + 1, dx1=d1 + 1, dx2=d1 + 1)
    if kind == "distmult":
        K = p["W"].shape[0]
        return dict(y=d1 + 2, dx1=K + 2, dx2=K + 2, dW=B + 2)
    K = p["W"].shape[2]
    return dict(y=d1 + d2 + 2 + (d2 if p.get("V2") is not None else 0), dx1=K + d2 + 2, dx2=K + d1 + 2, dW=B + 2,
                dV1=B + 1, dV2=B + 1, db=B)


# ------------------------------------------------------------------------------------------------ evaluation
def evaluate(f, x1: Tensor, x2: Tensor, p: Dict[str, Optional[Tensor]], cy: Tensor, dtype=torch.float64) -> Dict[str, Tensor]:
    """{'y', 'dx1', 'dx2', 'dW', ...}: ``f`` and its gradients against ``cy`` in ``dtype`` (parameters that are None: no key)."""
    x1, x2 = (t.detach().to(dtype).requires_grad_() for t in (x1, x2))
    p = {k: v.detach().to(dtype).requires_grad_() for k, v in (p or {}).items() if v is not None}
    y = f(x1, x2, p)
    names = [k for k in PARAMS if k in p]
    grads = torch.autograd.grad(y, [x1, x2] + [p[k] for k in names], cy.to(dtype))
    out = dict(y=y.detach(), dx1=grads[0], dx2=grads[1])
    out.update({"d" + k: g for k, g in zip(names, grads[2:])})
    return out


def reference(kind: str, x1: Tensor, x2: Tensor, p, cy: Tensor) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """(float64 values, element-wise bounds r * 2**-24 * S) of the feature and of every gradient against ``cy``."""
    f = FEATURE[kind]
    want = evaluate(f, x1, x2, p, cy)
    ab = lambda t: None if t is None else t.detach().abs()
    S = evaluate(f, ab(x1), ab(x2), {k: ab(v) for k, v in (p or {}).items()}, ab(cy))
    r = rounds(kind, x1, x2, p or {})
    return want, {k: r[k] * U * S[k] for k in want}


def ratio(got: Tensor, want: Tensor, bound: Tensor) -> float:
    """Worst err / bound over the elements (0 / 0 counts as 0, err > 0 against a bound of 0 as inf)."""
    from parity_util import bound_ratio
    return bound_ratio(got, want, bound)[0]


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(kind: str, shape, seed: int = 0, V1: bool = True, V2: bool = True, b: bool = True):
    """(x1, x2, params, cy) in float32: inputs and cotangent randn, parameters randn * 0.3, fixed seed."""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    if kind in ("sym", "hole"):
        B, d = shape
        return rn(B, d), rn(B, d), {}, rn(B, 2 * d if kind == "sym" else d)
    if kind == "distmult":
        B, d, K = shape
        return rn(B, d), rn(B, d), dict(W=rn(K, d) * 0.3), rn(B, K)
    B, d1, d2, K = shape
    x1, x2 = rn(B, d1), rn(B, d2)
    W, v1, v2, bb = rn(d1, d2, K) * 0.3, rn(d1, K) * 0.3, rn(d2, K) * 0.3, rn(K) * 0.3        # drawn whether present or not
    return x1, x2, dict(W=W, V1=v1 if V1 else None, V2=v2 if V2 else None, b=bb if b else None), rn(B, K)
