"""Packed-row float64 reference of BiMPM, one drug pair at a time, from the formulas in the header of csrc/bmp_bimpm.hip,
with the maxima's selections made explicit.

    m(u, v)  = u.v / ((|u| + 1e-5)(|v| + 1e-5))
    pool     s_ijk = m(P_k*x_i, P_k*y_j)            m1_ik = max_j s_ijk  (arg j1s [n1,H]),  m2_jk = max_i s_ijk  (arg i2s [n2,H])
    att_ij   = m(x_i, y_j)
    mean     M2_i = sum_j w2_j att_ij y_j / max(sum_j w2_j att_ij, 1e-4)          mm1_ik = m(Q_k*x_i, Q_0*M2_i)
    max      T2_ic = max_j att_ij y_jc  (arg jT2 [n1,d]),  T1_jc = max_i att_ij x_ic  (arg iT1 [n2,d])
                                                                                  mx1_ik = m(R_k*x_i, R_0*T2_i)
    mol_1 = sum_i w1_i [m1_i | mm1_i | mx1_i],  side 2 alike.
Sums carry the row multiplicities w; maxima run over the rows with w > 0 and count a row once.

Selections.  Every maximum is taken as ``torch.gather`` at an index array, so the result is a smooth function of the
inputs and autograd gives the gradient FOR THOSE SELECTIONS: the winner's term, all of it (the kernel's convention: a tie
goes to the first index, strict `>`, and the gradient to that one winner).  Without ``sel=`` the indices are the arg-maxima
of the float64 score tables (first index on ties, ``torch.argmax``); with ``sel=`` they are forced, e.g. to the ones a
float32 kernel made, which removes near-ties from a gradient comparison instead of hiding them in a tolerance.

Zero norms.  |u| is not differentiable at u = 0; the kernel takes the subgradient 0 there (the `nu > 0` guard of
bm_dmatch), and so does ``_norm`` below (``torch.where`` on a safe argument: finite gradients, where sqrt gives NaN).

tau -- how far below the float64 maximum a float32 selection may lie.  A pooled score is computed in float32 as
    t = fl( fl(s * ia) / fl(nPB + eps) ),   s = sum_c (p_c p_c x_c) y_c,   ia = fl(1 / fl(nPA + eps)),   nP = sqrt(sum_c (p_c x_c)^2)
with u = 2^-24, to first order in u and for ANY summation order:
    s    two roundings in p_c p_c x_c and d accumulating (fused) steps: |fl(s) - s| <= (d + 2) u sum_c |p_c^2 x_c y_c|
                                                                                  <= (d + 2) u nPA nPB      (Cauchy-Schwarz)
    nP   one rounding in p_c x_c (twice in its square), d accumulating steps: relative (d + 2) u on a sum of non-negative
         terms, halved by the root, plus the root's own rounding: (d/2 + 2) u;  + eps: (d/2 + 3) u;  1 / that: (d/2 + 4) u
    t    s * ia: one more u;  / fl(nPB + eps): (d/2 + 3) u + u
so |fl(t) - t| <= [(d + 2) + (d/2 + 4) + 1 + (d/2 + 4)] u = (2 d + 11) u, as |t| <= 1 and nPA nPB / ((nPA + eps)(nPB + eps)) <= 1.
att_ij has the same form with fewer operations.  ``score_bound(d)`` is (2 d + 16) u: the five spare u cover the second-order
terms and the one rounding of att_ij * y_jc.  A float32 arg-max j and the float64 arg-max j* both carry that error, so
    pool:  s64[j] >= s64[j*] - 2 score_bound(d)                                   = tau_pool(d)
    max:   att_ij y_jc is the bounded att times y_jc:  >= max - 2 score_bound(d) max_j |y_jc|   = tau_att(d, Y)[c]
(the inputs are float32 numbers, exact in float64: no input rounding).  tests/test_bimpm_ref.py confirms that a float32
evaluation of this file never needs more; the GPU tests hold the kernel's selections to it.
"""
import torch

EPS = 1e-5           # chainer.functions.normalize
DIV_EPS = 1e-4       # div_with_small_value
U32 = 2.0 ** -24

SEL_NAMES = ("jT2", "iT1", "j1s", "i2s")


def score_bound(d):
    return (2 * d + 16) * U32


def tau_pool(d):
    return 2 * score_bound(d)


def tau_att(d, other, w_other):
    """[d]: per feature column, for maxima of att * other[:, c] over the rows of ``other`` with w > 0."""
    a = other.double().abs()
    return 2 * score_bound(d) * torch.where((w_other > 0)[:, None], a, torch.zeros_like(a)).max(dim=0).values


def _norm(u):
    """|u| over the last axis with derivative 0 at u = 0."""
    s = (u * u).sum(-1)
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def _match_vec(x, V, W, nWx):
    """m(W_k * x_a, W_0 * V_a) -> [n, H]"""
    z = W[0] * V
    return ((W[None] * x[:, None]) * z[:, None]).sum(-1) / ((nWx + EPS) * (_norm(z) + EPS)[:, None])


def _argmax_live(table, live, dim):
    """first arg-max along ``dim`` (0 or 1) of a [n1, n2, *] table over the live rows of that axis"""
    mask = live[:, None, None] if dim == 0 else live[None, :, None]
    return table.masked_fill(~mask, float("-inf")).argmax(dim=dim)


def score_tables(x1, x2, P):
    """the detached tables the maxima run over: pool [n1,n2,H] = s_ijk, T2 [n1,n2,d] = att_ij y_jc, T1 [n1,n2,d] = att_ij x_ic"""
    with torch.no_grad():
        nP1, nP2 = _norm(P[None] * x1[:, None]), _norm(P[None] * x2[:, None])
        att = (x1 @ x2.t()) / ((_norm(x1) + EPS)[:, None] * (_norm(x2) + EPS)[None])
        pool = torch.einsum("ikc,jc->ijk", (P * P)[None] * x1[:, None], x2) / ((nP1 + EPS)[:, None] * (nP2 + EPS)[None])
        return dict(pool=pool, T2=att[:, :, None] * x2[None], T1=att[:, :, None] * x1[:, None])


def bimpm_pair(x1, x2, w1, w2, P, Q, R, sel=None, dtype=torch.float64, tables=True):
    """One pair.  x1 [n1,d], x2 [n2,d], w1 [n1], w2 [n2], P/Q/R [H,d].  Returns a dict: mol_1, mol_2 [3H]; sel (the four
    int64 index arrays used); D2 [n1], D1 [n2] (the attention sums before the clamp); and, with ``tables``, scores: the
    detached tables the unforced selections are taken from -- pool [n1,n2,H], T2 [n1,n2,d] = att_ij y_jc, T1 = att_ij x_ic."""
    x1, x2, w1, w2, P, Q, R = (t.to(dtype) for t in (x1, x2, w1, w2, P, Q, R))
    live1, live2 = w1 > 0, w2 > 0
    nP1, nP2 = _norm(P[None] * x1[:, None]), _norm(P[None] * x2[:, None])          # [n, H]
    nQ1, nQ2 = _norm(Q[None] * x1[:, None]), _norm(Q[None] * x2[:, None])
    nR1, nR2 = _norm(R[None] * x1[:, None]), _norm(R[None] * x2[:, None])
    att = (x1 @ x2.t()) / ((_norm(x1) + EPS)[:, None] * (_norm(x2) + EPS)[None])   # [n1, n2]
    scores = None
    if tables or sel is None:
        scores = score_tables(x1, x2, P)
    if sel is None:
        sel = dict(jT2=_argmax_live(scores["T2"], live2, 1), iT1=_argmax_live(scores["T1"], live1, 0),
                   j1s=_argmax_live(scores["pool"], live2, 1), i2s=_argmax_live(scores["pool"], live1, 0))
    sel = {k: torch.as_tensor(sel[k]).long() for k in SEL_NAMES}
    jT2, iT1, j1s, i2s = (sel[k] for k in SEL_NAMES)
    # (1) max-pooling matching at the selected partners
    P2 = (P * P)[None]
    m1 = (P2 * x1[:, None] * x2[j1s]).sum(-1) / ((nP1 + EPS) * (nP2.gather(0, j1s) + EPS))
    m2 = (P2 * x2[:, None] * x1[i2s]).sum(-1) / ((nP2 + EPS) * (nP1.gather(0, i2s) + EPS))
    # (3) attentive mean
    a2, a1 = att * w2[None], att * w1[:, None]
    D2, D1 = a2.sum(1), a1.sum(0)
    M2 = (a2 @ x2) / torch.clamp(D2, min=DIV_EPS)[:, None]
    M1 = (a1.t() @ x1) / torch.clamp(D1, min=DIV_EPS)[:, None]
    # (4) attentive max at the selected partners
    T2 = att.gather(1, jT2) * x2.gather(0, jT2)
    T1 = att.t().gather(1, iT1) * x1.gather(0, iT1)
    f1 = torch.cat([m1, _match_vec(x1, M2, Q, nQ1), _match_vec(x1, T2, R, nR1)], dim=1)
    f2 = torch.cat([m2, _match_vec(x2, M1, Q, nQ2), _match_vec(x2, T1, R, nR2)], dim=1)
    zero = torch.zeros((), dtype=dtype)
    mol_1 = torch.where(live1[:, None], w1[:, None] * f1, zero).sum(0)
    mol_2 = torch.where(live2[:, None], w2[:, None] * f2, zero).sum(0)
    return dict(mol_1=mol_1, mol_2=mol_2, sel=sel, D2=D2.detach(), D1=D1.detach(), scores=scores if tables else None)


def _gaps(x1, x2, w1, w2, P, sel):
    """per pair, no data-dependent shapes (it is vmapped over equal-shaped pairs): (4 flags: an index of a row with w > 0 out
    of range or on a row with w = 0; 4 worst (float64 maximum - score at the selection) / tau over the rows with w > 0)"""
    d = x1.shape[-1]
    x1, x2, P = x1.double(), x2.double(), P.double()
    live1, live2 = w1 > 0, w2 > 0
    scores = score_tables(x1, x2, P)
    #        table, axis of the maximum, live rows of that axis, live rows of the owner axis, tau
    spec = dict(jT2=("T2", 1, live2, live1, tau_att(d, x2, w2)), iT1=("T1", 0, live1, live2, tau_att(d, x1, w1)),
                j1s=("pool", 1, live2, live1, tau_pool(d)), i2s=("pool", 0, live1, live2, tau_pool(d)))
    bad, gaps = [], []
    for name in SEL_NAMES:
        tab, dim, live_o, live_a, tau_n = spec[name]
        s = sel[name].long()
        n_o = live_o.shape[0]
        idx = s.clamp(0, n_o - 1)
        bad.append((live_a[:, None] & ((s != idx) | ~live_o[idx])).any())
        t = scores[tab]
        mask = live_o[:, None, None] if dim == 0 else live_o[None, :, None]
        best = t.masked_fill(~mask, float("-inf")).max(dim=dim).values
        got = t.gather(dim, idx.unsqueeze(dim)).squeeze(dim)
        gap = (best - got) / tau_n
        gaps.append(torch.where(live_a[:, None], gap, torch.zeros_like(gap)).max())
    return torch.stack(bad), torch.stack(gaps)


def selection_gaps(x1, x2, w1, w2, P, sel):
    """How the selections ``sel`` of one pair stand against the float64 score tables: asserts every index (of a row with
    w > 0) in range and on a row with w > 0, and returns {name: max over those rows of (float64 maximum - score at the
    selection) / tau}; a selection is valid where that is <= 1.  Rows with w = 0 reach neither an output nor a gradient and
    are not judged."""
    bad, gaps = _gaps(x1, x2, w1, w2, P, {k: torch.as_tensor(sel[k]) for k in SEL_NAMES})
    assert not bad.any(), f"an index out of range or on a row with w = 0: {dict(zip(SEL_NAMES, bad.tolist()))}"
    return dict(zip(SEL_NAMES, gaps.tolist()))


def _groups(n1, n2):
    """pairs of one (n1, n2) shape are evaluated in one vmapped call of the per-pair function"""
    by = {}
    for p, key in enumerate(zip(n1, n2)):
        by.setdefault(key, []).append(p)
    return by


def _rows(X, r, n, ps):
    return X[torch.tensor([[r[p] + i for i in range(n)] for p in ps], dtype=torch.long)]


def packed_selection_gaps(X1, X2, w1, w2, r1, n1, r2, n2, P, sels):
    """``selection_gaps`` for every pair of a packed batch -> [B, 4] (columns SEL_NAMES)"""
    out = torch.zeros(len(r1), 4, dtype=torch.float64)
    for (a, b), ps in _groups(n1, n2).items():
        sel = {k: torch.stack([torch.as_tensor(sels[p][k]) for p in ps]) for k in SEL_NAMES}
        bad, gaps = torch.vmap(lambda x, y, wx, wy, s: _gaps(x, y, wx, wy, P, s))(
            _rows(X1, r1, a, ps), _rows(X2, r2, b, ps), _rows(w1, r1, a, ps), _rows(w2, r2, b, ps), sel)
        assert not bad.any(), f"pairs {[ps[i] for i in bad.any(1).nonzero().flatten().tolist()]}: an index out of range or on a row with w = 0"
        out[ps] = gaps
    return out


def bimpm_packed(X1, X2, w1, w2, r1, n1, r2, n2, P, Q, R, sels=None):
    """The B pairs of a packed batch: rows r1[p] .. r1[p] + n1[p] of X1 against rows r2[p] .. of X2 (X1 and X2 may be one
    tensor).  float64 throughout; autograd reaches X1, X2, P, Q, R where they require it, and a row of no pair gets no
    gradient.  sels: per pair, forced selections.  ``bimpm_pair`` is applied pair by pair, vmapped over the pairs of one
    shape.  Returns mol_1, mol_2 [B, 3H] and per pair a dict with the attention sums D2, D1."""
    B = len(r1)
    o1, o2, res = [None] * B, [None] * B, [None] * B

    def one(x, y, wx, wy, s):
        r = bimpm_pair(x, y, wx, wy, P, Q, R, sel=s, tables=False)
        return r["mol_1"], r["mol_2"], r["D2"], r["D1"]

    for (a, b), ps in _groups(n1, n2).items():
        args = (_rows(X1, r1, a, ps), _rows(X2, r2, b, ps), _rows(w1, r1, a, ps), _rows(w2, r2, b, ps))
        if sels is None:
            m1, m2, D2, D1 = torch.vmap(lambda x, y, wx, wy: one(x, y, wx, wy, None))(*args)
        else:
            sel = {k: torch.stack([torch.as_tensor(sels[p][k]) for p in ps]) for k in SEL_NAMES}
            m1, m2, D2, D1 = torch.vmap(one)(*args, sel)
        for i, p in enumerate(ps):
            o1[p], o2[p], res[p] = m1[i], m2[i], dict(D2=D2[i], D1=D1[i])
    return torch.stack(o1), torch.stack(o2), res
