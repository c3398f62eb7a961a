"""GPU parity of the segment operators of csrc/bmp_seg.hip, one by one, and of the five coarse co-attention modules built
on them, against the float64 packed restatement tests/seg_ref.py (pinned to the dense oracle in tests/test_seg_ref.py).

The shared batch (seg_ref.fixture_batch) has molecules of 2..301 rows: it wraps the 64-lane row loops of the softmax
kernels, takes every remainder of the 4-row groups of the pool backward and the correlation, fills a tile, spans several
tiles and leaves tail rows that belong to no molecule.  The widths turn every column loop at least twice and leave a
ragged tail: 72 and 320 for the 64- and 256-wide loops, 24 / 40 / 72 for the 32-lane dot product.
Tolerance: 1e-4 of the tensor's max-abs (test_gpu_ops.TOL); index-only results are compared bit for bit."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import seg_ref as SR                                   # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from test_gpu_ops import close, dev, to_dev            # noqa: E402


def _idx(pb):
    """Index tensors of a packed batch as the kernels take them (device) and as seg_ref takes them (host)."""
    rm = SR.row_mol_of(pb.mol_row0, pb.mol_nrows, pb.n_rows)
    assert torch.equal(rm.int(), pb.row_mol)
    d = dev()
    return SimpleNamespace(pb=pb, N=pb.n_rows, M=pb.n_mols, w=pb.row_w, row0=pb.mol_row0, nrows=pb.mol_nrows, row_mol=rm,
                           dead=rm < 0, wd=pb.row_w.to(d), row0d=pb.mol_row0.to(d), nrowsd=pb.mol_nrows.to(d),
                           row_mold=pb.row_mol.to(d))


@pytest.fixture(scope="module")
def fx():
    pb, p1, p2 = SR.fixture_batch()
    f = _idx(pb)
    f.p1, f.p2 = p1, p2
    assert int(f.dead.sum()) > 0
    return f


@pytest.fixture(scope="module")
def tiny():
    """The four smallest molecules alone (2, 3, 4 and 5 rows), for the correlation at its width bound."""
    return _idx(SR.fixture_batch(sizes=SR.SIZES[:4], partner=(0, 2, 1, 3))[1])


def _rand(g, *shape, scale=1.0):
    """float32 values, so that the kernel and the float64 reference start from the same numbers"""
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


# name -> (kernel call, reference call), both on (f, dict of inputs); row-shaped inputs first
def _ops():
    from bmp import coarse as C
    return {
        "segpool": (lambda f, i: C.SegPoolFn.apply(i["A"], i["Y"], f.wd, f.row0d, f.nrowsd),
                    lambda f, i: SR.segpool(i["A"], i["Y"], f.w, f.row0, f.nrows)),
        "segsoftmax": (lambda f, i: C.SegSoftmaxFn.apply(i["s"], f.wd, f.row0d, f.nrowsd),
                       lambda f, i: SR.segsoftmax(i["s"], f.w, f.row0, f.nrows)),
        "rowbcast": (lambda f, i: C.RowBcastFn.apply(i["q"], f.row_mold, f.row0d, f.nrowsd),
                     lambda f, i: SR.rowbcast(i["q"], f.row_mol)),
        "rowdot": (lambda f, i: C.RowDotFn.apply(i["x"], i["u"], i.get("s0"), f.row_mold, f.row0d, f.nrowsd),
                   lambda f, i: SR.rowdot(i["x"], i["u"], i.get("s0"), f.row_mol)),
        "rowcorr": (lambda f, i: C.RowCorrFn.apply(i["a"], i["q"], f.row0d, f.nrowsd),
                    lambda f, i: SR.rowcorr(i["a"], i["q"], f.row0, f.nrows)),
    }


def _gpu(f, op, inputs, cot):
    """Kernel forward and backward: (output, {input name: gradient}), on the host."""
    leaf = {k: v.detach().clone().to(dev()).requires_grad_() for k, v in inputs.items()}
    out = _ops()[op][0](f, leaf)
    (out * cot.to(dev())).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: v.grad.cpu() for k, v in leaf.items()}


def _ref(f, op, inputs, cot):
    leaf = {k: v.detach().double().requires_grad_() for k, v in inputs.items()}
    out = _ops()[op][1](f, leaf)
    (out * cot.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaf.items()}


def _parity(f, op, inputs, g, tag):
    shape = {"segpool": lambda: (f.M, inputs["Y"].shape[1]), "segsoftmax": lambda: (f.N,),
             "rowbcast": lambda: (f.N, inputs["q"].shape[1]), "rowdot": lambda: (f.N,),
             "rowcorr": lambda: tuple(inputs["a"].shape)}[op]()
    cot = _rand(g, *shape)
    out_r, gr_r = _ref(f, op, inputs, cot)
    out, gr = _gpu(f, op, inputs, cot)
    close(out, out_r, f"{op} {tag} out")
    for k in inputs:
        close(gr[k], gr_r[k], f"{op} {tag} d{k}")
    return out, gr


# ------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("o", [8, 24, 72, 320])
@pytest.mark.parametrize("gate", [False, True])
def test_segpool(fx, o, gate):
    g = torch.Generator().manual_seed(o + gate)
    _parity(fx, "segpool", dict(A=_rand(g, fx.N, o if gate else 1), Y=_rand(g, fx.N, o)), g, f"o={o} ca={o if gate else 1}")


@pytest.mark.parametrize("offset", [0.0, 80.0])
def test_segsoftmax(fx, offset):
    """Scores offset by +80: exp(80) overflows nothing only because the kernel subtracts the molecule's maximum."""
    g = torch.Generator().manual_seed(7)
    _parity(fx, "segsoftmax", dict(s=_rand(g, fx.N, scale=2.0) + offset), g, f"offset={offset}")


@pytest.mark.parametrize("c", [8, 72, 320])
def test_rowbcast(fx, c):
    g = torch.Generator().manual_seed(c)
    q = _rand(g, fx.M, c)
    out, _ = _parity(fx, "rowbcast", dict(q=q), g, f"c={c}")
    live = ~fx.dead
    assert torch.equal(out[live], q[fx.row_mol[live]])               # a pure copy
    assert torch.equal(out[fx.dead], torch.zeros(int(fx.dead.sum()), c))


@pytest.mark.parametrize("d", [8, 24, 40, 72, 320])
@pytest.mark.parametrize("bias", [False, True])
def test_rowdot(fx, d, bias):
    g = torch.Generator().manual_seed(d + bias)
    inputs = dict(x=_rand(g, fx.N, d), u=_rand(g, fx.M, d))
    if bias:
        inputs["s0"] = _rand(g, fx.M)
    _parity(fx, "rowdot", inputs, g, f"d={d} s0={bias}")


@pytest.mark.parametrize("o", [8, 24, 72, 320])
def test_rowcorr(fx, o):
    g = torch.Generator().manual_seed(o)
    _parity(fx, "rowcorr", dict(a=_rand(g, fx.N, o), q=_rand(g, fx.M, o)), g, f"o={o}")


def test_rowcorr_at_the_width_bound(tiny):
    g = torch.Generator().manual_seed(1024)
    _parity(tiny, "rowcorr", dict(a=_rand(g, tiny.N, 1024), q=_rand(g, tiny.M, 1024)), g, "o=1024")


# -------------------------------------------------------------------- asymmetric known answers, bit for bit
def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float()


@pytest.mark.parametrize("o", [24, 320])
def test_rowcorr_of_unit_rows_reads_the_rotated_vector(fx, o):
    """a[r] = e_t gives e[r][k] = q[m][(t + k) mod o] exactly: a transposed or mirrored index cannot hide behind
    random data."""
    g = torch.Generator().manual_seed(o)
    t = (7 * torch.arange(fx.N) + 3) % o
    a = torch.zeros(fx.N, o).index_put((torch.arange(fx.N), t), torch.ones(fx.N))
    q = _rand(g, fx.M, o)
    e, _ = _gpu(fx, "rowcorr", dict(a=a, q=q), torch.zeros(fx.N, o))
    live = ~fx.dead
    col = (t[:, None] + torch.arange(o)[None, :]) % o
    want = torch.gather(q[fx.row_mol.clamp(min=0)], 1, col)
    assert torch.equal(e[live], want[live])
    assert torch.equal(e[fx.dead], torch.zeros(int(fx.dead.sum()), o))


@pytest.mark.parametrize("o", [24, 320])
def test_rowcorr_with_a_unit_vector_rotates_the_rows(fx, o):
    """q[m] = e_s gives e[r][k] = a[r][(s - k) mod o] and da[r][t] = de[r][(s - t) mod o]; with small integers in a and
    de every sum is exact in float32, so dq[m][j] = sum_r sum_t a[r][t] de[r][(j - t) mod o] is exact as well."""
    g = torch.Generator().manual_seed(o + 1)
    s = (5 * torch.arange(fx.M) + 2) % o
    q = torch.zeros(fx.M, o).index_put((torch.arange(fx.M), s), torch.ones(fx.M))
    a, de = _ints(g, fx.N, o), _ints(g, fx.N, o)
    e, gr = _gpu(fx, "rowcorr", dict(a=a, q=q), de)
    live = ~fx.dead
    rot = (s[fx.row_mol.clamp(min=0)][:, None] - torch.arange(o)[None, :]) % o
    assert torch.equal(e[live], torch.gather(a, 1, rot)[live])
    assert torch.equal(gr["a"][live], torch.gather(de, 1, rot)[live])
    _, gr_r = _ref(fx, "rowcorr", dict(a=a, q=q), de)
    assert float(gr_r["q"].abs().max()) < 2 ** 24
    assert torch.equal(gr["q"].double(), gr_r["q"])


# ------------------------------------------------------------------------------ rows outside every molecule
def _op_inputs(f, op, g):
    return {"segpool": lambda: dict(A=_rand(g, f.N, 72), Y=_rand(g, f.N, 72)),
            "segpool1": lambda: dict(A=_rand(g, f.N, 1), Y=_rand(g, f.N, 72)),
            "segsoftmax": lambda: dict(s=_rand(g, f.N)),
            "rowbcast": lambda: dict(q=_rand(g, f.M, 72)),
            "rowdot": lambda: dict(x=_rand(g, f.N, 72), u=_rand(g, f.M, 72), s0=_rand(g, f.M)),
            "rowcorr": lambda: dict(a=_rand(g, f.N, 72), q=_rand(g, f.M, 72))}[op]()


@pytest.mark.parametrize("op", ["segpool", "segpool1", "segsoftmax", "rowbcast", "rowdot", "rowcorr"])
def test_rows_of_no_molecule(fx, op):
    """Random finite values in the rows of no molecule (inputs and incoming gradients): every per-row output and
    gradient is exactly 0 there, and nothing a molecule gets changes when those rows change."""
    g = torch.Generator().manual_seed(11)
    name = op.rstrip("1")
    inputs = _op_inputs(fx, op, g)
    probe = _ops()[name][1](fx, {k: v.double() for k, v in inputs.items()})
    cot = _rand(g, *probe.shape)
    out, gr = _gpu(fx, name, inputs, cot)
    per_row = [("out", out)] if out.shape[0] == fx.N else []
    per_row += [(f"d{k}", v) for k, v in gr.items() if v.shape[0] == fx.N]
    assert per_row
    for nm, t in per_row:
        assert torch.isfinite(t).all() and float(t[fx.dead].abs().max()) == 0.0, f"{op} {nm}"
    inputs2 = {k: (torch.where(fx.dead.reshape(-1, *[1] * (v.dim() - 1)), _rand(g, *v.shape, scale=50.0), v)
                   if v.shape[0] == fx.N else v) for k, v in inputs.items()}
    cot2 = torch.where(fx.dead.reshape(-1, *[1] * (cot.dim() - 1)), _rand(g, *cot.shape, scale=50.0), cot) \
        if cot.shape[0] == fx.N else cot
    out2, gr2 = _gpu(fx, name, inputs2, cot2)
    assert torch.equal(out, out2), op
    for k in gr:
        assert torch.equal(gr[k], gr2[k]), f"{op} d{k}"


# ------------------------------------------------------------------------------ argument checks of the C ABI
def test_argument_checks_return_nonzero_and_write_nothing(fx):
    from bmp import _lib
    from bmp._lib import ptr, stream
    L = _lib.lib()
    d = dev()
    N, M, o = fx.N, fx.M, 8
    z = lambda *s: torch.zeros(*s, device=d)
    mark = lambda *s: torch.full(s, 7.0, device=d)
    A, Y, q = z(N, o), z(N, o), z(M, o)
    outs = []

    def fresh(*s):
        outs.append(mark(*s))
        return outs[-1]
    w, r0, nr, rm = fx.wd, fx.row0d, fx.nrowsd, fx.row_mold
    rcs = {
        "segpool_fwd ca=2": L.bmp_segpool_fwd(ptr(A), 2, ptr(Y), o, ptr(w), ptr(r0), ptr(nr), M, ptr(fresh(M, o)), stream()),
        "segpool_bwd ca=2": L.bmp_segpool_bwd(ptr(q), ptr(A), 2, ptr(Y), o, ptr(w), ptr(r0), ptr(nr), M, N, ptr(fresh(N, o)),
                                              ptr(fresh(N, o)), stream()),
        "rowcorr_fwd o=1028": L.bmp_rowcorr_fwd(ptr(z(N, 1028)), 1028, ptr(z(M, 1028)), ptr(r0), ptr(nr), M,
                                                ptr(fresh(N, 1028)), stream()),
        "rowcorr_bwd o=1028": L.bmp_rowcorr_bwd(ptr(z(N, 1028)), ptr(z(N, 1028)), 1028, ptr(z(M, 1028)), ptr(r0), ptr(nr), M,
                                                ptr(fresh(N, 1028)), ptr(fresh(M, 1028)), stream()),
        "segpool_fwd M=0": L.bmp_segpool_fwd(ptr(A), o, ptr(Y), o, ptr(w), ptr(r0), ptr(nr), 0, ptr(fresh(M, o)), stream()),
        "segpool_bwd M=0": L.bmp_segpool_bwd(ptr(q), ptr(A), o, ptr(Y), o, ptr(w), ptr(r0), ptr(nr), 0, N, ptr(fresh(N, o)),
                                             ptr(fresh(N, o)), stream()),
        "segsoftmax_fwd M=0": L.bmp_segsoftmax_fwd(ptr(z(N)), ptr(w), ptr(r0), ptr(nr), 0, N, ptr(fresh(N)), stream()),
        "segsoftmax_bwd M=0": L.bmp_segsoftmax_bwd(ptr(z(N)), ptr(z(N)), ptr(w), ptr(r0), ptr(nr), 0, N, ptr(fresh(N)),
                                                   stream()),
        "rowbcast_bwd M=0": L.bmp_rowbcast_bwd(ptr(Y), o, ptr(r0), ptr(nr), 0, ptr(fresh(M, o)), stream()),
        "rowdot_bwd M=0": L.bmp_rowdot_bwd(ptr(z(N)), ptr(Y), o, ptr(q), ptr(rm), ptr(r0), ptr(nr), 0, N, ptr(fresh(N, o)),
                                           ptr(fresh(M, o)), ptr(fresh(M)), stream()),
        "rowcorr_fwd M=0": L.bmp_rowcorr_fwd(ptr(A), o, ptr(q), ptr(r0), ptr(nr), 0, ptr(fresh(N, o)), stream()),
        "rowcorr_bwd M=0": L.bmp_rowcorr_bwd(ptr(A), ptr(A), o, ptr(q), ptr(r0), ptr(nr), 0, ptr(fresh(N, o)),
                                             ptr(fresh(M, o)), stream()),
    }
    torch.cuda.synchronize()
    for name, rc in rcs.items():
        assert rc != 0, name
    for t in outs:
        assert bool((t == 7.0).all())


# ---------------------------------------------------------------------------------------------------- modules
def _build(kind, hid, out, act, tying, head, seed):
    from bmp import coarse as C
    dr = O._Draw(seed, torch.float64, 0.2)
    if kind == "parallel":
        O.init_parallel(dr, "", hid, out, 1, weight_tying=tying)
        mod = C.ParallelCoattention(hid, out, 1, activation=act, weight_tying=tying)
        ref = lambda p, s1, g1, s2, g2: SR.parallel(p, s1, g1, s2, g2, activation=act, weight_tying=tying)
    elif kind == "circ":
        dr.lin("j_layer", hid, out)
        mod = C.CircularParallelCoattention(hid, out, activation=act)
        ref = lambda p, s1, g1, s2, g2: SR.circ(p, s1, g1, s2, g2, activation=act)
    elif kind == "alternating":
        O.init_alternating(dr, "", hid, out, head)
        mod = C.AlternatingCoattention(hid, out, head, weight_tying=True)
        ref = lambda p, s1, g1, s2, g2: SR.alternating(p, s1, g1, s2, g2)
    elif kind == "global":
        O.init_global(dr, "", hid, out, weight_tying=tying)
        mod = C.GlobalCoattention(hid, out, weight_tying=tying)
        ref = lambda p, s1, g1, s2, g2: SR.global_(p, s1, s2, weight_tying=tying)
    else:
        O.init_neural(dr, "", hid, out, weight_tying=tying)
        # doc . context is a sum of out_dim products and feeds a sigmoid: as drawn it is ~10 everywhere with sigmoid
        # activations (every factor in (0, 1)) and beyond +-14 on a sixth of the rows at out_dim = 320, where the gate is
        # flat and hides everything in front of it.  tanh: parameters scaled by 0.3; sigmoid: biases lowered by 2
        # (factors of ~0.12).  The test asserts the live gate on the reference.
        for k in dr.p:
            dr.p[k] = dr.p[k] - 2.0 if act == "sigmoid" and k.endswith("/b") else dr.p[k] * (0.3 if act == "tanh" else 1.0)
        mod = C.NeuralCoattention(hid, out, activation=act, weight_tying=tying)
        ref = lambda p, s1, g1, s2, g2, **kw: SR.neural(p, s1, s2, activation=act, weight_tying=tying, **kw)
    return dr.p, mod, ref


MODULE_CASES = [
    # kind, hidden_dim, out_dim, activation, weight_tying, head
    ("parallel", 24, 72, "tanh", True, 1), ("parallel", 72, 40, "sigmoid", False, 1), ("parallel", 160, 320, "tanh", False, 1),
    ("circ", 24, 72, "tanh", True, 0), ("circ", 72, 40, "sigmoid", True, 0), ("circ", 160, 320, "tanh", True, 0),
    ("alternating", 24, 72, "tanh", True, 5), ("alternating", 72, 40, "tanh", True, 5),
    ("alternating", 160, 320, "tanh", True, 5),
    ("global", 24, 72, "sigmoid", True, 0), ("global", 72, 40, "sigmoid", False, 0), ("global", 160, 320, "sigmoid", False, 0),
    ("neural", 24, 72, "tanh", True, 0), ("neural", 72, 40, "sigmoid", False, 0), ("neural", 160, 320, "tanh", False, 0),
    ("neural", SR.RELU_CASE["hidden_dim"], SR.RELU_CASE["out_dim"], "relu", SR.RELU_CASE["weight_tying"], 0),
]


@pytest.mark.parametrize("kind,hid,out,act,tying,head", MODULE_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-{'tied' if c[4] else 'untied'}" for c in MODULE_CASES])
def test_coarse_module(fx, kind, hid, out, act, tying, head):
    """One coarse module on PackedAtoms(X, pb) of the shared batch with random atom states and readouts: outputs, dX,
    dg and every parameter gradient vs seg_ref, on the two-sided batch in one call and as two one-sided batches.
    Untied modules get distinct parameters per focus (the oracle's initialisers draw them one after the other)."""
    from bmp.ggnn import PackedAtoms
    from bmp.snapshot import grad_dict, load_param_dict
    pb, B = fx.pb, fx.M // 2
    p, mod, ref = _build(kind, hid, out, act, tying, head, seed=hid + out)
    g = torch.Generator().manual_seed(hid * 7 + out)
    X = _rand(g, pb.n_rows, hid).double()
    if act == "relu":                   # the parameters and atom states whose pre-activations clear the kink band
        p, X = SR.relu_case_inputs(SR.RELU_SEED)
    if not tying:
        twins = [k for k in p if "/1/" in k]
        assert twins and all(not torch.equal(p[k], p[k.replace("/1/", "/0/")]) for k in twins)
    p = {k: v.float().double().requires_grad_() for k, v in p.items()}
    # readouts of size ~ 1 / sqrt(out_dim): the energies stay of order 1 and the activations off their flat ends
    g_1, g_2 = (_rand(g, B, out, scale=out ** -0.5).double().requires_grad_() for _ in range(2))
    c_1, c_2 = (_rand(g, B, out).double() for _ in range(2))
    Xr = X.clone().requires_grad_()
    en = []
    r1, r2 = ref(p, *[v for pair in zip(SR.sides_of(pb, Xr), (g_1, g_2)) for v in pair],
                 **(dict(energy_out=en) if kind == "neural" else {}))
    if kind == "neural":                # the gate is off its flat ends: what lies in front of it reaches the gradients
        gate = torch.sigmoid(torch.cat(en).detach())
        slope = gate * (1 - gate)
        assert slope.median() > 1e-2 and (slope < 1e-3).double().mean() < 0.01
    ((r1 * c_1).sum() + (r2 * c_2).sum()).backward()

    mod = mod.to(dev())
    load_param_dict(mod, p)
    n1 = fx.p1.n_rows
    for form in ("joint", "split"):
        mod.zero_grad(set_to_none=True)
        gd = [t.detach().float().to(dev()).requires_grad_() for t in (g_1, g_2)]
        if form == "joint":
            Xd = [X.float().to(dev()).requires_grad_()]
            pbd = to_dev(pb)
            at1 = at2 = PackedAtoms(Xd[0], pbd)
        else:
            Xd = [X[:n1].float().to(dev()).requires_grad_(), X[n1:].float().to(dev()).requires_grad_()]
            at1, at2 = PackedAtoms(Xd[0], to_dev(fx.p1)), PackedAtoms(Xd[1], to_dev(fx.p2))
        o1, o2 = mod(at1, gd[0], at2, gd[1])
        close(o1, r1, f"{form} compact_1"); close(o2, r2, f"{form} compact_2")
        ((o1 * c_1.float().to(dev())).sum() + (o2 * c_2.float().to(dev())).sum()).backward()
        dX = torch.cat([x.grad for x in Xd])
        close(dX, Xr.grad, f"{form} dX")
        assert float(dX.cpu()[fx.dead].abs().max()) == 0.0
        for k, (got, want) in enumerate(zip(gd, (g_1, g_2)), 1):
            if want.grad is None:       # Global and Neural ignore the readouts, Alternating g_1 (side 2 asks with compact_1)
                assert got.grad is None or float(got.grad.abs().max()) == 0.0
            else:
                close(got.grad, want.grad, f"{form} dg_{k}")
        grads = grad_dict(mod)
        assert set(grads) == set(p)
        for name, gr in grads.items():
            want = p[name].grad
            # a bias added right before a softmax has an analytically zero gradient (shift invariance): compared on the
            # scale of the weight gradient of the same layer, as in test_gpu_pair.test_coarse_coattention_pair
            floor = p["energy_layers_2/0/W"].grad.abs().max().item() if name == "energy_layers_2/0/b" else 1e-6
            close(gr, want, f"{form} grad {name}", floor=floor)
