"""The fused RelGCN layer for d_in != d_out (csrc/bmp_relgcn_rect.hip): one layer against the unfused operators and the float64
restatement of its contract (tests/relgcn_rect_ref.py), the default encoder RelGCN(out_channels=64, scale_adj=True) -- ch_list
[16, 128, 64] -- against the float64 dense oracle, forward-only evaluation, the row lists, tile tables, the layout plan and the
recorded step.

Tolerances, all the project's: ``close`` as it stands (max-norm 1e-4) against float64 and between the fused and the unfused
form, 1e-5 between two float32 runs of the same kernels in two batch layouts (tests/table_harness.py), bit for bit where the same
kernel sums the same rows.  Every test forces ``REL_RECT_DEFAULT`` on: none depends on the measured default.

Batches: the ``pairs`` shape of tests/test_gpu_relgcn.py (40 synthetic molecules of 2 to 30 atoms, 13 pairs, about 3 tiles),
"one_atom" (one molecule of one atom: two rows, the tile's second half empty) and "no_multi" (no double and no triple bond: two
types' blocks are zero in every tile); the two small ones also in the encoder layout, where their tiles are table entries; and
"dense", the harness's one-tile batch of more than FZ_ECAP CSR entries, which the kernels do not stage in LDS."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O                        # noqa: E402
from bmp import synth, packed                          # noqa: E402
from test_gpu_ops import close, dev, to_dev, T         # noqa: E402
import relgcn_rect_ref as RR                           # noqa: E402
import table_harness as H                              # noqa: E402

_CACHE = {}
NAMES = ("out", "dx", "dWT", "dbE", "dWsT", "dbs")


@pytest.fixture
def rect_on(monkeypatch):
    from bmp import functional as Fn
    return H.force_on(monkeypatch, Fn.REL_RECT_DEFAULT)


def _pairs():
    if "store" not in _CACHE:
        store = synth.make_store(40, seed=9, n_lo=2, n_hi=30, n_mean=10)
        rs = np.random.RandomState(2)
        i1, i2 = rs.randint(0, 40, 13), rs.randint(0, 40, 13)
        _CACHE["store"] = (store, i1, i2, packed.pack_from_store(packed.MolStore(store), [i1, i2], device="cpu", with_dense_map=True))
    return _CACHE["store"]


def _host_batch(name):
    """Host PackedMolBatch, adjacency rescaled (models/relgcn.py:20-28): "pairs", "one_atom", "no_multi", and "<small>/table":
    the same molecules in the encoder layout (a tile table)."""
    if name not in _CACHE:
        from bmp import enclayout
        from bmp.relgcn import rescale_adj
        base, _, form = name.partition("/")
        if base == "pairs":
            pb = _pairs()[3]
        elif base == "dense":
            # one four-block tile whose CSR does not fit the kernels' staging in LDS (more than FZ_ECAP entries): the gathers and
            # the type masks walk the global arrays.  As the harness's table entry, and as a whole tile without the table.
            import dataclasses
            pb = H.table("dense").pb_enc
            assert pb.n_rows == 128 and int(pb.csr_ptr[128]) > 1024 and int(pb.csrT_ptr[128]) > 1024
            if form != "table":
                pb = dataclasses.replace(pb, mt_row0=None, mt_nblk=None, n_mtiles=pb.n_tiles, _cache={})
                assert pb.n_mtiles == 1
        else:
            if base == "one_atom":
                store = [synth.Molecule(np.array([6], dtype=np.int32), np.zeros((0, 3), dtype=np.int32))]
            else:
                store = synth.make_store(12, seed=17, n_lo=2, n_hi=30, n_mean=12)
                for m in store:
                    m.bonds[:, 2] = np.where((m.bonds[:, 2] == 1) | (m.bonds[:, 2] == 2), 3, m.bonds[:, 2])
                assert sum(len(m.bonds) for m in store) > 0
            ms, inst = packed.MolStore(store), np.arange(len(store))
            if form == "table":
                pb = enclayout.encode_from_store(ms, [inst], dedup=False, n_cu=4).pb_enc
                assert pb.mt_row0 is not None and pb.tile_stride == 0 and not pb.oversized
                cover = np.zeros(pb.n_rows, dtype=int)
                for a, k in zip(pb.mt_row0.numpy(), pb.mt_nblk.numpy()):
                    cover[a:a + 32 * k] += 1
                assert (cover == 1).all()                # the table's tiles hold every row once
                if base == "one_atom":
                    assert pb.mt_nblk.tolist()[0] == 1
            else:
                pb = packed.pack_from_store(ms, [inst], device="cpu")
                assert pb.mt_row0 is None
            if base == "no_multi":
                assert not np.isin(pb.csr_col.numpy() & 3, (1, 2)).any()
        _CACHE[name] = rescale_adj(pb)
    return _CACHE[name]


def _mol_rows(pb):
    rows = torch.zeros(pb.n_rows, dtype=torch.bool)
    for r0, nr in zip(pb.mol_row0.tolist(), pb.mol_nrows.tolist()):
        rows[r0:r0 + nr] = True                          # rows of no molecule carry unspecified values
    return rows


def _operands(N, d_in, d_out, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s_: torch.randn(*s_, generator=g, dtype=torch.float64) * 0.2
    return dict(x=mk(N, d_in) * 3, WT=mk(4 * d_in, d_out), bE=mk(4, d_out), WsT=mk(d_in, d_out), bs=mk(d_out), cw=mk(N, d_out))


def _run_layer(fn, o, pbd, act):
    from bmp import functional as Fn
    x, WT, bE, WsT, bs = (o[k].float().to(dev()).requires_grad_() for k in ("x", "WT", "bE", "WsT", "bs"))
    y = fn.apply(x, WT, bE, WsT, bs, pbd, Fn.ACT[act])
    (y * o["cw"].float().to(dev())).sum().backward()
    return dict(zip(NAMES, (y.detach(), x.grad, WT.grad, bE.grad, WsT.grad, bs.grad)))


# ---- 6. one layer against the unfused operators and the restatement ----
@pytest.mark.parametrize("batch", ["pairs", "one_atom", "one_atom/table", "no_multi", "no_multi/table", "dense", "dense/table"])
@pytest.mark.parametrize("d_in,d_out,act", [(16, 128, "tanh"), (128, 64, "tanh"), (16, 32, "identity"), (64, 32, "tanh"),
                                            (32, 128, "identity"), (64, 128, "tanh")])
def test_rect_layer_equals_the_unfused_path_and_the_restatement(batch, d_in, d_out, act, rect_on):
    Fn = rect_on
    pbh = _host_batch(batch)
    pbd = to_dev(pbh)
    o = _operands(pbh.n_rows, d_in, d_out, 1000 * d_in + d_out)
    fused = _run_layer(Fn.RelRectLayerFn, o, pbd, act)
    comp = _run_layer(Fn.MsgFn, o, pbd, act)
    adj = torch.from_numpy(H.dense_adj(pbh)[0])
    rows = _mol_rows(pbh)
    # (the cotangent of the rows of no molecule enters the weight gradients of every form alike)
    out64, g64 = RR.layer(o["x"], adj, o["WT"], o["bE"], o["WsT"], o["bs"], act, o["cw"])
    ref = dict(out=out64, **g64)
    for name in NAMES:
        a, b, c = fused[name], comp[name], ref[name]
        if name in ("out", "dx"):
            a, b, c = a[rows.to(dev())], b[rows.to(dev())], c[rows]
        close(a, b, f"{batch} {d_in}->{d_out} {name} vs unfused")
        close(a, c, f"{batch} {d_in}->{d_out} {name} vs float64")
    assert fused["out"][rows.to(dev())].abs().max() > 0 and fused["dWsT"].abs().max() > 0


# ---- 7. the encoder against the float64 dense oracle ----
def _oracle_case(ch_list, out, scale):
    key = ("oracle", tuple(ch_list), out, scale)
    if key not in _CACHE:
        store, i1, i2, _pb = _pairs()
        dr = O._Draw(3, torch.float64, 0.2)
        O.init_relgcn(dr, "", out, ch_list)
        p = {k: v.requires_grad_() for k, v in dr.p.items()}
        a1, j1 = synth.concat_mols([store[k] for k in i1]); a2, j2 = synth.concat_mols([store[k] for k in i2])
        g1, at1 = O.relgcn_forward(p, T(a1), T(j1).double(), len(ch_list) - 1, scale)
        g2, at2 = O.relgcn_forward(p, T(a2), T(j2).double(), len(ch_list) - 1, scale)
        g_ref = torch.cat((g1, g2))
        gen = torch.Generator().manual_seed(5)
        cg = torch.randn(g_ref.shape, dtype=torch.float64, generator=gen); ca = torch.randn(at1.shape, dtype=torch.float64, generator=gen)
        ((g_ref * cg).sum() + 0.1 * (at1 * ca).sum()).backward()
        _CACHE[key] = dict(p={k: v.detach() for k, v in p.items()}, grads={k: v.grad for k, v in p.items()}, g=g_ref.detach(),
                           at1=at1.detach(), at2=at2.detach(), cg=cg, ca=ca)
    return _CACHE[key]


def _encoder_run(enc, pbd, ref, grad=True):
    from bmp.snapshot import grad_dict
    enc.zero_grad()
    g = enc(pbd)
    atoms = enc.get_atom_array()
    a0, a1 = atoms.dense(0), atoms.dense(1)
    if grad:
        ((g * ref["cg"].float().to(dev())).sum() + 0.1 * (a0 * ref["ca"].float().to(dev())).sum()).backward()
    return g.detach(), a0.detach(), a1.detach(), ({k: v.clone() for k, v in grad_dict(enc).items()} if grad else {})


@pytest.mark.parametrize("ch_list,out,scale,layers", [(None, 64, True, 2), ([16, 64, 64, 32], 16, False, 3)])
def test_encoder_matches_dense_oracle_on_the_fused_layers(ch_list, out, scale, layers, rect_on):
    from bmp.relgcn import RelGCN
    from bmp.snapshot import load_param_dict
    Fn = rect_on
    ref = _oracle_case(ch_list or [16, 128, 64], out, scale)
    enc = RelGCN(out_channels=out, ch_list=ch_list, scale_adj=scale).to(dev())
    load_param_dict(enc, ref["p"])
    pbd = to_dev(_pairs()[3])
    (g, a0, a1, grads), tk = H.took(Fn.REL_PATHS, lambda: _encoder_run(enc, pbd, ref))
    assert tk == H.fused(layers), tk                    # every layer fused: 2 of 2, 3 of 3
    close(g, ref["g"], "g"); close(a0, ref["at1"], "atoms 1"); close(a1, ref["at2"], "atoms 2")
    for name, gr in grads.items():
        close(gr, ref["grads"][name], f"grad {name}")


# ---- 8. forward-only evaluation; two runs ----
def test_forward_only_and_two_runs_are_bit_identical(rect_on):
    from bmp.relgcn import RelGCN
    from bmp.snapshot import load_param_dict
    Fn = rect_on
    ref = _oracle_case([16, 128, 64], 64, True)
    enc = RelGCN(out_channels=64, scale_adj=True).to(dev())
    load_param_dict(enc, ref["p"])
    pbd = to_dev(_pairs()[3])
    first = _encoder_run(enc, pbd, ref)
    again = _encoder_run(enc, pbd, ref)
    assert all(torch.equal(a, b) for a, b in zip(first[:3], again[:3]))
    assert sorted(first[3]) == sorted(again[3]) and all(torch.equal(first[3][k], again[3][k]) for k in first[3])
    assert any(v.abs().max() > 0 for v in first[3].values())
    with torch.no_grad():
        (g, a0, a1, _), tk = H.took(Fn.REL_PATHS, lambda: _encoder_run(enc, pbd, ref, grad=False))
    assert tk == H.fused(2)
    assert torch.equal(g, first[0]) and torch.equal(a0, first[1]) and torch.equal(a1, first[2])
    # the layer itself: under no_grad no wdeg is kept and the output is the training forward's
    o = _operands(pbd.n_rows, 16, 128, 7)
    args = [o[k].float().to(dev()) for k in ("x", "WT", "bE", "WsT", "bs")]
    pbs = to_dev(_host_batch("pairs"))
    y_train = Fn.RelRectLayerFn.apply(args[0].clone().requires_grad_(), *args[1:], pbs, Fn.ACT["tanh"])
    with torch.no_grad():
        y_eval = Fn.RelRectLayerFn.apply(*args, pbs, Fn.ACT["tanh"])
    assert torch.equal(y_eval, y_train.detach())


# ---- through the C ABI ----
def _abi_weights(d_in, d_out, seed):
    from bmp.functional import pack_k4, rel_rect_pack_bwd
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    WT, WsT = rnd(4 * d_in, d_out) / d_in ** 0.5, rnd(d_in, d_out) / d_in ** 0.5
    Wnat_p, Ws_p = rel_rect_pack_bwd(WT, WsT)
    return dict(WTp=pack_k4(WT), bE=0.3 * rnd(4, d_out), WsTp=pack_k4(WsT), bs=0.3 * rnd(d_out), Wnat_p=Wnat_p, Ws_p=Ws_p)


def _abi_fwd(d_in, d_out, n_tiles, h, csr, W, out, wdeg, tab=(None, None, 0), act=2):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    check(_lib.lib().bmp_relgcn_rect_fwd(ptr(h), 0, n_tiles, d_in, d_out, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ptr(W["WTp"]), ptr(W["bE"]),
                                         ptr(W["WsTp"]), ptr(W["bs"]), act, ptr(out), ptr(wdeg), *tab, stream()), "bmp_relgcn_rect_fwd")


def _abi_bwd_code(d_in, d_out, n_tiles, dout, out, csrT, W, dh, gda, tab=(None, None, 0), skip=0, act=2):
    from bmp import _lib
    from bmp._lib import ptr, stream
    return _lib.lib().bmp_relgcn_rect_bwd(ptr(dout), ptr(out), act, n_tiles, d_in, d_out, ptr(csrT[0]), ptr(csrT[1]), ptr(csrT[2]),
                                          ptr(W["Wnat_p"]), ptr(W["Ws_p"]), ptr(dh), ptr(gda), *tab, skip, stream())


def _abi_bwd(*a, **kw):
    from bmp._lib import check
    check(_abi_bwd_code(*a, **kw), "bmp_relgcn_rect_bwd")


def _abi_wgrad(d_in, d_out, h, wdeg, gda, lists=(None, None)):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    L = _lib.lib()
    N = h.shape[0]
    f = lambda *s: torch.full(s, float("nan"), device=dev())
    o1, dbE, cs = f(d_in, 5 * d_out), f(4, d_out), f(5 * d_out)
    nws = L.bmp_relgcn_rect_wgrad_ws_floats(N, d_in, d_out)
    ws = torch.empty(max(nws, 4), device=dev())
    check(L.bmp_relgcn_rect_wgrad(ptr(h), ptr(wdeg), ptr(gda), N, d_in, d_out, ptr(o1), ptr(dbE), ptr(cs), 0, ptr(lists[0]), ptr(lists[1]),
                                  ptr(ws), nws, stream()), "bmp_relgcn_rect_wgrad")
    torch.cuda.synchronize()
    return dict(o1=o1, dbE=dbE, cs=cs)


# ---- 9. the row lists ----
def test_row_lists_and_the_refused_skip(rect_on):
    """(128, 64): gda prefilled with NaN and skip_zero_g = 1 -- the blocks of rows without a bond of the type stay NaN -- and the
    weight gradients through the row lists are finite and equal the all-rows launch on the fully written gda.  (16, 128): the
    weight gradients read every row, so skip_zero_g = 1 is an error and nothing is launched."""
    from bmp import _lib
    Fn = rect_on
    pbd = to_dev(_host_batch("pairs"))
    N, nt = pbd.n_rows, pbd.n_tiles
    csr, csrT = (pbd.csr_ptr, pbd.csr_col, pbd.csr_val), (pbd.csrT_ptr, pbd.csrT_col, pbd.csrT_val)
    L = _lib.lib()
    d_in, d_out = 128, 64
    assert L.bmp_relgcn_rect_lists_used(N, d_in, d_out) and not L.bmp_relgcn_rect_lists_used(N, 16, 128)
    W = _abi_weights(d_in, d_out, 3)
    g = torch.Generator().manual_seed(8)
    h, dout = torch.randn(N, d_in, generator=g).to(dev()), torch.randn(N, d_out, generator=g).to(dev())
    out, wdeg = torch.empty(N, d_out, device=dev()), torch.empty(N, 4, device=dev())
    _abi_fwd(d_in, d_out, nt, h, csr, W, out, wdeg)
    res = {}
    tri, trc = Fn.type_rows(pbd)
    assert tri is not None
    for skip, lists in ((0, (None, None)), (1, (tri, trc))):
        dh = torch.full((N, d_in), float("nan"), device=dev())
        gda = torch.full((N, 5 * d_out), float("nan"), device=dev())
        _abi_bwd(d_in, d_out, nt, dout, out, csrT, W, dh, gda, skip=skip)
        res[skip] = dict(_abi_wgrad(d_in, d_out, h, wdeg, gda, lists), dh=dh, gda=gda)
    assert torch.isfinite(res[0]["gda"]).all() and torch.isnan(res[1]["gda"]).any()       # the skip left blocks unwritten
    assert torch.equal(res[0]["dh"], res[1]["dh"])
    for k in ("o1", "dbE", "cs"):
        assert torch.isfinite(res[1][k]).all(), k
        close(res[1][k], res[0][k], f"row lists: {k} vs the all-rows launch")
    # a pair whose weight gradients read every row
    W = _abi_weights(16, 128, 4)
    dout, out = torch.randn(N, 128, generator=g).to(dev()), torch.tanh(torch.randn(N, 128, generator=g)).to(dev())
    dh, gda = torch.full((N, 16), float("nan"), device=dev()), torch.full((N, 640), float("nan"), device=dev())
    assert _abi_bwd_code(16, 128, nt, dout, out, csrT, W, dh, gda, skip=1) != 0
    torch.cuda.synchronize()
    assert torch.isnan(dh).all() and torch.isnan(gda).all()                                # nothing was launched
    assert _abi_bwd_code(16, 128, nt, dout, out, csrT, W, dh, gda, skip=0) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dh).all() and torch.isfinite(gda).all()


# ---- 10. tile tables ----
def _pair_model():
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.relgcn import RelGCN
    torch.manual_seed(5)
    return GraphConvPredictorForPair(RelGCN(out_channels=64, scale_adj=True), None, build_link_predictor("mlp", 64, 1)).to(dev())


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (True, 5)])
def test_default_encoder_trains_in_the_encoder_layout(dedup, n_cu, rect_on):
    Fn = rect_on
    model = _pair_model()
    H.encoder_layout_against_per_instance(H.world("hand"), model, Fn.REL_PATHS, f"relgcn rect dedup={dedup} n_cu={n_cu}", dedup, n_cu,
                                          H.fused(2), atoms=model.graph_conv.get_atom_array, nonzero="graph_conv/rgcn_convs")


@pytest.mark.parametrize("ns", sorted(H.STRIDE_BLOCKS))
@pytest.mark.parametrize("d_in,d_out", [(16, 128), (128, 64), (64, 32)])
def test_table_of_1_to_4_live_blocks_gives_the_whole_tile_result(d_in, d_out, ns):
    """Three tiles at rows 0, 128, 256 with 1, 2, 3 / 1, 3, 4 live blocks: the dead rows of h, dout and out are NaN (never read),
    every written array is prefilled with NaN and has a 128-row NaN canary behind mt_rows.  The live rows equal, bit for bit,
    the whole-tile launch on the same molecules (dead rows zero there); dead rows and canary stay NaN.  The new entries refuse
    the bad tables of the harness that their arguments can express (they take no stride: dense rows only)."""
    from bmp._lib import ptr
    N = H.STRIDE_ROWS
    csr, csrT, r0, nb, live = H.stride_case(ns)
    W = _abi_weights(d_in, d_out, 11)
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    h, dout = rnd(N, d_in), rnd(N, d_out)
    zero_dead = lambda x, live_: torch.where(live_[:, None], x, torch.zeros_like(x))
    res = {}
    for form, tab, dead in (("table", (ptr(r0), ptr(nb), N), H.nan_dead), ("whole", (None, None, 0), zero_dead)):
        out, wdeg, dh, gda = H.nan_rows(d_out), H.nan_rows(4), H.nan_rows(d_in), H.nan_rows(5 * d_out)
        _abi_fwd(d_in, d_out, 3, dead(h, live), csr, W, out, wdeg, tab)
        torch.cuda.synchronize()
        res[form] = dict(out=out.clone(), wdeg=wdeg)
        out[:N] = dead(out[:N], live)
        _abi_bwd(d_in, d_out, 3, dead(dout, live), out, csrT, W, dh, gda, tab)
        torch.cuda.synchronize()
        res[form].update(dh=dh, gda=gda)
    for k, x in res["table"].items():
        assert torch.isnan(x[N:]).all() and torch.isnan(res["whole"][k][N:]).all(), k          # the canary behind mt_rows
        assert torch.isnan(x[:N][~live]).all(), k                                               # no dead row is written
        assert torch.isfinite(x[:N][live]).all(), k
        assert torch.equal(x[:N][live], res["whole"][k][:N][live]), (k, (x[:N][live] - res["whole"][k][:N][live]).abs().max().item())
        assert x[:N][live].abs().max() > 0, k
    out, wdeg, dh, gda = (torch.empty(N, w, device=dev()) for w in (d_out, 4, d_in, 5 * d_out))
    for bad in H.bad_tables(r0, nb):
        if bad[3] != 0:
            continue                                     # (a stride: not an argument of these entries)
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_fwd(d_in, d_out, 3, h, csr, W, out, wdeg, bad[:3])
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_bwd(d_in, d_out, 3, dout, res["whole"]["out"][:N].contiguous(), csrT, W, dh, gda, bad[:3])


# ---- 11. the layout plan and the recorded step ----
def test_planned_step_equals_eager_step(rect_on):
    """tests/test_plan.py::test_planned_step_equals_eager_step for the default RelGCN + MLP model."""
    from bmp.dp import FlatAdam
    Fn = rect_on
    store = synth.make_store(40, seed=3, n_lo=4, n_hi=40, n_mean=14)
    i1, i2 = np.arange(0, 16), np.arange(16, 32)
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev())
    t = (torch.arange(16, device=dev()) % 2).int().view(-1, 1)
    model = _pair_model()
    y, tk = H.took(Fn.REL_PATHS, lambda: model(pb))
    assert tk == H.fused(2), tk
    model.loss(y, t).backward()
    eager = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in model.parameters()]).clone()
    y_eager = y.detach().clone()
    opt = FlatAdam(model, alpha=1e-3)
    y2, tk = H.took(Fn.REL_PATHS, lambda: opt.functional_forward(pb))
    assert tk == H.fused(2), tk
    assert opt.plan is not None and {"c0.o1", "c1.o1"} <= set(opt.plan.G["graph_conv."]) and "c0.dWT" not in opt.plan.G["graph_conv."]
    model.loss(y2, t).backward()
    opt.collect_grads()
    assert torch.equal(y2.detach(), y_eager)
    scale = eager.abs().max().item()
    assert scale > 0 and (opt.grad - eager).abs().max().item() <= 1e-5 * scale
    # a plan keeps the forms it was built with: the switch turned off afterwards changes nothing for this optimizer
    for key in Fn.REL_RECT_DEFAULT:
        Fn.REL_RECT_DEFAULT[key] = False                 # (the fixture's monkeypatch puts the entries back)
    y3, tk = H.took(Fn.REL_PATHS, lambda: opt.functional_forward(pb))
    assert tk == H.fused(2), tk
    model.loss(y3, t).backward()
    opt.collect_grads()
    assert torch.equal(y3.detach(), y_eager) and (opt.grad - eager).abs().max().item() <= 1e-5 * scale


def test_planned_layer_keeps_no_wdeg_under_no_grad(rect_on, monkeypatch):
    """A stack with an unfused layer hands the planned rectangular layer no buffers: it allocates its own, and under no_grad
    without the backward's wdeg; the output is the training forward's bit for bit."""
    Fn = rect_on
    pbs = to_dev(_host_batch("pairs"))
    d_in, d_out = 128, 64
    o = _operands(pbs.n_rows, d_in, d_out, 21)
    WT, bE, WsT, bs = (o[k].float().to(dev()) for k in ("WT", "bE", "WsT", "bs"))
    Wnat_p, Ws_p = Fn.rel_rect_pack_bwd(WT, WsT)
    W = dict(WTp=Fn.pack_k4(WT), bE=bE, WsTp=Fn.pack_k4(WsT), bs=bs, Wnat_p=Wnat_p, Ws_p=Ws_p)
    G = dict(o1=torch.empty(d_in, 5 * d_out, device=dev()), dbE=torch.empty(4, d_out, device=dev()), cs=torch.empty(5 * d_out, device=dev()))
    made = []
    real = Fn.rel_buffers
    monkeypatch.setattr(Fn, "rel_buffers", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    x = o["x"].float().to(dev())
    y_train = Fn.PRelRectLayerFn.apply(x.clone().requires_grad_(), pbs, W, G, {}, "c1", Fn.ACT["tanh"])
    with torch.no_grad():
        y_eval = Fn.PRelRectLayerFn.apply(x, pbs, W, G, {}, "c1", Fn.ACT["tanh"])
    assert len(made) == 2 and made[0][1] is not None and made[1][1] is None
    assert torch.equal(y_eval, y_train.detach()) and y_eval.abs().max() > 0


def test_static_batch_recorded_step_replays_the_fused_layers(rect_on):
    Fn = rect_on
    H.static_recorded_step_replays_on_the_table_kernels(_pair_model, Fn.REL_PATHS, "relgcn rect")
