"""CPU checks of the rectangular fused RelGCN layer (csrc/bmp_relgcn_rect.hip): the support table and the C ABI's new symbols,
the layout plan's shapes and tables for the default stack [16, 128, 64], the float64 restatement of the kernel contract
(tests/relgcn_rect_ref.py) against autograd of the reference's order, and zero scratch in every kernel of the file.
The tests that need the rectangular form in the plan force ``REL_RECT_DEFAULT`` on: they do not depend on the measured default."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

import relgcn_rect_ref as RR
import table_harness as H
from bmp.plan import LayoutPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = {(16, 32), (16, 64), (16, 128), (32, 64), (32, 128), (64, 32), (64, 128), (128, 32), (128, 64)}
NEW = ("bmp_relgcn_rect_supported", "bmp_relgcn_rect_lists_used", "bmp_relgcn_rect_fwd", "bmp_relgcn_rect_bwd",
       "bmp_relgcn_rect_wgrad_ws_floats", "bmp_relgcn_rect_wgrad")


@pytest.fixture
def rect_on(monkeypatch):
    from bmp import functional as Fn
    return H.force_on(monkeypatch, Fn.REL_RECT_DEFAULT)


def test_support_table_and_new_symbols():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    from bmp import functional as Fn
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmp.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    L = _lib.lib()
    widths = (8, 16, 24, 32, 64, 128, 256)
    assert {(a, b) for a in widths for b in widths if L.bmp_relgcn_rect_supported(a, b)} == NINE
    assert {(a, b) for a in widths for b in widths if L.bmp_relgcn_layer_supported(a, b)} == {(64, 64), (128, 128)}
    assert set(Fn.REL_RECT_DEFAULT) == NINE == set(Fn.REL_RECT_PAIRS)
    # the row lists are the licence of the pairs whose weight gradients come from the fused launch, and of no other
    for a, b in NINE:
        assert bool(L.bmp_relgcn_rect_lists_used(384, a, b)) == (a >= 64 and b >= 64), (a, b)
        assert L.bmp_relgcn_rect_wgrad_ws_floats(384, a, b) > 0
    assert not L.bmp_relgcn_rect_lists_used(384 + 8, 128, 64) and not L.bmp_relgcn_rect_lists_used(384, 64, 64)


def test_plan_shapes_of_the_default_stack(rect_on):
    from bmp.relgcn import RelGCN
    enc = RelGCN(out_channels=64)
    assert [enc._fused(l) for l in range(2)] == ["rect", "rect"]
    spec = enc.gk_spec()
    assert spec["c0.o1"] == (16, 640) and spec["c0.dbE"] == (4, 128) and spec["c0.cs"] == (640,) and spec["c1.o1"] == (128, 320)
    assert spec["c1.dbE"] == (4, 64) and spec["c1.cs"] == (320,)
    assert "c0.dWT" not in spec and "c1.dWT" not in spec
    with torch.no_grad():
        P = enc.prepared_layouts()
    # K4 packs; the backward's operands of the 16-wide layer padded to 32 output columns per block
    assert tuple(P["c0.WTp"].shape) == (16, 128, 4) and tuple(P["c0.WsTp"].shape) == (4, 128, 4)
    assert tuple(P["c0.Wnat_p"].shape) == (32, 128, 4) and tuple(P["c0.Ws_p"].shape) == (32, 32, 4)
    assert tuple(P["c1.Wnat_p"].shape) == (16, 512, 4) and tuple(P["c1.Ws_p"].shape) == (16, 128, 4)
    mixed = RelGCN(out_channels=16, ch_list=[16, 64, 64, 32])
    assert [mixed._fused(l) for l in range(3)] == ["rect", "square", "rect"]


def test_switch_off_keeps_the_unfused_plan(monkeypatch):
    from bmp import functional as Fn
    from bmp.relgcn import RelGCN
    for key in Fn.REL_RECT_DEFAULT:
        monkeypatch.setitem(Fn.REL_RECT_DEFAULT, key, False)
    enc = RelGCN(out_channels=64)
    assert [enc._fused(l) for l in range(2)] == [None, None]
    assert enc.gk_spec()["c0.dWT"] == (64, 128) and "c0.o1" not in enc.gk_spec()


def test_backward_pack_pads_the_16_wide_blocks():
    from bmp.functional import rel_rect_pack_bwd
    g = torch.Generator().manual_seed(2)
    for d_in, d_out in ((16, 32), (32, 64), (64, 32)):
        WT, WsT = torch.randn(4 * d_in, d_out, generator=g), torch.randn(d_in, d_out, generator=g)
        Wn_p, Ws_p = rel_rect_pack_bwd(WT, WsT)
        dip = max(d_in, 32)
        unpack = lambda Wp: Wp.permute(0, 2, 1).reshape(d_out, -1)          # [K/4][N][4] -> [K x N]
        Wn, Ws = unpack(Wn_p).reshape(d_out, 4, dip), unpack(Ws_p)
        assert torch.equal(Ws[:, :d_in], WsT.t()) and (Ws[:, d_in:] == 0).all()
        for e in range(4):
            assert torch.equal(Wn[:, e, :d_in], WT[e * d_in:(e + 1) * d_in].t()) and (Wn[:, e, d_in:] == 0).all()


@pytest.mark.parametrize("ch_list,out", [([16, 128, 64], 64), ([16, 64, 64, 32], 16)])
def test_plan_tables_match_layout_code(ch_list, out, rect_on):
    """The two checks of tests/test_plan.py::test_plan_tables_match_layout_code for the stacks that change width."""
    from bmp.relgcn import RelGCN
    torch.manual_seed(11)
    rel = RelGCN(out_channels=out, ch_list=ch_list)
    assert all(rel._fused(l) for l in range(len(ch_list) - 1))
    with torch.no_grad():
        for p in rel.parameters():
            p.copy_(torch.randn_like(p))
    mods = [("rel.", rel)]
    names = ["rel." + n for n, _ in rel.named_parameters()]
    shapes = [tuple(p.shape) for p in rel.parameters()]
    flat = torch.cat([p.detach().reshape(-1) for p in rel.parameters()])
    plan = LayoutPlan(mods, names, shapes, "cpu")
    plan.prepare(flat)                                   # (i) prepare == the layout functions, bit for bit
    with torch.no_grad():
        ref = rel.prepared_layouts()
    assert set(ref) == set(plan.P["rel."])
    for k, v in ref.items():
        assert torch.equal(plan.P["rel."][k], v.contiguous()), k
    plan.gk.copy_(torch.randn_like(plan.gk))             # (ii) collect == autograd through primary_layouts
    got = torch.zeros_like(flat)
    plan.collect(got)
    params = list(rel.parameters())
    prim = rel.primary_layouts()
    pg = rel.primary_grads(plan.G["rel."])
    loss = sum((prim[k] * t).sum() for k in prim for t in pg[k])
    gs = torch.autograd.grad(loss, params, allow_unused=True)
    want = torch.cat([(g if g is not None else torch.zeros_like(p)).reshape(-1) for g, p in zip(gs, params)])
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6), (got - want).abs().max()


@pytest.mark.parametrize("act", ["tanh", "identity"])
@pytest.mark.parametrize("d_in,d_out", [(16, 32), (32, 16)])
def test_restatement_equals_autograd_of_the_reference_order(d_in, d_out, act):
    """3 molecules of 1, 2 and 5 atoms, dense adjacency: the kernel contract restated in float64 (gather first; G_e, gda, o1,
    dbE, cs and the slicing) against torch autograd of adj_e @ (h W_e^T + b_e) plus the self term, to 1e-12."""
    adj = RR.molecules_adj((1, 2, 5), seed=4)
    N = adj.shape[1]
    assert N == 8 and (adj[:, 0] == 0).all() and (adj[:, :, 0] == 0).all()        # the one-atom molecule has no bond
    g = torch.Generator().manual_seed(100 * d_in + d_out)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    ops = dict(h=r(N, d_in), WT=r(4 * d_in, d_out) / d_in ** 0.5, bE=0.3 * r(4, d_out), WsT=r(d_in, d_out) / d_in ** 0.5, bs=0.3 * r(d_out))
    cot = r(N, d_out)
    out, got = RR.layer(ops["h"], adj, ops["WT"], ops["bE"], ops["WsT"], ops["bs"], act, cot)
    q = {k: v.clone().requires_grad_() for k, v in ops.items()}
    ref = RR.reference_order(q["h"], adj, q["WT"], q["bE"], q["WsT"], q["bs"], act)
    (ref * cot).sum().backward()
    tol = lambda a, b, name: (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1.0) or pytest.fail(name)
    tol(out, ref.detach(), "out")
    for name, key in (("dx", "h"), ("dWT", "WT"), ("dbE", "bE"), ("dWsT", "WsT"), ("dbs", "bs")):
        tol(got[name], q[key].grad, name)


def test_rect_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_relgcn_rect.hip"), "-o", os.path.join(tmp, "rect.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 36, names       # nine pairs x forward and backward x whole tiles and tile table
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
