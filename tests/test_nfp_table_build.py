"""CPU checks of the tile-table form of the NFP encoder: the new C entries in the header, the ctypes table and the library and
their argument checks (which return before any launch: no GPU is needed), the new translation unit's eight kernels without scratch,
the derived data on the encoder layout in its host form, the formula of the readout on encoder rows against the dense float64
restatement, and the layout check of ``PairBatches``.

The formula (tests/nfp_ref.py is the restatement): a padded position has atom id 0, an empty adjacency row and column and degree
class 0, so it leaves layer l as sigmoid(B_l) whatever the molecule, and for instance i of encoded molecule uid[i]
    g_inst[i] = g_real[uid[i]] + padcount[i] * sum_l softmax(sigmoid(B_l) . Wo_l^T + bo_l).
It is exact: float64 on both sides, 1e-12 of the tensor's max."""
import re
import tempfile

import numpy as np
import pytest
import torch

import nfp_ref as NR
import nfp_tables as NT
from enc_tables import TABLES
from parity_util import close
from table_build import BAD_TABLES, CSRC, P, bad_id, check_table_entries, header_args, lib, resource_usage

TABLE_ENTRIES = ("bmp_nfp_layer_table_fwd", "bmp_nfp_layer_table_bwd", "bmp_nfp_readout_table_fwd", "bmp_nfp_readout_table_bwd")
ENTRIES = ("bmp_nfp_layer_table_supported", "bmp_nfp_readout_table_supported") + TABLE_ENTRIES


def test_header_and_ctypes_table_declare_the_entry_points():
    _l = lib()
    from bmp import functional as Fn
    for name in ENTRIES + ("bmp_nfp_rows_enc", "bmp_nfp_inst_expand", "bmp_nfp_inst_reduce"):
        args = header_args(name)
        assert name in _l.SIGNATURES, name
        assert len(args) == len(_l.SIGNATURES[name][1]), (name, len(args), len(_l.SIGNATURES[name][1]))
        assert hasattr(_l.lib(), name), name
    check_table_entries(TABLE_ENTRIES)
    kern = open(CSRC + "/bmp_kernels.h").read()
    for name in ENTRIES:
        assert re.search(r'extern "C" int %s\s*\(' % name, kern), name
    assert set(Fn.NFP_TABLE_DEFAULT) == {64, 128} and all(type(v) is bool for v in Fn.NFP_TABLE_DEFAULT.values())
    assert Fn.NFP_LAYER_PATHS.keys() == {"fused", "composed"} and callable(Fn.nfp_table_ok)
    assert Fn.NFP_PATHS.keys() == {"layer_tile", "layer_rows", "readout_tile", "readout_rows"}


def test_library_serves_the_widths_of_the_whole_tile_entries():
    L = lib().lib()
    widths = (8, 16, 24, 32, 40, 64, 128, 256)
    assert [d for d in widths if L.bmp_nfp_layer_table_supported(d)] == [64, 128]
    for d in widths:
        for o in (4, 8, 12, 64, 128, 136):
            assert bool(L.bmp_nfp_readout_table_supported(d, o)) == bool(L.bmp_nfp_readout_tile_supported(d, o)), (d, o)
    assert L.bmp_nfp_readout_table_supported(64, 8) and L.bmp_nfp_readout_table_supported(128, 128)


def _calls(L, d=64, o=8, r0=P, nb=P, rows=384, stride=0, n_tiles=3, fv=P, out=P):
    tab = (r0, nb, rows, stride, None)
    return (L.bmp_nfp_layer_table_fwd(P, n_tiles, d, P, P, P, P, P, P, P, fv, out, *tab),
            L.bmp_nfp_layer_table_bwd(P, P, n_tiles, d, P, P, P, P, P, P, P, P, P, *tab),
            L.bmp_nfp_readout_table_fwd(P, n_tiles, d, o, P, P, P, P, P, P, 0, *tab),
            L.bmp_nfp_readout_table_bwd(P, P, P, n_tiles, d, o, P, P, P, P, P, P, P, 1 << 40, *tab))


@pytest.mark.parametrize("bad", BAD_TABLES + [dict(d=32), dict(n_tiles=0)], ids=bad_id)
def test_entries_check_their_arguments_before_any_launch(bad):
    assert all(rc < -1000 for rc in _calls(lib().lib(), **bad)), bad


def test_layer_forward_takes_a_null_fv_only_on_a_table():
    L = lib().lib()
    assert _calls(L, o=12)[2] < -1000 and _calls(L, o=12)[3] < -1000          # a readout width the kernels do not take
    assert _calls(L, fv=P + 4)[0] < -1000 and _calls(L, out=P + 4)[0] < -1000 and _calls(L, out=None)[0] < -1000
    # the whole-tile entry keeps its contract: fv is required there
    assert L.bmp_nfp_layer_tile_fwd(P, 3, 64, P, P, P, P, P, P, P, None, P, None) < -1000


def _kind(name):
    m = re.search(r"k_nfp_(readout_)?(?:table|tile)_(fwd|bwd)ILi(\d+)E", name)
    assert m, name
    return ("readout" if m.group(1) else "layer", m.group(2), m.group(3))


def test_table_kernels_do_not_spill_and_need_no_more_lds_than_the_whole_tile_forms():
    """2 entries x 2 directions x 2 widths = 8 kernels in their own translation unit, none with scratch, each within the 512
    registers a SIMD's lane has for the two waves of a 512-thread workgroup, and their static LDS (the rank block of the layer,
    the row -> molecule block of the readout) at or below the whole-tile form's -- the dynamic part is the same expression in
    both entries (wt_lds_bytes(d); the readout's z tile)."""
    with tempfile.TemporaryDirectory() as tmp:
        names, scratch, vgpr, agpr, occ, lds = resource_usage("bmp_nfp_table.hip", tmp, "--cuda-device-only")
        whole = resource_usage("bmp_nfp.hip", tmp, "--cuda-device-only")
    assert len(names) == len(scratch) == len(vgpr) == len(agpr) == len(occ) == len(lds) == 8, names
    assert sorted(_kind(n) for n in names) == sorted((r, f, d) for r in ("layer", "readout") for f in ("fwd", "bwd") for d in ("64", "128"))
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    for n, v, a, o in zip(names, vgpr, agpr, occ):
        assert v + a <= 256 and o >= 2, (n, v, a, o)
    tile_lds = {_kind(n): l for n, l in zip(whole[0], whole[5]) if "_tile_" in n}
    assert len(tile_lds) == 8, whole[0]
    for n, l in zip(names, lds):
        print(f"[lds] {n}: static {l} B, whole-tile form {tile_lds[_kind(n)]} B")
        assert l <= tile_lds[_kind(n)], (n, l, tile_lds[_kind(n)])
    src = open(CSRC + "/bmp_nfp_table.hip").read()
    assert src.count("wt_lds_bytes(d)") == 2 and src.count("(size_t)WT_R * (d + 4 + NFP_LDZ)") == 1 and src.count("(size_t)WT_R * NFP_LDZ") == 1


# ---- the store, and the derived data on the encoder layout ----
@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_table_of_the_store_holds_every_class(name):
    from bmp.nfp import nfp_derived
    eb = NT.table(name)
    NT.check_classes(eb.pb_enc, nfp_derived(eb.pb_enc, enc=True))
    assert NT.store()[NT.SINGLE].n == 1 and len(NT.store()[NT.SINGLE].bonds) == 0


def _world_batch(which, dedup, n_cu=5):
    from bmp import enclayout, packed
    mols, I1, I2 = NT.world_molecules(which)
    return mols, I1, I2, enclayout.encode_from_store(packed.MolStore(mols), [I1, I2], dedup=dedup, n_cu=n_cu)


@pytest.mark.parametrize("dedup", [False, True], ids=["instances", "dedup"])
@pytest.mark.parametrize("which", ["hand", "single"])
def test_derived_data_on_the_encoder_layout_equals_the_per_instance_batch_atom_by_atom(which, dedup):
    from bmp.nfp import nfp_derived
    mols, I1, I2, eb = _world_batch(which, dedup)
    pe, pi = eb.pb_enc, eb.pb
    ne, ni = nfp_derived(pe, enc=True), nfp_derived(pi)
    assert ne["enc"] and not ni["enc"] and ni["bwd_w"] is pi.row_w
    with pytest.raises(ValueError, match="other row convention"):
        nfp_derived(pe)                                        # the caller says which convention holds; a second one is refused
    rm = pe.row_mol.numpy()
    sw, dc, lw = ne["self_w"].numpy(), ne["deg_class"].numpy(), ne["bwd_w"].numpy()
    assert (sw[rm >= 0] == 1).all() and (sw[rm < 0] == 0).all() and (dc[rm < 0] == 0).all()
    assert (lw[rm != -1] == 1).all() and (lw[rm == -1] == 0).all() and (rm <= -2).any() and (rm == -1).any()
    uid, e0, en = eb.uid.numpy(), eb.enc_row0.numpy(), eb.enc_n.numpy()
    i0 = pi.mol_row0.numpy()
    swi, dci = ni["self_w"].numpy(), ni["deg_class"].numpy()
    seen = np.zeros(pe.n_rows, dtype=bool)
    for i, u in enumerate(uid):
        n = en[u]
        assert n == mols[np.concatenate((I1, I2))[i]].n
        assert (sw[e0[u]:e0[u] + n] == swi[i0[i]:i0[i] + n]).all() and (dc[e0[u]:e0[u] + n] == dci[i0[i]:i0[i] + n]).all()
        assert sw[e0[u] + n - 1] == 1                           # the last real atom is no pad row here
        assert swi[i0[i] + n] == 0 and dci[i0[i] + n] == 0      # ... the per-instance batch has its pad row behind it
        seen[e0[u]:e0[u] + n] = True
    assert (seen == (rm >= 0)).all()
    if which == "single":
        assert 1 in set(dc[rm >= 0])                            # the single-atom molecule: class 1 by its self loop alone


# ---- the formula ----
def _model(p, d, o, layers):
    from bmp.nfp import NFP
    from bmp.snapshot import load_param_dict
    enc = NFP(out_dim=o, hidden_dim=d, n_layers=layers).double()
    load_param_dict(enc, p)
    return enc


@pytest.mark.parametrize("dedup", [False, True], ids=["instances", "dedup"])
@pytest.mark.parametrize("which", ["hand", "single"])
def test_readout_on_encoder_rows_plus_the_pad_term_is_the_dense_readout(which, dedup):
    from bmp.nfp import inst_readout_host, nfp_derived, pad_count
    d, o, layers = 16, 8, 3
    mols, I1, I2, eb = _world_batch(which, dedup)
    if which == "hand":                                        # sides of different padded counts: 127 and 96 positions
        from bmp import enclayout, packed
        I2 = np.where(I2 == 7, 6, I2)
        eb = enclayout.encode_from_store(packed.MolStore(mols), [I1, I2], dedup=dedup, n_cu=5)
    A1, A2 = max(mols[k].n for k in I1), max(mols[k].n for k in I2)
    assert A1 != A2
    pc = pad_count(eb).numpy()
    want = np.concatenate(([A1 - mols[k].n for k in I1], [A2 - mols[k].n for k in I2]))
    assert (pc == want).all() and (pc == 0).any() and (pc > 0).any()
    p = NR.make_nfp_params(7, d, o, layers)
    g_real, h = NR.nfp_forward_packed(p, eb.pb_enc, nfp_derived(eb.pb_enc, enc=True))
    enc = _model(p, d, o, layers)
    with torch.no_grad():
        pad = enc.pad_term()
        g = inst_readout_host(g_real, pad, eb)
    g_ref = torch.cat([NR.nfp_forward(p, *NR.nfp_adj([mols[k] for k in side]))[0] for side in (I1, I2)])
    err = (g - g_ref).abs().max().item()
    print(f"[formula] {which} dedup={dedup}: U = {eb.n_encoded}, rows = {eb.pb_enc.n_rows}, max |g - g_ref| = {err:.3e}")
    close(g, g_ref, "g from encoder rows + pad term vs dense", tol=1e-12)
    B_last = sum(p[f"layers/{layers - 1}/graph_linears/{k}/b"] for k in range(NR.N_DEG))      # (the restatement's order of the sum)
    pads = eb.pb_enc.row_mol.numpy() <= -2
    assert pads.any() and torch.equal(h[torch.from_numpy(pads)], torch.sigmoid(B_last).expand(int(pads.sum()), d))


# ---- refusals ----
def test_check_encoder_accepts_an_nfp_model_and_concat_hidden_still_raises():
    from bmp.nfp import NFP
    from bmp.predictor import build_pair_predictor
    from bmp.trainer import PairBatches
    z = np.zeros(4, dtype=np.int64)
    for attn in (None, "nie"):
        model = build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=3, attn=attn, encoder="nfp")
        assert callable(model.graph_conv.encode_rows) and callable(model.graph_conv.readout_enc)
        assert model.graph_conv.plannable() is False
        for layout, dedup in (("instance", False), ("encoder", False), ("encoder", True), ("static", False)):
            PairBatches(None, z, z, z, 2, layout=layout, dedup=dedup).check_encoder(model)
    with pytest.raises(NotImplementedError, match="concat_hidden"):
        NFP(out_dim=16, hidden_dim=64, concat_hidden=True)
    with pytest.raises(NotImplementedError, match="max_degree"):
        NFP(out_dim=16, hidden_dim=64, max_degree=5)
    with pytest.raises(RuntimeError, match="GPU only"):        # a CPU batch: refused as in forward
        NFP(out_dim=16, hidden_dim=64).encode_rows(NT.table("seven").pb_enc)
    with pytest.raises(NotImplementedError, match="float atom features"):
        NFP(out_dim=16, hidden_dim=64).encode_rows(np.zeros((2, 3, 16), np.float32))
