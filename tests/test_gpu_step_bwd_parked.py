"""The GGNN step backward (`bmp_ggnn_step_bwd`, k_ggnn_step_bwd) with the direct part of dh parked in the dh rows: a later
call's threads store `ex = dh' (1 - z) + d(r*h) r` into dh after the da_r phase and load the same 16-byte pieces back in the
epilogue, so dh is written twice and read once by the launch that produces it.

Every case goes through the C entry and checks
  * dh and every written block of gda against a float64 evaluation of the step backward (2e-5 of the tensor's max-abs, the
    bound of the fused step everywhere else in the suite), on the rows of the tiles' live blocks;
  * two launches on the same inputs, dh and gda prefilled with NaN before each, for exact equality: a thread that read a dh
    piece it had not written itself would return the prefill;
  * on a tile table at a fixed stride: the rows of a tile's other blocks are exact zeros in dh and gda (they are cleared, and
    never read back as ex), the inputs' rows there are NaN (never read), and the canary behind the last tile stays NaN.

Shapes: d = 128 (2 x 4 waves, two row blocks per wave) and d = 64 (4 x 2 waves, one), first and later call; one whole tile and
two; random molecules of 3-40 atoms, one of them across row 64 of its tile (the transposed gather crosses the two wave groups); a
table of tiles with 1, 2, 3 and 4 live blocks (a dead second group, a group with one live block of two, slots that neither store
nor reload); the same four heights at the fixed stride 128 with one molecule per tile; skip_zero_g off and on (on: a G_e block
is compared where the row has a bond of type e, the others are not written).

dh and dhout are never one buffer in the library's callers (bmp/functional.py allocates dh per call), so that case is not run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from parity_util import close              # noqa: E402

TOL = 2e-5
CANARY = 128
LAYOUTS = ("one_tile", "two_tiles", "table", "stride")
HEIGHTS = [1, 2, 3, 4]                      # live 32-row blocks of the table's and the stride case's tiles
STRIDE_ATOMS = [20, 40, 70, 120]            # one molecule per tile at the fixed stride: 1, 2, 3 and 4 live blocks
_CACHE = {}


def dev():
    assert torch.cuda.is_available(), "GPU test selected without a GPU"
    return torch.device("cuda:0")


def _molecule(rs, row0, n):
    """Directed entries (row, other, type, value) of one molecule on rows [row0, row0 + n): a chain plus a few ring closures,
    bond types drawn like the DDI batches' (single .55, double .10, triple .01, aromatic .34), both directions with values
    of their own."""
    bonds = [(i, i + 1) for i in range(n - 1)] + [(int(a), int(b)) for a, b in rs.randint(0, n, (n // 4, 2)) if abs(a - b) > 1]
    ent = []
    for a, b in bonds:
        e = int(rs.choice(4, p=[.55, .10, .01, .34]))
        ent.append((row0 + a, row0 + b, e, rs.uniform(.2, 1.)))
        ent.append((row0 + b, row0 + a, e, rs.uniform(.2, 1.)))
    return ent


def _fill(rs, row0, rows, ent, spans):
    """Random molecules of 3-40 atoms on rows [row0, row0 + rows), packed one behind the other."""
    at = 0
    while rows - at >= 3:
        n = min(int(rs.randint(3, 41)), rows - at)
        ent += _molecule(rs, row0 + at, n)
        spans.append((at, at + n))
        at += n


def layout(name):
    """(N rows, tile row0s, live blocks per tile, table or None, stride, entries) of one of LAYOUTS; built once."""
    if name not in _CACHE:
        rs = np.random.RandomState(dict(one_tile=11, two_tiles=12, table=13, stride=14)[name])
        ent, spans = [], []
        if name in ("one_tile", "two_tiles"):
            nt = 1 if name == "one_tile" else 2
            row0, nblk, tab, stride = [128 * t for t in range(nt)], [4] * nt, False, 0
            for t in range(nt):
                _fill(rs, 128 * t, 128, ent, spans)
            assert any(a < 64 < b for a, b in spans), spans        # a molecule across the two halves of a tile
        elif name == "table":
            nblk, tab, stride = HEIGHTS, True, 0
            row0 = np.concatenate(([0], np.cumsum(32 * np.array(nblk))[:-1])).tolist()       # the tiles abut
            for r0, k in zip(row0, nblk):
                _fill(rs, r0, 32 * k, ent, spans)
        else:
            nblk, tab, stride = HEIGHTS, True, 128
            row0 = [128 * t for t in range(4)]
            assert [(n + 31) // 32 for n in STRIDE_ATOMS] == nblk
            for r0, n in zip(row0, STRIDE_ATOMS):
                ent += _molecule(rs, r0, n)
        N = 128 * len(row0) if stride or not tab else 32 * sum(nblk)
        live = np.zeros(N, dtype=bool)
        tile_of = np.full(N, -1)
        for t, (r0, k) in enumerate(zip(row0, nblk)):
            live[r0:r0 + 32 * k] = True
            tile_of[r0:r0 + 32 * k] = t
        assert all(tile_of[r] >= 0 and tile_of[r] == tile_of[o] for r, o, _, _ in ent)       # bonds inside a tile's live blocks
        assert {e for _, _, e, _ in ent} >= {0, 1, 3}               # a rare type among them: the type-sorted row order moves rows
        _CACHE[name] = dict(N=N, row0=row0, nblk=nblk, tab=tab, stride=stride, ent=ent, live=live)
    return _CACHE[name]


def operands(name, d, first):
    """Inputs of one (layout, d, first), float64 on the host, and the float64 result; built once and never changed."""
    key = (name, d, first)
    if key not in _CACHE:
        lay = layout(name)
        N = lay["N"]
        g = torch.Generator().manual_seed(1000 * d + 10 * LAYOUTS.index(name) + first)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        dhout, h = rnd(N, d), rnd(N, d)
        rz, c = torch.sigmoid(rnd(N, 2 * d)), torch.tanh(rnd(N, d))
        WT, AT, UcT = rnd(4 * d, d) / d ** .5, rnd(2 * d, 3 * d) / d ** .5, rnd(d, d) / d ** .5
        # float32 values, so that the float64 evaluation starts from what the kernel reads
        dhout, h, rz, c, WT, AT, UcT = (t.float().double() for t in (dhout, h, rz, c, WT, AT, UcT))
        ent = lay["ent"]
        ent = sorted(ent, key=lambda t: (t[0], t[1], t[2]))
        val = np.array([v for *_, v in ent], dtype=np.float32)
        S = torch.zeros(4, N, N, dtype=torch.float64)
        has = torch.zeros(N, 4, dtype=torch.bool)
        for (r, o, e, _), v in zip(ent, val):
            S[e, r, o] += float(v)
            has[r, e] = True
        # ---- the step backward in float64 (the kernel's head comment names the terms) ----
        r, z = rz[:, :d], rz[:, d:]
        dac = dhout * z * (1 - c * c)
        Ah, Am = AT[:d], AT[d:]                                   # [h ; m] rows, [r | z | c] columns
        dh, dm = dac @ Ah[:, 2 * d:].T, dac @ Am[:, 2 * d:].T
        if first:
            daz, dar = dhout * c * z * (1 - z), None
        else:
            daz = dhout * (c - h) * z * (1 - z)
            drh = dac @ UcT.T
            dar = drh * h * r * (1 - r)
            dh = dh + dar @ Ah[:, :d].T + dhout * (1 - z) + drh * r
            dm = dm + dar @ Am[:, :d].T
        dh, dm = dh + daz @ Ah[:, d:2 * d].T, dm + daz @ Am[:, d:2 * d].T
        G = [S[e] @ dm for e in range(4)]
        for e in range(4):
            dh = dh + G[e] @ WT[e * d:(e + 1) * d].T
        ptr_ = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(np.bincount([t[0] for t in ent], minlength=N), out=ptr_[1:])
        _CACHE[key] = dict(dhout=dhout, h=h, rz=rz, c=c, WT=WT, AT=AT, UcT=UcT, dh=dh, G=G, dar=dar, daz=daz, dac=dac, has=has,
                           ptr=torch.from_numpy(ptr_.astype(np.int32)),
                           col=torch.tensor([(o << 2) | e for _, o, e, _ in ent], dtype=torch.int32), val=torch.from_numpy(val))
    return _CACHE[key]


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("first", [0, 1], ids=["later", "first"])
@pytest.mark.parametrize("d", [128, 64])
def test_step_backward_with_parked_dh(d, first, name):
    from bmp import functional as Fn
    from bmp._lib import check, lib, ptr, stream
    L = lib()
    lay, op = layout(name), operands(name, d, first)
    N, live = lay["N"], torch.from_numpy(lay["live"])
    f32 = lambda t: t.float().to(dev()).contiguous()
    # the rows outside the tiles' live blocks (the stride case has them) are never read: NaN
    rows_in = lambda t: f32(torch.where(live[:, None], t, torch.full_like(t, float("nan"))))
    dhout, h, rz, c = (rows_in(op[k]) for k in ("dhout", "h", "rz", "c"))
    Wnat, A, Uc = (Fn.pack_k4(f32(op[k]).t()) for k in ("WT", "AT", "UcT"))
    cptr, ccol, cval = op["ptr"].to(dev()), op["col"].to(dev()), op["val"].to(dev())
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev())
    r0, nb = (i32(lay["row0"]), i32(lay["nblk"])) if lay["tab"] else (None, None)

    def launch(skip):
        dh = torch.full((N + CANARY, d), float("nan"), device=dev())
        gda = torch.full((N + CANARY, 7 * d), float("nan"), device=dev())
        check(L.bmp_ggnn_step_bwd(ptr(dhout), ptr(h), ptr(rz), ptr(c), len(lay["row0"]), d, first, ptr(cptr), ptr(ccol), ptr(cval),
                                  ptr(Wnat), ptr(A), ptr(Uc), ptr(dh), ptr(gda), ptr(r0), ptr(nb), N, lay["stride"], skip, stream()),
              "bmp_ggnn_step_bwd")
        torch.cuda.synchronize()
        return dh.cpu(), gda.cpu()

    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=4242.0), torch.nan_to_num(b, nan=4242.0)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))
    for skip in (0, 1):
        tag = f"d {d} {'first' if first else 'later'} {name} skip {skip}"
        dh, gda = launch(skip)
        dh2, gda2 = launch(skip)
        assert same(dh, dh2) and same(gda, gda2), f"{tag}: two launches differ"
        assert torch.isnan(dh[N:]).all() and torch.isnan(gda[N:]).all(), f"{tag}: rows behind the last tile written"
        dh, gda = dh[:N], gda[:N]
        close(dh[live], op["dh"][live], f"{tag}: dh", tol=TOL)
        blocks = [("da_c", 6, op["dac"]), ("da_z", 5, op["daz"])] + ([] if first else [("da_r", 4, op["dar"])])
        for nm, k, want in blocks:
            close(gda[live][:, k * d:(k + 1) * d], want[live], f"{tag}: gda {nm}", tol=TOL)
        for e in range(4):
            rows = live & op["has"][:, e] if skip else live
            scale = max(op["G"][e][live].abs().max().item(), 1e-6)          # of the whole block, whichever rows are written
            close(gda[rows][:, e * d:(e + 1) * d], op["G"][e][rows], f"{tag}: gda G_{e}", tol=TOL, floor=scale)
        if first:                                     # (the first call writes no da_r, bmp_ggnn_step_wgrad reads none)
            assert torch.isnan(gda[live][:, 4 * d:5 * d]).all(), tag
        if lay["stride"]:
            assert not live.all()
            assert (dh[~live] == 0).all() and (gda[~live] == 0).all(), f"{tag}: a cleared row is not zero"
        assert dh[live].abs().max() > 0
