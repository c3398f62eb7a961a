"""CPU check of the workspace sizes of the fused step / layer weight gradients: bmp_ggnn_step_wgrad_ws_floats and
bmp_relgcn_layer_wgrad_ws_floats must cover the slabs that bmp_launch_wgrad_fused writes for EVERY problem set the call can
build (first or later GGNN call, with or without the row lists).  The plan is restated here (wgrad_fused_plan and the slab
offsets of bmp_launch_wgrad_fused in bmp_gemm.hip; the problem sets of step_wgrad_problems / rel_wgrad_problem in
bmp_fused.hip); the library's sizes are host arithmetic, no GPU call is made."""
import numpy as np
import pytest

TYPE_FRAC = [float(np.float32(f)) for f in (0.78, 0.24, 0.05, 0.58)]
LIVE_FRAC = float(np.float32(0.3))


def _prob(K, Nn, cs=False, zero_only=False, rfrac=None, wrow=False):
    return dict(K=K, Nn=Nn, cs=cs, zero_only=zero_only, rfrac=rfrac, wrow=wrow)


def _step_problems(d, first, lists, live):
    g1 = _prob(d, 2 * d if first else 3 * d)
    g2 = _prob(d, d, zero_only=bool(first))
    if not lists:
        return [_prob(d, 6 * d if first else 7 * d, cs=True), g1, g2]
    g0 = _prob(d, 2 * d if first else 3 * d, cs=True)
    if live and not first:
        g0["rfrac"] = g1["rfrac"] = LIVE_FRAC
    return [g0, g1, g2] + [_prob(d, d, cs=True, rfrac=f) for f in TYPE_FRAC]


def _rel_problems(d, lists):
    if not lists:
        return [_prob(d, 5 * d, cs=True, wrow=True)]
    return [_prob(d, d, cs=True, wrow=True)] + [_prob(d, d, cs=True, rfrac=f) for f in TYPE_FRAC]


def _slab_floats(probs, N):
    """Floats of ws that bmp_launch_wgrad_fused reaches: the zero row, then S x Krows x Nn per problem."""
    tiles = [0 if p["zero_only"] else (p["Nn"] + 127) // 128 for p in probs]
    wtiles = sum(t * (p["rfrac"] if p["rfrac"] is not None else 1.0) for t, p in zip(tiles, probs))
    end = 128
    for p in probs:
        s = int(512.0 / (wtiles if wtiles > 0.0 else 1.0))
        s = max(min(s, max(N // 256, 1)), 1)
        r = (N + s - 1) // s
        r = (r + 31) & ~31
        sfull = (N + r - 1) // r
        if p["zero_only"]:
            S = 0
        elif p["rfrac"] is not None:
            S = min(max(int(sfull * p["rfrac"] + 0.5), 1), sfull)
        else:
            S = sfull
        want_cs = p["cs"] and not p["zero_only"]
        krows = p["K"] + want_cs + (4 if (p["wrow"] and want_cs) else 0)
        end += S * krows * p["Nn"]
    return end


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    return _lib.lib()


@pytest.mark.parametrize("d", [64, 128])
def test_step_and_layer_wgrad_workspace_covers_every_problem_set(L, d):
    for N in range(32, 128 * 640 + 1, 32):
        ws = L.bmp_ggnn_step_wgrad_ws_floats(N, d)
        for first in (0, 1):
            for lists, live in ((False, False), (True, False), (True, True)):
                need = _slab_floats(_step_problems(d, first, lists, live), N)
                assert ws >= need, (N, d, first, lists, live, ws, need)
        ws = L.bmp_relgcn_layer_wgrad_ws_floats(N, d)
        for lists in (False, True):
            need = _slab_floats(_rel_problems(d, lists), N)
            assert ws >= need, (N, d, lists, ws, need)


def test_the_restated_plan_is_the_library_one(L):
    """Against the sizes the library reports: the largest variant, counted with the K + 5 rows per problem that
    bmp_wgrad_fused_ws_floats reserves, is exactly the step's workspace (so the model above is not vacuous)."""
    def reserved(probs, N):
        return _slab_floats([dict(p, K=p["K"] + 5, cs=False, wrow=False) for p in probs], N)
    for d in (64, 128):
        for N in range(32, 128 * 640 + 1, 352):
            want = max(reserved(_step_problems(d, first, lists, live), N)
                       for first in (0, 1) for lists, live in ((False, False), (True, False), (True, True)))
            assert L.bmp_ggnn_step_wgrad_ws_floats(N, d) == want, (N, d)
            want = max(reserved(_rel_problems(d, lists), N) for lists in (False, True))
            assert L.bmp_relgcn_layer_wgrad_ws_floats(N, d) == want, (N, d)
