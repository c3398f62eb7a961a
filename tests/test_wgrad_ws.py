"""CPU check of the workspace sizes of the fused step / layer weight gradients: bmp_ggnn_step_wgrad_ws_floats and
bmp_relgcn_layer_wgrad_ws_floats must cover the slabs that bmp_launch_wgrad_fused writes for EVERY problem set the call can
build (first or later GGNN call, with or without the row lists).  The plan is restated in tests/wgrad_ref.py (wgrad_fused_plan and the slab
offsets of bmp_launch_wgrad_fused in bmp_gemm.hip; the problem sets of step_wgrad_problems / rel_wgrad_problem in
bmp_fused.hip); the library's sizes are host arithmetic, no GPU call is made."""
import pytest

from wgrad_ref import rel_problems as _rel_problems, slab_floats as _slab_floats, step_problems as _step_problems


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
