"""The round order of the pipelined forward update (k_gs_update_fwd<KT, S, true>): the dots of a tile run one round after its product, in
the shadow of the next store drain, from a panel that stays in registers one round longer; the panel in LDS comes back and the new one goes there in front
of the drain; the last columns of the next tile's panel are issued behind the neighbour loads, which ask out of range in a round whose poll did not match.
What that adds to the states of test_gpu_step_forward_pipeline.py: a tile's dots that are still pending when the loop ends, when the workgroup has no further
tile, when its publisher lags or when the workgroup goes dead; a panel that is one tile behind the rows it is multiplied with; a single-row tile whose one
y waits a round for its dots.

Method, helpers and checks are those of test_gpu_step_forward.py and test_gpu_step_forward_pipeline.py: 31 Lanczos steps with the form on against the same
run with KS_DEBUG_NO_STEP_FORWARD, storage pre-filled with 0xFF bytes and guard rows checked, a forced grid of 4 workgroups (_forced_grid_checks: the
stored columns keep their bits, T and beta to 1e-12, the Lanczos relation, an orthonormal basis; bytes where the grid holds every tile)."""
import numpy as np
import pytest

from test_gpu_step_forward import _band5, _run
from test_gpu_step_forward_pipeline import DEPTH_G, DEPTH_N, M, _forced_grid_checks, _off, _took_every_launch

pytestmark = pytest.mark.gpu

# 1, 3 and 5 tiles on 4 workgroups: workgroups without a tile, with one tile (its dots run behind the loop) and with two
EMPTY_N = [512 * 1, 512 * 3, 512 * 5]
# the odd last row as a workgroup's only tile (513: workgroup 1; 512 * 4 + 1: workgroup 0's second tile behind a full first round is the single row),
# as its last tile (512 * 7 + 1: workgroup 3) and as its last tile behind a full round of every workgroup (512 * 8 + 1: workgroup 0's third)
LAST_ROW_N = [513, 512 * 4 + 1, 512 * 7 + 1, 512 * 8 + 1]


def _band5_off(ks, ctx, debug, n):
    return _off(ks, ctx, debug, ("band5", n), lambda ks, ctx: _band5(ks, ctx, n))


@pytest.mark.parametrize("n", EMPTY_N + LAST_ROW_N)
def test_pending_dots_at_the_end_of_the_loop(ctx, debug, n):
    import slepc_amd as ks
    A, v0, off = _band5_off(ks, ctx, debug, n)
    on = _run(ks, ctx, debug, A, v0, M, True, grid=DEPTH_G)
    _took_every_launch(on["stats"])
    _forced_grid_checks(A, off, on, DEPTH_G)


@pytest.mark.parametrize("n", DEPTH_N)
def test_a_lagging_publisher_meets_pending_dots(ctx, debug, n):
    import slepc_amd as ks
    A, v0, off = _band5_off(ks, ctx, debug, n)
    on = _run(ks, ctx, debug, A, v0, M, True, grid=DEPTH_G, lag_odd=True)
    _took_every_launch(on["stats"])
    _forced_grid_checks(A, off, on, DEPTH_G)


@pytest.mark.parametrize("hook", [{"abort_wg": 1}, {"budget": 0}], ids=["workgroup-1-gives-up", "budget-0"])
@pytest.mark.parametrize("n", DEPTH_N)
def test_a_workgroup_that_goes_dead_drops_its_pending_dots(ctx, debug, n, hook):
    """Every launch gives up (the existing hooks' give-up path): the pending dots are skipped, no partial is written, every C-phase still completes, and the
    ordinary product and dot sweep behind the launch leave the ordinary run."""
    import slepc_amd as ks
    A, v0, off = _band5_off(ks, ctx, debug, n)
    ab = _run(ks, ctx, debug, A, v0, M, True, grid=DEPTH_G, **hook)
    st = ab["stats"]
    assert st["enqueued"] == M - 1 and st["taken"] >= M - 3
    assert st["aborted"] == st["taken"] and st["completed"] == 0 and st["fell_back"] == st["enqueued"]
    _forced_grid_checks(A, off, ab, DEPTH_G)
    assert ab["beta"] == off["beta"] and np.array_equal(ab["T"], off["T"])
    assert np.array_equal(ab["V"].view(np.uint64), off["V"].view(np.uint64))


def test_the_launch_own_grid_with_lagging_workgroups(ctx, debug):
    """n = 655 873 at one workgroup per CU, odd workgroups lagging: the whole run is the ordinary run's bytes."""
    import slepc_amd as ks
    n = 655873
    A, v0, off = _band5_off(ks, ctx, debug, n)
    on = _run(ks, ctx, debug, A, v0, M, True, grid=0, lag_odd=True)
    _took_every_launch(on["stats"])
    assert (on["mm"], on["brk"], on["passes"]) == (off["mm"], off["brk"], off["passes"])
    assert on["guard"] and off["guard"]
    assert on["beta"] == off["beta"] and np.array_equal(on["T"], off["T"])
    assert np.array_equal(on["V"].view(np.uint64), off["V"].view(np.uint64))
