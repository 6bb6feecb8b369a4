"""The pipelined form of the forward update (k_gs_update_fwd<KT, S, true>): the panel loads of a workgroup's next tile go out behind the
publish of the tile just computed, in front of the A-phase of the tile before, and the panel just computed waits in LDS meanwhile. What that can get wrong is
the rotation of three panels through two sets of registers and one LDS buffer - a panel read back one round late or early, a tile's own rows of the column
taken from the wrong tile, the loads of a round that has no tile, a workgroup that goes dead with a panel parked - and the deeper issue order of the loads
around the hand-off. The library takes the pipelined form from a column count on (FWD_PIPE_MIN_K, ks_gs.hip) and the form without the park below it; the
runs here have M = 31 steps, so that the forward launch sees every column count 1 .. 30, both forms, all four classes of accumulator sets and the widest
parked panel.

Method and helpers are those of test_gpu_step_forward.py: every case is a Lanczos run with the form on and one with KS_DEBUG_NO_STEP_FORWARD from the same
start vector, in storage pre-filled with 0xFF bytes whose guard rows are checked afterwards.
 - With its own grid (one workgroup per CU) the whole run is compared as bytes.
 - With a forced grid of fewer workgroups than tiles the stored columns and y keep their bits and the next step's dots are the same products summed in that
   grid's order: column 1 bit for bit, T and beta to TOL = 1e-12, the Lanczos relation to 1e-12 with the products of Mat.mult, an orthonormal basis, identical
   pass counts. Where the forced grid holds every tile at once the run is compared as bytes as well."""
import numpy as np
import pytest

from test_gpu_step_forward import TOL, _band5, _run, _same_run, _start_vector

pytestmark = pytest.mark.gpu

M = 31                # steps of a run: column counts 1 .. 30 in the forward launch, 32 columns of storage (the form's limit)

_CACHE = {}


def _off(ks, ctx, debug, key, make):
    """(matrix, start vector, the run with the form off) of a shape: computed once, shared by the tests, never modified."""
    if key not in _CACHE:
        A = make(ks, ctx)
        v0 = _start_vector(A.n)
        _CACHE[key] = (A, v0, _run(ks, ctx, debug, A, v0, M, False))
    return _CACHE[key]


def _forced_grid_checks(A, off, on, grid):
    """The checks of test_forward_run_equals_the_ordinary_run for a forced grid."""
    _same_run(off, on, M)
    assert np.array_equal(off["V"][:, 0], on["V"][:, 0]) and np.array_equal(off["V"][:, 1], on["V"][:, 1])
    if (A.n + 511) // 512 <= grid:
        assert on["beta"] == off["beta"] and np.array_equal(on["T"], off["T"])
        assert np.array_equal(on["V"].view(np.uint64), off["V"].view(np.uint64))
    Vd = on["V"]
    assert np.abs(Vd.T @ Vd - np.eye(M + 1)).max() < 1e-13
    T = on["T"]
    Tm = np.diag(T[:M, 0]) + np.diag(T[: M - 1, 1], 1) + np.diag(T[: M - 1, 1], -1)
    AV = np.stack([A.mult(Vd[:, j]) for j in range(M)], axis=1)
    R = AV - Vd[:, :M] @ Tm
    R[:, M - 1] -= on["beta"] * Vd[:, M]
    assert np.abs(R).max() < TOL


def _took_every_launch(st):
    assert st["enqueued"] == M - 1 and st["refused"] == ""
    assert st["taken"] == st["completed"] and st["aborted"] == 0 and st["taken"] >= M - 3
    assert st["fell_back"] == st["enqueued"] - st["taken"]


@pytest.mark.parametrize("hooks", [{}, {"lag_odd": True}, {"budget": 0}], ids=["even-load", "odd-workgroups-lag", "every-wait-gives-up"])
@pytest.mark.parametrize("n", [655873, 655872])
def test_every_column_count_with_the_launch_own_grid(ctx, debug, n, hooks):
    """1 281 tiles and one odd last row (n = 655 873), 1 281 tiles exactly (n = 655 872): five to six rounds of 256 workgroups, the last one partly empty,
    at every column count 1 .. 30. T, beta and every column of the basis are the ordinary run's bytes; under budget = 0 every launch falls back and the bytes
    still match."""
    import slepc_amd as ks
    A, v0, off = _off(ks, ctx, debug, ("band5", n), lambda ks, ctx: _band5(ks, ctx, n))
    assert A.n >= 4 * 512 * ctx.device_info()["num_cu"]
    on = _run(ks, ctx, debug, A, v0, M, True, grid=0, **hooks)
    st = on["stats"]
    assert st["enqueued"] == M - 1 and st["refused"] == ""
    if hooks.get("budget") == 0:
        assert st["taken"] >= M - 3 and st["aborted"] == st["taken"] and st["completed"] == 0 and st["fell_back"] == st["enqueued"]
    else:
        _took_every_launch(st)
    assert (on["mm"], on["brk"], on["passes"]) == (off["mm"], off["brk"], off["passes"]) == (M, False, off["passes"])
    assert on["guard"] and off["guard"]
    assert on["beta"] == off["beta"] and np.array_equal(on["T"], off["T"])
    assert np.array_equal(on["V"].view(np.uint64), off["V"].view(np.uint64))


# n -> tiles per workgroup at a forced grid of 4: 512 * 4 * r rows give every workgroup r tiles (r = 1: nothing rotates, r = 2: the prologue's loads and one
# more, r = 3: the first panel that comes back from LDS while another is in flight, 4 and 7: the steady state at both parities); 11 tiles: workgroups of 3 and
# of 2 tiles in one launch; 9 tiles and one row: 3, 3, 2, 2 with the odd last row on its own in the third round.
DEPTH_G = 4
DEPTH_N = [512 * DEPTH_G * r for r in (1, 2, 3, 4, 7)] + [512 * (DEPTH_G * 3 - 1), 512 * (DEPTH_G * 3 - 3) + 1]


@pytest.mark.parametrize("n", DEPTH_N)
def test_rotation_depth(ctx, debug, n):
    import slepc_amd as ks
    A, v0, off = _off(ks, ctx, debug, ("band5", n), lambda ks, ctx: _band5(ks, ctx, n))
    on = _run(ks, ctx, debug, A, v0, M, True, grid=DEPTH_G)
    _took_every_launch(on["stats"])
    _forced_grid_checks(A, off, on, DEPTH_G)


@pytest.mark.parametrize("n", DEPTH_N)
def test_rotation_depth_with_a_workgroup_that_gives_up(ctx, debug, n):
    """Workgroup 1 gives up at its first wait, with a panel parked and the next one in flight: it and every workgroup that sees the abort word still complete
    and publish every C-phase (every column is stored), and the ordinary product and dot sweep behind the launch redo y and the partials."""
    import slepc_amd as ks
    A, v0, off = _off(ks, ctx, debug, ("band5", n), lambda ks, ctx: _band5(ks, ctx, n))
    ab = _run(ks, ctx, debug, A, v0, M, True, grid=DEPTH_G, abort_wg=1)
    st = ab["stats"]
    assert st["enqueued"] == M - 1 and st["taken"] >= M - 3
    assert st["aborted"] == st["taken"] and st["completed"] == 0 and st["fell_back"] == st["enqueued"]
    _forced_grid_checks(A, off, ab, DEPTH_G)


@pytest.mark.parametrize("lag", [False, True], ids=["even-load", "odd-workgroups-lag"])
@pytest.mark.parametrize("grid", [12, 40])
def test_far_neighbours(ctx, debug, grid, lag):
    """64 x 64 x 20 points: the far neighbours 8 tiles away. Grid 12 is the bound far + 2 = G: the A-phase of round i - 1 waits for tiles of round i, which their
    workgroups publish before they issue the loads of round i + 1. Grid 40: four rounds, neighbours in the round before, the same and the next one."""
    import slepc_amd as ks
    A, v0, off = _off(ks, ctx, debug, "lap3d-64x64x20", lambda ks, ctx: ks.Mat.laplacian3d(ctx, 64, 64, 20))
    on = _run(ks, ctx, debug, A, v0, M, True, grid=grid, **({"lag_odd": True} if lag else {}))
    _took_every_launch(on["stats"])
    _forced_grid_checks(A, off, on, grid)
    if ("even", grid) not in _CACHE:
        _CACHE[("even", grid)] = on if not lag else _run(ks, ctx, debug, A, v0, M, True, grid=grid)
    even = _CACHE[("even", grid)]
    # the order of every sum is fixed by the grid, not by timing
    assert np.array_equal(on["T"], even["T"]) and np.array_equal(on["V"].view(np.uint64), even["V"].view(np.uint64)) and on["passes"] == even["passes"]
