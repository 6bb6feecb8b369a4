"""Shared inputs of the tests that run the row sweeps of the block solvers (k_block_residual, k_ritz_residual, k_oblique_dot / k_oblique_update,
k_restart_fused, k_dot_sweep) in the forms they take at workload size: nontemporal loads of the basis, and more than one tile per workgroup.

Which load form a call ran is read from the library (Context.basis_load_counts, the verdicts of ks_basis_loads_plain): nothing here restates the
size rule. streaming_ld finds the leading dimension at which a launcher switches to streaming loads by asking that hook, so a case of a few
thousand rows reaches the streaming form with a large ld - storage that is allocated and never touched beyond row n."""
import numpy as np

TILE = 512                 # rows of a tile of the 256-thread sweeps on 16-byte aligned columns (ks_sweeps.cuh: SW_BLOCK x 2)
RESTART_TILE = 128         # rows of a wave's tile in k_restart_fused (ks_panel.hip: RF_ROWS)
RESTART_WAVES = 4          # waves of a workgroup there
SWEEP_PER_CU = 4           # ks_sweep_grid: k_oblique_update
RITZ_PER_CU = 2            # ks_ritz_residual
BLOCK_RESIDUAL_PER_CU = 8  # ksl_block_residual: the occupancy result, at most 8


def dot_per_cu(k):
    """workgroups per CU of a dot sweep over k columns (ksk_dot, launch_oblique_dot)"""
    return max(1, min(4, (30 + k - 1) // k))


def even_ld(n):
    """the smallest even leading dimension >= n + 2"""
    return n + 2 + n % 2


def counted(ctx, fn):
    """fn() and the (plain, streaming) verdicts the library counted while it ran"""
    ctx.basis_load_counts(reset=True)
    out = fn()
    return out, ctx.basis_load_counts(reset=True)


def _dot_sweep_streams(ctx, columns, ld):
    """one dot sweep over a BV of one row, `columns` columns and this ld: did the library choose streaming loads?"""
    import slepc_amd as ks
    V = ks.BV(ctx, 1, columns, ld=ld)
    V.SetActiveColumns(0, 1)
    _, (plain, streaming) = counted(ctx, lambda: V.DotVec(V.column_ptr(0)))
    V.destroy()
    assert plain + streaming == 1, (plain, streaming)
    return streaming == 1


_first_streaming_ld = {}


def streaming_ld(ctx, n, columns):
    """The smallest even ld >= n + 2 at which the library reports streaming loads for a basis of `columns` columns. The search starts where 200 MB
    of storage end and goes up from there; the answer is the hook's. (A launcher that counts other columns than the BV's own - three blocks of
    the active width, 2 m + ncols - passes that count: the rule is one function of (columns, ld).)"""
    if columns not in _first_streaming_ld:
        ld = -(-200_000_000 // (8 * columns))
        ld += ld % 2
        for attempt in range(12):
            if _dot_sweep_streams(ctx, columns, ld):
                break
            ld = ld + 2 if attempt < 2 else (ld * 5 // 4) // 2 * 2
        else:
            raise AssertionError("no streaming form up to ld = %d with %d columns" % (ld, columns))
        _first_streaming_ld[columns] = ld
    return max(even_ld(n), _first_streaming_ld[columns])


def two_round_n(per_cu, num_cu, tile=TILE):
    """Rows at which a grid of per_cu * num_cu workgroups gives every workgroup one tile and some a second, the last tile being a single row."""
    return per_cu * num_cu * tile + tile + 1


def walk(n, per_cu, num_cu, tile=TILE):
    """(tiles, largest grid the launcher can choose) of a sweep over n rows"""
    return -(-n // tile), per_cu * num_cu


def fill_nan(ctx, *bvs):
    """the whole storage of each BV <- NaN bytes (rows n .. ld - 1 keep them: a read past the row guard shows in the result)"""
    for bv in bvs:
        nc = bv.nc
        ctx.memset(bv.column_ptr(-nc), 0xFF, (nc + bv.m) * bv.ld * 8)
    ctx.synchronize()


def spread_rows(n, tile=TILE, per_tile=3, limit=4096):
    """At most `limit` rows with some in every tile of n rows: the last, the first and one in the middle of each tile, as many of them as the
    limit allows (the single row of a last tile included)."""
    ntiles = -(-n // tile)
    per_tile = max(1, min(per_tile, 3, limit // ntiles))
    rows = []
    for t in range(ntiles):
        lo, hi = t * tile, min(n, (t + 1) * tile)
        rows += [hi - 1, lo, (lo + hi) // 2][:per_tile]
    rows = np.unique(np.array(rows, dtype=np.int64))
    assert len(rows) <= limit and rows.max() == n - 1
    return rows
