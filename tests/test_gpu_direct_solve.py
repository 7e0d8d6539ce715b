"""GPU: is A x = b? The device triangular solves of DirectSolver (csrc/direct_solve.hip) against a
high-precision solution of the same linear system, through the hook aa_test_direct_solve
(capi.test_direct_solve): small systems (tests/direct_solve_cases.py) built to land on each kernel
family -- row tasks k_fwd / k_bwd, split-K tiles strided and packed in three widths with and
without non-temporal loads, streamed or one launch per level, fused subtrees with and without
their LDS-resident vectors, one and two sets, branches -- on each threshold and each edge. Every
case asserts through the plan summary (DirectSolver::plan_summary) that it ran the path it was
written for.

Metric, for every x the device returns:
    err(x)  = max over the 3 columns of |x - x_ref|_inf / |x_ref|_inf
    berr(x) = |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf)          (in long double)
x_ref: fp64 LU refined with long-double residuals (direct_solve_cases.reference). The yardstick is
the same quantity for x_host = factor_solve_host with the SAME factor in plain host loops (which
tests/cpp/part_solve.cpp and explicit_tree.cpp pin to A x = b): what fp64 with this factor can do.
    assert err(x_gpu) <= 8 * max(err(x_host), 64 eps)        and the same for berr.
Device and host compute the same products G_s f in different summation orders (split-K partials,
lane-strided rows): another rounding constant, not another order of magnitude. A structural defect
(a dropped row, a stale update vector, a wrong tile clip) is ten orders above this bound.

AA_TEST_SOLVE_DUMP=<file> appends one JSON line per checked x (case, err / berr of device and host).

Measured on one MI355X (largest device / host ratio per family; err and berr of the host solve are
2e-15 .. 5e-15 and 1e-16 .. 6e-16 throughout, below the 64 eps floor of the bound, so the largest
device error is 0.31 of the bound):

    family                              cases   err gpu/host   berr gpu/host
    grids, one set                          9           1.06            1.31
    arrow / chain / single, one set        49           1.22            1.68
    degenerate                              5           1.03            1.00
    kernel-family matrix                   16           0.92            0.57
    fused-subtree variants                 21           0.92            0.63
    two sets                                6           1.22            1.43
    reuse / gated / streamed               12           0.97            0.97
    branches                                9           1.06            1.09
    device factor                           8           1.00            1.22
    unit right-hand sides                   4           0.99            1.70

Sensitivity (one-off, arithmetic-only mutations of direct_solve.hip, one at a time): red_tiles
dropping the last partial failed 48 of 104 cases (the file before sixteen more arrow shapes at the
64 / 128 thresholds were added), bwd_row without the M rows' subtraction
70, k_bwd striding G by the un-padded p instead of ldr 47 (odd p only), the fused forward's update
vectors scaled by 1 + 1e-10 41. Of the solver's bit-identity tests the first two were noticed only
because the trajectories turned NaN, the third by one side assertion of one case, the fourth by none.
"""
import json
import os

import numpy as np
import pytest

import direct_solve_cases as dsc
from direct_solve_cases import EPS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not dsc.HAVE_LONGDOUBLE,
                                 reason="np.longdouble is not wider than float64 here: no high-precision reference")]

KNOBS = ("AA_SOLVE_MIN_SUBTREES", "AA_SOLVE_PACKED", "AA_SOLVE_TILE", "AA_SOLVE_MIN_TILES", "AA_FACTOR_NT",
         "AA_FACTOR_NT_ROWS", "AA_SUB_LDS_U", "AA_SUB_LDS_X", "AA_SUB_BLOCK", "AA_SOLVE_STREAM", "AA_SOLVE_STREAM_GATED",
         "AA_SOLVE_BRANCHES", "AA_SOLVE_BRANCHES_REJECT", "AA_SOLVE_WAVEP", "AA_SOLVE_WAVER", "AA_DENSE_MIN_FRONT",
         "AA_DENSE_GPU", "AA_SUB_TIMING", "AA_SOLVE_STATS")


def run(pkg, ctx, monkeypatch, name, b0, b1=None, script=None, env=None, **over):
    """One hook call on case `name` with its own parameters and knobs, `env` on top."""
    c = dsc.get_case(name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**c.env, **(env or {})}.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))
    prm = {**c.params, **over}
    try:
        return pkg.capi.test_direct_solve(ctx, c.A, c.xyz, b0, b1, script=(pkg.capi.AA_SOLVE_B0,) if script is None else script,
                                          tree=c.tree, **prm)
    except pkg.capi.AAError as e:
        if e.code == -3:   # AA_ERR_DEVICE: nothing more may run on a device that has faulted
            pytest.exit(f"device error in {name}: {e}", returncode=3)
        raise


def untouched(x, pkg):
    return np.all(x == pkg.capi.SOLVE_SENTINEL)


def check_accuracy(label, A, x_gpu, x_host, x_ref, b):
    assert np.all(np.isfinite(x_gpu)), label
    eg, eh = dsc.err(x_gpu, x_ref), dsc.err(x_host, x_ref)
    bg, bh = dsc.berr(A, x_gpu, b), dsc.berr(A, x_host, b)
    rec = dict(case=label, n=A.shape[0], err_gpu=eg, err_host=eh, berr_gpu=bg, berr_host=bh,
               err_ratio=eg / max(eh, 64 * EPS), berr_ratio=bg / max(bh, 64 * EPS), err_gpu_over_host=eg / eh if eh else 0.0,
               berr_gpu_over_host=bg / bh if bh else 0.0)
    print(json.dumps(rec))
    if os.environ.get("AA_TEST_SOLVE_DUMP"):
        with open(os.environ["AA_TEST_SOLVE_DUMP"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert eg <= 8 * max(eh, 64 * EPS), rec
    assert bg <= 8 * max(bh, 64 * EPS), rec


def classes(tree, wave_p, wave_r):
    """(forward row, forward tiled, backward row, backward tiled) supernode counts of a block system."""
    beg, end, parent = tree
    p = (end - beg).astype(int)
    nb = np.zeros(len(p), int)
    for s in range(len(p)):
        a = parent[s]
        while a >= 0:
            nb[s] += p[a]
            a = parent[a]
    frow, brow = p <= wave_p, p + nb <= wave_r
    return int(frow.sum()), int((~frow).sum()), int(brow.sum()), int((~brow).sum()), p, nb


# ---- 1. every system, one set --------------------------------------------------------------------
def _fused(P):
    assert P["fused_subtrees"] > 0 and P["fused_supernodes"] > 0, P


def _levels_only(P):
    assert P["fused_subtrees"] == 0 and P["fused_supernodes"] == 0 and P["levels"] > 0, P


def _tiles(P):
    assert P["fwd_tiles"] > 0 and P["bwd_tiles"] > 0, P


def _g24_levels(P):
    _levels_only(P), _tiles(P)
    assert P["fwd_tasks"] > 0 and P["bwd_tasks"] > 0, P
    assert P["fwd_row_bwd_tile_nodes"] > 0 and P["odd_p_nodes"] > 0, P   # a mixed class; the ldr pad


def _g24_wide_rows(P):
    _levels_only(P)
    assert P["fwd_tiles"] > 0 and P["bwd_tiles"] == 0 and P["bwd_tasks"] > 0, P   # every backward sweep as row tasks
    assert P["fwd_tile_bwd_row_nodes"] > 0 and P["row_R_max"] > 256 and P["row_p_max"] > 64, P   # the other mixed class; long rows


def _g24_elastic(P):
    _fused(P)
    assert P["fwd_tasks"] > 0 and P["bwd_tasks"] > 0 and P["row_R_max"] > 128 and P["row_p_max"] > 64, P   # the 256 / 128 blocks


def _cloth(P):
    _fused(P)
    assert P["fwd_tasks"] > 0 and P["bwd_tasks"] > 0, P


def _dense_root(P):
    _levels_only(P), _tiles(P)
    assert P["tile_p_max"] > 1024 and P["fwd_tasks"] > 0, P   # multi-column tiles; the leaves as row tasks


def _holes(P):
    _fused(P)
    assert P["supernodes"] > 50, P   # an irregular tree, not one collapsed front


GRID_PLAN = {
    "g12_fused": lambda P: (_fused(P), _tiles(P)),
    "g24_fused": lambda P: (_fused(P), _tiles(P)),
    "g24_levels": _g24_levels,
    "g24_wide_rows": _g24_wide_rows,
    "g24_elastic": _g24_elastic,
    "cloth48": _cloth,
    "g16_dense_root": _dense_root,
    "g24_two_roots": lambda P: (_fused(P), _tiles(P)),
    "g14_holes": _holes,
}


@pytest.mark.parametrize("name", sorted(dsc.ALL_SPECS))
def test_gpu_solve_matches_reference(pkg, ctx, monkeypatch, name):
    c = dsc.get_case(name)
    b0, _ = dsc.case_rhs(name)
    x_ref, _ = dsc.case_reference(name)
    r = run(pkg, ctx, monkeypatch, name, b0)
    P = r.plan
    print(name, P)
    assert untouched(r.x[0][1], pkg)
    if c.family == "grid":
        GRID_PLAN[name](P)
        if name == "g24_two_roots":   # a root in each half
            import scipy.sparse.csgraph as csg
            _, comp = csg.connected_components(c.A, directed=False)
            assert set(comp[r.depth == 0]) == {0, 1}
    elif c.family == "arrow":
        fr, ft, br, bt, p, nb = classes(c.tree, c.params["wave_p"], c.params["wave_r"])
        assert P["fused_subtrees"] == 0 and P["supernodes"] == len(p), P
        assert (P["fwd_row_nodes"], P["fwd_tile_nodes"], P["bwd_row_nodes"], P["bwd_tile_nodes"]) == (fr, ft, br, bt), P
        assert (P["fwd_tasks"] > 0, P["fwd_tiles"] > 0, P["bwd_tasks"] > 0, P["bwd_tiles"] > 0) == (fr > 0, ft > 0, br > 0, bt > 0), P
        assert P["odd_p_nodes"] == int((p % 2 == 1).sum()), P
        if name in ("arrow_p100_nb300", "arrow_p1_nb400"):   # R = 400 / 401 forward rows: two 256-row blocks per leaf
            assert P["multi_block_fwd_nodes"] == 2, P
        parent = c.tree[2]
        height, depth = np.zeros(len(p), int), np.zeros(len(p), int)
        for s in range(len(p)):
            if parent[s] >= 0:
                height[parent[s]] = max(height[parent[s]], height[s] + 1)
        for s in reversed(range(len(p))):
            depth[s] = depth[parent[s]] + 1 if parent[s] >= 0 else 0
        assert np.array_equal(r.height, np.repeat(height, p)) and np.array_equal(r.depth, np.repeat(depth, p))
    else:
        _levels_only(P)
        if name in ("n1", "n2", "below_leaf"):
            assert P["supernodes"] == 1, P
        if name == "diagonal":
            assert P["supernodes"] >= 2 and np.all(r.depth == 0) and np.all(r.height == 0), P
    check_accuracy(name, c.A, r.x[0][0], r.x_host[0], x_ref, b0)


# ---- 2. the kernel-family matrix on 24 x 10 x 12 (leaf 8, wave 16 / 32) ---------------------------
FAMILY = [(8, 1, 64, 0), (8, 1, 128, 1), (8, 1, 256, 0), (8, 0, 64, 1), (8, 0, 128, 0), (8, 0, 256, 1), (8, 1, 64, 1),
          (8, 0, 256, 0), (4096, 1, 64, 1), (4096, 1, 128, 0), (4096, 1, 256, 1), (4096, 0, 64, 0), (4096, 0, 128, 1),
          (4096, 0, 256, 0), (4096, 1, 256, 0), (4096, 0, 64, 1)]


@pytest.mark.parametrize("min_sub,packed,tile,nt", FAMILY)
def test_gpu_kernel_family_matrix(pkg, ctx, monkeypatch, min_sub, packed, tile, nt):
    name = "g24_fused"
    c = dsc.get_case(name)
    b0, _ = dsc.case_rhs(name)
    x_ref, _ = dsc.case_reference(name)
    r = run(pkg, ctx, monkeypatch, name, b0, env={"AA_SOLVE_MIN_SUBTREES": min_sub, "AA_SOLVE_PACKED": packed,
                                                   "AA_SOLVE_TILE": tile, "AA_FACTOR_NT": nt, "AA_FACTOR_NT_ROWS": nt})
    P = r.plan
    assert P["fwd_tiles"] > 0 and P["bwd_tiles"] > 0 and P["fwd_tile_w"] == tile and P["bwd_tile_w"] == tile, P
    assert (P["packed"], P["nt"], P["nt_rows"]) == (packed, nt, nt), P
    assert (P["fused_subtrees"] > 0) == (min_sub == 8), P
    if min_sub == 4096:
        assert P["fwd_tasks"] > 0 and P["bwd_tasks"] > 0, P
    check_accuracy(f"family ms{min_sub} pk{packed} w{tile} nt{nt}", c.A, r.x[0][0], r.x_host[0], x_ref, b0)


# ---- 3. fused-subtree variants ---------------------------------------------------------------------
FUSED_ENV = {"g24_fused": {}, "g12_fused": {}, "chain_odd": {"AA_SOLVE_MIN_SUBTREES": 1}}   # (the chain: leaves + middle fused)


@pytest.mark.parametrize("lds_u,lds_x,block", [(None, None, None), ("0", "0", None), ("0", None, None), (None, "0", None),
                                              (None, None, 256), (None, None, 512), (None, None, 1024)])
@pytest.mark.parametrize("name", sorted(FUSED_ENV))
def test_gpu_fused_subtree_variants(pkg, ctx, monkeypatch, name, lds_u, lds_x, block):
    c = dsc.get_case(name)
    b0, _ = dsc.case_rhs(name)
    x_ref, _ = dsc.case_reference(name)
    r = run(pkg, ctx, monkeypatch, name, b0, env={**FUSED_ENV[name], "AA_SUB_LDS_U": lds_u, "AA_SUB_LDS_X": lds_x,
                                                   "AA_SUB_BLOCK": block})
    P = r.plan
    _fused(P)
    assert (P["sub_u"] > 0) == (lds_u is None) and (P["sub_x"] > 0) == (lds_x is None), P
    assert P["sub_block"] == (block or 1024), P
    if name == "chain_odd":
        assert P["fused_supernodes"] == 4 and P["fused_subtrees"] == 1, P
    check_accuracy(f"fused {name} u{lds_u} x{lds_x} blk{block}", c.A, r.x[0][0], r.x_host[0], x_ref, b0)


# ---- 4. two sets -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("g24_levels", {"AA_SOLVE_TILE": 64}), ("g24_fused", {}), ("arrow_p193_nb191", {})])
def test_gpu_two_sets_bit_identical_to_one_set(pkg, ctx, monkeypatch, name, env):
    """solve2(b0, b1) == solve(b0), solve(b1) on the same object, bit for bit (direct_solve.hpp), and
    a one-set solver built `wide` == the two-set solver."""
    K = pkg.capi
    c = dsc.get_case(name)
    b0, b1 = dsc.case_rhs(name)
    x0_ref, x1_ref = dsc.case_reference(name)
    two = run(pkg, ctx, monkeypatch, name, b0, b1, script=(K.AA_SOLVE_B0, K.AA_SOLVE_B1, K.AA_SOLVE_BOTH), env=env, max_sets=2)
    assert two.plan["max_sets"] == 2
    assert np.array_equal(two.x[2][0], two.x[0][0]) and np.array_equal(two.x[2][1], two.x[1][0])
    assert untouched(two.x[0][1], pkg) and untouched(two.x[1][1], pkg)
    wide = run(pkg, ctx, monkeypatch, name, b0, b1, script=(K.AA_SOLVE_B0, K.AA_SOLVE_B1), env=env, max_sets=1, wide=True)
    assert wide.plan["max_sets"] == 1
    assert np.array_equal(wide.x[0][0], two.x[0][0]) and np.array_equal(wide.x[1][0], two.x[1][0])
    check_accuracy(f"two sets {name} x0", c.A, two.x[2][0], two.x_host[0], x0_ref, b0)
    check_accuracy(f"two sets {name} x1", c.A, two.x[2][1], two.x_host[1], x1_ref, b1)


# ---- 5. one solver object reused ------------------------------------------------------------------
STREAM_KNOBS = {"AA_SOLVE_TILE": 64, "AA_SOLVE_MIN_SUBTREES": 4096}   # (with wave 16 / 32: test_gpu_streamed_levels_bit_identical's)


@pytest.mark.parametrize("name", ["g24_levels", "chain_odd_small_waves"])
@pytest.mark.parametrize("stream_all", [None, "1"])
def test_gpu_solver_reuse_gates_and_streams(pkg, ctx, monkeypatch, name, stream_all):
    """One object through solve, a skipped gated solve, a taken (streamed) gated solve, solve2, a
    `done` solve and solve again: the tile counters are reset by the last tile and the streamed
    runs' words are zeroed per solve, so nothing may depend on what ran before."""
    K = pkg.capi
    over = {}
    if name == "chain_odd_small_waves":   # every supernode tiled: three tile-only levels, streamed both ways
        name, over = "chain_odd", dict(dsc.SMALL_WAVES)
    c = dsc.get_case(name)
    b0, b1 = dsc.case_rhs(name)
    x0_ref, x1_ref = dsc.case_reference(name)
    script = (K.AA_SOLVE_B0, K.AA_SOLVE_GATED_SKIP_B0, K.AA_SOLVE_GATED_TAKE_B1, K.AA_SOLVE_BOTH, K.AA_SOLVE_DONE_B1,
              K.AA_SOLVE_B1, K.AA_SOLVE_B0)
    r = run(pkg, ctx, monkeypatch, name, b0, b1, script=script, env={**STREAM_KNOBS, "AA_SOLVE_STREAM": stream_all},
            max_sets=2, **over)
    P = r.plan
    assert P["fwd_streams"] > 0 and P["bwd_streams"] > 0 and P["packed"] == 1, P
    assert P["stream_gated"] == 1 and P["stream_all"] == (1 if stream_all else 0), P
    first, skipped, taken, both, done, plain_b1, last = r.x
    assert untouched(skipped[0], pkg) and untouched(skipped[1], pkg)
    assert untouched(done[0], pkg) and untouched(done[1], pkg)
    assert untouched(first[1], pkg) and untouched(taken[1], pkg)
    assert np.array_equal(taken[0], plain_b1[0])
    assert np.array_equal(first[0], last[0])
    assert np.array_equal(both[0], first[0]) and np.array_equal(both[1], plain_b1[0])
    check_accuracy(f"reuse {name} stream{stream_all} first", c.A, first[0], r.x_host[0], x0_ref, b0)
    check_accuracy(f"reuse {name} stream{stream_all} gated", c.A, taken[0], r.x_host[1], x1_ref, b1)
    check_accuracy(f"reuse {name} stream{stream_all} last", c.A, last[0], r.x_host[0], x0_ref, b0)


# ---- 6. branches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g24_two_roots", "g24_fused", "g24_levels"])
def test_gpu_branches_bit_identical(pkg, ctx, monkeypatch, name):
    c = dsc.get_case(name)
    b0, _ = dsc.case_rhs(name)
    x_ref, _ = dsc.case_reference(name)
    xs = []
    for nbr in (1, 2, 3):
        r = run(pkg, ctx, monkeypatch, name, b0, default_branches=nbr)
        assert r.plan["branches"] == nbr, r.plan
        check_accuracy(f"branches {name} {nbr}", c.A, r.x[0][0], r.x_host[0], x_ref, b0)
        xs.append(r.x[0][0])
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], xs[2])


# ---- 7. the factor from the device ----------------------------------------------------------------
@pytest.mark.parametrize("name,min_front", [("g12_fused", 1), ("chain_odd", 1), ("single_p1", 1), ("single_p63", 1),
                                            ("single_p64", 1), ("single_p65", 1), ("single_p129", 1), ("g24_fused", 64)])
def test_gpu_device_factor_solves_the_system(pkg, ctx, monkeypatch, name, min_front):
    """factor_on_device with every front (AA_DENSE_MIN_FRONT=1) on the dense backend -- k_scatter_coo,
    k_extend_add, k_potf2 (partial last block, several blocks), trsm / syrk, k_to_rowmajor -- or only
    the fronts of order >= 64 (host-held and device-held update matrices in one tree)."""
    c = dsc.get_case(name)
    b0, _ = dsc.case_rhs(name)
    x_ref, _ = dsc.case_reference(name)
    r = run(pkg, ctx, monkeypatch, name, b0, env={"AA_DENSE_MIN_FRONT": min_front}, device_factor=True)
    check_accuracy(f"device factor {name} min_front {min_front}", c.A, r.x[0][0], r.x_host[0], x_ref, b0)


# ---- 8. unit right-hand sides ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g24_levels", "g24_fused"])
def test_gpu_unit_right_hand_sides(pkg, ctx, monkeypatch, name):
    """A unit vector on a root pivot and one on a deepest-leaf pivot: an error on a single path
    through the tree cannot average out."""
    K = pkg.capi
    c = dsc.get_case(name)
    b, _ = dsc.case_rhs(name)
    info = run(pkg, ctx, monkeypatch, name, b, script=())
    root = int(np.flatnonzero(info.depth == 0)[0])
    leaves = np.flatnonzero(info.height == 0)
    leaf = int(leaves[np.argmax(info.depth[leaves])])
    assert info.depth[leaf] >= 3 and info.height[root] >= 3
    b0, b1 = dsc.unit_rhs(c.n, root), dsc.unit_rhs(c.n, leaf)
    x_ref = dsc.reference(c.A, np.hstack([b0, b1]))
    r = run(pkg, ctx, monkeypatch, name, b0, b1, script=(K.AA_SOLVE_B0, K.AA_SOLVE_B1))
    check_accuracy(f"unit root {name}", c.A, r.x[0][0], r.x_host[0], x_ref[:, :3], b0)
    check_accuracy(f"unit leaf {name}", c.A, r.x[1][0], r.x_host[1], x_ref[:, 3:], b1)
