"""CPU self-check of the systems and the reference that tests/test_gpu_direct_solve.py holds the GPU
triangular solve to (tests/direct_solve_cases.py), and of the explicit supernode tree on the host
(tests/cpp/explicit_tree.cpp): a wrong yardstick must not pass for a wrong kernel, or hide one.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import direct_solve_cases as dsc
from conftest import REPO

ALL = sorted(dsc.ALL_SPECS)

pytestmark = pytest.mark.skipif(not dsc.HAVE_LONGDOUBLE,
                                reason="np.longdouble is not wider than float64 here: no high-precision reference")


def test_longdouble_is_extended_precision():
    assert dsc.LD_EPS < 2e-19


@pytest.mark.parametrize("name", ALL)
def test_system_is_symmetric_positive_definite_and_well_conditioned(name):
    c = dsc.get_case(name)
    A = c.A
    assert A.shape == (c.n, c.n) and c.xyz.shape == (c.n, 3)
    assert A.has_sorted_indices and np.all(A.diagonal() > 0) and A.nnz == (A + A.T).nnz   # full symmetric pattern
    assert abs(A - A.T).max() == 0.0
    assert c.n <= 3000 or c.family == "grid"
    if c.n <= 3000:
        np.linalg.cholesky(A.toarray())
    else:   # (the 16^3 grid: strictly diagonally dominant with a positive diagonal)
        off = abs(A).sum(axis=1).A1 - A.diagonal()
        assert np.all(A.diagonal() > off)
    assert dsc.cond2(A) < 1e6


@pytest.mark.parametrize("name", ALL)
def test_reference_solves_the_system_to_long_double_rounding(name):
    c = dsc.get_case(name)
    b = np.hstack(dsc.case_rhs(name))
    x = np.hstack(dsc.case_reference(name))
    assert x.dtype == np.longdouble
    r = dsc._residual_ld(c.A, x, b.astype(np.longdouble))
    back = np.abs(r).max() / (np.longdouble(dsc.norm_inf_A(c.A)) * np.abs(x).max() + np.abs(b).max())
    assert back < 1e-17, float(back)
    # per column too: the three scales (1, 1e3, 1e-3) must not hide in one another
    for j in range(b.shape[1]):
        bj = np.abs(r[:, j]).max() / (np.longdouble(dsc.norm_inf_A(c.A)) * np.abs(x[:, j]).max() + np.abs(b[:, j]).max())
        assert bj < 1e-17, (j, float(bj))
    # and the metrics see an error of one unit in the last place of one entry
    x64 = x[:, :3].astype(np.float64)
    i = int(np.argmax(np.abs(x64[:, 0])))
    bumped = x64.copy()
    bumped[i, 0] = np.nextafter(bumped[i, 0], np.inf) + 8 * np.spacing(bumped[i, 0])
    assert dsc.err(bumped, x[:, :3]) > dsc.err(x64, x[:, :3])


@pytest.mark.parametrize("name", sorted(dsc.ARROW_SPECS))
def test_explicit_tree_is_a_postorder_whose_ancestors_hold_every_coupling(name):
    c = dsc.get_case(name)
    assert dsc.check_tree(c.tree, c.n)
    beg, end, parent = c.tree
    owner = np.repeat(np.arange(len(beg)), end - beg)
    coo = c.A.tocoo()
    lo, hi = owner[np.minimum(coo.row, coo.col)], owner[np.maximum(coo.row, coo.col)]
    anc = np.zeros((len(beg), len(beg)), bool)
    for s in range(len(beg)):
        a = s
        while a >= 0:
            anc[s, a] = True
            a = parent[a]
    assert np.all(anc[lo, hi])


def test_case_lists_cover_what_the_solver_tests_name():
    for p in dsc.SINGLE_P:
        assert f"single_p{p}" in dsc.ARROW_SPECS
    for p, nb in dsc.LEAF_P_NB:
        c = dsc.get_case(f"arrow_p{p}_nb{nb}")
        assert tuple(c.tree[1] - c.tree[0]) == (p, p, nb)
    c = dsc.get_case("chain_odd")
    assert all(int(m) % 2 == 1 for m in c.tree[1] - c.tree[0])
    two = dsc.get_case("g24_two_roots").A
    import scipy.sparse.csgraph as csg
    assert csg.connected_components(two, directed=False)[0] == 2
    iso = dsc.get_case("isolated_vertex").A
    assert iso[17].nnz == 1 and csg.connected_components(iso, directed=False)[0] == 2
    assert dsc.get_case("diagonal").A.nnz == 40
    n = dsc.get_case("g14_holes").n
    assert 600 < n < 800


def test_explicit_tree_factors_and_solves_on_the_host(tmp_path):
    """tests/cpp/explicit_tree.cpp: arrow, chain and single-supernode systems through
    aa::explicit_tree -> multifrontal_cholesky -> factor_solve_host (A x = b at 1e-10, bnd exactly
    the ancestors' pivots); trees that A does not respect are refused; the degenerate graphs pass
    nested_dissection."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "explicit_tree")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", os.path.join(REPO, "tests", "cpp", "explicit_tree.cpp"),
                    os.path.join(REPO, "aa-admm_amd", "csrc", "spd_direct.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, OMP_NUM_THREADS="2"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("TREE_OK") == 5 and r.stdout.count("REFUSED_OK") == 4 and r.stdout.count("ND_OK") == 3


def test_solve_plan_invariants_on_the_host(tmp_path):
    """tests/cpp/solve_plan.cpp: grid systems through nested_dissection -> multifrontal_cholesky ->
    plan_solve (aa-admm_amd/csrc/solve_plan.cpp, no HIP) for the settings the GPU cases use -- tile
    widths, packed on / off, streams off / gated / all, branches, one and two sets, the dense top for
    2 and 3 parts. Per plan: membership, level order, forward / backward coverage, the top's split,
    branch ranges, the streamed runs' counters and queue order, the fused subtrees' items and LDS
    offsets, packed offsets; the one-set plan built wide equals the two-set plan."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "solve_plan")
    csrc = os.path.join(REPO, "aa-admm_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I", csrc, os.path.join(REPO, "tests", "cpp", "solve_plan.cpp"),
                    os.path.join(csrc, "solve_plan.cpp"), os.path.join(csrc, "spd_direct.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, OMP_NUM_THREADS="2"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("PLAN_OK") == 1 and "FAIL" not in r.stdout
