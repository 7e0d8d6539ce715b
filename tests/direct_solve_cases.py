"""Linear systems for the tests of the GPU sparse triangular solve (DirectSolver, csrc/direct_solve.hip)
and their high-precision reference. Pure numpy / scipy: no GPU, no library.

* grid systems: the generator of tests/cpp/part_solve.cpp restated (27-point connectivity on an
  nx x ny x nz block, node (i*ny + j)*nz + k at (0.1 i, 0.1 j + 0.001 i, 0.1 k), off-diagonals -w,
  w ~ U(0.5, 1.5), diagonal = row sum + 0.05 U(0.5, 1.5)), optionally cut in two or with nodes
  deleted; ordered by the library's nested dissection;
* block systems with an explicit supernode tree (arrow: k leaves under one root; chain: leaf ->
  middle -> root): dense SPD blocks B B^T / m + I, every block coupled densely to all of its
  ancestors, so supernode s has exactly sizes[s] pivots and a boundary of all its ancestors' pivots;
* degenerate systems (n = 1, n = 2, fewer nodes than a leaf, an isolated vertex, a diagonal matrix).

reference(): x_ref = A^-1 b from an fp64 LU, refined with the residual b - A x accumulated in
np.longdouble (80-bit: eps 1.08e-19) until the correction is below 1e-17 relative.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)
EPS = float(np.finfo(np.float64).eps)
HAVE_LONGDOUBLE = LD_EPS < 2e-19   # 80-bit extended (or better); a 64-bit long double cannot referee fp64


@dataclass
class Case:
    name: str
    family: str                    # "grid" | "arrow" | "degenerate"
    A: sp.csr_matrix               # full symmetric pattern, sorted columns, every diagonal entry stored
    xyz: np.ndarray                # (n, 3)
    tree: tuple | None = None      # explicit supernode tree (beg, end, parent), postorder, identity permutation
    params: dict = field(default_factory=dict)   # leaf_size, top_rows, wave_p, wave_r
    env: dict = field(default_factory=dict)      # AA_SOLVE_* knobs the case is defined with

    @property
    def n(self):
        return self.A.shape[0]


# ---------------------------------------------------------------------------------- grid systems
_HALF_STENCIL = [(di, dj, dk) for di in (0, 1) for dj in (-1, 0, 1) for dk in (-1, 0, 1)
                 if not (di == 0 and (dj < 0 or (dj == 0 and dk <= 0)))]


def grid_system(nx, ny, nz, seed, cut_i=None, keep_fraction=None):
    """(A, xyz) of the 27-point grid. cut_i: no edge between planes i < cut_i and i >= cut_i (two
    components). keep_fraction: only a seeded random subset of the nodes is kept (renumbered)."""
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    I, J, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    I, J, K = I.ravel(), J.ravel(), K.ravel()
    ids = (I * ny + J) * nz + K
    assert np.array_equal(ids, np.arange(n))
    keep = np.ones(n, bool)
    if keep_fraction is not None:
        keep = rng.random(n) < keep_fraction
    ea, eb = [], []
    for di, dj, dk in _HALF_STENCIL:
        i2, j2, k2 = I + di, J + dj, K + dk
        ok = (i2 < nx) & (j2 >= 0) & (j2 < ny) & (k2 >= 0) & (k2 < nz)
        if cut_i is not None:
            ok &= ~((I < cut_i) & (i2 >= cut_i))
        b = (i2 * ny + j2) * nz + k2
        ok &= keep & keep[np.where(ok, b, 0)]
        ea.append(ids[ok])
        eb.append(b[ok])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    w = rng.uniform(0.5, 1.5, len(ea))
    mass = 0.05 * rng.uniform(0.5, 1.5, n)
    diag = mass + np.bincount(ea, w, n) + np.bincount(eb, w, n)
    rows = np.concatenate([ea, eb, np.arange(n)])
    cols = np.concatenate([eb, ea, np.arange(n)])
    vals = np.concatenate([-w, -w, diag])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    xyz = np.stack([0.1 * I, 0.1 * J + 0.001 * I, 0.1 * K], axis=1).astype(np.float64)
    if not keep.all():
        sel = np.flatnonzero(keep)
        A = A[sel][:, sel].tocsr()
        xyz = xyz[sel]
    A.sum_duplicates()
    A.sort_indices()
    return A, np.ascontiguousarray(xyz)


# ------------------------------------------------------------- block systems with an explicit tree
def block_system(sizes, parent, seed):
    """Dense SPD blocks in postorder (parent[s] > s, -1 = root), each coupled densely to all of its
    ancestors. Diagonal blocks B B^T / m + I (smallest eigenvalue >= 1); the couplings are U(-1, 1)
    scaled so that the off-diagonal part has Frobenius norm <= 0.7: A is SPD with smallest
    eigenvalue >= 0.3. Returns (A csr, xyz, (beg, end, parent))."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    parent = np.asarray(parent, np.int64)
    end = np.cumsum(sizes)
    beg = end - sizes
    n = int(end[-1])
    D = np.zeros((n, n))
    mask = np.zeros((n, n), bool)
    ncpl = 0
    for s, m in enumerate(sizes):
        a = parent[s]
        while a >= 0:
            ncpl += int(m * sizes[a])
            a = parent[a]
    scale = 0.7 / np.sqrt(2.0 * max(ncpl, 1))
    for s, m in enumerate(sizes):
        B = rng.standard_normal((m, m))
        D[beg[s]:end[s], beg[s]:end[s]] = B @ B.T / m + np.eye(m)
        mask[beg[s]:end[s], beg[s]:end[s]] = True
        a = parent[s]
        while a >= 0:
            C = rng.uniform(-1.0, 1.0, (m, sizes[a])) * scale
            D[beg[s]:end[s], beg[a]:end[a]] = C
            D[beg[a]:end[a], beg[s]:end[s]] = C.T
            mask[beg[s]:end[s], beg[a]:end[a]] = True
            mask[beg[a]:end[a], beg[s]:end[s]] = True
            a = parent[a]
    D = 0.5 * (D + D.T)
    r, c = np.nonzero(mask)
    A = sp.csr_matrix((D[r, c], (r, c)), shape=(n, n))
    A.sort_indices()
    xyz = np.zeros((n, 3))
    xyz[:, 0] = np.arange(n)
    return A, xyz, (beg.astype(np.int32), end.astype(np.int32), parent.astype(np.int32))


def arrow_system(p, q, k, seed):
    """k leaves of p pivots under a root of q: every leaf has nb = q, the root nb = 0. q = 0: the
    leaves alone (k = 1: a single supernode with no boundary)."""
    if q == 0:
        return block_system([p] * k, [-1] * k, seed)
    return block_system([p] * k + [q], [k] * k + [-1], seed)


def chain_system(p_leaf, p_mid, p_root, k, seed):
    """k leaves -> one middle -> root: the middle has children and a boundary (nb = p_root), the
    leaves nb = p_mid + p_root."""
    return block_system([p_leaf] * k + [p_mid, p_root], [k] * k + [k + 1, -1], seed)


def check_tree(tree, n):
    """The explicit tree is a postorder of contiguous pivot ranges covering [0, n)."""
    beg, end, parent = (np.asarray(a) for a in tree)
    assert len(beg) == len(end) == len(parent) >= 1
    assert beg[0] == 0 and end[-1] == n
    assert np.array_equal(beg[1:], end[:-1]) and np.all(end >= beg)
    for s, a in enumerate(parent):
        assert a == -1 or s < a < len(parent), (s, a)
    return True


# -------------------------------------------------------------------------------------- reference
def _residual_ld(A, x, b):
    """b - A x accumulated in long double. x, b (n, k) long double."""
    A = A.tocsr()
    prod = A.data.astype(LD)[:, None] * x[A.indices]
    assert np.all(np.diff(A.indptr) > 0)   # (reduceat: every row stores its diagonal)
    return b - np.add.reduceat(prod, A.indptr[:-1], axis=0)


def norm_inf_A(A):
    return float(abs(A).sum(axis=1).max())


def reference(A, b, dense=False):
    """x_ref (n, k) in long double with A x_ref = b to long-double rounding."""
    if not HAVE_LONGDOUBLE:
        raise RuntimeError("np.longdouble is not wider than float64 here: no high-precision reference")
    b = np.asarray(b, np.float64)
    if dense or A.shape[0] <= 2:
        Ad = A.toarray()
        solve = lambda r: np.linalg.solve(Ad, r)
    else:
        lu = spla.splu(A.tocsc())
        solve = lu.solve
    bl = b.astype(LD)
    x = solve(b).astype(LD)
    for _ in range(8):
        dx = solve(_residual_ld(A, x, bl).astype(np.float64))
        x = x + dx.astype(LD)
        if np.all(np.abs(dx).max(axis=0) <= 1e-17 * np.abs(x).max(axis=0).astype(np.float64)):
            return x
    raise RuntimeError("reference refinement did not converge")


def err(x, x_ref):
    """max over the columns of |x - x_ref|_inf / |x_ref|_inf."""
    d = np.abs(np.asarray(x, np.float64).astype(LD) - x_ref).max(axis=0)
    return float((d / np.abs(x_ref).max(axis=0)).max())


def berr(A, x, b):
    """|A x - b|_inf / (|A|_inf |x|_inf + |b|_inf), in long double, all columns together."""
    xl = np.asarray(x, np.float64).astype(LD)
    r = _residual_ld(A, xl, np.asarray(b, np.float64).astype(LD))
    return float(np.abs(r).max() / (LD(norm_inf_A(A)) * np.abs(xl).max() + np.abs(b).max()))


def cond2(A):
    """2-norm condition number of an SPD matrix (dense eigenvalues for small n, Lanczos otherwise)."""
    n = A.shape[0]
    if n <= 1200:
        w = np.linalg.eigvalsh(A.toarray())
        return float(w[-1] / w[0])
    hi = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    lo = spla.eigsh(A.tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-6)[0]
    return float(hi / lo)


def rhs(n, seed):
    """(b0, b1): independent (n, 3) normal columns scaled by 1, 1e3, 1e-3."""
    rng = np.random.default_rng(1000003 + seed)
    s = np.array([1.0, 1e3, 1e-3])
    return rng.standard_normal((n, 3)) * s, rng.standard_normal((n, 3)) * s


def unit_rhs(n, row):
    b = np.zeros((n, 3))
    b[row] = [1.0, 1e3, 1e-3]
    return b


# ---------------------------------------------------------------------------------------- cases
SMALL_WAVES = dict(wave_p=16, wave_r=32)
GEOM_WAVES = dict(wave_p=64, wave_r=128)
DEFAULT_WAVES = dict(wave_p=192, wave_r=384)


def _grid_case(name, dims, seed, leaf, top, waves, min_sub, **kw):
    A, xyz = grid_system(*dims, seed, **kw)
    return Case(name, "grid", A, xyz, None, dict(leaf_size=leaf, top_rows=top, **waves),
                {"AA_SOLVE_MIN_SUBTREES": str(min_sub)})


GRID_SPECS = {
    "g12_fused": lambda: _grid_case("g12_fused", (12, 6, 6), 11, 8, 0, SMALL_WAVES, 4),
    "g24_fused": lambda: _grid_case("g24_fused", (24, 10, 12), 12, 8, 0, SMALL_WAVES, 8),
    "g24_levels": lambda: _grid_case("g24_levels", (24, 10, 12), 12, 8, 0, SMALL_WAVES, 4096),
    "g24_wide_rows": lambda: _grid_case("g24_wide_rows", (24, 10, 12), 12, 8, 0, dict(wave_p=24, wave_r=400), 4096),
    "g24_elastic": lambda: _grid_case("g24_elastic", (24, 10, 12), 12, 32, 256, DEFAULT_WAVES, 4),
    "cloth48": lambda: _grid_case("cloth48", (48, 48, 1), 13, 16, 0, GEOM_WAVES, 8),
    "g16_dense_root": lambda: _grid_case("g16_dense_root", (16, 16, 16), 14, 128, 4096, DEFAULT_WAVES, 256),
    "g24_two_roots": lambda: _grid_case("g24_two_roots", (24, 10, 12), 12, 8, 256, SMALL_WAVES, 8, cut_i=12),
    "g14_holes": lambda: _grid_case("g14_holes", (14, 10, 10), 15, 8, 0, SMALL_WAVES, 8, keep_fraction=0.5),
}

SINGLE_P = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 513)
LEAF_P_NB = ((192, 192), (192, 193), (193, 191), (200, 100), (100, 300), (65, 64), (1, 400), (257, 129))
CHAIN = dict(p_leaf=67, p_mid=131, p_root=197, k=3)   # odd throughout; the middle is tiled at 64/128


def _arrow_case(name, built, waves):
    A, xyz, tree = built
    return Case(name, "arrow", A, xyz, tree, dict(leaf_size=0, top_rows=0, **waves), {})


ARROW_SPECS = {}
for _p in SINGLE_P:
    ARROW_SPECS[f"single_p{_p}"] = functools.partial(
        lambda p: _arrow_case(f"single_p{p}", arrow_system(p, 0, 1, 100 + p), DEFAULT_WAVES), _p)
for _p, _nb in LEAF_P_NB:
    ARROW_SPECS[f"arrow_p{_p}_nb{_nb}"] = functools.partial(
        lambda p, nb: _arrow_case(f"arrow_p{p}_nb{nb}", arrow_system(p, nb, 2, 1000 * p + nb), DEFAULT_WAVES), _p, _nb)
ARROW_SPECS["chain_odd"] = lambda: _arrow_case("chain_odd", chain_system(seed=77, **CHAIN), DEFAULT_WAVES)
# once with the geometry solver's thresholds (64 / 128): the same shapes land in other classes
for _p in SINGLE_P:
    ARROW_SPECS[f"single_p{_p}_geom"] = functools.partial(
        lambda p: _arrow_case(f"single_p{p}_geom", arrow_system(p, 0, 1, 100 + p), GEOM_WAVES), _p)
for _p, _nb in LEAF_P_NB + ((64, 64),):
    ARROW_SPECS[f"arrow_p{_p}_nb{_nb}_geom"] = functools.partial(
        lambda p, nb: _arrow_case(f"arrow_p{p}_nb{nb}_geom", arrow_system(p, nb, 2, 1000 * p + nb), GEOM_WAVES), _p, _nb)
ARROW_SPECS["chain_odd_geom"] = lambda: _arrow_case("chain_odd_geom", chain_system(seed=77, **CHAIN), GEOM_WAVES)


def _degenerate(name):
    prm = dict(leaf_size=8, top_rows=0, **SMALL_WAVES)
    if name == "n1":
        A = sp.csr_matrix(np.array([[2.5]]))
        xyz = np.zeros((1, 3))
    elif name == "n2":
        A = sp.csr_matrix(np.array([[2.0, -0.75], [-0.75, 3.0]]))
        xyz = np.array([[0.0, 0, 0], [0.1, 0, 0]])
    elif name == "below_leaf":     # 5 nodes on a path, leaf 8: one supernode
        A, xyz = grid_system(5, 1, 1, 21)
    elif name == "isolated_vertex":   # a 5x4x3 grid whose node 17 has lost all its edges
        A, xyz = grid_system(5, 4, 3, 22)
        A = A.tolil()
        d = A[17, 17]
        nbrs = [j for j in A.rows[17] if j != 17]
        for j in nbrs:
            A[j, j] += A[17, j]   # (the neighbour's diagonal drops that edge's weight)
            A[17, j] = 0.0
            A[j, 17] = 0.0
        A[17, 17] = d
        A = A.tocsr()
        A.eliminate_zeros()
        A.sort_indices()
    elif name == "diagonal":       # every separator empty: many roots
        rng = np.random.default_rng(23)
        A = sp.diags(rng.uniform(0.5, 4.0, 40)).tocsr()
        xyz = rng.random((40, 3))
    else:
        raise KeyError(name)
    return Case(name, "degenerate", A.tocsr(), np.ascontiguousarray(xyz, np.float64), None, prm, {})


DEGENERATE_SPECS = {k: functools.partial(_degenerate, k) for k in ("n1", "n2", "below_leaf", "isolated_vertex", "diagonal")}

ALL_SPECS = {**GRID_SPECS, **ARROW_SPECS, **DEGENERATE_SPECS}


@functools.lru_cache(maxsize=None)
def get_case(name) -> Case:
    return ALL_SPECS[name]()


@functools.lru_cache(maxsize=None)
def case_rhs(name):
    c = get_case(name)
    return rhs(c.n, sum(map(ord, name)))


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(x_ref of b0, x_ref of b1), computed once per case and shared (read only)."""
    c = get_case(name)
    b0, b1 = case_rhs(name)
    x = reference(c.A, np.hstack([b0, b1]), dense=c.family == "arrow")
    x.setflags(write=False)
    return x[:, :3], x[:, 3:]
