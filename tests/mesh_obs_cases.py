"""Meshes, queries and the brute-force fp64 oracle of the triangle-mesh obstacle tests
(tests/test_mesh_obstacle.py on the CPU, tests/test_gpu_mesh_obstacle.py on the GPU).

The oracle restates the obstacle's semantics (include/aa_admm.h, aa_elastic_add_mesh_obstacle)
without any of the library's machinery: Ericson's closest point against every triangle, first
minimum; the angle-weighted pseudonormal of the feature that triangle's region names; inside iff
(q - c) . n < 0. An independent inside test -- the generalized winding number from Van Oosterom &
Strackee solid angles, inside iff > 0.5 -- must agree on every kept query.
"""
import functools

import numpy as np

SEED = 7
REGIONS = ("A", "B", "AB", "C", "CA", "BC", "FACE")   # the order of Ericson's branches
MAX_EXCLUDED = 0.01     # share of a mesh's queries that may be left out


# ----------------------------------------------------------------------------- meshes
def cube():
    V = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # outward
    F = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return V, np.array(F, np.int32)


def l_prism(h=0.6):
    P = np.array([(0, 0), (1, 0), (1, 0.5), (0.5, 0.5), (0.5, 1), (0, 1)], float)   # CCW, concave at P[3]
    n = len(P)
    V = np.array([(x, y, 0.0) for x, y in P] + [(x, y, h) for x, y in P])
    fan = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]
    F = [(a, c, b) for a, b, c in fan] + [(a + n, b + n, c + n) for a, b, c in fan]
    for i in range(n):
        j = (i + 1) % n
        F += [(i, j, j + n), (i, j + n, i + n)]
    return V, np.array(F, np.int32)


def torus(nu=16, nv=8, R=0.35, r=0.15):
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    U, W = np.meshgrid(u, v, indexing="ij")
    V = np.stack([(R + r * np.cos(W)) * np.cos(U), r * np.sin(W), (R + r * np.cos(W)) * np.sin(U)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    F = []
    for i in range(nu):
        for j in range(nv):
            for t in ((idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i + 1, j))):
                k = (i + j) % 3   # rotate the corners so that every vertex is some first-found triangle's a, b and c
                F.append(t[k:] + t[:k])
    return V, np.array(F, np.int32)


def sliver():
    """A thin wedge: the two faces on edge (0, 1) meet at about 11 degrees, so a point just outside
    that edge lies behind the plane of one of them."""
    V = np.array([(0, 0, 0), (1, 0, 0), (0.5, 0.8, 0.08), (0.5, 0.8, -0.08)], float)
    return V, np.array([(0, 1, 2), (1, 0, 3), (0, 2, 3), (1, 3, 2)], np.int32)


def box(lo, hi):
    V, F = cube()
    return np.asarray(lo, float) + V * (np.asarray(hi, float) - np.asarray(lo, float)), F


MESHES = {"cube": cube, "l_prism": l_prism, "torus": torus, "sliver": sliver}
N_TRIS = {"cube": 12, "l_prism": 20, "torus": 256, "sliver": 4}


def signed_volume(V, F):
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def queries(V, F, seed=SEED):
    """2 000 uniform in the bounding box inflated by 25 %, 300 at vertices + N(0, 0.05^2), 300 at
    edge midpoints + the same noise."""
    rng = np.random.default_rng(seed)
    lo, hi = V.min(0), V.max(0)
    ext = hi - lo
    Q0 = rng.uniform(lo - 0.125 * ext, hi + 0.125 * ext, size=(2000, 3))
    Q1 = V[rng.integers(0, len(V), 300)] + rng.normal(0.0, 0.05, size=(300, 3))
    E = np.unique(np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1), axis=0)
    e = E[rng.integers(0, len(E), 300)]
    Q2 = 0.5 * (V[e[:, 0]] + V[e[:, 1]]) + rng.normal(0.0, 0.05, size=(300, 3))
    return np.concatenate([Q0, Q1, Q2])


# ----------------------------------------------------------------------------- oracle
def ericson(V, F, Q):
    """Closest point of every query on every triangle: (C (n, m, 3), region (n, m))."""
    a, b, c = (V[F[:, k]][None, :, :] for k in range(3))
    p = Q[:, None, :]
    dot = lambda x, y: (x * y).sum(-1)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0),
             (d3 >= 0) & (d4 <= d3),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0),
             (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    region = np.select(conds, [0, 1, 2, 3, 4, 5], default=6)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab = (d1 / (d1 - d3))[..., None]
        t_ca = (d2 / (d2 - d6))[..., None]
        t_bc = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
        den = 1.0 / (va + vb + vc)
        cand = [a + 0 * p, b + 0 * p, a + t_ab * ab, c + 0 * p, a + t_ca * ac, b + t_bc * (c - b),
                a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]]
    C = np.zeros(region.shape + (3,))
    for k in range(7):
        m = region == k
        C[m] = cand[k][m]
    return C, region


def pseudonormals(V, F):
    """(face (m, 3), edge {(lo, hi): n}, vertex (nv, 3)) angle-weighted pseudonormals."""
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    fn = np.cross(b - a, c - a)
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    vn = np.zeros_like(V)
    en = {}
    for t, f in enumerate(F):
        for k in range(3):
            p, q, r = int(f[k]), int(f[(k + 1) % 3]), int(f[(k + 2) % 3])
            e1, e2 = V[q] - V[p], V[r] - V[p]
            ang = np.arccos(np.clip(e1 @ e2 / np.sqrt((e1 @ e1) * (e2 @ e2)), -1.0, 1.0))
            vn[p] += ang * fn[t]
            en[(min(p, q), max(p, q))] = en.get((min(p, q), max(p, q)), 0.0) + fn[t]
    return fn, en, vn


def feature_normal(F, pn, t, region):
    fn, en, vn = pn
    f = F[t]
    if region == 6:
        return fn[t]
    if region in (0, 1, 3):
        return vn[f[{0: 0, 1: 1, 3: 2}[region]]]
    p, q = {2: (f[0], f[1]), 4: (f[2], f[0]), 5: (f[1], f[2])}[region]
    return en[(min(p, q), max(p, q))]


def winding_number(V, F, Q):
    a, b, c = (V[F[:, k]][None] - Q[:, None] for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)


class Oracle:
    """Per query: closest point c, first-minimum triangle tri, its region, inside flag, |q - c|,
    `keep` (not excluded), `unique` (no other triangle within a relative 1e-9 of the minimum),
    the winding-number inside flag `inside_wn` and the naive rule's `inside_naive` (the face normal
    of the first-found triangle)."""

    def __init__(self, V, F, Q):
        pn = pseudonormals(V, F)
        C, R = ericson(V, F, Q)
        d = np.linalg.norm(Q[:, None] - C, axis=-1)
        n = len(Q)
        self.tri = d.argmin(1)
        i = np.arange(n)
        self.c, self.region, self.dist = C[i, self.tri], R[i, self.tri], d[i, self.tri]
        N = np.array([feature_normal(F, pn, self.tri[k], self.region[k]) for k in range(n)])
        self.inside = ((Q - self.c) * N).sum(1) < 0
        self.inside_naive = ((Q - self.c) * pn[0][self.tri]).sum(1) < 0
        self.inside_wn = winding_number(V, F, Q) > 0.5
        near = d <= self.dist[:, None] * (1.0 + 1e-9)
        other = np.linalg.norm(C - self.c[:, None], axis=-1) > 1e-9
        self.unique = near.sum(1) == 1
        self.keep = ~((self.dist < 1e-12) | (near & other).any(1))
        self.dx = np.where(self.inside, -self.dist, self.dist)


@functools.lru_cache(maxsize=None)
def case(name):
    """(V, F, Q, Oracle) of a mesh; computed once per session and shared (do not modify)."""
    V, F = MESHES[name]()
    Q = queries(V, F)
    return V, F, Q, Oracle(V, F, Q)


# ----------------------------------------------------------------------------- ordering rule
OBS_FLOOR, OBS_SPHERE, OBS_MESH = 0, 2, 5


def collision_prox_rule(obstacles, mesh_oracles, Q):
    """Collision::prox on candidates Q in numpy: the obstacles compete in insertion order with
    `if (dx > best) continue`, except that a mesh's inside hit replaces the running (dx, point)
    unconditionally and a miss leaves it untouched. mesh_oracles[m] is the Oracle of mesh m on Q."""
    n = len(Q)
    best = np.full(n, np.finfo(float).max)
    pt = np.zeros((n, 3))
    for kind, prm in obstacles:
        if kind == OBS_FLOOR:
            dx = Q[:, 1] - prm[0]
            p = Q.copy()
            p[:, 1] = prm[0]
            take = ~(dx > best)
        elif kind == OBS_SPHERE:
            ctr, r = np.asarray(prm[:3], float), prm[3]
            d = Q - ctr
            nrm = np.linalg.norm(d, axis=1)
            dx = nrm - r
            p = ctr + d / nrm[:, None] * r
            take = ~(dx > best)
        else:
            o = mesh_oracles[int(prm[0])]
            dx, p, take = -o.dist, o.c, o.inside
        best = np.where(take, dx, best)
        pt = np.where(take[:, None], p, pt)
    return np.where((best < 0)[:, None], pt, Q)
