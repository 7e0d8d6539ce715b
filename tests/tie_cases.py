"""Shared oracle of the tie tests (tests/test_ties.py, tests/test_gpu_ties.py).

A tie (aa_elastic_add_ties) is a spring between two barycentric anchors: one reduction row
(-a_0 .. -a_{na-1}, +b_0 .. +b_{nb-1}) over its na + nb nodes, weight sqrt(k), the spring's prox. This
module restates the host builder in numpy (ties()) and extends tests/spring_cases.py's port of the
(u,x) loop: TieProblem appends the tie rows after the spring rows and registers each entry of
Scene.ties as one more spring group, so spring_cases.admm_ux(scene, problem=TieProblem) is the port
(its prox loop, margin and mixed bookkeeping included). The port forms D x with numpy's matrix
product; the kernels sum a tie's terms over its vertices in stored order, left to right from 0, one
fused multiply-add each. The two differ by rounding, which the trajectory tolerances cover.

The scenes follow the issue's definitions; T is the pinned, moving triangle they hang from.
"""
import dataclasses

import numpy as np

import bending_cases as bc
import spring_cases as sp
from golden_io import compare, scenes

SPRING, TETHER, STRUT, HARD = sp.SPRING, sp.TETHER, sp.STRUT, sp.HARD


# ------------------------------------------------------------------------------------------ model
def ties(V, nodes_a, w_a, nodes_b, w_b, k, rest=None):
    """(idx (m, nv), G (m, nv), L (m,), w (m,)) as the host builder makes them: vertices A's then B's,
    G = (-a, +b); derived L with each anchor summed left to right from its first term."""
    w_a, w_b = np.asarray(w_a, np.float64), np.asarray(w_b, np.float64)
    m, na, nb = w_a.shape[0], w_a.shape[1], w_b.shape[1]
    ia, ib = np.asarray(nodes_a, np.int64).reshape(m, na), np.asarray(nodes_b, np.int64).reshape(m, nb)
    k = np.broadcast_to(np.asarray(k, np.float64), (m,))
    if rest is None:
        V = np.asarray(V, np.float64)
        pa = w_a[:, 0, None] * V[ia[:, 0]]
        for i in range(1, na):
            pa = pa + w_a[:, i, None] * V[ia[:, i]]
        pb = w_b[:, 0, None] * V[ib[:, 0]]
        for j in range(1, nb):
            pb = pb + w_b[:, j, None] * V[ib[:, j]]
        L = sp.norm3(pb - pa)
    else:
        L = np.broadcast_to(np.asarray(rest, np.float64), (m,)).copy()
    return np.concatenate([ia, ib], 1), np.concatenate([-w_a, w_b], 1), L, np.sqrt(k)


def anchors(x, entry):
    """(p_A, p_B) of a Scene.ties entry at the positions x."""
    ia, wa, ib, wb = (np.asarray(a) for a in entry[:4])
    x = np.asarray(x, np.float64).reshape(-1, 3)
    return (wa[:, :, None] * x[ia]).sum(1), (wb[:, :, None] * x[ib]).sum(1)


# ------------------------------------------------------------------------------------------ the port
class TieProblem(sp.SpringProblem):
    """SpringProblem plus one row per tie, after the spring rows."""

    def __init__(self, scene):
        super().__init__(scene)
        n = scene.n_nodes
        rows, w = [], []
        r0 = self.D.shape[0]
        for ia, wa, ib, wb, k, L, mode in (getattr(scene, "ties", None) or []):
            idx, G, L, ws = ties(scene.rest_x, ia, wa, ib, wb, k, L)
            self.spring_groups.append((np.arange(r0 + len(rows), r0 + len(rows) + len(idx)), L, int(mode)))
            for e in range(len(idx)):
                row = np.zeros(n)
                row[idx[e]] += G[e]
                rows.append(row)
                w.append(ws[e])
        if rows:
            self.D = np.vstack([self.D, np.array(rows)]) if self.D.size else np.array(rows)
            self.w = np.concatenate([self.w, np.array(w)])


def admm_ux(scene, **kw):
    return sp.admm_ux(scene, problem=TieProblem, **kw)


def dense_minimiser(scene):
    """spring_cases.dense_minimiser statement by statement with TieProblem (that function constructs
    SpringProblem by name): the exact first-step minimiser of a scene whose terms are all quadratic.
    Returns (x* on all nodes, max |x* - xbar|)."""
    P = TieProblem(scene)
    n = scene.n_nodes
    pins = np.asarray(scene.pin_idx, np.int64)
    is_pin = np.zeros(n, bool)
    is_pin[pins] = True
    free = np.nonzero(~is_pin)[0]
    m, dt = np.asarray(scene.masses, np.float64), scene.dt
    x = np.array(scene.x, np.float64)
    v = np.zeros((n, 3))
    v[free, 1] += dt * scene.gravity
    xbar = x[free] + dt * v[free]
    WD = P.w[:, None] * P.D
    A = np.diag(m[free]) + dt * dt * (WD[:, free].T @ WD[:, free])
    xpin = np.asarray(scene.pin_pts, np.float64) + np.asarray(scene.pin_vel, np.float64)
    rhs = m[free, None] * xbar - dt * dt * (WD[:, free].T @ (WD[:, pins] @ xpin))
    out = x.copy()
    out[pins] = xpin
    out[free] = np.linalg.solve(A, rhs)
    return out, float(np.abs(out[free] - xbar).max())


# ------------------------------------------------------------------------------------------ scenes
T_X = np.array([[-0.3, 0.0, -0.2], [0.4, 0.0, -0.1], [0.0, 0.0, 0.5]])
T_VEL = np.array([[0.02, 0.01, 0.0], [0.02, -0.01, 0.0], [0.0, 0.01, 0.01]])
TET_X = np.vstack([T_X, [[0.05, 0.4, 0.1]]])
TET_VEL = np.vstack([T_VEL, [[0.01, 0.0, 0.0]]])
PENDANT_W3 = np.array([[0.2, 0.3, 0.5], [0.6, 0.3, 0.1], [0.15, 0.7, 0.15]])
PENDANT_W4 = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.2, 0.2, 0.1], [0.1, 0.6, 0.1, 0.2]])
PENDANT_OFF = np.array([[0.1, -0.35, 0.05], [-0.05, -0.3, 0.1], [0.0, -0.4, -0.1]])


def _scene(x, n_pins, pin_vel, springs, ties_, *, mass=0.01, **kw):
    x = np.array(x, np.float64)
    pins = np.arange(n_pins, dtype=np.int32)
    kw.setdefault("iters", 30)
    return scenes.Scene(x=x, masses=np.full(len(x), float(mass)), groups=[], pin_idx=pins, pin_pts=x[pins].copy(),
                        pin_vel=np.asarray(pin_vel, np.float64).reshape(n_pins, 3), variant=scenes.VARIANT_H, springs=springs,
                        ties=ties_, **kw)


def _hung(base, vel, W, off, mode, L, ring, **kw):
    """Free masses hung by node-anchor ties (anchor A on the pinned simplex `base`, B the mass) of
    k = 50, started at their anchor plus `off`; soft springs (k = 30, derived L) along `ring`."""
    nb, m = len(base), len(W)
    W, base = np.asarray(W, np.float64), np.asarray(base, np.float64)
    p = W[:, 0, None] * base[0]
    for i in range(1, nb):   # left to right: tests/cpp/facade_ties.cpp forms the same bits
        p = p + W[:, i, None] * base[i]
    x = np.vstack([base, p + off])
    ia = np.tile(np.arange(nb, dtype=np.int32), (m, 1))
    ib = (nb + np.arange(m, dtype=np.int32)).reshape(-1, 1)
    tie = (ia, np.array(W, np.float64), ib, np.ones((m, 1)), 50.0, np.full(m, float(L)), int(mode))
    return _scene(x, nb, vel, [(np.asarray(ring, np.int32) + nb, 30.0, None, SPRING)], [tie], **kw)


def pendants(mode=SPRING, L=0.3, **kw):
    kw.setdefault("n_steps", 3)
    return _hung(T_X, T_VEL, PENDANT_W3, PENDANT_OFF, mode, L, [[0, 1], [1, 2], [2, 0]], aa_m=4, name="pendants", **kw)


def pendants_tet(mode=SPRING, L=0.3, **kw):
    kw.setdefault("n_steps", 3)
    return _hung(TET_X, TET_VEL, PENDANT_W4, PENDANT_OFF, mode, L, [[0, 1], [1, 2], [2, 0]], aa_m=4, name="pendants_tet", **kw)


def fringe300(mode=SPRING, **kw):
    rng = np.random.default_rng(5)
    W = rng.dirichlet([2, 2, 2], 300)
    off = np.stack([0.05 * rng.normal(size=300), -0.3 - 0.1 * rng.random(300), 0.05 * rng.normal(size=300)], 1)
    ring = [[i, i + 1] for i in range(299)]
    kw.setdefault("n_steps", 2)
    return _hung(T_X, T_VEL, W, off, mode, 0.3, ring, aa_m=4, name="fringe300", **kw)


def panel_mesh():
    V, F = scenes.tri_grid(3, 3)
    V2 = V + np.array([0.03, -0.15, -0.02])
    return np.concatenate([V, V2]), np.concatenate([F, F + len(V)]).astype(np.int32), len(V), len(F)


def panel_ties(x, F, nF, lo, hi, k=5.0, mode=SPRING, rest="scaled"):
    rng = np.random.default_rng(1)
    ta = rng.choice(nF, 6, False)
    tb = rng.choice(nF, 6, False)
    w_a = rng.dirichlet([2, 2, 2], 6)
    w_b = rng.dirichlet([2, 2, 2], 6)
    f = np.where(rng.random(6) < 0.5, lo, hi)
    entry = (F[:nF][ta].astype(np.int32), w_a, F[nF:][tb].astype(np.int32), w_b, float(k))
    if isinstance(rest, str):
        pa, pb = anchors(x, entry)
        return entry + (f * sp.norm3(pb - pa), int(mode))
    return entry + (rest, int(mode))


def panels(mode=SPRING, lo=0.9, hi=0.9, *, pins=(0, 3), rest="scaled", k=5.0, **kw):
    """Two 4 x 4-node panels, one under the other, joined by six triangle-triangle ties (nv = 6)."""
    x, F, nV, nF = panel_mesh()
    kw.setdefault("n_steps", 2)
    sc = bc._scene(x, F, list(pins), bend=None, name="panels", **kw)
    sc.ties = [panel_ties(x, F, nF, lo, hi, k, mode, rest)]
    return sc


def skew_edges(mode=SPRING, **kw):
    """The shapes the other scenes do not reach: a node-edge tie (nv = 3: node 3 from the point
    (0.35, 0.65) of T's edge (0, 1)) and an edge-edge tie (nv = 4: the point (0.4, 0.6) of the free edge
    (4, 5) from the point (0.7, 0.3) of T's edge (1, 2)), k = 50, L = 0.3, each a group of its own; the
    three free masses are joined in a ring by soft springs (k = 30, derived L) as in pendants."""
    pa1 = 0.35 * T_X[0] + 0.65 * T_X[1]
    pa2 = 0.7 * T_X[1] + 0.3 * T_X[2]
    x = np.vstack([T_X, pa1 + PENDANT_OFF[0], pa2 + PENDANT_OFF[1] + [0.1, 0.0, -0.05], pa2 + PENDANT_OFF[2] + [-0.1, 0.05, 0.1]])
    t1 = (np.array([[0, 1]], np.int32), np.array([[0.35, 0.65]]), np.array([[3]], np.int32), np.ones((1, 1)), 50.0, np.array([0.3]), int(mode))
    t2 = (np.array([[1, 2]], np.int32), np.array([[0.7, 0.3]]), np.array([[4, 5]], np.int32), np.array([[0.4, 0.6]]), 50.0,
          np.array([0.3]), int(mode))
    kw.setdefault("n_steps", 3)
    return _scene(x, 3, T_VEL, [(np.array([[3, 4], [4, 5], [5, 3]], np.int32), 30.0, None, SPRING)], [t1, t2], aa_m=4,
                  name="skew_edges", **kw)


# Every trajectory the GPU is held to, shared with the CPU conditioning test.
TRAJ = {
    "pendants": lambda: pendants(),
    "pendants_tet": lambda: pendants_tet(),
    "fringe300": lambda: fringe300(),
    "pendants_hard": lambda: pendants(HARD),
    "pendants_tet_hard": lambda: pendants_tet(HARD),
    "pendants_hard_strut": lambda: pendants(HARD | STRUT, 0.45),
    "pendants_hard_tether": lambda: pendants(HARD | TETHER, 0.3),
    "panels_m0": lambda: panels(accel=0),
    "panels_m3": lambda: panels(aa_m=3),
    "panels_m5": lambda: panels(aa_m=5),
    "panels_tether": lambda: panels(TETHER, 0.85, 1.2),
    "panels_strut": lambda: panels(STRUT, 0.85, 1.2),
    "panels_hard_tether": lambda: panels(HARD | TETHER, 0.85, 1.2),
    "fringe300_tether": lambda: fringe300(TETHER),
    "skew_edges": lambda: skew_edges(),
}


def tie_mode(sc):
    return sc.ties[0][6]


_PORT = {}


def port(name):
    """(scene, the port's run, its problem object), computed once per name and left unchanged."""
    if name not in _PORT:
        sc = TRAJ[name]()
        keep = {}
        _PORT[name] = (sc, admm_ux(sc, keep=keep), keep["P"])
    return _PORT[name]


def one_ulp_noise(sc, seed=7):
    """The scene with every initial coordinate moved by one ulp up or down; the rest shape (the
    membrane's, the derived lengths') stays the unperturbed one."""
    up = np.random.default_rng(seed).random(sc.x.shape) < 0.5
    x = np.where(up, np.nextafter(sc.x, np.inf), np.nextafter(sc.x, -np.inf))
    return dataclasses.replace(sc, x=x, rest=np.array(sc.rest_x, np.float64))


def deviations(want, got):
    """Worst (comb / comb_0, prim / prim_0) over the steps, final x and v relative."""
    dc = max(np.abs(w["comb"][:min(len(w["comb"]), len(g["comb"]))] - g["comb"][:min(len(w["comb"]), len(g["comb"]))]).max() / w["comb"][0]
             for w, g in zip(want, got))
    dp = max(np.abs(w["prim"][:min(len(w["prim"]), len(g["prim"]))] - g["prim"][:min(len(w["prim"]), len(g["prim"]))]).max() / w["prim"][0]
             for w, g in zip(want, got))
    gx, gv = np.asarray(got[-1]["x"]).reshape(-1, 3), np.asarray(got[-1]["v"]).reshape(-1, 3)
    return (dc, dp, np.linalg.norm(gx - want[-1]["x"]) / np.linalg.norm(want[-1]["x"]),
            np.linalg.norm(gv - want[-1]["v"]) / np.linalg.norm(want[-1]["v"]))


def check_trajectory(want, got, tol):
    """golden_io.compare at tol (curves tol comb_0 and 10 tol prim_0, reject flags over 20 iterations,
    final x tol relative) plus equal record counts and final v at tol relative: the list of failures."""
    got = [dict(g) for g in got]
    got[-1]["x"] = np.asarray(got[-1]["x"]).reshape(-1, 3)
    fails = [f"step {k}: {len(g['comb'])} records, port {len(w['comb'])}" for k, (w, g) in enumerate(zip(want, got))
             if len(w["comb"]) != len(g["comb"])]
    fails += compare(want, got, tol, tol)
    dv = deviations(want, got)[3]
    if not dv <= tol:
        fails.append(f"final v rel err {dv:.3e} (tol {tol:g})")
    return fails


# ------------------------------------------------------------------------------------------ closed forms
def hanging_mass_scene(n_steps=60):
    """One mass hung by a soft tie (k = 36, L = 0.5) from the point (0.2, 0.3, 0.5) of the pinned,
    standing T, started at rest length straight below it; spring_cases.hanging_mass_scene's numbers
    (omega dt = 2, no Anderson, 40 iterations)."""
    w = np.array([[0.2, 0.3, 0.5]])
    x = np.vstack([T_X, w @ T_X + [0.0, -0.5, 0.0]])
    tie = (np.array([[0, 1, 2]], np.int32), w, np.array([[3]], np.int32), np.ones((1, 1)), 36.0, np.array([0.5]), SPRING)
    return _scene(x, 3, np.zeros((3, 3)), None, [tie], n_steps=n_steps, accel=0, iters=40, name="hanging_tie")


def hanging_mass_error(out, sc):
    """(|extension - m g / k|, sideways drift) after the last step."""
    x = np.asarray(out[-1]["x"]).reshape(-1, 3)
    pa, pb = anchors(x, sc.ties[0])
    d = (pb - pa)[0]
    return abs((-d[1] - 0.5) - sc.masses[3] * abs(sc.gravity) / sc.ties[0][4]), float(np.hypot(d[0], d[2]))


def two_triangles_scene(n_steps=5):
    """Two free triangles, each stiffened by three springs (k = 80, derived L), joined by one
    triangle-triangle tie with dyadic weights (each side sums to 1 exactly), k = 20, L = 0.4; no
    gravity, no pins: the tie's row sums to zero, so the total momentum stays zero."""
    A = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.05], [0.1, 0.05, 0.3]])
    B = A[:, [2, 1, 0]] * [1.0, -1.0, 1.0] + [0.1, 0.6, -0.05]
    x = np.vstack([A, B])
    edges = np.array([[0, 1], [1, 2], [2, 0], [3, 4], [4, 5], [5, 3]], np.int32)
    tie = (np.array([[0, 1, 2]], np.int32), np.array([[0.5, 0.25, 0.25]]), np.array([[3, 4, 5]], np.int32),
           np.array([[0.125, 0.625, 0.25]]), 20.0, np.array([0.4]), SPRING)
    sc = _scene(x, 0, np.zeros((0, 3)), [(edges, 80.0, None, SPRING)], [tie], n_steps=n_steps, aa_m=4, gravity=0.0, name="two_triangles")
    sc.masses = np.array([0.01, 0.02, 0.015, 0.012, 0.01, 0.018])
    return sc


def momentum_ratio(out, sc):
    """max over the steps of |sum m v|inf / sum m |v|."""
    m = np.asarray(sc.masses)[:, None]
    worst = 0.0
    for o in out:
        v = np.asarray(o["v"]).reshape(-1, 3)
        worst = max(worst, float(np.abs((m * v).sum(0)).max() / (m * np.abs(v)).sum()))
    return worst


def zero_length_panels(iters=100):
    """Zero-length soft ties only, on the panels' nodes (a quadratic problem; the membrane's prox is
    not quadratic and is left out): panels' six ties with L = 0, nodes 0 and 3 pinned, no Anderson,
    one step."""
    x, F, nV, nF = panel_mesh()
    sc = bc._scene(x, F, [0, 3], bend=None, membrane=False, masses=scenes.tri_masses(x, F, 1.0), n_steps=1, accel=0, iters=iters,
                   name="zero_length_panels")
    sc.ties = [panel_ties(x, F, nF, 1.0, 1.0, 5.0, SPRING, rest=np.zeros(6))]
    return sc


def long_ties_13(**kw):
    """spring_cases.long_ties_13's pattern with node-triangle ties: a 13 x 13 cloth whose x = 0 edge
    nodes are each tied to a point of a triangle at the far edge, and likewise between the z edges,
    0.9 of that distance long: 26 ties across the top bisection of the dissection."""
    V, F = scenes.tri_grid(12, 12)
    sc = bc._scene(V, F, [0, 168], bend=None, n_steps=2, **kw)
    src = np.array([13 * j for j in range(13)] + [i for i in range(13)], np.int32)
    far = np.array([13 * j + 12 for j in range(13)] + [156 + i for i in range(13)], np.int32)
    tri = np.array([int(np.nonzero((F == f).any(1) & ~(F == s).any(1))[0][0]) for s, f in zip(src, far)])
    w = np.tile(np.array([[0.5, 0.3, 0.2]]), (26, 1))
    entry = (F[tri].astype(np.int32), w, src.reshape(-1, 1), np.ones((26, 1)), 5.0)
    pa, pb = anchors(V, entry)
    sc.ties = [entry + (0.9 * sp.norm3(pb - pa), SPRING)]
    sc.name = "long_ties_13"
    return sc
