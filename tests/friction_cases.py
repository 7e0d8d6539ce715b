"""The numpy restatement of the friction pass (include/aa_admm.h, aa_elastic_set_obstacle_friction;
csrc/device_prox.hpp contact_friction) and the cases of its tests: tests/test_friction.py on the
CPU, tests/test_gpu_friction.py on the GPU.

Every function states the device's arithmetic operation by operation. numpy's elementwise fp64
add, multiply, divide and sqrt are correctly rounded and never contracted into an FMA, and every
sum is parenthesised left to right as the device writes it, so the results are meant to agree with
the device's bit for bit (the idiom of kinematic_cases.to_local / to_world, which are reused for
the pose transforms).
"""
import types

import numpy as np

import kinematic_cases as kc
import mesh_obs_cases as mc

OBS_FLOOR, OBS_SLIDE_FLOOR, OBS_SPHERE, OBS_PLANE_HALF_SPHERE, OBS_CYLINDER, OBS_MESH = range(6)
DBL_MAX = np.finfo(float).max


def candidate(x, u, w):
    """collision_candidate: q = (1/w) (w x + u)."""
    w = np.broadcast_to(np.asarray(w, float), (len(x),))[:, None]
    iw = 1.0 / w
    return iw * (w * x + u)


def row_of(kind, prm):
    """The 8 doubles of an obstacle row as the solver stores it (SLIDE_FLOOR: the normal normalised)."""
    o = np.zeros(8)
    a = np.asarray(prm, float).reshape(-1)
    o[0] = kind
    o[1:1 + len(a)] = a
    if kind == OBS_SLIDE_FLOOR:
        z2 = (o[4] * o[4] + o[5] * o[5]) + o[6] * o[6]
        if z2 > 0.0:
            o[4:7] = o[4:7] / np.sqrt(z2)
    return o


def _sq3(a, b, c):
    return (a * a + b * b) + c * c


def contact_rule(obstacles, mesh_oracles, Q, exempt=None):
    """The obstacle walk of Collision::prox on candidates Q, also reporting the row that supplied the
    final (dx, point): (hit, row, c). obstacles: (type, params) in insertion order, rows as given to
    the device (a SLIDE_FLOOR normal of unit length); mesh_oracles[m]: an object with dist, c, inside
    per query (mesh_obs_cases.Oracle, kinematic_cases.local_oracle); exempt[m]: per query, True =
    this query's node skips mesh m."""
    n = len(Q)
    best = np.full(n, DBL_MAX)
    pt = np.zeros((n, 3))
    row = np.full(n, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, (kind, prm) in enumerate(obstacles):
            o = np.zeros(8)
            o[1:1 + len(prm)] = np.asarray(prm, float)
            if kind == OBS_FLOOR:
                dx = Q[:, 1] - o[1]
                p = np.stack([Q[:, 0], np.full(n, o[1]), Q[:, 2]], 1)
                take = ~(dx > best)
            elif kind == OBS_SLIDE_FLOOR:
                l0, l1, l2 = Q[:, 0] - o[1], Q[:, 1] - o[2], Q[:, 2] - o[3]
                dx = l0 * o[4] + l1 * o[5] + l2 * o[6]
                p = np.stack([Q[:, 0] - dx * o[4], Q[:, 1] - dx * o[5], Q[:, 2] - dx * o[6]], 1)
                take = ~(dx > best)
            elif kind in (OBS_SPHERE, OBS_CYLINDER):
                d0, d1 = Q[:, 0] - o[1], Q[:, 1] - o[2]
                d2 = Q[:, 2] - o[3] if kind == OBS_SPHERE else np.full(n, 0.0 - o[3])
                z2 = _sq3(d0, d1, d2)
                nrm = np.sqrt(z2)
                dx = nrm - o[4]
                ok = z2 > 0.0
                d0, d1, d2 = (np.where(ok, d / nrm, d) for d in (d0, d1, d2))
                if kind == OBS_SPHERE:
                    p = np.stack([o[1] + d0 * o[4], o[2] + d1 * o[4], o[3] + d2 * o[4]], 1)
                else:
                    p = np.stack([o[1] + d0 * o[4] + 0.0, o[2] + d1 * o[4] + 0.0, o[3] + d2 * o[4] + Q[:, 2]], 1)
                take = ~(dx > best)
            elif kind == OBS_PLANE_HALF_SPHERE:
                dc = np.sqrt(_sq3(Q[:, 0] - o[1], np.zeros(n), Q[:, 2] - o[3])) - o[4]
                dpl = Q[:, 1] - o[2]
                d0, d1, d2 = Q[:, 0] - o[1], Q[:, 1] - o[2], Q[:, 2] - o[3]
                z2 = _sq3(d0, d1, d2)
                nrm = np.sqrt(z2)
                ok = z2 > 0.0
                d0, d1, d2 = (np.where(ok, d / nrm, d) for d in (d0, d1, d2))
                dx_s = np.where(dpl > 0, nrm + o[4], o[4] - nrm)
                p_s = np.stack([o[1] + d0 * o[4], o[2] + d1 * o[4], o[3] + d2 * o[4]], 1)
                p_f = np.stack([Q[:, 0], np.full(n, o[2]), Q[:, 2]], 1)
                flat = dc > 0
                dx = np.where(flat, dpl, dx_s)
                p = np.where(flat[:, None], p_f, p_s)
                take = ~(dx > best)
            else:
                m = int(prm[0])
                om = mesh_oracles[m]
                dx, p, take = -om.dist, om.c, om.inside.copy()
                if exempt is not None and exempt[m] is not None:
                    take &= ~np.asarray(exempt[m], bool)
            best = np.where(take, dx, best)
            pt = np.where(take[:, None], p, pt)
            row = np.where(take, k, row)
    return best < 0, row, pt


def obstacle_displacement(rows, rows_prev, poses, poses_prev, still, row, c):
    """Step 5: g at the contact points c (n, 3) of obstacle rows `row` (n,). rows / rows_prev: (k, 8)
    stored rows now and during the previous step; poses / poses_prev: per mesh (R, t) or None (the
    identity); still: per mesh, True = g is 0."""
    g = np.zeros_like(c)
    for k in np.unique(row[row >= 0]):
        sel = row == k
        o, op = rows[k], rows_prev[k]
        kind = int(o[0])
        if kind == OBS_MESH:
            m = int(o[1])
            if still is not None and still[m]:
                continue
            R, t = poses[m] if poses is not None and poses[m] is not None else kc.IDENTITY
            Rp, tp = poses_prev[m] if poses_prev is not None and poses_prev[m] is not None else kc.IDENTITY
            cl = kc.to_local(np.asarray(R, float), np.asarray(t, float), c[sel])
            g[sel] = c[sel] - kc.to_world(np.asarray(Rp, float), np.asarray(tp, float), cl)
        elif kind == OBS_FLOOR:
            g[sel, 1] = o[1] - op[1]
        else:
            g[sel] = o[1:4] - op[1:4]
    return g


def friction_steps(q, c, hit, u, x_old, x_new, g, w, m, p, dt, mu_r, pinned=None):
    """Steps 3 to 6 on the contacts `hit`, given the device's contact points c: a namespace of
    hit (after the l == 0 rule), n, j, rt, s and x'. mu_r: the coefficient of each query's row."""
    n_q = len(q)
    w = np.broadcast_to(np.asarray(w, float), (n_q,))
    m = np.broadcast_to(np.asarray(m, float), (n_q,))
    mu_r = np.broadcast_to(np.asarray(mu_r, float), (n_q,))
    pinned = np.zeros(n_q, bool) if pinned is None else np.asarray(pinned, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = c - q
        l = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        hit = hit & ~(l == 0.0)
        n = e / l[:, None]
        un = (u[:, 0] * n[:, 0] + u[:, 1] * n[:, 1]) + u[:, 2] * n[:, 2]
        k = (((p * dt) * dt) * w) / m
        j = np.where(un < 0.0, k * (-un), 0.0)
        rel = (x_new - x_old) - g
        rn = (rel[:, 0] * n[:, 0] + rel[:, 1] * n[:, 1]) + rel[:, 2] * n[:, 2]
        rt = rel - rn[:, None] * n
        lt = np.sqrt((rt[:, 0] * rt[:, 0] + rt[:, 1] * rt[:, 1]) + rt[:, 2] * rt[:, 2])
        off = (mu_r == 0.0) | (j == 0.0) | ~(lt > 0.0) | pinned
        a = (mu_r * j) / lt
        s = np.where(off, 0.0, np.where(a < 1.0, a, 1.0))
    z3 = np.zeros((n_q, 3))
    n = np.where(hit[:, None], n, z3)
    rt = np.where(hit[:, None], rt, z3)
    j = np.where(hit, j, 0.0)
    s = np.where(hit, s, 0.0)
    x = np.where((s != 0.0)[:, None], x_new - s[:, None] * rt, x_new)
    return types.SimpleNamespace(hit=hit, n=n, j=j, rt=rt, s=s, x=x, lt=np.where(hit, lt, 0.0))


# ----------------------------------------------------------------------------- hook cases
W, PENALTY, DT = 3.7, 1.3, 1.0 / 30.0
N_Q = 300


def queries_near(Q, seed, mu_rows):
    """Per-query state around candidates Q (n, 3): a random dual u (both signs along any normal),
    x_new = Q - u / w (so the candidate lands at Q up to rounding), x_old a small step away, a
    mass. The sizes are chosen so that mu j / lt falls on both sides of 1 for the coefficients used."""
    rng = np.random.default_rng(seed)
    n = len(Q)
    u = rng.normal(0.0, 1.0, size=(n, 3))
    x_new = Q - u / W
    x_old = x_new - rng.normal(0.0, 3e-3, size=(n, 3))
    m = rng.uniform(0.5, 2.0, size=n)
    return types.SimpleNamespace(u=u, x_new=x_new, x_old=x_old, m=m, w=np.full(n, W), mu=np.asarray(mu_rows, float))


def straddle(fn_point, n, seed, spread=0.08):
    """n points at surface points fn_point(rng, n) (n, 3) plus N(0, spread^2) noise."""
    rng = np.random.default_rng(seed)
    return fn_point(rng, n) + rng.normal(0.0, spread, size=(n, 3))


def analytic_cases():
    """name -> (obstacles now, obstacles previous, mu per row, surface sampler)."""
    def floor_pts(rng, n):
        return np.stack([rng.uniform(-1, 1, n), np.full(n, -0.2), rng.uniform(-1, 1, n)], 1)

    def slide_pts(rng, n):
        nrm = row_of(OBS_SLIDE_FLOOR, (0.1, -0.3, 0.2, 0.5, 3.0 ** 0.5 / 2.0, 0.2))[4:7]
        p = rng.uniform(-1, 1, (n, 3))
        ctr = np.array([0.1, -0.3, 0.2])
        return p - ((p - ctr) @ nrm)[:, None] * nrm

    def sphere_pts(rng, n):
        d = rng.normal(size=(n, 3))
        return np.array([0.3, -1.2, 0.1]) + 0.45 * d / np.linalg.norm(d, axis=1)[:, None]

    def half_pts(rng, n):   # half on the plane outside the bump, half on the bump's sphere
        a = np.stack([rng.uniform(-2, 2, n), np.full(n, -2.6), rng.uniform(-2, 2, n)], 1)
        d = rng.normal(size=(n, 3))
        d[:, 1] = np.abs(d[:, 1])
        b = np.array([0.2, -2.6, 0.0]) + 0.8 * d / np.linalg.norm(d, axis=1)[:, None]
        return np.where((np.arange(n) % 2 == 0)[:, None], a, b)

    def cyl_pts(rng, n):
        a = rng.uniform(0, 2 * np.pi, n)
        return np.stack([-0.6 + 0.3 * np.cos(a), -1.0 + 0.3 * np.sin(a), rng.uniform(-1, 1, n)], 1)

    slide = (0.1, -0.3, 0.2) + tuple(row_of(OBS_SLIDE_FLOOR, (0, 0, 0, 0.5, 3.0 ** 0.5 / 2.0, 0.2))[4:7])
    slide_prev = (0.099, -0.3015, 0.2) + tuple(row_of(OBS_SLIDE_FLOOR, (0, 0, 0, 0.4, 0.9, 0.1))[4:7])   # the normal changed too
    return {
        "floor": ([(OBS_FLOOR, (-0.2,))], [(OBS_FLOOR, (-0.21,))], [0.5], floor_pts),
        "slide_floor": ([(OBS_SLIDE_FLOOR, slide)], [(OBS_SLIDE_FLOOR, slide_prev)], [2.0], slide_pts),
        "sphere": ([(OBS_SPHERE, (0.3, -1.2, 0.1, 0.45))], [(OBS_SPHERE, (0.299, -1.2, 0.1015, 0.5))], [0.5], sphere_pts),
        "half_sphere": ([(OBS_PLANE_HALF_SPHERE, (0.2, -2.6, 0.0, 0.8))], [(OBS_PLANE_HALF_SPHERE, (0.2, -2.601, 0.001, 0.8))], [2.0],
                        half_pts),
        "cylinder": ([(OBS_CYLINDER, (-0.6, -1.0, 0.0, 0.3))], [(OBS_CYLINDER, (-0.601, -1.0005, 0.0, 0.3))], [0.5], cyl_pts),
        "mu_zero": ([(OBS_FLOOR, (-0.2,))], [(OBS_FLOOR, (-0.21,))], [0.0], floor_pts),
    }
