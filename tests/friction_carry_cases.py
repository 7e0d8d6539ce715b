"""The numpy restatement of a carrying mesh's displacement (include/aa_admm.h, step 5 of
aa_elastic_set_obstacle_friction as extended by aa_elastic_set_mesh_obstacle_carry;
csrc/device_prox.hpp tri_barycentric and mesh_carry_displacement) and the cases of its tests:
tests/test_friction_carry.py on the CPU, tests/test_gpu_friction_carry.py on the GPU.

As in tests/friction_cases.py every function states the device's arithmetic operation by operation
-- numpy's elementwise fp64 operations are correctly rounded and never contracted, every sum is
parenthesised as the device writes it -- so the results are meant to agree with the device's bit for
bit.
"""
import numpy as np

import friction_cases as fc
import kinematic_cases as kc
import mesh_obs_cases as mc

CP_TOL = 1e-13   # the project's closest-point bar, times max(1, max|q|)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def barycentric(A, B, C, cl):
    """(b (n, 3), den (n,)) of the points cl on the triangles (A, B, C), all (n, 3): Cramer's rule on
    the edge Gram matrix; b = (1, 0, 0) where !(den > 0)."""
    e1, e2, d = B - A, C - A, cl - A
    d11, d12, d22, p1, p2 = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2), dot3(d, e1), dot3(d, e2)
    den = d11 * d22 - d12 * d12
    with np.errstate(invalid="ignore", divide="ignore"):
        b1 = (d22 * p1 - d12 * p2) / den
        b2 = (d11 * p2 - d12 * p1) / den
        b0 = (1.0 - b1) - b2
    ok = den > 0.0
    b = np.where(ok[:, None], np.stack([b0, b1, b2], 1), np.array([1.0, 0.0, 0.0]))
    return b, den


def interpolate(b, A, B, C):
    return (b[:, [0]] * A + b[:, [1]] * B) + b[:, [2]] * C


def carry_displacement(c, cl, b, tri_now, tri_prev, pose_prev):
    """g at the world contact points c (cl the same in the obstacle frame now) from the corners now
    and in the previous vertices, tri_now / tri_prev = (A, B, C) each (n, 3), the weights b and the
    previous pose (R, t) or None."""
    (A, B, C), (Am, Bm, Cm) = tri_now, tri_prev
    gl = interpolate(b, A - Am, B - Bm, C - Cm)
    pl = cl - gl
    Rp, tp = pose_prev if pose_prev is not None else kc.IDENTITY
    return c - kc.to_world(np.asarray(Rp, float), np.asarray(tp, float), pl)


def mesh_carry_g(V, V_prev, F, tri, c, pose, pose_prev, b=None):
    """The whole of step 5 for contacts on one carrying mesh: (g, b, den). V / V_prev (nv, 3) the
    vertices now and previous, F the caller's triangles, tri (n,) the caller's triangle of each
    contact, c (n, 3) the world points; b given = the device's weights are used as they are."""
    R, t = pose if pose is not None else kc.IDENTITY
    cl = kc.to_local(np.asarray(R, float), np.asarray(t, float), c)
    f = np.asarray(F)[tri]
    now = tuple(np.asarray(V, float)[f[:, k]] for k in range(3))
    prev = tuple(np.asarray(V_prev, float)[f[:, k]] for k in range(3))
    b_own, den = barycentric(*now, cl)
    if b is None:
        b = b_own
    return carry_displacement(c, cl, b, now, prev, pose_prev), b_own, den


def obstacle_displacement(rows, rows_prev, meshes, verts_prev, carry, poses, poses_prev, still, row, c, tri):
    """friction_cases.obstacle_displacement with the carry rule: a mesh with carry[m] set takes
    mesh_carry_g (and is never still), every other row the plain rule. Returns (g, b), b = the
    weights of every mesh-row contact (0 elsewhere)."""
    g = fc.obstacle_displacement(rows, rows_prev, poses, poses_prev, still, row, c)
    b = np.zeros_like(c)
    for k in np.unique(row[row >= 0]):
        if int(rows[k][0]) != fc.OBS_MESH:
            continue
        m = int(rows[k][1])
        sel = row == k
        V, F = meshes[m]
        Vp = V if verts_prev[m] is None else verts_prev[m]
        gm, bm, _ = mesh_carry_g(V, Vp, F, tri[sel], c[sel], None if poses is None else poses[m],
                                 None if poses_prev is None else poses_prev[m])
        b[sel] = bm
        if carry[m]:
            g[sel] = gm
    return g, b


# ----------------------------------------------------------------------------- samples
def surface_samples(V, F, seed=3, per_tri=4):
    """Points on every triangle of (V, F) with the weights that made them: per triangle `per_tri`
    strictly inside the face, one on each edge and the three vertices. Returns (tri (n,), w (n, 3),
    cl (n, 3)), cl = (w0 A + w1 B) + w2 C."""
    rng = np.random.default_rng(seed)
    nf = len(F)
    ws = []
    inside = rng.dirichlet((1.0, 1.0, 1.0), size=(nf, per_tri))
    ws.append(inside)
    t = rng.uniform(0.1, 0.9, size=(nf, 3))
    edges = np.zeros((nf, 3, 3))
    for e, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        edges[:, e, i] = 1.0 - t[:, e]
        edges[:, e, j] = t[:, e]
    ws.append(edges)
    ws.append(np.broadcast_to(np.eye(3), (nf, 3, 3)))
    w = np.concatenate(ws, axis=1)
    tri = np.repeat(np.arange(nf), w.shape[1])
    w = w.reshape(-1, 3)
    A, B, C = (V[F[tri, k]] for k in range(3))
    return tri, w, interpolate(w, A, B, C)


def shared_edges(F):
    """(t0, t1, p, q): every undirected edge (p, q) with its two incident triangles."""
    seen, out = {}, []
    for t, f in enumerate(F):
        for k in range(3):
            p, q = int(f[k]), int(f[(k + 1) % 3])
            key = (min(p, q), max(p, q))
            if key in seen:
                out.append((seen[key], t, key[0], key[1]))
            else:
                seen[key] = t
    return out


RIGID = (kc.rotation((0.3, 1.0, -0.2), 0.04), np.array([0.003, -0.002, 0.005]))   # a small rigid motion
