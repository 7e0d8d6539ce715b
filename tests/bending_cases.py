"""Shared oracle of the bending tests (tests/test_bending.py, tests/test_gpu_bending.py).

The reference has no bending term, so the committed oracle (oracle/oracle_elastic.cpp) cannot judge
a scene with hinges. This module restates in numpy
  * the hinge model of aa_elastic_add_bending (hinges()), and
  * the (u,x) branch of oracle_elastic.cpp::step with Anderson acceleration from oracle_common.hpp
    (admm_ux_numpy()), with a dense A and np.linalg.solve in place of the envelope Cholesky, the
    triangles' reduction built as oracle_elastic.cpp's build() does and their prox taken from
    pyoracle.tri_prox, the normal-equation solve from pyoracle.cod_solve.
test_bending.py anchors the port to the committed oracle on triangles-only scenes; the GPU tests
then hold the solver to the port on scenes with hinges.
"""
import numpy as np

from golden_io import scenes


# ------------------------------------------------------------------------------------------ model
def cot(p, a, b):
    u, v = a - p, b - p
    c = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    return ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])


def tri_area(V, t):
    u, v = V[t[1]] - V[t[0]], V[t[2]] - V[t[0]]
    c = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    return 0.5 * np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])


def hinge_row(x0, x1, x2, x3):
    a0, a1 = cot(x0, x1, x2), cot(x1, x0, x2)
    b0, b1 = cot(x0, x1, x3), cot(x1, x0, x3)
    return np.array([a1 + b1, a0 + b0, -(a0 + a1), -(b0 + b1)])


def hinges(V, F, k_bend, flat_rest=True):
    """The hinges of a triangle list: (idx (h, 4) int, K (h, 4), kappa (h,), r (h,)), one per interior
    edge in increasing (x0, x1); x2 is the opposite vertex in the triangle with the lower index."""
    V = np.asarray(V, np.float64)
    edges = {}
    for ti, t in enumerate(np.asarray(F)):
        for k in range(3):
            a, b, c = int(t[k]), int(t[(k + 1) % 3]), int(t[(k + 2) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((ti, c))
    idx, K, kap, r = [], [], [], []
    for (i0, i1), lst in sorted(edges.items()):
        if len(lst) != 2:
            continue
        (ta, i2), (tb, i3) = sorted(lst)
        X = V[[i0, i1, i2, i3]]
        k = hinge_row(*X)
        idx.append((i0, i1, i2, i3))
        K.append(k)
        kap.append(3.0 * k_bend / (tri_area(V, F[ta]) + tri_area(V, F[tb])))
        z = ((k[0] * X[0] + k[1] * X[1]) + k[2] * X[2]) + k[3] * X[3]
        r.append(0.0 if flat_rest else np.sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]))
    return (np.array(idx, np.int64).reshape(-1, 4), np.array(K, np.float64).reshape(-1, 4), np.array(kap, np.float64),
            np.array(r, np.float64))


def hinge_prox(v, r):
    """argmin 1/2 kappa (|z| - r)^2 + 1/2 kappa |z - v|^2 = s v, s = 1/2 + 1/2 (r / |v|); v = 0: z = v."""
    v = np.asarray(v, np.float64)
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(n == 0.0, 1.0, 0.5 + 0.5 * (r / n))
    return s[..., None] * v


# ------------------------------------------------------------------------------------------ meshes
def two_triangles():
    """A scalene pair sharing edge (0, 1)."""
    V = np.array([[0.0, 0.0, 0.0], [1.3, 0.0, 0.0], [0.4, 0.0, 0.9], [0.7, 0.0, -0.6]])
    return V, np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def folded_pair(theta, L=1.3):
    """(rest, folded): the scalene pair flat and with its second triangle turned by theta about the edge."""
    rest = np.array([[0.0, 0.0, 0.0], [L, 0.0, 0.0], [0.4, 0.9, 0.0], [0.7, -0.6, 0.0]])
    fold = rest.copy()
    fold[3] = [0.7, -0.6 * np.cos(theta), 0.6 * np.sin(theta)]
    return rest, fold, np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def half_cylinder(nx=8, ny=3, R=0.5, width=0.6, shear=0.3):
    """scenes.tri_grid's triangles on a half-cylinder of radius R about the z axis: a curved rest
    shape. Row j is turned by `shear` columns against row 0, so no two neighbouring triangles are
    coplanar: every hinge, the diagonals' included, has r > 0."""
    _, F = scenes.tri_grid(nx, ny)
    zs = np.linspace(0.0, width, ny + 1)
    V = np.array([[-R * np.cos(p), R * np.sin(p), z]
                  for j, z in enumerate(zs) for p in np.pi * (np.arange(nx + 1) + shear * j) / (nx + shear * ny)])
    return V, F


HOST_CASES = {   # name -> (V, F, flat_rest, expected hinge count or None)
    "pair": lambda: (*two_triangles(), True, 1),
    "grid3": lambda: (*scenes.tri_grid(2, 2), True, 8),
    "grid13": lambda: (*scenes.tri_grid(12, 12), True, 408),
    "half_cylinder": lambda: (*half_cylinder(), False, None),
}


# ------------------------------------------------------------------------------------------ scenes
def _scene(V, F, pins, *, bend, flat_rest=True, membrane=True, masses=None, **kw):
    pins = np.asarray(pins, np.int32)
    g = [scenes.ElementGroup(scenes.TRI, scenes.LINEAR, 50.0, 0.1, np.asarray(F, np.int32), 0.95, 1.05)] if membrane else []
    kw.setdefault("iters", 30)
    return scenes.Scene(x=np.array(V, np.float64), masses=scenes.tri_masses(V, F, 1.0) if masses is None else masses,
                        groups=g, pin_idx=pins, pin_pts=np.array(V, np.float64)[pins].copy(), pin_vel=np.zeros((len(pins), 3)),
                        variant=scenes.VARIANT_H, bending=None if bend is None else [(np.asarray(F, np.int32), bend, flat_rest)],
                        **kw)


def pair_scene(**kw):
    """Two triangles and one hinge, no pins (in free fall, started with a fold so that the hinge works)."""
    V, F = two_triangles()
    sc = _scene(V, F, [], bend=5e-2, n_steps=3, aa_m=3, **kw)
    sc.rest = np.array(V)
    sc.x = np.array(V)
    sc.x[3, 1] += 0.2   # fold about the shared edge
    return sc


def grid3_scene(**kw):
    """3 x 3 grid with the centre node pinned: it lies inside hinges and triangles (the Cp path, a slot with pos < 0)."""
    V, F = scenes.tri_grid(2, 2)
    return _scene(V, F, [4, 0], bend=1e-2, n_steps=3, aa_m=4, **kw)


def half_cylinder_scene(flat_rest=False, gravity=-9.8, n_steps=3, **kw):
    V, F = half_cylinder()
    pins = np.arange(0, len(V), 9)   # column 0 of every row (nx = 8)
    return _scene(V, F, pins, bend=1e-2, flat_rest=flat_rest, gravity=gravity, n_steps=n_steps, **kw)


def minimiser_scene(iters=100):
    """Hinges only, 13 x 13, flat rest, k_bend 1e-2, the x = 0 edge pinned, node mass 0.1 / n, dt 1/30, no Anderson."""
    sc = scenes.cantilever_strip(12, 12, 1e-2, size=1.0, clamp=False, membrane=False, iters=iters, accel=0, n_steps=1)
    sc.masses = np.full(sc.n_nodes, 0.1 / sc.n_nodes)
    return sc


# ------------------------------------------------------------------------------------------ the port
class _Problem:
    """Rows of D (one per column of every element, x 3 coordinates), their weights and the prox."""

    def __init__(self, scene):
        import pyoracle
        self.oracle = pyoracle
        n = scene.n_nodes
        rest = np.asarray(scene.rest_x, np.float64)
        rows, w, self.tris, self.hinge_rows, self.hinge_r = [], [], [], [], []
        for g in scene.groups:
            if g.kind != scenes.TRI or g.per_element:
                raise ValueError("admm_ux_numpy: uniform triangle groups and hinges only")
            mu = g.E / (2.0 * (1.0 + g.nu))
            lam = g.E * g.nu / ((1.0 + g.nu) * (1.0 - 2.0 * g.nu))
            k = lam + (2.0 / 3.0) * mu
            for t in np.asarray(g.idx):
                # oracle_elastic.cpp build(), the triangle branch
                P = rest[t]
                e12, e13 = P[1] - P[0], P[2] - P[0]
                n1 = e12 / np.sqrt(e12[0] * e12[0] + e12[1] * e12[1] + e12[2] * e12[2])
                d = e13[0] * n1[0] + e13[1] * n1[1] + e13[2] * n1[2]
                n2 = e13 - d * n1
                n2 = n2 / np.sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2])
                dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
                b00, b01, b10, b11 = dot(n1, e12), dot(n1, e13), dot(n2, e12), dot(n2, e13)
                det = b00 * b11 - b01 * b10
                inv = 1.0 / det
                R = [[b11 * inv, -b01 * inv], [-b10 * inv, b00 * inv]]
                wt = np.sqrt(k * (0.5 * det))
                self.tris.append((len(rows), g.limit_min, g.limit_max))
                for c in range(2):
                    row = np.zeros(n)
                    row[t[0]], row[t[1]], row[t[2]] = -R[0][c] - R[1][c], R[0][c], R[1][c]
                    rows.append(row)
                    w.append(wt)
        for tris, k_bend, flat in (getattr(scene, "bending", None) or []):
            idx, K, kap, r = hinges(rest, tris, k_bend, flat)
            for e in range(len(idx)):
                row = np.zeros(n)
                row[idx[e]] = K[e]
                self.hinge_rows.append(len(rows))
                self.hinge_r.append(r[e])
                rows.append(row)
                w.append(np.sqrt(kap[e]))
        self.D = np.array(rows).reshape(-1, n)
        self.w = np.array(w)
        self.hinge_rows = np.array(self.hinge_rows, np.int64)
        self.hinge_r = np.array(self.hinge_r)

    def prox(self, vin):
        out = np.empty_like(vin)
        for r0, lmin, lmax in self.tris:
            out[r0:r0 + 2] = self.oracle.tri_prox(vin[r0:r0 + 2].reshape(6), lmin, lmax, variant=1).reshape(2, 3)
        if len(self.hinge_rows):
            out[self.hinge_rows] = hinge_prox(vin[self.hinge_rows], self.hinge_r)
        return out


class _Anderson:
    """oracle_common.hpp Anderson (init / reset / compute), arithmetic statement by statement."""

    def __init__(self, m, dim, eff, u0, cod):
        self.m, self.dim, self.eff, self.cod = m, dim, eff, cod
        self.u = u0.copy()
        self.dF, self.dG = np.zeros((m, eff)), np.zeros((m, dim))
        self.scale, self.M, self.theta = np.zeros(m), np.zeros((m, m)), np.zeros(m)
        self.iter = self.col = 0

    def reset(self, u0):
        self.u = u0.copy()
        self.iter = self.col = 0

    def compute(self, g):
        G, eff, m = g.copy(), self.eff, self.m
        F = G[:eff] - self.u[:eff]
        if self.iter == 0:
            self.dF[0], self.dG[0] = -F, -G
            self.u = G.copy()
        else:
            col = self.col
            self.dF[col] += F
            self.dG[col] += G
            eps = 1e-14
            sc = max(eps, np.sqrt(np.dot(self.dF[col], self.dF[col])))
            self.scale[col] = sc
            self.dF[col] /= sc
            mk = min(m, self.iter)
            if mk == 1:
                self.theta[0] = 0.0
                sq = np.dot(self.dF[col], self.dF[col])
                self.M[0, 0] = sq
                dn = np.sqrt(sq)
                if dn > eps:
                    self.theta[0] = np.dot(self.dF[col] / dn, F / dn)
            else:
                for c in range(mk):
                    t = np.dot(self.dF[col], self.dF[c])
                    self.M[col, c] = self.M[c, col] = t
                rhs = np.array([np.dot(self.dF[c], F) for c in range(mk)])
                self.theta[:mk] = self.cod(self.M[:mk, :mk], rhs)
            s = np.zeros(self.dim)
            for c in range(mk):
                s += self.dG[c] * (self.theta[c] / self.scale[c])
            self.u = G - s
            self.col = (col + 1) % m
            self.dF[self.col], self.dG[self.col] = -F, -G
        self.iter += 1
        return self.u.copy()


def admm_ux_numpy(scene, n_steps=None):
    """The (u,x) variant's time steps on a scene of triangle groups and hinges: per-step dicts
    (prim, comb, reject, x, v) like capi.run_scene's."""
    if scene.variant != scenes.VARIANT_H:
        raise ValueError("admm_ux_numpy: the (u,x) variant only")
    P = _Problem(scene)
    n = scene.n_nodes
    n_steps = scene.n_steps if n_steps is None else n_steps
    pins = np.asarray(scene.pin_idx, np.int64)
    is_pin = np.zeros(n, bool)
    is_pin[pins] = True
    free = np.nonzero(~is_pin)[0]
    mass = np.asarray(scene.masses, np.float64)
    dt, aa = scene.dt, scene.accel != 0
    pdt2 = scene.penalty * dt * dt
    D, w = P.D, P.w
    Df, Dp = D[:, free], D[:, pins]
    WDf = w[:, None] * Df
    A = np.diag(mass[free]) + pdt2 * (WDf.T @ WDf)
    Z3, nf = D.shape[0], len(free)
    x, v = np.array(scene.x, np.float64), np.zeros((n, 3))
    out = []
    for k in range(1, n_steps + 1):
        xpin = np.asarray(scene.pin_pts, np.float64) + k * np.asarray(scene.pin_vel, np.float64)
        Cp = Dp @ xpin if len(pins) else np.zeros((Z3, 3))   # P_pinned x_pin; c_e = -w Cp
        Px = lambda xf: Df @ xf + Cp
        prim2 = lambda xf, z: float(np.sum((w[:, None] * (Px(xf) - z)) ** 2))
        dual2 = lambda x1, x0: float(np.sum((w[:, None] * (Df @ (x1 - x0))) ** 2))
        update_z = lambda xf, u: P.prox(Px(xf) + u / w[:, None])
        if abs(scene.gravity) > 0:
            v[free, 1] += dt * scene.gravity
        xbar = x[free] + dt * v[free]
        Mxbar = mass[free, None] * xbar

        def global_solve(z, u):
            t = w[:, None] * z + (-w[:, None] * Cp) - u
            return np.linalg.solve(A, Mxbar + pdt2 * (Df.T @ (w[:, None] * t)))

        xf, u = xbar.copy(), np.zeros((Z3, 3))
        z = Px(xbar)
        prev_prim, eps = 1e20, 1e-20
        z = update_z(xf, u)
        xf = global_solve(z, u)
        u = u + (w[:, None] * Px(xf) - w[:, None] * z)
        du, dx = u.copy(), xf.copy()
        pack = lambda a, b: np.concatenate([a.ravel(), b.ravel()])
        acc = _Anderson(scene.aa_m, 3 * (Z3 + nf), 3 * Z3, pack(u, xf), P.oracle.cod_solve) if aa and scene.aa_m > 0 else None
        rec = dict(prim=[], comb=[], reject=[])
        for _ in range(scene.iters):
            z = update_z(xf, u)
            prim = np.sqrt(prim2(xf, z))
            rej = 0
            if aa and prev_prim < prim:
                u, xf = du.copy(), dx.copy()
                acc.reset(pack(u, xf))
                z = update_z(xf, u)
                prim = np.sqrt(prim2(xf, z))
                rej = 1
            last_x = xf.copy()
            prev_prim = prim
            xf = global_solve(z, u)
            comb = prim2(xf, z) + dual2(xf, last_x)
            if comb < eps:
                break
            u = u + (w[:, None] * Px(xf) - w[:, None] * z)
            if aa:
                du, dx = u.copy(), xf.copy()
                ux = acc.compute(pack(du, dx))
                u, xf = ux[:3 * Z3].reshape(Z3, 3).copy(), ux[3 * Z3:].reshape(nf, 3).copy()
            rec["prim"].append(prim)
            rec["comb"].append(comb)
            rec["reject"].append(rej)
        final = dx if aa else xf
        nx = np.empty((n, 3))
        nx[free] = final
        nx[pins] = xpin
        v = (nx - x) * (1.0 / dt)
        x = nx
        out.append(dict(prim=np.array(rec["prim"]), comb=np.array(rec["comb"]), reject=np.array(rec["reject"], np.int32),
                        x=x.copy(), v=v.copy()))
    return out


def dense_minimiser(scene):
    """The exact first-step minimiser of 1/(2 dt^2) |x - xbar|_M^2 + 1/2 sum kappa |K x|^2 on a
    hinges-only flat-rest scene: (M + dt^2 sum kappa K^T K) x = M xbar - dt^2 (w D_f)^T (w D_p x_pin).
    Returns (x* on all nodes, max |x* - xbar|)."""
    P = _Problem(scene)
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
    rhs = m[free, None] * xbar - dt * dt * (WD[:, free].T @ (WD[:, pins] @ np.asarray(scene.pin_pts, np.float64)))
    out = x.copy()
    out[free] = np.linalg.solve(A, rhs)
    return out, float(np.abs(out[free] - xbar).max())
