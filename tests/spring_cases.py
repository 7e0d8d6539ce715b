"""Shared oracle of the spring tests (tests/test_springs.py, tests/test_gpu_springs.py).

The reference has no two-node spring, so the committed oracle cannot judge a scene with springs. This
module restates in numpy
  * the spring model of aa_elastic_add_springs (springs(), spring_prox()), and
  * the (u,x) loop with springs: SpringProblem extends tests/bending_cases.py's _Problem -- the
    spring rows (-1, +1) come after the hinge rows, weight sqrt(k), prox spring_prox -- and
    admm_ux() is bending_cases.admm_ux_numpy statement by statement with the problem class as a
    parameter (that function constructs _Problem by name). test_springs.py shows that
    admm_ux(scene, bc._Problem) reproduces bc.admm_ux_numpy bit for bit; the GPU tests then hold
    the solver to admm_ux(scene) on scenes with springs.
SpringProblem also keeps, over every prox evaluation of a run, the smallest distance of a one-sided
spring from its threshold, min |n - L| / max(L, n), and whether some evaluation saw active and
inactive one-sided springs together: a trajectory comparison means something only away from the
threshold.
"""
import numpy as np

import bending_cases as bc
from golden_io import scenes

SPRING, TETHER, STRUT, HARD = 0, 1, 2, 4
MODES = (SPRING, TETHER, STRUT, HARD, HARD | TETHER, HARD | STRUT)


# ------------------------------------------------------------------------------------------ model
def norm3(v):
    v = np.asarray(v, np.float64)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def spring_prox(v, L, mode):
    """z = s v. mode & 3: 0 two-sided, 1 tether (n <= L: z = v), 2 strut (n >= L: z = v); soft
    s = 1/2 + 1/2 (L / n), hard (mode & 4) s = L / n; n = 0: z = v. L scalar or per row."""
    v = np.asarray(v, np.float64)
    n = norm3(v)
    L = np.broadcast_to(np.asarray(L, np.float64), n.shape)
    side = mode & 3
    slack = (n == 0.0) | ((n <= L) if side == 1 else (n >= L) if side == 2 else np.zeros(n.shape, bool))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = L / n
        s = q if mode & 4 else 0.5 + 0.5 * q
        out = s[..., None] * v
    return np.where(slack[..., None], v, out)


def spring_energy(z, L, mode):
    """U(z) / k; inf outside a hard form's set."""
    n = norm3(z)
    side = mode & 3
    d = n - L if side == 0 else np.maximum(0.0, n - L) if side == 1 else np.maximum(0.0, L - n)
    if mode & 4:
        return np.where(np.abs(d) <= 1e-12 * np.maximum(1.0, L), 0.0, np.inf)
    return 0.5 * d * d


def springs(V, pairs, k, rest=None):
    """(idx (m, 2), G (m, 2), L (m,), w (m,)) as the host builder makes them."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    m = len(pairs)
    k = np.broadcast_to(np.asarray(k, np.float64), (m,))
    if rest is None:
        d = np.asarray(V, np.float64)[pairs[:, 1]] - np.asarray(V, np.float64)[pairs[:, 0]]
        L = norm3(d)
    else:
        L = np.broadcast_to(np.asarray(rest, np.float64), (m,)).copy()
    return pairs, np.tile(np.array([-1.0, 1.0]), (m, 1)), L, np.sqrt(k)


# ------------------------------------------------------------------------------------------ the port
class SpringProblem(bc._Problem):
    """_Problem plus the spring rows, after the hinge rows."""

    def __init__(self, scene):
        super().__init__(scene)
        n = scene.n_nodes
        rest = np.asarray(scene.rest_x, np.float64)
        rows, w, self.spring_groups = [], [], []
        r0 = self.D.shape[0]
        for pairs, k, L, mode in (getattr(scene, "springs", None) or []):
            idx, G, L, ws = springs(rest, pairs, k, L)
            self.spring_groups.append((np.arange(r0 + len(rows), r0 + len(rows) + len(idx)), L, int(mode)))
            for e in range(len(idx)):
                row = np.zeros(n)
                row[idx[e, 0]] += G[e, 0]
                row[idx[e, 1]] += G[e, 1]
                rows.append(row)
                w.append(ws[e])
        if rows:
            self.D = np.vstack([self.D, np.array(rows)]) if self.D.size else np.array(rows)
            self.w = np.concatenate([self.w, np.array(w)])
        self.margin, self.mixed, self.evaluations = np.inf, False, 0

    def prox(self, vin):
        out = super().prox(vin)
        self.evaluations += 1
        for rows, L, mode in self.spring_groups:
            v = vin[rows]
            out[rows] = spring_prox(v, L, mode)
            if mode & 3:
                nn = norm3(v)
                with np.errstate(divide="ignore", invalid="ignore"):
                    m = np.abs(nn - L) / np.maximum(L, nn)
                self.margin = min(self.margin, float(np.nanmin(m)))
                active = (nn > L) if (mode & 3) == 1 else (nn < L)
                self.mixed = self.mixed or bool(active.any() and (~active).any())
        return out


def admm_ux(scene, problem=SpringProblem, n_steps=None, keep=None):
    """bending_cases.admm_ux_numpy with the problem class as a parameter: per-step dicts (prim, comb,
    reject, x, v). keep: a dict that receives the problem object under "P"."""
    if scene.variant != scenes.VARIANT_H:
        raise ValueError("admm_ux: the (u,x) variant only")
    P = problem(scene)
    if keep is not None:
        keep["P"] = P
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
        acc = bc._Anderson(scene.aa_m, 3 * (Z3 + nf), 3 * Z3, pack(u, xf), P.oracle.cod_solve) if aa and scene.aa_m > 0 else None
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
    """The exact first-step minimiser of a scene whose terms are all quadratic in x (zero-length soft
    springs, flat-rest hinges): (M + dt^2 (w D_f)^T (w D_f)) x = M xbar - dt^2 (w D_f)^T (w D_p x_pin).
    Returns (x* on all nodes, max |x* - xbar|)."""
    P = SpringProblem(scene)
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
def _springs_only(x, pins, pairs, k, rest, mode, *, mass=0.01, pin_vel=None, **kw):
    x = np.array(x, np.float64)
    pins = np.asarray(pins, np.int32)
    kw.setdefault("iters", 30)
    return scenes.Scene(x=x, masses=np.full(len(x), float(mass)), groups=[], pin_idx=pins, pin_pts=x[pins].copy(),
                        pin_vel=np.zeros((len(pins), 3)) if pin_vel is None else np.asarray(pin_vel, np.float64),
                        variant=scenes.VARIANT_H, springs=[(np.asarray(pairs, np.int32), k, rest, mode)], **kw)


def pair_scene(**kw):
    """Two free nodes and one spring (L = 0.3), started stretched to 0.5, in free fall."""
    x = [[0.0, 0.0, 0.0], [0.4, 0.3, 0.0]]
    return _springs_only(x, [], [[0, 1]], 50.0, np.array([0.3]), SPRING, n_steps=3, aa_m=3, **kw)


def chain5(mode=SPRING, *, rest_scale=1.0, pin_vel=(0.02, 0.01, 0.0), k=50.0, n_steps=3, **kw):
    """Five nodes 0.2 apart along x, joined in a row, node 0 pinned and moving by pin_vel per step:
    the Cp path, a slot with pos < 0, the soft attachment. Under gravity the chain swings down."""
    x = [[0.2 * i, 0.0, 0.0] for i in range(5)]
    pairs = [[i, i + 1] for i in range(4)]
    rest = rest_scale * scenes.pair_lengths(np.array(x), np.array(pairs))
    return _springs_only(x, [0], pairs, k, rest, mode, pin_vel=[pin_vel], n_steps=n_steps, aa_m=4, **kw)


def net5(**kw):
    """spring_net(5, 5) with every rest length 0.9 of the initial distance: a taut net. The flat net
    at its rest lengths resists gravity at second order only, and the port itself does not define
    that trajectory to the tolerances: one-ulp noise on the initial positions moves its prim curve
    by 1.2e-7 prim_0 (comb: 2.5e-9 comb_0); on the taut net by 4.4e-11 (1.7e-12)."""
    kw.setdefault("n_steps", 2)
    kw.setdefault("rest_scale", 0.9)
    return scenes.spring_net(5, 5, **kw)


def mixed_net(mode, *, seed=1, lo=0.85, hi=1.2, pins=None, n_steps=2, **kw):
    """net5 with each rest length its initial distance times lo or hi, drawn per spring: from the
    first iteration some one-sided springs are active and some are slack. pins: the pinned nodes
    (default: the four corners)."""
    sc = scenes.spring_net(5, 5, mode=mode, n_steps=n_steps, **kw)
    pairs = sc.springs[0][0]
    f = np.where(np.random.default_rng(seed).random(len(pairs)) < 0.5, lo, hi)
    sc.springs = [(pairs, sc.springs[0][1], f * scenes.pair_lengths(sc.x, pairs), mode)]
    if pins is not None:
        p = np.asarray(pins, np.int32)
        sc.pin_idx, sc.pin_pts, sc.pin_vel = p, sc.x[p].copy(), np.zeros((len(p), 3))
    return sc


def long_ties_13(**kw):
    """A 13 x 13 cloth (tri_grid(12, 12), cloth()'s membrane, two diagonal corners pinned) with a soft
    spring from every node of its x = 0 edge to the node opposite on the far edge, and likewise
    between the two z edges, 0.9 of that distance long (they pull the edges together): 26 springs
    that cross the top bisection of the dissection, adjacency the mesh does not have."""
    V, F = scenes.tri_grid(12, 12)
    sc = bc._scene(V, F, [0, 168], bend=None, n_steps=2, **kw)
    pairs = [[13 * j, 13 * j + 12] for j in range(13)] + [[i, 156 + i] for i in range(13)]
    pairs = np.array(pairs, np.int32)
    sc.springs = [(pairs, 5.0, 0.9 * scenes.pair_lengths(V, pairs), SPRING)]
    sc.name = "long_ties_13"
    return sc


# One scene per one-sided / hard mode, shared by the CPU margin test and the GPU trajectories.
#   tether / strut (soft): the mixed net hanging from one corner / from two. Chosen among one, two
#   and four pinned corners by the port's own conditioning (its prim and comb curves under one-ulp
#   noise on the initial positions: 1.4e-10 / 2.6e-11 and 9.5e-11 / 3.1e-11 of prim_0 / comb_0;
#   struts between four pinned corners buckle the flat net and measure up to 6e-10 comb_0).
#   hard: the chain with rigid links dragged by its moving anchor (a pendulum started level).
#   hard | tether, hard | strut: the mixed net hanging from ONE corner -- with one pin every set of
#   hard one-sided lengths is feasible (four pinned corners and shortened tethers are not).
ONE_SIDED = {
    "net5_tether": lambda: mixed_net(TETHER, pins=[0]),
    "net5_strut": lambda: mixed_net(STRUT, pins=[0, 4]),
    "chain5_hard": lambda: chain5(HARD),
    "net5_hard_tether": lambda: mixed_net(HARD | TETHER, pins=[0]),
    "net5_hard_strut": lambda: mixed_net(HARD | STRUT, pins=[0]),
}


def tethered_cloth_free():
    """scenes.tethered_cloth() without its obstacle: the port's scene for the tether-length bound."""
    return scenes.tethered_cloth(obstacle=False)


def tether_violation(x, sc):
    """max over the hard tethers of |x_b - x_a| / L - 1."""
    pairs, _, rest, _ = sc.springs[0]
    L = scenes.pair_lengths(sc.rest_x, pairs) if rest is None else np.asarray(rest, np.float64)
    return float((scenes.pair_lengths(np.asarray(x).reshape(-1, 3), pairs) / L - 1.0).max())


def stitches_only_scene(iters=100):
    """Zero-length soft springs only (a quadratic problem): net5's structural and shear pairs with
    L = 0, corners pinned, no Anderson, one step."""
    sc = scenes.spring_net(5, 5, k=2.0, rest_scale=0.0, iters=iters, accel=0, n_steps=1)
    return sc


def hanging_mass_scene(n_steps=60):
    """One mass on a soft vertical spring from a pinned anchor, under gravity: settles at extension
    m g / k. k = 36, m = 0.01, dt = 1/30: omega dt = sqrt(k / m) dt = 2, so implicit Euler damps the
    swing by 1 / sqrt(5) per step. Started at rest length. No Anderson: on this one-dimensional
    linear problem Anderson's first extrapolation is exact, the loop leaves at comb < 1e-20 and hands
    back the last plain iterate (as the reference's loop does), which is two iterations old -- the
    accelerated run settles 1.9e-3 off, the plain one 1.3e-11."""
    x = [[0.0, 0.0, 0.0], [0.0, -0.5, 0.0]]
    return _springs_only(x, [0], [[0, 1]], 36.0, np.array([0.5]), SPRING, mass=0.01, n_steps=n_steps, accel=0, iters=40)


def hanging_mass_error(out, sc):
    """|extension - m g / k| after the last step."""
    k, m = sc.springs[0][1], sc.masses[1]
    x = np.asarray(out[-1]["x"]).reshape(-1, 3)
    return abs((x[0, 1] - x[1, 1] - 0.5) - m * abs(sc.gravity) / k)
