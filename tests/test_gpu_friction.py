"""GPU tests of obstacle friction (include/aa_admm.h, aa_elastic_set_obstacle_friction).

The device function is pinned through its hook (aa_test_contact_friction) to the numpy restatement
of tests/friction_cases.py: the contact query against the restated obstacle walk and the brute-force
mesh oracle, the arithmetic after it bit for bit. The model is pinned by physics with a closed form
on a small stiff tet block: the weight it rests with, the acceleration it slides at, the speed it
is carried at.
"""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

import friction_cases as fc
import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

pytestmark = pytest.mark.gpu

CP_TOL = 1e-13   # the project's closest-point bar, times max(1, max|q|)


# ----------------------------------------------------------------------------- the hook
def _check_hook(pkg, ctx, name, obstacles, obstacles_prev, mu, meshes, Qc, seed, poses=None, poses_prev=None, still=None,
                q_nodes=None, exempt=None, pinned=None):
    """(a) the device's contact flag, row and point against the restated walk on the candidate;
    (b) given the device's (row, c), every later field and x' bit for bit. Returns the device's
    result and the restatement."""
    s = fc.queries_near(Qc, seed, mu)
    got = pkg.capi.hook_contact_friction(ctx, obstacles, obstacles_prev, mu, meshes, s.x_old, s.x_new, s.u, s.w, s.m,
                                         fc.PENALTY, fc.DT, q_nodes=q_nodes, pinned=pinned, exempt=exempt, poses=poses,
                                         poses_prev=poses_prev, mesh_still=still)
    q = fc.candidate(s.x_new, s.u, s.w)
    n = len(q)
    oracles, keep = [], np.ones(n, bool)
    for k, (V, F) in enumerate(meshes):
        R, t = poses[k] if poses is not None and poses[k] is not None else kc.IDENTITY
        oracles.append(kc.local_oracle(V, F, np.asarray(R, float), np.asarray(t, float), q))
        keep &= oracles[-1].keep
    masks = None
    if exempt is not None:
        masks = [None if e is None else np.isin(q_nodes, e) for e in exempt]
    hit, row, c = fc.contact_rule(obstacles, oracles, q, masks)
    tol = CP_TOL * max(1.0, np.abs(q).max())
    both = keep & hit
    print(f"{name}: {n} queries, {hit.sum()} in contact, kept {keep.sum()}, flag mismatches {(got['hit'] != hit)[keep].sum()}, "
          f"row mismatches {(got['row'] != row)[both].sum()}, max |c - c_ref| {np.abs(got['point'] - c)[both].max() if both.any() else 0.0:.3e}")
    assert (~keep).sum() <= max(3, mc.MAX_EXCLUDED * n)
    assert hit.sum() >= 20 and (~hit).sum() >= 20                                   # the queries straddle the surface
    assert np.array_equal(got["hit"][keep], hit[keep])
    assert np.array_equal(got["row"][both], row[both]) and (got["row"][~got["hit"]] == -1).all()
    assert np.abs(got["point"] - c)[both].max() <= tol
    # (b)
    rows = np.array([fc.row_of(k, p) for k, p in obstacles])
    rows_prev = np.array([fc.row_of(k, p) for k, p in obstacles_prev])
    g = fc.obstacle_displacement(rows, rows_prev, poses, poses_prev, still, got["row"], got["point"])
    mu_r = np.where(got["hit"], np.asarray(mu, float)[np.maximum(got["row"], 0)], 0.0)
    r = fc.friction_steps(q, got["point"], got["hit"], s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, mu_r, pinned)
    stick, slip = (r.s == 1.0).sum(), ((r.s > 0) & (r.s < 1)).sum()
    print(f"{name}: stick {stick}, slip {slip}, u.n < 0 on {(r.j > 0).sum()} of {r.hit.sum()} contacts, max |g| {np.abs(g).max():.3e}")
    assert np.array_equal(r.hit, got["hit"])
    for key, want in (("normal", r.n), ("push", r.j), ("slip", r.rt), ("scale", r.s), ("x", r.x)):
        assert np.array_equal(got[key], want), f"{name}: {key} differs, max {np.abs(got[key] - want).max():.3e}"
    assert np.array_equal(got["x"][r.s == 0.0], s.x_new[r.s == 0.0])                # unfiltered lanes: x_new's bits
    assert (r.j[r.hit] > 0).any() and (r.j[r.hit] == 0).any()                       # the dual points inward and outward
    return got, r, s


@pytest.mark.parametrize("name", ["floor", "slide_floor", "sphere", "half_sphere", "cylinder", "mu_zero"])
def test_gpu_hook_analytic(name, pkg, ctx):
    obs, prev, mu, sampler = fc.analytic_cases()[name]
    Qc = fc.straddle(sampler, fc.N_Q, 21)
    got, r, s = _check_hook(pkg, ctx, name, obs, prev, mu, [], Qc, 22)
    if mu[0] == 0.0:
        assert not r.s.any() and np.array_equal(got["x"], s.x_new) and r.hit.sum() > 30
    else:
        assert (r.s == 1.0).sum() >= 10 and ((r.s > 0) & (r.s < 1)).sum() >= 10     # both regimes
        assert np.abs(got["x"] - s.x_new).max() > 1e-4


@pytest.fixture(scope="module")
def mixed():
    Vt, Ft = mc.torus()
    Vc, Fc = mc.box((-0.2, -0.1, -0.2), (0.2, 0.3, 0.2))
    Qc = np.random.default_rng(11).uniform((-0.65, -0.3, -0.65), (0.65, 0.4, 0.65), size=(fc.N_Q, 3))
    return (Vt, Ft), (Vc, Fc), Qc


@pytest.mark.parametrize("order", ["floor_mesh", "mesh_sphere_mesh"])
def test_gpu_hook_lists(order, mixed, pkg, ctx):
    """Mixed lists: the row reported is the one whose point the prox would take, and each row's own
    coefficient and displacement are used."""
    torus, cube, Qc = mixed
    R0 = kc.rotation((0, 1, 0), -0.04)
    if order == "floor_mesh":
        obs = [(fc.OBS_FLOOR, (0.05,)), (fc.OBS_MESH, (0,))]
        prev = [(fc.OBS_FLOOR, (0.045,)), (fc.OBS_MESH, (0,))]
        got, r, s = _check_hook(pkg, ctx, order, obs, prev, [0.5, 2.0], [torus], Qc, 31, poses=[None],
                                poses_prev=[(R0, np.array([0.0, -0.005, 0.0]))])
        assert set(np.unique(got["row"][got["hit"]])) == {0, 1}
    else:
        obs = [(fc.OBS_MESH, (0,)), (fc.OBS_SPHERE, (0.3, 0.0, 0.0, 0.25)), (fc.OBS_MESH, (1,))]
        prev = [(fc.OBS_MESH, (0,)), (fc.OBS_SPHERE, (0.29, 0.0, 0.005, 0.25)), (fc.OBS_MESH, (1,))]
        got, r, s = _check_hook(pkg, ctx, order, obs, prev, [0.5, 0.0, 2.0], [torus, cube], Qc, 32, poses=[None, None],
                                poses_prev=[(R0, np.zeros(3)), (np.eye(3), np.array([0.004, 0.0, 0.0]))])
        assert set(np.unique(got["row"][got["hit"]])) == {0, 1, 2}
        assert not r.s[got["row"] == 1].any()                                       # the sphere's coefficient is 0


@pytest.mark.parametrize("posed", [False, True])
@pytest.mark.parametrize("name", list(mc.MESHES))
def test_gpu_hook_meshes(name, posed, pkg, ctx):
    """The cube, L-prism, sliver and 16 x 8 torus, unposed and posed, the previous pose different."""
    V, F = mc.MESHES[name]()
    Q = mc.queries(V, F)[::9][:fc.N_Q]
    if posed:
        R, t = kc.POSES["P_rot"]
        pose, pose_prev = (R, t), (kc.rotation((1.0, 2.0, 3.0), 0.7 - 0.03), t - np.array([0.002, 0.0, -0.003]))
        Qc = Q @ R.T + t
    else:
        pose, pose_prev = None, (kc.rotation((0, 1, 0), -0.03), np.array([0.0, 0.002, 0.0]))
        Qc = Q
    _check_hook(pkg, ctx, f"{name}{'_posed' if posed else ''}", [(fc.OBS_MESH, (0,))], [(fc.OBS_MESH, (0,))], [0.8], [(V, F)],
                Qc, 41, poses=[pose], poses_prev=[pose_prev])


def test_gpu_hook_exempt_pinned_still(mixed, pkg, ctx):
    """An exempt node skips the mesh and lands on the floor's row; a pinned lane is reported with
    s = 0; a mesh marked still has g = 0."""
    torus, cube, Qc = mixed
    obs = [(fc.OBS_FLOOR, (-0.05,)), (fc.OBS_MESH, (0,))]
    prev = [(fc.OBS_FLOOR, (-0.055,)), (fc.OBS_MESH, (0,))]
    nodes = (np.arange(len(Qc)) % 5).astype(np.int32)
    pinned = np.arange(len(Qc)) % 3 == 0
    prev_pose = [(kc.rotation((0, 1, 0), -0.04), np.zeros(3))]
    got, r, s = _check_hook(pkg, ctx, "exempt_pinned", obs, prev, [0.5, 2.0], [torus], Qc, 51, poses=[None], poses_prev=prev_pose,
                            q_nodes=nodes, exempt=[[1, 3]], pinned=pinned)
    ex = np.isin(nodes, [1, 3])
    assert (got["row"][got["hit"] & ex] == 0).all() and (got["row"][got["hit"] & ~ex] == 1).any()
    assert not got["scale"][pinned].any() and np.array_equal(got["x"][pinned], s.x_new[pinned])
    assert (got["hit"] & pinned).sum() > 10 and got["push"][pinned].any()
    still, r2, _ = _check_hook(pkg, ctx, "still", obs, prev, [0.5, 2.0], [torus], Qc, 51, poses=[None], poses_prev=prev_pose,
                               still=[True])
    moving, r3, _ = _check_hook(pkg, ctx, "moving", obs, prev, [0.5, 2.0], [torus], Qc, 51, poses=[None], poses_prev=prev_pose)
    on_mesh = still["hit"] & (still["row"] == 1)
    assert on_mesh.sum() > 10 and not np.array_equal(still["slip"][on_mesh], moving["slip"][on_mesh])
    assert np.array_equal(still["slip"][~on_mesh], moving["slip"][~on_mesh])


# ----------------------------------------------------------------------------- the solver
G = 9.8


class Run:
    """A scene run step by step: x[k], v[k] after step k (x[0] the start), contacts[k - 1] of step
    k. The invariants of every run are asserted on the way."""

    def __init__(self, pkg, ctx, sc, n_steps=None, each_step=None, before_init=None):
        s = pkg.capi.solver_from_scene(ctx, sc)
        if before_init:
            before_init(s)
        s.initialize(pkg.capi.settings_from_scene(sc))
        self.sc, self.x, self.v, self.contacts = sc, [np.array(sc.x, float)], [], []
        coll = np.sort(np.asarray(sc.collision_idx))
        for k in range(1, (n_steps or sc.n_steps) + 1):
            if sc.obstacle_motion:
                for row, prm in enumerate(sc.obstacle_motion[min(k, len(sc.obstacle_motion)) - 1]):
                    s.set_obstacle(row, sc.obstacles[row][0], prm)
            if sc.mesh_obstacle_poses is not None:
                p = sc.mesh_obstacle_poses[min(k, len(sc.mesh_obstacle_poses)) - 1]
                for m in range(p.shape[0]):
                    s.set_mesh_obstacle_pose(m, p[m, :9].reshape(3, 3), p[m, 9:])
            if each_step:
                each_step(s, k)
            s.step()
            x, v, c = s.x, s.v, s.contacts()
            assert np.array_equal(v, (x - self.x[-1]) * (1.0 / sc.dt))                 # position and velocity stay consistent
            assert np.isin(c["node"], coll).all() and (np.diff(c["node"]) > 0).all()  # records only for collision terms, in term order
            assert ((c["scale"] >= 0) & (c["scale"] <= 1)).all() and (c["push"] >= 0).all()
            self.x.append(x); self.v.append(v); self.contacts.append(c)
        self.mu = [s.obstacle_friction(r) for r in range(s.num_obstacles())]
        s.close()
        self.m = np.asarray(sc.masses, float)

    def com(self, arr):
        return (self.m[:, None] * arr).sum(0) / self.m.sum()


# Bars: twice the deviation measured on an MI355X (DESIGN.md section 3.7 records the figures), each
# below the cap the model has to meet (5 % for the resting weight, 10 % for the sliding acceleration).
P1_MEASURED, P1_CAP = 1.788e-12, 0.05
P2_MEASURED, P2_CAP = {0.0: 2.367e-11, 0.2: 4.408e-6}, 0.10


def test_gpu_p1_resting_weight(pkg, ctx):
    """P1: the block at rest on a FLOOR, the solve run to convergence, recording on, mu = 0:
    sum m_i j_i over the contacts is M g dt^2 -- the scale and sign of step 4."""
    sc = scenes.block_on_incline(0.0, None, iters=150, n_steps=30)
    run = Run(pkg, ctx, sc)
    M = run.m.sum()
    ratio = np.array([(run.m[c["node"]] * c["push"]).sum() / (M * G * sc.dt ** 2) for c in run.contacts])
    dev = np.abs(ratio[-10:] - 1.0).max()
    print(f"P1: sum m j / (M g dt^2) over the last ten steps {ratio[-10:].min():.6f} .. {ratio[-10:].max():.6f}, deviation {dev:.3e}, "
          f"contacts {[len(c['node']) for c in run.contacts[-3:]]}, bar {2 * P1_MEASURED:.3e}")
    assert run.mu == [0.0] and all(not c["scale"].any() for c in run.contacts)
    assert all((c["obstacle"] == 0).all() and np.abs(c["normal"] - [0.0, 1.0, 0.0]).max() < 1e-12 for c in run.contacts[-10:])
    assert 2 * P1_MEASURED <= P1_CAP
    assert dev <= 2 * P1_MEASURED


def _incline_runs(pkg, ctx):
    out = {}
    for mu in (0.0, 0.2, 0.6):
        # the filter is explicit: the solve that follows has to carry a bottom node's lost slip to the
        # rest of the stiff block, which takes a converged solve (at 40 iterations the block creeps)
        out[mu] = Run(pkg, ctx, scenes.block_on_incline(20.0, mu if mu else None, n_steps=40, iters=150))
    return out


@pytest.fixture(scope="module")
def incline(pkg, ctx):
    return _incline_runs(pkg, ctx)


def _slope_along(run, downhill, first):
    v = np.array([run.com(v) @ downhill for v in run.v])
    t = run.sc.dt * np.arange(1, len(v) + 1)
    return np.polyfit(t[first:], v[first:], 1)[0]


@pytest.mark.parametrize("mu", [0.0, 0.2])
def test_gpu_p2_sliding_acceleration(mu, incline):
    """P2: the block on a SLIDE_FLOOR tilted by 20 degrees accelerates along it at
    g (sin theta - mu cos theta). The two targets differ by a factor 2.2: without the feature the
    mu = 0.2 case fails."""
    th = np.deg2rad(20.0)
    downhill = np.array([np.cos(th), -np.sin(th), 0.0])
    want = G * (np.sin(th) - mu * np.cos(th))
    a = _slope_along(incline[mu], downhill, 15)
    dev = abs(a / want - 1.0)
    print(f"P2 mu = {mu}: acceleration along the incline {a:.5f}, closed form {want:.5f}, deviation {dev:.3e}, bar {2 * P2_MEASURED[mu]:.3e}")
    assert 2 * P2_MEASURED[mu] <= P2_CAP
    assert dev <= 2 * P2_MEASURED[mu]
    sliding = [c for c in incline[mu].contacts[15:]]
    if mu:
        assert sum(((c["scale"] > 0) & (c["scale"] < 1)).any() for c in sliding) >= 0.8 * len(sliding)   # kinetic friction
    else:
        assert all(not c["scale"].any() for c in sliding)


def test_gpu_p2_static_friction_holds(incline):
    """mu = 0.6 > tan 20: the block stays, and a sticking node does not move along the surface."""
    th = np.deg2rad(20.0)
    downhill = np.array([np.cos(th), -np.sin(th), 0.0])
    free, held = incline[0.0], incline[0.6]
    d_free = (free.com(free.x[-1]) - free.com(free.x[-11])) @ downhill
    d_held = (held.com(held.x[-1]) - held.com(held.x[-11])) @ downhill
    size = np.ptp(held.x[0], axis=0).max()
    worst, sticking = 0.0, 0
    for k, c in enumerate(held.contacts):
        st = c["scale"] == 1.0
        d = (held.x[k + 1] - held.x[k])[c["node"][st]]
        dt_ = d - (d * c["normal"][st]).sum(1)[:, None] * c["normal"][st]
        worst = max(worst, np.abs(dt_).max() if st.any() else 0.0)
        sticking += st.sum()
    print(f"P2 mu = 0.6: displacement along the incline over the last ten steps {d_held:.3e} (frictionless {d_free:.3e}), "
          f"{sticking} sticking records, max tangential step of one {worst:.3e} (block size {size})")
    assert abs(d_held) < 0.05 * abs(d_free)
    assert sticking > 10 * len(held.contacts[-1]["node"]) and worst <= 1e-12 * size


def _tangential_residual(run, g_of_step):
    """max |(x' - x_old - g)_t| over the s = 1 records of a run."""
    worst, n = 0.0, 0
    for k, c in enumerate(run.contacts):
        st = c["scale"] == 1.0
        if not st.any():
            continue
        d = (run.x[k + 1] - run.x[k])[c["node"][st]] - g_of_step(k + 1, c)[st]
        worst = max(worst, np.abs(d - (d * c["normal"][st]).sum(1)[:, None] * c["normal"][st]).max())
        n += st.sum()
    return worst, n


def test_gpu_p3_carried_by_a_moving_floor(pkg, ctx):
    """P3: a horizontal SLIDE_FLOOR whose centre moves 0.01 in x per step. mu = 1: after a few
    steps of slipping (the floor starts at once, mu g dt per step is what friction can give) the
    block sticks and moves with the floor; mu = 0: it stays."""
    shift = 0.01
    run = Run(pkg, ctx, scenes.block_on_moving_floor(1.0, shift=shift, n_steps=40))
    size = np.ptp(run.x[0], axis=0).max()
    g_of = lambda k, c: np.tile([shift if k > 1 else 0.0, 0.0, 0.0], (len(c["node"]), 1))   # the first step: previous = now
    worst, n = _tangential_residual(run, g_of)
    per_step = (run.com(run.x[-1]) - run.com(run.x[-11]))[0] / 10.0
    print(f"P3 floor mu = 1: {n} sticking records, max |(x' - x_old - g)_t| {worst:.3e}; centre of mass moves {per_step:.6f} per step "
          f"over the last ten (floor {shift})")
    assert n > 10 * len(run.contacts[-1]["node"]) and worst <= 1e-12 * size
    assert abs(per_step / shift - 1.0) <= 0.02
    assert all((c["scale"][c["push"] > 0] == 1.0).all() for c in run.contacts[-10:])   # every loaded node sticks
    free = Run(pkg, ctx, scenes.block_on_moving_floor(None, shift=shift, n_steps=40))
    drift = np.abs(free.com(free.x[-1]) - free.com(free.x[0]))[[0, 2]].max()
    print(f"P3 floor mu = 0: centre of mass drift in the plane {drift:.3e}")
    assert drift <= 1e-9 * size


def test_gpu_p3_carried_by_a_turning_slab(pkg, ctx):
    """The same on a slab mesh turned about y by a fixed angle per step through its pose, g restated
    from the poses in numpy: the sticking nodes have no slip relative to the slab, and the block
    turns with it."""
    dth = 0.01
    sc = scenes.block_on_turntable(1.0, dtheta=dth, n_steps=40)
    run = Run(pkg, ctx, sc)
    size = np.ptp(run.x[0], axis=0).max()
    rows = np.array([fc.row_of(fc.OBS_MESH, (0,))])

    def g_of(k, c):
        now = (scenes.rotation_y(k * dth), np.zeros(3))
        prev = (scenes.rotation_y((k - 1) * dth), np.zeros(3)) if k > 1 else now
        return fc.obstacle_displacement(rows, rows, [now], [prev], [False], c["obstacle"], c["point"])
    worst, n = _tangential_residual(run, g_of)

    def angle(x):   # the block's turn about y: its mass-weighted mean over the nodes off the axis
        r0, r1 = run.x[0][:, [0, 2]], x[:, [0, 2]]
        far = np.linalg.norm(r0, axis=1) > 0.2 * size
        a = np.arctan2(r0[far, 0] * r1[far, 1] - r0[far, 1] * r1[far, 0], (r0[far] * r1[far]).sum(1))
        return (run.m[far] * a).sum() / run.m[far].sum()
    # rotation_y turns x towards -z: the angle from +x to +z decreases by dtheta per step
    per_step = (angle(run.x[-1]) - angle(run.x[-11])) / 10.0
    print(f"P3 slab mu = 1: {n} sticking records, max |(x' - x_old - g)_t| {worst:.3e}; the block turns {per_step:.6f} per step "
          f"over the last ten (slab {-dth})")
    assert n > 10 * len(run.contacts[-1]["node"]) and worst <= 1e-12 * size
    assert abs(per_step / -dth - 1.0) <= 0.02
    free = Run(pkg, ctx, scenes.block_on_turntable(None, dtheta=dth, n_steps=40))
    print(f"P3 slab mu = 0: the block turns {angle(free.x[-1]):.3e} in all")
    assert abs(angle(free.x[-1])) <= 1e-9


def test_gpu_pinned_collision_node_is_reported_unfiltered(pkg, ctx):
    """A collision term on a pinned node: in the records, never filtered."""
    sc = scenes.block_on_moving_floor(1.0, n_steps=4)
    pin = int(sc.collision_idx[0])
    sc.pin_idx = np.array([pin], np.int32)
    sc.pin_pts = sc.x[[pin]] - np.array([[0.0, 1e-3, 0.0]])     # a little under the floor: its term is in contact
    sc.pin_vel = np.zeros((1, 3))
    run = Run(pkg, ctx, sc)
    for k, c in enumerate(run.contacts):
        at = c["node"] == pin
        assert at.sum() == 1 and c["scale"][at] == 0.0 and c["push"][at] > 0.0
        assert np.array_equal(run.x[k + 1][pin], sc.pin_pts[0])
    assert any((c["scale"][c["node"] != pin] > 0).any() for c in run.contacts)


def test_gpu_bitwise_neutrality(pkg, ctx):
    """mu = 0 on every row with recording on computes what a solver that never heard of friction
    computes; and a coefficient set after a captured, contact-free first step gives the run that
    had it from the start."""
    plain = Run(pkg, ctx, scenes.block_on_incline(20.0, None, n_steps=8, record=False))
    zero = Run(pkg, ctx, scenes.block_on_incline(20.0, 0.0, n_steps=8, record=True))
    assert all(len(c["node"]) == 0 for c in plain.contacts) and all(len(c["node"]) > 0 for c in zero.contacts[2:])
    for a, b in zip(plain.x + plain.v, zero.x + zero.v):
        assert np.array_equal(a, b)
    lifted = scenes.block_on_incline(20.0, 0.3, n_steps=10, record=False, lift=0.003)
    before = Run(pkg, ctx, lifted)
    late = dataclasses.replace(lifted, obstacle_friction=None)
    after = Run(pkg, ctx, late, each_step=lambda s, k: s.set_obstacle_friction(0, 0.3) if k == 2 else None)
    assert len(before.contacts[0]["node"]) == 0 and any((c["scale"] > 0).any() for c in before.contacts)
    assert before.mu == after.mu == [0.3]
    for a, b in zip(before.x + before.v, after.x + after.v):
        assert np.array_equal(a, b)
    slid = Run(pkg, ctx, dataclasses.replace(lifted, obstacle_friction=None, record_contacts=True))
    assert not np.array_equal(slid.x[-1], before.x[-1])                              # the coefficient does something


def test_gpu_errors(pkg, ctx):
    import ctypes as C
    AAError = pkg.capi.AAError
    sc = scenes.block_on_incline(20.0, None, n_steps=1, record=False)
    s = pkg.capi.solver_from_scene(ctx, sc)
    lib = pkg.capi.lib()
    for when in ("before", "after"):
        for idx in (-1, 1):
            with pytest.raises(AAError, match="out of range") as e:
                s.set_obstacle_friction(idx, 0.5)
            assert e.value.code == -1
            with pytest.raises(AAError, match="out of range"):
                s.obstacle_friction(idx)
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(AAError, match="finite and >= 0"):
                s.set_obstacle_friction(0, bad)
        assert lib.aa_elastic_get_obstacle_friction(s.h, 0, None) == -1 and b"null mu" in lib.aa_last_error()
        assert lib.aa_elastic_get_contacts(s.h, 0, None, None, None, None, None, None, None, None) == -1 and b"null n" in lib.aa_last_error()
        assert s.obstacle_friction(0) == 0.0 and len(s.contacts()["node"]) == 0
        if when == "before":
            s.initialize(pkg.capi.settings_from_scene(sc))
            s.step()
    s.set_obstacle_friction(0, 0.25)
    assert s.obstacle_friction(0) == 0.25
    s.close()
    # a solver partitioned over more than one rank: at whichever of set and initialize comes later
    comm = pkg.capi.Comm.solo(0, 2)
    s = pkg.capi.solver_from_scene(ctx, sc, comm)
    s.set_obstacle_friction(0, 0.5)
    with pytest.raises(AAError, match="partitioned over 2 ranks") as e:
        s.initialize(pkg.capi.settings_from_scene(sc))
    assert e.value.code == -1
    s.set_obstacle_friction(0, 0.0)
    s.record_contacts(True)
    with pytest.raises(AAError, match="partitioned over 2 ranks"):
        s.initialize(pkg.capi.settings_from_scene(sc))
    s.record_contacts(False)
    s.initialize(pkg.capi.settings_from_scene(sc))
    with pytest.raises(AAError, match="partitioned over 2 ranks"):
        s.set_obstacle_friction(0, 0.5)
    with pytest.raises(AAError, match="partitioned over 2 ranks"):
        s.record_contacts(True)
    s.set_obstacle_friction(0, 0.0)                                                 # no friction asked for: fine
    s.close()
    comm.close()


def test_gpu_facade_friction_matches_binding(tmp_path, pkg, ctx):
    """tests/cpp/facade_friction.cpp drives the incline through the C++ facade: the binding's bits."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe, scene, out = str(tmp_path / "facade_friction"), str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_friction.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    sc = scenes.block_on_incline(20.0, 0.2, n_steps=12)
    g = sc.groups[0]
    nrm = sc.obstacles[0][1][3:5]
    with open(scene, "wb") as f:
        f.write(struct.pack("6i", sc.n_nodes, len(g.idx), len(sc.collision_idx), sc.n_steps, sc.iters, sc.aa_m))
        f.write(struct.pack("6d", nrm[0], nrm[1], 0.2, sc.dt, g.E, g.nu))
        for a in (sc.x, sc.rest_x, sc.masses):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(np.ascontiguousarray(g.idx, np.int32).tobytes())
        f.write(np.ascontiguousarray(sc.collision_idx, np.int32).tobytes())
    r = subprocess.run([exe, scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n_c, n_stick = struct.unpack("2i", raw[:8])
    x = np.frombuffer(raw[8:], np.float64).reshape(-1, 3)
    want = Run(pkg, ctx, sc)
    assert np.array_equal(x, want.x[-1])
    assert n_c == len(want.contacts[-1]["node"]) > 0 and n_stick == (want.contacts[-1]["scale"] == 1.0).sum()


def test_gpu_demo_spinning_torus_drags_the_cloth(pkg, ctx):
    """cloth_on_spinning_torus(friction = 0.5): the cloth's angular momentum about the spin axis has
    the spin's sign and exceeds the frictionless run's."""
    L = {}
    for mu in (None, 0.5):
        sc = scenes.cloth_on_spinning_torus(n_steps=20, friction=mu)
        out, s = pkg.capi.run_scene(ctx, sc)
        s.close()
        x, v = out[-1]["x"], out[-1]["v"]
        L[mu] = float((np.asarray(sc.masses) * (x[:, 2] * v[:, 0] - x[:, 0] * v[:, 2])).sum())   # (r x m v)_y
    # rotation_y(theta) with growing theta turns +z towards +x: angular momentum about +y is positive
    print(f"demo: angular momentum about the spin axis, frictionless {L[None]:.6e}, friction 0.5 {L[0.5]:.6e}")
    assert L[0.5] > 0 and L[0.5] > abs(L[None])
