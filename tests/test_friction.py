"""CPU tests of obstacle friction: the numpy restatement of the pass (tests/friction_cases.py)
checked against itself and against the existing restatement of the collision prox, the scene
builders, and the C ABI's argument checks that need no device."""
import os
import subprocess

import numpy as np

import friction_cases as fc
import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes


def _contacts(seed=3, n=400, mu=0.5):
    """Queries straddling a floor at y = 0 with the floor's contact points: everything
    friction_steps needs."""
    rng = np.random.default_rng(seed)
    Q = np.stack([rng.uniform(-1, 1, n), rng.normal(0.0, 0.05, n), rng.uniform(-1, 1, n)], 1)
    s = fc.queries_near(Q, seed + 1, [mu])
    q = fc.candidate(s.x_new, s.u, s.w)
    hit, row, c = fc.contact_rule([(fc.OBS_FLOOR, (0.0,))], [], q)
    g = fc.obstacle_displacement(np.array([fc.row_of(fc.OBS_FLOOR, (0.0,))]), np.array([fc.row_of(fc.OBS_FLOOR, (-0.001,))]),
                                 None, None, None, row, c)
    return s, q, hit, row, c, g


def test_mu_zero_is_the_identity():
    s, q, hit, row, c, g = _contacts()
    r = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 0.0)
    assert hit.sum() > 100 and (~hit).sum() > 100
    assert np.array_equal(r.x, s.x_new) and not r.s.any()
    assert (r.j[hit] >= 0).all() and (r.j[hit] > 0).any() and (r.j[hit] == 0).any()   # u points both ways
    assert np.array_equal(g[hit], np.tile([0.0, 0.001, 0.0], (hit.sum(), 1)))


def test_full_stick_removes_the_tangential_slip():
    """s = 1: what is left of (x' - x_old) - g has no tangential part, up to rounding."""
    s, q, hit, row, c, g = _contacts()
    r = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 1e6)
    stick = r.s == 1.0
    assert stick.sum() > 50 and np.array_equal(stick, hit & (r.j > 0))
    rel = (r.x - s.x_old) - g
    rt = rel - (rel * r.n).sum(1)[:, None] * r.n
    size = np.abs(s.x_new - s.x_old).max()
    assert np.abs(rt[stick]).max() <= 8 * np.finfo(float).eps * size
    assert np.abs(((s.x_new - s.x_old) - g)[stick] - rel[stick]).max() > 1e-4     # there was slip to remove
    assert np.array_equal(r.x[~stick], s.x_new[~stick])


def test_stick_slip_switch_is_at_mu_j_equal_lt():
    s, q, hit, row, c, g = _contacts()
    r0 = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 1.0)
    act = hit & (r0.j > 0) & (r0.lt > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu_eq = np.where(act, r0.lt / r0.j, 0.0)
    below = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 0.999 * mu_eq)
    above = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 1.001 * mu_eq)
    assert act.sum() > 50
    assert (below.s[act] < 1.0).all() and (below.s[act] > 0.99).all()
    assert (above.s[act] == 1.0).all()
    # kinetic: the node loses mu j of slip
    lost = np.linalg.norm(below.x - s.x_new, axis=1)
    assert np.allclose(lost[act], 0.999 * mu_eq[act] * r0.j[act], rtol=1e-12, atol=0)
    # with the fixed coefficients of the hook cases both regimes occur
    both = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 0.5)
    assert ((both.s > 0) & (both.s < 1)).sum() > 10 and (both.s == 1).sum() > 10


def test_pinned_lanes_are_reported_not_filtered():
    s, q, hit, row, c, g = _contacts()
    pinned = np.arange(len(q)) % 2 == 0
    r = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 0.5, pinned)
    free = fc.friction_steps(q, c, hit, s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, 0.5)
    assert not r.s[pinned].any() and np.array_equal(r.x[pinned], s.x_new[pinned])
    assert np.array_equal(r.j, free.j) and np.array_equal(r.rt, free.rt) and np.array_equal(r.s[~pinned], free.s[~pinned])


def test_contact_rule_agrees_with_the_prox_rule():
    """On the obstacle types the existing restatement covers, contact_rule's point is
    collision_prox_rule's, and its row is the last obstacle that took the payload."""
    Vt, Ft = mc.torus()
    rng = np.random.default_rng(11)
    Q = rng.uniform((-0.65, -0.3, -0.65), (0.65, 0.4, 0.65), size=(600, 3))
    ot = mc.Oracle(Vt, Ft, Q)
    floor, sphere, mesh = (mc.OBS_FLOOR, [0.05]), (mc.OBS_SPHERE, [0.3, 0.0, 0.0, 0.25]), (mc.OBS_MESH, [0])
    for obs in ([floor, mesh], [mesh, floor], [mesh, sphere, mesh], [sphere]):
        hit, row, c = fc.contact_rule(obs, [ot], Q)
        want = mc.collision_prox_rule(obs, [ot], Q)
        assert np.array_equal(hit, (want != Q).any(1))
        assert np.abs(np.where(hit[:, None], c, Q) - want).max() <= 1e-15
        assert set(np.unique(row[hit])) <= set(range(len(obs)))
    hit, row, c = fc.contact_rule([floor, mesh], [ot], Q)
    assert (row[hit & ot.inside] == 1).all() and (row[hit & ~ot.inside] == 0).all()   # a mesh hit replaces unconditionally
    ex = np.arange(len(Q)) % 3 == 0
    hit_e, row_e, _ = fc.contact_rule([floor, mesh], [ot], Q, exempt=[ex])
    assert (row_e[hit_e & ex] == 0).all() and np.array_equal(row_e[~ex], row[~ex])


def test_obstacle_displacement():
    rng = np.random.default_rng(5)
    c = rng.uniform(-1, 1, (50, 3))
    rows = np.array([fc.row_of(fc.OBS_SPHERE, (0.3, -1.2, 0.1, 0.45)), fc.row_of(fc.OBS_MESH, (0,)), fc.row_of(fc.OBS_FLOOR, (0.5,))])
    prev = np.array([fc.row_of(fc.OBS_SPHERE, (0.2, -1.0, 0.1, 0.9)), fc.row_of(fc.OBS_MESH, (0,)), fc.row_of(fc.OBS_FLOOR, (0.25,))])
    row = np.arange(50) % 3
    R1, R0 = kc.rotation((0, 1, 0), 0.3), kc.rotation((0, 1, 0), 0.25)
    t1, t0 = np.array([0.1, 0.0, 0.0]), np.zeros(3)
    g = fc.obstacle_displacement(rows, prev, [(R1, t1)], [(R0, t0)], [False], row, c)
    assert np.array_equal(g[row == 0], np.tile(rows[0, 1:4] - prev[0, 1:4], ((row == 0).sum(), 1)))   # the radius does not count
    assert np.array_equal(g[row == 2], np.tile([0.0, 0.25, 0.0], ((row == 2).sum(), 1)))
    cm = c[row == 1]
    want = cm - ((cm - t1) @ R1 @ R0.T + t0)      # c - (R0 R1^T (c - t1) + t0)
    assert np.abs(g[row == 1] - want).max() <= 1e-15
    assert not fc.obstacle_displacement(rows, prev, [(R1, t1)], [(R0, t0)], [True], row, c)[row == 1].any()
    # no pose counts as the identity, and previous = now leaves only rounding
    g0 = fc.obstacle_displacement(rows, rows, [None], [None], [False], row, c)
    assert not g0.any()
    g1 = fc.obstacle_displacement(rows, rows, [(R1, t1)], [(R1, t1)], [False], row, c)
    assert np.abs(g1).max() <= 1e-15


def test_scene_builders():
    sc = scenes.block_on_incline(20.0, 0.2)
    th = np.deg2rad(20.0)
    nrm = np.array([np.sin(th), np.cos(th), 0.0])
    bottom = sc.collision_idx
    assert len(bottom) == 25 and sc.n_nodes == 75 and sc.n_elements() == 160
    assert np.abs(sc.x[bottom] @ nrm).max() <= 1e-15 and (np.delete(sc.x, bottom, 0) @ nrm > 0.1).all()
    assert sc.obstacles[0][0] == fc.OBS_SLIDE_FLOOR and sc.obstacle_friction == [0.2] and sc.record_contacts
    assert scenes.block_on_incline(20.0).obstacle_friction is None
    assert scenes.block_on_incline(0.0).obstacles == [(fc.OBS_FLOOR, (0.0,))]
    mv = scenes.block_on_moving_floor(1.0, n_steps=5)
    assert [m[0][0] for m in mv.obstacle_motion] == [0.01 * k for k in range(1, 6)] and mv.obstacle_friction == [1.0]
    tt = scenes.block_on_turntable(1.0, n_steps=4)
    V, F = tt.mesh_obstacles[0]
    assert mc.signed_volume(V, F) > 0 and V[:, 1].max() == 0.0 and tt.obstacles == [] and tt.mesh_obstacle_poses.shape == (4, 1, 12)
    # today's scenes are unchanged by default
    a, b = scenes.cloth_on_spinning_torus(n_steps=3), scenes.cloth_on_spinning_torus(n_steps=3, friction=0.5)
    assert a.obstacle_friction is None and not a.record_contacts and a.obstacle_motion is None
    assert b.obstacle_friction == [0.5] and np.array_equal(a.x, b.x) and np.array_equal(a.mesh_obstacle_poses, b.mesh_obstacle_poses)
    assert scenes.cloth(4, 4).obstacle_friction is None


def test_exports_and_null_arguments(pkg):
    """The new entry points exist, and a null handle or context is AA_ERR_ARG without a device."""
    import ctypes as C
    lib = pkg.capi.lib()
    for name in ("aa_elastic_set_obstacle_friction", "aa_elastic_get_obstacle_friction", "aa_elastic_record_contacts",
                 "aa_elastic_get_contacts", "aa_test_contact_friction"):
        assert name in pkg.capi.EXPORTS and hasattr(lib, name)
    mu, n = C.c_double(), C.c_int()
    assert lib.aa_elastic_set_obstacle_friction(None, 0, C.c_double(0.5)) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_get_obstacle_friction(None, 0, C.byref(mu)) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_record_contacts(None, 1) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_get_contacts(None, 0, C.byref(n), None, None, None, None, None, None, None) == -1
    assert b"null" in lib.aa_last_error()
    args = [None] * 32
    args[4] = args[9] = args[15] = 0
    args[23], args[24] = C.c_double(1.0), C.c_double(0.01)
    assert lib.aa_test_contact_friction(*args) == -1 and b"null context" in lib.aa_last_error()


def test_facade_friction_builds(tmp_path):
    lib = os.path.join(REPO, "aa-admm_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_friction.cpp"), "-o", str(tmp_path / "facade_friction"),
                    "-L" + lib, "-laa_admm", "-Wl,-rpath," + lib], check=True)
