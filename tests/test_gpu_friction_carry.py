"""GPU tests of carrying mesh obstacles (include/aa_admm.h, aa_elastic_set_mesh_obstacle_carry).

The carry form of the pass's device function is pinned through its hook
(aa_test_contact_friction_carry) to the numpy restatement of tests/friction_carry_cases.py: the
contact query against the brute-force mesh oracle, triangle included, everything after it bit for
bit. The model is pinned by what it is for: a block on a surface that moves through its vertices
(a conveyor, a twisting slab) or that is another body (a sliding block) is carried as one on a posed
surface is, and a solver in which no mesh carries computes what it always did.
"""
import dataclasses
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import deform_cases as dc
import friction_carry_cases as cc
import friction_cases as fc
import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

pytestmark = pytest.mark.gpu

CP_TOL = cc.CP_TOL
GOLDEN = os.path.join(REPO, "tests", "golden", "friction_carry", "parent_moving_floor.npz")


# ----------------------------------------------------------------------------- the hook
def _check_carry(pkg, ctx, name, obstacles, obstacles_prev, mu, meshes, verts_prev, carry, Qc, seed, poses=None, poses_prev=None,
                 still=None):
    """(a) the device's contact flag, row, point and triangle against the restated walk on the
    brute-force oracle; (b) given the device's (row, c, tri), b, g and every later field and x' bit
    for bit. Returns the device's result, the restatement and the queries."""
    s = fc.queries_near(Qc, seed, mu)
    got = pkg.capi.hook_contact_friction_carry(ctx, obstacles, obstacles_prev, mu, meshes, s.x_old, s.x_new, s.u, s.w, s.m,
                                               fc.PENALTY, fc.DT, verts_prev, carry, poses=poses, poses_prev=poses_prev,
                                               mesh_still=still)
    q = fc.candidate(s.x_new, s.u, s.w)
    n = len(q)
    oracles, raw, keep = [], [], np.ones(n, bool)
    for k, (V, F) in enumerate(meshes):
        R, t = poses[k] if poses is not None and poses[k] is not None else kc.IDENTITY
        o = mc.Oracle(V, F, kc.to_local(np.asarray(R, float), np.asarray(t, float), q))
        raw.append(o)
        oracles.append(kc.local_oracle(V, F, np.asarray(R, float), np.asarray(t, float), q))
        keep &= o.keep
    hit, row, c = fc.contact_rule(obstacles, oracles, q, None)
    tol = CP_TOL * max(1.0, np.abs(q).max())
    both = keep & hit
    rows = np.array([fc.row_of(k, p) for k, p in obstacles])
    rows_prev = np.array([fc.row_of(k, p) for k, p in obstacles_prev])
    on_mesh = got["hit"] & (rows[np.maximum(got["row"], 0), 0] == fc.OBS_MESH)
    tri_checked = tri_bad = 0
    for k in np.unique(row[both]):
        if int(rows[k][0]) != fc.OBS_MESH:
            continue
        o = raw[int(rows[k][1])]
        sel = both & (row == k) & (got["row"] == k) & o.unique
        tri_checked += sel.sum()
        tri_bad += (got["tri"][sel] != o.tri[sel]).sum()
    print(f"{name}: {n} queries, {hit.sum()} in contact ({on_mesh.sum()} on a mesh), kept {keep.sum()}, flag mismatches "
          f"{(got['hit'] != hit)[keep].sum()}, row mismatches {(got['row'] != row)[both].sum()}, triangle mismatches {tri_bad} of "
          f"{tri_checked} unique, max |c - c_ref| {np.abs(got['point'] - c)[both].max() if both.any() else 0.0:.3e}")
    assert (~keep).sum() <= max(3, mc.MAX_EXCLUDED * n)
    assert hit.sum() >= 20 and (~hit).sum() >= 20
    assert np.array_equal(got["hit"][keep], hit[keep])
    assert np.array_equal(got["row"][both], row[both]) and (got["row"][~got["hit"]] == -1).all()
    assert np.abs(got["point"] - c)[both].max() <= tol
    assert tri_checked >= 20 and tri_bad == 0
    assert (got["tri"][~on_mesh] == -1).all() and not got["bary"][~on_mesh].any()
    for k, (V, F) in enumerate(meshes):
        at = on_mesh & (rows[np.maximum(got["row"], 0), 1] == k)
        assert ((got["tri"][at] >= 0) & (got["tri"][at] < len(F))).all()
    # (b)
    g, b = cc.obstacle_displacement(rows, rows_prev, meshes, verts_prev, carry, poses, poses_prev, still, got["row"], got["point"],
                                    got["tri"])
    mu_r = np.where(got["hit"], np.asarray(mu, float)[np.maximum(got["row"], 0)], 0.0)
    r = fc.friction_steps(q, got["point"], got["hit"], s.u, s.x_old, s.x_new, g, s.w, s.m, fc.PENALTY, fc.DT, mu_r, None)
    stick, slip = (r.s == 1.0).sum(), ((r.s > 0) & (r.s < 1)).sum()
    print(f"{name}: stick {stick}, slip {slip}, max |g| {np.abs(g).max():.3e}, b in [{got['bary'][on_mesh].min():.3f}, "
          f"{got['bary'][on_mesh].max():.3f}]")
    assert np.array_equal(r.hit, got["hit"])
    assert np.array_equal(got["bary"], np.where(r.hit[:, None], b, 0.0)), f"{name}: b differs, max {np.abs(got['bary'] - b).max():.3e}"
    for key, want in (("normal", r.n), ("push", r.j), ("slip", r.rt), ("scale", r.s), ("x", r.x)):
        assert np.array_equal(got[key], want), f"{name}: {key} differs, max {np.abs(got[key] - want).max():.3e}"
    assert np.array_equal(got["x"][r.s == 0.0], s.x_new[r.s == 0.0])
    assert stick + slip >= 5
    return got, r, s, g


def _prev_vertices(V, kind):
    if kind == "identical":
        return V.copy()
    if kind == "translated":
        return V - np.array([0.003, -0.001, 0.002])
    return dc.deform(V, 0.5)


@pytest.mark.parametrize("kind", ["identical", "translated", "deformed"])
@pytest.mark.parametrize("posed", [False, True])
@pytest.mark.parametrize("name", list(mc.MESHES))
def test_gpu_hook_meshes(name, posed, kind, pkg, ctx):
    """The cube, L-prism, sliver and 16 x 8 torus, unposed and posed with a different previous pose,
    the previous vertices identical, translated, or the twist-bend-stretch at strength 0.5."""
    V, F = dc.base(name)
    Q = mc.queries(V, F)[::9][:fc.N_Q]
    if posed:
        R, t = kc.POSES["P_rot"]
        pose, pose_prev = (R, t), (kc.rotation((1.0, 2.0, 3.0), 0.7 - 0.03), t - np.array([0.002, 0.0, -0.003]))
        Qc = Q @ R.T + t
    else:
        pose, pose_prev = None, (kc.rotation((0, 1, 0), -0.03), np.array([0.0, 0.002, 0.0]))
        Qc = Q
    obs = [(fc.OBS_MESH, (0,))]
    label = f"{name}{'_posed' if posed else ''}_{kind}"
    Vp = _prev_vertices(V, kind)
    got, r, s, g = _check_carry(pkg, ctx, label, obs, obs, [0.8], [(V, F)], [Vp], [True], Qc, 41, poses=[pose], poses_prev=[pose_prev])
    plain = pkg.capi.hook_contact_friction(ctx, obs, obs, [0.8], [(V, F)], s.x_old, s.x_new, s.u, s.w, s.m, fc.PENALTY, fc.DT,
                                           poses=[pose], poses_prev=[pose_prev])
    for key in ("hit", "row", "point", "normal", "push"):          # the walk and the normal force do not depend on carry
        assert np.array_equal(got[key], plain[key]), key
    if kind == "identical":   # unchanged vertices: the plain pass's bits throughout
        for key in ("slip", "scale", "x"):
            assert np.array_equal(got[key], plain[key]), key
    else:
        assert not np.array_equal(got["slip"], plain["slip"])


def test_gpu_hook_list_one_carries(pkg, ctx):
    """floor -> mesh -> sphere -> mesh, the torus carrying (translated previous vertices), the cube
    not (a different previous pose): each row's own rule, and features for both meshes."""
    Vt, Ft = mc.torus()
    Vc, Fc = mc.box((-0.2, -0.1, -0.2), (0.2, 0.3, 0.2))
    Qc = np.random.default_rng(11).uniform((-0.65, -0.3, -0.65), (0.65, 0.4, 0.65), size=(fc.N_Q, 3))
    obs = [(fc.OBS_FLOOR, (-0.1,)), (fc.OBS_MESH, (0,)), (fc.OBS_SPHERE, (0.3, 0.0, 0.0, 0.25)), (fc.OBS_MESH, (1,))]
    prev = [(fc.OBS_FLOOR, (-0.105,)), (fc.OBS_MESH, (0,)), (fc.OBS_SPHERE, (0.29, 0.0, 0.005, 0.25)), (fc.OBS_MESH, (1,))]
    poses_prev = [None, (np.eye(3), np.array([0.004, 0.0, 0.0]))]
    Vt_prev = _prev_vertices(Vt, "translated")
    args = (obs, prev, [0.5, 2.0, 0.5, 2.0], [(Vt, Ft), (Vc, Fc)])
    got, r, s, g = _check_carry(pkg, ctx, "list", *args, [Vt_prev, None], [True, False], Qc, 32, poses=[None, None], poses_prev=poses_prev)
    assert set(np.unique(got["row"][got["hit"]])) == {0, 1, 2, 3}
    on_torus, on_cube = got["hit"] & (got["row"] == 1), got["hit"] & (got["row"] == 3)
    assert (got["tri"][on_torus] >= 0).all() and (got["tri"][on_cube] >= 0).all() and (got["tri"][got["hit"] & (got["row"] % 2 == 0)] == -1).all()
    assert np.abs(g[on_torus] - [0.003, -0.001, 0.002]).max() <= 1e-15                # the torus' own translation
    assert np.abs(g[on_cube] - [-0.004, 0.0, 0.0]).max() <= 1e-15                     # the cube's pose
    # the cube marked still: its g is 0; the torus, carrying, is never still
    got2, _, _, g2 = _check_carry(pkg, ctx, "list_still", *args, [Vt_prev, None], [True, False], Qc, 32, poses=[None, None],
                                  poses_prev=poses_prev, still=[True, True])
    assert not g2[on_cube].any() and np.array_equal(g2[on_torus], g[on_torus]) and np.array_equal(got2["tri"], got["tri"])


# ----------------------------------------------------------------------------- the solver
class Run:
    """A scene run step by step through the binding as capi.run_scene does, keeping x[k], v[k]
    (x[0] the start), contacts[k - 1] and features[k - 1] of step k."""

    def __init__(self, pkg, ctx, sc, n_steps=None, each_step=None, scripted_nodes=None, lib_check=True):
        s = pkg.capi.solver_from_scene(ctx, sc)
        s.initialize(pkg.capi.settings_from_scene(sc))
        if sc.initial_velocity is not None:
            s.set_v(sc.initial_velocity)
        self.sc, self.x, self.v, self.contacts, self.features = sc, [np.array(sc.x, float)], [], [], []
        for k in range(1, (n_steps or sc.n_steps) + 1):
            if sc.obstacle_motion:
                for row, prm in enumerate(sc.obstacle_motion[min(k, len(sc.obstacle_motion)) - 1]):
                    s.set_obstacle(row, sc.obstacles[row][0], prm)
            if sc.mesh_obstacle_poses is not None:
                p = sc.mesh_obstacle_poses[min(k, len(sc.mesh_obstacle_poses)) - 1]
                for m in range(p.shape[0]):
                    s.set_mesh_obstacle_pose(m, p[m, :9].reshape(3, 3), p[m, 9:])
            if sc.mesh_obstacle_vertices:
                for m, V in enumerate(sc.mesh_obstacle_vertices[min(k, len(sc.mesh_obstacle_vertices)) - 1]):
                    s.set_mesh_obstacle_vertices(m, V)
            if scripted_nodes is not None:       # the binding's oracle: the vertex setter with the start state
                s.set_mesh_obstacle_vertices(0, self.x[-1][scripted_nodes])
            if each_step:
                each_step(s, k)
            s.step()
            x, v, c, f = s.x, s.v, s.contacts(), s.contact_features()
            assert np.array_equal(v, (x - self.x[-1]) * (1.0 / sc.dt))
            assert len(f["tri"]) in (0, len(c["node"]))
            self.x.append(x); self.v.append(v); self.contacts.append(c); self.features.append(f)
        self.carry = [s.mesh_obstacle_carry(m) for m in range(len(sc.mesh_obstacles))]
        s.close()
        self.m = np.asarray(sc.masses, float)

    def com(self, arr, nodes=None):
        nodes = np.arange(len(self.m)) if nodes is None else nodes
        return (self.m[nodes, None] * arr[nodes]).sum(0) / self.m[nodes].sum()

    def same_as(self, other):
        return (all(np.array_equal(a, b) for a, b in zip(self.x + self.v, other.x + other.v)) and
                all(np.array_equal(a[k], b[k]) for a, b in zip(self.contacts, other.contacts) for k in a))


def _carry_g(run, k, c, f, F, V_now, V_prev):
    """g of step k's contacts restated from the device's features and the vertices the test supplied."""
    g, _, _ = cc.mesh_carry_g(V_now, V_prev, F, f["tri"], c["point"], None, None, b=f["bary"])
    return g


def _p3_shared(run, g_of_step):
    """The P3 assertions of test_gpu_friction.py: the sticking records' tangential residual, their
    number, and every loaded node sticking over the last ten steps."""
    size = np.ptp(run.x[0], axis=0).max()
    worst, n = 0.0, 0
    for k, (c, f) in enumerate(zip(run.contacts, run.features)):
        st = c["scale"] == 1.0
        if not st.any():
            continue
        d = (run.x[k + 1] - run.x[k])[c["node"][st]] - g_of_step(k + 1, c, f)[st]
        worst = max(worst, np.abs(d - (d * c["normal"][st]).sum(1)[:, None] * c["normal"][st]).max())
        n += st.sum()
    print(f"{run.sc.name}: {n} sticking records, max |(x' - x_old - g)_t| {worst:.3e} (bar {1e-12 * size:.1e}), "
          f"{len(run.contacts[-1]['node'])} final contacts")
    assert n > 10 * len(run.contacts[-1]["node"]) and worst <= 1e-12 * size
    assert all((c["scale"][c["push"] > 0] == 1.0).all() for c in run.contacts[-10:])
    return size


def _slab_g(sc):
    F = sc.mesh_obstacles[0][1]
    shapes = [sc.mesh_obstacles[0][0]] + [v[0] for v in sc.mesh_obstacle_vertices]   # shapes[k]: the vertices of step k

    def g_of(k, c, f):   # the first step: previous = now
        return cc.mesh_carry_g(shapes[k], shapes[k - 1] if k > 1 else shapes[k], F, f["tri"], c["point"], None, None, b=f["bary"])[0]
    return g_of


def test_gpu_conveyor_carries_the_block(pkg, ctx):
    """The slab translated through the vertex setter, carry on: the block is carried at the slab's
    speed; carry off: today's behaviour, the block is braked where it is."""
    shift = 0.01
    sc = scenes.block_on_conveyor_mesh(1.0, shift, n_steps=40, iters=150)
    run = Run(pkg, ctx, sc)
    _p3_shared(run, _slab_g(sc))
    per_step = (run.com(run.x[-1]) - run.com(run.x[-11]))[0] / 10.0
    assert run.carry == [True] and all(len(f["tri"]) == len(c["node"]) for f, c in zip(run.features, run.contacts))
    assert all(np.isin(f["tri"], (6, 7)).all() for f in run.features)                 # the slab's top face (quad 3: y = 0)
    off = Run(pkg, ctx, scenes.block_on_conveyor_mesh(1.0, shift, n_steps=40, iters=150, carry=False))
    per_step_off = (off.com(off.x[-1]) - off.com(off.x[-11]))[0] / 10.0
    print(f"conveyor: centre of mass moves {per_step:.6f} per step over the last ten with carry (slab {shift}), {per_step_off:.3e} without")
    assert abs(per_step / shift - 1.0) <= 0.02
    assert abs(per_step_off) < 0.05 * shift
    assert off.carry == [False] and all(len(f["tri"]) == 0 for f in off.features)     # the plain pass: no features


def test_gpu_twisting_slab_turns_the_block(pkg, ctx):
    """The slab's vertices rotated about y through the vertex setter, carry on: the block turns with
    it as it does on the pose-driven turntable."""
    dth = 0.01
    sc = scenes.block_on_twisting_slab(1.0, dth, n_steps=40, iters=150)
    run = Run(pkg, ctx, sc)
    size = _p3_shared(run, _slab_g(sc))

    def angle(r, x):   # test_gpu_p3_carried_by_a_turning_slab's construction
        r0, r1 = r.x[0][:, [0, 2]], x[:, [0, 2]]
        far = np.linalg.norm(r0, axis=1) > 0.2 * size
        a = np.arctan2(r0[far, 0] * r1[far, 1] - r0[far, 1] * r1[far, 0], (r0[far] * r1[far]).sum(1))
        return (r.m[far] * a).sum() / r.m[far].sum()
    per_step = (angle(run, run.x[-1]) - angle(run, run.x[-11])) / 10.0
    posed = Run(pkg, ctx, scenes.block_on_turntable(1.0, dtheta=dth, n_steps=40, iters=150))
    per_step_posed = (angle(posed, posed.x[-1]) - angle(posed, posed.x[-11])) / 10.0
    print(f"twisting slab: the block turns {per_step:.8f} per step over the last ten (slab {-dth}); the pose-driven turntable "
          f"{per_step_posed:.8f}; difference {per_step - per_step_posed:.3e}")
    assert abs(per_step / -dth - 1.0) <= 0.02


@pytest.fixture(scope="module")
def sliding(pkg, ctx):
    sc = scenes.block_on_sliding_block(1.0, 0.6, n_steps=40, iters=150)
    return sc, Run(pkg, ctx, sc)


def _block_steps(run, sc):
    lower = np.asarray(sc.mesh_obstacle_exempt[0])
    upper = np.setdiff1d(np.arange(sc.n_nodes), lower)
    d_lo = (run.com(run.x[-1], lower) - run.com(run.x[-11], lower))[0] / 10.0
    d_up = (run.com(run.x[-1], upper) - run.com(run.x[-11], upper))[0] / 10.0
    return d_lo, d_up


def test_gpu_sliding_block_carries_the_upper_block(sliding, pkg, ctx):
    """Body on body: the upper block rides on the sliding lower one with carry, and is braked against
    the world without."""
    sc, run = sliding
    d_lo, d_up = _block_steps(run, sc)
    off = Run(pkg, ctx, dataclasses.replace(sc, mesh_obstacle_carry=[False]))
    o_lo, o_up = _block_steps(off, sc)
    print(f"sliding block: per step over the last ten, lower {d_lo:.6f}, upper {d_up:.6f} (ratio {d_up / d_lo:.5f}) with carry; "
          f"lower {o_lo:.6f}, upper {o_up:.3e} without")
    assert d_lo > 0.005
    assert abs(d_up / d_lo - 1.0) <= 0.02
    assert abs(o_up) < 0.05 * abs(o_lo)
    upper_terms = np.setdiff1d(sc.collision_idx, sc.mesh_obstacle_exempt[0])
    last = run.contacts[-1]
    assert np.isin(upper_terms, last["node"]).any() and (last["obstacle"][np.isin(last["node"], upper_terms)] == 1).all()


def test_gpu_sliding_block_bound_is_the_scripted_run(sliding, pkg, ctx):
    """The bound run is bitwise the run that calls the vertex setter with x[nodes] before every step
    (the binding's established oracle), carry on in both."""
    sc, run = sliding
    nodes = sc.mesh_obstacle_bindings[0]
    scripted = Run(pkg, ctx, dataclasses.replace(sc, mesh_obstacle_bindings=None), scripted_nodes=nodes)
    assert scripted.carry == [True]
    for k in range(sc.n_steps + 1):
        assert np.array_equal(run.x[k], scripted.x[k]), f"x differs after step {k}"
    for k in range(sc.n_steps):
        assert all(np.array_equal(run.contacts[k][key], scripted.contacts[k][key]) for key in run.contacts[k])
        assert all(np.array_equal(run.features[k][key], scripted.features[k][key]) for key in ("tri", "bary"))
    assert any((c["scale"] > 0).any() for c in run.contacts)


def test_gpu_neutral_on_a_never_deformed_mesh(pkg, ctx):
    """block_on_turntable with carry switched on for its never-deformed slab is bitwise the run with
    carry off: every corner difference is an exact zero."""
    sc = scenes.block_on_turntable(1.0, n_steps=40, iters=150)
    off = Run(pkg, ctx, sc)
    on = Run(pkg, ctx, dataclasses.replace(sc, mesh_obstacle_carry=[True]))
    assert on.carry == [True] and off.carry == [False]
    assert on.same_as(off) and any((c["scale"] > 0).any() for c in on.contacts)
    assert all(len(f["tri"]) == len(c["node"]) for f, c in zip(on.features, on.contacts)) and len(on.features[-1]["tri"]) > 0


def test_gpu_carry_switched_on_late(pkg, ctx):
    """Carry switched on after a captured, contact-free first step gives the run that had it from
    the start. The block starts 0.012 above the conveyor, so the first two steps are free of
    contact: from the third step on both runs hold the same previous vertices (the ones of the step
    before), and no displacement was read before that."""
    sc = scenes.block_on_conveyor_mesh(1.0, 0.01, n_steps=40, iters=150)
    sc.x = sc.x + np.array([0.0, 0.012, 0.0])
    before = Run(pkg, ctx, sc)
    late = Run(pkg, ctx, dataclasses.replace(sc, mesh_obstacle_carry=None),
               each_step=lambda s, k: s.set_mesh_obstacle_carry(0, True) if k == 2 else None)
    assert len(before.contacts[0]["node"]) == 0 and len(before.contacts[1]["node"]) == 0
    assert any((c["scale"] > 0).any() for c in before.contacts) and before.carry == late.carry == [True]
    assert len(late.features[0]["tri"]) == 0                                        # the first step ran the plain pass
    assert before.same_as(late)
    never = Run(pkg, ctx, dataclasses.replace(sc, mesh_obstacle_carry=None))
    assert not np.array_equal(never.x[-1], before.x[-1])                              # the switch does something


def _digest(arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_gpu_no_carry_is_the_parent(pkg, ctx):
    """A solver that never switches carry on gives bitwise the x, v and contacts the parent commit
    gave on block_on_moving_floor (tests/golden/friction_carry/parent_moving_floor.npz, recorded by
    tests/golden/make_golden_friction_carry.py from the parent's library on an MI355X: the last step
    in full, every step by digest)."""
    run = Run(pkg, ctx, scenes.block_on_moving_floor(1.0, shift=0.01, n_steps=40, iters=150))
    want = np.load(GOLDEN)
    keys = ("node", "obstacle", "point", "normal", "push", "slip", "scale")
    assert np.array_equal(run.x[-1], want["x"]) and np.array_equal(run.v[-1], want["v"])
    for key in keys:
        assert np.array_equal(run.contacts[-1][key], want[key]), key
    assert _digest(run.x[1:]) == str(want["x_digest"]) and _digest(run.v) == str(want["v_digest"])
    assert _digest([c[key] for c in run.contacts for key in keys]) == str(want["contacts_digest"])
    assert all(len(f["tri"]) == 0 for f in run.features)


def test_gpu_errors(pkg, ctx):
    AAError = pkg.capi.AAError
    sc = scenes.block_on_turntable(1.0, n_steps=1)
    s = pkg.capi.solver_from_scene(ctx, sc)
    lib = pkg.capi.lib()
    for when in ("before", "after"):
        for mesh in (-1, 1):
            with pytest.raises(AAError, match="unknown mesh id") as e:
                s.set_mesh_obstacle_carry(mesh, True)
            assert e.value.code == -1
            with pytest.raises(AAError, match="unknown mesh id"):
                s.mesh_obstacle_carry(mesh)
        assert lib.aa_elastic_get_mesh_obstacle_carry(s.h, 0, None) == -1 and b"null on" in lib.aa_last_error()
        assert lib.aa_elastic_get_contact_features(s.h, 0, None, None, None) == -1 and b"null n" in lib.aa_last_error()
        assert not s.mesh_obstacle_carry(0) and len(s.contact_features()["tri"]) == 0
        if when == "before":
            s.initialize(pkg.capi.settings_from_scene(sc))
            for _ in range(3):
                s.step()
    assert len(s.contacts()["node"]) > 0 and len(s.contact_features()["tri"]) == 0      # a plain pass: n = 0
    s.set_mesh_obstacle_carry(0, True)
    s.step()
    assert s.mesh_obstacle_carry(0) and len(s.contact_features()["tri"]) == len(s.contacts()["node"]) > 0
    s.set_mesh_obstacle_carry(0, False)
    s.step()
    assert not s.mesh_obstacle_carry(0) and len(s.contact_features()["tri"]) == 0
    s.close()
    # a solver partitioned over more than one rank: refused after initialize, as the friction setter is
    comm = pkg.capi.Comm.solo(0, 2)
    plain = dataclasses.replace(sc, obstacle_friction=None, record_contacts=False)
    s = pkg.capi.solver_from_scene(ctx, plain, comm)
    s.initialize(pkg.capi.settings_from_scene(plain))
    with pytest.raises(AAError, match="partitioned over 2 ranks") as e:
        s.set_mesh_obstacle_carry(0, True)
    assert e.value.code == -1 and not s.mesh_obstacle_carry(0)
    s.set_mesh_obstacle_carry(0, False)                                             # switching off: fine
    s.close()
    comm.close()


def test_gpu_facade_carry_matches_binding(tmp_path, pkg, ctx):
    """tests/cpp/facade_carry.cpp drives the conveyor through the C++ facade: the binding's bits."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe, scene, out = str(tmp_path / "facade_carry"), str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_carry.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    sc = scenes.block_on_conveyor_mesh(1.0, 0.01, n_steps=12)
    g = sc.groups[0]
    V, F = sc.mesh_obstacles[0]
    with open(scene, "wb") as f:
        f.write(struct.pack("8i", sc.n_nodes, len(g.idx), len(sc.collision_idx), sc.n_steps, sc.iters, sc.aa_m, len(V), len(F)))
        f.write(struct.pack("5d", 0.01, 1.0, sc.dt, g.E, g.nu))
        for a in (sc.x, sc.rest_x, sc.masses):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(np.ascontiguousarray(g.idx, np.int32).tobytes())
        f.write(np.ascontiguousarray(sc.collision_idx, np.int32).tobytes())
        f.write(np.ascontiguousarray(V, np.float64).tobytes())
        f.write(np.ascontiguousarray(F, np.int32).tobytes())
    r = subprocess.run([exe, scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n_c, n_stick = struct.unpack("2i", raw[:8])
    x = np.frombuffer(raw[8:], np.float64).reshape(-1, 3)
    want = Run(pkg, ctx, sc)
    assert np.array_equal(x, want.x[-1])
    assert n_c == len(want.contacts[-1]["node"]) > 0 and n_stick == (want.contacts[-1]["scale"] == 1.0).sum() > 0
