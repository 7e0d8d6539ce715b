"""GPU tests of the kinematic mesh obstacle (aa_elastic_set_mesh_obstacle_pose) and of the
re-parameterised analytic obstacle (aa_elastic_set_obstacle), pinned to the brute-force oracle of
tests/mesh_obs_cases.py through the restated transform of tests/kinematic_cases.py (both
self-checked on the CPU by tests/test_kinematic_obstacle.py)."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import GOLDEN, scenes

pytestmark = pytest.mark.gpu

CP_TOL = 1e-13   # the project's closest-point bar (unit-size meshes)


# --------------------------------------------------------------------------- 1: posed signed distance
@pytest.mark.parametrize("name,pose", kc.CASES)
def test_gpu_posed_sdf_matches_oracle(name, pose, pkg, ctx):
    """aa_test_mesh_sdf_posed on the 2 600 world queries (and on the first 1 000, whose last wave is
    partial, bitwise the prefix). Against O_l, the oracle in the obstacle frame at the restated q_l:
    inside flags equal on every kept query, |dx| to 1e-13, the closest point to 1e-13 max(1, max|Q_w|)
    of R c_l + t, the triangle equal where unique. Against O_w, the mesh moved to the world: flags
    equal and closest points to 1e-12 max(1, max|Q_w|) on the jointly kept queries."""
    V, F, R, t, Q_w, q_l, ol, ow = kc.case(name, pose)
    scale = max(1.0, np.abs(Q_w).max())
    c_ref = kc.to_world(R, t, ol.c)
    full = None
    for n in (len(Q_w), 1000):
        c, dx, tri = pkg.capi.hook_mesh_sdf(ctx, V, F, Q_w[:n], (R, t))
        kn = ol.keep[:n]
        both = kn & ow.keep[:n]
        print(f"{name} {pose} n={n}: inside mismatches {((dx < 0) != ol.inside[:n])[kn].sum()} (local) "
              f"{((dx < 0) != ow.inside[:n])[both].sum()} (world), max ||dx| - d| {np.abs(np.abs(dx) - ol.dist[:n])[kn].max():.3e}, "
              f"max |c - (R c_l + t)| {np.abs(c - c_ref[:n])[kn].max():.3e}, max |c - c_w| {np.abs(c - ow.c[:n])[both].max():.3e}, "
              f"triangle mismatches {(tri != ol.tri[:n])[kn & ol.unique[:n]].sum()}")
        assert np.array_equal((dx < 0)[kn], ol.inside[:n][kn])
        assert np.abs(np.abs(dx) - ol.dist[:n])[kn].max() <= CP_TOL
        assert np.abs(c - c_ref[:n])[kn].max() <= CP_TOL * scale
        u = kn & ol.unique[:n]
        assert np.array_equal(tri[u], ol.tri[:n][u])
        assert ((tri >= 0) & (tri < len(F))).all()
        assert np.array_equal((dx < 0)[both], ow.inside[:n][both])
        assert np.abs(c - ow.c[:n])[both].max() <= 1e-12 * scale
        if full is None:
            full = (c, dx, tri)
        else:   # a query's answer does not depend on the launch it is in
            assert np.array_equal(c, full[0][:n]) and np.array_equal(dx, full[1][:n]) and np.array_equal(tri, full[2][:n])


# --------------------------------------------------------------------------- the falling horse
def _horse(n_steps, iters=13):
    d = np.load(os.path.join(GOLDEN, "mesh_horse759.npz"))
    sc = scenes.plinko_hit(d["verts"], d["tets"], n_steps=n_steps, iters=iters)
    sc.obstacles = []
    return sc


def _slab(sc, y0):
    lo, hi = sc.x.min(0), sc.x.max(0)
    ext = hi - lo
    return mc.box((lo[0] - 2 * ext[0], y0 - 4 * ext[1], lo[2] - 2 * ext[2]), (hi[0] + 2 * ext[0], y0, hi[2] + 2 * ext[2]))


def _run(pkg, ctx, sc, n_steps, before=(), each_step=None, after_first=()):
    """x after each step. `before`: calls on the solver before initialize; `each_step(s, k)`: before
    step k = 1..n_steps; `after_first`: after the first step."""
    s = pkg.capi.solver_from_scene(ctx, sc)
    for f in before:
        f(s)
    s.initialize(pkg.capi.settings_from_scene(sc))
    xs = []
    for k in range(1, n_steps + 1):
        if each_step is not None:
            each_step(s, k)
        s.step()
        xs.append(s.x.copy())
        if k == 1:
            for f in after_first:
                f(s)
    s.close()
    return xs


N_STEPS = 8
FLOOR_DROP = 0.05   # the surface lies this far below the mesh's lowest node: contact from the 3rd step
BAND = 1e-4         # a node counts as held by the surface when it ends the step below y + BAND


def _compare_runs(xa, xb, ys, scale):
    """The slab test's rule: over the leading steps in which both runs end with the same nodes held
    by the surface (at height ys[k] in step k), positions agree to 1e-9 relative; returns how many of
    those steps had contact."""
    same, contact = 0, 0
    for k in range(len(xa)):
        on_a, on_b = xa[k][:, 1] <= ys[k] + BAND, xb[k][:, 1] <= ys[k] + BAND
        err = np.abs(xa[k] - xb[k]).max() / scale
        print(f"step {k + 1}: on the surface {on_a.sum()} / {on_b.sum()}, max rel diff {err:.3e}, lowest y - surface {xa[k][:, 1].min() - ys[k]:.3e}")
        if same == k and np.array_equal(on_a, on_b):
            assert err <= 1e-9
            same += 1
            contact += bool(on_a.any())
    print(f"{same} of {len(xa)} steps with the same contact set, {contact} of them with contact")
    return contact


# --------------------------------------------------------------------------- 2: identity is free
@pytest.mark.parametrize("name", list(mc.MESHES))
def test_gpu_identity_pose_is_bitwise_unposed_sdf(name, pkg, ctx):
    V, F, Q, _ = mc.case(name)
    a = pkg.capi.hook_mesh_sdf(ctx, V, F, Q)
    b = pkg.capi.hook_mesh_sdf(ctx, V, F, Q, kc.IDENTITY)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_gpu_identity_pose_is_bitwise_unposed_run(pkg, ctx):
    """Six steps of the falling horse over the slab mesh: the identity pose set before initialize
    gives bit for bit the unposed trajectory (which has contact)."""
    sc = _horse(6)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    add = lambda s: s.add_mesh_obstacle(V, F)
    x0 = _run(pkg, ctx, sc, 6, before=[add])
    x1 = _run(pkg, ctx, sc, 6, before=[add, lambda s: s.set_mesh_obstacle_pose(0, *kc.IDENTITY)])
    assert min(x[:, 1].min() for x in x0) <= y0 + BAND
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 3: ordering with poses
def test_gpu_collision_prox_ordering_with_poses(pkg, ctx):
    """aa_test_collision_prox_posed on mesh -> sphere -> mesh, the first mesh (a torus given in a
    frame turned by P_rot^-1 and posed with P_rot, so that it lies where the ordering test's torus
    does) posed and the second (a box) not, against the numpy restatement of the ordering rule fed
    one oracle per mesh, each asked in its mesh's frame with the points mapped back."""
    R, t = kc.POSES["P_rot"]
    Vt, Ft = mc.torus()
    Vl = (Vt - t) @ R                                  # R^T (v - t): posed, the torus is back around the origin
    cube = mc.box((-0.2, -0.1, -0.2), (0.2, 0.3, 0.2))
    Q = np.random.default_rng(11).uniform((-0.65, -0.3, -0.65), (0.65, 0.4, 0.65), size=(3000, 3))
    ot = kc.local_oracle(Vl, Ft, R, t, Q)
    oc = mc.Oracle(cube[0], cube[1], Q)
    sphere = (mc.OBS_SPHERE, [0.3, 0.0, 0.0, 0.25])
    obs = [(mc.OBS_MESH, [0]), sphere, (mc.OBS_MESH, [1])]
    in_s = np.linalg.norm(Q - np.array([0.3, 0.0, 0.0]), axis=1) < 0.25
    in_a, in_b = ot.inside | oc.inside, in_s
    assert (ot.inside & in_s & ~oc.inside).any() and (oc.inside & in_s).any() and (ot.inside & oc.inside).any()
    keep = ot.keep & oc.keep
    assert (~keep).sum() <= mc.MAX_EXCLUDED * len(Q)
    for regime in (in_a & in_b, in_a & ~in_b, ~in_a & in_b, ~in_a & ~in_b):   # both, one only, neither
        assert (regime & keep).sum() >= 10
    want = mc.collision_prox_rule(obs, [ot, oc], Q)
    got = pkg.capi.hook_collision_prox(ctx, obs, [(Vl, Ft), cube], Q, poses=[(R, t), None])
    moved = (want != Q).any(1)
    print(f"moved {moved[keep].sum()} of {keep.sum()}, max |got - want| {np.abs(got - want)[keep].max():.3e}")
    assert np.array_equal((got != Q).any(1)[keep], moved[keep])
    assert np.abs(got - want)[keep].max() <= CP_TOL
    assert np.array_equal(got[keep & ~moved], Q[keep & ~moved])   # untouched candidates come back bit for bit


# --------------------------------------------------------------------------- 4: constant pose
def test_gpu_constant_pose_matches_pretransformed_slab(pkg, ctx):
    """The falling horse over the static slab mesh, and over the same slab given in a frame turned by
    P_rot^-1 and posed with P_rot (its top face back at y0): the slab test's rule and bar."""
    sc = _horse(N_STEPS)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    R, t = kc.POSES["P_rot"]
    Vl = (V - t) @ R
    top = kc.world_vertices(R, t, Vl)[:, 1].max()
    t = t + np.array([0.0, y0 - top, 0.0])             # the top face at y0 (a rounding's worth)
    assert abs(kc.world_vertices(R, t, Vl)[:, 1].max() - y0) <= 1e-15 * max(1.0, abs(y0))
    xs = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_mesh_obstacle(V, F)])
    xp = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_mesh_obstacle(Vl, F), lambda s: s.set_mesh_obstacle_pose(0, R, t)])
    assert _compare_runs(xs, xp, [y0] * N_STEPS, np.abs(sc.x).max()) >= 2


# --------------------------------------------------------------------------- 5: moving obstacles
DY = 0.01   # the surface's rise per step: contact by step 3 (the fixed surface's first contact), the rise
            # over 8 steps 0.08 -- far more than the depth a held node ends under the soft surface


def test_gpu_rising_slab_matches_rising_floor(pkg, ctx):
    """Run A: the slab mesh rises by DY per step through set_mesh_obstacle_pose. Run B: Floor(y)
    rises alike through set_obstacle. The slab test's rule and bar, the surface of step k at
    y0 + k DY; and the horse's lowest node ends at least 4 DY above where it ends over the fixed
    floor, so a pose that does nothing fails."""
    sc = _horse(N_STEPS)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    ys = [y0 + k * DY for k in range(1, N_STEPS + 1)]
    I = np.eye(3)
    xa = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_mesh_obstacle(V, F)],
              each_step=lambda s, k: s.set_mesh_obstacle_pose(0, I, [0.0, ys[k - 1] - y0, 0.0]))
    xb = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_obstacle(scenes.OBS_FLOOR, [y0])],
              each_step=lambda s, k: s.set_obstacle(0, scenes.OBS_FLOOR, [ys[k - 1]]))
    xf = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_obstacle(scenes.OBS_FLOOR, [y0])])
    assert _compare_runs(xa, xb, ys, np.abs(sc.x).max()) >= 2
    assert (xa[2][:, 1] <= ys[2] + BAND).any()         # contact by step 3
    lift_a, lift_b = xa[-1][:, 1].min() - xf[-1][:, 1].min(), xb[-1][:, 1].min() - xf[-1][:, 1].min()
    print(f"lowest node over the fixed floor {xf[-1][:, 1].min() - y0:.3e} (rel. y0), lifted by {lift_a:.4f} (mesh) / {lift_b:.4f} (floor)")
    assert lift_a >= 4 * DY and lift_b >= 4 * DY


# --------------------------------------------------------------------------- 6: pose after capture
def test_gpu_pose_set_after_capture_is_bitwise(pkg, ctx):
    """A pose set after the first step -- which had no contact and whose graph was captured -- gives
    bit for bit the trajectory of a solver that had the pose before initialize: the replayed graph
    reads the new row."""
    sc = _horse(6)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    R = kc.rotation((0.0, 1.0, 0.0), 0.3)              # about the slab's vertical axis, and 0.01 up
    ctr = 0.5 * (V.min(0) + V.max(0))
    t = ctr - R @ ctr + np.array([0.0, 0.01, 0.0])
    add = lambda s: s.add_mesh_obstacle(V, F)
    pose = lambda s: s.set_mesh_obstacle_pose(0, R, t)
    x0 = _run(pkg, ctx, sc, 6, before=[add, pose])
    x1 = _run(pkg, ctx, sc, 6, before=[add], after_first=[pose])
    xu = _run(pkg, ctx, sc, 6, before=[add])
    assert x0[0][:, 1].min() > y0 + 0.01 + 1e-3               # no contact in the first step
    assert min(x[:, 1].min() for x in x0) <= y0 + 0.01 + BAND  # contact later
    assert not np.array_equal(x0[-1], xu[-1])                  # and the pose matters
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 7: the demo scene
def test_gpu_spinning_torus_scene(pkg, ctx):
    """Two runs of the spinning-torus demo are bitwise equal, differ from the still torus' run, and
    after the last step no node lies deeper than 0.05 inside the torus at its final pose."""
    sc = scenes.cloth_on_spinning_torus(n_steps=10)
    runs = []
    for _ in range(2):
        out, s = pkg.capi.run_scene(ctx, sc)
        Rl, tl, posed = s.mesh_obstacle_pose(0)
        s.close()
        runs.append([h["x"].copy() for h in out])
    for p, q in zip(*runs):
        assert np.array_equal(p, q)
    Rn, tn = sc.mesh_obstacle_poses[-1, 0, :9].reshape(3, 3), sc.mesh_obstacle_poses[-1, 0, 9:]
    assert posed and np.array_equal(Rl, Rn) and np.array_equal(tl, tn)
    still, s = pkg.capi.run_scene(ctx, scenes.cloth_on_torus(n_steps=10))
    s.close()
    assert not np.array_equal(still[-1]["x"], runs[0][-1])
    V, F = sc.mesh_obstacles[0]
    x = runs[0][-1]
    o = mc.Oracle(kc.world_vertices(Rn, tn, V), F, x)
    print(f"lowest node {x[:, 1].min():.4f}, deepest penetration {o.dist[o.inside].max() if o.inside.any() else 0.0:.3e}")
    assert x[:, 1].max() > 0.0 and x[:, 1].min() < sc.x[0, 1] - 0.1
    assert not o.inside.any() or o.dist[o.inside].max() < 0.05


# --------------------------------------------------------------------------- 8: errors
def test_gpu_kinematic_obstacle_errors(pkg, ctx):
    AAError = pkg.capi.AAError
    V, F = mc.cube()
    R, t = kc.POSES["P_rot"]
    s = pkg.capi.Solver(ctx)
    assert s.num_obstacles() == 0
    with pytest.raises(AAError, match="unknown mesh id 0"):
        s.set_mesh_obstacle_pose(0, R, t)
    s.add_obstacle(scenes.OBS_FLOOR, [-1.0])
    assert s.add_mesh_obstacle(V, F) == 0
    s.add_obstacle(scenes.OBS_SPHERE, [0.0, 0.0, 0.0, 0.5])
    assert s.num_obstacles() == 3
    # poses
    Ru, tu, posed = s.mesh_obstacle_pose(0)
    assert not posed and np.array_equal(Ru, np.eye(3)) and not tu.any()
    s.set_mesh_obstacle_pose(0, R, t)
    Rg, tg, posed = s.mesh_obstacle_pose(0)
    assert posed and np.array_equal(Rg, R) and np.array_equal(tg, t)   # used as given
    for bad in (1, -1):
        with pytest.raises(AAError, match="unknown mesh id"):
            s.set_mesh_obstacle_pose(bad, R, t)
        with pytest.raises(AAError, match="unknown mesh id"):
            s.mesh_obstacle_pose(bad)
    with pytest.raises(AAError, match="reflection"):
        s.set_mesh_obstacle_pose(0, R @ np.diag([1.0, 1.0, -1.0]), t)
    with pytest.raises(AAError, match="not orthonormal"):
        s.set_mesh_obstacle_pose(0, 1.001 * R, t)
    Rn = R.copy()
    Rn[1, 2] = np.nan
    with pytest.raises(AAError, match="not finite"):
        s.set_mesh_obstacle_pose(0, Rn, t)
    with pytest.raises(AAError, match="not finite"):
        s.set_mesh_obstacle_pose(0, R, [0.0, np.inf, 0.0])
    Rg, tg, posed = s.mesh_obstacle_pose(0)
    assert posed and np.array_equal(Rg, R) and np.array_equal(tg, t)   # a refused pose changes nothing
    s.set_mesh_obstacle_pose(0, None)
    assert not s.mesh_obstacle_pose(0)[2]
    # analytic rows
    s.set_obstacle(0, scenes.OBS_FLOOR, [-0.5])
    s.set_obstacle(2, scenes.OBS_SPHERE, [0.1, 0.0, 0.0, 0.5])
    with pytest.raises(AAError, match="is a mesh"):
        s.set_obstacle(1, scenes.OBS_MESH, [0])
    with pytest.raises(AAError, match="type mismatch"):
        s.set_obstacle(0, scenes.OBS_SPHERE, [0.0, 0.0, 0.0, 1.0])
    for bad in (3, -1):
        with pytest.raises(AAError, match="out of range"):
            s.set_obstacle(bad, scenes.OBS_FLOOR, [0.0])
    with pytest.raises(AAError, match="null parameters"):
        s.set_obstacle(0, scenes.OBS_FLOOR, None)
    with pytest.raises(AAError, match="not finite"):
        s.set_obstacle(2, scenes.OBS_SPHERE, [0.0, np.nan, 0.0, 1.0])
    assert s.num_obstacles() == 3
    s.close()
    # the hooks validate alike
    with pytest.raises(AAError, match="reflection"):
        pkg.capi.hook_mesh_sdf(ctx, V, F, np.zeros((1, 3)), (np.diag([1.0, 1.0, -1.0]), np.zeros(3)))
    with pytest.raises(AAError, match="not orthonormal"):
        pkg.capi.hook_collision_prox(ctx, [(mc.OBS_MESH, [0])], [(V, F)], np.zeros((1, 3)), poses=[(1.001 * R, t)])


# --------------------------------------------------------------------------- 9: the facade
def test_gpu_facade_lifts_a_cloth(tmp_path):
    """admm::Solver::set_obstacle_pose / update_obstacle (tests/cpp/facade_kinematic.cpp run): a cloth
    dropped on a box of five tets that rises by 0.02 per step ends on the box's final top face."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe = str(tmp_path / "facade_kinematic")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_kinematic.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    os.makedirs(tmp_path / "result")
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    top, ymin = (float(v) for v in r.stdout.split()[-2:])
    print(f"final top face {top}, lowest node {ymin}")
    assert top == pytest.approx(12 * 0.02, abs=1e-12)
    assert -1e-2 <= ymin - top <= 0.05, (top, ymin)
