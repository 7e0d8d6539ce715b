"""GPU tests of the triangle-mesh passive obstacle (PassiveMesh) of the collision terms, pinned to
the brute-force fp64 oracle of tests/mesh_obs_cases.py (self-checked on the CPU by
tests/test_mesh_obstacle.py)."""
import os
import subprocess

import numpy as np
import pytest

import mesh_obs_cases as mc
from conftest import REPO
from golden_io import GOLDEN, scenes

pytestmark = pytest.mark.gpu

CP_TOL = 1e-13   # the project's closest-point bar (unit-size meshes)


@pytest.mark.parametrize("name", list(mc.MESHES))
def test_gpu_mesh_sdf_matches_oracle(name, pkg, ctx):
    """aa_test_mesh_sdf on 2 600 queries (and on the first 1 000, whose last wave is partial):
    inside flags equal on every kept query, closest points and |dx| to 1e-13, the triangle index
    equal where the oracle's minimum is unique."""
    V, F, Q, o = mc.case(name)
    k = o.keep
    assert (~k).sum() <= mc.MAX_EXCLUDED * len(Q)
    full = None
    for n in (len(Q), 1000):
        c, dx, tri = pkg.capi.hook_mesh_sdf(ctx, V, F, Q[:n])
        kn = k[:n]
        print(f"{name} n={n}: inside mismatches {((dx < 0) != o.inside[:n])[kn].sum()}, "
              f"max |c - c_ref| {np.abs(c - o.c[:n])[kn].max():.3e}, max ||dx| - d| {np.abs(np.abs(dx) - o.dist[:n])[kn].max():.3e}, "
              f"triangle mismatches {(tri != o.tri[:n])[kn & o.unique[:n]].sum()}")
        assert np.array_equal((dx < 0)[kn], o.inside[:n][kn])
        assert np.abs(c - o.c[:n])[kn].max() <= CP_TOL
        assert np.abs(np.abs(dx) - o.dist[:n])[kn].max() <= CP_TOL
        u = kn & o.unique[:n]
        assert np.array_equal(tri[u], o.tri[:n][u])
        assert ((tri >= 0) & (tri < len(F))).all()
        if full is None:
            full = (c, dx, tri)
        else:   # a query's answer does not depend on the launch it is in
            assert np.array_equal(c, full[0][:n]) and np.array_equal(dx, full[1][:n]) and np.array_equal(tri, full[2][:n])


def _mixed_case():
    """Torus and cube over a floor and a sphere: queries inside both, one only or neither."""
    Vt, Ft = mc.torus()
    Vc, Fc = mc.box((-0.2, -0.1, -0.2), (0.2, 0.3, 0.2))
    rng = np.random.default_rng(11)
    Q = rng.uniform((-0.65, -0.3, -0.65), (0.65, 0.4, 0.65), size=(3000, 3))
    return (Vt, Ft), (Vc, Fc), Q, mc.Oracle(Vt, Ft, Q), mc.Oracle(Vc, Fc, Q)


@pytest.fixture(scope="module")
def mixed():
    return _mixed_case()


@pytest.mark.parametrize("order", ["floor_mesh", "mesh_floor", "mesh_sphere_mesh"])
def test_gpu_collision_prox_ordering(order, mixed, pkg, ctx):
    """aa_test_collision_prox on mixed obstacle lists against the numpy restatement of the
    ordering rule: a mesh's inside hit replaces the running payload unconditionally, obstacles
    after it compete with their own `dx > best` test."""
    torus, cube, Q, ot, oc = mixed
    floor = (mc.OBS_FLOOR, [0.05])
    sphere = (mc.OBS_SPHERE, [0.3, 0.0, 0.0, 0.25])
    if order == "floor_mesh":
        obs, meshes, oracles = [floor, (mc.OBS_MESH, [0])], [torus], [ot]
        in_a, in_b = Q[:, 1] < 0.05, ot.inside
    elif order == "mesh_floor":
        obs, meshes, oracles = [(mc.OBS_MESH, [0]), floor], [torus], [ot]
        in_a, in_b = ot.inside, Q[:, 1] < 0.05
    else:
        obs, meshes, oracles = [(mc.OBS_MESH, [0]), sphere, (mc.OBS_MESH, [1])], [torus, cube], [ot, oc]
        in_s = np.linalg.norm(Q - np.array([0.3, 0.0, 0.0]), axis=1) < 0.25
        in_a, in_b = ot.inside | oc.inside, in_s
        assert (ot.inside & in_s & ~oc.inside).any() and (oc.inside & in_s).any() and (ot.inside & oc.inside).any()
    keep = np.logical_and.reduce([o.keep for o in oracles])
    assert (~keep).sum() <= mc.MAX_EXCLUDED * len(Q)
    for regime in (in_a & in_b, in_a & ~in_b, ~in_a & in_b, ~in_a & ~in_b):   # both, one only, neither
        assert (regime & keep).sum() >= 10
    want = mc.collision_prox_rule(obs, oracles, Q)
    got = pkg.capi.hook_collision_prox(ctx, obs, meshes, Q)
    moved = (want != Q).any(1)
    print(f"{order}: moved {moved[keep].sum()} of {keep.sum()}, max |got - want| {np.abs(got - want)[keep].max():.3e}")
    assert np.array_equal((got != Q).any(1)[keep], moved[keep])
    assert np.abs(got - want)[keep].max() <= CP_TOL
    assert np.array_equal(got[keep & ~moved], Q[keep & ~moved])   # untouched candidates come back bit for bit


def _horse(n_steps, iters=13):
    d = np.load(os.path.join(GOLDEN, "mesh_horse759.npz"))
    sc = scenes.plinko_hit(d["verts"], d["tets"], n_steps=n_steps, iters=iters)
    sc.obstacles = []
    return sc


def _slab(sc, y0):
    lo, hi = sc.x.min(0), sc.x.max(0)
    ext = hi - lo
    return mc.box((lo[0] - 2 * ext[0], y0 - 4 * ext[1], lo[2] - 2 * ext[2]), (hi[0] + 2 * ext[0], y0, hi[2] + 2 * ext[2]))


def _run(pkg, ctx, sc, n_steps, before=(), after_first=()):
    """x after each step; `before` / `after_first`: obstacle adders called before initialize / after
    the first step."""
    s = pkg.capi.solver_from_scene(ctx, sc)
    for add in before:
        add(s)
    s.initialize(pkg.capi.settings_from_scene(sc))
    xs = []
    for k in range(n_steps):
        s.step()
        xs.append(s.x.copy())
        if k == 0:
            for add in after_first:
                add(s)
    s.close()
    return xs


N_STEPS = 8
FLOOR_DROP = 0.05   # the floor lies this far below the mesh's lowest node: contact from the 3rd step
BAND = 1e-4         # a node counts as held by the surface when it ends the step below y0 + BAND (the
                    # collision terms are soft: held nodes end a little under the surface)


def test_gpu_slab_mesh_matches_floor(pkg, ctx):
    """The falling horse of test_gpu_obstacles_after_initialize over Floor(y0) and over a slab mesh
    whose top face is at y0: positions agree to 1e-9 relative over the leading steps in which both
    runs end with the same nodes held by the surface (contact decisions are discrete); at least two of
    those steps have contact."""
    sc = _horse(N_STEPS)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    xf = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_obstacle(scenes.OBS_FLOOR, [y0])])
    xm = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_mesh_obstacle(V, F)])
    scale = np.abs(sc.x).max()
    same, contact = 0, 0
    for k in range(N_STEPS):
        on_f, on_m = xf[k][:, 1] <= y0 + BAND, xm[k][:, 1] <= y0 + BAND
        err = np.abs(xf[k] - xm[k]).max() / scale
        print(f"step {k + 1}: on the surface {on_f.sum()} / {on_m.sum()}, max rel diff {err:.3e}, lowest y - y0 {xm[k][:, 1].min() - y0:.3e}")
        if same == k and np.array_equal(on_f, on_m):
            assert err <= 1e-9
            same += 1
            contact += bool(on_f.any())
    print(f"{same} of {N_STEPS} steps with the same contact set, {contact} of them with contact")
    assert contact >= 2


def test_gpu_mesh_added_after_initialize_is_bitwise(pkg, ctx):
    """A mesh obstacle added after the first step -- whose graph was captured with the plain
    collision kernel, and which had no contact -- gives bit for bit the trajectory of a solver that
    had the mesh from the start."""
    sc = _horse(6)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    add = lambda s: s.add_mesh_obstacle(V, F)
    x0 = _run(pkg, ctx, sc, 6, before=[add])
    x1 = _run(pkg, ctx, sc, 6, after_first=[add])
    assert x0[0][:, 1].min() > y0 + 1e-3                     # no contact in the first step
    assert min(x[:, 1].min() for x in x0) <= y0 + BAND       # contact later
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)


def test_gpu_torus_scene_is_deterministic(pkg, ctx):
    """Two runs of the cloth-on-torus demo scene are bitwise equal, and the cloth ends up draped
    on the torus (its rim stays above the torus' mid-plane while free fall would pass it). The
    walk is always cold (no warm start from a node's last triangle), so there is no other variant
    to compare."""
    sc = scenes.cloth_on_torus(n_steps=10)
    a = _run(pkg, ctx, sc, 10)
    b = _run(pkg, ctx, sc, 10)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    V, F = sc.mesh_obstacles[0]
    o = mc.Oracle(V, F, a[-1])
    print(f"lowest node {a[-1][:, 1].min():.4f}, deepest penetration {o.dist[o.inside].max() if o.inside.any() else 0.0:.3e}")
    assert a[-1][:, 1].max() > 0.0 and a[-1][:, 1].min() < sc.x[0, 1] - 0.1
    assert not o.inside.any() or o.dist[o.inside].max() < 0.05


def test_gpu_mesh_obstacle_errors(pkg, ctx):
    V, F = mc.cube()
    sc = scenes.cloth(4, 4, variant=scenes.VARIANT_X, iters=5)
    s = pkg.capi.solver_from_scene(ctx, sc)
    s.add_mesh_obstacle(V, F)
    with pytest.raises(pkg.capi.AAError, match="No collisions with LDLT solver"):   # as the analytic obstacles
        s.initialize(pkg.capi.settings_from_scene(sc))
    s.close()
    s = pkg.capi.Solver(ctx)
    with pytest.raises(pkg.capi.AAError, match="unknown obstacle type"):
        s.add_obstacle(scenes.OBS_MESH, [0])
    with pytest.raises(pkg.capi.AAError, match="open"):
        s.add_mesh_obstacle(V, F[1:])
    for k in range(16):
        assert s.add_mesh_obstacle(V + k, F) == k
    with pytest.raises(pkg.capi.AAError, match="too many mesh obstacles"):
        s.add_mesh_obstacle(V, F)
    s.close()


def test_gpu_facade_passive_mesh_holds_a_cloth(tmp_path):
    """admm::PassiveMesh::from_tets through admm::Solver::add_obstacle (tests/cpp/facade_mesh.cpp
    run): a cloth dropped on a box of five tets stays on its top face (y = 0); free fall would
    reach y = -0.7."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe = str(tmp_path / "facade_mesh")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_mesh.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    os.makedirs(tmp_path / "result")
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    ymin = float(r.stdout.split()[-1])
    assert -1e-2 <= ymin <= 0.05, ymin
