"""GPU tests of the deforming mesh obstacle (aa_elastic_set_mesh_obstacle_vertices): the device
refit (csrc/mesh_refit.hip) against its host restatement, the signed distance on the refitted tree
against the brute-force oracle of tests/mesh_obs_cases.py and against a freshly built tree, and the
setter in the solver, the scene runner and the C++ facade. The shapes are those of
tests/deform_cases.py, self-checked on the CPU by tests/test_deforming_obstacle.py."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import deform_cases as dc
import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import GOLDEN, scenes

pytestmark = pytest.mark.gpu

CP_TOL = 1e-13   # the project's closest-point bar (unit-size meshes)
VERTEX_SLOTS = np.r_[0:3, 3:6, 9:12]      # pn entries of corner a, b, c: sums of acos x normal
EXACT_SLOTS = np.r_[6:9, 12:15, 15:21]    # edges ab, ca, bc and the face: no acos in them


# --------------------------------------------------------------------------- 1: the tables
@pytest.mark.parametrize("name,s", dc.CASES, ids=dc.IDS)
def test_gpu_refit_tables_match_host(name, s, pkg, ctx):
    """What the kernels wrote against refit_mesh_obstacle_host: the nodes (all 128 bytes), the leaf
    triangles, the root box and the face and edge pseudonormals bit for bit; the vertex
    pseudonormals -- sums of at most 8 terms angle x unit normal whose angles come from the device's
    acos instead of the host's, a few ulp of pi apart -- to 1e-13."""
    V, F, W = dc.shape(name, s)
    host = pkg.capi.hook_mesh_refit_tables(None, V, F, W, device=0)
    dev = pkg.capi.hook_mesh_refit_tables(ctx, V, F, W, device=1)
    dv = np.abs(dev["pn"][:, VERTEX_SLOTS] - host["pn"][:, VERTEX_SLOTS]).max()
    print(f"{name} s={s}: {len(host['nodes'])} nodes, node bytes differing {(dev['nodes'] != host['nodes']).sum()}, "
          f"tris {(dev['tris'] != host['tris']).sum()}, exact pn entries {(dev['pn'][:, EXACT_SLOTS] != host['pn'][:, EXACT_SLOTS]).sum()}, "
          f"max |vertex pn diff| {dv:.3e}")
    assert np.array_equal(dev["orig"], host["orig"])
    assert dev["nodes"].shape == host["nodes"].shape and np.array_equal(dev["nodes"], host["nodes"])
    assert np.array_equal(dev["tris"].view(np.uint64), host["tris"].view(np.uint64))
    assert np.array_equal(dev["lo"], host["lo"]) and np.array_equal(dev["hi"], host["hi"])
    assert np.array_equal(dev["pn"][:, EXACT_SLOTS].view(np.uint64), host["pn"][:, EXACT_SLOTS].view(np.uint64))
    assert dv <= 1e-13
    if s is None:   # the device's tables as built are the host's, and the identity refit keeps them
        built = pkg.capi.hook_mesh_refit_tables(ctx, V, F, None, device=1)
        assert np.array_equal(built["nodes"], dev["nodes"]) and np.array_equal(built["tris"], dev["tris"])


# --------------------------------------------------------------------------- 2: against the oracle
@pytest.mark.parametrize("name,s", dc.CASES, ids=dc.IDS)
def test_gpu_deformed_sdf_matches_oracle(name, s, pkg, ctx):
    """aa_test_mesh_sdf_deformed on the 2 600 queries of the deformed shape (and on the first 1 000,
    bitwise the prefix) against Oracle(V', F, Q): the criteria of test_gpu_mesh_sdf_matches_oracle."""
    V, F, W, Q, o = dc.case(name, s)
    assert (~o.keep).sum() <= mc.MAX_EXCLUDED * len(Q)
    full = None
    for n in (len(Q), 1000):
        c, dx, tri = pkg.capi.hook_mesh_sdf_deformed(ctx, V, F, W, Q[:n])
        k = o.keep[:n]
        u = k & o.unique[:n]
        print(f"{name} s={s} n={n}: excluded {(~k).sum()}, inside mismatches {((dx < 0) != o.inside[:n])[k].sum()}, "
              f"max |c - c_ref| {np.abs(c - o.c[:n])[k].max():.3e}, max ||dx| - d| {np.abs(np.abs(dx) - o.dist[:n])[k].max():.3e}, "
              f"triangle mismatches {(tri != o.tri[:n])[u].sum()} of {u.sum()}")
        assert np.array_equal((dx < 0)[k], o.inside[:n][k])
        assert np.abs(c - o.c[:n])[k].max() <= CP_TOL
        assert np.abs(np.abs(dx) - o.dist[:n])[k].max() <= CP_TOL
        assert np.array_equal(tri[u], o.tri[:n][u])
        assert ((tri >= 0) & (tri < len(F))).all()
        if full is None:
            full = (c, dx, tri)
        else:   # a query's answer does not depend on the launch it is in
            assert np.array_equal(c, full[0][:n]) and np.array_equal(dx, full[1][:n]) and np.array_equal(tri, full[2][:n])


# --------------------------------------------------------------------------- 3: against a fresh tree
@pytest.mark.parametrize("pose", [None, "P_rot"])
@pytest.mark.parametrize("s", [0.5, 1.0])
def test_gpu_refitted_tree_answers_like_a_fresh_one(s, pose, pkg, ctx):
    """The torus refitted to V' against a mesh freshly built from V', unposed and posed: where the
    closest triangle is unique the closest point, dx and the triangle are bitwise equal (the walk is
    exact for any conservative bounds; only the order of visits differs); everywhere kept, 1e-13."""
    V, F, W, Q, o = dc.case("torus", s)
    P = None if pose is None else kc.POSES[pose]
    Qw = Q if P is None else kc.to_world(P[0], P[1], Q)
    scale = max(1.0, np.abs(Qw).max())
    a = pkg.capi.hook_mesh_sdf_deformed(ctx, V, F, W, Qw, P)
    b = pkg.capi.hook_mesh_sdf(ctx, W, F, Qw, P)
    k, u = o.keep, o.keep & o.unique
    print(f"torus s={s} pose={pose}: unique {u.sum()} of {k.sum()} kept, max |c diff| {np.abs(a[0] - b[0])[k].max():.3e}, "
          f"max |dx diff| {np.abs(a[1] - b[1])[k].max():.3e}, bitwise differing on unique: c {(a[0] != b[0])[u].any(1).sum()}, "
          f"dx {(a[1] != b[1])[u].sum()}, tri {(a[2] != b[2])[u].sum()}")
    for x, y in zip(a, b):
        assert np.array_equal(x[u], y[u])
    assert np.abs(a[0] - b[0])[k].max() <= CP_TOL * scale and np.abs(a[1] - b[1])[k].max() <= CP_TOL


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


def _run(pkg, ctx, sc, n_steps, before=(), each_step=None):
    """x after each step. `before`: calls on the solver before initialize; `each_step(s, k)`: before
    step k = 1..n_steps."""
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
    s.close()
    return xs


N_STEPS = 8
FLOOR_DROP = 0.05   # the surface lies this far below the mesh's lowest node: contact from the 3rd step
BAND = 1e-4         # a node counts as held by the surface when it ends the step below y + BAND
DY = 0.01           # the surface's rise per step


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


# --------------------------------------------------------------------------- 4: a rising top
def test_gpu_rising_top_matches_rising_floor(pkg, ctx):
    """Run A: only the top vertices of the slab mesh move up, by DY per step, through
    set_mesh_obstacle_vertices (the slab grows thicker). Run B: Floor(y) rises alike through
    set_obstacle. The slab test's rule and bar, the surface of step k at y0 + k DY; and the horse's
    lowest node ends at least 4 DY above where it ends over the fixed floor, so a setter that does
    nothing fails."""
    sc = _horse(N_STEPS)
    y0 = float(sc.x[:, 1].min() - FLOOR_DROP)
    V, F = _slab(sc, y0)
    y0 = float(V[:, 1].max())                          # the top face as stored (a rounding's worth from y0)
    top = V[:, 1] == y0
    assert top.sum() == 4
    ys = [y0 + k * DY for k in range(1, N_STEPS + 1)]

    def raise_top(s, k):
        W = V.copy()
        W[top, 1] = ys[k - 1]
        s.set_mesh_obstacle_vertices(0, W)
        assert np.array_equal(s.mesh_obstacle_vertices(0), W)

    xa = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_mesh_obstacle(V, F)], each_step=raise_top)
    xb = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_obstacle(scenes.OBS_FLOOR, [y0])],
              each_step=lambda s, k: s.set_obstacle(0, scenes.OBS_FLOOR, [ys[k - 1]]))
    xf = _run(pkg, ctx, sc, N_STEPS, before=[lambda s: s.add_obstacle(scenes.OBS_FLOOR, [y0])])
    assert _compare_runs(xa, xb, ys, np.abs(sc.x).max()) >= 2
    lift = xa[-1][:, 1].min() - xf[-1][:, 1].min()
    print(f"lowest node lifted by {lift:.4f} over the fixed floor's run")
    assert lift >= 4 * DY


# --------------------------------------------------------------------------- 5: unchanged vertices
def test_gpu_unchanged_vertices_are_bitwise_free(pkg, ctx):
    """cloth_on_torus with the setter called with the torus' own vertices before every step (the
    first call before the graph is captured, the others after): bit for bit the run without."""
    sc = scenes.cloth_on_torus(n_steps=8)
    V, F = sc.mesh_obstacles[0]
    x0 = _run(pkg, ctx, sc, 8)
    x1 = _run(pkg, ctx, sc, 8, each_step=lambda s, k: s.set_mesh_obstacle_vertices(0, V))
    o = mc.Oracle(V, F, x0[-1])
    assert (o.dist < 0.02).any()                       # the cloth lies on the torus by then
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 6: the demo scene
def test_gpu_breathing_torus_scene(pkg, ctx):
    """Two runs of the breathing-torus demo are bitwise equal; after the last step no node lies
    deeper than 0.05 inside the torus at its final shape; and the cloth's rim ends higher than over
    the torus frozen at its smallest radius, the one it is added with (the same scene without the
    vertex list)."""
    sc = scenes.cloth_on_breathing_torus(n_steps=10)
    runs = []
    for _ in range(2):
        out, s = pkg.capi.run_scene(ctx, sc)
        Vl = s.mesh_obstacle_vertices(0)
        s.close()
        runs.append([h["x"].copy() for h in out])
    for p, q in zip(*runs):
        assert np.array_equal(p, q)
    Vn, F = sc.mesh_obstacle_vertices[-1][0], sc.mesh_obstacles[0][1]
    assert np.array_equal(Vl, Vn)
    frozen, s = pkg.capi.run_scene(ctx, dataclasses.replace(sc, mesh_obstacle_vertices=None))
    s.close()
    x, xf = runs[0][-1], frozen[-1]["x"]
    o = mc.Oracle(Vn, F, x)
    half = np.abs(sc.x[:, [0, 2]]).max()
    rim = np.abs(sc.x[:, [0, 2]]).max(1) >= half * (1 - 1e-9)
    print(f"deepest penetration {o.dist[o.inside].max() if o.inside.any() else 0.0:.3e}, {rim.sum()} rim nodes, "
          f"mean rim height {x[rim, 1].mean():.4f} (breathing) / {xf[rim, 1].mean():.4f} (frozen)")
    assert not o.inside.any() or o.dist[o.inside].max() < 0.05
    assert rim.sum() >= 40 and x[rim, 1].mean() > xf[rim, 1].mean()


# --------------------------------------------------------------------------- 7: errors
def test_gpu_refused_vertices_change_nothing(pkg, ctx):
    """An unknown id, a NaN vertex, a vertex collapsed onto its neighbour and V' = -V are AA_ERR_ARG
    naming the cause; after each, get returns the old vertices and the next step is bit for bit the
    step of a run without the refused call."""
    AAError = pkg.capi.AAError
    sc = scenes.cloth_on_torus(n_steps=8)
    V, F = sc.mesh_obstacles[0]
    W = scenes.torus_mesh(16, 8, 0.6, 0.27)[0]
    assert W.shape == V.shape
    nan = W.copy()
    nan[5, 2] = np.nan
    flat = W.copy()
    flat[F[7, 1]] = flat[F[7, 0]]
    bad = [(1, W, "unknown mesh id 1"), (0, nan, "vertex 5 has a non-finite coordinate"), (0, flat, "has zero area"),
           (0, -W, "signed volume")]

    def good(s, k):
        if k == 3:
            s.set_mesh_obstacle_vertices(0, W)

    def good_and_bad(s, k):
        good(s, k)
        have = s.mesh_obstacle_vertices(0)
        for mesh_id, X, msg in bad:
            with pytest.raises(AAError, match=msg) as e:
                s.set_mesh_obstacle_vertices(mesh_id, X)
            assert e.value.code == -1
            assert np.array_equal(s.mesh_obstacle_vertices(0), have)
        assert np.array_equal(have, V if k < 3 else W)
        lib = pkg.capi.lib()
        assert lib.aa_elastic_set_mesh_obstacle_vertices(s.h, 0, None) == -1 and b"null" in lib.aa_last_error()

    x0 = _run(pkg, ctx, sc, 8, each_step=good)
    x1 = _run(pkg, ctx, sc, 8, each_step=good_and_bad)
    xs = _run(pkg, ctx, sc, 8)
    assert not np.array_equal(x0[-1], xs[-1])          # the accepted shape matters ...
    for a, b in zip(x0, x1):                           # ... and the refused ones do not
        assert np.array_equal(a, b)
    s = pkg.capi.Solver(ctx)
    with pytest.raises(AAError, match="unknown mesh id 0"):
        s.set_mesh_obstacle_vertices(0, W)
    with pytest.raises(AAError, match="unknown mesh id 0"):
        s.mesh_obstacle_vertices(0)
    assert s.add_mesh_obstacle(V, F) == 0
    with pytest.raises(AAError, match="vertices given"):
        s.set_mesh_obstacle_vertices(0, W[:-1])
    s.set_mesh_obstacle_vertices(0, W)                 # before initialize
    assert np.array_equal(s.mesh_obstacle_vertices(0), W) and s.num_obstacles() == 1
    s.close()


# --------------------------------------------------------------------------- 8: the facade
def test_gpu_facade_raises_a_box_top(tmp_path):
    """admm::Solver::set_obstacle_vertices (tests/cpp/facade_deform.cpp run): a cloth dropped on a box
    of five tets whose top vertices rise by 0.02 per step ends on the raised top face."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe = str(tmp_path / "facade_deform")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_deform.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    os.makedirs(tmp_path / "result")
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    top, ymin = (float(v) for v in r.stdout.split()[-2:])
    print(f"final top face {top}, lowest node {ymin}")
    assert top == pytest.approx(12 * 0.02, abs=1e-12)
    assert -1e-2 <= ymin - top <= 0.05, (top, ymin)
