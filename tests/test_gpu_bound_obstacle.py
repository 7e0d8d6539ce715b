"""GPU tests of the bound mesh obstacle (aa_elastic_bind_mesh_obstacle: a mesh whose vertices follow
solver nodes, gathered, checked and refitted on the device at the top of every step) and of the
exemption (aa_elastic_set_mesh_obstacle_exempt). The oracle is the project's own existing path: the
vertex setter, its refit kernels and the collision prox without exemption."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import bound_cases as bc
import deform_cases as dc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

pytestmark = pytest.mark.gpu

VERTEX_SLOTS = np.r_[0:3, 3:6, 9:12]      # pn entries of corner a, b, c: sums of acos x normal
EXACT_SLOTS = np.r_[6:9, 12:15, 15:21]    # edges ab, ca, bc and the face: no acos in them


def _torus_above_a_chunk():
    return mc.torus(17, 8)                # 272 triangles: one full chunk of the vol6 sum and a partial one


# (name, (V, F, V')): the smallest shapes that reach each path -- a single-leaf tree, the cube, exactly
# one chunk of the vol6 sum (256), a chunk and a part (272), nine chunks and split nodes (2 304); the
# sliver (4) and the cube (12) lie below one chunk
def _shapes():
    out = [(name, dc.shape(name, 0.5)) for name in ("sliver", "cube", "torus", "torus_fine")]
    V, F = _torus_above_a_chunk()
    out.append(("torus272", (V, F, dc.deform(V, 0.5))))
    return out


SHAPES = _shapes()


def _same_tables(a, b, what):
    assert np.array_equal(a["orig"], b["orig"]), what
    assert a["nodes"].shape == b["nodes"].shape and np.array_equal(a["nodes"], b["nodes"]), what
    assert np.array_equal(bc.bits(a["tris"]), bc.bits(b["tris"])), what
    assert np.array_equal(bc.bits(a["lo"]), bc.bits(b["lo"])) and np.array_equal(bc.bits(a["hi"]), bc.bits(b["hi"])), what
    assert np.array_equal(bc.bits(a["pn"][:, EXACT_SLOTS]), bc.bits(b["pn"][:, EXACT_SLOTS])), what
    dv = np.abs(a["pn"][:, VERTEX_SLOTS] - b["pn"][:, VERTEX_SLOTS]).max()
    assert dv <= 1e-13, (what, dv)
    return dv


# --------------------------------------------------------------------------- 1: the kernels
@pytest.mark.parametrize("name,shape", SHAPES, ids=[n for n, _ in SHAPES])
def test_gpu_bound_refit_matches_existing_path(name, shape, pkg, ctx):
    """aa_test_bound_refit(device = 1) on a permuted, decoy-padded node array whose decoys hold NaN,
    against the vertex setter's device path on x[nodes] and against the host restatement."""
    V, F, W = shape
    assert {"sliver": 4, "cube": 12, "torus": 256, "torus272": 272, "torus_fine": 2304}[name] == len(F)
    X, nodes = bc.embed(W, decoy_nan=True)
    assert np.isnan(X).any() and np.array_equal(X[nodes], W)
    dev = pkg.capi.hook_bound_refit(ctx, V, F, X, nodes, device=1)
    host = pkg.capi.hook_bound_refit(None, V, F, X, nodes, device=0)
    setter = pkg.capi.hook_mesh_refit_tables(ctx, V, F, X[nodes], device=1)
    d1 = _same_tables(dev, setter, "against the setter's kernels")
    d0 = _same_tables(dev, host, "against the host")
    print(f"{name}: {len(F)} triangles, {len(dev['nodes'])} nodes, vol6 {dev['vol6']!r}, max |vertex pn diff| {d1:.3e} (setter) {d0:.3e} (host)")
    assert dev["taken"] and host["taken"] and dev["cause"] == host["cause"] == 0
    assert bc.bits(dev["vol6"]) == bc.bits(host["vol6"]) == bc.bits(bc.vol6_chunked(W, F))


# --------------------------------------------------------------------------- 2: refusals on the device
@pytest.mark.parametrize("name,shape", [SHAPES[1], SHAPES[3]], ids=["cube", "torus_fine"])
def test_gpu_bound_refit_refusals(name, shape, pkg, ctx):
    """A NaN in a bound node, a vertex collapsed onto its neighbour and x = -x: the status names the
    cause (the host's), vol6 has the host's bits, and every table is bitwise the built one. A good
    shape after the refused one refits as if nothing had happened: every output, status and vol6
    included, is bitwise that of the good shape alone."""
    V, F, W = shape
    X, nodes = bc.embed(W)
    built = pkg.capi.hook_mesh_refit_tables(ctx, V, F, None, device=1)
    good = pkg.capi.hook_bound_refit(ctx, V, F, X, nodes, device=1)
    assert good["taken"]
    nan = X.copy()
    nan[nodes[len(nodes) // 2], 1] = np.nan
    flat = X.copy()
    flat[nodes[F[len(F) - 1, 1]]] = flat[nodes[F[len(F) - 1, 0]]]
    for Y, cause in ((nan, 1), (flat, 2), (-X, 3)):
        dev = pkg.capi.hook_bound_refit(ctx, V, F, Y, nodes, device=1)
        host = pkg.capi.hook_bound_refit(None, V, F, Y, nodes, device=0)
        print(f"{name} cause {cause}: device {dev['cause']}, host {host['cause']}, vol6 {dev['vol6']!r}")
        assert not dev["taken"] and dev["cause"] == host["cause"] == cause
        if cause != 1:
            assert bc.bits(dev["vol6"]) == bc.bits(host["vol6"])
        for k in built:
            assert np.array_equal(dev[k].view(np.uint8), built[k].view(np.uint8)), (cause, k)
        after = pkg.capi.hook_bound_refit(ctx, V, F, X, nodes, device=1, X_first=Y)
        assert after["taken"] and after["cause"] == 0 and bc.bits(after["vol6"]) == bc.bits(good["vol6"])
        for k in built:
            assert np.array_equal(after[k].view(np.uint8), good[k].view(np.uint8)), (cause, k)


# --------------------------------------------------------------------------- the solver
def _run(pkg, ctx, sc, n_steps, before=(), each_step=None, after_step=None):
    """x after each step. `before`: calls on the solver before initialize; `each_step(s, k)`: before
    step k = 1..n_steps; `after_step(s, k)`: after it."""
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
        if after_step is not None:
            after_step(s, k)
    s.close()
    return xs


def _set_x(s, x):
    s.set_state(x, s.v)


# --------------------------------------------------------------------------- 3: bound = scripted
def test_gpu_bound_run_equals_scripted_run(pkg, ctx):
    """Run A: cloth_on_soft_block over 8 steps, bound. Run B: the same scene unbound with
    set_mesh_obstacle_vertices(0, x[nodes]) before every step. Bit for bit after every step. The
    controls: the mesh frozen at its added shape differs from A by the last step, and by then a cloth
    node is within 0.02 of the block's surface."""
    sc = scenes.cloth_on_soft_block()
    nodes = sc.mesh_obstacle_bindings[0]
    V, F = sc.mesh_obstacles[0]
    unbound = dataclasses.replace(sc, mesh_obstacle_bindings=None)
    starts, status = [], []

    def note_start(s, k):
        starts.append(s.x.copy())

    def check_bound(s, k):
        assert np.array_equal(s.mesh_obstacle_vertices(0), starts[k - 1][nodes])
        status.append(s.mesh_obstacle_status(0))

    xa = _run(pkg, ctx, sc, 8, each_step=note_start, after_step=check_bound)
    xb = _run(pkg, ctx, unbound, 8, each_step=lambda s, k: s.set_mesh_obstacle_vertices(0, s.x[nodes]))
    xf = _run(pkg, ctx, unbound, 8)
    xa2 = _run(pkg, ctx, sc, 8)
    assert np.array_equal(starts[0], sc.x)
    assert status[-1] == dict(bound=True, refits=8, skipped=0, last_cause=0)
    assert [st["refits"] for st in status] == list(range(1, 9))
    cloth = sc.collision_idx
    o = mc.Oracle(xa[-1][nodes], F, xa[-1][cloth])
    sag = sc.x[nodes, 1].max() - xa[-1][nodes, 1].max()
    print(f"block top sagged by {sag:.4f}; nearest cloth node {o.dist.min():.4f} from the surface; "
          f"max |bound - frozen| at the last step {np.abs(xa[-1] - xf[-1]).max():.3e}")
    for k, (a, b) in enumerate(zip(xa, xb)):
        assert np.array_equal(a, b), f"step {k + 1}: max diff {np.abs(a - b).max():.3e}"
    for a, b in zip(xa, xa2):
        assert np.array_equal(a, b)
    assert not np.array_equal(xa[-1], xf[-1])
    assert (o.dist < 0.02).any()


# --------------------------------------------------------------------------- 4: a skipped refit
def test_gpu_skipped_refit_in_the_solver(pkg, ctx):
    """The cloth over the bound block, 4 steps. After step 2 set_x collapses one surface triangle:
    step 3 skips its refit (skipped = 1, cause 2) and is bitwise the step of a run whose mesh was
    unbound after step 2. After set_x restores a sound shape, step 4 refits again -- and is bitwise
    the step of that run with the setter called on the same vertices: a refused shape leaves
    nothing behind."""
    sc = scenes.cloth_on_soft_block(n_steps=4)
    nodes = sc.mesh_obstacle_bindings[0]
    V, F = sc.mesh_obstacles[0]
    nb = int(sc.groups[0].idx.max()) + 1
    tri = F[len(F) // 2]
    seen = {}

    def edits(s, k):
        if k == 3:
            x = s.x.copy()
            x[nodes[tri[1]]] = x[nodes[tri[0]]]
            _set_x(s, x)
        if k == 4:
            x = s.x.copy()
            x[:nb] = sc.x[:nb]
            _set_x(s, x)
            seen["x4"] = x

    def bound_after(s, k):
        st = s.mesh_obstacle_status(0)
        seen[k] = (st, s.mesh_obstacle_vertices(0))

    def scripted(s, k):
        if k == 3:
            s.bind_mesh_obstacle(0, None)
            assert not s.mesh_obstacle_status(0)["bound"]
        edits(s, k)
        if k == 4:
            s.set_mesh_obstacle_vertices(0, s.x[nodes])

    starts = []
    xa = _run(pkg, ctx, sc, 4, each_step=lambda s, k: (starts.append(s.x.copy()), edits(s, k)), after_step=bound_after)
    xb = _run(pkg, ctx, sc, 4, each_step=scripted)
    print({k: v[0] for k, v in seen.items() if k != "x4"})
    assert seen[2][0] == dict(bound=True, refits=2, skipped=0, last_cause=0)
    assert seen[3][0] == dict(bound=True, refits=2, skipped=1, last_cause=2)
    assert np.array_equal(seen[3][1], starts[1][nodes])          # the shape of step 2's start stays in force
    assert seen[4][0]["refits"] == 3 and seen[4][0]["skipped"] == 1
    assert np.array_equal(seen[4][1], seen["x4"][nodes])
    for k, (a, b) in enumerate(zip(xa, xb)):
        assert np.array_equal(a, b), f"step {k + 1}: max diff {np.abs(a - b).max():.3e}"


# --------------------------------------------------------------------------- 5: exemption at the prox
@pytest.mark.parametrize("order", ["floor_mesh", "mesh_floor", "mesh_sphere_mesh"])
def test_gpu_exempt_prox_equals_deleted_rows(order, pkg, ctx):
    """aa_test_collision_prox_exempt on the mixed lists of test_gpu_collision_prox_ordering, the
    queries spread over three exempt sets (node = query index mod 3: exempt from nothing, from the
    first mesh, from every mesh): bitwise aa_test_collision_prox_posed on the list without the
    query's exempt mesh rows."""
    torus = mc.torus()
    cube = mc.box((-0.2, -0.1, -0.2), (0.2, 0.3, 0.2))
    Q = np.random.default_rng(11).uniform((-0.65, -0.3, -0.65), (0.65, 0.4, 0.65), size=(1500, 3))
    floor = (mc.OBS_FLOOR, [0.05])
    sphere = (mc.OBS_SPHERE, [0.3, 0.0, 0.0, 0.25])
    if order == "floor_mesh":
        obs, meshes = [floor, (mc.OBS_MESH, [0])], [torus]
    elif order == "mesh_floor":
        obs, meshes = [(mc.OBS_MESH, [0]), floor], [torus]
    else:
        obs, meshes = [(mc.OBS_MESH, [0]), sphere, (mc.OBS_MESH, [1])], [torus, cube]
    node = (np.arange(len(Q)) % 3).astype(np.int32)
    exempt = [[1, 2]] + [[2]] * (len(meshes) - 1)          # mesh 0: nodes 1 and 2; later meshes: node 2
    poses = [None] * len(meshes)
    got = pkg.capi.hook_collision_prox_exempt(ctx, obs, meshes, Q, node, exempt, poses)
    full = pkg.capi.hook_collision_prox(ctx, obs, meshes, Q, poses)
    differs = 0
    for g in range(3):
        skip = {m for m in range(len(meshes)) if g in exempt[m]}
        kept = [(t, p) for t, p in obs if not (t == mc.OBS_MESH and int(p[0]) in skip)]
        want = pkg.capi.hook_collision_prox(ctx, kept, meshes, Q[node == g], poses)
        assert np.array_equal(bc.bits(got[node == g]), bc.bits(want)), (order, g)
        differs += (full[node == g] != want).any(1).sum()
    print(f"{order}: {differs} queries answered differently than without exemption")
    assert differs >= 10                                   # the exemption matters on these queries
    none = pkg.capi.hook_collision_prox_exempt(ctx, obs, meshes, Q, node, [None] * len(meshes), poses)
    assert np.array_equal(bc.bits(none), bc.bits(full))


# --------------------------------------------------------------------------- 6: exemption in the solver
def _falling_block(n_steps=4):
    """A 3 x 3 x 3-cell block (64 nodes, 8 of them interior) falling onto Floor, every node a
    collision node, its boundary mesh obstacle 0 bound to its surface nodes."""
    v, t = scenes.kuhn_tet_blocks(3, 3, 3)
    v = v * 0.2
    faces = scenes.tet_boundary_faces(v, t)
    surf = np.unique(faces).astype(np.int32)
    local = np.full(len(v), -1, np.int32)
    local[surf] = np.arange(len(surf), dtype=np.int32)
    assert len(v) - len(surf) == 8
    sc = scenes.Scene(x=v, masses=scenes.tet_masses(v, t, 1522.0), groups=[scenes.ElementGroup(scenes.TET, scenes.LINEAR, 2e5, 0.3, t)],
                      pin_idx=np.zeros(0, np.int32), pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), variant=scenes.VARIANT_H,
                      iters=30, aa_m=6, n_steps=n_steps, accel=1, name="falling_block")
    sc.obstacles = [(scenes.OBS_FLOOR, [-0.01])]
    sc.mesh_obstacles = [(v[surf].copy(), local[faces].astype(np.int32))]
    sc.mesh_obstacle_bindings = [surf]
    sc.collision_idx = np.arange(len(v), dtype=np.int32)
    return sc


def test_gpu_exempt_body_equals_absent_mesh(pkg, ctx):
    """With every node exempt from the block's own bound surface the trajectory is bitwise that of
    the scene whose mesh is added unbound and shifted far outside (every lane culls there, where the
    exempt lanes skip). Without the exemption the interior nodes are thrown to the surface."""
    sc = _falling_block()
    V, F = sc.mesh_obstacles[0]
    everyone = np.arange(sc.n_nodes, dtype=np.int32)
    status = []
    xe = _run(pkg, ctx, dataclasses.replace(sc, mesh_obstacle_exempt=[everyone]), 4,
              after_step=lambda s, k: status.append(s.mesh_obstacle_status(0)))
    far = dataclasses.replace(sc, mesh_obstacles=[(V + np.array([100.0, 0.0, 0.0]), F)], mesh_obstacle_bindings=None)
    xf = _run(pkg, ctx, far, 4)
    xn = _run(pkg, ctx, sc, 4)
    assert status[-1] == dict(bound=True, refits=4, skipped=0, last_cause=0)
    print(f"lowest node {xe[-1][:, 1].min():.4f} (floor at -0.01); max |exempt - not exempt| {np.abs(xe[-1] - xn[-1]).max():.3e}")
    for k, (a, b) in enumerate(zip(xe, xf)):
        assert np.array_equal(a, b), f"step {k + 1}: max diff {np.abs(a - b).max():.3e}"
    assert xe[-1][:, 1].min() < sc.x[:, 1].min()           # it fell
    assert not np.array_equal(xe[-1], xn[-1])
    # an exemption set after initialize and cleared again: the graph is kept, the answer follows
    def toggle(s, k):
        if k == 1:
            s.set_mesh_obstacle_exempt(0, everyone)
        if k == 3:
            s.set_mesh_obstacle_exempt(0, None)
    xt = _run(pkg, ctx, sc, 4, each_step=toggle)
    assert np.array_equal(xt[0], xe[0]) and np.array_equal(xt[1], xe[1]) and not np.array_equal(xt[3], xe[3])


# --------------------------------------------------------------------------- 7: errors
def test_gpu_bound_obstacle_errors(pkg, ctx):
    """Every refusal with its code and message; after each, the next step is bitwise the step of a
    run without the refused calls."""
    AAError = pkg.capi.AAError
    sc = scenes.cloth_on_soft_block(n_steps=3)
    nodes = sc.mesh_obstacle_bindings[0]
    V, F = sc.mesh_obstacles[0]
    R = scenes.rotation_y(0.1)

    def refused(s, k):
        bad_node = nodes.copy()
        bad_node[3] = sc.n_nodes
        calls = [
            (lambda: s.bind_mesh_obstacle(1, nodes), "unknown mesh id 1"),
            (lambda: s.bind_mesh_obstacle(0, nodes[:-1]), f"{len(nodes) - 1} nodes given, mesh 0 has {len(nodes)} vertices"),
            (lambda: s.bind_mesh_obstacle(0, bad_node), f"vertex 3 names node {sc.n_nodes}, out of range"),
            (lambda: s.set_mesh_obstacle_pose(0, R, np.zeros(3)), "mesh 0 is bound to solver nodes"),
            (lambda: s.set_mesh_obstacle_vertices(0, V), "mesh 0 is bound to solver nodes"),
            (lambda: s.set_mesh_obstacle_exempt(1, [0]), "unknown mesh id 1"),
            (lambda: s.set_mesh_obstacle_exempt(0, [-1]), "entry 0 names node -1, out of range"),
            (lambda: s.mesh_obstacle_status(1), "unknown mesh id 1"),
        ]
        for call, msg in calls:
            with pytest.raises(AAError, match=msg) as e:
                call()
            assert e.value.code == -1
        assert s.mesh_obstacle_status(0)["bound"]

    x0 = _run(pkg, ctx, sc, 3)
    x1 = _run(pkg, ctx, sc, 3, each_step=refused)
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    # a posed mesh cannot be bound; a partitioned solver cannot bind
    s = pkg.capi.solver_from_scene(ctx, dataclasses.replace(sc, mesh_obstacle_bindings=None))
    s.set_mesh_obstacle_pose(0, R, np.zeros(3))
    with pytest.raises(AAError, match="mesh 0 has a pose") as e:
        s.bind_mesh_obstacle(0, nodes)
    assert e.value.code == -1
    s.set_mesh_obstacle_pose(0)
    s.bind_mesh_obstacle(0, nodes)                        # unposed again: taken, before initialize
    s.bind_mesh_obstacle(0, None)
    assert s.mesh_obstacle_status(0) == dict(bound=False, refits=0, skipped=0, last_cause=0)
    s.close()
    comm = pkg.capi.Comm.solo(0, 2)
    s = pkg.capi.solver_from_scene(ctx, dataclasses.replace(sc, mesh_obstacle_bindings=None), comm)
    with pytest.raises(AAError, match="partitioned over 2 ranks") as e:
        s.bind_mesh_obstacle(0, nodes)
    assert e.value.code == -1
    s.close()
    comm.close()


def test_gpu_unbind_refreshes_the_host_row(pkg, ctx):
    """After unbinding, a pose set and cleared again writes the mesh's row whole: the root box must
    be the refitted one, not the one from add time -- the run equals the run that only unbinds."""
    sc = scenes.cloth_on_soft_block(n_steps=6)

    def unbind(s, k):
        if k == 4:
            s.bind_mesh_obstacle(0, None)

    def unbind_and_touch(s, k):
        if k == 4:
            s.bind_mesh_obstacle(0, None)
            s.set_mesh_obstacle_pose(0, np.eye(3), np.zeros(3))
            s.set_mesh_obstacle_pose(0)
            assert np.array_equal(s.mesh_obstacle_vertices(0), starts[2][sc.mesh_obstacle_bindings[0]])

    starts = []
    xa = _run(pkg, ctx, sc, 6, each_step=lambda s, k: (starts.append(s.x.copy()), unbind(s, k)))
    xb = _run(pkg, ctx, sc, 6, each_step=unbind_and_touch)
    for a, b in zip(xa, xb):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 8: the facade
def test_gpu_facade_cloth_on_a_sagging_block(tmp_path):
    """admm::Solver::bind_obstacle / exempt_from_obstacle (tests/cpp/facade_bound.cpp run): the block's
    top face (rest height 0.6) has sagged by at least 0.03 after 8 steps -- the CPU oracle's run of the
    same block alone gives 0.07 to 0.12 -- and the cloth's middle node lies on the sagged face, not at
    the rest height: no lower than 0.01 under the face's lowest node, no higher than 0.04 over its
    highest (the obstacle lags one step, in which the face moves by up to 0.02)."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe = str(tmp_path / "facade_bound")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_bound.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    os.makedirs(tmp_path / "result")
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    tmin, tmax, mid = (float(v) for v in r.stdout.split()[-5:-2])
    refits, skipped = (int(v) for v in r.stdout.split()[-2:])
    print(f"top face between {tmin:.4f} and {tmax:.4f} (rest 0.6), the cloth's middle node at {mid:.4f}, {refits} refits, {skipped} skipped")
    assert refits == 8 and skipped == 0
    assert tmax <= 0.6 - 0.03
    assert tmin - 0.01 <= mid <= tmax + 0.04
