"""CPU tests of a carrying mesh's displacement: the numpy restatement (tests/friction_carry_cases.py)
checked for the properties the model is chosen for, on the cube, L-prism, sliver and 16 x 8 torus of
tests/mesh_obs_cases.py; the scene builders; and the C ABI's argument checks that need no device."""
import os
import subprocess

import numpy as np
import pytest

import friction_carry_cases as cc
import friction_cases as fc
import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

MESHES = list(mc.MESHES)


@pytest.mark.parametrize("name", MESHES)
def test_den_is_positive_on_every_triangle(name):
    """The condition the other tests rest on: no triangle of these meshes takes the !(den > 0)
    fallback."""
    V, F = mc.MESHES[name]()
    A, B, C = (V[F[:, k]] for k in range(3))
    _, den = cc.barycentric(A, B, C, A)
    print(f"{name}: den {den.min():.3e} .. {den.max():.3e}")
    assert (den > 0.0).all()


@pytest.mark.parametrize("name", MESHES)
def test_weights_return_the_point(name):
    """b0 A + b1 B + b2 C gives c_l back within the closest-point bar, inside faces, on edges and at
    vertices."""
    V, F = mc.MESHES[name]()
    tri, w, cl = cc.surface_samples(V, F)
    A, B, C = (V[F[tri, k]] for k in range(3))
    b, den = cc.barycentric(A, B, C, cl)
    tol = cc.CP_TOL * max(1.0, np.abs(cl).max())
    err = np.abs(cc.interpolate(b, A, B, C) - cl).max()
    print(f"{name}: {len(cl)} points, max |b.ABC - c_l| {err:.3e} (bar {tol:.1e}), max |b - w| {np.abs(b - w).max():.3e}")
    assert (den > 0).all() and err <= tol
    assert np.abs(b.sum(1) - 1.0).max() <= 4 * np.finfo(float).eps


@pytest.mark.parametrize("posed", [False, True])
@pytest.mark.parametrize("name", MESHES)
def test_rigidly_moved_vertices_give_the_rigid_displacement(name, posed):
    """V- a rigidly moved copy of V: g is obstacle_displacement's value for that motion within the
    bar; V- = V: bit for bit the rigid value, whatever the poses."""
    V, F = mc.MESHES[name]()
    tri, _, cl = cc.surface_samples(V, F)
    pose = kc.POSES["P_rot"] if posed else None
    R, t = pose if posed else kc.IDENTITY
    c = kc.to_world(R, t, cl)
    rows = np.array([fc.row_of(fc.OBS_MESH, (0,))])
    row = np.zeros(len(c), int)
    tol = cc.CP_TOL * max(1.0, np.abs(c).max())
    # (a) the motion in the vertices, the pose unchanged: the same as the motion in the pose
    Rm, tm = cc.RIGID
    V_prev = V @ Rm.T + tm
    g, _, _ = cc.mesh_carry_g(V, V_prev, F, tri, c, pose, pose)
    pose_prev = (R @ Rm, R @ tm + t)              # x -> R (Rm x + tm) + t
    want = fc.obstacle_displacement(rows, rows, [pose], [pose_prev], [False], row, c)
    print(f"{name}{' posed' if posed else ''}: max |g - g_rigid| {np.abs(g - want).max():.3e} (bar {tol:.1e}), max |g| {np.abs(g).max():.3e}")
    assert np.abs(g - want).max() <= tol and np.abs(g).max() > 1e-3
    # (b) unchanged vertices and a different previous pose: the rigid expression's bits
    other = (kc.rotation((1.0, 2.0, 3.0), 0.7 - 0.03), t - np.array([0.002, 0.0, -0.003])) if posed else \
        (kc.rotation((0, 1, 0), -0.03), np.array([0.0, 0.002, 0.0]))
    g0, _, _ = cc.mesh_carry_g(V, V.copy(), F, tri, c, pose, other)
    want0 = fc.obstacle_displacement(rows, rows, [pose], [other], [False], row, c)
    assert np.array_equal(g0, want0) and np.abs(g0).max() > 1e-3


@pytest.mark.parametrize("name", MESHES)
def test_shared_edge_gives_one_displacement(name):
    """A point on a shared edge: the two incident triangles give the same g within the bar, for a
    deformation that is not rigid."""
    import deform_cases as dc
    V, F = dc.base(name)
    V_prev = dc.deform(V, 0.5)
    rng = np.random.default_rng(9)
    E = cc.shared_edges(F)
    t0, t1, p, q = (np.array(x) for x in zip(*E))
    s = rng.uniform(0.0, 1.0, len(E))[:, None]
    s[::5] = 0.0                                   # some at the shared vertex itself
    cl = (1.0 - s) * V[p] + s * V[q]
    g0, _, _ = cc.mesh_carry_g(V, V_prev, F, t0, cl, None, None)
    g1, _, _ = cc.mesh_carry_g(V, V_prev, F, t1, cl, None, None)
    tol = cc.CP_TOL * max(1.0, np.abs(cl).max(), np.abs(V_prev).max())
    print(f"{name}: {len(E)} edges, max |g(t0) - g(t1)| {np.abs(g0 - g1).max():.3e} (bar {tol:.1e}), max |g| {np.abs(g0).max():.3e}")
    assert len(E) == 3 * len(F) // 2
    assert np.abs(g0 - g1).max() <= tol and np.abs(g0).max() > 1e-2


def test_scene_builders():
    cv = scenes.block_on_conveyor_mesh(1.0, 0.01, n_steps=5)
    V, F = cv.mesh_obstacles[0]
    tt = scenes.block_on_turntable(1.0, n_steps=5)
    assert np.array_equal(V, tt.mesh_obstacles[0][0]) and np.array_equal(F, tt.mesh_obstacles[0][1])
    assert cv.mesh_obstacle_carry == [True] and cv.obstacle_friction == [1.0] and cv.obstacles == [] and cv.mesh_obstacle_poses is None
    assert all(np.array_equal(cv.mesh_obstacle_vertices[k][0], V + [0.01 * (k + 1), 0.0, 0.0]) for k in range(5))
    assert scenes.block_on_conveyor_mesh(1.0, 0.01, carry=False).mesh_obstacle_carry == [False]
    tw = scenes.block_on_twisting_slab(1.0, 0.01, n_steps=5)
    assert np.abs(tw.mesh_obstacle_vertices[2][0] - V @ scenes.rotation_y(0.03).T).max() == 0.0 and tw.mesh_obstacle_carry == [True]
    assert np.array_equal(tw.x, tt.x) and np.array_equal(tw.collision_idx, tt.collision_idx)
    sb = scenes.block_on_sliding_block(1.0, 0.6, n_steps=5)
    Vb, Fb = sb.mesh_obstacles[0]
    lower = sb.mesh_obstacle_exempt[0]
    assert mc.signed_volume(Vb, Fb) > 0 and np.array_equal(Vb, sb.x[sb.mesh_obstacle_bindings[0]])
    assert sb.obstacles == [(fc.OBS_FLOOR, (0.0,))] and sb.obstacle_friction == [0.0, 1.0] and sb.mesh_obstacle_carry == [True]
    assert np.array_equal(sb.initial_velocity[lower], np.tile([0.6, 0.0, 0.0], (len(lower), 1)))
    upper = np.setdiff1d(np.arange(sb.n_nodes), lower)
    assert not sb.initial_velocity[upper].any() and len(upper) == 75
    top = sb.x[lower, 1].max()
    on_top = np.intersect1d(sb.collision_idx, upper)
    assert len(on_top) == 25 and (sb.x[on_top, 1] == top).all() and (sb.x[np.intersect1d(sb.collision_idx, lower), 1] == 0.0).all()
    assert np.abs(sb.x[on_top][:, [0, 2]]).max() < np.abs(Vb[:, [0, 2]]).max() - 0.3       # well inside the lower block's top face
    # today's scenes are unchanged by default
    assert tt.mesh_obstacle_carry is None and tt.initial_velocity is None and scenes.cloth(4, 4).mesh_obstacle_carry is None


def test_exports_and_null_arguments(pkg):
    """The new entry points exist, and a null handle or context is AA_ERR_ARG without a device."""
    import ctypes as C
    lib = pkg.capi.lib()
    for name in ("aa_elastic_set_mesh_obstacle_carry", "aa_elastic_get_mesh_obstacle_carry", "aa_elastic_get_contact_features",
                 "aa_test_contact_friction_carry"):
        assert name in pkg.capi.EXPORTS and hasattr(lib, name)
    on, n = C.c_int(), C.c_int()
    assert lib.aa_elastic_set_mesh_obstacle_carry(None, 0, 1) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_get_mesh_obstacle_carry(None, 0, C.byref(on)) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_get_contact_features(None, 0, C.byref(n), None, None) == -1 and b"null" in lib.aa_last_error()
    args = [None] * 37
    args[4] = args[9] = args[15] = 0
    args[23], args[24] = C.c_double(1.0), C.c_double(0.01)
    assert lib.aa_test_contact_friction_carry(*args) == -1 and b"null context" in lib.aa_last_error()


def test_facade_carry_builds(tmp_path):
    lib = os.path.join(REPO, "aa-admm_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_carry.cpp"), "-o", str(tmp_path / "facade_carry"),
                    "-L" + lib, "-laa_admm", "-Wl,-rpath," + lib], check=True)
