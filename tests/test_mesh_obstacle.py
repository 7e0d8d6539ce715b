"""CPU tests of the triangle-mesh passive obstacle (PassiveMesh): the host preparation
(csrc/mesh_obstacle.hpp: validation, pseudonormal table, leaf order) in a stand-alone program,
the self-check of the brute-force oracle the GPU tests are pinned to (tests/mesh_obs_cases.py),
the C++ facade's admm::PassiveMesh and the Python scene helpers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

CSRC = os.path.join(REPO, "aa-admm_amd", "csrc")


def test_host_preparation_validates_and_builds_pseudonormals(tmp_path):
    """tests/cpp/mesh_obstacle.cpp: the four meshes are accepted, each broken variant is refused
    with ERR_ARG naming the element, the tables are in leaf order, the cube's pseudonormals are the
    expected ones."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    path = tmp_path / "meshes.txt"
    with open(path, "w") as f:
        for name, make in mc.MESHES.items():
            V, F = make()
            assert len(F) == mc.N_TRIS[name]
            f.write(f"{name} {len(V)} {len(F)}\n")
            f.write("\n".join(" ".join(repr(float(c)) for c in v) for v in V) + "\n")
            f.write("\n".join(" ".join(str(int(i)) for i in t) for t in F) + "\n")
    exe = str(tmp_path / "mesh_obstacle")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "mesh_obstacle.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok 4 meshes" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", list(mc.MESHES))
def test_oracle_self_check(name):
    """The oracle the GPU tests use: at most 1 % of a mesh's queries are left out, and on every
    kept query the pseudonormal's inside flag equals the generalized winding number's. Every one of
    Ericson's seven regions occurs, and both signs."""
    V, F, Q, o = mc.case(name)
    assert mc.signed_volume(V, F) > 0
    assert len(Q) == 2600
    k = o.keep
    assert (~k).sum() <= mc.MAX_EXCLUDED * len(Q), f"{(~k).sum()} of {len(Q)} queries excluded"
    assert np.array_equal(o.inside[k], o.inside_wn[k]), f"{(o.inside[k] != o.inside_wn[k]).sum()} disagree"
    assert (np.bincount(o.region[k], minlength=7) > 0).all(), np.bincount(o.region[k], minlength=7)
    assert o.inside[k].any() and (~o.inside[k]).any()


def test_sliver_tells_the_pseudonormal_from_the_face_normal():
    """On the sliver the naive rule -- the face normal of the first-found closest triangle -- calls
    outside points near the sharp edge inside; the pseudonormal does not. So a test against this
    oracle on this mesh fails for an implementation of the naive rule."""
    V, F, Q, o = mc.case("sliver")
    k = o.keep
    wrong = k & (o.inside_naive != o.inside_wn)
    assert wrong.sum() >= 50, wrong.sum()
    assert (~o.inside_wn[wrong]).all()           # all of them outside points called inside
    assert (o.region[wrong] != 6).all()          # ... whose closest point is on an edge or a vertex
    assert np.array_equal(o.inside[k], o.inside_wn[k])


def test_collision_prox_rule_regimes():
    """The numpy ordering rule: a mesh's inside hit overrides a deeper earlier floor hit, a later
    floor competes with its own test, a miss leaves the payload alone."""
    V, F = mc.box((0, 0, 0), (1, 1, 1))
    Q = np.array([[0.5, 0.9, 0.5], [0.5, 1.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 0.1]])
    o = mc.Oracle(V, F, Q)
    floor = (mc.OBS_FLOOR, [2.0])
    mesh = (mc.OBS_MESH, [0])
    got = mc.collision_prox_rule([floor, mesh], [o], Q)     # mesh last: it wins wherever it is hit
    np.testing.assert_allclose(got, [[0.5, 1.0, 0.5], [0.5, 2.0, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 0.0]], atol=1e-15)
    got = mc.collision_prox_rule([mesh, floor], [o], Q)     # floor last: deeper than every mesh hit here
    np.testing.assert_allclose(got, [[0.5, 2.0, 0.5], [0.5, 2.0, 0.5], [0.5, 2.5, 0.5], [0.5, 2.0, 0.1]], atol=1e-15)


def test_facade_passive_mesh(tmp_path):
    """include/aa_admm.hpp compiles with admm::PassiveMesh; from_tets takes the outward boundary
    faces (tests/cpp/facade_mesh.cpp without arguments touches no GPU)."""
    lib = os.path.join(REPO, "aa-admm_amd")
    exe = str(tmp_path / "facade_mesh")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_mesh.cpp"), "-o", exe, "-L" + lib, "-laa_admm",
                    "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_tet_boundary_faces_and_scene_field(pkg):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], float)
    for tets in ([[0, 1, 2, 3]], [[0, 2, 1, 3]], [[0, 1, 2, 3], [1, 2, 3, 4]], [[0, 1, 2, 3], [4, 3, 2, 1]]):
        F = scenes.tet_boundary_faces(v, np.array(tets, np.int32))
        assert F.dtype == np.int32 and len(F) == (4 if len(tets) == 1 else 6)
        vol = sum(abs(np.linalg.det(v[t[1:]] - v[t[0]])) / 6.0 for t in tets)
        assert abs(mc.signed_volume(v, F) - vol) < 1e-15
        d = {}
        for t in F:
            for a in range(3):
                d[(t[a], t[(a + 1) % 3])] = d.get((t[a], t[(a + 1) % 3]), 0) + 1
        assert all(n == 1 and d.get((q, p)) == 1 for (p, q), n in d.items())
    sc = scenes.cloth_on_torus()
    assert sc.variant == scenes.VARIANT_H and len(sc.mesh_obstacles) == 1 and len(sc.collision_idx) == sc.n_nodes
    V, F = sc.mesh_obstacles[0]
    assert len(F) == 256 and mc.signed_volume(V, F) > 0
    assert scenes.cloth(4, 4).mesh_obstacles == []
    assert "aa_elastic_add_mesh_obstacle" in pkg.capi.EXPORTS and scenes.OBS_MESH == 5


def test_add_mesh_obstacle_argument_errors_without_device(pkg):
    lib = pkg.capi.lib()
    assert lib.aa_elastic_add_mesh_obstacle(None, None, 0, None, 0, None) == -1
    assert b"null" in lib.aa_last_error()
