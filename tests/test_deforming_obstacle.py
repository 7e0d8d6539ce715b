"""CPU tests of the deforming mesh obstacle (aa_elastic_set_mesh_obstacle_vertices): the host
restatement of the refit (csrc/mesh_obstacle.hpp, refit_mesh_obstacle_host) in a stand-alone program
built with the address and undefined-behaviour sanitizers, the self-check of the cases the GPU tests
use (tests/deform_cases.py) and the scene layer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import deform_cases as dc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

CSRC = os.path.join(REPO, "aa-admm_amd", "csrc")
CORNER_SLOT, EDGE_SLOT = (0, 1, 3), (2, 5, 4)   # a b c; ab bc ca


def _pn_rows(V, F):
    """mc.pseudonormals per triangle in the table's feature order: (m, 21)."""
    fn, en, vn = mc.pseudonormals(V, F)
    out = np.zeros((len(F), 21))
    for t, f in enumerate(F):
        for a in range(3):
            p, q = int(f[a]), int(f[(a + 1) % 3])
            out[t, 3 * CORNER_SLOT[a]:3 * CORNER_SLOT[a] + 3] = vn[p]
            out[t, 3 * EDGE_SLOT[a]:3 * EDGE_SLOT[a] + 3] = en[(min(p, q), max(p, q))]
        out[t, 18:] = fn[t]
    return out


def test_host_refit_program(tmp_path):
    """tests/cpp/mesh_refit.cpp on every case: conservative (and tight) node bounds, the identity
    refit bit for bit, pn against mc.pseudonormals to 1e-13, the refusals."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    path = tmp_path / "cases.txt"
    n = 0
    with open(path, "w") as f:
        for name, s in dc.CASES:
            V, F, W = dc.shape(name, s)
            f.write(f"{name}-{s} {len(V)} {len(F)}\n")
            f.write("\n".join(" ".join(repr(float(c)) for c in v) for v in V) + "\n")
            f.write("\n".join(" ".join(str(int(i)) for i in t) for t in F) + "\n")
            f.write("\n".join(" ".join(repr(float(c)) for c in v) for v in W) + "\n")
            f.write("\n".join(" ".join(repr(float(c)) for c in row) for row in _pn_rows(W, F)) + "\n")
            n += 1
    exe = str(tmp_path / "mesh_refit")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "mesh_refit.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and f"ok {n} cases" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


@pytest.mark.parametrize("name,s", dc.CASES, ids=dc.IDS)
def test_deformed_case_self_check(name, s):
    """Every case is a sound obstacle and a sound oracle: positive volume, no tiny triangle, at most
    1 % of the queries left out, and the pseudonormal's inside flag equal to the winding number's on
    every kept query."""
    V, F, W, Q, o = dc.case(name, s)
    assert W.shape == V.shape and mc.signed_volume(W, F) > 0
    assert dc.min_area(W, F) >= 3e-4
    assert len(Q) == 2600
    k = o.keep
    assert (~k).sum() <= mc.MAX_EXCLUDED * len(Q), f"{(~k).sum()} of {len(Q)} queries excluded"
    assert np.array_equal(o.inside[k], o.inside_wn[k]), f"{(o.inside[k] != o.inside_wn[k]).sum()} disagree"
    assert o.inside[k].any() and (~o.inside[k]).any()
    if s is None:
        assert np.array_equal(W, V) and W is not V
    else:
        assert np.abs(W - V).max() > 0.01


def test_the_fine_torus_has_split_nodes():
    """kRefitChunk (csrc/mesh_obstacle.hpp) is 1024 triangles: the fine torus' root and its two
    children are reduced in chunks, the coarse meshes have single-leaf and partial-wave nodes only."""
    assert len(dc.base("torus_fine")[1]) == 2304 and len(dc.base("torus")[1]) == 256
    assert len(dc.base("sliver")[1]) == 4


def test_breathing_torus_scene(pkg):
    plain = scenes.cloth_on_torus(n_steps=6)       # the existing demo is as it was: ring = 0.3 of the sheet's side
    assert np.array_equal(plain.mesh_obstacles[0][0], scenes.torus_mesh(16, 8, 0.3 * 2.0, 0.4 * (0.3 * 2.0))[0])
    assert plain.x[0, 1] == 0.4 * (0.3 * 2.0) + 0.15 and plain.mesh_obstacle_vertices is None
    base = scenes.cloth_on_torus(n_steps=6, ring=0.42)
    sc = scenes.cloth_on_breathing_torus(n_steps=6)
    V0, F = sc.mesh_obstacles[0]
    assert np.array_equal(V0, base.mesh_obstacles[0][0]) and np.array_equal(F, base.mesh_obstacles[0][1])
    assert np.array_equal(sc.x, base.x) and base.mesh_obstacle_vertices is None
    assert scenes.cloth(4, 4).mesh_obstacle_vertices is None
    shapes = sc.mesh_obstacle_vertices
    assert len(shapes) == 6 and all(len(row) == 1 for row in shapes)
    r0 = np.abs(V0[:, 1]).max()
    radii = []
    for row in shapes:
        assert row[0].shape == V0.shape and row[0].dtype == np.float64
        assert mc.signed_volume(row[0], F) > 0
        radii.append(np.abs(row[0][:, 1]).max())
    assert all(b > a for a, b in zip([r0] + radii, radii))        # growing over these steps ...
    full = scenes.cloth_on_breathing_torus(n_steps=40).mesh_obstacle_vertices
    rr = [np.abs(row[0][:, 1]).max() for row in full]
    assert min(rr) >= r0 * (1 - 1e-12) and rr[9] == max(rr) and rr[19] < rr[14] < rr[9]   # ... and back
    for name in ("aa_elastic_set_mesh_obstacle_vertices", "aa_elastic_get_mesh_obstacle_vertices", "aa_test_mesh_refit_tables",
                 "aa_test_mesh_sdf_deformed"):
        assert name in pkg.capi.EXPORTS


def test_host_refit_hook_without_device(pkg):
    """aa_test_mesh_refit_tables with device = 0 needs no context: the identity reproduces the built
    tables, a deformed shape gives the pseudonormals of a mesh built from it, and a refused shape is
    AA_ERR_ARG naming the cause."""
    V, F, W = dc.shape("torus", 0.5)
    built = pkg.capi.hook_mesh_refit_tables(None, V, F, None, device=0)
    same = pkg.capi.hook_mesh_refit_tables(None, V, F, V, device=0)
    for k in built:
        assert np.array_equal(built[k], same[k]), k
    got = pkg.capi.hook_mesh_refit_tables(None, V, F, W, device=0)
    assert np.array_equal(got["orig"], built["orig"]) and got["nodes"].shape == built["nodes"].shape
    assert np.array_equal(got["tris"], W[F[got["orig"]]].reshape(-1, 9))
    assert np.abs(got["pn"] - _pn_rows(W, F)[got["orig"]]).max() <= 1e-13
    assert np.array_equal(got["lo"], W.min(0)) and np.array_equal(got["hi"], W.max(0))
    with pytest.raises(pkg.capi.AAError, match="signed volume"):
        pkg.capi.hook_mesh_refit_tables(None, V, F, -V, device=0)
    lib = pkg.capi.lib()
    assert lib.aa_elastic_set_mesh_obstacle_vertices(None, 0, None) == -1 and b"null" in lib.aa_last_error()
