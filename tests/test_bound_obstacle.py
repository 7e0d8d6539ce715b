"""CPU tests of the bound mesh obstacle (aa_elastic_bind_mesh_obstacle) and the exemption
(aa_elastic_set_mesh_obstacle_exempt): the host restatement of gather + check + refit
(csrc/mesh_obstacle.hpp) in a stand-alone program built with the address and undefined-behaviour
sanitizers, the same through the hook without a device, the scene layer and the null-handle paths."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bound_cases as bc
import deform_cases as dc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

CSRC = os.path.join(REPO, "aa-admm_amd", "csrc")


def test_host_bound_refit_program(tmp_path):
    """tests/cpp/bound_refit.cpp on every deform_cases shape, embedded in a permuted, decoy-padded
    node array: tables bitwise those of refit_mesh_obstacle_host on x[nodes], vol6 bitwise the numpy
    restatement of the chunked sum, the three refusals."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    path = tmp_path / "cases.txt"
    n = 0
    with open(path, "w") as f:
        for name, s in dc.CASES:
            V, F, W = dc.shape(name, s)
            X, nodes = bc.embed(W, seed=11 + n)
            assert len(X) >= len(W) + 30 and np.array_equal(X[nodes], W)
            f.write(f"{name}-{s} {len(V)} {len(F)} {len(X)}\n")
            f.write("\n".join(" ".join(repr(float(c)) for c in v) for v in V) + "\n")
            f.write("\n".join(" ".join(str(int(i)) for i in t) for t in F) + "\n")
            f.write("\n".join(" ".join(repr(float(c)) for c in v) for v in X) + "\n")
            f.write(" ".join(str(int(i)) for i in nodes) + "\n")
            f.write(float(bc.vol6_chunked(W, F)).hex() + "\n")
            n += 1
    exe = str(tmp_path / "bound_refit")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "bound_refit.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and f"ok {n} cases" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_chunked_sum_is_a_signed_volume():
    """The restated sum is 6 x the signed volume up to rounding, and the chunk is 256."""
    V, F, W = dc.shape("torus_fine", 0.5)
    assert len(F) == 9 * bc.CHUNK
    assert abs(bc.vol6_chunked(W, F) - 6.0 * mc.signed_volume(W, F)) <= 1e-12 * abs(6.0 * mc.signed_volume(W, F))


def test_host_bound_hook_without_device(pkg):
    """aa_test_bound_refit with device = 0 and no context."""
    V, F, W = dc.shape("torus", 0.5)
    X, nodes = bc.embed(W, decoy_nan=True)
    built = pkg.capi.hook_mesh_refit_tables(None, V, F, None, device=0)
    want = pkg.capi.hook_mesh_refit_tables(None, V, F, X[nodes], device=0)
    got = pkg.capi.hook_bound_refit(None, V, F, X, nodes, device=0)
    assert got["taken"] and got["cause"] == 0
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert bc.bits(got["vol6"]) == bc.bits(bc.vol6_chunked(W, F))
    bad = []
    Y = X.copy(); Y[nodes[1], 2] = np.nan; bad.append((Y, 1))
    Y = X.copy(); Y[nodes[F[2, 1]]] = Y[nodes[F[2, 0]]]; bad.append((Y, 2))
    bad.append((-X, 3))
    for Y, cause in bad:
        r = pkg.capi.hook_bound_refit(None, V, F, Y, nodes, device=0)
        assert not r["taken"] and r["cause"] == cause
        for k in built:
            assert np.array_equal(r[k], built[k]), (cause, k)
        after = pkg.capi.hook_bound_refit(None, V, F, X, nodes, device=0, X_first=Y)   # a good shape after a refused one
        for k in got:
            assert np.array_equal(after[k], got[k]), (cause, k)
    with pytest.raises(pkg.capi.AAError, match="out of range"):
        pkg.capi.hook_bound_refit(None, V, F, X, np.where(np.arange(len(nodes)) == 3, len(X), nodes), device=0)


def test_soft_block_scene(pkg):
    sc = scenes.cloth_on_soft_block()
    (V, F), = sc.mesh_obstacles
    nodes, = sc.mesh_obstacle_bindings
    assert sc.variant == scenes.VARIANT_H and sc.n_steps == 8 and sc.mesh_obstacle_exempt is None
    # closed, consistently oriented (every directed edge once, its reverse once), outward
    edges = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    fwd = {(int(a), int(b)) for a, b in edges}
    assert len(fwd) == len(edges) and all((b, a) in fwd for a, b in fwd)
    assert mc.signed_volume(V, F) > 0
    tets = sc.groups[0].idx
    nb = int(tets.max()) + 1
    block = sc.x[:nb]
    assert abs(mc.signed_volume(V, F) - np.prod(block.max(0) - block.min(0))) < 1e-12
    # the binding indexes exactly the block's surface nodes: those on a face of its bounding box
    on_box = np.nonzero(np.any((np.abs(block - block.min(0)) < 1e-12) | (np.abs(block - block.max(0)) < 1e-12), axis=1))[0]
    assert np.array_equal(np.sort(nodes), on_box) and len(np.unique(nodes)) == len(nodes) == len(V)
    assert np.array_equal(sc.x[nodes], V)
    assert len(on_box) < nb                                     # it has interior nodes
    # pinned bottom face; the cloth is 12 x 12 cells, above the block, and holds the collision nodes
    assert np.array_equal(np.sort(sc.pin_idx), np.nonzero(block[:, 1] == block[:, 1].min())[0])
    cloth = scenes.tri_blocks(12, 12)[0]
    assert np.array_equal(sc.collision_idx, np.arange(nb, nb + len(cloth)))
    assert sc.x[nb:, 1].min() > block[:, 1].max() and len(sc.x) == nb + len(cloth)
    for other in (scenes.cloth(4, 4), scenes.cloth_on_torus(n_steps=2), scenes.cloth_on_breathing_torus(n_steps=2)):
        assert other.mesh_obstacle_bindings is None and other.mesh_obstacle_exempt is None
    for name in ("aa_elastic_bind_mesh_obstacle", "aa_elastic_mesh_obstacle_status", "aa_elastic_set_mesh_obstacle_exempt",
                 "aa_test_bound_refit", "aa_test_collision_prox_exempt"):
        assert name in pkg.capi.EXPORTS
        assert hasattr(pkg.capi.lib(), name)


def test_null_handle(pkg):
    """A null handle or null pointers are AA_ERR_ARG without a device."""
    import ctypes as C
    lib = pkg.capi.lib()
    one = (C.c_int * 1)(0)
    assert lib.aa_elastic_bind_mesh_obstacle(None, 0, one, 1) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_set_mesh_obstacle_exempt(None, 0, one, 1) == -1 and b"null" in lib.aa_last_error()
    assert lib.aa_elastic_mesh_obstacle_status(None, 0, None, None, None, None) == -1 and b"null" in lib.aa_last_error()
    V, F = dc.base("cube")
    v = np.ascontiguousarray(V, np.float64)
    f = np.ascontiguousarray(F, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib.aa_test_bound_refit(None, v.ctypes.data_as(dp), len(v), f.ctypes.data_as(ip), len(f), None, 0, None, 0,
                                 None, None, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"null" in lib.aa_last_error()
    rc = lib.aa_test_bound_refit(None, v.ctypes.data_as(dp), len(v), f.ctypes.data_as(ip), len(f), None, 0, None, 1,
                                 None, None, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"null context" in lib.aa_last_error()
    rc = lib.aa_test_collision_prox_exempt(None, None, 0, None, None, None, None, 0, None, None, None, 0, None, None, None)
    assert rc == -1 and b"null context" in lib.aa_last_error()
