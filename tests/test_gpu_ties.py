"""GPU tests of the tie term (aa_elastic_add_ties) and of the closest-point query that finds its
anchors (aa_closest_on_triangles): whole trajectories against the numpy port with tie rows
(tests/tie_cases.py; tests/test_ties.py holds the port to its conditioning and margin conditions),
three closed forms, the rest shape as an equilibrium, the runtime counts, bitwise guards, ties beside
contact and friction, the refusals, and the query against brute force on closed and open lists."""
import dataclasses

import numpy as np
import pytest

import friction_carry_cases as fc
import mesh_obs_cases as mc
import spring_cases as sp
import tie_cases as tc
from golden_io import scenes

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KEYS = ("prim", "comb", "reject", "x", "v")
CP_TOL = 1e-13   # the project's closest-point bar (unit-size meshes; test_gpu_mesh_obstacle.py)


def _run(pkg, ctx, sc, n_steps=None):
    out, s = pkg.capi.run_scene(ctx, sc, n_steps)
    s.close()
    return out


def _runtime(pkg, ctx, sc):
    s = pkg.capi.solver_from_scene(ctx, sc)
    s.initialize(pkg.capi.settings_from_scene(sc))
    rt = s.runtime()
    s.close()
    return rt


# ---------------------------------------------------------------- a. trajectories against the port
@pytest.mark.parametrize("name", list(tc.TRAJ))
def test_trajectory_matches_port(name, pkg, ctx):
    """The project's closed-form tolerances, as test_gpu_springs.test_trajectory_matches_port states
    them: curves 1e-9 comb_0 of each step (prim 1e-8 prim_0), equal record counts, reject flags equal
    over the first 20 iterations, final x and v 1e-9 relative. The one-sided scenes satisfy the margin
    condition in the port (asserted again here on the shared run)."""
    sc, want, P = tc.port(name)
    if tc.tie_mode(sc) & 3:
        assert P.margin >= 1e-6 and P.mixed
    got = _run(pkg, ctx, sc)
    d = tc.deviations(want, got)
    print(f"{name}: records {[len(g['comb']) for g in got]} (port {[len(w['comb']) for w in want]}), comb dev {d[0]:.3e}, "
          f"prim dev {d[1]:.3e}, x rel {d[2]:.3e}, v rel {d[3]:.3e}, rejects {[int(g['reject'].sum()) for g in got]}")
    fails = tc.check_trajectory(want, got, 1e-9)
    assert not fails, fails
    if name == "panels_m3":
        rt = _runtime(pkg, ctx, sc)
        assert rt.n_elements == 36 + 6 and rt.z_dim == 36 * 6 + 6 * 3


def test_long_ties_keep_the_factor_sparse(pkg, ctx):
    """A 13 x 13 cloth with 26 node-triangle ties across the top bisection of the dissection
    (tie_cases.long_ties_13): the counts are the triangles' and the ties', and the factor stays below
    one dense front. The run matches the port like the trajectories above."""
    sc = tc.long_ties_13()
    rt = _runtime(pkg, ctx, sc)
    assert rt.n_elements == 288 + 26 and rt.z_dim == 288 * 6 + 26 * 3 and rt.n_free == 167
    assert rt.nnz_factor < rt.n_free * (rt.n_free + 1) // 2, rt.nnz_factor
    want, got = tc.admm_ux(sc), _run(pkg, ctx, sc)
    print("long_ties_13: comb %.3e prim %.3e x %.3e v %.3e" % tc.deviations(want, got))
    fails = tc.check_trajectory(want, got, 1e-9)
    assert not fails, fails


# ---------------------------------------------------------------- b. closed forms
def test_hanging_mass_settles_at_mg_over_k(pkg, ctx):
    """One mass hung by a soft tie from a point of the pinned triangle, 60 steps: |extension - m g / k|
    <= 8 max(port's error, 64 eps 0.5), the springs' form; the sideways drift alike."""
    sc = tc.hanging_mass_scene()
    port, port_drift = tc.hanging_mass_error(tc.admm_ux(sc), sc)
    err, drift = tc.hanging_mass_error(_run(pkg, ctx, sc), sc)
    print(f"|extension - m g / k|: GPU {err:.3e}, port {port:.3e}; drift GPU {drift:.3e}, port {port_drift:.3e}")
    assert err <= 8 * max(port, 64 * EPS * 0.5)
    assert drift <= 8 * max(port_drift, 64 * EPS * 0.5)


def test_a_tie_is_an_internal_force(pkg, ctx):
    """Two free triangles joined by one triangle-triangle tie, no gravity: |sum m v|inf / sum m |v| <=
    8 max(port's value, 64 eps) at every step."""
    sc = tc.two_triangles_scene()
    port = tc.momentum_ratio(tc.admm_ux(sc), sc)
    out = _run(pkg, ctx, sc)
    got = tc.momentum_ratio(out, sc)
    print(f"momentum ratio: GPU {got:.3e}, port {port:.3e}")
    assert got <= 8 * max(port, 64 * EPS)
    assert np.abs(out[-1]["v"]).max() > 1e-3


def test_reaches_the_dense_minimiser_of_zero_length_ties(pkg, ctx):
    """Zero-length soft ties only on the panels' nodes (quadratic), no Anderson, one step, 100
    iterations: |x - x*|inf <= 8 max(port's error, 64 eps max|x*|)."""
    sc = tc.zero_length_panels()
    xstar, move = tc.dense_minimiser(sc)
    port = np.abs(tc.admm_ux(sc)[0]["x"] - xstar).max()
    err = np.abs(_run(pkg, ctx, sc)[0]["x"].reshape(-1, 3) - xstar).max()
    print(f"|x - x*|inf: GPU {err:.3e}, port {port:.3e}; displacement {move:.3e}")
    assert err <= 8 * max(port, 64 * EPS * np.abs(xstar).max())


# ---------------------------------------------------------------- c. rest equilibrium
def test_rest_is_an_equilibrium(pkg, ctx):
    """panels with derived L (rest = None), gravity 0, no pins, 5 steps: every node within 1e-12 of the
    extent of where it started. All L scaled by 0.9: it moves by more than 1e-6 of the extent."""
    keep = tc.panels(pins=(), rest=None, gravity=0.0, n_steps=5)
    assert keep.ties[0][5] is None and len(keep.pin_idx) == 0
    ext = float((keep.x.max(0) - keep.x.min(0)).max())
    x = _run(pkg, ctx, keep)[-1]["x"].reshape(-1, 3)
    print(f"derived L: max move {np.abs(x - keep.x).max() / ext:.3e} of the extent")
    assert np.abs(x - keep.x).max() <= 1e-12 * ext
    short = tc.panels(pins=(), lo=0.9, hi=0.9, gravity=0.0, n_steps=5)
    xs = _run(pkg, ctx, short)[-1]["x"].reshape(-1, 3)
    print(f"0.9 L: max move {np.abs(xs - short.x).max() / ext:.3e} of the extent")
    assert np.abs(xs - short.x).max() > 1e-6 * ext


# ---------------------------------------------------------------- d. beside the rest of the solver
def test_scene_without_the_field_is_bitwise_the_same(pkg, ctx):
    """A scene object without the `ties` attribute, ties=None and ties=[] give bitwise equal runs and
    equal runtime() counts."""
    sc = scenes.stitched_panels(n_steps=2)
    assert sc.ties is None

    class Bare:
        pass

    bare = Bare()
    for f in dataclasses.fields(sc):
        if f.name != "ties":
            setattr(bare, f.name, getattr(sc, f.name))
    bare.rest_x, bare.n_nodes = sc.rest_x, sc.n_nodes
    assert not hasattr(bare, "ties")
    empty = dataclasses.replace(sc, ties=[])
    runs, counts = [], []
    for scene in (sc, bare, empty):
        out, s = pkg.capi.run_scene(ctx, scene)
        rt = s.runtime()
        counts.append((rt.n_elements, rt.z_dim, rt.n_free, rt.n_pinned, rt.nnz_factor))
        s.close()
        runs.append(out)
    assert counts[0] == counts[1] == counts[2]
    for other in runs[1:]:
        for k in range(2):
            for key in KEYS:
                assert np.array_equal(runs[0][k][key], other[k][key]), (k, key)


def test_patch_on_block_over_a_floor_with_friction(pkg, ctx, monkeypatch):
    """patch_on_block: node-triangle ties beside tets, triangles, a floor and its friction pass, 2
    steps. Graph replay equals eager bitwise, a rerun is bitwise equal, x is finite, contacts are
    recorded, and the ties hold the patch to the block (no tie longer than twice its rest length)."""
    sc = scenes.patch_on_block(n_steps=2)
    a, b = _run(pkg, ctx, sc), _run(pkg, ctx, sc)
    monkeypatch.setenv("AA_ADMM_NO_GRAPH", "1")
    eager = _run(pkg, ctx, sc)
    monkeypatch.delenv("AA_ADMM_NO_GRAPH")
    for k in range(sc.n_steps):
        for key in KEYS:
            assert np.array_equal(a[k][key], b[k][key]), ("rerun", k, key)
            assert np.array_equal(a[k][key], eager[k][key]), ("eager", k, key)
    got, s = pkg.capi.run_scene(ctx, sc)
    n_contacts = len(s.contacts()["node"])
    s.close()
    assert n_contacts > 0 and all(np.isfinite(o["x"]).all() for o in a)
    pa, pb = tc.anchors(a[-1]["x"], sc.ties[0])
    assert sp.norm3(pb - pa).max() < 2 * 0.03
    sewn = scenes.sewn_panels_offset()
    out = _run(pkg, ctx, sewn)
    pa0, pb0 = tc.anchors(sewn.x, sewn.ties[0])
    pa, pb = tc.anchors(out[-1]["x"], sewn.ties[0])
    assert np.isfinite(out[-1]["x"]).all() and sp.norm3(pb - pa).max() < sp.norm3(pb0 - pa0).min()   # the seam closes


# ---------------------------------------------------------------- e. refusals
def test_refusals(pkg, ctx):
    AAError = pkg.capi.AAError
    sc = dataclasses.replace(tc.pendants(iters=5, n_steps=1), springs=None)   # ties alone: the springs' refusals come first
    ia, wa, ib, wb, k, rest, mode = sc.ties[0]
    # the z-AA variant
    s = pkg.capi.solver_from_scene(ctx, sc)
    st = pkg.capi.settings_from_scene(sc)
    st.variant = pkg.capi.AA_VARIANT_Z
    with pytest.raises(AAError, match="ties exist in the \\(u,x\\) variant only") as e:
        s.initialize(st)
    assert e.value.code == -1
    s.close()
    # a partitioned solver
    comm = pkg.capi.Comm.solo(0, 2)
    s = pkg.capi.solver_from_scene(ctx, sc, comm)
    with pytest.raises(AAError, match="ties need one rank") as e:
        s.initialize(pkg.capi.settings_from_scene(sc))
    assert e.value.code == -1 and "2 ranks" in str(e.value)
    s.close()
    comm.close()
    # AA_ERR_ARG cases on one solver: a refused call touches nothing
    s = pkg.capi.solver_from_scene(ctx, sc)

    def at(a, i, j, val):
        a = np.array(a)
        a[i, j] = val
        return a

    cases = [
        (dict(nodes_a=at(ia, 1, 2, sc.n_nodes)), "tie 1.*out of range"),
        (dict(nodes_b=at(ib, 2, 0, -1)), "tie 2.*out of range"),
        (dict(nodes_b=at(ib, 0, 0, 1)), "tie 0.*node 1 twice"),
        (dict(w_a=at(wa, 1, 0, np.nan)), "tie 1.*non-finite weight"),
        (dict(w_a=at(wa, 2, 0, 0.15 + 1e-11)), "tie 2.*anchor A.*sum to 1"),
        (dict(k=[50.0, 0.0, 50.0]), "tie 1.*k must be"),
        (dict(rest=[0.3, 0.3, -1.0]), "tie 2.*rest"),
        (dict(mode=3), "unknown mode 3"),
        (dict(nodes_a=ia[:, :1], w_a=np.ones((3, 1))), "aa_elastic_add_springs"),
        (dict(nodes_a=np.tile([[0, 1, 2, 4]], (3, 1)), w_a=np.full((3, 4), 0.25), nodes_b=np.tile([[3, 5, 6]], (3, 1)),
              w_b=np.tile([[0.5, 0.25, 0.25]], (3, 1))), "na \\+ nb = 7.*not provided"),
    ]
    base = dict(nodes_a=ia, w_a=wa, nodes_b=ib, w_b=wb, k=k, rest=rest, mode=mode)
    for kw, pattern in cases:
        with pytest.raises(AAError, match=pattern) as e:
            s.add_ties(**{**base, **kw})
        assert e.value.code == -1, pattern
    # after all that the solver is the scene's, bit for bit, and add_ties after initialize is a state error
    s.initialize(pkg.capi.settings_from_scene(sc))
    n_el = s.runtime().n_elements
    assert n_el == 3
    with pytest.raises(AAError, match="after initialize") as e:
        s.add_ties(**base)
    assert e.value.code == -2
    s.set_pins(sc.pin_idx, sc.pin_pts + sc.pin_vel)
    s.step()
    assert s.runtime().n_elements == n_el
    assert np.array_equal(s.x, _run(pkg, ctx, sc)[0]["x"])
    s.close()


# ---------------------------------------------------------------- f. the closest-point query
def _open_sheet():
    V, F = scenes.tri_grid(4, 4)
    V = V.copy()
    V[:, 1] = 0.05 * np.sin(3.0 * V[:, 0]) * np.cos(2.0 * V[:, 2])   # not flat: the distances have three components
    return V, F


def _brute(V, F, Q):
    C, _ = mc.ericson(V, F, Q)
    d = np.linalg.norm(Q[:, None] - C, axis=-1)
    tri = d.argmin(1)
    i = np.arange(len(Q))
    c, dist = C[i, tri], d[i, tri]
    near = d <= dist[:, None] * (1.0 + 1e-9)
    other = np.linalg.norm(C - c[:, None], axis=-1) > 1e-9
    return c, dist, tri, near.sum(1) == 1, ~(near & other).any(1)


@pytest.mark.parametrize("name", list(mc.MESHES) + ["open_sheet"])
def test_closest_on_triangles_matches_brute_force(name, pkg, ctx):
    """aa_closest_on_triangles on 2 600 queries per mesh -- the cube, L-prism, sliver and 16 x 8 torus
    of the mesh-obstacle tests and one open sheet -- against Ericson's test on every triangle, and
    against the oracle's closest point: the distance to 1e-13 on every query, the point to 1e-13
    where no second triangle ties with another point, the triangle equal where the minimum is unique;
    the weights bitwise friction_carry_cases.barycentric on the returned triangle and point."""
    import pyoracle
    if name == "open_sheet":
        V, F = _open_sheet()
        Q = mc.queries(V, F)
    else:
        V, F, Q, _ = mc.case(name)
    c_ref, dist, tri_ref, unique, single = _brute(V, F, Q)
    c, tri, b = pkg.capi.closest_on_triangles(ctx, V, F, Q)
    d = np.linalg.norm(Q - c, axis=1)
    c_or = pyoracle.closest_point(V, F, Q)
    print(f"{name}: max ||q - c| - d| {np.abs(d - dist).max():.3e}, max |c - c_ref| {np.abs(c - c_ref)[single].max():.3e}, "
          f"oracle {np.abs(c - c_or)[single].max():.3e}, triangle mismatches {(tri != tri_ref)[unique].sum()} of {unique.sum()}")
    assert ((tri >= 0) & (tri < len(F))).all()
    assert np.abs(d - dist).max() <= CP_TOL
    assert np.abs(c - c_ref)[single].max() <= CP_TOL and np.abs(c - c_or)[single].max() <= CP_TOL
    assert np.array_equal(tri[unique], tri_ref[unique]) and unique.sum() > 100
    A, B, C = V[F[tri, 0]], V[F[tri, 1]], V[F[tri, 2]]
    want_b, den = fc.barycentric(A, B, C, c)
    assert (den > 0).all() and b.tobytes() == want_b.tobytes()
    assert np.abs(fc.interpolate(b, A, B, C) - c).max() <= CP_TOL   # the weights give the point back
    # a partial last wave, and outputs left out
    c1, t1, b1 = pkg.capi.closest_on_triangles(ctx, V, F, Q[:1000])
    assert np.array_equal(c1, c[:1000]) and np.array_equal(t1, tri[:1000]) and np.array_equal(b1, b[:1000])


def test_closest_on_triangles_refuses(pkg, ctx):
    AAError = pkg.capi.AAError
    V, F = _open_sheet()
    Q = np.zeros((3, 3))
    Vn = V.copy()
    Vn[7, 1] = np.nan
    Fi, Fz = F.copy(), F.copy()
    Fi[5, 2] = len(V)
    Fz[9] = [3, 3, 4]
    Qn = Q.copy()
    Qn[2, 0] = np.inf
    for args, pattern in [((Vn, F, Q), "vertex 7.*non-finite"), ((V, Fi, Q), "triangle 5.*out of range"),
                          ((V, Fz, Q), "triangle 9.*zero area"), ((V, F, Qn), "query 2.*non-finite"),
                          ((V, F[:0], Q), "empty")]:
        with pytest.raises(AAError, match=pattern) as e:
            pkg.capi.closest_on_triangles(ctx, *args)
        assert e.value.code == -1
    c, tri, b = pkg.capi.closest_on_triangles(ctx, V, F, Q[:0])
    assert c.shape == (0, 3) and tri.shape == (0,)


def test_ties_to_surface_on_the_patch_rim(pkg, ctx):
    """capi.ties_to_surface on patch_on_block's rim against the block's faces: na = 3, nb = 1, the
    triangles the scene builder's host query found, and a derived L (the host builder's statement)
    equal to the query's distance to 1e-13. The entry binds and runs."""
    sc = scenes.patch_on_block(floor=False, n_steps=1)
    ia, wa, ib, wb, k, rest, mode = sc.ties[0]
    faces = scenes.tet_boundary_faces(sc.x[:27], sc.groups[0].idx)
    entry = pkg.capi.ties_to_surface(ctx, sc.x, ib[:, 0], faces, k)
    assert entry[0].shape == (16, 3) and entry[2].shape == (16, 1) and entry[5] is None and entry[6] == scenes.SPRING
    c, tri, b = pkg.capi.closest_on_triangles(ctx, sc.x, faces, sc.x[ib[:, 0]])
    L = tc.ties(sc.x, *entry[:5], None)[2]
    print(f"derived L against the query's distance: {np.abs(L - np.linalg.norm(sc.x[ib[:, 0]] - c, axis=1)).max():.3e}")
    assert np.abs(L - np.linalg.norm(sc.x[ib[:, 0]] - c, axis=1)).max() <= CP_TOL
    assert np.abs(L - 0.03).max() <= CP_TOL and np.array_equal(np.sort(entry[0], 1), np.sort(ia, 1))
    out = _run(pkg, ctx, dataclasses.replace(sc, ties=[entry]))
    assert np.isfinite(out[0]["x"]).all()
