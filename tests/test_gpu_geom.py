"""GPU parity of the Geometry (ALM) HIP path (through the C ABI) against the reference's golden
vectors and the oracle. Tolerances (written here): combined-residual curves
judged relative to comb_0 -- 1e-8 over the first 40 accepted iterations and 1e-6 over the whole
curve (Anderson trajectories amplify rounding differences; the oracle meets the same bounds
against the reference); solutions 1e-8 relative; closest points 1e-13 absolute."""
import os
import re
import sys

import numpy as np
import pytest

from golden_io import GOLDEN, compare_geom, geom_case_names, load_geom_case, load_npz

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", geom_case_names())
def test_gpu_geom_matches_reference_golden(name, pkg, ctx):
    sc, ref = load_geom_case(name)
    got, g = pkg.capi.run_geom(ctx, sc)
    fails = compare_geom(ref, got, 1e-8, 1e-8, n_check=40) + compare_geom(ref, got, 1e-6, 1e-6)
    assert not fails, fails
    rt = g.runtime()
    assert rt.accepted == sc.iters
    if sc.solver == "alm":   # GeometrySolver records every iteration (a reset swaps, it does not repeat)
        assert rt.iterations == rt.accepted + rt.rejects
    assert np.all(np.diff(got["time_s"]) >= 0)
    g.close()


def test_gpu_geom_element_tables(pkg, ctx):
    """The device projections (plane k = 3..8 by one-sided Jacobi in registers, the closed-form
    angle rotation, edge normalisation) on the reference's own element table
    (geom_elements.npz, made by oracle/_ref/ref_geom_element from Constraint.h:194-414), at the
    oracle's tolerances."""
    gs = pkg.geom_scenes
    d = np.load(os.path.join(GOLDEN, "geom_elements.npz"))
    for k in (3, 4, 5, 6, 8):
        X, Y = d[f"plane{k}_in"], d[f"plane{k}_out"]
        got = pkg.capi.hook_geom_project(ctx, gs.PLANE, k, None, X.reshape(len(X), k, 3))
        np.testing.assert_allclose(got.reshape(Y.shape), Y, rtol=0, atol=1e-12 * max(1.0, np.abs(X).max()))
    for name, ctype, k, atol in (("angle", gs.ANGLE, 3, 1e-12), ("edge", gs.EDGE, 2, 1e-14)):
        X, Y, P = d[name + "_in"], d[name + "_out"], d[name + "_prm"]
        for x, y, p in zip(X, Y, P):
            got = pkg.capi.hook_geom_project(ctx, ctype, k, p, x.reshape(1, k - 1, 3))
            np.testing.assert_allclose(got.reshape(y.shape), y, rtol=0, atol=atol)


def test_gpu_geom_full_size_c5(pkg, ctx):
    """BASELINE configs[4] at full size (707 x 707 wire mesh: 501 264 points, ~1 M edge-length and
    ~1 M angle constraints + the reference-surface constraint, m = 20) against the reference's own
    run of the same scene (tests/golden/full_c5_wire707.npz, make_golden_geom.py --full-c5; 10
    accepted iterations): the residual curve relative to comb_0 (1e-8) and 512 sampled solution
    points plus the column sums (1e-8 of the coordinate scale)."""
    gs = pkg.geom_scenes
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_geom import scene_digest
    ref = np.load(os.path.join(GOLDEN, "full_c5_wire707.npz"))
    sc = gs.wire_grid(707, 707, iters=10, aa_m=20)
    assert np.array_equal(scene_digest(sc), ref["digest"]), "regenerated scene differs from the fixture's"
    got, g = pkg.capi.run_geom(ctx, sc)
    rt = g.runtime()
    assert rt.n_points == 501264 and rt.accepted == 10
    c, rc = got["comb"], ref["comb"]
    assert len(c) == len(rc) == 10 and np.all(np.isfinite(c))
    assert np.abs(c - rc).max() <= 1e-8 * rc[0], np.abs(c - rc).max() / rc[0]
    x = got["x"]
    scale = np.abs(ref["x_sample"]).max()
    assert np.abs(x[ref["sample"]] - ref["x_sample"]).max() <= 1e-8 * scale
    assert np.allclose(x.sum(0), ref["x_sum"], rtol=1e-8, atol=1e-8 * scale * len(x))
    g.close()


def test_gpu_closest_points_match_reference(pkg, ctx):
    d = np.load(os.path.join(GOLDEN, "geom_elements.npz"))
    g = pkg.capi.GeomSolver(ctx)
    sid = g.add_ref_surface(d["closest_V"], d["closest_F"])
    got = g.closest_points(sid, d["closest_in"])
    np.testing.assert_allclose(got, d["closest_out"], rtol=0, atol=1e-13)
    g.close()


@pytest.mark.parametrize("builder", [
    lambda gs: gs.pq_heightfield(40, 40, iters=60, aa_m=10),
    lambda gs: gs.wire_grid(40, 40, iters=60, aa_m=20),
    lambda gs: gs.pq_heightfield(30, 30, iters=40, aa_m=0),
])
def test_gpu_geom_matches_oracle(builder, pkg, ctx, oracle):
    sc = builder(pkg.geom_scenes)
    want = oracle.run_geom(sc)
    got, g = pkg.capi.run_geom(ctx, sc)
    fails = compare_geom(want, got, 1e-8, 1e-8, n_check=40) + compare_geom(want, got, 1e-6, 1e-6)
    assert not fails, fails
    g.close()


def _closest_brute(V, F, P, chunk=256):
    """Exact squared distance from each point of P to the triangle set (V, F): numpy restatement
    of the point-triangle test (Ericson's regions) over every triangle; test infrastructure."""
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    out = np.empty(len(P))
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        ab, ac, ap = B - A, C - A, p - A
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        bp = p - B
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        cp = p - C
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        with np.errstate(divide="ignore", invalid="ignore"):
            den = 1.0 / (va + vb + vc)
            q = A + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
            v_ab = d1 / (d1 - d3)
            w_ac = d2 / (d2 - d6)
            w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        regions = [
            ((d1 <= 0) & (d2 <= 0), A + 0 * p),
            ((d3 >= 0) & (d4 <= d3), B + 0 * p),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), A + ab * v_ab[..., None]),
            ((d6 >= 0) & (d5 <= d6), C + 0 * p),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), A + ac * w_ac[..., None]),
            ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), B + (C - B) * w_bc[..., None]),
        ]
        done = np.zeros(d1.shape, bool)
        for m, qq in regions:
            sel = m & ~done
            q = np.where(sel[..., None], qq, q)
            done |= sel
        out[s:s + chunk] = ((p - q) ** 2).sum(-1).min(1)
    return out


@pytest.mark.parametrize("group", ["0", "4"])
def test_gpu_closest_points_brute_force(group, pkg, ctx, monkeypatch):
    """The BVH walk's node bounds (AABB, oriented box in fp32 with slack, fp64 descent) never prune
    the closest triangle: GPU closest-point distances equal a brute-force minimum over every
    triangle (1e-10 relative, 1e-13 of the surface's span absolute) on a smooth height field, a
    sheared one, a random triangle soup (intersecting slivers) and two stacked layers, for points
    on, near and far from the surface, with one lane and with four lanes per query."""
    monkeypatch.setenv("AA_CP_GROUP", group)
    rng = np.random.default_rng(11)
    surfs = []
    gs = pkg.geom_scenes
    surfs.append(gs.field_trimesh(40, 40))
    surfs.append(gs.field_trimesh(30, 50, shear=1.2))
    Vs = rng.uniform(-1, 1, (900, 3))
    surfs.append((Vs, rng.integers(0, 900, (1500, 3)).astype(np.int32)))
    V2, F2 = gs.field_trimesh(25, 25)
    V3 = np.concatenate([V2, V2 + [0.0, 0.0, 0.02]])
    surfs.append((V3, np.concatenate([F2, F2 + len(V2)]).astype(np.int32)))
    for V, F in surfs:
        V = np.asarray(V, np.float64); F = np.asarray(F, np.int32)
        F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]
        lo, hi = V.min(0), V.max(0)
        span = (hi - lo).max()
        P = np.concatenate([rng.uniform(lo - 0.3 * span, hi + 0.3 * span, (600, 3)),
                            V[rng.integers(0, len(V), 600)] + rng.normal(0, 0.01 * span, (600, 3)),
                            V[rng.integers(0, len(V), 200)]])
        g = pkg.capi.GeomSolver(ctx)
        sid = g.add_ref_surface(V, F)
        q = g.closest_points(sid, P)
        g.close()
        d_gpu = ((P - q) ** 2).sum(1)
        d_ref = _closest_brute(V, F, P)
        # distances, not their squares: a point on the surface has |p - q| ~ 1e-4 and its square
        # carries the rounding of p - q (~1e-16 |p|) relative to a tiny value
        np.testing.assert_allclose(np.sqrt(d_gpu), np.sqrt(d_ref), rtol=1e-10, atol=1e-13 * span)


@pytest.mark.parametrize("group", ["4", "8"])
def test_gpu_closest_point_group_traversal_bit_identical(group, pkg, ctx, monkeypatch):
    """The group traversal (AA_CP_GROUP lanes per query over the collapsed tree, read when a
    reference surface is added) returns bvh_closest's triangle and point bit for bit: its tie
    rule restates the depth-first first-found order. Closest points of the reference's own test
    surface and whole PQ / wire solves (their warm-started queries) against one lane per query."""
    d = np.load(os.path.join(GOLDEN, "geom_elements.npz"))
    scenes = [pkg.geom_scenes.pq_heightfield(48, 48, iters=40, aa_m=10, noise=0.3),
              pkg.geom_scenes.wire_grid(32, 32, iters=40, aa_m=20)]
    out = {}
    for g_ in ("0", group):
        monkeypatch.setenv("AA_CP_GROUP", g_)
        g = pkg.capi.GeomSolver(ctx)
        sid = g.add_ref_surface(d["closest_V"], d["closest_F"])
        rng = np.random.default_rng(5)
        P = d["closest_in"]
        P = np.concatenate([P, P[rng.integers(0, len(P), 4000)] + rng.normal(0, 0.05, (4000, 3))])
        out[g_] = [g.closest_points(sid, P)]
        g.close()
        for sc in scenes:
            got, gs = pkg.capi.run_geom(ctx, sc)
            out[g_] += [got["comb"], got["x"]]
            gs.close()
    for a, b in zip(out["0"], out[group]):
        assert np.array_equal(a, b)


def test_gpu_geom_deterministic(pkg, ctx):
    sc = pkg.geom_scenes.wire_grid(24, 24, iters=30, aa_m=6)
    a, ga = pkg.capi.run_geom(ctx, sc)
    b, gb = pkg.capi.run_geom(ctx, sc)
    assert np.array_equal(a["comb"], b["comb"]) and np.array_equal(a["x"], b["x"])
    # a second solve on the same solver (factor reused) reproduces the first
    ga.solve(sc.x0, 1e-8, sc.iters, sc.aa_m)
    assert np.array_equal(ga.history()["comb"], a["comb"])
    ga.close(); gb.close()


def test_gpu_geom_full_size_c3(pkg, ctx):
    """BASELINE configs[2] at full size (317 x 317 quads = 100 489 planarity constraints, 101 124
    points scattered 0.3 h off the surface, m = 10) against the reference's own run of the same
    scene (tests/golden/full_c3_pq317.npz, make_golden_geom.py --full): the residual curve
    relative to comb_0 (1e-8 over the first 40 iterations, 1e-6 over all 100), the solution on
    256 sampled points and its column sums (1e-6 of the coordinate scale), and the faces ending
    flatter than they started."""
    gs = pkg.geom_scenes
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_geom import scene_digest
    ref = np.load(os.path.join(GOLDEN, "full_c3_pq317.npz"))
    sc = gs.pq_heightfield(317, 317, iters=100, aa_m=10, noise=0.3)
    assert np.array_equal(scene_digest(sc), ref["digest"]), "regenerated scene differs from the fixture's"
    got, g = pkg.capi.run_geom(ctx, sc)
    rt = g.runtime()
    assert rt.n_points == 101124 and rt.hard_cols == 4 * 100489 and rt.accepted == 100
    c, rc = got["comb"], ref["comb"]
    assert len(c) == len(rc) == 100 and np.all(np.isfinite(c))
    assert np.abs(c[:40] - rc[:40]).max() <= 1e-8 * rc[0]
    assert np.abs(c - rc).max() <= 1e-6 * rc[0]
    x = got["x"]
    scale = np.abs(ref["x_sample"]).max()
    assert np.abs(x[ref["sample"]] - ref["x_sample"]).max() <= 1e-6 * scale
    assert np.allclose(x.sum(0), ref["x_sum"], rtol=1e-6, atol=1e-6 * scale * len(x))

    def planarity(X):
        Q = sc.groups[1].idx
        P = X[Q] - X[Q].mean(1, keepdims=True)
        n = np.linalg.svd(P, full_matrices=True)[2][:, 2, :]
        return np.abs(np.einsum("fkd,fd->fk", P, n)).max() / sc.avg_edge_length()

    assert planarity(x) < 0.5 * planarity(sc.x0)
    g.close()


def test_gpu_geom_error_behaviour(pkg, ctx):
    capi = pkg.capi
    g = capi.GeomSolver(ctx)
    with pytest.raises(capi.AAError) as e:             # solve before setup ("solver not initialized")
        g.solve(np.zeros((4, 3)), 1e-8, 10, 0)
    assert e.value.code == -2
    with pytest.raises(capi.AAError):                  # a plane needs at least 3 points (any valence above)
        g.add_constraints(True, capi.AA_CON_PLANE, np.arange(2)[None], 1.0)
    with pytest.raises(capi.AAError):                  # angle constraints take exactly 3 indices
        g.add_constraints(True, capi.AA_CON_ANGLE, np.arange(4)[None], 1.0, np.array([[0.5, 2.0]]))
    with pytest.raises(capi.AAError):                  # unknown reference surface
        g.add_constraints(False, capi.AA_CON_POINT_TO_REF, np.array([0]), 1.0, np.array([[3.0]]))
    g.add_constraints(True, capi.AA_CON_EDGE, np.array([[0, 1]]), 1.0, np.array([[1.0]]))
    with pytest.raises(capi.AAError) as e:             # point 2 has no constraint: not SPD
        g.setup(3, 10.0)
    assert e.value.code == -4
    g.close()



def test_gpu_geom_run_to_eps_stop(pkg, ctx):
    """aa_geom_set_stop: the run-to-epsilon mode of the bench's geometry leg. The reference
    computes residual_eps = rel_eps^2 cols^2 2 (ALMGeometrySolver.h:172) but its test is commented
    out (:258-260); enabled here it ends the loop after the first accepted iteration below it. The
    stopped run is a bit-identical prefix of the uncapped run; a raised cap on the same solver
    (history re-allocated, captured chunk dropped) is the round-3 regression case."""
    sc = pkg.geom_scenes.pq_heightfield(20, 20, iters=60, aa_m=6, noise=0.3)
    full, g = pkg.capi.run_geom(ctx, sc)
    c = full["comb"]
    assert len(c) == 60
    cols = g.runtime().hard_cols
    # relative level: comb <= r comb_0
    r = c[20] / c[0] * (1 + 1e-9)
    k = int(np.nonzero(c <= r * c[0])[0][0])
    g.set_stop(False, r)
    g.solve(sc.x0, 1e-8, 500, sc.aa_m)
    h = g.history()["comb"]
    assert len(h) == k + 1 and np.array_equal(h, c[:k + 1])
    # the reference's absolute residual_eps
    thr = c[30] * (1 + 1e-9)
    j = int(np.nonzero(c < thr)[0][0])
    g.set_stop(True, 0.0)
    g.solve(sc.x0, np.sqrt(thr / 2.0) / cols, 500, sc.aa_m)
    h = g.history()["comb"]
    assert len(h) == j + 1 and np.array_equal(h, c[:j + 1])
    assert g.runtime().accepted == j + 1
    # stop off again: the reference loop, max_iter accepted iterations
    g.set_stop(False, 0.0)
    g.solve(sc.x0, 1e-8, 60, sc.aa_m)
    assert np.array_equal(g.history()["comb"], c)
    assert np.array_equal(g.solution(), full["x"])
    with pytest.raises(Exception):
        g.set_stop(False, -1.0)
    g.close()


def test_gpu_c5_eps_regime_matches_reference(pkg, ctx):
    """C5's run-to-epsilon regime pinned to the reference: the wire-mesh recipe
    (edge-length + angle + reference-surface closeness, ALM, Anderson m = 20) on a 150 x 150 grid,
    2 000 accepted iterations without a stop (the reference's own stop is commented out,
    ALMGeometrySolver.h:258-260), against the reference's curve (tests/golden/eps_wire150_ref.npz,
    tools/ref_geom_curve.py, oracle/_ref/ref_geom from Geometry/WireMeshOpt.cpp:233-337's solver).
    Neither reaches residual_eps (ALMGeometrySolver.h:172): both level off near 460 eps. The curve
    must match to 1e-8 comb_0 over 200 iterations and 1e-5 comb_0 over all 2 000, and the floor
    min(comb) to within 10 %."""
    ref = np.load(os.path.join(GOLDEN, "eps_wire150_ref.npz"))
    want = ref["comb"]
    sc = pkg.geom_scenes.wire_grid(150, 150, iters=len(want), aa_m=20)
    got, g = pkg.capi.run_geom(ctx, sc)
    c = np.asarray(got["comb"])
    assert len(c) == len(want)
    err = np.abs(c - want) / want[0]
    assert err[:200].max() <= 1e-8, err[:200].max()
    assert err.max() <= 1e-5, err.max()
    assert abs(c.min() / want.min() - 1.0) <= 0.1, (c.min(), want.min())
    assert c.min() > float(ref["eps_abs"]) and want.min() > float(ref["eps_abs"])
    g.close()


@pytest.mark.parametrize("min_sub", ["64", "16"])
def test_gpu_geom_fused_subtrees_lds_vectors_bit_identical(pkg, ctx, monkeypatch, capfd, min_sub):
    """The geometry solver's fused subtrees with their update vectors and boundary x rows in LDS
    (DirectSolver kSubU / kSubX) against HBM (AA_SUB_LDS_U=0 / AA_SUB_LDS_X=0): bit-identical
    ALM trajectories; few subtrees make them tall (many levels, most update vectors inside)."""
    sc = pkg.geom_scenes.pq_heightfield(160, 150, iters=60, aa_m=10, noise=0.3)
    monkeypatch.setenv("AA_SOLVE_MIN_SUBTREES", min_sub)
    monkeypatch.setenv("AA_SOLVE_STATS", "1")
    runs = []
    for on in ("0", "1"):
        monkeypatch.setenv("AA_SUB_LDS_U", on)
        monkeypatch.setenv("AA_SUB_LDS_X", on)
        capfd.readouterr()
        h, g = pkg.capi.run_geom(ctx, sc)
        err = capfd.readouterr().err
        runs.append((h, g.runtime().rejects))
        g.close()
    m = re.search(r"fused subtrees in LDS: update vectors (\d+) / (\d+) .* x rows (\d+) / (\d+)", err)
    assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, err[-2000:]
    (a, ra), (b, rb) = runs
    assert np.array_equal(a["comb"], b["comb"]) and np.array_equal(a["x"], b["x"]) and ra == rb


def test_gpu_c3_eps_regime_matches_reference(pkg, ctx):
    """C3's run-to-epsilon pinned to the reference past the crossing: the full
    PQ 317 x 317 scene (m = 10), 1 500 accepted iterations without a stop, against the reference's
    curves (tests/golden/eps_pq317_ref.npz, tools/ref_geom_curve.py -> tools/eps_fixture.py,
    oracle/_ref/ref_geom from ALMGeometrySolver.h:163-283). Up to iteration 1 068 the curves
    agree to 1e-9 comb_0; there the ALM/Anderson loop branches on rounding-level differences: the
    reference itself, started from positions perturbed by 1e-13 relative, takes the branch that
    crosses residual_eps (ALMGeometrySolver.h:172) at iteration 1 145, unperturbed (and at 1e-15 /
    1e-12) the one that crosses at 1 332. The GPU must follow one of the reference's two branches
    (1e-3 relative after iteration 1 068, the branches themselves differ by up to 17 %), cross 1e-8
    comb_0 within +-3 iterations of the reference and eps_abs within +-5 of its branch, and reach
    that branch's floor within 10 %."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_geom import scene_digest
    ref = np.load(os.path.join(GOLDEN, "eps_pq317_ref.npz"))
    branches = [ref["comb"], ref["comb_alt"]]
    eps = float(ref["eps_abs"])
    sc = pkg.geom_scenes.pq_heightfield(317, 317, iters=len(branches[0]), aa_m=10, noise=0.3)
    assert np.array_equal(scene_digest(sc), ref["digest"]), "regenerated scene differs from the fixture's"
    got, g = pkg.capi.run_geom(ctx, sc)
    g.close()
    c = np.asarray(got["comb"])
    want = branches[0]
    assert len(c) == len(want)
    assert (np.abs(c - want) / want[0])[:1000].max() <= 1e-9
    first = lambda x, thr: int(np.nonzero(x <= thr)[0][0]) + 1
    assert abs(first(c, 1e-8 * want[0]) - first(want, 1e-8 * want[0])) <= 3
    dev = [(np.abs(c - b) / b)[1068:].max() for b in branches]
    k = int(np.argmin(dev))
    assert dev[k] <= 1e-3, dev
    b = branches[k]
    assert (c < eps).any() and (b < eps).any()
    assert abs(first(c, eps * (1 - 1e-15)) - first(b, eps * (1 - 1e-15))) <= 5
    assert abs(c.min() / b.min() - 1.0) <= 0.1


@pytest.mark.parametrize("case,key", [("geom_airport3k_aa10", "pq_airport3k"), ("geom_costa2k_wire_aa5", "wire_costa2k")])
def test_gpu_quality_reports_match_reference_apps(case, key, pkg, ctx, tmp_path):
    """The applications' before/after report files (geom_report; PlanarityOpt.cpp:263-275,
    WireMeshOpt.cpp:306-325) from the GPU solution, with the distances to the reference surface
    taken by the solver's own closest-point BVH: the reference app's values
    (tests/golden/quality_reports.npz) within 1e-4 of each file's largest value (the solution's
    parity bar is 1e-6; corner angles of short edges amplify it)."""
    import io
    gr = pkg.geom_report
    q = load_npz(os.path.join(GOLDEN, "quality_reports.npz"))
    d = load_npz(os.path.join(GOLDEN, case + ".npz"))
    sc, ref = load_geom_case(case)
    got, g = pkg.capi.run_geom(ctx, sc)
    closest = lambda P: g.closest_points(0, P)   # noqa: E731
    buf = io.StringIO()
    if key == "pq_airport3k":
        sizes, idx = q[key + "__face_sizes"], q[key + "__face_idx"]
        faces = np.split(idx, np.cumsum(sizes)[:-1])
        gr.planarity_report(d["x0"], got["x"], [list(map(int, f)) for f in faces], d["s0_V"], d["s0_F"],
                            result_dir=str(tmp_path), closest=closest, out=buf)
        names = ["planarityErrBefore", "planatityErrAfter"]
    else:
        faces = d["g1_idx"].reshape(-1, 4, 3)[:, :, 0].tolist()
        gr.wiremesh_report(d["x0"], got["x"], faces, d["s0_V"], d["s0_F"], float(d["g2_params"][0, 0]),
                           result_dir=str(tmp_path), closest=closest, out=buf)
        names = [f"{t}_wiremeshErr{w}" for t in ("edge", "angle", "ref") for w in ("Before", "After")]
    g.close()
    for name in names:
        want = q[f"{key}__{name}"]
        have = np.loadtxt(os.path.join(tmp_path, name + ".txt"))
        tol = (1e-10 if name.endswith("Before") else 1e-4) * np.abs(want).max()
        assert np.abs(have - want).max() <= tol, (name, np.abs(have - want).max() / np.abs(want).max())
    num = lambda ln: [float(t) for t in re.findall(r"[-+]?\d+(?:\.\d*)?(?:e[-+]?\d+)?", ln.split(":", 1)[-1])]  # noqa: E731
    for a, b in zip(buf.getvalue().splitlines(), q[key + "__stdout"]):
        assert a.split(":")[0] == b.split(":")[0]
        np.testing.assert_allclose(num(a), num(b), rtol=1e-4, atol=1e-12)


@pytest.mark.parametrize("builder", [lambda gs: gs.pq_heightfield(90, 90, iters=40, aa_m=10),
                                     lambda gs: gs.wire_grid(90, 90, iters=40, aa_m=20)])
def test_gpu_geom_solve_branches_bit_identical(builder, pkg, ctx, monkeypatch):
    """Geometry: the global solve as parallel branches (AA_SOLVE_BRANCHES=2 / 4) is bit-identical
    to the single-stream sweep (the same tasks, tiles and sums)."""
    sc = builder(pkg.geom_scenes)
    monkeypatch.setenv("AA_SOLVE_BRANCHES", "1")
    want, g = pkg.capi.run_geom(ctx, sc)
    g.close()
    for b in ("2", "4"):
        monkeypatch.setenv("AA_SOLVE_BRANCHES", b)
        got, g = pkg.capi.run_geom(ctx, sc)
        g.close()
        assert np.array_equal(got["comb"], want["comb"]) and np.array_equal(got["x"], want["x"]), b
