"""CPU tests of the tie term (aa_elastic_add_ties): the host builder (csrc/ties.hpp) in a stand-alone
program against the numpy restatement with every refusal; the numpy port with tie rows
(tests/tie_cases.py) against two closed forms and a dense minimiser; and the conditioning and margin
conditions of every trajectory scene the GPU tests use."""
import os
import subprocess

import numpy as np
import pytest

import spring_cases as sp
import tie_cases as tc
from conftest import REPO
from golden_io import scenes

CSRC = os.path.join(REPO, "aa-admm_amd", "csrc")
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------- host builder
def _write_case(f, name, V, ia, wa, ib, wb, mode, k, rest, flags):
    wa, wb = np.asarray(wa, np.float64), np.asarray(wb, np.float64)
    n, na, nb = wa.shape[0], wa.shape[1], wb.shape[1]
    nums = lambda a: " ".join(repr(float(c)) for c in np.asarray(a, np.float64).reshape(-1)) + "\n"
    ints = lambda a: " ".join(str(int(c)) for c in np.asarray(a).reshape(-1)) + "\n"
    f.write(f"{name} {len(V)} {n} {na} {nb} {mode} {flags}\n")
    f.write(nums(V) + ints(ia) + nums(wa) + ints(ib) + nums(wb))
    f.write(nums(np.broadcast_to(k, (n,))) + nums(np.zeros(n) if rest is None else np.broadcast_to(rest, (n,))))


def _good():
    rng = np.random.default_rng(3)
    V = rng.normal(size=(12, 3))
    out = {}
    for na, nb in [(1, 2), (2, 1), (2, 2), (3, 1), (1, 3), (1, 4), (4, 1), (3, 2), (2, 3), (3, 3), (4, 2), (2, 4)]:
        n = 5
        idx = np.array([rng.choice(12, na + nb, False) for _ in range(n)])
        wa, wb = rng.dirichlet(np.full(na, 2.0), n), rng.dirichlet(np.full(nb, 2.0), n)
        k = 10.0 ** rng.uniform(-1, 3, size=n)
        out[f"derived_{na}{nb}"] = (V, idx[:, :na], wa, idx[:, na:], wb, 0, k, None, 1)
        out[f"given_{na}{nb}"] = (V, idx[:, :na], wa, idx[:, na:], wb, 5, k, rng.uniform(0, 1, n), 2)
    # weights outside [0, 1], a zero weight, a sum off by less than 1e-12: used as given
    wa = np.array([[1.5, -0.5, 0.0], [0.0, 1.0, 0.0], [0.25, 0.5, 0.25 + 5e-13]])
    out["extrapolated"] = (V, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], wa, [[9], [10], [11]], np.ones((3, 1)), 6, 2.0, None, 1)
    out["empty"] = (V, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 1)), np.zeros((0, 1)), 1, 2.0, None, 0)
    return out


def _refused():
    """name -> (case..., words the message must contain); all AA_ERR_ARG (-1)"""
    V = np.random.default_rng(4).normal(size=(10, 3))
    ia = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]])
    ib = np.array([[6], [7], [8], [9]])
    wa, wb = np.tile([[0.2, 0.3, 0.5]], (4, 1)), np.ones((4, 1))
    k, rest = np.full(4, 2.0), np.full(4, 0.4)
    bad = lambda i, val, arr: np.concatenate([arr[:i], [val], arr[i + 1:]])

    def at(a, i, j, val):
        a = np.array(a, np.float64 if np.asarray(a).dtype.kind == "f" else np.int64)
        a[i, j] = val
        return a

    two = (V, ia[:, :1], wb, ib, wb, 0, k, None, 1)
    return {
        "index_high": (V, at(ia, 2, 1, 10), wa, ib, wb, 0, k, None, 1, ("tie 2", "out of range")),
        "index_negative": (V, ia, wa, at(ib, 1, 0, -1), wb, 0, k, None, 1, ("tie 1", "out of range")),
        "twice_within": (V, at(ia, 3, 2, 3), wa, ib, wb, 0, k, None, 1, ("tie 3", "node 3 twice")),
        "twice_across": (V, ia, wa, at(ib, 0, 0, 1), wb, 0, k, None, 1, ("tie 0", "node 1 twice")),
        "weight_nan": (V, ia, at(wa, 1, 0, np.nan), ib, wb, 0, k, None, 1, ("tie 1", "non-finite weight")),
        "weight_inf": (V, ia, wa, ib, at(wb, 2, 0, np.inf), 0, k, None, 1, ("tie 2", "non-finite weight")),
        "sum_a": (V, ia, at(wa, 2, 1, 0.3 + 2e-12), ib, wb, 0, k, None, 1, ("tie 2", "anchor A", "sum to 1")),
        "sum_b": (V, ia, wa, ib, at(wb, 3, 0, 1.0 - 2e-12), 0, k, None, 1, ("tie 3", "anchor B", "sum to 1")),
        "k_zero": (V, ia, wa, ib, wb, 0, bad(2, 0.0, k), None, 1, ("tie 2", "k must be")),
        "k_negative": (V, ia, wa, ib, wb, 1, bad(3, -1.0, k), None, 1, ("tie 3", "k must be")),
        "k_nan": (V, ia, wa, ib, wb, 2, bad(0, np.nan, k), None, 1, ("tie 0", "k must be")),
        "k_inf": (V, ia, wa, ib, wb, 4, bad(1, np.inf, k), None, 1, ("tie 1", "k must be")),
        "rest_negative": (V, ia, wa, ib, wb, 0, k, bad(1, -0.1, rest), 3, ("tie 1", "rest")),
        "rest_nan": (V, ia, wa, ib, wb, 5, k, bad(2, np.nan, rest), 3, ("tie 2", "rest")),
        "rest_inf": (V, ia, wa, ib, wb, 6, k, bad(3, np.inf, rest), 3, ("tie 3", "rest")),
        "mode_3": (V, ia, wa, ib, wb, 3, k, None, 1, ("unknown mode 3",)),
        "mode_7": (V, ia, wa, ib, wb, 7, k, None, 1, ("unknown mode 7",)),
        "mode_negative": (V, ia, wa, ib, wb, -1, k, None, 1, ("unknown mode -1",)),
        "two_nodes": two + (("aa_elastic_add_springs",),),
        "seven_nodes": (V, np.tile([[0, 1, 2]], (4, 1)), wa, np.tile([[3, 4, 5, 6]], (4, 1)), np.full((4, 4), 0.25), 0, k, None, 1,
                        ("na + nb = 7", "not provided")),
        "eight_nodes": (V, np.tile([[0, 1, 2, 7]], (4, 1)), np.full((4, 4), 0.25), np.tile([[3, 4, 5, 6]], (4, 1)), np.full((4, 4), 0.25),
                        0, k, None, 1, ("na + nb = 8", "not provided")),
        "five_in_anchor": (V, np.tile([[0, 1, 2, 7, 8]], (4, 1)), np.full((4, 5), 0.2), ib, wb, 0, k, None, 1, ("1 to 4 nodes",)),
        "null_nodes": (V, ia, wa, ib, wb, 0, k, None, 1 | 4, ("null",)),
        "null_k": (V, ia, wa, ib, wb, 0, k, None, 1 | 8, ("null",)),
        "null_weights": (V, ia, wa, ib, wb, 0, k, None, 1 | 16, ("null",)),
        "no_rest_no_verts": (V, ia, wa, ib, wb, 0, k, None, 0, ("rest == NULL", "verts3")),
    }


def test_host_builder_matches_numpy_and_refuses(tmp_path):
    """tests/cpp/ties.cpp against tie_cases.ties for every (na, nb) with 3 <= na + nb <= 6: idx equal,
    G = (-a, +b) bitwise (the weights as given, not renormalised -- weights outside [0, 1], a zero
    weight and a sum 5e-13 off included), L and w bitwise for given and derived L (the anchors summed
    left to right from their first term); every refusal with its code and its tie named."""
    good, refused = _good(), _refused()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for name, c in good.items():
            _write_case(f, name, *c)
        for name, c in refused.items():
            _write_case(f, name, *c[:9])
    exe = str(tmp_path / "ties")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "ties.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and f"ok {len(good) + len(refused)} cases" in r.stdout, r.stdout[-2000:] + r.stderr
    got, errors, cur, nvs = {}, {}, None, {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "set":
            cur = got.setdefault(t[1], [])
            nvs[t[1]] = int(t[3])
        elif t[0] == "t":
            cur.append(t[1:])
        elif t[0] == "error":
            errors[t[1]] = (int(t[2]), line)
    assert not (set(errors) & set(good)), errors
    for name, (V, ia, wa, ib, wb, mode, k, rest, flags) in good.items():
        idx, G, L, w = tc.ties(V, ia, wa, ib, wb, k, rest)
        assert len(got[name]) == len(idx)
        if not len(idx):
            continue
        nv = idx.shape[1]
        assert nvs[name] == nv
        have_i = np.array([[int(a) for a in row[:nv]] for row in got[name]])
        have = np.array([[float(a) for a in row[nv:]] for row in got[name]])
        assert np.array_equal(have_i, idx)
        assert have[:, :nv].tobytes() == G.tobytes()
        assert np.array_equal(G, np.concatenate([-np.asarray(wa, np.float64), np.asarray(wb, np.float64)], 1))
        assert np.array_equal(have[:, nv], L), (name, np.abs(have[:, nv] - L).max())
        assert np.array_equal(have[:, nv + 1], w), name
        if rest is None:
            assert (L > 0).all()
    for name, c in refused.items():
        assert name in errors, (name, r.stdout[-500:])
        assert errors[name][0] == -1 and all(word in errors[name][1] for word in c[9]), errors[name]


# ---------------------------------------------------------------- the port
def test_tie_problem_rows():
    """TieProblem: one row per tie after the spring rows, (-a, +b) on its nodes, summing to zero (an
    internal force); sqrt(k) appended to w; one spring group per Scene.ties entry."""
    sc = tc.skew_edges()
    base = sp.SpringProblem(sc)
    P = tc.TieProblem(sc)
    assert P.D.shape[0] == base.D.shape[0] + 2 and np.array_equal(P.D[:-2], base.D)
    assert np.array_equal(P.D[-2], [-0.35, -0.65, 0, 1, 0, 0]) and np.array_equal(P.D[-1], [0, -0.7, -0.3, 0, 0.4, 0.6])
    assert np.abs(P.D[-2:].sum(1)).max() <= EPS
    assert np.array_equal(P.w[-2:], np.sqrt([50.0, 50.0])) and len(P.spring_groups) == len(base.spring_groups) + 2
    rows, L, mode = P.spring_groups[-1]
    assert list(rows) == [P.D.shape[0] - 1] and L[0] == 0.3 and mode == tc.SPRING
    # without ties the port is the springs' port bit for bit
    net = sp.net5(n_steps=1)
    a, b = sp.admm_ux(net), tc.admm_ux(net)
    assert all(a[0][key].tobytes() == b[0][key].tobytes() for key in a[0])


def test_port_hangs_a_mass_from_a_point_of_a_triangle():
    """One mass hung by a soft tie from the point (0.2, 0.3, 0.5) of the pinned, standing T, 60 steps:
    extension - m g / k measured 1.3e-11, sideways drift 4e-15; 1e-10 of the tie's length is asked, as
    of the hanging spring."""
    sc = tc.hanging_mass_scene()
    out = tc.admm_ux(sc)
    err, drift = tc.hanging_mass_error(out, sc)
    print(f"port: |extension - m g / k| {err:.3e}, drift {drift:.3e}")
    assert err <= 1e-10 * 0.5 and drift <= 1e-10 * 0.5
    assert np.abs(out[-1]["v"]).max() <= 1e-8


def test_port_conserves_momentum_across_a_tie():
    """Two free triangles joined by one triangle-triangle tie, no gravity: |sum m v|inf / sum m |v| at
    every step. Measured 1.1e-13 (the bar: 1e-10, far below the 1e-9 the GPU is held to), and the
    triangles do move."""
    sc = tc.two_triangles_scene()
    out = tc.admm_ux(sc)
    r = tc.momentum_ratio(out, sc)
    print(f"port: momentum ratio {r:.3e}")
    assert r <= 1e-10
    assert np.abs(out[-1]["v"]).max() > 1e-3


def test_port_reaches_the_dense_minimiser_of_zero_length_ties():
    """Zero-length soft ties only (quadratic): the port's first step against the dense solve, the
    stitches' bar 1e-10 max|x*|. Measured 2.0e-12 against a displacement of 6.8e-2."""
    sc = tc.zero_length_panels()
    xstar, move = tc.dense_minimiser(sc)
    err = np.abs(tc.admm_ux(sc)[0]["x"] - xstar).max()
    print(f"port: |x - x*|inf {err:.3e}, displacement {move:.3e}")
    assert move > 1e-3 and err <= 1e-10 * np.abs(xstar).max()


# ---------------------------------------------------------------- conditioning
@pytest.mark.parametrize("name", list(tc.TRAJ))
def test_trajectory_scenes_are_well_conditioned(name):
    """Every trajectory scene of the GPU tests: with each initial coordinate moved by one ulp up or
    down (default_rng(7)) the port's own curves move by at most a quarter of the GPU test's bar -- comb
    2.5e-10 comb_0, prim 2.5e-9 prim_0, final x and v 2.5e-10 relative -- with equal record counts and
    equal reject flags over the first 20 iterations. One-sided scenes keep min |n - L| / max(L, n) >=
    1e-6 over every prox evaluation and see active and slack ties together. Measured: worst comb
    1.8e-11 (skew_edges), worst prim 9.4e-11 (skew_edges), worst v 5.3e-11 (pendants_tet_hard); the
    soft panels runs <= 1e-13; margins 6.2e-5 (fringe300_tether), 1.2e-4 (pendants_hard_strut), >= 1e-2
    elsewhere."""
    sc, want, P = tc.port(name)
    got = tc.admm_ux(tc.one_ulp_noise(sc))
    d = tc.deviations(want, got)
    print(f"{name}: comb {d[0]:.2e} prim {d[1]:.2e} x {d[2]:.2e} v {d[3]:.2e}; margin {P.margin:.2e}, mixed {P.mixed}")
    fails = tc.check_trajectory(want, got, 2.5e-10)
    assert not fails, fails
    assert all(np.isfinite(o["x"]).all() for o in want)
    if tc.tie_mode(sc) & 3:
        assert P.margin >= 1e-6 and P.mixed


# ---------------------------------------------------------------- scenes
def test_scene_builders():
    """Scene.ties defaults to None; the tie scenes carry what they say."""
    assert scenes.cloth(4, 4).ties is None and scenes.spring_net(3, 3).ties is None
    sw = scenes.sewn_panels_offset()
    (ia, wa, ib, wb, k, rest, mode), = sw.ties
    assert ia.shape == (7, 3) and ib.shape == (7, 3) and (rest == 0).all() and mode == scenes.SPRING
    assert ia.max() < 25 <= ib.min()                                   # one anchor on each panel
    assert wa.min() > 0 and wb.min() > 0 and np.abs(wa.sum(1) - 1).max() <= 1e-12 and np.abs(wb.sum(1) - 1).max() <= 1e-12
    pa, pb = tc.anchors(sw.x, sw.ties[0])
    assert np.allclose(pa[:, 2], pb[:, 2]) and (sp.norm3(pb - pa) > 0.04).all()
    d = sw.x[25:, None, :] - sw.x[None, :25, :]                          # no node faces a node across the seam
    assert np.abs(d[..., 2]).min() > 1e-3
    pb_ = scenes.patch_on_block()
    (ia, wa, ib, wb, k, rest, mode), = pb_.ties
    assert ia.shape == (16, 3) and ib.shape == (16, 1) and rest is None and (wb == 1).all()
    assert ia.max() < 27 <= ib.min() and wa.min() > 0
    pa, pb = tc.anchors(pb_.x, pb_.ties[0])
    assert np.allclose(sp.norm3(pb - pa), 0.03) and np.allclose(pa[:, [0, 2]], pb[:, [0, 2]])
    assert pb_.obstacles[0][0] == scenes.OBS_FLOOR and pb_.obstacle_friction == [0.5] and len(pb_.collision_idx) == 9
    # the host query agrees with brute force on its own triangle
    V, F = scenes.tri_grid(4, 4)
    Q = np.random.default_rng(0).uniform(-0.2, 1.2, size=(50, 3)) * [1, 0.3, 1]
    c, tri, b = scenes.closest_on_surface(V, F, Q)
    assert np.abs((b[:, :, None] * V[F[tri]]).sum(1) - c).max() <= 1e-14
    assert tc.long_ties_13().ties[0][0].shape == (26, 3)
