"""CPU tests of the spring term: the prox against a brute-force search, the host builder
(csrc/springs.hpp) in a stand-alone program against the numpy restatement with every refusal, the
numpy port of the (u,x) loop with springs (tests/spring_cases.py) -- bit for bit the committed
bending port where there are no springs -- against two closed forms, and the margin condition of
the one-sided and hard scenes the GPU tests use."""
import os
import subprocess

import numpy as np
import pytest

import bending_cases as bc
import spring_cases as sp
from conftest import REPO
from golden_io import scenes

CSRC = os.path.join(REPO, "aa-admm_amd", "csrc")
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------- prox
def _feasible(t, L, mode):
    """Lengths |t| a hard form admits."""
    side = mode & 3
    a = np.abs(t)
    return a == L if side == 0 else a <= L if side == 1 else a >= L


def _objective(t, n, L, mode):
    """U(t vhat) / k + 1/2 (t - n)^2 for z = t vhat along v (t may be negative)."""
    a = np.abs(t)
    side = mode & 3
    d = a - L if side == 0 else np.maximum(0.0, a - L) if side == 1 else np.maximum(0.0, L - a)
    U = np.where(_feasible(t, L, mode), 0.0, np.inf) if mode & 4 else 0.5 * d * d
    return U + 0.5 * (t - n) ** 2


@pytest.mark.parametrize("mode", sp.MODES)
def test_spring_prox_is_the_minimiser(mode):
    """z = s v against a 1-D search along v (20 001 points on [-(n + L), 2 (n + L)] plus +-L and n),
    and no nearby point -- projected onto the set for a hard form -- does better. Includes n = L
    exactly, n = 0 and L = 0; the inactive branch returns v bitwise."""
    rng = np.random.default_rng(7 + mode)
    for L in (0.0, 0.5, 2.0):
        d = rng.normal(size=(40, 3))
        d /= sp.norm3(d)[:, None]
        lengths = np.concatenate([10.0 ** rng.uniform(-3, 1.5, size=34), [L, L, 0.999 * L + 1e-3, 1.001 * L + 1e-3, 0.0, 0.0]])
        v = d * lengths[:, None]
        v[34] = [L, 0.0, 0.0]          # n = L bitwise
        v[35] = [0.0, 0.0, -L]
        n = sp.norm3(v)
        assert n[34] == L and n[35] == L and n[-1] == 0.0
        z = sp.spring_prox(v, L, mode)
        side = mode & 3
        slack = (n == 0) | ((n <= L) if side == 1 else (n >= L) if side == 2 else False)
        assert slack[34] == (side != 0 or L == 0.0) and slack[-1]
        for i in np.nonzero(slack)[0]:
            assert z[i].tobytes() == v[i].tobytes(), (mode, L, i)
        for i in range(len(v)):
            if n[i] == 0.0:
                continue
            vhat = v[i] / n[i]
            t_star = float(z[i] @ vhat)
            assert np.abs(z[i] - t_star * vhat).max() <= 4 * EPS * max(n[i], L)   # z lies along v
            span = n[i] + L
            grid = np.concatenate([np.linspace(-span, 2 * span, 20001), [L, -L, n[i], t_star]])
            f = _objective(grid, n[i], L, mode)
            best = grid[np.argmin(f)]
            f_star = _objective(np.array([t_star]), n[i], L, mode)[0] if not (mode & 4) else 0.5 * (t_star - n[i]) ** 2
            if mode & 4:   # the returned length is in the set (to rounding)
                a = abs(t_star)
                ok = abs(a - L) <= 4 * EPS * max(L, n[i]) if side == 0 or not slack[i] else (a <= L if side == 1 else a >= L)
                assert ok, (mode, L, i, t_star)
            assert f_star <= f.min() + 1e-12 * span * span, (mode, L, i, t_star, best)
            assert abs(t_star - best) <= 3 * span / 20000 + 1e-12, (mode, L, i, t_star, best)
        # perturbed directions
        w = np.nonzero(n > 0)[0]
        for _ in range(20):
            q = z[w] + rng.normal(size=(len(w), 3)) * 1e-3 * np.maximum(n[w], L)[:, None]
            nq = sp.norm3(q)
            if mode & 4:   # onto the set: |q| = L, <= L or >= L
                target = np.full(len(w), L) if side == 0 else np.minimum(nq, L) if side == 1 else np.maximum(nq, L)
                q = q * (target / nq)[:, None]
                nq = sp.norm3(q)
                U_q, U_z = 0.0, 0.0
            else:
                dd = lambda a: a - L if side == 0 else np.maximum(0.0, a - L) if side == 1 else np.maximum(0.0, L - a)
                U_q, U_z = 0.5 * dd(nq) ** 2, 0.5 * dd(sp.norm3(z[w])) ** 2
            fq = U_q + 0.5 * np.sum((q - v[w]) ** 2, -1)
            fz = U_z + 0.5 * np.sum((z[w] - v[w]) ** 2, -1)
            assert (fq >= fz - 64 * EPS * np.maximum(n[w], L) ** 2).all(), (mode, L)
    assert np.array_equal(sp.spring_prox(np.zeros((1, 3)), 2.0, mode), np.zeros((1, 3)))


# ---------------------------------------------------------------- host builder
def _write_case(f, name, V, pairs, mode, k, rest, flags):
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(pairs)
    f.write(f"{name} {len(V)} {n} {mode} {flags}\n")
    f.write("\n".join(" ".join(repr(float(c)) for c in v) for v in V) + "\n")
    f.write("\n".join(" ".join(str(int(i)) for i in p) for p in pairs) + "\n")
    f.write(" ".join(repr(float(c)) for c in np.broadcast_to(k, (n,))) + "\n")
    f.write(" ".join(repr(float(c)) for c in (np.zeros(n) if rest is None else np.broadcast_to(rest, (n,)))) + "\n")


def _refused():
    """name -> (V, pairs, mode, k, rest, flags, words the message must contain); all AA_ERR_ARG (-1)"""
    V = scenes.spring_net(3, 3).x
    P = scenes.net_pairs(3, 3)
    k = np.full(len(P), 2.0)
    bad = lambda i, val, arr: np.concatenate([arr[:i], [val], arr[i + 1:]])
    Pi = P.copy(); Pi[5, 1] = 9
    Pn = P.copy(); Pn[4, 0] = -1
    Ps = P.copy(); Ps[7] = [3, 3]
    rest = np.full(len(P), 0.4)
    return {
        "index_high": (V, Pi, 0, k, None, 1, ("spring 5", "out of range")),
        "index_negative": (V, Pn, 0, k, None, 1, ("spring 4", "out of range")),
        "self": (V, Ps, 0, k, None, 1, ("spring 7", "itself")),
        "k_zero": (V, P, 0, bad(2, 0.0, k), None, 1, ("spring 2", "k must be")),
        "k_negative": (V, P, 1, bad(3, -1.0, k), None, 1, ("spring 3", "k must be")),
        "k_nan": (V, P, 2, bad(0, np.nan, k), None, 1, ("spring 0", "k must be")),
        "k_inf": (V, P, 4, bad(6, np.inf, k), None, 1, ("spring 6", "k must be")),
        "rest_negative": (V, P, 0, k, bad(1, -0.1, rest), 3, ("spring 1", "rest")),
        "rest_nan": (V, P, 5, k, bad(8, np.nan, rest), 3, ("spring 8", "rest")),
        "rest_inf": (V, P, 6, k, bad(9, np.inf, rest), 3, ("spring 9", "rest")),
        "mode_3": (V, P, 3, k, None, 1, ("unknown mode 3",)),
        "mode_7": (V, P, 7, k, None, 1, ("unknown mode 7",)),
        "mode_8": (V, P, 8, k, None, 1, ("unknown mode 8",)),
        "mode_negative": (V, P, -1, k, None, 1, ("unknown mode -1",)),
        "null_pairs": (V, P, 0, k, None, 1 | 4, ("null",)),
        "null_k": (V, P, 0, k, None, 1 | 8, ("null",)),
        "no_rest_no_verts": (V, P, 0, k, None, 0, ("rest == NULL", "verts3")),
    }


def test_host_builder_matches_numpy_and_refuses(tmp_path):
    """tests/cpp/springs.cpp against spring_cases.springs: idx and G equal, L and w bitwise (a
    difference, three products, a square root in the same order) for given and derived L; every
    refusal with its code and its spring named; rest given needs no vertices."""
    V = scenes.spring_net(4, 3).x.copy()
    V[:, 1] = 0.1 * np.sin(np.arange(len(V)))       # lengths that are not round numbers
    P = scenes.net_pairs(4, 3)
    rng = np.random.default_rng(2)
    k = 10.0 ** rng.uniform(-1, 3, size=len(P))
    given = rng.uniform(0.0, 1.0, size=len(P))
    given[3] = 0.0
    good = {"derived": (V, P, 0, k, None, 1), "given": (V, P, 5, k, given, 3), "given_no_verts": (V, P, 2, k, given, 2),
            "parallel": (V, np.array([[0, 1], [1, 0], [0, 1]]), 6, k[:3], None, 1), "empty": (V, np.zeros((0, 2)), 1, k[:0], None, 0)}
    refused = _refused()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for name, c in good.items():
            _write_case(f, name, *c)
        for name, c in refused.items():
            _write_case(f, name, *c[:6])
    exe = str(tmp_path / "springs")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "springs.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and f"ok {len(good) + len(refused)} cases" in r.stdout, r.stdout[-2000:] + r.stderr
    got, errors, cur = {}, {}, None
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "set":
            cur = got.setdefault(t[1], [])
        elif t[0] == "s":
            cur.append(([int(a) for a in t[1:3]], [float(a) for a in t[3:]]))
        elif t[0] == "error":
            errors[t[1]] = (int(t[2]), line)
    assert not (set(errors) & set(good)), errors
    for name, (Vc, Pc, mode, kc, rest, flags) in good.items():
        idx, G, L, w = sp.springs(Vc, Pc, kc, rest)
        assert len(got[name]) == len(idx)
        if not len(idx):
            continue
        assert np.array_equal(np.array([g[0] for g in got[name]]), idx)
        have = np.array([g[1] for g in got[name]])
        assert np.array_equal(have[:, :2], G) and (G == [-1.0, 1.0]).all()
        assert np.array_equal(have[:, 2], L), (name, np.abs(have[:, 2] - L).max())
        assert np.array_equal(have[:, 3], w), (name, np.abs(have[:, 3] - w).max())
        assert np.array_equal(w * w, np.sqrt(kc) ** 2)
    assert np.array_equal(sp.springs(V, P, k, None)[2], scenes.pair_lengths(V, P)) and (sp.springs(V, P, k, None)[2] > 0).all()
    for name, c in refused.items():
        assert name in errors, (name, r.stdout[-500:])
        assert errors[name][0] == -1 and all(word in errors[name][1] for word in c[6]), errors[name]


# ---------------------------------------------------------------- the port
@pytest.mark.parametrize("make", [bc.grid3_scene, bc.pair_scene])
def test_port_copy_reproduces_the_bending_port_bit_for_bit(make):
    """spring_cases.admm_ux is bending_cases.admm_ux_numpy with the problem class as a parameter: with
    bc._Problem, and with SpringProblem on a scene without springs, every record is bitwise equal."""
    sc = make()
    want = bc.admm_ux_numpy(sc)
    for problem in (bc._Problem, sp.SpringProblem):
        got = sp.admm_ux(sc, problem)
        assert len(got) == len(want) == sc.n_steps
        for k in range(len(want)):
            assert set(got[k]) == set(want[k])
            for key in want[k]:
                assert got[k][key].tobytes() == want[k][key].tobytes(), (problem.__name__, k, key)


def test_port_reaches_the_dense_minimiser_of_stitches():
    """Zero-length soft springs only (5 x 5 net, corners pinned, no Anderson, up to 100 iterations):
    the problem is quadratic, and the port's first step is held to the dense solve's x* by the bar
    test_bending.test_port_reaches_the_dense_minimiser sets for hinges, 1e-10 max|x*|. Measured
    3.1e-12 against a displacement of 1.1e-1 (the loop leaves at comb < 1e-20 after 33 iterations)."""
    sc = sp.stitches_only_scene()
    assert (sc.springs[0][2] == 0.0).all() and sc.springs[0][3] == sp.SPRING
    xstar, move = sp.dense_minimiser(sc)
    got = sp.admm_ux(sc)[0]["x"]
    err = np.abs(got - xstar).max()
    print(f"port: |x - x*|inf {err:.3e}, displacement {move:.3e}")
    assert move > 1e-3
    assert err <= 1e-10 * np.abs(xstar).max()


def test_port_settles_the_hanging_mass():
    """One mass on a soft spring under gravity from a pinned anchor: after 60 steps (omega dt = 2) the
    extension is m g / k = 2.72e-3. The port's error is recorded (printed; the GPU test's bar is
    built on it): 1.3e-11. Like the minimiser above it has to lie below the 1e-9 relative the GPU is
    held to: 1e-10 of the spring's length is asked."""
    sc = sp.hanging_mass_scene()
    k, m = sc.springs[0][1], sc.masses[1]
    assert abs(np.sqrt(k / m) * sc.dt - 2.0) < 1e-12
    out = sp.admm_ux(sc)
    err = sp.hanging_mass_error(out, sc)
    print(f"port: |extension - m g / k| {err:.3e} of {m * 9.8 / k:.3e}")
    assert err <= 1e-10 * 0.5
    assert np.abs(out[-1]["v"]).max() <= 1e-8     # at rest


# ---------------------------------------------------------------- margin condition
@pytest.mark.parametrize("name", list(sp.ONE_SIDED) + ["tethered_cloth"])
def test_one_sided_scenes_stay_away_from_the_threshold(name):
    """Every one-sided or hard scene the GPU tests run: over every prox evaluation of the port's run,
    min |n - L| / max(L, n) >= 1e-6 over all one-sided springs (none left out), and some evaluation
    sees active and inactive springs together. The two-sided hard form has no decision at n = L --
    s = L / n is continuous there, and n -> L is its converged state -- so chain5_hard has no
    threshold to keep away from (its margin is inf; only n = 0 branches, and no link collapses)."""
    sc = sp.tethered_cloth_free() if name == "tethered_cloth" else sp.ONE_SIDED[name]()
    keep = {}
    out = sp.admm_ux(sc, keep=keep)
    P = keep["P"]
    print(f"{name}: margin {P.margin:.3e} over {P.evaluations} evaluations, mixed {P.mixed}")
    assert all(np.isfinite(o["x"]).all() for o in out)
    mode = sc.springs[0][3]
    if mode & 3:
        assert P.margin >= 1e-6
        assert P.mixed
    else:
        assert mode == sp.HARD and P.margin == np.inf
        pairs = sc.springs[0][0]
        assert all(scenes.pair_lengths(o["x"], pairs).min() > 0.1 for o in out)


def test_hard_scenes_are_hard():
    """The hard forms do what they say in the port: chain5_hard keeps its links at L, the hard
    one-sided nets end their last step within the ADMM residual of their sets."""
    sc = sp.ONE_SIDED["chain5_hard"]()
    x = sp.admm_ux(sc)[-1]["x"]
    pairs, _, L, _ = sc.springs[0]
    assert np.abs(scenes.pair_lengths(x, pairs) / L - 1.0).max() < 1e-6
    assert np.abs(x[1:] - sc.x[1:]).max() > 1e-2    # and it moved


# ---------------------------------------------------------------- scenes
def test_scene_builders():
    """Scene.springs defaults to None; the spring scenes carry what they say."""
    assert scenes.cloth(4, 4).springs is None and bc.grid3_scene().springs is None
    net = scenes.spring_net(5, 5)
    (pairs, k, rest, mode), = net.springs
    assert len(pairs) == 2 * 5 * 4 + 2 * 4 * 4 and rest is None and mode == scenes.SPRING and not net.groups
    assert list(net.pin_idx) == [0, 4, 20, 24]
    assert np.allclose(scenes.spring_net(5, 5, rest_scale=0.9).springs[0][2], 0.9 * scenes.pair_lengths(net.x, pairs))
    st = scenes.stitched_panels()
    assert (st.springs[0][2] == 0).all() and len(st.springs[0][0]) == 5 and st.bending is not None and len(st.groups) == 1
    assert (scenes.pair_lengths(st.x, st.springs[0][0]) > 0).all()
    tc = scenes.tethered_cloth()
    assert tc.springs[0][3] == scenes.SPRING_HARD | scenes.SPRING_TETHER and len(tc.mesh_obstacles) == 1 and tc.obstacle_friction == [0.5]
    assert set(tc.springs[0][0][:, 0]) <= set(tc.pin_idx) and not (set(tc.springs[0][0][:, 1]) & set(tc.pin_idx))
    hb = scenes.hanging_block()
    assert hb.groups[0].kind == scenes.TET and len(hb.pin_idx) == 4 and np.abs(hb.pin_vel).max() > 0
    assert set(hb.springs[0][0][:, 0]) == set(hb.pin_idx) and (hb.springs[0][0][:, 1] < hb.n_nodes - 4).all()
    lt = sp.long_ties_13()
    assert lt.n_nodes == 169 and len(lt.springs[0][0]) == 26
