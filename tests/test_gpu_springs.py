"""GPU tests of the spring term (aa_elastic_add_springs): the spring prox through its hook, whole
trajectories against the numpy port of the (u,x) loop with springs (tests/spring_cases.py, shown by
tests/test_springs.py to be the committed bending port bit for bit where there are no springs), two
closed forms, the rest shape as an equilibrium, springs beside tets, moving anchors, mesh contact and
friction, bitwise guards (a scene without the field, graph replay, run to run), and the refusals."""
import dataclasses

import numpy as np
import pytest

import spring_cases as sp
from golden_io import compare, scenes

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KEYS = ("prim", "comb", "reject", "x", "v")


def _run(pkg, ctx, sc, n_steps=None):
    out, s = pkg.capi.run_scene(ctx, sc, n_steps)
    s.close()
    return out


# ---------------------------------------------------------------- a. prox hook
@pytest.mark.parametrize("mode", sp.MODES)
def test_spring_prox_hook(mode, pkg, ctx):
    """Op 6: 300 vectors with |v| in [1e-6, 1e3] plus v = 0 plus vectors with n == L bitwise (on an
    axis, so that no rounding of the norm is involved), L in {0, 0.5, 2}: |z - z_numpy| <= 8 eps
    max(|v|, L) per component (the hinge hook's bar: the device contracts the norm to FMA). Inactive
    and n = 0 cases are v bitwise; the iteration count is 0. A vector whose own n lies within the
    norm's rounding of L may fall on either side of the decision on the device; none of the random
    ones does (asserted), so none is left out."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(300, 3))
    rnd = d / np.linalg.norm(d, axis=1, keepdims=True) * (10.0 ** rng.uniform(-6, 3, size=(300, 1)))
    side = mode & 3
    for L in (0.0, 0.5, 2.0):
        on = np.array([[L, 0.0, 0.0], [0.0, -L, 0.0], [0.0, 0.0, L]])
        v = np.vstack([rnd, np.zeros((1, 3)), on])
        n = sp.norm3(v)
        assert (n[301:] == L).all()
        assert (np.abs(n[:300] - L) > 8 * EPS * np.maximum(n[:300], L)).all()   # the decision is not a matter of rounding
        z, it = pkg.capi.hook_prox(ctx, 6, [L, mode], v)
        want = sp.spring_prox(v, L, mode)
        bar = 8 * EPS * np.maximum(n, L)[:, None]
        assert (np.abs(z - want) <= bar).all(), (mode, L, (np.abs(z - want) / np.maximum(bar, 1e-300)).max())
        slack = (n == 0.0) | ((n <= L) if side == 1 else (n >= L) if side == 2 else np.zeros(len(n), bool))
        assert slack[300] and (slack[301:].all() if side or L == 0.0 else not slack[301:].any())
        assert z[slack].tobytes() == v[slack].tobytes()
        assert (it == 0).all()
        if side == 0 and L > 0:   # the rest length matters
            assert np.linalg.norm(z[:300], axis=1).min() >= (0.999 if mode & 4 else 0.49) * L
        if (mode & 4) and (~slack).any():   # a hard form's active output has length L
            assert np.abs(sp.norm3(z[~slack]) - L).max() <= 8 * EPS * max(L, 1e-300)


# ---------------------------------------------------------------- b. trajectories against the port
_PORT = {}


def _port(name, make):
    if name not in _PORT:   # computed once, shared, never changed
        sc = make()
        keep = {}
        _PORT[name] = (sc, sp.admm_ux(sc, keep=keep), keep["P"])
    return _PORT[name]


TRAJ = {
    "pair": lambda: sp.pair_scene(),
    "chain5_moving_anchor": lambda: sp.chain5(),
    "net5": lambda: sp.net5(),
    "net5_m0": lambda: sp.net5(accel=0),
    "net5_m3": lambda: sp.net5(aa_m=3),
    "net5_m5": lambda: sp.net5(aa_m=5),
    "net5_penalty2": lambda: sp.net5(penalty=2.0),
    "stitched_panels": lambda: scenes.stitched_panels(),
    "long_ties_13": lambda: sp.long_ties_13(),
    **sp.ONE_SIDED,
}


@pytest.mark.parametrize("name", list(TRAJ))
def test_trajectory_matches_port(name, pkg, ctx):
    """The project's closed-form tolerances, as test_gpu_bending.test_trajectory_matches_port states
    them: curves 1e-9 comb_0 of each step (prim 1e-8 prim_0), equal record counts, reject flags equal
    over the first 20 iterations, final x and v 1e-9 relative. The one-sided and hard scenes satisfy
    the margin condition in the port (tests/test_springs.py; asserted again here on the shared run)."""
    sc, want, P = _port(name, TRAJ[name])
    if name in sp.ONE_SIDED and sc.springs[0][3] & 3:
        assert P.margin >= 1e-6 and P.mixed
    got = _run(pkg, ctx, sc)
    for k, (w, g) in enumerate(zip(want, got)):
        n = min(len(w["comb"]), len(g["comb"]))
        print(f"{name} step {k}: {len(g['comb'])} records (port {len(w['comb'])}), comb dev "
              f"{np.abs(w['comb'][:n] - g['comb'][:n]).max() / w['comb'][0]:.3e}, rejects {int(g['reject'].sum())}")
        assert len(w["comb"]) == len(g["comb"])
    gx, gv = got[-1]["x"].reshape(-1, 3), got[-1]["v"].reshape(-1, 3)
    print(f"x rel {np.linalg.norm(gx - want[-1]['x']) / np.linalg.norm(want[-1]['x']):.3e}, "
          f"v rel {np.linalg.norm(gv - want[-1]['v']) / np.linalg.norm(want[-1]['v']):.3e}")
    got[-1]["x"] = gx
    fails = compare(want, got, 1e-9, 1e-9)
    assert not fails, fails
    assert np.linalg.norm(gv - want[-1]["v"]) <= 1e-9 * np.linalg.norm(want[-1]["v"])
    if name == "long_ties_13":
        s = pkg.capi.solver_from_scene(ctx, sc)
        s.initialize(pkg.capi.settings_from_scene(sc))
        rt = s.runtime()
        s.close()
        assert rt.n_elements == 288 + 26 and rt.z_dim == 288 * 6 + 26 * 3 and rt.n_free == 167
        # the tree is not one dense front: the case tests what it claims
        assert rt.nnz_factor < rt.n_free * (rt.n_free + 1) // 2, rt.nnz_factor
    if name == "net5":
        s = pkg.capi.solver_from_scene(ctx, sc)
        s.initialize(pkg.capi.settings_from_scene(sc))
        rt = s.runtime()
        s.close()
        assert rt.n_elements == 72 and rt.z_dim == 72 * 3


# ---------------------------------------------------------------- c. closed forms
def test_reaches_the_dense_minimiser_of_stitches(pkg, ctx):
    """The zero-length-springs step of tests/test_springs.py on the GPU: |x - x*|inf <= 8 max(port's
    error, 64 eps max|x*|), test_gpu_bending.test_reaches_the_dense_minimiser's form."""
    sc = sp.stitches_only_scene()
    xstar, move = sp.dense_minimiser(sc)
    port = np.abs(sp.admm_ux(sc)[0]["x"] - xstar).max()
    got = _run(pkg, ctx, sc)[0]["x"].reshape(-1, 3)
    err = np.abs(got - xstar).max()
    print(f"|x - x*|inf: GPU {err:.3e}, port {port:.3e}; displacement {move:.3e}")
    assert err <= 8 * max(port, 64 * EPS * np.abs(xstar).max())


def test_hanging_mass_settles_at_mg_over_k(pkg, ctx):
    """One mass on a soft spring from a pinned anchor, 60 steps: |extension - m g / k| <= 8 max(port's
    error, 64 eps L) with L = 0.5 the scale of the positions."""
    sc = sp.hanging_mass_scene()
    port = sp.hanging_mass_error(sp.admm_ux(sc), sc)
    err = sp.hanging_mass_error(_run(pkg, ctx, sc), sc)
    print(f"|extension - m g / k|: GPU {err:.3e}, port {port:.3e}; extension {sc.masses[1] * 9.8 / sc.springs[0][1]:.3e}")
    assert err <= 8 * max(port, 64 * EPS * 0.5)


# ---------------------------------------------------------------- d. rest equilibrium
def test_rest_is_an_equilibrium(pkg, ctx):
    """spring_net, gravity 0, derived L, 5 steps: every node within 1e-12 of the extent of where it
    started (host L and device |v| differ by rounding only). All L scaled by 0.9: it moves by more
    than 1e-6 of the extent."""
    keep = scenes.spring_net(5, 5, gravity=0.0, n_steps=5)
    assert keep.springs[0][2] is None
    ext = float((keep.x.max(0) - keep.x.min(0)).max())
    x = _run(pkg, ctx, keep)[-1]["x"].reshape(-1, 3)
    print(f"derived L: max move {np.abs(x - keep.x).max() / ext:.3e} of the extent")
    assert np.abs(x - keep.x).max() <= 1e-12 * ext
    short = scenes.spring_net(5, 5, gravity=0.0, n_steps=5, rest_scale=0.9)
    xs = _run(pkg, ctx, short)[-1]["x"].reshape(-1, 3)
    print(f"0.9 L: max move {np.abs(xs - short.x).max() / ext:.3e} of the extent")
    assert np.abs(xs - short.x).max() > 1e-6 * ext


# ---------------------------------------------------------------- e. beside the rest of the solver
def _bitwise_three_ways(pkg, ctx, sc, monkeypatch):
    a, b = _run(pkg, ctx, sc), _run(pkg, ctx, sc)
    monkeypatch.setenv("AA_ADMM_NO_GRAPH", "1")
    eager = _run(pkg, ctx, sc)
    monkeypatch.delenv("AA_ADMM_NO_GRAPH")
    for k in range(sc.n_steps):
        for key in KEYS:
            assert np.array_equal(a[k][key], b[k][key]), ("rerun", k, key)
            assert np.array_equal(a[k][key], eager[k][key]), ("eager", k, key)
    return a


def test_hanging_block_follows_its_moving_anchors(pkg, ctx, monkeypatch):
    """Tets + springs + anchors moved every step through set_pins: graph replay equals eager bitwise,
    a rerun is bitwise equal, x is finite, the anchors are where pin_vel puts them, and the block's
    centre follows them sideways (the springs drag it) while its weight stretches the springs."""
    sc = scenes.hanging_block()
    out = _bitwise_three_ways(pkg, ctx, sc, monkeypatch)
    x = out[-1]["x"].reshape(-1, 3)
    assert np.isfinite(x).all()
    nb = sc.n_nodes - 4
    assert np.allclose(x[nb:], sc.pin_pts + sc.n_steps * sc.pin_vel, rtol=0, atol=1e-15)
    pairs = sc.springs[0][0]
    assert (scenes.pair_lengths(x, pairs) > scenes.pair_lengths(sc.x, pairs)).all()
    assert x[:nb, 0].mean() - sc.x[:nb, 0].mean() > 1e-4


def test_tethered_cloth_on_an_obstacle_with_friction(pkg, ctx, monkeypatch):
    """tethered_cloth: hard tethers beside triangles, a mesh obstacle and its friction pass. Graph
    replay equals eager bitwise, a rerun is bitwise equal, contacts are recorded, x is finite, and at
    the end of every step no tether is longer than L (1 + delta), delta = 8 x the port's worst
    violation on the same scene without the obstacle (both printed). Measured: port 4.8e-7 (delta
    3.9e-6), GPU 3.5e-8 with the scene's patch of 10 collision-checked nodes. With every free node
    collision-checked (collide_radius=None) the same bound is missed by far, 1.1e-1: each collision
    term weighs 5.7e3 against the tethers' 7 and 30 iterations leave comb at 1e-1 (scenes.tethered_cloth)."""
    sc = scenes.tethered_cloth()
    free = sp.tethered_cloth_free()
    port = max(sp.tether_violation(o["x"], free) for o in sp.admm_ux(free))
    assert port > 0
    out = _bitwise_three_ways(pkg, ctx, sc, monkeypatch)
    got, s = pkg.capi.run_scene(ctx, sc)
    n_contacts = len(s.contacts()["node"])
    s.close()
    assert n_contacts > 0 and all(np.isfinite(o["x"]).all() for o in out)
    assert np.array_equal(got[-1]["x"], out[-1]["x"])
    worst = max(sp.tether_violation(o["x"], sc) for o in out)
    print(f"worst tether violation: GPU {worst:.3e}, port (no obstacle) {port:.3e}, delta {8 * port:.3e}; {n_contacts} contacts")
    assert worst <= 8 * port


# ---------------------------------------------------------------- f. nothing else moved
def test_scene_without_the_field_is_bitwise_the_same(pkg, ctx):
    """scenes.cloth(12, 12, bend=1e-2): a scene object without the `springs` attribute, springs=None
    and springs=[] give bitwise equal runs and equal runtime() counts."""
    sc = scenes.cloth(12, 12, bend=1e-2, iters=30, n_steps=2)
    assert sc.springs is None

    class Bare:
        pass

    bare = Bare()
    for f in dataclasses.fields(sc):
        if f.name != "springs":
            setattr(bare, f.name, getattr(sc, f.name))
    bare.rest_x, bare.n_nodes = sc.rest_x, sc.n_nodes
    assert not hasattr(bare, "springs")
    empty = dataclasses.replace(sc, springs=[])
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


# ---------------------------------------------------------------- g. refusals
def test_refusals(pkg, ctx):
    AAError = pkg.capi.AAError
    sc = sp.net5(iters=5, n_steps=1)
    pairs = sc.springs[0][0]
    # the z-AA variant
    s = pkg.capi.solver_from_scene(ctx, sc)
    st = pkg.capi.settings_from_scene(sc)
    st.variant = pkg.capi.AA_VARIANT_Z
    with pytest.raises(AAError, match="springs exist in the \\(u,x\\) variant only") as e:
        s.initialize(st)
    assert e.value.code == -1
    s.close()
    # a partitioned solver
    comm = pkg.capi.Comm.solo(0, 2)
    s = pkg.capi.solver_from_scene(ctx, sc, comm)
    with pytest.raises(AAError, match="springs need one rank") as e:
        s.initialize(pkg.capi.settings_from_scene(sc))
    assert e.value.code == -1 and "2 ranks" in str(e.value)
    s.close()
    comm.close()
    # every AA_ERR_ARG case, each on the same solver: a refused call touches nothing
    s = pkg.capi.solver_from_scene(ctx, sc)
    n = sc.n_nodes
    k = np.full(len(pairs), 50.0)
    bad = lambda i, val, arr: np.concatenate([arr[:i], [val], arr[i + 1:]])
    p_hi, p_neg, p_self = pairs.copy(), pairs.copy(), pairs.copy()
    p_hi[5, 1], p_neg[4, 0], p_self[7] = n, -1, [3, 3]
    rest = np.full(len(pairs), 0.2)
    cases = [
        (dict(pairs=p_hi, k=k), "spring 5.*out of range"),
        (dict(pairs=p_neg, k=k), "spring 4.*out of range"),
        (dict(pairs=p_self, k=k), "spring 7.*itself"),
        (dict(pairs=pairs, k=bad(2, 0.0, k)), "spring 2.*k must be"),
        (dict(pairs=pairs, k=bad(3, -1.0, k)), "spring 3.*k must be"),
        (dict(pairs=pairs, k=bad(0, np.nan, k)), "spring 0.*k must be"),
        (dict(pairs=pairs, k=bad(6, np.inf, k)), "spring 6.*k must be"),
        (dict(pairs=pairs, k=k, rest=bad(1, -0.1, rest)), "spring 1.*rest"),
        (dict(pairs=pairs, k=k, rest=bad(8, np.nan, rest)), "spring 8.*rest"),
        (dict(pairs=pairs, k=k, rest=bad(9, np.inf, rest)), "spring 9.*rest"),
        (dict(pairs=pairs, k=k, mode=3), "unknown mode 3"),
        (dict(pairs=pairs, k=k, mode=7), "unknown mode 7"),
        (dict(pairs=pairs, k=k, mode=8), "unknown mode 8"),
        (dict(pairs=pairs, k=k, mode=-1), "unknown mode -1"),
    ]
    for kw, pattern in cases:
        with pytest.raises(AAError, match=pattern) as e:
            s.add_springs(**kw)
        assert e.value.code == -1, pattern
    import ctypes as C
    L = pkg.capi.lib()
    dp, ip = pkg.capi._dp, pkg.capi._ip
    x = np.ascontiguousarray(sc.x).reshape(-1)
    pf = np.ascontiguousarray(pairs, np.int32).reshape(-1)
    m = C.c_int(len(pairs))
    raw = [
        ((dp(x), None, m, C.c_int(0), dp(k), None, C.c_int(0)), "null"),            # pairs
        ((dp(x), ip(pf), m, C.c_int(0), None, None, C.c_int(0)), "null"),           # k
        ((None, ip(pf), m, C.c_int(0), dp(k), None, C.c_int(0)), "rest == NULL"),   # neither rest nor verts
        ((dp(x), ip(pf), m, C.c_int(0), dp(k), None, C.c_int(1)), "out of range"),  # offset pushes node 24 out
    ]
    for args, word in raw:
        assert L.aa_elastic_add_springs(s.h, *args) == -1
        assert word in L.aa_last_error().decode()
    # after all that the solver is the scene's, bit for bit, and add_springs after initialize is a state error
    s.initialize(pkg.capi.settings_from_scene(sc))
    n_el = s.runtime().n_elements
    assert n_el == len(pairs)
    with pytest.raises(AAError, match="after initialize") as e:
        s.add_springs(pairs, 50.0)
    assert e.value.code == -2
    s.step()
    assert s.runtime().n_elements == n_el and np.isfinite(s.x).all()
    assert np.array_equal(s.x, _run(pkg, ctx, sc)[0]["x"])
    s.close()
    # scalar k is broadcast, rest given without vertices, an empty call: the solver runs
    s = pkg.capi.solver_from_scene(ctx, dataclasses.replace(sc, springs=None))
    s.add_springs(pairs[:0], 50.0)
    s.add_springs(pairs, 50.0, rest=sc.springs[0][2], mode=pkg.capi.AA_SPRING)
    s.initialize(pkg.capi.settings_from_scene(sc))
    s.step()
    assert np.array_equal(s.x, _run(pkg, ctx, sc)[0]["x"])
    s.close()
