"""GPU tests of the bending term (aa_elastic_add_bending): the hinge prox through its hook, whole
trajectories against the numpy port of the (u,x) loop (tests/bending_cases.py, anchored to the
committed oracle by tests/test_bending.py), the exact minimiser of a hinges-only step, a curved
rest shape as an equilibrium, bitwise guards (a scene without the field, graph replay, run to run),
bending beside mesh contact with friction, and the refusals."""
import dataclasses

import numpy as np
import pytest

import bending_cases as bc
from golden_io import compare, scenes

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _run(pkg, ctx, sc, n_steps=None):
    out, s = pkg.capi.run_scene(ctx, sc, n_steps)
    s.close()
    return out


# ---------------------------------------------------------------- a. prox hook
def test_hinge_prox_hook(pkg, ctx):
    """300 vectors with |v| in [1e-6, 1e3] plus v = 0, r in {0, 0.5, 2}: |z - z_numpy| <= 8 eps
    max(|v|, r) per component (the device contracts to FMA; three roundings separate the two);
    v = 0 gives z = 0 bitwise."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(300, 3))
    v = d / np.linalg.norm(d, axis=1, keepdims=True) * (10.0 ** rng.uniform(-6, 3, size=(300, 1)))
    v = np.vstack([v, np.zeros((1, 3))])
    for r in (0.0, 0.5, 2.0):
        z, it = pkg.capi.hook_prox(ctx, 5, [r], v)
        want = bc.hinge_prox(v, r)
        bar = 8 * EPS * np.maximum(np.linalg.norm(v, axis=1), r)[:, None]
        assert (np.abs(z - want) <= bar).all(), (r, (np.abs(z - want) / np.maximum(bar, 1e-300)).max())
        assert z[-1].tobytes() == np.zeros(3).tobytes()
        assert (it == 0).all()
        if r > 0:   # the rest length matters: short vectors are pushed out to about r / 2
            assert np.linalg.norm(z[:-1], axis=1).min() >= 0.49 * r


# ---------------------------------------------------------------- b. trajectories against the port
_PORT = {}


def _port(name, make):
    if name not in _PORT:   # computed once, shared, never changed
        sc = make()
        _PORT[name] = (sc, bc.admm_ux_numpy(sc))
    return _PORT[name]


TRAJ = {
    "pair": lambda: bc.pair_scene(),
    "grid3_pinned_inside": lambda: bc.grid3_scene(),
    "strip13": lambda: scenes.cantilever_strip(12, 12, 1e-2, iters=30, n_steps=2),
    "strip13_m0": lambda: scenes.cantilever_strip(12, 12, 1e-2, iters=30, n_steps=2, accel=0),
    "strip13_m5": lambda: scenes.cantilever_strip(12, 12, 1e-2, iters=30, n_steps=2, aa_m=5),
    "strip13_penalty2": lambda: scenes.cantilever_strip(12, 12, 1e-2, iters=30, n_steps=2, penalty=2.0),
    "half_cylinder_curved_rest": lambda: bc.half_cylinder_scene(flat_rest=False, n_steps=2),
}


@pytest.mark.parametrize("name", list(TRAJ))
def test_trajectory_matches_port(name, pkg, ctx):
    """The project's closed-form tolerances: curves 1e-9 comb_0 of each step (prim 1e-8 prim_0), reject
    flags equal over the first 20 iterations, final x and v 1e-9 relative."""
    sc, want = _port(name, TRAJ[name])
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
    if name.startswith("strip13"):
        s = pkg.capi.solver_from_scene(ctx, sc)
        s.initialize(pkg.capi.settings_from_scene(sc))
        rt = s.runtime()
        s.close()
        assert rt.n_elements == 288 + 408 and rt.z_dim == 288 * 6 + 408 * 3   # two blocks of hinges, the second partial


# ---------------------------------------------------------------- c. minimiser
def test_reaches_the_dense_minimiser(pkg, ctx):
    """The hinges-only step of tests/test_bending.py on the GPU: |x - x*|inf <= 8 max(port's error,
    64 eps max|x*|)."""
    sc = bc.minimiser_scene()
    xstar, move = bc.dense_minimiser(sc)
    port = np.abs(bc.admm_ux_numpy(sc)[0]["x"] - xstar).max()
    got = _run(pkg, ctx, sc)[0]["x"].reshape(-1, 3)
    err = np.abs(got - xstar).max()
    print(f"|x - x*|inf: GPU {err:.3e}, port {port:.3e}; displacement {move:.3e}")
    assert err <= 8 * max(port, 64 * EPS * np.abs(xstar).max())


# ---------------------------------------------------------------- d. rest equilibrium
def test_curved_rest_shape_is_an_equilibrium(pkg, ctx):
    """Half-cylinder strip, gravity 0, 5 steps. flat_rest 0: every node within 1e-12 of the mesh's extent
    of its rest position (host r and device |v| differ by rounding only). flat_rest 1: it moves by
    more than 1e-6 of the extent -- the switch does something."""
    keep = bc.half_cylinder_scene(flat_rest=False, gravity=0.0, n_steps=5)
    ext = float((keep.x.max(0) - keep.x.min(0)).max())
    x = _run(pkg, ctx, keep)[-1]["x"].reshape(-1, 3)
    print(f"flat_rest 0: max move {np.abs(x - keep.x).max() / ext:.3e} of the extent")
    assert np.abs(x - keep.x).max() <= 1e-12 * ext
    flat = bc.half_cylinder_scene(flat_rest=True, gravity=0.0, n_steps=5)
    xf = _run(pkg, ctx, flat)[-1]["x"].reshape(-1, 3)
    print(f"flat_rest 1: max move {np.abs(xf - flat.x).max() / ext:.3e} of the extent")
    assert np.abs(xf - flat.x).max() > 1e-6 * ext


# ---------------------------------------------------------------- e. nothing else moved
def test_scene_without_the_field_is_bitwise_the_same(pkg, ctx):
    """scenes.cloth(12, 12) with bending=None against a scene object that has no such attribute."""
    sc = scenes.cloth(12, 12, iters=30, n_steps=2)
    assert sc.bending is None

    class Bare:
        pass

    bare = Bare()
    for f in dataclasses.fields(sc):
        if f.name != "bending":
            setattr(bare, f.name, getattr(sc, f.name))
    bare.rest_x, bare.n_nodes = sc.rest_x, sc.n_nodes
    assert not hasattr(bare, "bending")
    a, b = _run(pkg, ctx, sc), _run(pkg, ctx, bare)
    for k in range(2):
        for key in ("prim", "comb", "reject", "x", "v"):
            assert np.array_equal(a[k][key], b[k][key]), (k, key)


def test_bent_strip_graph_replay_and_rerun_are_bitwise(pkg, ctx, monkeypatch):
    """The bent strip: two runs are bitwise equal, and a graph-replayed step equals an eager one."""
    sc = scenes.cantilever_strip(12, 12, 1e-2, iters=30, n_steps=3)
    a, b = _run(pkg, ctx, sc), _run(pkg, ctx, sc)
    monkeypatch.setenv("AA_ADMM_NO_GRAPH", "1")
    eager = _run(pkg, ctx, sc)
    for k in range(3):
        for key in ("prim", "comb", "reject", "x", "v"):
            assert np.array_equal(a[k][key], b[k][key]), ("rerun", k, key)
            assert np.array_equal(a[k][key], eager[k][key]), ("eager", k, key)
    assert sum(int(s["reject"].sum()) for s in a) >= 0 and np.abs(a[-1]["x"].reshape(-1, 3) - sc.x).max() > 1e-4


# ---------------------------------------------------------------- f. coexistence
def test_bending_beside_mesh_contact_and_friction(pkg, ctx):
    """cloth_on_torus(bend=1e-2) with friction 0.5, 10 steps: finishes finite, no step fails, contacts
    are recorded, and x differs from the membrane-only run by more than 1e-6."""
    runs = {}
    for bend in (None, 1e-2):
        sc = scenes.cloth_on_torus(bend=bend)
        sc.obstacle_friction = [0.5]
        sc.record_contacts = True
        out, s = pkg.capi.run_scene(ctx, sc)   # a failing step raises
        n_contacts = len(s.contacts()["node"])
        s.close()
        runs[bend] = out[-1]["x"].reshape(-1, 3)
        assert len(out) == 10 and np.isfinite(runs[bend]).all() and n_contacts > 0
    assert np.abs(runs[1e-2] - runs[None]).max() > 1e-6


# ---------------------------------------------------------------- g. refusals
def test_refusals(pkg, ctx):
    AAError = pkg.capi.AAError
    sc = scenes.cantilever_strip(4, 2, 1e-2, iters=5, n_steps=1)
    # the z-AA variant
    s = pkg.capi.solver_from_scene(ctx, sc)
    st = pkg.capi.settings_from_scene(sc)
    st.variant = pkg.capi.AA_VARIANT_Z
    with pytest.raises(AAError, match="bending hinges exist in the \\(u,x\\) variant only") as e:
        s.initialize(st)
    assert e.value.code == -1
    s.close()
    # a partitioned solver
    comm = pkg.capi.Comm.solo(0, 2)
    s = pkg.capi.solver_from_scene(ctx, sc, comm)
    with pytest.raises(AAError, match="bending needs one rank") as e:
        s.initialize(pkg.capi.settings_from_scene(sc))
    assert e.value.code == -1 and "2 ranks" in str(e.value)
    s.close()
    comm.close()
    # after initialize; k_bend = 0; both leave the solver as it was
    s = pkg.capi.solver_from_scene(ctx, sc)
    tris = sc.bending[0][0]
    with pytest.raises(AAError, match="k_bend") as e:
        s.add_bending(sc.rest_x, tris, 0.0)
    assert e.value.code == -1
    with pytest.raises(AAError, match="triangle 1.*out of range") as e:
        s.add_bending(sc.rest_x, np.array([[0, 1, 6], [1, 0, sc.n_nodes]], np.int32), 1.0)
    assert e.value.code == -1
    s.initialize(pkg.capi.settings_from_scene(sc))
    n = s.runtime().n_elements
    with pytest.raises(AAError, match="after initialize") as e:
        s.add_bending(sc.rest_x, tris, 1e-2)
    assert e.value.code == -2
    s.step()
    assert s.runtime().n_elements == n and np.isfinite(s.x).all()
    s.close()
    # a list without an interior edge: an empty group, 0 hinges, and the solver runs
    s = pkg.capi.solver_from_scene(ctx, dataclasses.replace(sc, bending=None))
    assert s.add_bending(sc.rest_x, tris[:1], 1e-2) == 0
    assert s.add_bending(sc.rest_x, tris, 1e-2) == len(bc.hinges(sc.rest_x, tris, 1e-2)[0])
    s.initialize(pkg.capi.settings_from_scene(sc))
    s.step()
    assert np.array_equal(s.x, _run(pkg, ctx, sc)[0]["x"])
    s.close()
