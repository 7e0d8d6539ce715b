"""CPU: per-element material parameters (aa_elastic_add_*_var). The scene helpers, the fixtures of
tests/golden/varmat/ (the reference's own runs of one EnergyTerm per element, each with its Lame;
tests/golden/make_golden_varmat.py), the oracle against them, and the C++ facade's overloads."""
import os

import numpy as np
import pytest

import varmat_cases
from conftest import REPO
from golden_io import compare, scenes
from test_facade import build

FACADE_SRC = os.path.join(REPO, "tests", "cpp", "facade_varmat.cpp")


def test_with_material_levels_assigns_seeded_levels():
    base = scenes.cloth(4, 4)
    lv = varmat_cases.CLOTH_LEVELS
    sc = scenes.with_material_levels(base, **lv)
    (g,) = sc.groups
    n = len(base.groups[0].idx)
    lvl = np.random.default_rng(7).integers(0, 8, n)
    assert g.per_element and not base.groups[0].per_element
    assert np.array_equal(g.E, lv["E_levels"][lvl]) and np.array_equal(g.nu, lv["nu_levels"][lvl])
    assert np.array_equal(g.limit_min, lv["lmin_levels"][lvl]) and np.array_equal(g.limit_max, lv["lmax_levels"][lvl])
    assert np.array_equal(g.idx, base.groups[0].idx) and base.groups[0].E == 50.0   # the input scene is untouched
    assert len(set(lvl)) > 1
    other = scenes.with_material_levels(base, **lv, seed=8)
    assert not np.array_equal(other.groups[0].E, g.E)
    # tets: the limits keep the group's scalars
    t = scenes.with_material_levels(scenes.cantilever(2, 1, 1), **varmat_cases.TET_LEVELS)
    assert np.ndim(t.groups[0].limit_min) == 0 and t.groups[0].limit_max == 100.0
    with pytest.raises(ValueError):
        scenes.with_material_levels(scenes.beams(1), **varmat_cases.TET_LEVELS)   # three groups
    with pytest.raises(ValueError):
        scenes.with_material_levels(base, lv["E_levels"], lv["nu_levels"][:5])


def test_per_element_groups_counts_order_values():
    sc = scenes.with_material_levels(scenes.cloth(3, 2), **varmat_cases.CLOTH_LEVELS)
    (g,) = sc.groups
    ex = scenes.per_element_groups(sc)
    assert len(ex.groups) == len(g.idx) == ex.n_elements() == sc.n_elements()
    for e, h in enumerate(ex.groups):
        assert h.kind == g.kind and h.material == g.material and not h.per_element
        assert h.idx.shape == (1, 3) and np.array_equal(h.idx[0], g.idx[e])
        assert (h.E, h.nu, h.limit_min, h.limit_max) == (g.E[e], g.nu[e], g.limit_min[e], g.limit_max[e])
    assert ex.x is sc.x and ex.iters == sc.iters and len(sc.groups) == 1
    # mixed scene: a uniform group expands with its scalars, group order kept
    b = scenes.beams(1)
    b.groups[1].E = np.linspace(1e6, 1e7, len(b.groups[1].idx))
    eb = scenes.per_element_groups(b)
    n0, n1 = len(b.groups[0].idx), len(b.groups[1].idx)
    assert len(eb.groups) == b.n_elements()
    assert [h.material for h in eb.groups[:n0]] == [b.groups[0].material] * n0
    assert [h.E for h in eb.groups[n0:n0 + n1]] == list(b.groups[1].E) and eb.groups[0].E == 1e7
    assert all(h.nu == 0.399 for h in eb.groups)
    with pytest.raises(ValueError):
        b.groups[1].E = np.ones(3)
        scenes.per_element_groups(b)


@pytest.mark.parametrize("name", varmat_cases.names())
def test_fixture_shapes_and_inputs(name):
    sc, ref = varmat_cases.load(name)
    want = varmat_cases.cases()[name]
    (g,), (w,) = sc.groups, want.groups
    n = len(g.idx)
    for a, b in zip(g.material_arrays(), w.material_arrays()):
        assert a.shape == (n,) and np.array_equal(a, b)
    assert len(np.unique(g.E)) == 8
    assert np.array_equal(g.idx, w.idx) and np.array_equal(sc.x, want.x) and np.array_equal(sc.masses, want.masses)
    assert (g.kind, g.material, sc.variant, sc.iters, sc.n_steps, sc.aa_m) == (w.kind, w.material, want.variant,
                                                                              want.iters, want.n_steps, want.aa_m)
    assert len(ref) == sc.n_steps == 2
    for st in ref:
        k = len(st["prim"])
        assert 0 < k <= sc.iters and len(st["comb"]) == len(st["reject"]) == k
        assert st["x"].shape == st["v"].shape == (sc.n_nodes, 3)
        assert all(np.isfinite(st[key]).all() for key in ("prim", "comb", "x", "v"))
    # the recorded Anderson rejects: none on the tets, 0 + 4 on the cloth
    assert [int(np.sum(st["reject"])) for st in ref] == ([0, 4] if name.startswith("cloth") else [0, 0])
    assert os.path.getsize(os.path.join(varmat_cases.VARMAT, name + ".npz")) < 100 << 10


@pytest.mark.parametrize("name", varmat_cases.names())
def test_oracle_matches_reference_per_element(name, oracle):
    sc, ref = varmat_cases.load(name)
    got = oracle.run_elastic(scenes.per_element_groups(sc))
    assert [len(s["prim"]) for s in got] == [len(s["prim"]) for s in ref]
    got[-1]["x"] = got[-1]["x"].reshape(-1, 3)
    tol = varmat_cases.TOL[name]
    fails = compare(ref, got, tol, tol)
    assert not fails, fails


def test_facade_varmat_builds(tmp_path):
    build(str(tmp_path / "facade_varmat"), FACADE_SRC)
