"""GPU: with the concurrent combined-residual pass on, iteration `it` keeps its
working u in the parity buffer du_at(it): the gradient pass writes it there, the reject branch reads
default_u of it - 1 from the other buffer and writes this one, and neither the default_u copy in the
window beside the pass's local step nor the restore of u on a reject exists any more. No operand
and no order of summation changes: every run here is bit-identical to the layout AA_Z_WINDOW=0
restores (u in a buffer of its own), and to the in-line (AA_CONCURRENT=0) and sequential
(AA_Z_PIPELINE=0) orders."""
import numpy as np
import pytest

import varmat_cases
from golden_io import scenes

pytestmark = pytest.mark.gpu

KEYS = ("prim", "comb", "reject", "x", "v", "iterations", "rejects")


def run(capi, ctx, sc):
    got, s = capi.run_scene(ctx, sc)
    s.close()
    return got


def assert_equal(want, got, tag):
    assert len(want) == len(got), tag
    for k, (a, b) in enumerate(zip(want, got)):
        for key in KEYS:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (tag, k, key, len(a["comb"]), len(b["comb"]))


def test_gpu_z_window_rejects_taken(pkg, ctx, monkeypatch):
    """8 000 tets (the recipe of the golden drop20_z_nh_aa6_rej), rejects in both steps: the reject
    branch reads default_u where it lies and writes the other parity buffer."""
    sc = scenes.tet_drop(20, 8, 10, iters=100, n_steps=2)
    want = run(pkg.capi, ctx, sc)
    for st in want:
        assert int(np.sum(st["reject"])) >= 1 and st["rejects"] >= 1
    for knob in ("AA_Z_WINDOW", "AA_CONCURRENT", "AA_Z_PIPELINE"):
        with monkeypatch.context() as m:
            m.setenv(knob, "0")
            assert_equal(want, run(pkg.capi, ctx, sc), knob)


@pytest.mark.parametrize("iters", [1, 2, 3, 4])
def test_gpu_z_window_short_steps(iters, pkg, ctx, monkeypatch):
    """One to four iterations: no pass forked (1), one pass and the last one in line (2), both
    parities of the alternating buffers as source and target of a step's u (3, 4)."""
    sc = scenes.tet_drop(6, 4, 4, iters=iters, n_steps=2)
    want = run(pkg.capi, ctx, sc)
    assert all(len(st["comb"]) == iters for st in want)
    monkeypatch.setenv("AA_Z_WINDOW", "0")
    assert_equal(want, run(pkg.capi, ctx, sc), iters)


def run_to_eps_matches_capped(capi, ctx, sc, eps, k):
    """A step that stops at comb_k <= eps * comb_0 is bit-identical to one capped at k + 1 iterations
    from the same state: history, positions, velocities."""
    a = capi.solver_from_scene(ctx, sc)
    a.initialize(capi.settings_from_scene(sc))
    a.set_iterations(sc.iters, eps)
    b = capi.solver_from_scene(ctx, sc)
    b.initialize(capi.settings_from_scene(sc))
    b.set_iterations(k + 1, 0.0)
    a.step()
    b.step()
    ha, hb, ta = a.history(), b.history(), a.times()
    assert len(ha["comb"]) == k + 1 == a.runtime().iterations, (k, len(ha["comb"]), a.runtime().iterations)
    for key in ("prim", "comb", "reject"):
        assert np.array_equal(ha[key], hb[key]), (k, key)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.v, b.v), k
    assert a.runtime().rejects == b.runtime().rejects, k
    assert len(ta) == k + 1 and np.all(ta > 0) and np.all(np.diff(ta) > 0)
    a.close(); b.close()


@pytest.mark.parametrize("window", ["1", "0"])
def test_gpu_z_window_breaks_found_by_concurrent_pass(window, pkg, ctx, monkeypatch):
    """A break at comb_k is found by the pass that runs beside iteration k + 1, which by then has
    written its u into the other parity buffer: the step still ends as if it had stopped at k --
    at the first running minimum, at an odd and an even k (either buffer holding the speculative
    iteration's u) and at the last one."""
    monkeypatch.setenv("AA_Z_WINDOW", window)
    sc = scenes.tet_drop(6, 4, 4, iters=40, n_steps=1)
    comb = run(pkg.capi, ctx, sc)[0]["comb"]
    R = [k for k in range(1, len(comb)) if comb[k] < comb[:k].min()]
    odd, even = [k for k in R if k % 2 == 1], [k for k in R if k % 2 == 0]
    assert odd and even, R
    for k in sorted({R[0], odd[len(odd) // 2], even[len(even) // 2], R[-1]}):
        run_to_eps_matches_capped(pkg.capi, ctx, sc, comb[k] / comb[0] * (1 + 1e-12), k)


def test_gpu_z_window_pinned(pkg, ctx, monkeypatch):
    """The Z-variant NeoHookean cantilever of the golden cantilever_z_nh_aa6: pinned nodes, Cp != 0."""
    sc = scenes.cantilever(20, 4, 5, scenes.NEOHOOKEAN, iters=50, n_steps=1)
    assert len(sc.pin_idx) > 0
    want = run(pkg.capi, ctx, sc)
    monkeypatch.setenv("AA_Z_WINDOW", "0")
    assert_equal(want, run(pkg.capi, ctx, sc), "pinned")


def test_gpu_z_window_per_element(pkg, ctx, monkeypatch):
    """One group with per-element Lame parameters (aa_elastic_add_tets_var): the per-element
    instantiation of the gradient / dual-ascent kernel with separate input and output u."""
    sc = varmat_cases.cases()["drop6_z_nh_aa6"]
    assert len(sc.groups) == 1 and sc.groups[0].per_element
    want = run(pkg.capi, ctx, sc)
    monkeypatch.setenv("AA_Z_WINDOW", "0")
    assert_equal(want, run(pkg.capi, ctx, sc), "per-element")
