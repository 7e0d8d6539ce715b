"""GPU: the combined-residual pass folds its residual into its local step: for
hyperelastic tet groups without pins the work-queue kernel forms k_prim_z's two sums per element
where it used to store z_c, and k_prim_sum turns them into the block partials -- the same
statements in the same order, the same thread-to-element layout and block sum, so `comb`, the break
test and the epsilon stop see the same bits. Every other group keeps local step + k_prim_z, into the
same partial ranges. Each run here is compared with AA_COMB_FUSED=0 (the two-kernel path) by
np.array_equal: no tolerance."""
import dataclasses

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


def fused_matches_unfused(pkg, ctx, monkeypatch, sc, tag, extra=()):
    """The default run and the AA_COMB_FUSED=0 run of `sc` (both with the knobs `extra` set to 0)."""
    with monkeypatch.context() as m:
        for knob in extra:
            m.setenv(knob, "0")
        want = run(pkg.capi, ctx, sc)
        m.setenv("AA_COMB_FUSED", "0")
        assert_equal(want, run(pkg.capi, ctx, sc), tag)
    return want


@pytest.mark.parametrize("dims", [(1, 1, 2), (7, 5, 3)])
def test_gpu_comb_fused_small_and_partial_blocks(dims, pkg, ctx, monkeypatch):
    """10 tets: less than one wave, most lanes never hold an element. 525 tets: several blocks of
    partials, the last one partial."""
    sc = scenes.tet_drop(*dims, iters=12, n_steps=2)
    assert sc.n_elements() == 5 * dims[0] * dims[1] * dims[2]
    fused_matches_unfused(pkg, ctx, monkeypatch, sc, dims)


@pytest.mark.parametrize("iters", [1, 2, 3, 4])
def test_gpu_comb_fused_short_steps(iters, pkg, ctx, monkeypatch):
    """One to four iterations: no pass forked (1: the in-line tail alone), one pass plus the tail
    (2), both parities of the default_z / default_u buffers the pass reads (3, 4)."""
    sc = scenes.tet_drop(6, 4, 4, iters=iters, n_steps=2)
    want = fused_matches_unfused(pkg, ctx, monkeypatch, sc, iters)
    assert all(len(st["comb"]) == iters for st in want)


@pytest.mark.parametrize("extra", [(), ("AA_CONCURRENT",), ("AA_Z_PIPELINE",)])
def test_gpu_comb_fused_rejects_taken(extra, pkg, ctx, monkeypatch):
    """8 000 tets (the recipe of the golden drop20_z_nh_aa6_rej), rejects in both steps: the pass on
    the side stream, in line, and in the sequential order."""
    sc = scenes.tet_drop(20, 8, 10, iters=100, n_steps=2)
    want = fused_matches_unfused(pkg, ctx, monkeypatch, sc, extra, extra)
    for st in want:
        assert int(np.sum(st["reject"])) >= 1 and st["rejects"] >= 1


def eps_run(capi, ctx, sc, iters, eps):
    s = capi.solver_from_scene(ctx, sc)
    s.initialize(capi.settings_from_scene(sc))
    s.set_iterations(iters, eps)
    s.step()
    h = s.history()
    out = dict(prim=h["prim"], comb=h["comb"], reject=h["reject"], x=np.array(s.x), v=np.array(s.v),
               iterations=s.runtime().iterations, rejects=s.runtime().rejects)
    s.close()
    return out


def test_gpu_comb_fused_eps_stop_mid_step(pkg, ctx, monkeypatch):
    """A step that stops at comb_k <= eps * comb_0, the break found by the concurrent pass from the
    fused sums: it is bit-identical to a twin capped at k + 1 iterations, and to the same stop with
    AA_COMB_FUSED=0 -- at an odd and an even k."""
    sc = scenes.tet_drop(6, 4, 4, iters=40, n_steps=1)
    comb = run(pkg.capi, ctx, sc)[0]["comb"]
    R = [k for k in range(1, len(comb)) if comb[k] < comb[:k].min()]
    odd, even = [k for k in R if k % 2 == 1], [k for k in R if k % 2 == 0]
    assert odd and even, R
    for k in (odd[len(odd) // 2], even[len(even) // 2]):
        assert k + 1 < sc.iters
        eps = comb[k] / comb[0] * (1 + 1e-12)
        a = eps_run(pkg.capi, ctx, sc, sc.iters, eps)
        b = eps_run(pkg.capi, ctx, sc, k + 1, 0.0)
        assert len(a["comb"]) == k + 1 == a["iterations"], (k, len(a["comb"]), a["iterations"])
        assert_equal([a], [b], ("capped", k))
        with monkeypatch.context() as m:
            m.setenv("AA_COMB_FUSED", "0")
            assert_equal([a], [eps_run(pkg.capi, ctx, sc, sc.iters, eps)], ("unfused", k))


def test_gpu_comb_fused_per_element(pkg, ctx, monkeypatch):
    """One group with per-element Lame parameters: the GroupVar instantiation of the residual form."""
    sc = varmat_cases.cases()["drop6_z_nh_aa6"]
    assert len(sc.groups) == 1 and sc.groups[0].per_element
    fused_matches_unfused(pkg, ctx, monkeypatch, sc, "per-element")


def test_gpu_comb_fused_pinned_falls_back(pkg, ctx, monkeypatch):
    """The Z-variant NeoHookean cantilever of the golden cantilever_z_nh_aa6: a group with pinned
    nodes keeps the plain queue + k_prim_z whatever the knob says."""
    sc = scenes.cantilever(20, 4, 5, scenes.NEOHOOKEAN, iters=50, n_steps=1)
    assert len(sc.pin_idx) > 0
    fused_matches_unfused(pkg, ctx, monkeypatch, sc, "pinned")


def test_gpu_comb_fused_mixed_groups(pkg, ctx, monkeypatch):
    """Three groups over one free-falling block: NeoHookean (fused), linear tets (no queue: local step
    + k_prim_z), NeoHookean again (fused). The group sizes are no multiples of the block, so each
    group's partials start where the previous group's partial block ended: the offsets of fused and
    fallback groups line up, before and after one another."""
    sc = scenes.tet_drop(6, 4, 4, iters=30, n_steps=2)
    (g,) = sc.groups
    a, b = 300, 390
    assert 0 < a < b < len(g.idx) and a % 256 and (b - a) % 256 and (len(g.idx) - b) % 256
    parts = [dataclasses.replace(g, idx=g.idx[:a].copy()),
             dataclasses.replace(g, material=scenes.LINEAR, idx=g.idx[a:b].copy()),
             dataclasses.replace(g, idx=g.idx[b:].copy())]
    sc = dataclasses.replace(sc, groups=parts)
    fused_matches_unfused(pkg, ctx, monkeypatch, sc, "mixed")
