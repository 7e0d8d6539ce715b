"""CPU: the references of tests/anderson_cases.py against the reference's own AndersonAcceleration
class (tests/golden/anderson.npz, made by tests/golden/make_golden_anderson.py from three chains of
init + compute), against what Anderson acceleration is (GMRES on a linear map), and the case
tables' own precondition (well-conditioned normal equations on the non-degenerate chains)."""
import numpy as np
import pytest

import anderson_cases as ac

GOLDEN_TOL = ac.GOLDEN_TOL
golden = ac.golden
needs_ld = pytest.mark.skipif(not ac.HAVE_LONGDOUBLE, reason="np.longdouble is not wider than float64 here")


def rebuild(m, eff, u0, G, u, k):
    """The class's state before call k, from the (G_i, u_i) pairs alone: column (i - 1) % m holds
    (F_i - F_{i-1}) / |.| and G_i - G_{i-1} of call i, the open column -F_{k-1} and -G_{k-1}."""
    dim = G.shape[1]
    us = np.vstack([u0[None], u])
    F = G[:, :eff] - us[:-1, :eff]
    st = ac.clean_state(m, eff, dim - eff, eff, us[k])
    if k == 0:
        return st
    mk, col = min(m, k), (k - 1) % m
    done = []
    for i in range(k - mk + 1, k):
        c = (i - 1) % m
        d = -F[i - 1] + F[i]
        s = max(ac.SCALE_EPS, float(np.sqrt(d @ d)))
        st["dF"][c], st["dG"][c], st["scale"][c] = d / s, -G[i - 1] + G[i], s
        done.append(c)
    for a in done:
        for b in done:
            st["M"][a, b] = st["dF"][a] @ st["dF"][b]
    st["dF"][col], st["dG"][col] = -F[k - 1], -G[k - 1]
    st.update(aa_iter=k, aa_col=col)
    return st


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@needs_ld
@pytest.mark.parametrize("name", ["m3", "m6", "m20"])
def test_ref_step_predicts_the_class(name):
    """(a) ref_step out of the rebuilt state gives the class's next iterate. Measured 2.6e-16
    (anderson_cases.GOLDEN_MEASURED; m3 1.8e-16, m6 1.7e-16, m20 2.6e-16); the tolerance is 16 times that."""
    m, eff, u0, G, u = golden()[name]
    assert G.shape[0] == 2 * m + 3
    worst = 0.0
    for k in range(G.shape[0]):
        r = ac.ref_step(rebuild(m, eff, u0, G, u, k), G[k])
        worst = max(worst, rel(u[k], r.u.astype(np.float64)))
    print(f"{name}: worst relative deviation {worst:.3e}")
    assert worst <= GOLDEN_TOL


@pytest.mark.parametrize("name", ["m3", "m6", "m20"])
def test_port_step_follows_the_class(name):
    """(b) the float64 port run as a chain over the same G reproduces the class's u sequence."""
    m, eff, u0, G, u = golden()[name]
    st = ac.clean_state(m, eff, G.shape[1] - eff, eff, u0)
    worst = 0.0
    for k in range(G.shape[0]):
        uk, st = ac.port_step(st, G[k])
        worst = max(worst, rel(uk, u[k]))
    print(f"{name}: worst relative deviation {worst:.3e}")
    assert worst <= GOLDEN_TOL


@needs_ld
@pytest.mark.parametrize("d,m", [(4, 4), (6, 8), (9, 12)])
def test_ref_step_is_gmres_on_a_linear_map(d, m):
    """(c) on a d-dimensional linear map with m >= d, Anderson acceleration is GMRES: the residual
    |G(u) - u| falls by ten orders within d + 1 steps."""
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d))
    A *= 0.9 / np.linalg.norm(A, 2)
    b = rng.standard_normal(d)
    st = ac.clean_state(m, d, 0, d, rng.standard_normal(d))
    res0 = np.linalg.norm(A @ st["cur"] + b - st["cur"])
    for _ in range(d + 1):
        st = ac.ref_step(st, A @ st["cur"] + b).next
    res = np.linalg.norm(A @ st["cur"] + b - st["cur"])
    print(f"d={d} m={m}: {res0:.3e} -> {res:.3e}")
    assert res <= 1e-10 * res0


def _chain_key(c):
    return (c.dim, c.na, c.eff, c.m, c.mask, c.kind, c.seed)


_UNIQUE = {}
for _c in ac.CASES:
    if not _c.degenerate:
        _UNIQUE.setdefault(_chain_key(_c), _c)


@needs_ld
@pytest.mark.parametrize("case", list(_UNIQUE.values()), ids=lambda c: c.name)
def test_case_chains_are_well_conditioned(case):
    """(d) every non-degenerate case keeps cond_2(M) <= 1e6 along its reference chain, so theta is
    well defined where the GPU test compares it; the chain's outputs stay finite."""
    worst = 0.0
    for st, G, r in ac.reference_chain(case):
        assert np.all(np.isfinite(r.next["cur"]))
        if r.mk > 1:
            worst = max(worst, float(np.linalg.cond(r.M[:r.mk, :r.mk])))
    assert worst <= ac.COND_MAX, worst


def test_case_table_reaches_every_edge():
    """The table holds what it was written for: every dim, window and instantiation of the issue."""
    cs = ac.CASES
    assert {1, 63, 64, 257, 511, 512, 513, 1537} <= {c.dim for c in cs}
    assert {1, 2, 5, 6, 7, 8, 10, 12, 16, 17, 20, 32} <= {c.m for c in cs}
    assert {ac.mix_instance(c.m, c.narrow) for c in cs} == {6, 7, 8, 12, 16, 32}
    for m in (c.m for c in cs if c.m <= 7):
        assert {c.narrow for c in cs if c.m == m} == {True, False}, m
    for m in (c.m for c in cs if c.m > 16):
        assert {c.rows for c in cs if c.m == m} == {True, False}, m
    assert {c.nblocks for c in cs} >= {0, 1, 3, 8}
    assert any(c.inplace and c.nb == 0 and c.eff == c.dim for c in cs)
    assert any(c.nb > 0 and c.eff == c.na for c in cs) and any(c.nb > 0 and c.eff == c.dim for c in cs)
    assert any(c.eff < c.na for c in cs)
    assert any(c.mask == ac.EMPTY for c in cs) and any(c.mask not in (ac.EMPTY, ac.FULL_MASK) for c in cs)
    assert {c.kind for c in cs} == {"chain", "reset", "repeat", "twin"}
    for c in cs:   # a mask's windows lie in the second segment and are disjoint
        lo1, hi1, lo2, hi2 = c.mask
        if c.mask not in (ac.EMPTY, ac.FULL_MASK):
            assert 0 <= lo1 < hi1 < lo2 < hi2 <= c.nb and c.eff == c.dim, c.name
