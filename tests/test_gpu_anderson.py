"""GPU: the Anderson step's kernels (k_aa_reduce<8|12|16|32>, k_aa_reduce_cols<32>, k_aa_solve,
k_aa_mix<6|7|8|12|16|32> in csrc/elastic_kernels.hip) one step at a time against a long-double
restatement of AndersonAcceleration::compute_impl (tests/anderson_cases.ref_step), through the hook
aa_test_anderson_step (capi.hook_anderson_step), which runs the solvers' own launch_aa_reduce ->
launch_aa_solve -> launch_aa_mix on an uploaded state and hands back all they can write.

A case (anderson_cases.CASES) is a chain of T = 2 m + 3 steps -- the ring wraps twice -- of
G_k = A u_k + b with u_k the device's previous output and |A|_2 = 0.9; the device's output state is
the next input. Every assertion is against ref_step of the device's own input state, so neither
drift nor the conditioning of theta enters the sums or the mix. With u = 2^-53, per step:

  reduce  tot_dev = the block partials summed over blocks in long double;
          |tot_dev[t] - tot_ref[t]| <= (n_in + nblocks + 8) u S_t on every live slot, S_t the sum of
          |a_i| |b_i| (first order, any summation order: one rounding each for F and dF_j + F, one a
          product, one an add); dead slots (c >= mk, c == col) exactly 0 in every block; copy_to == G.
  solve   from the partials summed in double in k_aa_solve's own order (chunk c sums blocks c,
          c + NCH, ..; then the chunks in order): scale[col] = max(1e-14, sqrt(tot_0)), M[c, col] =
          M[col, c] = tot[2 + c] / s, M[col, col] = tot_0 / s^2 within 4 u relative; every other entry
          of M and scale bitwise the input; the ring's integers exact; on the first call only the
          flags change.
  theta   non-degenerate chains, mk > 1: coef * scale against the mpmath solution of the device's own
          M and b, atol 1e-6 max(1, |theta|) (test_gpu_element_tables' COD tolerance); mk == 1: the
          closed form within 8 u relative.
  mix     from the device's own coef: out_i within (mk + 3) u (|g_i| + sum_c |d_c,i coef_c|) of
          g_i - sum_c d_c,i coef_c (d the old dG with + g in column j); dG_j = fl(dG_j + g), dF_jn =
          -F (i < eff), dG_jn = -G exactly; dF_j within 4 u relative of (dF_j + F) / s (F = fl(g -
          cur), as the next column stores it); cur == out; every other column bitwise the input; on
          the first call out == G.

Reset chains zero aa_iter and aa_col after step m + 1 and leave the stale history: from there on
they are bitwise a chain started from a clean state. Degenerate chains (G repeated exactly; two
identical history columns) are checked alike but for theta, and must stay finite. With done,
aa_skip or !aa_active every output is bitwise the input.

AA_TEST_ANDERSON_DUMP=<file> appends one JSON line per case (the worst ratio of each bound).

Measured on one MI355X, the worst ratio value / bound over each family's cases (theta: the
mk == 1 closed form's 8 u bound; against the 1e-6 tolerance of the mk > 1 solve the ratio is below
5e-5 everywhere; 60 tests, 10 s in all):

    family                              cases   reduce   solve   theta   mix    dF_j
    m <= 16                                25   0.012    0.37    0.24    0.54   0.50
    m > 16, column-parallel reduce          7   0.0013   0.36    0.09    0.50   0.49
    m > 16, row-parallel reduce             5   0.0006   0.35    0.16    0.46   0.47
    reset                                   3   0.0013   0.32    0.17    0.37   0.44
    degenerate                              4   0.0012   0.32    0.08    0.35   0.43
    the class's recorded chains             3   largest relative deviation 2.5e-16 of GOLDEN_TOL 4.2e-15

(The reduce bound is a worst case over any summation order, n u S; the kernels' pairwise wave and
block sums stay two orders below it, while one dropped O(1) entry is 1e13 above.)

Sensitivity (one-off, arithmetic-only mutations of elastic_kernels.hip, one at a time; tests of
this file's 60 that fail): dF strided by dim instead of eff in the two reduce kernels (the hook's dF
buffer padded to m x dim for that run, so that no read left it) 13; `c != col` dropped from the
column products 44; aa_jn = col instead of (col + 1) % m 44; the last chunk left out of k_aa_solve's
sum 5 -- the five cases with more blocks than NCH whose last chunk owns rows, added for it: none of
the issue's dims (at most 7 blocks) reaches that chunk; wave 0's zero-fill removed in
k_aa_reduce_cols 10.
"""
import json
import os

import numpy as np
import pytest

import anderson_cases as ac
from anderson_cases import LD, U

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ac.HAVE_LONGDOUBLE,
                                 reason="np.longdouble is not wider than float64 here: no high-precision reference")]

SENTINEL = -1.2345678901234567e+123
KBLOCK, SOLVE_THREADS = 256, 1024   # common.hpp kBlock; k_aa_solve's chunk layout (kSolveThreads1024)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def call(pkg, ctx, case, st, G, **over):
    dim = case.dim
    kw = dict(nblocks=case.nblocks, inplace=case.inplace, narrow=case.narrow, rows=case.rows,
              copy_to=np.full(dim, SENTINEL) if case.copy_to else None, out=None if case.inplace else np.full(dim, SENTINEL))
    kw.update(over)
    try:
        return pkg.capi.hook_anderson_step(ctx, st, G, **kw)
    except pkg.capi.AAError as e:
        if e.code == -3:   # AA_ERR_DEVICE: nothing more may run on a device that has faulted
            pytest.exit(f"device error in {case.name}: {e}", returncode=3)
        raise


def solve_sum(red):
    """The block partials summed in double as k_aa_solve does."""
    nb, nval = red.shape
    nch = SOLVE_THREADS // nval
    tot = np.zeros(nval)
    for c in range(nch):
        s = np.zeros(nval)
        for b in range(c, nb, nch):
            s = s + red[b]
        tot = tot + s
    return tot


class Worst:
    def __init__(self):
        self.r = dict(reduce=0.0, solve=0.0, theta1=0.0, theta=0.0, mix=0.0, dFj=0.0)

    def see(self, key, value, bound):
        """value <= bound elementwise; remembers the largest ratio."""
        value, bound = np.atleast_1d(np.asarray(value, LD)), np.atleast_1d(np.asarray(bound, LD))
        nz = bound > 0
        if np.any(nz):
            self.r[key] = max(self.r[key], float(np.max(value[nz] / bound[nz])))
        return bool(np.all(value <= bound))


def check_launch(case, res):
    """The step ran the instantiation the case was written for."""
    bucket = ac.window_bucket(case.m)
    assert res["bucket"] == bucket, (case.name, res["bucket"])
    assert res["cols"] == (-1 if bucket != 32 else 0 if case.rows else 1), (case.name, res["cols"])
    assert res["nblocks"] == (case.nblocks or min(512, (case.dim + KBLOCK - 1) // KBLOCK)), (case.name, res["nblocks"])
    assert res["red"].shape == (res["nblocks"], 2 + 2 * bucket)


def check_step(case, st, G, res, worst, theta=True):
    """Every output of one step against ref_step of its input state."""
    tag = f"{case.name} iter {st['aa_iter']}"
    m, eff, dim = case.m, case.eff, case.dim
    MM = ac.window_bucket(m)
    check_launch(case, res)
    r = ac.ref_step(st, G, solve=False)
    out = res["cur"] if case.inplace else res["out"]
    for k in ("cur", "dF", "dG", "scale", "M", "coef", "red"):
        assert np.all(np.isfinite(res[k])), (tag, k)
    assert np.all(np.isfinite(out)), tag
    if case.copy_to:
        assert same(res["copy_to"], G), tag
    for k in ("aa_skip", "aa_active", "done"):
        assert res[k] == st[k], (tag, k)
    F64 = G[:eff] - st["cur"][:eff]
    keep = np.ones(m, bool)     # history columns the step must not touch
    if r.first:
        assert same(out, G) and same(res["cur"], out), tag
        assert not res["red"].any(), tag
        assert (res["aa_iter"], res["aa_col"], res["aa_first"], res["aa_j"], res["aa_jn"], res["aa_mk"]) == (1, st["aa_col"], 1, 0, 0, 0), tag
        for k in ("scale", "M", "coef"):
            assert same(res[k], st[k]), (tag, k)
        assert res["aa_s"] == st["aa_s"], tag
        assert same(res["dF"][0], -F64) and same(res["dG"][0], -G), tag
        keep[0] = False
        assert same(res["dF"][keep], st["dF"][keep]) and same(res["dG"][keep], st["dG"][keep]), tag
        return
    mk, col, jn = r.mk, r.col, r.jn
    # ---- reduce
    red = res["red"]
    tot_dev = red.astype(LD).sum(axis=0)
    assert not red[:, ~r.live].any(), (tag, "dead slots")
    bound = (r.n_in + res["nblocks"] + 8) * U * r.S
    assert worst.see("reduce", np.abs(tot_dev - r.tot)[r.live], bound[r.live]), (tag, "reduce", np.abs(tot_dev - r.tot)[r.live] / bound[r.live])
    # ---- solve bookkeeping, from the device's own sums
    tot = solve_sum(red).astype(LD)
    s_ref = max(LD(ac.SCALE_EPS), np.sqrt(tot[0]))
    s = res["scale"][col]
    assert worst.see("solve", abs(LD(s) - s_ref), 4 * U * s_ref), (tag, "scale")
    assert res["aa_s"] == s, tag
    Mref, changed = st["M"].astype(LD), np.zeros((m, m), bool)
    b = np.zeros(mk, LD)
    for c in range(mk):
        if c != col:
            Mref[c, col] = Mref[col, c] = tot[2 + c] / LD(s)
            b[c] = tot[2 + MM + c]
        changed[c, col] = changed[col, c] = True
    Mref[col, col] = tot[0] / (LD(s) * LD(s))
    b[col] = tot[1] / LD(s)
    assert worst.see("solve", np.abs(res["M"].astype(LD) - Mref)[changed], (4 * U * np.abs(Mref))[changed]), (tag, "M")
    assert same(res["M"][~changed], st["M"][~changed]), (tag, "M elsewhere")
    assert same(res["M"], res["M"].T), (tag, "M symmetric")
    others = np.arange(m) != col
    assert same(res["scale"][others], st["scale"][others]), (tag, "scale elsewhere")
    assert same(res["coef"][mk:], st["coef"][mk:]), (tag, "coef past mk")
    got = (res["aa_iter"], res["aa_col"], res["aa_first"], res["aa_j"], res["aa_jn"], res["aa_mk"])
    assert got == (st["aa_iter"] + 1, jn, 0, col, jn, mk), (tag, got)
    # ---- theta
    th_dev = res["coef"][:mk] * res["scale"][:mk]
    if mk == 1:
        sq = tot[0] / (LD(s) * LD(s))
        th = (tot[1] / LD(s)) / sq if np.sqrt(sq) > ac.SCALE_EPS else LD(0)
        assert worst.see("theta1", abs(LD(th_dev[0]) - th), 8 * U * abs(th)), (tag, "theta", th_dev, th)
    elif theta:
        th = ac.mp_solve(res["M"][:mk, :mk], b.astype(np.float64))
        assert worst.see("theta", np.max(np.abs(th_dev - th)), 1e-6 * max(1.0, float(np.linalg.norm(th)))), (tag, "theta")
    # ---- mix, from the device's own coefficients
    g = G.astype(LD)
    d = st["dG"][:mk].astype(LD)
    d[col] += g
    coef = res["coef"][:mk].astype(LD)
    want = g - coef @ d
    bound = (mk + 3) * U * (np.abs(g) + np.abs(coef) @ np.abs(d))
    assert worst.see("mix", np.abs(out.astype(LD) - want), bound), (tag, "mix", float(np.max(np.abs(out.astype(LD) - want) / bound)))
    assert same(res["cur"], out), tag
    if jn != col:
        assert same(res["dG"][col], st["dG"][col] + G), (tag, "dG_j")
        dfj = (st["dF"][col].astype(LD) + F64.astype(LD)) / LD(res["aa_s"])
        assert worst.see("dFj", np.abs(res["dF"][col].astype(LD) - dfj), 4 * U * np.abs(dfj)), (tag, "dF_j")
    assert same(res["dF"][jn], -F64) and same(res["dG"][jn], -G), (tag, "the next column")
    keep[[col, jn]] = False
    assert same(res["dF"][keep], st["dF"][keep]) and same(res["dG"][keep], st["dG"][keep]), (tag, "other columns")


def report(case, worst, steps):
    rec = dict(case=case.name, steps=steps, **{k: round(v, 4) for k, v in worst.r.items()})
    print(json.dumps(rec))
    if os.environ.get("AA_TEST_ANDERSON_DUMP"):
        with open(os.environ["AA_TEST_ANDERSON_DUMP"], "a") as f:
            f.write(json.dumps(rec) + "\n")


def next_state(res):
    return ac.copy_state(res)


CHAINS = [c for c in ac.CASES if c.kind == "chain"]


@pytest.mark.parametrize("case", CHAINS, ids=lambda c: c.name)
def test_gpu_anderson_chain(pkg, ctx, case):
    f, st, worst = case.map(), case.start(), Worst()
    for k in range(case.T):
        G = f(st["cur"])
        res = call(pkg, ctx, case, st, G)
        check_step(case, st, G, res, worst)
        st = next_state(res)
    assert st["aa_iter"] == case.T and st["aa_col"] == (case.T - 1) % case.m
    report(case, worst, case.T)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.kind == "reset"], ids=lambda c: c.name)
def test_gpu_anderson_reset_leaves_no_trace(pkg, ctx, case):
    """aa_iter = aa_col = 0 after step m + 1, the stale dF, dG, M and scale left in place: every later
    step is bitwise that of a chain started from a clean state at the same iterate."""
    f, st, worst = case.map(), case.start(), Worst()
    for k in range(ac.RESET_AFTER(case.m)):
        G = f(st["cur"])
        res = call(pkg, ctx, case, st, G)
        check_step(case, st, G, res, worst)
        st = next_state(res)
    assert st["aa_iter"] > case.m and np.all(st["scale"] > 0) and np.all(st["M"].diagonal() > 0)   # the ring is full
    st.update(aa_iter=0, aa_col=0)
    clean = ac.clean_state(case.m, case.na, case.nb, case.eff, st["cur"], case.mask)
    for k in range(ac.RESET_AFTER(case.m), case.T):
        G = f(st["cur"])
        res, ref = call(pkg, ctx, case, st, G), call(pkg, ctx, case, clean, G)
        check_step(case, st, G, res, worst)
        mk = res["aa_mk"]
        out, out_ref = (res["cur"], ref["cur"]) if case.inplace else (res["out"], ref["out"])
        assert same(out, out_ref) and same(res["cur"], ref["cur"]) and same(res["red"], ref["red"]), (case.name, k)
        assert same(res["coef"][:mk], ref["coef"][:mk]) and (mk == 0 or res["aa_s"] == ref["aa_s"]), (case.name, k)
        assert all(res[key] == ref[key] for key in ac.CTL), (case.name, k)
        st, clean = next_state(res), next_state(ref)
    for key in ("dF", "dG", "M", "scale", "coef"):   # m + 2 steps later every column has been rewritten
        assert same(st[key], clean[key]), (case.name, key)
    report(case, worst, case.T)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.degenerate], ids=lambda c: c.name)
def test_gpu_anderson_degenerate(pkg, ctx, case):
    """G repeated exactly (dF_j = 0, the scale clamps at 1e-14), or two identical history columns
    (singular normal equations): all but theta is checked, and every output is finite."""
    f, st, worst = case.map(), case.start(), Worst()
    G0 = f(st["cur"])
    clamped = False
    for k in range(case.T):
        if case.kind == "twin" and k == 4:
            st = ac.make_twin(st)
        G = G0 if case.kind == "repeat" else f(st["cur"])
        res = call(pkg, ctx, case, st, G)
        check_step(case, st, G, res, worst, theta=False)
        clamped |= bool(k > 0 and res["aa_s"] == ac.SCALE_EPS)
        if case.kind == "repeat" and k >= 1:
            out = res["cur"] if case.inplace else res["out"]
            assert same(out, G0), (case.name, k)   # the fixed point of a constant map
        st = next_state(res)
    assert clamped == (case.kind == "repeat")
    report(case, worst, case.T)


@pytest.mark.parametrize("gate", ac.GATES)
@pytest.mark.parametrize("name", ["z_d257_m6", "alm_d257_m10_windows", "ux_d512_m17_cols", "ux_d512_m17_rows"])
def test_gpu_anderson_gates(pkg, ctx, name, gate):
    """done, aa_skip or !aa_active: the three kernels return at once -- every output is bitwise the
    input, and out, copy_to and the partials are untouched. On the first call and in mid-chain."""
    case = ac.CASE[name]
    f, st = case.map(), case.start()
    for k in range(4):
        gated = ac.copy_state(st)
        gated[gate] = 0 if gate == "aa_active" else 1
        G = f(st["cur"])
        res = call(pkg, ctx, case, gated, G)
        for key in ("cur", "dF", "dG", "scale", "M", "coef"):
            assert same(res[key], gated[key]), (name, gate, k, key)
        assert all(res[key] == gated[key] for key in ac.CTL) and res["aa_s"] == gated["aa_s"], (name, gate, k)
        assert not res["red"].any()
        if not case.inplace:
            assert np.all(res["out"] == SENTINEL)
        if case.copy_to:
            assert np.all(res["copy_to"] == SENTINEL)
        st = next_state(call(pkg, ctx, case, st, G))


@pytest.mark.parametrize("name", ["m3", "m6", "m20"])
def test_gpu_anderson_follows_the_class(pkg, ctx, name):
    """The reference's own AndersonAcceleration on three recorded chains (tests/golden/anderson.npz):
    the hook fed the same G sequence returns the class's u_k, at the tolerance the CPU test measured
    for ref_step on the same fixtures (anderson_cases.GOLDEN_TOL)."""
    m, eff, u0, G, u = ac.golden()[name]
    dim = G.shape[1]
    case = ac.Case("golden_" + name, dim, eff if eff < dim else dim, eff, m, inplace=eff == dim, copy_to=eff < dim)
    st, worst = ac.clean_state(m, case.na, case.nb, eff, u0), 0.0
    for k in range(G.shape[0]):
        res = call(pkg, ctx, case, st, G[k])
        out = res["cur"] if case.inplace else res["out"]
        worst = max(worst, float(np.max(np.abs(out - u[k])) / np.max(np.abs(u[k]))))
        st = next_state(res)
    rec = dict(case=case.name, worst=worst, tol=ac.GOLDEN_TOL)
    print(json.dumps(rec))
    if os.environ.get("AA_TEST_ANDERSON_DUMP"):
        with open(os.environ["AA_TEST_ANDERSON_DUMP"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert worst <= ac.GOLDEN_TOL


def test_gpu_anderson_hook_refusals(pkg, ctx):
    """The hook's argument checks: 1 <= m <= 32, 0 < eff <= dim, 0 <= aa_col < m, aa_iter >= 0, and
    the in-place form only with one segment."""
    import ctypes as C
    capi = pkg.capi
    case = ac.CASE["ux_d63_m5"]
    st, G = case.start(), case.map()(case.start()["cur"])
    for change in (dict(aa_col=5), dict(aa_col=-1), dict(aa_iter=-1)):
        bad = ac.copy_state(st)
        bad.update(change)
        with pytest.raises(capi.AAError) as e:
            call(pkg, ctx, case, bad, G)
        assert e.value.code == -1, change
    with pytest.raises(capi.AAError) as e:
        call(pkg, ctx, case, st, G, inplace=True, out=None)   # nb > 0
    assert e.value.code == -1
    z = np.zeros(64)
    i9, i3, m4 = np.zeros(9, np.int32), np.zeros(3, np.int32), np.zeros(4, np.int64)
    s = C.c_double(0.0)

    def raw(m, na, nb, eff):
        return capi.lib().aa_test_anderson_step(
            ctx.h, C.c_int(m), C.c_longlong(na), C.c_longlong(nb), C.c_longlong(eff), capi._dp(z), capi._dp(z), capi._dp(z),
            capi._dp(z), capi._ip(i9), capi._dp(z), capi._dp(z), capi._dp(z), C.byref(s),
            m4.ctypes.data_as(C.POINTER(C.c_longlong)), C.c_int(1), C.c_int(0), capi._dp(z), C.c_longlong(64), capi._dp(z),
            None, capi._ip(i3))
    for args in ((0, 1, 0, 1), (33, 1, 0, 1), (1, 1, 0, 0), (1, 1, 0, 2), (1, 0, 0, 1)):
        assert raw(*args) == -1, args
    assert raw(1, 1, 0, 1) == 0
