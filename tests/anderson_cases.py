"""Cases and references for the Anderson step's three kernels (k_aa_reduce / k_aa_reduce_cols,
k_aa_solve, k_aa_mix in csrc/elastic_kernels.hip), driven one step at a time through
aa_test_anderson_step (capi.hook_anderson_step). Plain numpy and mpmath, no GPU use.

A state is a dict: m, na, nb, eff, cur (dim), dF (m, eff) and dG (m, dim) with row c = history
column c, the Ctrl ints of capi.ANDERSON_CTL, scale (m), M (m, m), coef (m), aa_s, mask =
(lo1, hi1, lo2, hi2) -- what hook_anderson_step takes and gives back.

ref_step(state, G): one AndersonAcceleration::compute_impl step (AndersonAcceleration.h:154-211)
from that state, vectors in np.longdouble, the mk x mk solve in mpmath; with the device's extension
(the AAMask windows in the second segment) and in the device's layout of the sums.
port_step(state, G): the same function in float64, operation for operation (CPU checks only).
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)
HAVE_LONGDOUBLE = LD_EPS < 2e-19   # 80-bit extended (or better); a 64-bit long double cannot referee fp64
U = 2.0 ** -53
SCALE_EPS = 1e-14                  # AndersonAcceleration.h:167
FULL_MASK = (0, 0x7FFFFFFFFFFFFFFF, 0, 0)
CTL = ("aa_iter", "aa_col", "aa_skip", "aa_active", "done", "aa_mk", "aa_j", "aa_jn", "aa_first")
COND_MAX = 1e6                     # the non-degenerate chains keep cond_2(M) below this
MP_DPS = 40

# tests/golden/anderson.npz: the reference's own class on three recorded chains. Largest relative
# deviation max|u_golden - u_pred| / max|u_pred| of the class's u_{k+1} from ref_step's prediction
# out of the state rebuilt from the (G_k, u_k) pairs (tests/test_anderson_cases.py), over the three
# fixtures: 2.6e-16 (m20, call 18). The tolerance is 16 times that: another build may sum in
# another order.
GOLDEN_MEASURED = 2.6e-16
GOLDEN_TOL = 16 * GOLDEN_MEASURED


@functools.lru_cache(maxsize=None)
def golden():
    """name -> (m, eff, u0, G (T, dim), u (T, dim))"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anderson.npz"))
    return {n: (int(d[n + "_m"]), int(d[n + "_eff"]), d[n + "_u0"], d[n + "_G"], d[n + "_u"]) for n in ("m3", "m6", "m20")}


def window_bucket(m):
    """aa_window_bucket (csrc/elastic_kernels.hip) with its default knobs."""
    return 8 if m <= 8 else 12 if m <= 12 else 16 if m <= 16 else 32


def mix_instance(m, narrow):
    """The k_aa_mix<MM> launch_aa_mix picks."""
    return 6 if narrow and m <= 6 else 7 if narrow and m == 7 else window_bucket(m)


def clean_state(m, na, nb, eff, u0, mask=FULL_MASK):
    dim = na + nb
    return dict(m=m, na=na, nb=nb, eff=eff, cur=np.array(u0, np.float64).reshape(dim), dF=np.zeros((m, eff)),
                dG=np.zeros((m, dim)), scale=np.zeros(m), M=np.zeros((m, m)), coef=np.zeros(m), aa_s=0.0,
                mask=tuple(mask), aa_iter=0, aa_col=0, aa_skip=0, aa_active=1, done=0, aa_mk=0, aa_j=0, aa_jn=0,
                aa_first=0)


def copy_state(st):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in st.items() if k in _STATE_KEYS}


_STATE_KEYS = ("m", "na", "nb", "eff", "cur", "dF", "dG", "scale", "M", "coef", "aa_s", "mask") + CTL


def in_sums(st):
    """Bool (eff,): the entries that enter the dot products -- i < eff, and inside the mask windows
    where i lies in the second segment."""
    na, eff = st["na"], st["eff"]
    lo1, hi1, lo2, hi2 = st["mask"]
    i = np.arange(eff)
    j = i - na
    return (i < na) | ((j >= lo1) & (j < hi1)) | ((j >= lo2) & (j < hi2))


def mp_solve(M, b):
    """Exact-to-MP_DPS solution of the small system (M nonsingular), as float64."""
    import mpmath as mp
    with mp.workdps(MP_DPS):
        A = mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(M, np.float64)])
        x = mp.lu_solve(A, mp.matrix([mp.mpf(float(v)) for v in np.asarray(b, np.float64)]))
        return np.array([float(v) for v in x])


@dataclass
class RefStep:
    first: bool
    mk: int
    col: int
    jn: int
    n_in: int
    tot: np.ndarray      # (2 + 2 MM,) long double: |dF_j|^2, dF_j.F, dF_j.dF_c, dF_c.F
    S: np.ndarray        # the majorants sum |a_i| |b_i| of the same sums
    live: np.ndarray     # bool: the slots the kernels accumulate
    s: float
    M: np.ndarray        # (m, m) float64: the state's M with row / column col renewed from tot
    b: np.ndarray        # (mk,)
    theta: np.ndarray    # (mk,) or None (solve=False)
    u: np.ndarray        # (dim,) long double: the accelerated iterate (None without theta)
    next: dict           # the state after the step, rounded to float64 (None without theta)


def ref_step(st, G, solve=True):
    m, na, nb, eff = st["m"], st["na"], st["nb"], st["eff"]
    MM = window_bucket(m)
    g, cur = np.asarray(G, np.float64).astype(LD), st["cur"].astype(LD)
    dF, dG = st["dF"].astype(LD), st["dG"].astype(LD)
    it, col = st["aa_iter"], st["aa_col"]
    F = g[:eff] - cur[:eff]
    inm = in_sums(st)
    tot, S, live = np.zeros(2 + 2 * MM, LD), np.zeros(2 + 2 * MM, LD), np.zeros(2 + 2 * MM, bool)
    nxt = copy_state(st)
    if it == 0:
        nxt["dF"][0], nxt["dG"][0], nxt["cur"] = (-F).astype(np.float64), (-g).astype(np.float64), g.astype(np.float64)
        nxt.update(aa_iter=1, aa_first=1, aa_j=0, aa_jn=0, aa_mk=0)
        return RefStep(True, 0, col, 0, int(inm.sum()), tot, S, live, 0.0, st["M"].copy(), np.zeros(0), np.zeros(0), g, nxt)
    mk, jn = min(m, it), (col + 1) % m
    dfj = dF[col] + F
    aF = np.abs(g[:eff]) + np.abs(cur[:eff])
    aD = np.abs(dF[col]) + aF
    w = inm.astype(LD)
    tot[0], S[0] = np.sum(w * dfj * dfj), np.sum(w * aD * aD)
    tot[1], S[1] = np.sum(w * dfj * F), np.sum(w * aD * aF)
    live[:2] = True
    for c in range(mk):
        if c == col:
            continue
        tot[2 + c], S[2 + c] = np.sum(w * dfj * dF[c]), np.sum(w * aD * np.abs(dF[c]))
        tot[2 + MM + c], S[2 + MM + c] = np.sum(w * dF[c] * F), np.sum(w * np.abs(dF[c]) * aF)
        live[2 + c] = live[2 + MM + c] = True
    s = max(LD(SCALE_EPS), np.sqrt(tot[0]))
    M, scale = st["M"].astype(LD), st["scale"].astype(LD)
    scale[col] = s
    b = np.zeros(mk, LD)
    for c in range(mk):
        if c != col:
            M[c, col] = M[col, c] = tot[2 + c] / s
            b[c] = tot[2 + MM + c]
    M[col, col] = tot[0] / (s * s)
    b[col] = tot[1] / s
    M64, b64 = M.astype(np.float64), b.astype(np.float64)
    if not solve:
        return RefStep(False, mk, col, jn, int(inm.sum()), tot, S, live, float(s), M64, b64, None, None, None)
    if mk == 1:
        dn = np.sqrt(M[0, 0])
        theta = np.array([float(b[0] / (dn * dn)) if dn > SCALE_EPS else 0.0])
    else:
        theta = mp_solve(M64[:mk, :mk], b64)
    coef = theta.astype(LD) / scale[:mk]
    d = dG[:mk].copy()
    d[col] += g
    u = g - coef @ d
    nxt["dF"][col], nxt["dG"][col] = (dfj / s).astype(np.float64), d[col].astype(np.float64)
    nxt["dF"][jn], nxt["dG"][jn] = (-F).astype(np.float64), (-g).astype(np.float64)
    nxt["cur"], nxt["M"], nxt["scale"] = u.astype(np.float64), M64, scale.astype(np.float64)
    nxt["coef"][:mk] = coef.astype(np.float64)
    nxt.update(aa_iter=it + 1, aa_col=jn, aa_first=0, aa_j=col, aa_jn=jn, aa_mk=mk, aa_s=float(s))
    return RefStep(False, mk, col, jn, int(inm.sum()), tot, S, live, float(s), M64, b64, theta, u, nxt)


def port_step(st, G):
    """compute_impl in float64, statement for statement (no mask: the class has none). Returns
    (u, the next state); the COD solve is numpy's minimum-norm least squares."""
    m, eff = st["m"], st["eff"]
    G = np.asarray(G, np.float64)
    nxt = copy_state(st)
    dF, dG, Mx, scale = nxt["dF"], nxt["dG"], nxt["M"], nxt["scale"]
    it, col = st["aa_iter"], st["aa_col"]
    F = G[:eff] - st["cur"][:eff]
    if it == 0:
        dF[0], dG[0] = -F, -G
        nxt["cur"] = G.copy()
    else:
        dF[col] += F
        dG[col] += G
        s = max(SCALE_EPS, float(np.sqrt(dF[col] @ dF[col])))
        scale[col] = s
        dF[col] /= s
        mk = min(m, it)
        theta = np.zeros(mk)
        if mk == 1:
            sq = float(dF[col] @ dF[col])
            Mx[0, 0] = sq
            dn = np.sqrt(sq)
            if dn > SCALE_EPS:
                theta[0] = (dF[col] / dn) @ (F / dn)
        else:
            ip = dF[:mk] @ dF[col]
            Mx[col, :mk] = ip
            Mx[:mk, col] = ip
            theta = np.linalg.lstsq(Mx[:mk, :mk], dF[:mk] @ F, rcond=None)[0]
        nxt["cur"] = G - (theta / scale[:mk]) @ dG[:mk]
        col = (col + 1) % m
        dF[col], dG[col] = -F, -G
        nxt["aa_col"] = col
    nxt["aa_iter"] = it + 1
    return nxt["cur"].copy(), nxt


# ---- the fixed-point maps ------------------------------------------------------------------------
class Contraction:
    """G(u) = A u + b with A = rho P D H: H a Householder reflection, D random signs, P a random
    permutation -- orthogonal times rho = 0.9, so |A|_2 = 0.9 exactly, applied in O(dim)."""

    def __init__(self, dim, seed, rho=0.9):
        self.rho = rho
        rng = np.random.default_rng(seed)
        v = rng.standard_normal(dim)
        self.v = v / np.linalg.norm(v)
        self.sign = rng.choice([-1.0, 1.0], dim)
        self.perm = rng.permutation(dim)
        self.b = rng.standard_normal(dim)
        self.u0 = rng.standard_normal(dim)
        self.dim = dim

    def A(self, x):
        if self.dim == 1:
            return self.rho * self.sign * x
        return self.rho * (self.sign * (x - 2.0 * self.v * (self.v @ x)))[self.perm]

    def __call__(self, u):
        return self.A(np.asarray(u, np.float64)) + self.b


@dataclass(frozen=True)
class Case:
    name: str
    dim: int
    na: int
    eff: int
    m: int
    mask: tuple = FULL_MASK
    nblocks: int = 0
    inplace: bool = False
    copy_to: bool = True
    narrow: bool = True
    rows: bool = False
    kind: str = "chain"     # chain | reset | repeat | twin
    seed: int = 0

    @property
    def nb(self):
        return self.dim - self.na

    @property
    def T(self):
        return 2 * self.m + 3

    @property
    def degenerate(self):
        return self.kind in ("repeat", "twin")

    def map(self):
        return _map(self.dim, 1000 + self.seed)

    def start(self):
        return clean_state(self.m, self.na, self.nb, self.eff, self.map().u0, self.mask)


@functools.lru_cache(maxsize=None)
def _map(dim, seed):
    return Contraction(dim, seed)


def _z(dim, m, **kw):      # the Z variant: one segment, all of it effective, mixed in place
    return Case(f"z_d{dim}_m{m}" + _suffix(kw), dim, dim, dim, m, inplace=True, copy_to=False, **kw)


def _ux(dim, m, **kw):     # (u, x): the first segment, about two thirds, is the effective one
    na = max(1, (2 * dim) // 3)
    return Case(f"ux_d{dim}_m{m}" + _suffix(kw), dim, na, na, m, **kw)


def _alm(dim, m, **kw):    # the geometry ALM path: both segments effective, the mask over the second
    na = max(1, (2 * dim) // 3)
    return Case(f"alm_d{dim}_m{m}" + _suffix(kw), dim, na, dim, m, **kw)


def _suffix(kw):
    s = ""
    if kw.get("narrow") is False:
        s += "_bucketmix"
    if kw.get("rows"):
        s += "_rows"
    elif "rows" in kw:
        s += "_cols"
    if kw.get("nblocks"):
        s += f"_nb{kw['nblocks']}"
    if "mask" in kw:
        s += "_empty" if kw["mask"][1] == 0 and kw["mask"][3] == 0 else "_windows"
    if kw.get("kind", "chain") != "chain":
        s += "_" + kw["kind"]
    return s


def _windows(dim):
    """Two disjoint windows in the second segment of _alm(dim, ...)."""
    nb = dim - max(1, (2 * dim) // 3)
    return (nb // 8, nb // 3, nb // 2, nb - max(1, nb // 7))


EMPTY = (0, 0, 0, 0)

CASES = [
    # Z variant, in place: every mix instantiation, narrow and the bucket's
    _z(1, 1, nblocks=1),
    _z(63, 2), _z(63, 2, narrow=False),
    _z(64, 5, nblocks=3), _z(64, 5, narrow=False),
    _z(257, 6), _z(257, 6, narrow=False, nblocks=1),
    _z(511, 7, nblocks=3), _z(511, 7, narrow=False),
    _z(512, 8),
    _z(513, 10, nblocks=3),
    _z(1537, 12),
    _z(1537, 16, nblocks=1),
    # (u, x): two segments, eff = na, the history strides differ; wide windows with both reduce kernels
    _ux(63, 5), _ux(257, 1), _ux(257, 1, narrow=False), _ux(1537, 6, nblocks=1),
    _ux(512, 17, rows=False), _ux(512, 17, rows=True),
    _ux(513, 20, rows=False, nblocks=3), _ux(513, 20, rows=True, nblocks=3),
    _ux(1537, 32, rows=False), _ux(1537, 32, rows=True),
    # the ALM path: eff = dim over both segments, the mask's windows
    _alm(64, 8), _alm(512, 16),
    _alm(257, 10, mask=_windows(257)), _alm(511, 12, mask=EMPTY, nblocks=3),
    _alm(1537, 20, rows=False, mask=_windows(1537)), _alm(1537, 20, rows=True, mask=_windows(1537)),
    _alm(513, 20, rows=False, nblocks=8),   # the column-parallel kernel's blocks 2..7 own no rows
    _alm(513, 17, rows=False, nblocks=1, mask=EMPTY),
    # eff strictly inside the first segment
    Case("inner_d257_m7", 257, 200, 150, 7),
    # block partials past k_aa_solve's chunk count NCH = 1024 / (2 + 2 MM) (56, 39, 30, 15): the
    # smallest vectors whose last chunk still sums a block that owns rows (256 rows a block in the
    # row-parallel kernel, 512-row tiles in the column-parallel one)
    _z(14593, 8, nblocks=58), _z(10241, 12, nblocks=41), _z(7937, 16, nblocks=32),
    _ux(5761, 17, rows=True, nblocks=16), _alm(7681, 17, rows=False, nblocks=16),
    # a reset in mid-chain that leaves the stale history behind
    _z(257, 6, kind="reset"), _ux(513, 20, rows=False, kind="reset"), _alm(257, 10, mask=_windows(257), kind="reset"),
    # degenerate chains
    _z(64, 5, kind="repeat"), _ux(257, 8, kind="repeat"),
    _alm(257, 8, kind="twin"), _ux(512, 17, rows=False, kind="twin"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
GATES = ("done", "aa_skip", "aa_active")
RESET_AFTER = lambda m: m + 1   # noqa: E731  (steps run before the reset)


def make_twin(st):
    """Give the state two identical history columns (a finished one copied over another), M and
    scale with them: the normal equations turn singular."""
    st = copy_state(st)
    mk, col = min(st["m"], st["aa_iter"]), st["aa_col"]
    done = [c for c in range(mk) if c != col]
    a, b = done[0], done[-1]
    assert a != b
    st["dF"][b], st["dG"][b], st["scale"][b] = st["dF"][a], st["dG"][a], st["scale"][a]
    st["M"][b, :], st["M"][:, b] = st["M"][a, :], st["M"][:, a]
    st["M"][b, b] = st["M"][a, b] = st["M"][b, a] = st["M"][a, a]
    return st


def reference_chain(case, steps=None):
    """The case's chain run by ref_step on its own outputs: [(state, G, RefStep)] per step."""
    f, st, out = case.map(), case.start(), []
    for k in range(case.T if steps is None else steps):
        if case.kind == "reset" and k == RESET_AFTER(case.m):
            st = copy_state(st)
            st.update(aa_iter=0, aa_col=0)
        G = f(st["cur"])
        r = ref_step(st, G)
        out.append((st, G, r))
        st = r.next
    return out
