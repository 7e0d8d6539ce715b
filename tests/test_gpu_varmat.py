"""GPU: per-element material parameters (aa_elastic_add_tets_var / aa_elastic_add_tris_var): one
group, one launch per kernel class and one work queue for a scene whose Lame parameters vary from
element to element -- the reference's one EnergyTerm per element, each with its own Lame.

1. parity with the reference's own runs (tests/golden/varmat/, make_golden_varmat.py) at the
   project's bars: 1e-6 of comb_0 for the L-BFGS prox paths, 1e-9 for linear tets and cloth;
2. arrays holding one value are the uniform path bit for bit (k_e and the per-element kernels'
   arithmetic are the uniform kernels');
3. the partitioned solver carries the arrays with the elements it hands to each rank;
4. the scalar calls' errors, per element;
5. the C++ facade's std::vector<Lame> overloads drive the same device path."""
import ctypes as C
import dataclasses
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import varmat_cases
import varmat_part_worker
from conftest import REPO
from golden_io import compare, scenes
from test_facade import build

pytestmark = pytest.mark.gpu
S = scenes


def bits_equal(a, b):
    assert len(a) == len(b)
    for k, (sa, sb) in enumerate(zip(a, b)):
        for key in ("prim", "comb", "reject", "x", "v"):
            assert np.array_equal(sa[key], sb[key]), (k, key)


# ---------------------------------------------------------------- 1. the reference's own runs
@pytest.mark.parametrize("name", varmat_cases.names())
def test_gpu_per_element_matches_reference(name, pkg, ctx):
    sc, ref = varmat_cases.load(name)
    assert len(sc.groups) == 1 and sc.groups[0].per_element
    got, s = pkg.capi.run_scene(ctx, sc)
    assert s.runtime().n_elements == len(sc.groups[0].idx)
    s.close()
    tol = varmat_cases.TOL[name]
    assert [len(g["prim"]) for g in got] == [len(r["prim"]) for r in ref]
    fails = compare(ref, got, tol, tol)
    assert not fails, fails
    assert np.allclose(got[-1]["v"], ref[-1]["v"], rtol=0, atol=tol * 1e3 * max(1.0, np.abs(ref[-1]["v"]).max()))
    # control: every element at the mean level is a different scene -- a kernel that ignored the
    # arrays (or read one element's values for all) could not have passed above
    ctl, s = pkg.capi.run_scene(ctx, varmat_cases.mean_level_scene(name))
    s.close()
    assert compare(ref, ctl, tol, tol), "the uniform mean-level scene passes the per-element fixture"


# ---------------------------------------------------------------- 2. uniform arrays = uniform path
def with_arrays(sc, which=None):
    """The scene with the scalar materials of its groups (`which`: indices; default all) written as
    arrays of that one value."""
    groups = []
    for i, g in enumerate(sc.groups):
        if which is not None and i not in which:
            groups.append(g)
            continue
        n = len(g.idx)
        kw = dict(E=np.full(n, g.E), nu=np.full(n, g.nu))
        if g.kind == S.TRI:
            kw.update(limit_min=np.full(n, g.limit_min), limit_max=np.full(n, g.limit_max))
        groups.append(dataclasses.replace(g, **kw))
    return dataclasses.replace(sc, groups=groups)


UNIFORM = {
    "drop12": (lambda: S.tet_drop(12, 4, 6, iters=40, n_steps=2), None, {}),    # 22.5 waves: tail clamp, multi-wave claims
    "drop12_plain_refill": (lambda: S.tet_drop(12, 4, 6, iters=40, n_steps=2), None, {"AA_LQ_FUSED": "0"}),
    "cant_nh": (lambda: S.cantilever(8, 2, 2, S.NEOHOOKEAN), None, {}),
    "cant_stvk_noaa": (lambda: S.cantilever(8, 2, 2, S.STVK, accel=0), None, {}),
    "cant_lin_z": (lambda: S.cantilever(8, 2, 2, S.LINEAR), None, {}),
    "cant_lin_ux": (lambda: S.cantilever(8, 2, 2, S.LINEAR, variant=S.VARIANT_H), None, {}),
    # mixed uniform / per-element groups in one solver, the (u,x) local step with partials
    "beams_ux_middle": (lambda: S.beams(2, iters=40, n_steps=2, variant=S.VARIANT_H), (1,), {}),
    "cloth": (lambda: S.cloth(12, 12, iters=40, n_steps=2), None, {}),
}


@pytest.mark.parametrize("case", sorted(UNIFORM))
def test_uniform_arrays_are_the_uniform_path_bit_for_bit(case, pkg, ctx, monkeypatch):
    builder, which, env = UNIFORM[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = builder()
    var = with_arrays(sc, which)
    assert any(g.per_element for g in var.groups) and not any(g.per_element for g in sc.groups)
    want, s = pkg.capi.run_scene(ctx, sc)
    s.close()
    got, s = pkg.capi.run_scene(ctx, var)
    s.close()
    assert all(np.isfinite(st["x"]).all() for st in got)
    bits_equal(want, got)


# ---------------------------------------------------------------- 3. partitioned
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(nranks, out, timeout=240):
    """test_gpu_partition.run_ranks for tests/varmat_part_worker.py: front-check lines fail the run
    and every rank's runtime report is checked."""
    out.mkdir(parents=True, exist_ok=True)
    env = dict(os.environ, AA_OUT=str(out), AA_DEVICE="0", AA_COMM_VERIFY="1", OMP_NUM_THREADS="4")
    env.pop("AA_FRONT_RETRY", None)   # a wrong first factorization fails the run
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nranks}",
                        "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
                        os.path.join(REPO, "tests", "varmat_part_worker.py")],
                       capture_output=True, text=True, timeout=timeout, env=env)
    notes = [ln for ln in (r.stderr or "").splitlines() if "[front-check]" in ln]
    assert not notes, notes
    for k in range(nranks):
        rep = json.load(open(out / f"rank{k}.runtime.json"))
        assert all(os.path.dirname(v) == rep["expected"] for v in rep["bound"].values()), rep
    if r.returncode != 0:
        errs = "".join(f"--- {f.name}:\n{f.read_text()[-3000:]}\n" for f in sorted(out.glob("rank*.err")))
        assert False, errs + r.stdout[-1000:] + r.stderr[-2000:]
    return [dict(np.load(out / f"rank{k}.npz")) for k in range(nranks)]


def test_partitioned_per_element_matches_single_gpu(tmp_path, pkg, ctx):
    sc = varmat_part_worker.scene()
    want, s = pkg.capi.run_scene(ctx, sc)
    s.close()
    ranks = run_ranks(2, tmp_path)
    assert sum(int(r["n_elements"][0]) for r in ranks) == sc.n_elements() == 1440
    assert all(int(r["n_elements"][0]) > 0 for r in ranks)
    for k in ranks[0]:
        if k != "n_elements":
            assert np.array_equal(ranks[1][k], ranks[0][k]), k
    got = [{k: ranks[0][f"{k}{i}"] for k in ("prim", "comb", "reject", "x", "v")} for i in range(len(want))]
    assert [len(g["prim"]) for g in got] == [len(w["prim"]) for w in want]
    for w in want:
        w["x"] = w["x"].reshape(-1, 3)
    fails = compare(want, got, 1e-6, 1e-6)
    assert not fails, fails


# ---------------------------------------------------------------- 4. errors
def _tets():
    v, t = S.tet_blocks(2, 1, 1)
    return v, t, np.full(len(t), 4e6), np.full(len(t), 6e6)


def _fresh(pkg, ctx, v):
    s = pkg.capi.Solver(ctx)
    s.add_nodes(v, np.ones(3 * len(v)))
    return s


def test_per_element_errors(pkg, ctx):
    capi = pkg.capi
    v, t, mu, lam = _tets()
    vt, tt = S.tri_blocks(2, 2)
    n3 = len(tt)

    def fails(code, words, call, *args):
        with pytest.raises(capi.AAError) as ei:
            call(*args)
        assert ei.value.code == code, str(ei.value)
        for w in words:
            assert w in str(ei.value), str(ei.value)

    # triangle strain-limit ranges, per element
    s = _fresh(pkg, ctx, vt)
    lmin = np.full(n3, 0.95)
    lmin[5] = 1.01
    fails(-1, ("**TriEnergyTerm Error: Strain limit min should be -inf to 1", "element 5"),
          s.add_tris_var, vt, tt, 20.0, 5.0, lmin, 1.05)
    lmax = np.full(n3, 1.05)
    lmax[[7, 9]] = 0.99
    fails(-1, ("**TriEnergyTerm Error: Strain limit max should be 1 to inf", "element 7"),
          s.add_tris_var, vt, tt, 20.0, 5.0, 0.95, lmax)
    # weight <= 0: k_e = lambda_e + 2/3 mu_e <= 0 on one element
    s2 = _fresh(pkg, ctx, v)
    bad = lam.copy()
    bad[4] = -(2.0 / 3.0) * mu[4]
    fails(-4, ("**EnergyTerm::get_reduction Error: Some weight leq 0", "element 4"),
          s2.add_tets_var, v, t, capi.AA_NEOHOOKEAN, mu, bad)
    # inverted element
    ti = t.copy()
    ti[3, [0, 1]] = ti[3, [1, 0]]
    fails(-4, ("**TetEnergyTerm Error: Inverted initial tet", "element 3"), s2.add_tets_var, v, ti, capi.AA_NEOHOOKEAN, mu, lam)
    # non-finite mu / lambda
    nan = mu.copy()
    nan[2] = np.nan
    fails(-1, ("finite", "element 2"), s2.add_tets_var, v, t, capi.AA_STVK, nan, lam)
    inf = lam.copy()
    inf[6] = np.inf
    fails(-1, ("finite", "element 6"), s2.add_tets_var, v, t, capi.AA_LINEAR, mu, inf)
    # null array with n > 0
    vv, tf = np.ascontiguousarray(v, np.float64).reshape(-1), np.ascontiguousarray(t, np.int32).reshape(-1)
    rc = capi.lib().aa_elastic_add_tets_var(s2.h, capi._dp(vv), capi._ip(tf), C.c_int(len(t)), C.c_int(1), None, C.c_int(0))
    assert rc == -1 and b"null" in capi.lib().aa_last_error()
    v3, t3 = np.ascontiguousarray(vt, np.float64).reshape(-1), np.ascontiguousarray(tt, np.int32).reshape(-1)
    rc = capi.lib().aa_elastic_add_tris_var(s.h, capi._dp(v3), capi._ip(t3), C.c_int(n3), None, C.c_int(0))
    assert rc == -1 and b"null" in capi.lib().aa_last_error()
    # none of the failed calls left a group behind: the valid call binds and the solver runs
    s2.add_tets_var(v, t, capi.AA_NEOHOOKEAN, mu, lam)
    s2.initialize(capi.Settings(admm_iters=5, variant=capi.AA_VARIANT_Z, verbose=0))
    assert s2.runtime().n_elements == len(t)
    s2.step()
    assert np.isfinite(s2.x).all()
    s.close()
    s2.close()


# ---------------------------------------------------------------- 5. facade
def test_facade_varmat_matches_binding(tmp_path, pkg, ctx):
    exe, out = str(tmp_path / "facade_varmat"), str(tmp_path / "o.bin")
    build(exe, os.path.join(REPO, "tests", "cpp", "facade_varmat.cpp"))
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    xv = np.frombuffer(raw[4:], np.float64).reshape(2, n, 3)
    # the same graded beam through the Python binding (tests/cpp/facade_varmat.cpp)
    v, t = S.tet_blocks(8, 2, 2)
    v = v / 2.0
    X = np.repeat(np.arange(8), 5 * 2 * 2)   # the cell's x index of every tet (cells x-major, 5 tets each)
    g = S.ElementGroup(S.TET, S.NEOHOOKEAN, 1e5 + 9.9e6 * X / 7.0, 0.30 + 0.15 * X / 7.0, t)
    pins = np.nonzero(v[:, 0] == 0.0)[0].astype(np.int32)
    sc = S.Scene(x=v, masses=np.full(len(v), 0.05), groups=[g], pin_idx=pins, pin_pts=v[pins].copy(),
                 pin_vel=np.zeros((len(pins), 3)), variant=S.VARIANT_X, iters=30, aa_m=6, n_steps=2)
    assert n == sc.n_nodes
    want, s = pkg.capi.run_scene(ctx, sc)
    s.close()
    assert np.array_equal(xv[0], want[-1]["x"].reshape(-1, 3))
    assert np.array_equal(xv[1], want[-1]["v"].reshape(-1, 3))
    assert np.abs(xv[1]).max() > 0
