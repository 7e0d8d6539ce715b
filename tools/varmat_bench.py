"""Measurements of the per-element material path on the C4 scene (tet_drop(100, 40, 50), 1 000 000
NeoHookean tets, z-AA m=6), with Solver.bench_iterations / kernel_stats only:

  --mode same     the scene bound with the scalar call and with arrays holding that same value,
                  alternated in one process (two pairs): what the per-element instantiations cost
  --mode levels   64 material levels per element (scenes.with_material_levels), bound as one
                  per-element group ("var") and as 64 gathered scalar groups ("groups", the only
                  form without aa_elastic_add_tets_var -- AA_ADMM_LIB may point at such a build):
                  what the feature buys. With both forms, one step of each is compared at 1e-6.

Prints one JSON line; --out appends it to a file.

    python tools/varmat_bench.py --mode same
    python tools/varmat_bench.py --mode levels --forms var,groups
"""
import argparse
import dataclasses
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
pkg = importlib.import_module("aa-admm_amd")
capi, S = pkg.capi, pkg.scenes

CLASSES = ("local_z", "grad", "prim", "rhs", "solve", "aa")
ELEMENT_CLASSES = ("local_z", "grad", "prim")   # launched once per group


def levels(L):
    k = np.arange(L) / (L - 1.0)
    return dict(E_levels=1e6 * 10.0 ** k, nu_levels=0.30 + 0.15 * k)


def gathered_groups(sc):
    """One scalar group per distinct material of the scene's per-element group (elements gathered)."""
    (g,) = sc.groups
    E, nu, _, _ = g.material_arrays()
    mats, inv = np.unique(np.stack([E, nu], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return dataclasses.replace(sc, groups=[
        dataclasses.replace(g, E=float(mats[m, 0]), nu=float(mats[m, 1]), idx=g.idx[inv == m]) for m in range(len(mats))])


def with_arrays(sc):
    (g,) = sc.groups
    n = len(g.idx)
    return dataclasses.replace(sc, groups=[dataclasses.replace(g, E=np.full(n, g.E), nu=np.full(n, g.nu))])


def bind(ctx, sc):
    s = capi.solver_from_scene(ctx, sc)
    s.initialize(capi.settings_from_scene(sc))
    return s


def measure(s, iters, n_groups):
    ms = s.bench_iterations(iters)
    st = {k: s.kernel_stats(k) for k in CLASSES}
    per_iter = {k: round(1e3 * v["avg_ms"] * v["launches"] / iters, 1) for k, v in st.items()}
    return {"iter_us": round(1e3 * ms / iters, 1), "class_us_per_iter": per_iter,
            "local_z_us_per_pass": round(1e3 * st["local_z"]["avg_ms"], 1),
            "element_kernel_launches_per_iter": round(n_groups * sum(st[k]["launches"] for k in ELEMENT_CLASSES) / iters, 1)}


def step_ms(s):
    s.step()   # first step: graph capture
    s.step()
    return round(s.runtime().step_ms, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("same", "levels"), required=True)
    ap.add_argument("--size", default="100,40,50")
    ap.add_argument("--iters", type=int, default=40, help="iterations per bench_iterations call")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("--forms", default="var,groups")
    ap.add_argument("--out")
    a = ap.parse_args()
    cx, cy, cz = (int(v) for v in a.size.split(","))
    base = S.tet_drop(cx, cy, cz)
    ctx = capi.Context(0)
    res = {"mode": a.mode, "scene": f"tet_drop({cx},{cy},{cz})", "elements": base.n_elements(),
           "library": os.path.basename(capi.LIB_PATH), "bench_iters": a.iters}
    if a.mode == "same":
        forms = {"scalar": bind(ctx, base), "arrays": bind(ctx, with_arrays(base))}
        for f, s in forms.items():
            s.bench_iterations(5)   # warm-up
        res["runs"] = [{f: measure(s, a.iters, 1) for f, s in forms.items()} for _ in range(a.pairs)]
        lz = {f: np.mean([r[f]["local_z_us_per_pass"] for r in res["runs"]]) for f in forms}
        it = {f: np.mean([r[f]["iter_us"] for r in res["runs"]]) for f in forms}
        res["ratio_arrays_over_scalar"] = {"local_z": round(lz["arrays"] / lz["scalar"], 4),
                                           "iteration": round(it["arrays"] / it["scalar"], 4)}
    else:
        sc = S.with_material_levels(base, **levels(a.levels))
        scenes_ = {"var": sc, "groups": gathered_groups(sc)}
        res["levels"] = a.levels
        res["forms"] = {}
        traj = {}
        for f in a.forms.split(","):
            s = bind(ctx, scenes_[f])
            n_groups = len(scenes_[f].groups)
            ms = step_ms(s)   # the steps first, as bench.py: their second step is the one compared
            h = s.history()
            traj[f] = [dict(prim=h["prim"], comb=h["comb"], reject=h["reject"], x=s.x.reshape(-1, 3))]
            s.bench_iterations(5)
            runs = [measure(s, a.iters, n_groups) for _ in range(a.pairs)]
            res["forms"][f] = {"groups": n_groups, "runs": runs, "step_ms": ms}
            s.close()
        if len(traj) == 2:
            from golden_io import compare
            fails = compare(traj["groups"], traj["var"], 1e-6, 1e-6)
            res["forms_agree_1e-6"] = not fails
            res["compare_failures"] = fails
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()
    if a.mode == "levels" and res.get("forms_agree_1e-6") is False:
        sys.exit("the two forms differ: " + "; ".join(res["compare_failures"]))


if __name__ == "__main__":
    main()
