"""What bending hinges cost on the C2 cloth (scenes.cloth(), 112 x 112 cells, 50 176 triangles,
(u,x)-Anderson m=6): the scene without and with bend=1e-2, three alternated runs of each in one
process, with Solver.bench_iterations / kernel_stats only. Per form: iteration time, the local_z and
solve classes, the scalar factor's nnz(L) (the hinges couple each node to its second ring, so A_s
and its factor fill in), setup time and the element counts. No threshold: for the record.

    python tools/bending_timing.py --out profiles/bending.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("aa-admm_amd")
capi, S = pkg.capi, pkg.scenes

CLASSES = ("local_z", "resid", "rhs", "solve", "aa")


def bind(ctx, sc):
    s = capi.solver_from_scene(ctx, sc)
    s.initialize(capi.settings_from_scene(sc))
    return s


def measure(s, iters):
    ms = s.bench_iterations(iters)
    st = {k: s.kernel_stats(k) for k in CLASSES}
    return {"iter_us": round(1e3 * ms / iters, 1),
            "class_us_per_iter": {k: round(1e3 * v["avg_ms"] * v["launches"] / iters, 1) for k, v in st.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="112,112")
    ap.add_argument("--bend", type=float, default=1e-2)
    ap.add_argument("--iters", type=int, default=100, help="iterations per bench_iterations call")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    nx, ny = (int(v) for v in a.size.split(","))
    ctx = capi.Context(0)
    scenes_ = {"membrane": S.cloth(nx, ny), "bending": S.cloth(nx, ny, bend=a.bend)}
    res = {"scene": f"cloth({nx},{ny})", "bend": a.bend, "bench_iters": a.iters, "forms": {}}
    ctx.warm_dense()   # the process's one-time loads, kept out of the setup times
    bind(ctx, scenes_["membrane"]).close()
    solvers = {}
    for f, sc in scenes_.items():
        s = solvers[f] = bind(ctx, sc)
        rt = s.runtime()
        res["forms"][f] = {"elements": rt.n_elements, "z_dim": rt.z_dim, "nnz_L": int(rt.nnz_factor),
                           "setup_ms": round(rt.setup_ms, 1), "runs": []}
        s.bench_iterations(5)   # warm-up
    for _ in range(a.runs):   # alternated
        for f, s in solvers.items():
            res["forms"][f]["runs"].append(measure(s, a.iters))
    med = {f: float(np.median([r["iter_us"] for r in v["runs"]])) for f, v in res["forms"].items()}
    res["iter_us_median"] = med
    res["ratio_bending_over_membrane"] = {
        "iteration": round(med["bending"] / med["membrane"], 4),
        "nnz_L": round(res["forms"]["bending"]["nnz_L"] / res["forms"]["membrane"]["nnz_L"], 4),
        **{k: round(float(np.median([r["class_us_per_iter"][k] for r in res["forms"]["bending"]["runs"]])
                          / max(1e-9, np.median([r["class_us_per_iter"][k] for r in res["forms"]["membrane"]["runs"]]))), 4)
           for k in ("local_z", "solve")}}
    for s in solvers.values():
        s.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
