"""What springs cost on the C2 cloth (scenes.cloth(), 112 x 112 cells, 50 176 triangles,
(u,x)-Anderson m=6): the scene as it is ("membrane"), with a shear spring on both corner-to-corner
diagonals of every grid cell ("shear", 25 088 springs at their rest length: new adjacency between
corner nodes that share no triangle) and with a spring between the opposite nodes of the sheet's
edges ("long_ties", 226 springs of 0.9 their distance: long-range adjacency, which changes the
dissection and the fill). Three alternated runs of each in one process, with
Solver.bench_iterations / kernel_stats only. Per form: iteration time, the local_z, resid and solve
classes, the scalar factor's nnz(L), setup time and the element counts. No threshold: for the record.

    python tools/spring_timing.py --out profiles/springs.json
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


def spring_forms(nx, ny, k):
    """name -> scene: cloth(nx, ny) and its two spring variants (corner(i, j) = i (ny + 1) + j, tri_blocks)."""
    base = S.cloth(nx, ny)
    corner = lambda i, j: i * (ny + 1) + j
    shear = np.array([p for i in range(nx) for j in range(ny)
                      for p in ((corner(i, j), corner(i + 1, j + 1)), (corner(i + 1, j), corner(i, j + 1)))], np.int32)
    ties = np.array([(corner(0, j), corner(nx, j)) for j in range(ny + 1)] + [(corner(i, 0), corner(i, ny)) for i in range(nx + 1)],
                    np.int32)
    return {"membrane": base,
            "shear": dataclasses.replace(base, springs=[(shear, k, None, S.SPRING)]),
            "long_ties": dataclasses.replace(base, springs=[(ties, k, 0.9 * S.pair_lengths(base.x, ties), S.SPRING)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="112,112")
    ap.add_argument("--k", type=float, default=5.0)
    ap.add_argument("--iters", type=int, default=100, help="iterations per bench_iterations call")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    nx, ny = (int(v) for v in a.size.split(","))
    ctx = capi.Context(0)
    scenes_ = spring_forms(nx, ny, a.k)
    res = {"scene": f"cloth({nx},{ny})", "k": a.k, "bench_iters": a.iters, "forms": {}}
    ctx.warm_dense()   # the process's one-time loads, kept out of the setup times
    bind(ctx, scenes_["membrane"]).close()
    solvers = {}
    for f, sc in scenes_.items():
        s = solvers[f] = bind(ctx, sc)
        rt = s.runtime()
        res["forms"][f] = {"elements": rt.n_elements, "springs": 0 if sc.springs is None else len(sc.springs[0][0]), "z_dim": rt.z_dim,
                           "nnz_L": int(rt.nnz_factor), "setup_ms": round(rt.setup_ms, 1), "runs": []}
        s.bench_iterations(5)   # warm-up
    for _ in range(a.runs):   # alternated
        for f, s in solvers.items():
            res["forms"][f]["runs"].append(measure(s, a.iters))
    med = {f: float(np.median([r["iter_us"] for r in v["runs"]])) for f, v in res["forms"].items()}
    res["iter_us_median"] = med
    cls = lambda f, k: float(np.median([r["class_us_per_iter"][k] for r in res["forms"][f]["runs"]]))
    res["ratio_over_membrane"] = {
        f: {"iteration": round(med[f] / med["membrane"], 4),
            "nnz_L": round(res["forms"][f]["nnz_L"] / res["forms"]["membrane"]["nnz_L"], 4),
            **{k: round(cls(f, k) / max(1e-9, cls("membrane", k)), 4) for k in ("local_z", "resid", "solve")}}
        for f in ("shear", "long_ties")}
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
