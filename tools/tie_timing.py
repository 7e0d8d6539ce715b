"""What ties cost on the C2 cloth (scenes.cloth(), 112 x 112 cells, 50 176 triangles,
(u,x)-Anderson m=6): the scene as it is ("membrane"), with a spring between the opposite nodes of the
sheet's edges ("long_springs", tools/spring_timing.py's 226 long ties as two-node springs) and with
each of those nodes tied instead to a point inside a triangle at the opposite edge ("long_ties", 226
node-triangle ties, nv = 4, weights (0.5, 0.3, 0.2), 0.9 of their distance long): the same long-range
adjacency through three nodes per anchor. Three alternated runs of each in one process, with
Solver.bench_iterations / kernel_stats only. Per form: iteration time, the local_z, resid and solve
classes, the scalar factor's nnz(L), setup time and the element counts. No threshold: for the record.

    python tools/tie_timing.py --out profiles/ties.json
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spring_timing import S, bind, capi, measure, spring_forms   # noqa: E402


def tie_forms(nx, ny, k):
    """name -> scene: cloth(nx, ny), its long springs and the same as node-triangle ties."""
    forms = spring_forms(nx, ny, k)
    base = forms["membrane"]
    pairs = forms["long_ties"].springs[0][0]
    F = np.asarray(base.groups[0].idx, np.int32).reshape(-1, 3)
    first = {}   # node -> its first triangle
    for t, f in enumerate(F):
        for v in f:
            first.setdefault(int(v), t)
    tri = np.array([first[int(b)] for b in pairs[:, 1]])
    w = np.tile(np.array([[0.5, 0.3, 0.2]]), (len(pairs), 1))
    pa = (w[:, :, None] * base.x[F[tri]]).sum(1)
    d = base.x[pairs[:, 0]] - pa
    rest = 0.9 * np.sqrt((d * d).sum(1))
    entry = (F[tri], w, pairs[:, :1].astype(np.int32), np.ones((len(pairs), 1)), k, rest, S.SPRING)
    return {"membrane": base, "long_springs": forms["long_ties"], "long_ties": dataclasses.replace(base, ties=[entry])}


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
    scenes_ = tie_forms(nx, ny, a.k)
    res = {"scene": f"cloth({nx},{ny})", "k": a.k, "bench_iters": a.iters, "forms": {}}
    ctx.warm_dense()   # the process's one-time loads, kept out of the setup times
    bind(ctx, scenes_["membrane"]).close()
    solvers = {}
    for f, sc in scenes_.items():
        s = solvers[f] = bind(ctx, sc)
        rt = s.runtime()
        res["forms"][f] = {"elements": rt.n_elements, "springs": 0 if sc.springs is None else len(sc.springs[0][0]),
                           "ties": 0 if sc.ties is None else len(sc.ties[0][0]), "z_dim": rt.z_dim, "nnz_L": int(rt.nnz_factor),
                           "setup_ms": round(rt.setup_ms, 1), "runs": []}
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
        for f in ("long_springs", "long_ties")}
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
