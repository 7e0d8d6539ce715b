"""What a bound mesh obstacle costs, for the record (no threshold): cloth_on_soft_block scaled up -- a
thin soft block whose surface has some 10^5 triangles under a 64 x 64 cloth -- run bound
(aa_elastic_bind_mesh_obstacle: gather, check and refit on the device at the top of every step) and
run scripted (the same scene unbound, set_mesh_obstacle_vertices(0, x[nodes]) from the host before
every step, the setter's time counted with the step). `runs` alternated runs each, `steps` timed
steps after `warmup`; per run the mean wall ms per step, then their mean and spread (max - min).
The device time of gather + check + refit comes from the aa_test_bound_refit hook on the same
surface: device events, the median of 5 after a warm-up.

Prints one JSON line; --out writes it to a file.

    python tools/bound_obstacle_timing.py --out profiles/bound_obstacle.json
"""
import argparse
import dataclasses
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("aa-admm_amd")
capi, scenes = pkg.capi, pkg.scenes


def run(ctx, sc, nodes, bound, warmup, steps):
    s = capi.solver_from_scene(ctx, sc if bound else dataclasses.replace(sc, mesh_obstacle_bindings=None))
    s.initialize(capi.settings_from_scene(sc))
    ms = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        if not bound:
            s.set_mesh_obstacle_vertices(0, s.x[nodes])
        s.step()
        if k >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    x = s.x.copy()
    st = s.mesh_obstacle_status(0)
    s.close()
    return float(np.mean(ms)), x, st


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", default="160,2,160", help="the block in cubes (six tets each)")
    ap.add_argument("--cloth", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    cells = tuple(int(c) for c in a.cells.split(","))
    sc = scenes.cloth_on_soft_block(a.cloth, a.cloth, cells=cells, cell=0.9 / max(cells), iters=a.iters, n_steps=a.warmup + a.steps)
    nodes = sc.mesh_obstacle_bindings[0]
    V, F = sc.mesh_obstacles[0]
    ctx = capi.Context(0)
    bound, scripted, same = [], [], True
    for r in range(a.runs):
        tb, xb, st = run(ctx, sc, nodes, True, a.warmup, a.steps)
        ts, xs, _ = run(ctx, sc, nodes, False, a.warmup, a.steps)
        bound.append(tb)
        scripted.append(ts)
        same = same and bool(np.array_equal(xb, xs))
        print(f"run {r}: bound {tb:.3f} ms / step, scripted {ts:.3f} ms / step, bitwise equal {np.array_equal(xb, xs)}, {st}", file=sys.stderr)
    dev = [capi.hook_bound_refit(ctx, V, F, sc.x, nodes, device=1, timing=True)["ms"] for _ in range(a.runs)]
    ctx.close()
    stat = lambda v: dict(runs=[round(x, 4) for x in v], mean=round(float(np.mean(v)), 4), spread=round(float(max(v) - min(v)), 4))
    line = json.dumps(dict(tool="bound_obstacle_timing", surface_triangles=int(len(F)), surface_vertices=int(len(V)),
                           nodes=int(sc.n_nodes), tets=int(len(sc.groups[0].idx)), cloth_triangles=int(len(sc.groups[1].idx)),
                           iters=a.iters, steps=a.steps, warmup=a.warmup, step_ms_bound=stat(bound), step_ms_scripted=stat(scripted),
                           device_gather_check_refit_ms=stat(dev), trajectories_bitwise_equal=same))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
