"""What the friction pass costs, for the record (no threshold): the obstacle-course scene
(scenes.obstacle_course on the 759-node horse, every node collision-checked) with an icosphere of
5 120 triangles in its sphere's place and a friction coefficient on every obstacle row. Per step
the device time of the friction pass (device events around it, Solver.kernel_stats("friction")) and
the terms in contact; beside it the scene's "local_z" kernel class per pass from
Solver.bench_iterations, and the step time with and without the pass.

Prints one JSON line; --out writes it to a file.

    python tools/contact_friction_timing.py --out profiles/contact_friction.json
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
sys.path.insert(0, os.path.join(REPO, "tools"))
pkg = importlib.import_module("aa-admm_amd")
capi, S = pkg.capi, pkg.scenes
from mesh_obstacle_bench import icosphere  # noqa: E402


def run(ctx, sc, steps):
    s = capi.solver_from_scene(ctx, sc)
    s.initialize(capi.settings_from_scene(sc))
    pass_ms, step_ms, contacts = [], [], []
    for _ in range(steps):
        s.step()
        step_ms.append(s.runtime().step_ms)
        if sc.obstacle_friction:
            pass_ms.append(s.kernel_stats("friction")["avg_ms"])
            contacts.append(int(len(s.contacts()["node"])))
    s.bench_iterations(sc.iters)
    lz = s.kernel_stats("local_z")
    s.close()
    return pass_ms, step_ms, contacts, lz


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--mu", type=float, default=0.3)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = np.load(os.path.join(REPO, "tests", "golden", "mesh_horse759.npz"))
    sc = S.obstacle_course(d["verts"], d["tets"], n_steps=a.steps)
    kind, prm = sc.obstacles[0]
    sc.obstacles = sc.obstacles[1:]
    sc.mesh_obstacles = [icosphere(prm[:3], prm[3], 4)]
    rows = len(sc.obstacles) + 1
    ctx = capi.Context(0)
    with_f = dataclasses.replace(sc, obstacle_friction=[a.mu] * rows)
    run(ctx, with_f, 2)   # warm-up
    pass_ms, step_f, contacts, lz = run(ctx, with_f, a.steps)
    _, step_0, _, _ = run(ctx, sc, a.steps)
    out = {
        "what": "obstacle course (horse759, every node a collision term) with a 5 120-triangle icosphere, friction on every row; "
                "device time of the friction pass per step (device events) beside the local_z kernel class per pass",
        "collision_terms": int(len(sc.collision_idx)), "mesh_triangles": int(len(sc.mesh_obstacles[0][1])), "mu": a.mu,
        "steps": a.steps, "iters_per_step": sc.iters,
        "friction_pass_ms_per_step": [round(v, 5) for v in pass_ms], "friction_pass_ms_median": round(float(np.median(pass_ms)), 5),
        "contacts_per_step": contacts,
        "local_z_ms_per_pass": round(lz["avg_ms"], 5), "local_z_passes_timed": lz["launches"],
        "step_ms_median_with_friction": round(float(np.median(step_f)), 4), "step_ms_median_without": round(float(np.median(step_0)), 4),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
