"""What carry costs the friction pass, for the record (no threshold): the obstacle-course scene of
tools/contact_friction_timing.py (scenes.obstacle_course on the 759-node horse, every node
collision-checked, an icosphere of 5 120 triangles in its sphere's place, a friction coefficient on
every obstacle row), carry off against carry on for the icosphere. The carry-on leg calls the vertex
setter before every step with unchanged vertices, so both legs compute the same trajectory and the
pass does the same contacts' work. Per leg the device time of the pass per step (device events,
Solver.kernel_stats("friction")) and, with carry, of the refresh of the previous vertices alone
(Solver.kernel_stats("carry_copy")): three alternated runs each.

Prints one JSON line; --out writes it to a file.

    python tools/friction_carry_timing.py --out profiles/friction_carry.json
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


def run(ctx, sc, steps, carry):
    s = capi.solver_from_scene(ctx, sc)
    s.initialize(capi.settings_from_scene(sc))
    V = np.asarray(sc.mesh_obstacles[0][0], float)
    if carry:
        s.set_mesh_obstacle_carry(0, True)
    pass_ms, copy_ms, step_ms, contacts = [], [], [], []
    for _ in range(steps):
        if carry:
            s.set_mesh_obstacle_vertices(0, V)
        s.step()
        step_ms.append(s.runtime().step_ms)
        pass_ms.append(s.kernel_stats("friction")["avg_ms"])
        contacts.append(int(len(s.contacts()["node"])))
        if carry:
            copy_ms.append(s.kernel_stats("carry_copy")["avg_ms"])
    x = s.x
    s.close()
    return dict(pass_ms=pass_ms, copy_ms=copy_ms, step_ms=step_ms, contacts=contacts, x=x)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--mu", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = np.load(os.path.join(REPO, "tests", "golden", "mesh_horse759.npz"))
    sc = S.obstacle_course(d["verts"], d["tets"], n_steps=a.steps)
    kind, prm = sc.obstacles[0]
    sc.obstacles = sc.obstacles[1:]
    sc.mesh_obstacles = [icosphere(prm[:3], prm[3], 4)]
    rows = len(sc.obstacles) + 1
    sc = dataclasses.replace(sc, obstacle_friction=[a.mu] * rows)
    ctx = capi.Context(0)
    run(ctx, sc, 2, False)   # warm-up
    run(ctx, sc, 2, True)
    legs = {"off": [], "on": []}
    for _ in range(a.runs):   # alternated
        legs["off"].append(run(ctx, sc, a.steps, False))
        legs["on"].append(run(ctx, sc, a.steps, True))
    same = all(np.array_equal(legs["off"][0]["x"], r["x"]) for leg in legs.values() for r in leg)
    med = lambda leg, key: [round(float(np.median(r[key])), 5) for r in legs[leg]]
    tot = lambda leg, key: [round(float(np.sum(r[key])), 5) for r in legs[leg]]
    out = {
        "what": "obstacle course (horse759, every node a collision term) with a 5 120-triangle icosphere, friction on every row; "
                "device time of the friction pass per step (device events), carry off against carry on for the icosphere (the "
                "vertex setter called before every step with unchanged vertices), and of the refresh of the previous vertices alone",
        "collision_terms": int(len(sc.collision_idx)), "mesh_triangles": int(len(sc.mesh_obstacles[0][1])),
        "mesh_vertices": int(len(sc.mesh_obstacles[0][0])), "mu": a.mu, "steps": a.steps, "runs": a.runs, "iters_per_step": sc.iters,
        "trajectories_bitwise_equal": bool(same),
        "contacts_per_step": legs["on"][0]["contacts"],
        "pass_ms_median_per_run_carry_off": med("off", "pass_ms"), "pass_ms_median_per_run_carry_on": med("on", "pass_ms"),
        "pass_ms_sum_per_run_carry_off": tot("off", "pass_ms"), "pass_ms_sum_per_run_carry_on": tot("on", "pass_ms"),
        "pass_ms_per_step_carry_off": [round(v, 5) for v in legs["off"][0]["pass_ms"]],
        "pass_ms_per_step_carry_on": [round(v, 5) for v in legs["on"][0]["pass_ms"]],
        "carry_copy_ms_median_per_run": med("on", "copy_ms"),
        "step_ms_median_per_run_carry_off": med("off", "step_ms"), "step_ms_median_per_run_carry_on": med("on", "step_ms"),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
