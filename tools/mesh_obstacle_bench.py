"""What a triangle-mesh obstacle costs the collision terms' local step, for the record (no
threshold): the obstacle-course scene (scenes.obstacle_course on the 759-node horse, every node
collision-checked) with its analytic sphere, with an icosphere of about 5 k triangles in the
sphere's place, and with neither.

Per form: the "local_z" kernel class per pass from Solver.bench_iterations / kernel_stats (the
tet group's launch plus the collision group's; the tet group is the same in every form, so the
differences between forms are the collision kernel's), the step time, and -- for the mesh -- the
share of collision nodes inside the mesh's root box at the end of each step, i.e. the share of
lanes that pass the cull and walk the BVH.

--posed measures the kinematic obstacle instead: the icosphere as above against the same icosphere
given in a frame turned by a constant non-trivial pose's inverse and posed back
(Solver.set_mesh_obstacle_pose), i.e. the same world surface through the posed path.

Prints one JSON line; --out writes it to a file.

    python tools/mesh_obstacle_bench.py --out profiles/mesh_obstacle.json
    python tools/mesh_obstacle_bench.py --posed --out profiles/kinematic_obstacle.json
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


def icosphere(center, radius, level):
    """20 x 4^level triangles, outward."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, G = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return np.asarray(center, float) + radius * np.array(V), np.array(F, np.int32)


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def measure(ctx, sc, iters, steps, mesh=None, pose=None):
    """mesh: the obstacle's world-frame surface (for the root-box share); pose: set on mesh 0."""
    s = capi.solver_from_scene(ctx, sc)
    if pose is not None:
        s.set_mesh_obstacle_pose(0, *pose)
    s.initialize(capi.settings_from_scene(sc))
    share, step_ms = [], []
    for _ in range(steps):
        s.step()
        step_ms.append(s.runtime().step_ms)
        if mesh is not None:
            lo, hi = mesh[0].min(0), mesh[0].max(0)
            x = s.x.reshape(-1, 3)[sc.collision_idx]
            share.append(float(((x >= lo) & (x <= hi)).all(1).mean()))
    s.bench_iterations(5)   # warm-up
    runs = []
    for _ in range(3):
        s.bench_iterations(iters)
        runs.append(round(1e3 * s.kernel_stats("local_z")["avg_ms"], 2))
    s.close()
    out = {"local_z_us_per_pass": runs, "step_ms_median": round(float(np.median(step_ms[1:])), 3)}
    if mesh is not None:
        out["triangles"] = int(len(mesh[1]))
        out["root_box_share_per_step"] = [round(v, 3) for v in share]
        out["root_box_share_mean"] = round(float(np.mean(share)), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60, help="iterations per bench_iterations call")
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--level", type=int, default=4, help="icosphere subdivisions (4: 5 120 triangles)")
    ap.add_argument("--posed", action="store_true", help="the posed leg: icosphere unposed against a constant pose")
    ap.add_argument("--out")
    a = ap.parse_args()
    d = np.load(os.path.join(REPO, "tests", "golden", "mesh_horse759.npz"))
    base = S.obstacle_course(d["verts"], d["tets"], n_steps=a.steps)
    k = next(i for i, (kind, _) in enumerate(base.obstacles) if kind == S.OBS_SPHERE)
    prm = base.obstacles[k][1]
    mesh = icosphere(prm[:3], prm[3], a.level)
    rest = [o for i, o in enumerate(base.obstacles) if i != k]
    ctx = capi.Context(0)
    res = {"scene": "obstacle_course(horse759)", "collision_nodes": int(len(base.collision_idx)),
           "library": os.path.basename(capi.LIB_PATH), "bench_iters": a.iters, "forms": {}}
    forms = {"analytic_sphere": (base.obstacles, None, None), "no_sphere": (rest, None, None), "icosphere": (rest, mesh, None)}
    if a.posed:
        R, t = rotation((1.0, 2.0, 3.0), 0.7), np.array([0.3, -1.25, 2.0])
        res["pose"] = {"axis": [1, 2, 3], "angle_rad": 0.7, "t": t.tolist()}
        forms = {"icosphere": (rest, mesh, None), "icosphere_posed": (rest, mesh, (R, t))}
    for name, (obs, m, pose) in forms.items():
        sc = S.obstacle_course(d["verts"], d["tets"], n_steps=a.steps)
        sc.obstacles = list(obs)
        if m is not None:   # posed: the surface given as R^T (v - t), so that the pose puts it back
            sc.mesh_obstacles = [m if pose is None else ((m[0] - pose[1]) @ pose[0], m[1])]
        res["forms"][name] = measure(ctx, sc, a.iters, a.steps, m, pose)
    f = res["forms"]
    med = lambda n: float(np.median(f[n]["local_z_us_per_pass"]))
    if a.posed:
        res["posed_minus_unposed_us_per_pass"] = round(med("icosphere_posed") - med("icosphere"), 2)
    else:
        res["icosphere_minus_analytic_sphere_us_per_pass"] = round(med("icosphere") - med("analytic_sphere"), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
