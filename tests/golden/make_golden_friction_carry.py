"""Records what a build computes on scenes.block_on_moving_floor(1.0, shift=0.01, n_steps=40, iters=150): the
fixture of tests/test_gpu_friction_carry.py::test_gpu_no_carry_is_the_parent. Run on an MI355X with
AA_ADMM_LIB naming the library of the commit before carrying mesh obstacles (only entry points that
commit has are used):

    AA_ADMM_LIB=/path/to/parent/libaa_admm.so python tests/golden/make_golden_friction_carry.py

Writes tests/golden/friction_carry/parent_moving_floor.npz: x, v and the contact arrays of the last
step in full, and sha256 digests of x, v and the contact arrays over all steps.
"""
import hashlib
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
KEYS = ("node", "obstacle", "point", "normal", "push", "slip", "scale")


def digest(arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    pkg = importlib.import_module("aa-admm_amd")
    scenes, capi = pkg.scenes, pkg.capi
    print("library:", capi.LIB_PATH)
    ctx = capi.Context(0)
    sc = scenes.block_on_moving_floor(1.0, shift=0.01, n_steps=40, iters=150)
    s = capi.solver_from_scene(ctx, sc)
    s.initialize(capi.settings_from_scene(sc))
    xs, vs, cs = [], [], []
    for k in range(1, sc.n_steps + 1):
        for row, prm in enumerate(sc.obstacle_motion[k - 1]):
            s.set_obstacle(row, sc.obstacles[row][0], prm)
        s.step()
        xs.append(s.x); vs.append(s.v); cs.append(s.contacts())
    s.close()
    ctx.close()
    out = os.path.join(HERE, "friction_carry")
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "parent_moving_floor.npz"), x=xs[-1], v=vs[-1], x_digest=digest(xs), v_digest=digest(vs),
             contacts_digest=digest([c[k] for c in cs for k in KEYS]), **{k: cs[-1][k] for k in KEYS})
    print("contacts in the last step:", len(cs[-1]["node"]), "x digest", digest(xs))


if __name__ == "__main__":
    main()
