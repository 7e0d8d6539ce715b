"""One rank of a partitioned run of a per-element material scene (after tests/part_worker.py;
launched by torch.distributed.run from tests/test_gpu_varmat.py). Every rank binds the same scene
as one per-element group, attaches a host communicator and runs the time steps; rank r writes its
per-step history and final state to OUT/rank{r}.npz.

    AA_OUT=<dir> python -m torch.distributed.run ... varmat_part_worker.py
"""
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def scene():
    """tet_drop(12, 4, 6) (1 440 NeoHookean tets, no pins) with the drop fixture's 8 levels"""
    import varmat_cases
    S = varmat_cases.scenes
    return S.with_material_levels(S.tet_drop(12, 4, 6, iters=40, n_steps=2), **varmat_cases.DROP_LEVELS)


def main():
    # no torch in a rank process (aa-admm_amd/dist.py rank_setup; the rendezvous is aa-admm_amd/rdzv.py)
    pkg = importlib.import_module("aa-admm_amd")
    group, report = pkg.dist.rank_setup()
    rank = group.rank
    with open(os.path.join(os.environ["AA_OUT"], f"rank{rank}.runtime.json"), "w") as f:
        json.dump(report, f)
    ctx = pkg.capi.Context(int(os.environ.get("AA_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    comm = pkg.dist.host_comm(group)
    steps, s = pkg.capi.run_scene(ctx, scene(), comm=comm)
    out = {}
    for k, st in enumerate(steps):
        for key in ("prim", "comb", "reject", "x", "v"):
            out[f"{key}{k}"] = st[key]
    out["n_elements"] = np.array([s.runtime().n_elements])
    np.savez(os.path.join(os.environ["AA_OUT"], f"rank{rank}.npz"), **out)
    s.close()
    comm.close()
    ctx.close()
    group.close()


if __name__ == "__main__":
    try:
        main()
    except BaseException:   # the rank's own traceback, where the test can read it
        import traceback
        with open(os.path.join(os.environ.get("AA_OUT", "."), f"rank{os.environ.get('RANK', '0')}.err"), "w") as f:
            traceback.print_exc(file=f)
        raise
