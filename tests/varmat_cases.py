"""Per-element material scenes of the varmat fixtures (tests/golden/varmat/*.npz): the builders the
generator (tests/golden/make_golden_varmat.py) runs through the reference, and the fixture
(de)serialisation. Every scene has a single group whose E / nu (/ strain limits) are arrays:
8 levels, assigned by scenes.with_material_levels with seed 7."""
from __future__ import annotations

import os

import numpy as np

from golden_io import GOLDEN, scenes

VARMAT = os.path.join(GOLDEN, "varmat")
K = np.arange(8) / 7.0
TET_LEVELS = dict(E_levels=1e5 * 100.0 ** K, nu_levels=0.30 + 0.15 * K)
DROP_LEVELS = dict(E_levels=1e6 * 10.0 ** K, nu_levels=0.30 + 0.15 * K)
CLOTH_LEVELS = dict(E_levels=30.0 + 50.0 * K, nu_levels=0.05 + 0.2 * K, lmin_levels=0.93 + 0.04 * K,
                    lmax_levels=1.03 + 0.04 * K)
# parity bars against the reference (golden_io.compare): L-BFGS prox path / closed-form prox
TOL = {"cant8_z_nh_aa6": 1e-6, "cant8_z_stvk_aa6": 1e-6, "drop6_z_nh_aa6": 1e-6, "cant8_ux_lin_aa6": 1e-9,
       "cloth12_ux_aa6": 1e-9}


def base_scenes():
    S = scenes
    return {
        "cant8_z_nh_aa6": (S.cantilever(8, 2, 2, S.NEOHOOKEAN, iters=30, n_steps=2), TET_LEVELS),
        "cant8_z_stvk_aa6": (S.cantilever(8, 2, 2, S.STVK, iters=30, n_steps=2), TET_LEVELS),
        "cant8_ux_lin_aa6": (S.cantilever(8, 2, 2, S.LINEAR, iters=30, n_steps=2, variant=S.VARIANT_H), TET_LEVELS),
        "drop6_z_nh_aa6": (S.tet_drop(6, 2, 3, iters=40, n_steps=2), DROP_LEVELS),
        "cloth12_ux_aa6": (S.cloth(12, 12, iters=40, n_steps=2), CLOTH_LEVELS),
    }


def cases():
    """{name: scene with per-element materials}"""
    return {name: scenes.with_material_levels(sc, **lv) for name, (sc, lv) in base_scenes().items()}


def mean_level_scene(name):
    """The fixture's scene with every element given the mean of the level tables (scalars)."""
    sc, lv = base_scenes()[name]
    g = sc.groups[0]
    g.E, g.nu = float(np.mean(lv["E_levels"])), float(np.mean(lv["nu_levels"]))
    if "lmin_levels" in lv:
        g.limit_min, g.limit_max = float(np.mean(lv["lmin_levels"])), float(np.mean(lv["lmax_levels"]))
    return sc


def names():
    return sorted(TOL)


def save(path, sc, steps):
    (g,) = sc.groups
    E, nu, lmin, lmax = g.material_arrays()
    d = dict(x=sc.x, masses=sc.masses, pin_idx=sc.pin_idx, pin_pts=sc.pin_pts, pin_vel=sc.pin_vel,
             kind=np.array(g.kind), material=np.array(g.material), idx=g.idx, E=E, nu=nu, limit_min=lmin,
             limit_max=lmax,
             settings=np.array([sc.variant, sc.dt, sc.gravity, sc.penalty, sc.iters, sc.accel, sc.aa_m, sc.n_steps]),
             nrec=np.array([len(s["prim"]) for s in steps]),
             prim=np.concatenate([s["prim"] for s in steps]), comb=np.concatenate([s["comb"] for s in steps]),
             reject=np.concatenate([s["reject"] for s in steps]),
             xs=np.stack([s["x"] for s in steps]), vs=np.stack([s["v"] for s in steps]))
    if sc.rest is not None:
        d["rest"] = sc.rest
    np.savez_compressed(path, **d)


def load(name):
    """(scene with one per-element group, the reference's per-step outputs)"""
    with np.load(os.path.join(VARMAT, name + ".npz")) as d:
        st = d["settings"]
        g = scenes.ElementGroup(int(d["kind"]), int(d["material"]), d["E"], d["nu"], d["idx"].astype(np.int32),
                                d["limit_min"], d["limit_max"])
        sc = scenes.Scene(x=d["x"], masses=d["masses"], groups=[g], pin_idx=d["pin_idx"].astype(np.int32),
                          pin_pts=d["pin_pts"], pin_vel=d["pin_vel"], variant=int(st[0]), dt=float(st[1]),
                          gravity=float(st[2]), penalty=float(st[3]), iters=int(st[4]), accel=int(st[5]),
                          aa_m=int(st[6]), n_steps=int(st[7]), name=name, rest=d["rest"] if "rest" in d.files else None)
        steps, o = [], 0
        for k, n in enumerate(d["nrec"]):
            steps.append(dict(prim=d["prim"][o:o + n], comb=d["comb"][o:o + n], reject=d["reject"][o:o + n],
                              x=d["xs"][k], v=d["vs"][k]))
            o += n
    return sc, steps
