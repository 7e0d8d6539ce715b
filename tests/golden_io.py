"""Golden-fixture (de)serialisation: scene arrays + reference outputs as .npz (data only)."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
scenes = importlib.import_module("aa-admm_amd.scenes")
geom_scenes = importlib.import_module("aa-admm_amd.geom_scenes")
GOLDEN = os.path.join(REPO, "tests", "golden")
MAX_FILE_BYTES = 1 << 20   # no committed file is larger


def _parts_path(path):
    return os.path.join(os.path.dirname(path), "parts", os.path.basename(path))


def save_npz(path, d):
    """np.savez_compressed(path, **d) for a fixture that may not fit one committed file: while
    the file is above MAX_FILE_BYTES its largest array moves to parts/<file name> beside it
    (load_npz merges the two)."""
    main, rest = dict(d), {}
    np.savez_compressed(path, **main)
    for k in sorted(d, key=lambda k: -np.asarray(d[k]).nbytes):
        if os.path.getsize(path) <= MAX_FILE_BYTES:
            break
        rest[k] = main.pop(k)
        np.savez_compressed(path, **main)
    if rest:
        os.makedirs(os.path.dirname(_parts_path(path)), exist_ok=True)
        np.savez_compressed(_parts_path(path), **rest)
        assert os.path.getsize(_parts_path(path)) <= MAX_FILE_BYTES, "fixture needs more than two files"


def load_npz(path):
    """{name: array} of a fixture, with the arrays save_npz moved to parts/<file name>."""
    d = {}
    for p in (path, _parts_path(path)):
        if os.path.exists(p):
            with np.load(p) as z:
                d.update({k: z[k] for k in z.files})
    if not d:
        raise FileNotFoundError(path)
    return d


def save_case(path, sc, steps):
    d = dict(
        x=sc.x, masses=sc.masses, pin_idx=sc.pin_idx, pin_pts=sc.pin_pts, pin_vel=sc.pin_vel,
        g_kind=np.array([g.kind for g in sc.groups]), g_mat=np.array([g.material for g in sc.groups]),
        g_E=np.array([g.E for g in sc.groups]), g_nu=np.array([g.nu for g in sc.groups]),
        g_lmin=np.array([g.limit_min for g in sc.groups]), g_lmax=np.array([g.limit_max for g in sc.groups]),
        settings=np.array([sc.variant, sc.dt, sc.gravity, sc.penalty, sc.iters, sc.accel, sc.aa_m, sc.n_steps]),
        nrec=np.array([len(s["prim"]) for s in steps]),
        prim=np.concatenate([s["prim"] for s in steps]), comb=np.concatenate([s["comb"] for s in steps]),
        reject=np.concatenate([s["reject"] for s in steps]),
        xs=np.stack([s["x"] for s in steps]), vs=np.stack([s["v"] for s in steps]),
    )
    if all("resets" in s for s in steps):   # z-AA reference: its printed per-step reject counts
        d["ref_resets"] = np.array([s["resets"] for s in steps])
        d["reject_exact"] = np.array([s["reject_exact"] for s in steps])
    for i, g in enumerate(sc.groups):
        d[f"g{i}_idx"] = g.idx
    if sc.rest is not None:
        d["rest"] = sc.rest
    obs = getattr(sc, "obstacles", [])
    if obs:
        o = np.zeros((len(obs), 9))
        for k, (kind, prm) in enumerate(obs):
            q = np.asarray(prm, np.float64).reshape(-1)
            o[k, 0] = kind
            o[k, 1:1 + len(q)] = q
        d["obstacles"] = o
    if getattr(sc, "collision_idx", None) is not None:
        d["collision_idx"] = np.asarray(sc.collision_idx, np.int32)
    for k, (tris, direction) in enumerate(getattr(sc, "winds", [])):
        d[f"wind{k}_tris"] = np.asarray(tris, np.int32)
        d[f"wind{k}_dir"] = np.asarray(direction, np.float64)
    np.savez_compressed(path, **d)


def load_case(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    st = d["settings"]
    groups = [scenes.ElementGroup(int(d["g_kind"][i]), int(d["g_mat"][i]), float(d["g_E"][i]), float(d["g_nu"][i]),
                                  d[f"g{i}_idx"].astype(np.int32), float(d["g_lmin"][i]), float(d["g_lmax"][i]))
              for i in range(len(d["g_kind"]))]
    sc = scenes.Scene(x=d["x"], masses=d["masses"], groups=groups, pin_idx=d["pin_idx"].astype(np.int32),
                      pin_pts=d["pin_pts"], pin_vel=d["pin_vel"], variant=int(st[0]), dt=float(st[1]),
                      gravity=float(st[2]), penalty=float(st[3]), iters=int(st[4]), accel=int(st[5]),
                      aa_m=int(st[6]), n_steps=int(st[7]), name=name,
                      rest=d["rest"] if "rest" in d.files else None)
    if "obstacles" in d.files:
        sc.obstacles = [(int(r[0]), r[1:].copy()) for r in d["obstacles"]]
    if "collision_idx" in d.files:
        sc.collision_idx = d["collision_idx"].astype(np.int32)
    k = 0
    while f"wind{k}_tris" in d.files:
        sc.winds.append((d[f"wind{k}_tris"].astype(np.int32), d[f"wind{k}_dir"]))
        k += 1
    steps, o = [], 0
    for k, n in enumerate(d["nrec"]):
        steps.append(dict(prim=d["prim"][o:o + n], comb=d["comb"][o:o + n], reject=d["reject"][o:o + n],
                          x=d["xs"][k], v=d["vs"][k]))
        o += n
    return sc, steps


def case_names(extras=True):
    """Elastic trajectory fixtures; extras=False leaves out the scenes with obstacles, collision
    terms or wind (the oracle restates the core path only; those are pinned to the reference's
    own outputs directly)."""
    names = sorted(f[:-4] for f in os.listdir(GOLDEN)
                   if f.endswith(".npz") and f not in ("elements.npz", "geom_elements.npz", "anderson.npz")
                   and not f.startswith(("geom_", "full_", "mesh_", "eps_", "quality_")))
    if extras:
        return names
    out = []
    for n in names:
        with np.load(os.path.join(GOLDEN, n + ".npz")) as d:
            if not any(k in d.files for k in ("obstacles", "collision_idx", "wind0_tris")):
                out.append(n)
    return out


# ---------------------------------------------------------------------------- Geometry (ALM)
def save_geom_case(path, sc, outputs):
    d = dict(x0=sc.x0, ref_points=sc.ref_points, reg_kind=sc.reg_kind, reg_ptr=sc.reg_ptr, reg_idx=sc.reg_idx,
             reg_coef=sc.reg_coef, reg_weight=sc.reg_weight, reg_target=sc.reg_target,
             settings=np.array([sc.penalty, sc.iters, sc.aa_m, sc.avg_edge_length(),
                                1.0 if getattr(sc, "solver", "alm") == "plain" else 0.0]),
             g_meta=np.array([[g.type, int(g.hard), g.k] for g in sc.groups], np.int32).reshape(-1, 3),
             g_weight=np.array([g.weight for g in sc.groups], np.float64))
    for i, g in enumerate(sc.groups):
        d[f"g{i}_idx"] = g.idx
        if g.params is not None:
            d[f"g{i}_params"] = g.params
    for i, (V, F) in enumerate(sc.surfaces):
        d[f"s{i}_V"], d[f"s{i}_F"] = V, F
    for k, v in outputs.items():
        d["out_" + k] = v
    save_npz(path, d)


def load_geom_case(name):
    d = load_npz(os.path.join(GOLDEN, name + ".npz"))
    gs = geom_scenes
    groups = []
    for i, (t, h, k) in enumerate(d["g_meta"]):
        groups.append(gs.ConstraintGroup(int(t), d[f"g{i}_idx"].astype(np.int32), float(d["g_weight"][i]), bool(h),
                                         d[f"g{i}_params"] if f"g{i}_params" in d else None))
    surfaces, i = [], 0
    while f"s{i}_V" in d:
        surfaces.append((d[f"s{i}_V"], d[f"s{i}_F"].astype(np.int32)))
        i += 1
    st = d["settings"]
    sc = gs.GeomScene(x0=d["x0"], groups=groups, reg_kind=d["reg_kind"].astype(np.int32),
                      reg_ptr=d["reg_ptr"].astype(np.int32), reg_idx=d["reg_idx"].astype(np.int32),
                      reg_coef=d["reg_coef"], reg_weight=d["reg_weight"], reg_target=d["reg_target"],
                      ref_points=d["ref_points"], surfaces=surfaces, penalty=float(st[0]), iters=int(st[1]),
                      aa_m=int(st[2]), name=name, solver="plain" if len(st) > 4 and st[4] == 1.0 else "alm")
    sc._avg_edge = float(st[3])
    out = {k[4:]: d[k] for k in d if k.startswith("out_")}
    return sc, out


def geom_case_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("geom_") and f.endswith(".npz")
                  and f != "geom_elements.npz")


def compare_geom(ref, got, tol_comb, tol_x, n_check=None):
    """ALM residual curves judged relative to comb_0, plus the solution (get_solution)."""
    fails = []
    n = min(len(ref["comb"]), len(got["comb"]))
    if len(ref["comb"]) != len(got["comb"]):
        fails.append(f"record count {len(got['comb'])} != {len(ref['comb'])}")
    if n_check is not None:
        n = min(n, n_check)
    c0 = ref["comb"][0]
    dc = np.max(np.abs(ref["comb"][:n] - got["comb"][:n])) / c0
    if not dc <= tol_comb:
        fails.append(f"comb dev {dc:.3e} (tol {tol_comb:g})")
    xr, xg = ref["x"], got["x"]
    dx = np.linalg.norm(xr - xg) / np.linalg.norm(xr)
    if not dx <= tol_x:
        fails.append(f"final x rel err {dx:.3e} (tol {tol_x:g})")
    return fails


def compare(ref_steps, got_steps, tol_comb, tol_x, n_check=None):
    """Per-iteration residual parity judged relative to comb_0 / prim_0 of each time step
    (SURVEY.md §8c, Appendix B.12), plus final positions. Returns a list of failures."""
    fails = []
    for k, (r, g) in enumerate(zip(ref_steps, got_steps)):
        n = min(len(r["comb"]), len(g["comb"]))
        if n_check is not None:
            n = min(n, n_check)
        if n == 0:
            continue
        c0, p0 = r["comb"][0], r["prim"][0]
        dc = np.max(np.abs(r["comb"][:n] - g["comb"][:n])) / c0
        dp = np.max(np.abs(r["prim"][:n] - g["prim"][:n])) / p0
        if not (dc <= tol_comb and dp <= tol_comb * 10):
            fails.append(f"step {k}: comb dev {dc:.3e} prim dev {dp:.3e} (tol {tol_comb:g})")
        nr = min(n, 20)
        if np.any(r["reject"][:nr] != g["reject"][:nr]):
            fails.append(f"step {k}: reject flags differ in the first {nr} iterations")
    xr, xg = ref_steps[-1]["x"], got_steps[-1]["x"]
    dx = np.linalg.norm(xr - xg) / np.linalg.norm(xr)
    if not dx <= tol_x:
        fails.append(f"final x rel err {dx:.3e} (tol {tol_x:g})")
    return fails


def check_full_golden(got, ref, reject_slack=0):
    """A C4-recipe run against a reference fixture of make_golden.py --full / --bunny: per-step
    residual curves relative to comb_0 (1e-6, L-BFGS prox path; prim 1e-5), reject flags (equal,
    or at most reject_slack differing per step), positions and velocities on the sampled nodes
    and their column sums (1e-6 relative). Returns a list of failures."""
    fails = []
    o = 0
    for k, n in enumerate(ref["nrec"]):
        h = got[k]
        rc, rp, rr = ref["comb"][o:o + n], ref["prim"][o:o + n], ref["reject"][o:o + n]
        o += n
        if len(h["comb"]) != n:
            fails.append(f"step {k}: {len(h['comb'])} records, want {n}")
            continue
        dc = np.abs(h["comb"] - rc).max() / rc[0]
        if not dc <= 1e-6:
            fails.append(f"step {k}: comb dev {dc:.3e}")
        dp = np.abs(h["prim"] - rp).max() / rp[0]
        if not dp <= 1e-5:
            fails.append(f"step {k}: prim dev {dp:.3e}")
        nrej = int((np.asarray(h["reject"]) != rr).sum())
        if nrej > reject_slack:
            fails.append(f"step {k}: {nrej} reject flags differ")
        # the z-AA reference prints its per-step reject count (Solver.cpp:253) but logs no flags: a
        # reject whose recomputed prim does not rise is invisible in the fixture's flags, the count
        # still holds it
        if "ref_resets" in ref.files and int(np.sum(h["reject"])) != int(ref["ref_resets"][k]):
            fails.append(f"step {k}: {int(np.sum(h['reject']))} rejects, the reference {int(ref['ref_resets'][k])}")
        for key in ("x", "v"):
            want = ref[key + "_sample"][k]
            scale = np.abs(want).max()
            hk = np.asarray(h[key]).reshape(-1, 3)
            if not np.abs(hk[ref["sample"]] - want).max() <= 1e-6 * scale:
                fails.append(f"step {k}: {key} samples")
            if not np.allclose(hk.sum(0), ref[key + "_sum"][k], rtol=1e-6, atol=1e-6 * scale * len(hk)):
                fails.append(f"step {k}: {key} column sums")
    return fails
