"""What a deforming mesh obstacle costs, for the record (no threshold): the device refit
(aa_elastic_set_mesh_obstacle_vertices, csrc/mesh_refit.hip) beside the host preparation plus upload
it replaces, and the signed-distance kernel on the refitted tree -- whose node axes are those of the
shape the tree was built for -- beside the same kernel on a tree freshly built for the new shape.

A torus of nu x nv quads (default 448 x 224: 200 704 triangles) is built, then refitted to its image
under the test suite's deformation (tests/deform_cases.py: a twist about y growing with y, a
parabolic bend, an anisotropic stretch) at strengths s = 0 (the identity), 0.5 and 1.0. The queries
are uniform in the deformed shape's bounding box inflated by 25 %. Times come from the
aa_test_mesh_sdf_deformed hook: wall time for the host path, device events (median of 5 after a
warm-up) for the kernels.

Prints one JSON line; --out writes it to a file.

    python tools/mesh_refit_timing.py --out profiles/mesh_refit.json
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
capi = pkg.capi


def torus(nu, nv, R=0.35, r=0.15):
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    U, W = np.meshgrid(u, v, indexing="ij")
    V = np.stack([(R + r * np.cos(W)) * np.cos(U), r * np.sin(W), (R + r * np.cos(W)) * np.sin(U)], -1).reshape(-1, 3)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"))
    idx = lambda a, b: (a % nu) * nv + (b % nv)
    p00, p01, p11, p10 = idx(i, j), idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)
    F = np.concatenate([np.stack([p00, p01, p11], 1), np.stack([p00, p11, p10], 1)])
    return V, F.astype(np.int32)


def deform(V, s):
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    a = 2.5 * s * y
    X = np.cos(a) * x - np.sin(a) * z
    Z = np.sin(a) * x + np.cos(a) * z
    Y = y + 0.8 * s * X * X
    return np.stack([(1.0 + 0.4 * s) * X, Y, (1.0 - 0.3 * s) * Z], axis=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nu", type=int, default=448)
    ap.add_argument("--nv", type=int, default=224)
    ap.add_argument("--queries", type=int, default=1 << 17)
    ap.add_argument("--out")
    a = ap.parse_args()
    V, F = torus(a.nu, a.nv)
    ctx = capi.Context(0)
    rows = []
    for s in (0.0, 0.5, 1.0):
        W = deform(V, s)
        lo, hi = W.min(0), W.max(0)
        Q = np.random.default_rng(7).uniform(lo - 0.125 * (hi - lo), hi + 0.125 * (hi - lo), size=(a.queries, 3))
        c, dx, tri, ms = capi.hook_mesh_sdf_deformed(ctx, V, F, W, Q, timings=True)
        c2, dx2, tri2 = capi.hook_mesh_sdf(ctx, W, F, Q)
        rows.append(dict(s=s, host_prepare_upload_ms=ms[0], device_refit_ms=ms[1], sdf_refitted_ms=ms[2], sdf_fresh_ms=ms[3],
                         sdf_ratio=ms[2] / ms[3], refit_speedup=ms[0] / ms[1], inside_share=float((dx < 0).mean()),
                         max_abs_dx_diff_vs_fresh=float(np.abs(dx - dx2).max())))
        print(f"s={s}: host prepare + upload {ms[0]:.1f} ms, device refit {ms[1]:.3f} ms, sdf on the refitted tree {ms[2]:.3f} ms, "
              f"on a fresh tree {ms[3]:.3f} ms (x{ms[2] / ms[3]:.2f})", file=sys.stderr)
    ctx.close()
    line = json.dumps(dict(tool="mesh_refit_timing", triangles=int(len(F)), vertices=int(len(V)), queries=a.queries, rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
