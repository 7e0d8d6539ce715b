"""The deformation and the cases of the deforming mesh-obstacle tests
(tests/test_deforming_obstacle.py on the CPU, tests/test_gpu_deforming_obstacle.py on the GPU).

One orientation-preserving map of space with strength s, applied to a mesh's vertices -- a twist
about the y axis growing with y, a parabolic bend of y and an anisotropic stretch:
    a = 2.5 s y;  X = cos(a) x - sin(a) z;  Z = sin(a) x + cos(a) z;  Y = y + 0.8 s X X
    V' = ((1 + 0.4 s) X, Y, (1 - 0.3 s) Z)
Its Jacobian determinant is (1 + 0.4 s)(1 - 0.3 s) > 0, but the piecewise-linear image of a coarse
mesh can still invert at s = 1 (the sliver's volume turns negative), so the coarse meshes are used
at s = 0.5 only. On every case the signed volume is positive, the smallest triangle area is at
least 3e-4 and the oracle of tests/mesh_obs_cases.py is sound (test_deforming_obstacle.py checks it).
"""
import functools

import numpy as np

import mesh_obs_cases as mc


def deform(V, s):
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    a = 2.5 * s * y
    X = np.cos(a) * x - np.sin(a) * z
    Z = np.sin(a) * x + np.cos(a) * z
    Y = y + 0.8 * s * X * X
    return np.stack([(1.0 + 0.4 * s) * X, Y, (1.0 - 0.3 * s) * Z], axis=1)


def torus_fine():
    return mc.torus(48, 24)   # 2 304 triangles: the root covers more vertices than one block pass


MESHES = {"cube": mc.cube, "l_prism": mc.l_prism, "sliver": mc.sliver, "torus": mc.torus, "torus_fine": torus_fine}
CENTRED = ("cube", "l_prism", "sliver")   # centred on their vertex mean before the map

# (mesh, s); s = None is the identity V' = V
CASES = [("cube", 0.5), ("l_prism", 0.5), ("sliver", 0.5), ("torus", 0.5), ("torus", 1.0), ("torus_fine", 0.5),
         ("torus_fine", 1.0)] + [(name, None) for name in MESHES]
IDS = [f"{name}-{'id' if s is None else s}" for name, s in CASES]


@functools.lru_cache(maxsize=None)
def base(name):
    """(V, F) a case is built from; shared, do not modify."""
    V, F = MESHES[name]()
    if name in CENTRED:
        V = V - V.mean(0)
    return V, F


@functools.lru_cache(maxsize=None)
def shape(name, s):
    """(V, F, V') of a case; shared, do not modify."""
    V, F = base(name)
    return V, F, (V.copy() if s is None else deform(V, s))


@functools.lru_cache(maxsize=None)
def case(name, s):
    """(V, F, V', Q, Oracle(V', F, Q)) with Q = mc.queries(V', F); computed once per session."""
    V, F, W = shape(name, s)
    Q = mc.queries(W, F)
    return V, F, W, Q, mc.Oracle(W, F, Q)


def min_area(V, F):
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).min())
