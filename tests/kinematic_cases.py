"""Poses, the numpy restatement of the device transform and the posed oracles of the kinematic
mesh-obstacle tests (tests/test_kinematic_obstacle.py on the CPU, tests/test_gpu_kinematic_obstacle.py
on the GPU).

A posed obstacle is seen in the world as R v + t for its vertices v. The device (csrc/device_prox.hpp,
mesh_signed_distance) takes a candidate into the obstacle frame and the closest point back in a fixed
operation order without FMA contraction, restated here operation by operation:
    d = q - t;  q_l[i] = (R[0][i] d0 + R[1][i] d1) + R[2][i] d2
    c_w[i] = ((R[i][0] c0 + R[i][1] c1) + R[i][2] c2) + t[i]
Each (mesh, pose) case carries two oracles: O_l, the unposed mesh asked at q_l (what the device is
specified to compute), and O_w, the mesh with its vertices moved to the world frame asked at the
world queries (independent of the transform's direction).
"""
import functools
import types

import numpy as np

import mesh_obs_cases as mc


def rotation(axis, angle):
    """Rodrigues' rotation about `axis` by `angle` (3, 3)."""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


POSES = {
    "P_rot": (rotation((1.0, 2.0, 3.0), 0.7), np.array([0.3, -1.25, 2.0])),
    "P_tr": (np.eye(3), np.array([0.5, 0.25, -0.125])),
    "P_flip": (np.diag([1.0, -1.0, -1.0]), np.zeros(3)),   # half a turn about x
}
IDENTITY = (np.eye(3), np.zeros(3))


def to_local(R, t, Q):
    """World points into the obstacle frame, in the device's operation order."""
    d = Q - t
    return np.stack([(R[0, i] * d[:, 0] + R[1, i] * d[:, 1]) + R[2, i] * d[:, 2] for i in range(3)], axis=1)


def to_world(R, t, C):
    """Obstacle-frame points into the world, in the device's operation order."""
    return np.stack([((R[i, 0] * C[:, 0] + R[i, 1] * C[:, 1]) + R[i, 2] * C[:, 2]) + t[i] for i in range(3)], axis=1)


def world_vertices(R, t, V):
    return V @ R.T + t


def local_oracle(V, F, R, t, Q_w):
    """The oracle of a posed mesh on world candidates Q_w as collision_prox_rule reads it: asked in
    the mesh's frame, its closest points mapped back to the world."""
    o = mc.Oracle(V, F, to_local(R, t, Q_w))
    return types.SimpleNamespace(dist=o.dist, c=to_world(R, t, o.c), inside=o.inside, keep=o.keep)


@functools.lru_cache(maxsize=None)
def case(name, pose):
    """(V, F, R, t, Q_w, q_l, O_l, O_w) of a mesh under a pose; computed once per session and
    shared (do not modify)."""
    V, F = mc.MESHES[name]()
    R, t = POSES[pose]
    Q_w = mc.queries(V, F) @ R.T + t
    q_l = to_local(R, t, Q_w)
    return V, F, R, t, Q_w, q_l, mc.Oracle(V, F, q_l), mc.Oracle(world_vertices(R, t, V), F, Q_w)


CASES = [(m, p) for m in mc.MESHES for p in POSES]
