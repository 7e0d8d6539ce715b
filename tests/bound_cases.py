"""Shared pieces of the bound mesh-obstacle tests (tests/test_bound_obstacle.py on the CPU,
tests/test_gpu_bound_obstacle.py on the GPU): the embedding of a mesh's vertices in a node array and
the numpy restatement of the check's chunked signed-volume sum (csrc/mesh_obstacle.hpp,
check_bound_refit)."""
import numpy as np

CHUNK = 256   # kBoundChunk
N_DECOYS = 37


def embed(W, seed=5, decoy_nan=False):
    """(X, nodes): a node array X (len(W) + N_DECOYS, 3) holding the rows of W at the positions
    nodes -- a non-trivial permutation -- between decoy nodes the mesh does not name (NaN on request:
    a decoy must not trip the check). X[nodes] == W bit for bit."""
    rng = np.random.default_rng(seed)
    n = len(W) + N_DECOYS
    nodes = rng.permutation(n)[:len(W)].astype(np.int32)
    assert not np.array_equal(nodes, np.sort(nodes)) or len(W) < 2
    X = rng.uniform(-3.0, 3.0, (n, 3))
    if decoy_nan:
        decoy = np.setdiff1d(np.arange(n), nodes)
        X[decoy[::3]] = np.nan
    X[nodes] = W
    return X, nodes


def vol6_terms(V, F):
    """A . (B x C) per triangle with the operation order of mesh_detail::cross3 / dot3 (no FMA:
    numpy multiplies and adds separately)."""
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n0 = B[:, 1] * C[:, 2] - B[:, 2] * C[:, 1]
    n1 = B[:, 2] * C[:, 0] - B[:, 0] * C[:, 2]
    n2 = B[:, 0] * C[:, 1] - B[:, 1] * C[:, 0]
    return A[:, 0] * n0 + A[:, 1] * n1 + A[:, 2] * n2


def vol6_chunked(V, F):
    """The stated sum: chunks of 256 consecutive triangles (the last padded with 0.0), each reduced
    by the pairwise tree p[i] += p[i + w], w = 128 .. 1, the partials added in chunk order onto 0.0."""
    t = vol6_terms(np.asarray(V, np.float64), np.asarray(F))
    nc = (len(t) + CHUNK - 1) // CHUNK
    p = np.zeros(nc * CHUNK)
    p[:len(t)] = t
    p = p.reshape(nc, CHUNK)
    w = CHUNK // 2
    while w:
        p = p[:, :w] + p[:, w:2 * w]
        w //= 2
    total = np.float64(0.0)
    for c in range(nc):
        total = total + p[c, 0]
    return float(total)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)
