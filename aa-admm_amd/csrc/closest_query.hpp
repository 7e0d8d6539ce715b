// aa_closest_on_triangles: where on a triangle list does a point land. The host side (no HIP in
// prepare_closest_surface: a plain compiler builds it) validates the list and builds the BVH with
// the shared builder (bvh_build.hpp); the kernel (closest_kernels.hip) walks it, one lane per query.
// Unlike a mesh obstacle (mesh_obstacle.hpp) the list may be open or non-manifold: nothing is asked
// of it beyond finite vertices, indices in range and triangles of non-zero area, no pseudonormals
// are computed and no solver is involved.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "bvh_build.hpp"
#include "error.hpp"

namespace aa {

struct ClosestSurfaceHost {
    std::vector<BvhNode> nodes;
    std::vector<BvhTri> tris;   // leaf order
    std::vector<int> orig;      // leaf order -> the caller's triangle index
};

// Throws Error(ERR_ARG) naming the first offending vertex or triangle.
inline ClosestSurfaceHost prepare_closest_surface(const double* V, int nv, const int* F, int nf) {
    const std::string who = "closest_on_triangles: ";
    if (!V || !F || nv <= 0 || nf <= 0) throw Error(ERR_ARG, who + "empty triangle list");
    for (int t = 0; t < nf; ++t)
        for (int a = 0; a < 3; ++a)
            if (F[3 * (size_t)t + a] < 0 || F[3 * (size_t)t + a] >= nv)
                throw Error(ERR_ARG, who + "triangle " + std::to_string(t) + " has a vertex index out of range");
    for (int i = 0; i < nv; ++i)
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(V[3 * (size_t)i + d]))
                throw Error(ERR_ARG, who + "vertex " + std::to_string(i) + " has a non-finite coordinate");
    for (int t = 0; t < nf; ++t) {   // the mesh obstacles' zero-area test
        const double *A = V + 3 * (size_t)F[3 * (size_t)t], *B = V + 3 * (size_t)F[3 * (size_t)t + 1],
                     *C = V + 3 * (size_t)F[3 * (size_t)t + 2];
        const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, w[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
        const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        if (!(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 0.0))
            throw Error(ERR_ARG, who + "triangle " + std::to_string(t) + " has zero area");
    }
    ClosestSurfaceHost M;
    BvhBuilder B;
    B.V = V; B.F = F;
    B.ids.resize(nf);
    std::iota(B.ids.begin(), B.ids.end(), 0);
    B.cen.resize(3 * (size_t)nf);
    for (int t = 0; t < nf; ++t)
        for (int d = 0; d < 3; ++d)
            B.cen[3 * (size_t)t + d] = (V[3 * (size_t)F[3 * t] + d] + V[3 * (size_t)F[3 * t + 1] + d] + V[3 * (size_t)F[3 * t + 2] + d]) / 3.0;
    B.nodes = &M.nodes;
    B.tris = &M.tris;
    M.nodes.reserve(nf);
    M.tris.reserve(nf);
    B.build(0, nf);
    M.orig = B.ids;   // leaves are emitted left to right over ids[b, e): ids is the leaf order
    return M;
}
inline void validate_closest_queries(const double* q3, int n) {
    for (int i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(q3[3 * (size_t)i + d]))
                throw Error(ERR_ARG, "closest_on_triangles: query " + std::to_string(i) + " has a non-finite coordinate");
}

#if defined(__HIPCC__)
// per query i: closest[3 i ..] the closest point, tri[i] = orig[leaf triangle], bary[3 i ..] its
// dev::tri_barycentric on that triangle; any of the three outputs may be null
void launch_closest_on_triangles(const SurfDev& S, const int* orig, const double* q, int n, double* closest, int* tri,
                                 double* bary, hipStream_t s);
#endif

}  // namespace aa
