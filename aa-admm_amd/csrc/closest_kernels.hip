// The public closest-point query (aa_closest_on_triangles, closest_query.hpp) on the device
// (gfx950): one lane per query runs the exact stackless walk of bvh_device.hpp from a cold start
// (no warm triangle: the greedy descent seeds the bound), so the point is the exact minimum over
// the list and ties between triangles go to the walk's first found. The barycentric weights are
// dev::tri_barycentric of that point on the leaf triangle, whose corners are stored in the
// caller's order. A translation unit of its own: the walk's other call sites keep their code.
// Stated operation by operation for a host restatement, so nothing may be contracted into an FMA:
#pragma clang fp contract(off)
#include "closest_query.hpp"

#include "common.hpp"
#include "device_prox.hpp"

namespace aa {
namespace {

__global__ __launch_bounds__(kBlock) void k_closest_on_triangles(SurfDev S, const int* __restrict__ orig,
                                                                 const double* __restrict__ q, int n,
                                                                 double* __restrict__ closest, int* __restrict__ tri,
                                                                 double* __restrict__ bary) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;   // (an exited lane reads 0 in the walk's ballots: neither waited for nor counted)
    const double px = q[3 * (size_t)i], py = q[3 * (size_t)i + 1], pz = q[3 * (size_t)i + 2];
    double c[3];
    const int t = bvh_closest(S, px, py, pz, -1, c[0], c[1], c[2]);
    double b[3] = {0.0, 0.0, 0.0};
    if (t >= 0 && t < S.n_tris) dev::tri_barycentric(S.tris[t].v, c, b);
    if (closest) { closest[3 * (size_t)i] = c[0]; closest[3 * (size_t)i + 1] = c[1]; closest[3 * (size_t)i + 2] = c[2]; }
    if (tri) tri[i] = (t >= 0 && t < S.n_tris) ? orig[t] : -1;
    if (bary) { bary[3 * (size_t)i] = b[0]; bary[3 * (size_t)i + 1] = b[1]; bary[3 * (size_t)i + 2] = b[2]; }
}

}  // namespace

void launch_closest_on_triangles(const SurfDev& S, const int* orig, const double* q, int n, double* closest, int* tri,
                                 double* bary, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_closest_on_triangles, dim3(blocks_for(n)), dim3(kBlock), 0, s, S, orig, q, n, closest, tri, bary);
    AA_CHECK_LAUNCH();
}

}  // namespace aa
