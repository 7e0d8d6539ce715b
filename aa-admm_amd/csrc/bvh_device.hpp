// Device side of the triangle-surface BVH (bvh.hpp): Ericson's closest point on a triangle, the
// box lower bounds and the exact stackless closest-point walk. Shared by the Geometry kernels
// (geom_kernels.hip) and the mesh obstacles of the collision prox (device_prox.hpp); each
// translation unit gets its own copy (unnamed namespace), as when the code lived in
// geom_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh.hpp"

namespace aa {

namespace {

// Ericson closest point on a triangle (igl point_simplex_squared_distance.cpp:40-108). Every
// product-sum is an explicit fma and contraction is off, so the bits do not depend on how the
// compiler fuses the inlined code at each call site (the one-lane and the group traversal must
// agree bit for bit).
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    return fma(ax, bx, fma(ay, by, az * bz));
}
__device__ __forceinline__ double dist2(double px, double py, double pz, double qx, double qy, double qz) {
#pragma clang fp contract(off)
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    return fma(dx, dx, fma(dy, dy, dz * dz));
}
// A trailing `int&` receives the feature the closest point lies on, read from the branch taken:
// TRI_A / TRI_B / TRI_C a corner, TRI_AB / TRI_CA / TRI_BC an edge, TRI_FACE the interior (the
// mesh obstacles' pseudonormal lookup). Without it -- every Geometry call site -- nothing is
// added to the code.
enum TriRegion { TRI_A = 0, TRI_B = 1, TRI_AB = 2, TRI_C = 3, TRI_CA = 4, TRI_BC = 5, TRI_FACE = 6 };
template <class... R>
__device__ __forceinline__ void closest_on_tri(const double* t, double px, double py, double pz, double& cx,
                                               double& cy, double& cz, R&... region) {
#pragma clang fp contract(off)
    [[maybe_unused]] auto at = [&](int r) { if constexpr (sizeof...(R) != 0) ((region = r), ...); };
    const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], qx = t[6], qy = t[7], qz = t[8];
    const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = qx - ax, acy = qy - ay, acz = qz - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.0 && d2 <= 0.0) { cx = ax; cy = ay; cz = az; at(TRI_A); return; }
    const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0 && d4 <= d3) { cx = bx; cy = by; cz = bz; at(TRI_B); return; }
    const double vc = fma(d1, d4, -(d3 * d2));
    if (!(ax == bx && ay == by && az == bz) && vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        cx = fma(v, abx, ax); cy = fma(v, aby, ay); cz = fma(v, abz, az); at(TRI_AB); return;
    }
    const double cpx = px - qx, cpy = py - qy, cpz = pz - qz;
    const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0 && d5 <= d6) { cx = qx; cy = qy; cz = qz; at(TRI_C); return; }
    const double vb = fma(d5, d2, -(d1 * d6));
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
        cx = fma(w, acx, ax); cy = fma(w, acy, ay); cz = fma(w, acz, az); at(TRI_CA); return;
    }
    const double va = fma(d3, d6, -(d5 * d4));
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        cx = fma(w, qx - bx, bx); cy = fma(w, qy - by, by); cz = fma(w, qz - bz, bz); at(TRI_BC); return;
    }
    const double denom = 1.0 / (va + vb + vc);
    const double v = vb * denom, w = vc * denom;
    cx = fma(acx, w, fma(abx, v, ax)); cy = fma(acy, w, fma(aby, v, ay)); cz = fma(acz, w, fma(abz, v, az));
    at(TRI_FACE);
}

// Branch-free: max(lo - v, v - hi, 0) is the distance outside [lo, hi] bit for bit (one of the two
// differences is positive at most, and it is the one the comparisons would pick). The ternary
// form compiled to branches with each field's load sunk into its branch -- a load and a wait per
// field, serialised -- which made the greedy descent (a third of C5's queries) a long chain.
__device__ __forceinline__ double box_d2(const BvhNode& nd, double px, double py, double pz) {
    const double l0 = nd.lo[0], l1 = nd.lo[1], l2 = nd.lo[2], h0 = nd.hi[0], h1 = nd.hi[1], h2 = nd.hi[2];
    const double tx = fmax(fmax(l0 - px, px - h0), 0.0);
    const double ty = fmax(fmax(l1 - py, py - h1), 0.0);
    const double tz = fmax(fmax(l2 - pz, pz - h2), 0.0);
#ifdef AA_CP_NO_AABB
    const double b = 0.0 * (tx + ty + tz);
#else
    const double b = tx * tx + ty * ty + tz * tz;
#endif
    // oriented-box lower bound: the distances of (n.p, t1.p, t2.p) outside the node's ranges
    // (the axes are orthonormal to fp32 accuracy: shrunk by 4e-6 to stay below)
    auto outside = [](double v, float lo, float hi) { return fmax(fmax((double)lo - v, v - (double)hi), 0.0); };
    const double t = outside((double)nd.nrm[0] * px + (double)nd.nrm[1] * py + (double)nd.nrm[2] * pz, nd.dlo, nd.dhi);
    const double u1 = outside((double)nd.t1[0] * px + (double)nd.t1[1] * py + (double)nd.t1[2] * pz, nd.t1lo, nd.t1hi);
    const double u2 = outside((double)nd.t2[0] * px + (double)nd.t2[1] * py + (double)nd.t2[2] * pz, nd.t2lo, nd.t2hi);
    const double sl = (t * t + u1 * u1 + u2 * u2) * (1.0 - 4e-6);
    return b > sl ? b : sl;
}

// The same lower bound in fp32 arithmetic for the traversal's prune tests (AA_CP_F32=1, the
// default): the query is rounded to fp32 once, and every per-axis distance is shrunk by
// eps = 8 u (|qx| + |qy| + |qz|) (u = 2^-24), which covers the rounding of the query and of the
// fp32 dot products (|n_i| <= 1), so the bound stays below the true distance -- it only prunes
// less. No conversions per node, half the registers per operand. The greedy descent keeps the
// fp64 bound: its left / right choice picks the seed triangle, which decides ties. Single-lane
// traversal only (C5 z 1 366 -> 1 195 us); the group traversal measured slower with it (C3).
#ifndef AA_CP_F32
#define AA_CP_F32 1
#endif
struct QueryF { float x, y, z, eps; };
__device__ __forceinline__ QueryF query_f(double px, double py, double pz) {
    QueryF q;
    q.x = (float)px; q.y = (float)py; q.z = (float)pz;
    q.eps = 8.0f * 5.9604645e-8f * 1.0001f * (fabsf(q.x) + fabsf(q.y) + fabsf(q.z));
    return q;
}
__device__ __forceinline__ double box_d2f(const BvhNode& nd, const QueryF& q) {
    auto outside = [&](float v, float lo, float hi) { return fmaxf(fmaxf(fmaxf(lo - v, v - hi), 0.0f) - q.eps, 0.0f); };
    const float tx = outside(q.x, nd.lo[0], nd.hi[0]), ty = outside(q.y, nd.lo[1], nd.hi[1]),
                tz = outside(q.z, nd.lo[2], nd.hi[2]);
    const float t = outside(nd.nrm[0] * q.x + nd.nrm[1] * q.y + nd.nrm[2] * q.z, nd.dlo, nd.dhi);
    const float u1 = outside(nd.t1[0] * q.x + nd.t1[1] * q.y + nd.t1[2] * q.z, nd.t1lo, nd.t1hi);
    const float u2 = outside(nd.t2[0] * q.x + nd.t2[1] * q.y + nd.t2[2] * q.z, nd.t2lo, nd.t2hi);
    const float b = tx * tx + ty * ty + tz * tz, sl = t * t + u1 * u1 + u2 * u2;
    return (double)fmaxf(b, sl) * (1.0 - 4e-6);   // fp32 squares and sums: a few ulp
}
#if AA_CP_F32
#define CP_PRUNE_BOUND(nd) box_d2f((nd), Q)
#else
#define CP_PRUNE_BOUND(nd) box_d2((nd), px, py, pz)
#endif

// (warm distance / warm triangle's first edge)^2 up to which the warm bound is used alone: the
// greedy root-to-leaf descent (a chain of dependent node loads) only runs for points that slid
// farther than ~8 edges from their previous triangle (and on cold starts). Measured (round 2):
// always descending C3 995 / C5 157 it/s, never 1 056 / 154, 64 -> 1 056 / 158; 4 and 16 in between.
#ifndef AA_WARM_TIGHT
#define AA_WARM_TIGHT 64.0
#endif
// share of a wave's live lanes that must hold a leaf before the wave tests leaf triangles
// (0 = one loop: test as soon as any lane reaches a leaf); see bvh_closest
#ifndef AA_BVH_HOLD_PCT
#define AA_BVH_HOLD_PCT 50
#endif

#ifdef AA_CP_STATS
// diagnostics build only (-DAA_CP_STATS): per-query traversal counts of bvh_closest
__device__ unsigned long long g_cp_stats[64];
#define CP_STAT(i, v) atomicAdd(&g_cp_stats[(i)], (unsigned long long)(v))
#endif
// exact closest point on the surface. Stackless depth-first traversal over escape links
// (`skip` = the node after a subtree): no per-lane stack, so no scratch memory. The upper
// bound comes from `warm` (the previous iteration's triangle: points move little between ALM
// iterations) or, on a cold start, from a greedy descent to the nearest-box leaf; boxes that
// cannot beat it are skipped whole. Strictly smaller distances replace the best, so the result
// is the exact minimum (ties resolved toward the warm / first-found triangle).
__device__ int bvh_closest(const SurfDev& S, double px, double py, double pz, int warm, double& cx, double& cy,
                           double& cz) {
    double best = INFINITY;
    int best_t = -1;
    cx = px; cy = py; cz = pz;
    if (S.n_nodes == 0) return -1;
#ifdef AA_CP_STATS
    unsigned nbox = 0, ntri = 0;
    double e2s = 0;
#define CP_BOX() (++nbox)
#define CP_TRI() (++ntri)
#else
#define CP_BOX() ((void)0)
#define CP_TRI() ((void)0)
#endif
    auto test_tri = [&](int t) {
        CP_TRI();
        double qx, qy, qz;
        closest_on_tri(S.tris[t].v, px, py, pz, qx, qy, qz);
        const double d2 = dist2(px, py, pz, qx, qy, qz);
        if (d2 < best) { best = d2; best_t = t; cx = qx; cy = qy; cz = qz; }
    };
    bool tight = false;
    if (warm >= 0 && warm < S.n_tris) {
        test_tri(warm);
        const double* v = S.tris[warm].v;
        const double e2 = (v[3] - v[0]) * (v[3] - v[0]) + (v[4] - v[1]) * (v[4] - v[1]) + (v[5] - v[2]) * (v[5] - v[2]);
        tight = best <= AA_WARM_TIGHT * e2;
#ifdef AA_CP_STATS
        e2s = e2;
#endif
    }
    if (!tight)
    {   // greedy descent to the nearest-box leaf: a tight bound even when the point slid far
        // from its previous triangle (the warm bound alone then lets the traversal open every
        // box within that distance)
        // the chosen child's record comes with the pair just loaded: one dependent load per level
        int i = 0;
        BvhNode nd = S.nodes[0];
        for (;;) {
            if (bvh_count(nd) > 0) {
                for (int t = nd.a; t < nd.a + bvh_count(nd); ++t) test_tri(t);
                break;
            }
            const BvhNode cl = S.nodes[i + 1], cr = S.nodes[nd.a];   // both children's loads issued together
            const double dl = box_d2(cl, px, py, pz), dr = box_d2(cr, px, py, pz);
            CP_BOX(); CP_BOX();
            if (dl <= dr) { i = i + 1; nd = cl; } else { i = nd.a; nd = cr; }
        }
    }
    const int seed = best_t;
    [[maybe_unused]] const QueryF Q = query_f(px, py, pz);
    int i = 0;
#if AA_BVH_HOLD_PCT > 0
    // Two-phase ("while-while") schedule of the same per-lane traversal: a lane that reaches a
    // leaf whose box passes parks on it while the other lanes keep walking inner nodes; the
    // wave tests leaf triangles only once at least AA_BVH_HOLD_PCT % of its live lanes hold a
    // leaf (or none walks any more). Each lane visits the same nodes and tests the same
    // triangles in the same order as the one-loop form below -- only the interleaving across
    // the wave changes -- so the result is bit-identical. What changes is the SIMD use of the
    // triangle tests: in one loop, every step where any lane sits on a leaf runs the whole
    // (divergent) triangle body for the wave.
    int hold_a = -1, hold_n = 0;
    bool done = S.n_nodes <= 0;
    for (;;) {
        for (;;) {
            if (!done && hold_a < 0) {
                const BvhNode nd = S.nodes[i];
                CP_BOX();
                if (CP_PRUNE_BOUND(nd) < best) {
                    const int nc = bvh_count(nd);
                    if (nc > 0) { hold_a = nd.a; hold_n = nc; i = bvh_skip(nd); }
                    else i = i + 1;
                } else {
                    i = bvh_skip(nd);
                }
                if (hold_a < 0 && i >= S.n_nodes) done = true;
            }
            const unsigned long long live = __ballot(!done), held = __ballot(hold_a >= 0);
            const int nl = __popcll(live), nh = __popcll(held);
            if (nh == nl || (nh > 0 && 100 * nh >= AA_BVH_HOLD_PCT * nl)) break;
        }
        if (__ballot(!done) == 0ull) break;
        if (hold_a >= 0) {
            for (int t = hold_a; t < hold_a + hold_n; ++t)
                if (t != seed) test_tri(t);
            hold_a = -1;
            if (i >= S.n_nodes) done = true;
        }
    }
#else
    while (i < S.n_nodes) {
        const BvhNode nd = S.nodes[i];
        CP_BOX();
        if (CP_PRUNE_BOUND(nd) < best) {
            const int nc = bvh_count(nd);
            if (nc > 0) {
                for (int t = nd.a; t < nd.a + nc; ++t)
                    if (t != seed) test_tri(t);
                i = bvh_skip(nd);
            } else {
                i = i + 1;
            }
        } else {
            i = bvh_skip(nd);
        }
    }
#endif
#ifdef AA_CP_STATS
    {
        auto lg = [](double v) { int b = 0; while (v >= 2.0 && b < 15) { v *= 0.5; ++b; } return b; };
        CP_STAT(0, 1); CP_STAT(1, nbox); CP_STAT(2, ntri); CP_STAT(3, tight ? 1 : 0); CP_STAT(4, best_t != warm ? 1 : 0);
        CP_STAT(8 + lg((double)nbox), 1);
        // distance / warm edge length, log2 buckets from 2^-12
        if (e2s > 0) { double r = sqrt(best / e2s) * 4096.0; CP_STAT(24 + lg(r), 1); }
        // oracle: the same walk started with the final distance as the bound (what a perfect
        // seed would leave to test)
        unsigned ob = 0, ot = 0;
        for (int k = 0; k < S.n_nodes;) {
            const BvhNode nd = S.nodes[k];
            ++ob;
            if (CP_PRUNE_BOUND(nd) < best) {
                const int nc = bvh_count(nd);
                if (nc > 0) { ot += nc; k = bvh_skip(nd); } else k = k + 1;
            } else {
                k = bvh_skip(nd);
            }
        }
        CP_STAT(40, ob); CP_STAT(41, ot);
    }
#endif
#undef CP_BOX
#undef CP_TRI
    return best_t;
}

}  // namespace

}  // namespace aa
