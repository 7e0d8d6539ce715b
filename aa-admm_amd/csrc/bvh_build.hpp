// Host builder of the triangle-surface BVH (bvh.hpp). Used by GeomSolver::add_ref_surface and by
// the mesh obstacles of the collision terms (mesh_obstacle.hpp). Host only, no HIP.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bvh.hpp"
#include "error.hpp"

namespace aa {

// median-split BVH, leaves of <= 4 triangles, depth-first node order
struct BvhBuilder {
    const double* V;
    const int* F;
    std::vector<int> ids;
    std::vector<double> cen;
    std::vector<BvhNode>* nodes;
    std::vector<BvhTri>* tris;
    int leaf = 4;            // triangles per leaf (AA_CP_LEAF, 1..7)
    bool split_t1 = false;   // split along the principal tangent axis (AA_CP_SPLIT=t1)
    static float down(double v) {   // largest float <= v
        float f = (float)v;
        if ((double)f > v) f = std::nextafter(f, -INFINITY);
        return f;
    }
    static float up(double v) {     // smallest float >= v
        float f = (float)v;
        if ((double)f < v) f = std::nextafter(f, INFINITY);
        return f;
    }
    int build(int b, int e) {
        BvhNode nd{};
        double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        double clo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, chi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        for (int i = b; i < e; ++i) {
            const int t = ids[i];
            for (int a = 0; a < 3; ++a)
                for (int d = 0; d < 3; ++d) {
                    const double v = V[3 * (size_t)F[3 * (size_t)t + a] + d];
                    lo[d] = std::min(lo[d], v); hi[d] = std::max(hi[d], v);
                }
            for (int d = 0; d < 3; ++d) { clo[d] = std::min(clo[d], cen[3 * (size_t)t + d]); chi[d] = std::max(chi[d], cen[3 * (size_t)t + d]); }
        }
        for (int d = 0; d < 3; ++d) { nd.lo[d] = down(lo[d]); nd.hi[d] = up(hi[d]); }
        {   // slab: area-weighted mean normal of the subtree, range of n . v over its vertices
            double N[3] = {0, 0, 0};
            for (int i = b; i < e; ++i) {
                const double* A = V + 3 * (size_t)F[3 * (size_t)ids[i]];
                const double* Bv = V + 3 * (size_t)F[3 * (size_t)ids[i] + 1];
                const double* C = V + 3 * (size_t)F[3 * (size_t)ids[i] + 2];
                const double u[3] = {Bv[0] - A[0], Bv[1] - A[1], Bv[2] - A[2]}, w[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
                N[0] += u[1] * w[2] - u[2] * w[1]; N[1] += u[2] * w[0] - u[0] * w[2]; N[2] += u[0] * w[1] - u[1] * w[0];
            }
            const double l = std::sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
            for (int d = 0; d < 3; ++d) nd.nrm[d] = l > 0 ? (float)(N[d] / l) : 0.0f;
            double dl = DBL_MAX, dh = -DBL_MAX;
            for (int i = b; i < e; ++i)
                for (int a = 0; a < 3; ++a) {
                    const double* P = V + 3 * (size_t)F[3 * (size_t)ids[i] + a];
                    const double dd = (double)nd.nrm[0] * P[0] + (double)nd.nrm[1] * P[1] + (double)nd.nrm[2] * P[2];
                    dl = std::min(dl, dd); dh = std::max(dh, dd);
                }
            if (l > 0) { nd.dlo = down(dl); nd.dhi = up(dh); }
            else { nd.dlo = -FLT_MAX; nd.dhi = FLT_MAX; }   // degenerate patch: no slab bound
            // tangent axes: the principal directions of the vertices projected on the plane
            // normal to the (fp32) n, then their ranges (AA_CP_OBB=0: unbounded, slab only)
            for (int d = 0; d < 3; ++d) { nd.t1[d] = nd.t2[d] = 0.0f; }
            nd.t1lo = nd.t2lo = -FLT_MAX; nd.t1hi = nd.t2hi = FLT_MAX;
            static const bool obb = !(std::getenv("AA_CP_OBB") && std::getenv("AA_CP_OBB")[0] == '0');
            if (l > 0 && obb) {
                const double n[3] = {nd.nrm[0], nd.nrm[1], nd.nrm[2]};
                const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                const double nn[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
                // any unit e1 normal to n, e2 = n x e1
                const int k = std::fabs(nn[0]) < 0.6 ? 0 : (std::fabs(nn[1]) < 0.6 ? 1 : 2);
                double e1[3] = {0, 0, 0};
                e1[k] = 1.0;
                const double pr = e1[0] * nn[0] + e1[1] * nn[1] + e1[2] * nn[2];
                for (int d = 0; d < 3; ++d) e1[d] -= pr * nn[d];
                const double el = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
                for (int d = 0; d < 3; ++d) e1[d] /= el;
                const double e2[3] = {nn[1] * e1[2] - nn[2] * e1[1], nn[2] * e1[0] - nn[0] * e1[2], nn[0] * e1[1] - nn[1] * e1[0]};
                double m1 = 0, m2 = 0, c11 = 0, c22 = 0, c12 = 0, cnt = 0;
                for (int i = b; i < e; ++i)
                    for (int a = 0; a < 3; ++a) {
                        const double* P = V + 3 * (size_t)F[3 * (size_t)ids[i] + a];
                        const double x1 = e1[0] * P[0] + e1[1] * P[1] + e1[2] * P[2], x2 = e2[0] * P[0] + e2[1] * P[1] + e2[2] * P[2];
                        m1 += x1; m2 += x2; c11 += x1 * x1; c22 += x2 * x2; c12 += x1 * x2; cnt += 1;
                    }
                m1 /= cnt; m2 /= cnt;
                c11 = c11 / cnt - m1 * m1; c22 = c22 / cnt - m2 * m2; c12 = c12 / cnt - m1 * m2;
                const double th = 0.5 * std::atan2(2.0 * c12, c11 - c22);
                const double a1[3] = {std::cos(th) * e1[0] + std::sin(th) * e2[0], std::cos(th) * e1[1] + std::sin(th) * e2[1],
                                      std::cos(th) * e1[2] + std::sin(th) * e2[2]};
                const double a2[3] = {nn[1] * a1[2] - nn[2] * a1[1], nn[2] * a1[0] - nn[0] * a1[2], nn[0] * a1[1] - nn[1] * a1[0]};
                for (int d = 0; d < 3; ++d) { nd.t1[d] = (float)a1[d]; nd.t2[d] = (float)a2[d]; }
                double l1 = DBL_MAX, h1 = -DBL_MAX, l2 = DBL_MAX, h2 = -DBL_MAX;
                for (int i = b; i < e; ++i)
                    for (int a = 0; a < 3; ++a) {
                        const double* P = V + 3 * (size_t)F[3 * (size_t)ids[i] + a];
                        const double x1 = (double)nd.t1[0] * P[0] + (double)nd.t1[1] * P[1] + (double)nd.t1[2] * P[2];
                        const double x2 = (double)nd.t2[0] * P[0] + (double)nd.t2[1] * P[1] + (double)nd.t2[2] * P[2];
                        l1 = std::min(l1, x1); h1 = std::max(h1, x1); l2 = std::min(l2, x2); h2 = std::max(h2, x2);
                    }
                nd.t1lo = down(l1); nd.t1hi = up(h1); nd.t2lo = down(l2); nd.t2hi = up(h2);
            }
        }
        const int me = (int)nodes->size();
        if (me >= (1 << 29)) throw Error(ERR_ARG, "add_ref_surface: too many BVH nodes");
        nodes->push_back(nd);
        if (e - b <= leaf) {
            (*nodes)[me].a = (int)tris->size();
            (*nodes)[me].sn = (unsigned)(me + 1) | ((unsigned)(e - b) << 29);
            for (int i = b; i < e; ++i) {
                BvhTri tr;
                for (int a = 0; a < 3; ++a)
                    for (int d = 0; d < 3; ++d) tr.v[3 * a + d] = V[3 * (size_t)F[3 * (size_t)ids[i] + a] + d];
                tris->push_back(tr);
            }
            return me;
        }
        const int mid = (b + e) / 2;
        if (split_t1 && (nd.t1hi - nd.t1lo) < FLT_MAX) {   // median along the principal tangent axis
            const double a1[3] = {nd.t1[0], nd.t1[1], nd.t1[2]};
            auto key = [&](int p) { return a1[0] * cen[3 * (size_t)p] + a1[1] * cen[3 * (size_t)p + 1] + a1[2] * cen[3 * (size_t)p + 2]; };
            std::nth_element(ids.begin() + b, ids.begin() + mid, ids.begin() + e, [&](int p, int q) { return key(p) < key(q); });
        } else {   // median along the longest axis of the centroids' box
            int ax = 0;
            for (int d = 1; d < 3; ++d) if (chi[d] - clo[d] > chi[ax] - clo[ax]) ax = d;
            std::nth_element(ids.begin() + b, ids.begin() + mid, ids.begin() + e,
                             [&](int p, int q) { return cen[3 * (size_t)p + ax] < cen[3 * (size_t)q + ax]; });
        }
        build(b, mid);
        const int r = build(mid, e);
        (*nodes)[me].a = r;
        (*nodes)[me].sn = (unsigned)nodes->size();
        return me;
    }
};

}  // namespace aa
