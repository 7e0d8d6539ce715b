// Host preparation of a triangle-mesh passive obstacle of the collision terms (the reference's
// PassiveMesh, admm_anderson_hard_zxu/src/PassiveObject.hpp:138-178: a collision node inside the
// mesh moves to the nearest surface point). Host only, no HIP.
//
// The obstacle is a closed, edge-manifold, outward-oriented triangle surface. A query q is
// answered in fp64 by the project's exact closest-point walk (bvh_device.hpp bvh_closest) and
// signed by the angle-weighted pseudonormal n of the feature the closest point c lies on
// (Baerentzen & Aanaes, "Signed distance computation using the angle weighted pseudonormal",
// IEEE TVCG 11(3), 2005): inside iff (q - c) . n < 0. The sign is right for every q only on a
// closed manifold surface, hence the validation; n need not be of unit length.
//   face   -- the unit face normal;
//   edge   -- the sum of the two incident unit face normals;
//   vertex -- the sum over incident faces of (incident angle x unit face normal).
#pragma once
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <map>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "bvh.hpp"
#include "bvh_build.hpp"
#include "error.hpp"

namespace aa {

constexpr int kMaxMeshObstacles = 16;   // rows of a solver's mesh table (aa_admm.h)

struct MeshObstacleHost {
    std::vector<BvhNode> nodes;
    std::vector<BvhTri> tris;     // leaf order
    std::vector<double> pn;       // [tris][kPnStride], leaf order; feature k at 3 k (TriRegion order:
                                  // corner a, corner b, edge ab, corner c, edge ca, edge bc, face)
    std::vector<int> orig;        // leaf order -> the caller's triangle index
    double lo[3], hi[3];          // exact range of the surface's vertices
};

namespace mesh_detail {
AA_HD inline void sub3(const double* a, const double* b, double* r) { r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; }
AA_HD inline void cross3(const double* u, const double* w, double* r) {
    r[0] = u[1] * w[2] - u[2] * w[1]; r[1] = u[2] * w[0] - u[0] * w[2]; r[2] = u[0] * w[1] - u[1] * w[0];
}
AA_HD inline double dot3(const double* u, const double* w) { return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]; }
}  // namespace mesh_detail

// Throws Error(ERR_ARG) naming the first offending vertex, triangle or edge.
inline void validate_mesh_obstacle(const double* V, int nv, const int* F, int nf) {
    using namespace mesh_detail;
    const std::string who = "add_mesh_obstacle: ";
    if (!V || !F || nv <= 0 || nf <= 0) throw Error(ERR_ARG, who + "empty mesh");
    for (int t = 0; t < nf; ++t)
        for (int a = 0; a < 3; ++a)
            if (F[3 * (size_t)t + a] < 0 || F[3 * (size_t)t + a] >= nv)
                throw Error(ERR_ARG, who + "triangle " + std::to_string(t) + " has a vertex index out of range");
    for (int i = 0; i < nv; ++i)
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(V[3 * (size_t)i + d]))
                throw Error(ERR_ARG, who + "vertex " + std::to_string(i) + " has a non-finite coordinate");
    double vol6 = 0;
    for (int t = 0; t < nf; ++t) {
        const double *A = V + 3 * (size_t)F[3 * (size_t)t], *B = V + 3 * (size_t)F[3 * (size_t)t + 1],
                     *C = V + 3 * (size_t)F[3 * (size_t)t + 2];
        double u[3], w[3], n[3];
        sub3(B, A, u); sub3(C, A, w); cross3(u, w, n);
        if (!(dot3(n, n) > 0.0)) throw Error(ERR_ARG, who + "triangle " + std::to_string(t) + " has zero area");
        cross3(B, C, n);
        vol6 += dot3(A, n);
    }
    // closed and edge-manifold with consistent orientation: every directed edge once, and its
    // reverse once
    std::map<std::pair<int, int>, int> dir;
    for (int t = 0; t < nf; ++t)
        for (int a = 0; a < 3; ++a) ++dir[{F[3 * (size_t)t + a], F[3 * (size_t)t + (a + 1) % 3]}];
    for (int t = 0; t < nf; ++t)
        for (int a = 0; a < 3; ++a) {
            const int p = F[3 * (size_t)t + a], q = F[3 * (size_t)t + (a + 1) % 3];
            const int same = dir[{p, q}];
            const auto rev_it = dir.find({q, p});
            const int rev = rev_it == dir.end() ? 0 : rev_it->second;
            if (same == 1 && rev == 1) continue;
            const std::string e = "edge (" + std::to_string(p) + ", " + std::to_string(q) + ") of triangle " + std::to_string(t);
            if (same + rev == 1) throw Error(ERR_ARG, who + e + " lies in one face only: the surface is open");
            if (same + rev == 2) throw Error(ERR_ARG, who + e + " is run in the same direction by both its faces: inconsistent orientation");
            throw Error(ERR_ARG, who + e + " lies in " + std::to_string(same + rev) + " faces: the surface is not edge-manifold");
        }
    if (!(vol6 > 0.0)) throw Error(ERR_ARG, who + "the signed volume is not positive: the faces must be oriented outward");
}

// A kinematic obstacle's rigid pose, pose12 = R (row-major 3x3, obstacle frame -> world) then t.
// R is used as given, so it has to be a rotation already: throws Error(ERR_ARG) naming the cause
// for a non-finite entry, max|R^T R - I| > 1e-12, or det R <= 0 (a reflection would turn the
// surface inside out).
inline void validate_mesh_pose(const double* p, const std::string& who) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(p[i])) throw Error(ERR_ARG, who + "pose entry " + std::to_string(i) + " is not finite");
    double dev = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = p[i] * p[j] + p[3 + i] * p[3 + j] + p[6 + i] * p[6 + j];
            dev = std::max(dev, std::fabs(g - (i == j ? 1.0 : 0.0)));
        }
    if (dev > 1e-12) throw Error(ERR_ARG, who + "R is not orthonormal: max|R^T R - I| = " + std::to_string(dev) + " > 1e-12");
    const double det = p[0] * (p[4] * p[8] - p[5] * p[7]) - p[1] * (p[3] * p[8] - p[5] * p[6]) + p[2] * (p[3] * p[7] - p[4] * p[6]);
    if (!(det > 0.0)) throw Error(ERR_ARG, who + "det R <= 0: a reflection would turn the surface inside out");
}
// The pose (null = unposed) written into a table row
inline void apply_mesh_pose(MeshObsDev& d, const double* pose12) {
    d.posed = pose12 ? 1 : 0;
    for (int i = 0; i < 9; ++i) d.R[i] = pose12 ? pose12[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) d.t[i] = pose12 ? pose12[9 + i] : 0.0;
}

// Validates, builds the BVH with the Geometry side's builder and the pseudonormal table.
inline MeshObstacleHost prepare_mesh_obstacle(const double* V, int nv, const int* F, int nf) {
    using namespace mesh_detail;
    validate_mesh_obstacle(V, nv, F, nf);
    MeshObstacleHost M;
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

    // unit face normals, then the edge and vertex sums
    std::vector<double> fn(3 * (size_t)nf), vn(3 * (size_t)nv, 0.0);
    std::map<std::pair<int, int>, std::array<double, 3>> en;
    for (int t = 0; t < nf; ++t) {
        const int id[3] = {F[3 * (size_t)t], F[3 * (size_t)t + 1], F[3 * (size_t)t + 2]};
        double u[3], w[3], n[3];
        sub3(V + 3 * (size_t)id[1], V + 3 * (size_t)id[0], u);
        sub3(V + 3 * (size_t)id[2], V + 3 * (size_t)id[0], w);
        cross3(u, w, n);
        const double l = std::sqrt(dot3(n, n));
        for (int d = 0; d < 3; ++d) fn[3 * (size_t)t + d] = n[d] / l;
        for (int a = 0; a < 3; ++a) {
            const int p = id[a], q = id[(a + 1) % 3], r = id[(a + 2) % 3];
            double e1[3], e2[3];
            sub3(V + 3 * (size_t)q, V + 3 * (size_t)p, e1);
            sub3(V + 3 * (size_t)r, V + 3 * (size_t)p, e2);
            double c = dot3(e1, e2) / std::sqrt(dot3(e1, e1) * dot3(e2, e2));
            c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
            const double ang = std::acos(c);
            auto& E = en[{std::min(p, q), std::max(p, q)}];   // value-initialised to 0 on first use
            for (int d = 0; d < 3; ++d) {
                vn[3 * (size_t)p + d] += ang * fn[3 * (size_t)t + d];
                E[d] += fn[3 * (size_t)t + d];
            }
        }
    }
    M.pn.resize((size_t)kPnStride * nf);
    for (int k = 0; k < nf; ++k) {
        const int t = M.orig[k];
        const int a = F[3 * (size_t)t], b = F[3 * (size_t)t + 1], c = F[3 * (size_t)t + 2];
        double* P = M.pn.data() + (size_t)kPnStride * k;
        auto edge = [&](int p, int q) { return en[{std::min(p, q), std::max(p, q)}].data(); };
        const double* src[7] = {vn.data() + 3 * (size_t)a, vn.data() + 3 * (size_t)b, edge(a, b), vn.data() + 3 * (size_t)c,
                                edge(c, a), edge(b, c), fn.data() + 3 * (size_t)t};
        for (int f = 0; f < 7; ++f)
            for (int d = 0; d < 3; ++d) P[3 * f + d] = src[f][d];
    }
    for (int d = 0; d < 3; ++d) { M.lo[d] = DBL_MAX; M.hi[d] = -DBL_MAX; }
    for (int t = 0; t < nf; ++t)
        for (int a = 0; a < 3; ++a)
            for (int d = 0; d < 3; ++d) {
                const double v = V[3 * (size_t)F[3 * (size_t)t + a] + d];
                M.lo[d] = std::min(M.lo[d], v); M.hi[d] = std::max(M.hi[d], v);
            }
    return M;
}

// ---------------------------------------------------------------------------------------------
// Deforming obstacles: the refit of a prepared mesh to new vertex positions V' (same vertex count,
// same triangles). The tree keeps its node order, leaf contents and stored axes; what follows from
// the positions is recomputed:
//   tris[k].v    the corners of leaf triangle k read from V';
//   node boxes   lo[d] = down(min P[d]), hi[d] = up(max P[d]) over the 3 count vertices P of the
//                node's contiguous range of leaf triangles (BvhBuilder::down / up);
//   axis ranges  for each stored axis a of nrm, t1, t2 the range of
//                s = ((double)a[0] P[0] + (double)a[1] P[1]) + (double)a[2] P[2] (left to right, no
//                FMA contraction), rounded outward alike; a range the build stored as
//                (-FLT_MAX, FLT_MAX) -- a degenerate patch, AA_CP_OBB=0 -- stays so. The stale axes
//                are still orthonormal, so box_d2 / box_d2f stay lower bounds: the walk is exact,
//                the bounds only loosen as the shape leaves the one the tree was built for;
//   pn           prepare_mesh_obstacle's formulas on V' in a fixed summation order: a vertex's terms
//                in increasing caller triangle index from 0.0, an edge's (0 + fn[t_lo]) + fn[t_hi];
//   lo / hi      the exact fp64 range of the referenced vertices.
// refit_mesh_obstacle_host defines the result; the device kernels (mesh_refit.hip) reproduce it
// bit for bit except for acos (the corner angles of the vertex sums).
struct MeshRefitTables {
    int nv = 0;
    std::vector<int> F;          // the caller's triangles, [nf][3] (validation runs in their order)
    std::vector<int> leaf_vid;   // [nf][3] vertex ids of leaf triangle k, the build's corner order
    std::vector<int> node_beg, node_cnt;   // per node: its contiguous range of leaf triangles
    // per vertex the (leaf triangle, corner) pairs, 4 k + corner, in increasing CALLER triangle index
    std::vector<int> vt_ptr, vt;
    // [nf][3][2], leaf order: the two leaf triangles on edge ab, bc, ca, the lower caller index first
    std::vector<int> edge_tris;
    // node-bound reduction of the large nodes (more than kRefitChunk triangles): the nodes, and
    // their ranges cut into chunks of at most kRefitChunk triangles (big_chunk_ptr: CSR over chunks)
    std::vector<int> big_node, big_chunk_ptr, chunk_big, chunk_beg, chunk_cnt;
};
constexpr int kRefitChunk = 1024;

inline MeshRefitTables make_refit_tables(const MeshObstacleHost& M, int nv, const int* F, int nf) {
    MeshRefitTables T;
    T.nv = nv;
    T.F.assign(F, F + 3 * (size_t)nf);
    std::vector<int> leaf_of(nf);   // caller triangle -> leaf position
    T.leaf_vid.resize(3 * (size_t)nf);
    for (int k = 0; k < nf; ++k) {
        leaf_of[M.orig[k]] = k;
        for (int a = 0; a < 3; ++a) T.leaf_vid[3 * (size_t)k + a] = F[3 * (size_t)M.orig[k] + a];
    }
    const int nn = (int)M.nodes.size();
    T.node_beg.resize(nn); T.node_cnt.resize(nn);
    for (int i = nn - 1; i >= 0; --i) {   // children come after their parent in the depth-first order
        const BvhNode& nd = M.nodes[i];
        if (bvh_count(nd)) { T.node_beg[i] = nd.a; T.node_cnt[i] = bvh_count(nd); }
        else { T.node_beg[i] = T.node_beg[i + 1]; T.node_cnt[i] = T.node_beg[nd.a] + T.node_cnt[nd.a] - T.node_beg[i + 1]; }
    }
    T.vt_ptr.assign((size_t)nv + 1, 0);
    for (size_t i = 0; i < 3 * (size_t)nf; ++i) ++T.vt_ptr[F[i] + 1];
    for (int i = 0; i < nv; ++i) T.vt_ptr[i + 1] += T.vt_ptr[i];
    T.vt.resize(3 * (size_t)nf);
    std::vector<int> fill(T.vt_ptr.begin(), T.vt_ptr.end() - 1);
    std::map<std::pair<int, int>, std::pair<int, int>> et;   // edge -> its two caller triangles, lower first
    for (int t = 0; t < nf; ++t)
        for (int a = 0; a < 3; ++a) {
            const int p = F[3 * (size_t)t + a], q = F[3 * (size_t)t + (a + 1) % 3];
            T.vt[fill[p]++] = 4 * leaf_of[t] + a;
            auto it = et.find({std::min(p, q), std::max(p, q)});
            if (it == et.end()) et[{std::min(p, q), std::max(p, q)}] = {t, -1};
            else it->second.second = t;
        }
    T.edge_tris.resize(6 * (size_t)nf);
    for (int k = 0; k < nf; ++k)
        for (int a = 0; a < 3; ++a) {
            const int p = T.leaf_vid[3 * (size_t)k + a], q = T.leaf_vid[3 * (size_t)k + (a + 1) % 3];
            const auto& e = et[{std::min(p, q), std::max(p, q)}];
            T.edge_tris[6 * (size_t)k + 2 * a] = leaf_of[e.first];
            T.edge_tris[6 * (size_t)k + 2 * a + 1] = leaf_of[e.second];
        }
    T.big_chunk_ptr.push_back(0);
    for (int i = 0; i < nn; ++i) {
        if (T.node_cnt[i] <= kRefitChunk) continue;
        for (int b = 0; b < T.node_cnt[i]; b += kRefitChunk) {
            T.chunk_big.push_back((int)T.big_node.size());
            T.chunk_beg.push_back(T.node_beg[i] + b);
            T.chunk_cnt.push_back(std::min(kRefitChunk, T.node_cnt[i] - b));
        }
        T.big_node.push_back(i);
        T.big_chunk_ptr.push_back((int)T.chunk_big.size());
    }
    return T;
}

// What a refit checks of V' before anything is touched (the topology is not looked at again):
// throws Error(ERR_ARG) naming the cause. lo / hi receive the exact range of the referenced vertices.
inline void validate_mesh_refit(const MeshRefitTables& T, const double* V, const std::string& who, double* lo, double* hi) {
    using namespace mesh_detail;
    if (!V) throw Error(ERR_ARG, who + "null vertex array");
    for (int i = 0; i < T.nv; ++i)
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(V[3 * (size_t)i + d]))
                throw Error(ERR_ARG, who + "vertex " + std::to_string(i) + " has a non-finite coordinate");
    const int nf = (int)T.F.size() / 3;
    double vol6 = 0;
    for (int d = 0; d < 3; ++d) { lo[d] = DBL_MAX; hi[d] = -DBL_MAX; }
    for (int t = 0; t < nf; ++t) {
        const double *A = V + 3 * (size_t)T.F[3 * (size_t)t], *B = V + 3 * (size_t)T.F[3 * (size_t)t + 1],
                     *C = V + 3 * (size_t)T.F[3 * (size_t)t + 2];
        double u[3], w[3], n[3];
        sub3(B, A, u); sub3(C, A, w); cross3(u, w, n);
        if (!(dot3(n, n) > 0.0)) throw Error(ERR_ARG, who + "triangle " + std::to_string(t) + " has zero area");
        cross3(B, C, n);
        vol6 += dot3(A, n);
        for (const double* P : {A, B, C})
            for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], P[d]); hi[d] = std::max(hi[d], P[d]); }
    }
    if (!(vol6 > 0.0)) throw Error(ERR_ARG, who + "the signed volume is not positive: the deformed surface is turned inside out");
}

// Bound obstacles: a mesh whose vertex i follows solver node nodes[i]. The vertices are gathered on
// the device from the step's start state, which the host never sees, so the check that decides
// whether the refit is taken runs there too; check_bound_refit states it and the kernels of
// mesh_refit.hip reproduce it bit for bit. The causes are validate_mesh_refit's, tested in this
// order, the lowest-numbered one reported:
//   BOUND_NONFINITE  a non-finite coordinate among the nv gathered vertices;
//   BOUND_ZERO_AREA  a triangle with !(dot3(n, n) > 0);
//   BOUND_VOLUME     !(vol6 > 0), vol6 summed in a fixed shape: the triangles in the caller's order
//                    are cut into consecutive chunks of kBoundChunk = 256; a chunk's partial is the
//                    pairwise tree p[i] = p[i] + p[i + w], w = 128, 64, ..., 1 over its terms
//                    A . (B x C) (absent triangles of the last chunk enter as 0.0), and the partials
//                    are added in chunk order onto 0.0.
// lo / hi receive the exact range of the referenced vertices (meaningful when the cause is 0; a
// tie between -0.0 and +0.0 may resolve either way, which no comparison against the box sees).
constexpr int kBoundChunk = 256;
enum BoundCause { BOUND_OK = 0, BOUND_NONFINITE = 1, BOUND_ZERO_AREA = 2, BOUND_VOLUME = 3 };

namespace mesh_detail {
// one triangle of the check: whether its area vanishes, and its vol6 term A . (B x C)
AA_HD inline bool bound_tri_term(const double* A, const double* B, const double* C, double& term) {
    double u[3], w[3], n[3];
    sub3(B, A, u); sub3(C, A, w); cross3(u, w, n);
    const bool zero = !(dot3(n, n) > 0.0);
    cross3(B, C, n);
    term = dot3(A, n);
    return zero;
}
}  // namespace mesh_detail

// V[i] = x3[nodes[i]], i < nv (the host restatement of the device gather)
inline void gather_bound_vertices(const double* x3, const int* nodes, int nv, double* V) {
    for (int i = 0; i < nv; ++i)
        for (int d = 0; d < 3; ++d) V[3 * (size_t)i + d] = x3[3 * (size_t)nodes[i] + d];
}

inline int check_bound_refit(const MeshRefitTables& T, const double* V, double* vol6_out, double* lo, double* hi) {
    using namespace mesh_detail;
    bool bad = false, zero = false;
    for (size_t i = 0; i < 3 * (size_t)T.nv; ++i) bad = bad || !std::isfinite(V[i]);
    const int nf = (int)T.F.size() / 3;
    for (int d = 0; d < 3; ++d) { lo[d] = DBL_MAX; hi[d] = -DBL_MAX; }
    double vol6 = 0.0;
    for (int t0 = 0; t0 < nf; t0 += kBoundChunk) {
        double p[kBoundChunk];
        for (int j = 0; j < kBoundChunk; ++j) {
            p[j] = 0.0;
            const int t = t0 + j;
            if (t >= nf) continue;
            const double *A = V + 3 * (size_t)T.F[3 * (size_t)t], *B = V + 3 * (size_t)T.F[3 * (size_t)t + 1],
                         *C = V + 3 * (size_t)T.F[3 * (size_t)t + 2];
            if (bound_tri_term(A, B, C, p[j])) zero = true;
            for (const double* P : {A, B, C})
                for (int d = 0; d < 3; ++d) { lo[d] = P[d] < lo[d] ? P[d] : lo[d]; hi[d] = P[d] > hi[d] ? P[d] : hi[d]; }
        }
        for (int w = kBoundChunk / 2; w > 0; w >>= 1)
            for (int j = 0; j < w; ++j) p[j] = p[j] + p[j + w];
        vol6 = vol6 + p[0];
    }
    if (vol6_out) *vol6_out = vol6;
    return bad ? BOUND_NONFINITE : (zero ? BOUND_ZERO_AREA : (!(vol6 > 0.0) ? BOUND_VOLUME : BOUND_OK));
}

namespace mesh_detail {
// unit normal and the three clamped corner angles of a triangle (prepare_mesh_obstacle's formulas)
AA_HD inline void tri_normal_angles(const double* v9, double* fn, double* ang) {
    double u[3], w[3], n[3];
    sub3(v9 + 3, v9, u); sub3(v9 + 6, v9, w); cross3(u, w, n);
    const double l = std::sqrt(dot3(n, n));
    for (int d = 0; d < 3; ++d) fn[d] = n[d] / l;
    for (int a = 0; a < 3; ++a) {
        double e1[3], e2[3];
        sub3(v9 + 3 * ((a + 1) % 3), v9 + 3 * a, e1);
        sub3(v9 + 3 * ((a + 2) % 3), v9 + 3 * a, e2);
        double c = dot3(e1, e2) / std::sqrt(dot3(e1, e1) * dot3(e2, e2));
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
        ang[a] = std::acos(c);
    }
}
}  // namespace mesh_detail

// The refit itself, on the host: M (as prepared, or as refitted before) taken to the vertices V.
// V is expected to have passed validate_mesh_refit.
inline void refit_mesh_obstacle_host(MeshObstacleHost& M, const MeshRefitTables& T, const double* V) {
    using namespace mesh_detail;
    const int nf = (int)M.tris.size(), nn = (int)M.nodes.size();
    std::vector<double> fa(6 * (size_t)nf);   // per leaf triangle: unit normal, three corner angles
    for (int k = 0; k < nf; ++k) {
        for (int a = 0; a < 3; ++a)
            for (int d = 0; d < 3; ++d) M.tris[k].v[3 * a + d] = V[3 * (size_t)T.leaf_vid[3 * (size_t)k + a] + d];
        tri_normal_angles(M.tris[k].v, &fa[6 * (size_t)k], &fa[6 * (size_t)k + 3]);
    }
    static const int corner_slot[3] = {0, 1, 3}, edge_slot[3] = {2, 5, 4};   // a b c; ab bc ca
    for (int k = 0; k < nf; ++k) {
        double* P = M.pn.data() + (size_t)kPnStride * k;
        for (int a = 0; a < 3; ++a) {
            const int p = T.leaf_vid[3 * (size_t)k + a];
            double s[3] = {0.0, 0.0, 0.0};
            for (int j = T.vt_ptr[p]; j < T.vt_ptr[p + 1]; ++j) {
                const double* f = &fa[6 * (size_t)(T.vt[j] >> 2)];
                const double ang = f[3 + (T.vt[j] & 3)];
                for (int d = 0; d < 3; ++d) s[d] += ang * f[d];
            }
            const double* f0 = &fa[6 * (size_t)T.edge_tris[6 * (size_t)k + 2 * a]];
            const double* f1 = &fa[6 * (size_t)T.edge_tris[6 * (size_t)k + 2 * a + 1]];
            for (int d = 0; d < 3; ++d) {
                P[3 * corner_slot[a] + d] = s[d];
                P[3 * edge_slot[a] + d] = (0.0 + f0[d]) + f1[d];
            }
        }
        for (int d = 0; d < 3; ++d) P[18 + d] = fa[6 * (size_t)k + d];
    }
    for (int i = 0; i < nn; ++i) {
        BvhNode& nd = M.nodes[i];
        const float* axes[3] = {nd.nrm, nd.t1, nd.t2};
        double lo[6], hi[6];
        for (int c = 0; c < 6; ++c) { lo[c] = DBL_MAX; hi[c] = -DBL_MAX; }
        for (int k = T.node_beg[i]; k < T.node_beg[i] + T.node_cnt[i]; ++k)
            for (int a = 0; a < 3; ++a) {
                const double* P = M.tris[k].v + 3 * a;
                for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], P[d]); hi[d] = std::max(hi[d], P[d]); }
                for (int x = 0; x < 3; ++x) {
                    const double s = ((double)axes[x][0] * P[0] + (double)axes[x][1] * P[1]) + (double)axes[x][2] * P[2];
                    lo[3 + x] = std::min(lo[3 + x], s); hi[3 + x] = std::max(hi[3 + x], s);
                }
            }
        for (int d = 0; d < 3; ++d) { nd.lo[d] = BvhBuilder::down(lo[d]); nd.hi[d] = BvhBuilder::up(hi[d]); }
        float* rl[3] = {&nd.dlo, &nd.t1lo, &nd.t2lo};
        float* rh[3] = {&nd.dhi, &nd.t1hi, &nd.t2hi};
        for (int x = 0; x < 3; ++x) {
            if (*rl[x] == -FLT_MAX && *rh[x] == FLT_MAX) continue;   // stored unbounded: stays so
            *rl[x] = BvhBuilder::down(lo[3 + x]); *rh[x] = BvhBuilder::up(hi[3 + x]);
        }
    }
    for (int d = 0; d < 3; ++d) { M.lo[d] = DBL_MAX; M.hi[d] = -DBL_MAX; }
    for (int k = 0; k < nf; ++k)
        for (int c = 0; c < 9; ++c) { M.lo[c % 3] = std::min(M.lo[c % 3], M.tris[k].v[c]); M.hi[c % 3] = std::max(M.hi[c % 3], M.tris[k].v[c]); }
}

// A bound refit on the host: gather through nodes, check, and refit only when the check passes (a
// failed check leaves M exactly as it was). Returns the cause.
inline int bound_refit_host(MeshObstacleHost& M, const MeshRefitTables& T, const double* x3, const int* nodes, double* vol6) {
    std::vector<double> V(3 * (size_t)T.nv);
    gather_bound_vertices(x3, nodes, T.nv, V.data());
    double lo[3], hi[3];
    const int cause = check_bound_refit(T, V.data(), vol6, lo, hi);
    if (cause != BOUND_OK) return cause;
    refit_mesh_obstacle_host(M, T, V.data());
    for (int d = 0; d < 3; ++d) { M.lo[d] = lo[d]; M.hi[d] = hi[d]; }
    return cause;
}

}  // namespace aa
