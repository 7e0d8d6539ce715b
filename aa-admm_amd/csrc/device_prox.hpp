// Per-element proximal operators, device side (one element per thread, all in registers).
//
// Semantics follow the reference element plugins:
//   TriEnergyTerm::prox   (UX variant) admm_anderson_hard_zxu/src/TriEnergyTerm.cpp:74-105
//                          z = U clamp((1+S)/2) V^T
//   TriEnergyTerm::prox   (Z variant)  admm_anderson_xzu/src/TriEnergyTerm.cpp:77-108
//                          z = (U[I;0]V^T + F)/2 then per-column norm clamp
//   TetEnergyTerm::prox   admm_anderson_hard_zxu/src/TetEnergyTerm.cpp:74-96
//                          z = (U diag(1,1,det F<1e-16 ? -1 : 1) V^T + F)/2
//   TetEnergyTerm::get_gradient (Z variant, admm_anderson_xzu/src/TetEnergyTerm.cpp:156-165)
//
// The reference uses Eigen::JacobiSVD. The 3x2 SVD here is the exact one-rotation one-sided
// Jacobi (the projection z = sum_i f(s_i) u_i v_i^T is invariant to the SVD's sign and order
// freedom, so only rounding differs); the 3x3 SVD is a register-resident two-sided Jacobi with
// Eigen's 2x2 step, stopping rule and descending sort, so that the det-flip picks the same
// singular pair. The 3x3 path is compiled without FMA contraction (Eigen's x86 build has none):
// for a (near-)singular F the null-space pair, hence U diag(1,1,-1) V^T, is decided by rounding,
// and only the same operation-by-operation rounding reproduces the reference's choice there.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh_device.hpp"
#include "elastic_kernels.hpp"

namespace aa {
namespace dev {

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// ------------------------------------------------------------------ bending hinges (3x1)
// U(z) = 1/2 kappa (|z| - r)^2 with the ADMM weight w^2 = kappa (bending.hpp): the minimiser of
// U(z) + 1/2 w^2 |z - v|^2 lies along v at length (|v| + r) / 2, i.e. z = s v with
// s = 1/2 + 1/2 (r / |v|). v = 0 has no direction: z = v (stated, not derived; r = 0 gives the same).
__device__ __forceinline__ void hinge_prox(const double* v, double r, double* out) {
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double s = n == 0.0 ? 1.0 : 0.5 + 0.5 * (r / n);
    out[0] = s * v[0]; out[1] = s * v[1]; out[2] = s * v[2];
}

// ------------------------------------------------------------------ springs (3x1, two nodes)
// z = x_b - x_a, rest length L, w^2 = k (springs.hpp). mode & 3: 0 two-sided, U = 1/2 k (|z| - L)^2,
// the hinge's statement s = 1/2 + 1/2 (L / n); 1 tether, U = 1/2 k max(0, |z| - L)^2: slack at
// n <= L, z = v bitwise; 2 strut, U = 1/2 k max(0, L - |z|)^2: slack at n >= L. mode & 4 (hard): U
// the indicator of |z| = L / <= L / >= L, s = L / n where the soft form would act. n = 0 has no
// direction: z = v in every mode (stated, not derived).
__device__ __forceinline__ void spring_prox(const double* v, double L, int mode, double* out) {
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const int side = mode & 3;
    const bool slack = n == 0.0 || (side == 1 && n <= L) || (side == 2 && n >= L);
    if (slack) {
        out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
        return;
    }
    const double q = L / n;
    const double s = (mode & 4) ? q : 0.5 + 0.5 * q;
    out[0] = s * v[0]; out[1] = s * v[1]; out[2] = s * v[2];
}

// ------------------------------------------------------------------ triangles (3x2)
// z: column-major 3x2 (z[c*3+r]); mode 1 = UX (hard_zxu), 0 = Z (xzu)
__device__ __forceinline__ void tri_prox(const double* z, double* out, int mode, double lmin, double lmax) {
    const double* f0 = z;
    const double* f1 = z + 3;
    const double a = dot3(f0, f0), b = dot3(f1, f1), c = dot3(f0, f1);
    double cs = 1.0, sn = 0.0;
    if (c != 0.0) {
        const double zeta = (b - a) / (2.0 * c);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        cs = 1.0 / sqrt(1.0 + t * t);
        sn = cs * t;
    }
    double g0[3], g1[3];
    for (int r = 0; r < 3; ++r) { g0[r] = cs * f0[r] - sn * f1[r]; g1[r] = sn * f0[r] + cs * f1[r]; }
    double s0 = sqrt(dot3(g0, g0)), s1 = sqrt(dot3(g1, g1));
    double u0[3], u1[3];
    if (s0 > 0) { for (int r = 0; r < 3; ++r) u0[r] = g0[r] / s0; }
    else { u0[0] = 1; u0[1] = 0; u0[2] = 0; }
    if (s1 > 0) { for (int r = 0; r < 3; ++r) u1[r] = g1[r] / s1; }
    else {  // rank-deficient: any unit vector orthogonal to u0 (Eigen's choice is arbitrary too)
        double e[3] = {0, 0, 0};
        int k = fabs(u0[0]) <= fabs(u0[1]) ? (fabs(u0[0]) <= fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
        e[k] = 1;
        double d = dot3(e, u0);
        for (int r = 0; r < 3; ++r) u1[r] = e[r] - d * u0[r];
        double l = sqrt(dot3(u1, u1));
        for (int r = 0; r < 3; ++r) u1[r] /= l;
    }
    const double v0[2] = {cs, -sn}, v1[2] = {sn, cs};
    if (mode == 1) {
        double sg0 = (1.0 + s0) / 2.0, sg1 = (1.0 + s1) / 2.0;
        if (lmin > 0.0 || lmax < 99.0) {
            const double l0 = sg0, l1 = sg1;
            if (l0 < lmin) sg0 = lmin;
            if (l1 < lmin) sg1 = lmin;
            if (l0 > lmax) sg0 = lmax;
            if (l1 > lmax) sg1 = lmax;
        }
        for (int cc = 0; cc < 2; ++cc)
            for (int r = 0; r < 3; ++r) out[cc * 3 + r] = u0[r] * sg0 * v0[cc] + u1[r] * sg1 * v1[cc];
    } else {
        for (int cc = 0; cc < 2; ++cc)
            for (int r = 0; r < 3; ++r) out[cc * 3 + r] = 0.5 * ((u0[r] * v0[cc] + u1[r] * v1[cc]) + z[cc * 3 + r]);
        if (lmin > 0.0 || lmax < 99.0) {
            const double l0 = sqrt(dot3(out, out)), l1 = sqrt(dot3(out + 3, out + 3));
            if (l0 < lmin) for (int i = 0; i < 3; ++i) out[i] *= lmin / l0;
            if (l1 < lmin) for (int i = 3; i < 6; ++i) out[i] *= lmin / l1;
            if (l0 > lmax) for (int i = 0; i < 3; ++i) out[i] *= lmax / l0;
            if (l1 > lmax) for (int i = 3; i < 6; ++i) out[i] *= lmax / l1;
        }
    }
}

// ------------------------------------------------------------------ tets (3x3)
struct Rot2 { double c, s; };

__device__ __forceinline__ Rot2 jacobi_rot(double x, double y, double z) {  // J^T [[x y][y z]] J diagonal
#pragma clang fp contract(off)
    Rot2 r{1.0, 0.0};
    const double deno = 2.0 * fabs(y);
    if (deno < 2.2250738585072014e-308) return r;
    const double tau = (x - z) / deno;
    const double w = sqrt(tau * tau + 1.0);
    const double t = tau > 0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
    const double sign_t = t > 0 ? 1.0 : -1.0;
    const double n = 1.0 / sqrt(t * t + 1.0);
    r.s = -sign_t * (y > 0 ? 1.0 : -1.0) * fabs(t) * n;
    r.c = n;
    return r;
}

// W, U, V row-major 3x3 in registers; one Eigen-style 2x2 step on pair (P,Q)
template <int P, int Q>
__device__ __forceinline__ bool jacobi_pair(double (&W)[9], double (&U)[9], double (&V)[9], double& maxDiag) {
#pragma clang fp contract(off)
    const double thr = fmax(2.2250738585072014e-308, 2.0 * 2.220446049250313e-16 * maxDiag);
    if (!(fabs(W[P * 3 + Q]) > thr || fabs(W[Q * 3 + P]) > thr)) return false;
    // real 2x2 Jacobi SVD of [[W_pp W_pq][W_qp W_qq]]
    const double m00 = W[P * 3 + P], m01 = W[P * 3 + Q], m10 = W[Q * 3 + P], m11 = W[Q * 3 + Q];
    Rot2 r1;
    const double t = m00 + m11, d = m10 - m01;
    if (fabs(d) < 2.2250738585072014e-308) { r1.s = 0; r1.c = 1; }
    else { const double u = t / d; const double tmp = sqrt(1.0 + u * u); r1.s = 1.0 / tmp; r1.c = u / tmp; }
    const double a00 = r1.c * m00 + r1.s * m10, a01 = r1.c * m01 + r1.s * m11, a11 = -r1.s * m01 + r1.c * m11;
    const Rot2 jr = jacobi_rot(a00, a01, a11);
    const Rot2 jl{r1.c * jr.c + r1.s * jr.s, r1.c * (-jr.s) + r1.s * jr.c};  // r1 * jr^T
    // W = jl applied on the left to rows P,Q
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = W[P * 3 + i], y = W[Q * 3 + i];
        W[P * 3 + i] = jl.c * x + jl.s * y;
        W[Q * 3 + i] = -jl.s * x + jl.c * y;
    }
    // U = U * jl^T  (columns P,Q): apply_rotation(col_p, col_q, (jl^T)^T = jl)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = U[i * 3 + P], y = U[i * 3 + Q];
        U[i * 3 + P] = jl.c * x + jl.s * y;
        U[i * 3 + Q] = -jl.s * x + jl.c * y;
    }
    // W = W * jr, V = V * jr  (columns): apply_rotation(col_p, col_q, jr^T)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = W[i * 3 + P], y = W[i * 3 + Q];
        W[i * 3 + P] = jr.c * x - jr.s * y;
        W[i * 3 + Q] = jr.s * x + jr.c * y;
        const double vx = V[i * 3 + P], vy = V[i * 3 + Q];
        V[i * 3 + P] = jr.c * vx - jr.s * vy;
        V[i * 3 + Q] = jr.s * vx + jr.c * vy;
    }
    maxDiag = fmax(maxDiag, fmax(fabs(W[P * 3 + P]), fabs(W[Q * 3 + Q])));
    return true;
}

// F row-major 3x3 -> U S V^T, S descending (Eigen JacobiSVD semantics, square case)
__device__ __forceinline__ void svd3(const double (&F)[9], double (&U)[9], double (&S)[3], double (&V)[9]) {
#pragma clang fp contract(off)
    double scale = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) scale = fmax(scale, fabs(F[i]));
    if (scale == 0) scale = 1;
    double W[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { W[i] = F[i] / scale; U[i] = (i % 4 == 0) ? 1.0 : 0.0; V[i] = U[i]; }
    double maxDiag = fmax(fabs(W[0]), fmax(fabs(W[4]), fabs(W[8])));
    for (int sweep = 0; sweep < 32; ++sweep) {
        bool any = jacobi_pair<1, 0>(W, U, V, maxDiag);
        any |= jacobi_pair<2, 0>(W, U, V, maxDiag);
        any |= jacobi_pair<2, 1>(W, U, V, maxDiag);
        if (!any) break;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = W[i * 4];
        S[i] = fabs(a) * scale;
        if (a < 0) { U[0 * 3 + i] = -U[0 * 3 + i]; U[1 * 3 + i] = -U[1 * 3 + i]; U[2 * 3 + i] = -U[2 * 3 + i]; }
    }
    // selection sort, descending, first max wins (Eigen maxCoeff)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int pos = i;
#pragma unroll
        for (int k = i + 1; k < 3; ++k) if (S[k] > S[pos]) pos = k;
        if (pos != i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k == pos) {
                    double t = S[i]; S[i] = S[k]; S[k] = t;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        double tu = U[r * 3 + i]; U[r * 3 + i] = U[r * 3 + k]; U[r * 3 + k] = tu;
                        double tv = V[r * 3 + i]; V[r * 3 + i] = V[r * 3 + k]; V[r * 3 + k] = tv;
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ double det3rm(const double (&F)[9]) {
#pragma clang fp contract(off)
    return F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
}

// z column-major 9 -> out column-major 9
__device__ __forceinline__ void tet_linear_prox(const double* z, double* out) {
#pragma clang fp contract(off)
    double F[9], U[9], S[3], V[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) F[r * 3 + c] = z[c * 3 + r];
    svd3(F, U, S, V);
    const double s2 = det3rm(F) < 1e-16 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = U[r * 3 + 0] * V[c * 3 + 0] + U[r * 3 + 1] * V[c * 3 + 1] + U[r * 3 + 2] * s2 * V[c * 3 + 2];
            out[c * 3 + r] = 0.5 * (p + z[c * 3 + r]);
        }
}

// k*vol*(F - U V^T)   (Z variant get_gradient of the linear tet)
__device__ __forceinline__ void tet_linear_grad(const double* z, double kvol, double* g) {
#pragma clang fp contract(off)
    double F[9], U[9], S[3], V[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) F[r * 3 + c] = z[c * 3 + r];
    svd3(F, U, S, V);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = U[r * 3 + 0] * V[c * 3 + 0] + U[r * 3 + 1] * V[c * 3 + 1] + U[r * 3 + 2] * V[c * 3 + 2];
            g[c * 3 + r] = kvol * (F[r * 3 + c] - p);
        }
}

// Signed distance of q to a mesh obstacle (mesh_obstacle.hpp). Returns whether q is inside; then
// dx = -|q - c|, c = the closest surface point and tri its triangle (leaf order). c and tri are
// exactly bvh_closest's, cold start; the feature c lies on is read from closest_on_tri's branch on
// that triangle (the same arithmetic on the same inputs, so the same c), and q is inside iff
// (q - c) . n < 0 for the feature's pseudonormal n.
// A point outside the root box is not inside and skips the walk. Those lanes are masked off for
// the whole of bvh_closest: its two-phase schedule counts lanes with __ballot, which reads 0 for
// an inactive lane in both `live` and `held`, so a culled lane is neither waited for nor counted
// toward the hold share -- the schedule sees a wave of the remaining lanes only.
__device__ inline double mesh_closest_signed(const MeshObsDev& mo, const double* q, double* c, int& tri) {
#pragma clang fp contract(off)
    double cx, cy, cz;
    tri = bvh_closest(mo.surf, q[0], q[1], q[2], -1, cx, cy, cz);
    int region = TRI_FACE;
    closest_on_tri(mo.surf.tris[tri].v, q[0], q[1], q[2], cx, cy, cz, region);
    c[0] = cx; c[1] = cy; c[2] = cz;
    const double* n = mo.pn + (size_t)kPnStride * tri + 3 * region;
    return (q[0] - cx) * n[0] + (q[1] - cy) * n[1] + (q[2] - cz) * n[2];
}
__device__ inline bool mesh_in_root_box(const MeshObsDev& mo, const double* q) {
    return q[0] >= mo.lo[0] && q[0] <= mo.hi[0] && q[1] >= mo.lo[1] && q[1] <= mo.hi[1] && q[2] >= mo.lo[2] &&
           q[2] <= mo.hi[2];
}
// Kinematic rows (mo.posed, a wave-uniform branch: every lane reads the same row): the candidate
// goes into the obstacle frame, q_l = R^T (q - t), everything above runs there on q_l -- the cull
// after the transform, so a culled lane is still masked off for the whole walk -- and the closest
// point comes back, c_w = R c_l + t. The operation order is fixed (no contraction, sums left to
// right) so that a host restatement gives the same bits. dx is the obstacle-frame distance.
// An unposed row runs the arithmetic it always did.
__device__ inline void mesh_to_local(const MeshObsDev& mo, const double* q, double* ql) {
#pragma clang fp contract(off)
    const double d0 = q[0] - mo.t[0], d1 = q[1] - mo.t[1], d2 = q[2] - mo.t[2];
    for (int i = 0; i < 3; ++i) ql[i] = (mo.R[i] * d0 + mo.R[3 + i] * d1) + mo.R[6 + i] * d2;
}
__device__ inline void mesh_to_world(const MeshObsDev& mo, const double* cl, double* c) {
#pragma clang fp contract(off)
    const double c0 = cl[0], c1 = cl[1], c2 = cl[2];
    for (int i = 0; i < 3; ++i) c[i] = ((mo.R[3 * i] * c0 + mo.R[3 * i + 1] * c1) + mo.R[3 * i + 2] * c2) + mo.t[i];
}
__device__ inline bool mesh_signed_distance(const MeshObsDev& mo, const double* q, double& dx, double* c, int& tri) {
    double ql[3] = {q[0], q[1], q[2]};
    if (mo.posed) mesh_to_local(mo, q, ql);
    if (!mesh_in_root_box(mo, ql)) return false;
    if (!(mesh_closest_signed(mo, ql, c, tri) < 0.0)) return false;
    dx = -sqrt(dist2(ql[0], ql[1], ql[2], c[0], c[1], c[2]));
    if (mo.posed) mesh_to_world(mo, c, c);
    return true;
}
__device__ __forceinline__ const MeshObsDev* mesh_table_of(const MeshObsDev* t) { return t; }
// Exemption: the pack of the solver's mesh-aware form is (table, the element's node in the internal
// numbering); a node marked in a row's byte array skips that row as if it were not in the list. The
// form without a node (the table alone) has no exemption and the code it always had.
__device__ __forceinline__ const MeshObsDev* mesh_table_of(const MeshObsDev* t, int) { return t; }
__device__ __forceinline__ bool mesh_exempts(const MeshObsDev&, const MeshObsDev*) { return false; }
__device__ __forceinline__ bool mesh_exempts(const MeshObsDev& mo, const MeshObsDev*, int node) {
    return mo.exempt && mo.exempt[node];
}

// (1/w) * ((w x + u) - c) of an identity-reduction row, without FMA contraction (c = -w x_pin for
// a pinned node, whose x enters through c: the same sum)
__device__ inline void collision_candidate(const double* x, const double* u, double w, double* q) {
#pragma clang fp contract(off)
    const double iw = 1.0 / w;
    for (int i = 0; i < 3; ++i) q[i] = iw * (w * x[i] + u[i]);
}

// Collision::prox (admm_anderson_hard_zxu/src/CollisionEnergyTerm.hpp:79-91): the candidate q is
// tested against every passive obstacle in insertion order; an obstacle replaces the running
// (dx, point) when its signed distance is <= the current one (PassiveObject.hpp's `if (dx >
// p.dx) return;`), and q moves to the closest surface point when the final dx < 0. The
// signed-distance functions restate PassiveObject.hpp:32-136 with the reference's operation
// order (no FMA contraction, Eigen's norm / normalize: division by sqrt of the squared norm).
// Obstacle table: obs[0] = count, then kObsStride doubles each: type, parameters.
// Mesh-aware form: a trailing mesh table (the collision group's parameter pack, as GroupVar is
// the per-element materials') adds the OBS_MESH rows, o[1] = the mesh's row in the table. An
// inside hit replaces the running (dx, point) unconditionally -- PassiveMesh::signed_distance has
// no `if (dx > p.dx) return;` (PassiveObject.hpp:160-175) -- and a miss leaves it untouched. With
// the element's node after the table, a row that exempts the node is passed over (mesh_exempts).
// Without the table the code is the analytic shapes' alone.
template <class... M>
__device__ inline void collision_prox(const double* q, const double* obs, double* out, M... meshes) {
#pragma clang fp contract(off)
    double best = 1.79769313486231570815e+308;   // std::numeric_limits<double>::max()
    double pt[3] = {0.0, 0.0, 0.0};
    const int n = obs ? (int)obs[0] : 0;
    auto sq3 = [](double a, double b, double c) { return (a * a + b * b) + c * c; };   // squaredNorm
    for (int k = 0; k < n; ++k) {
        const double* o = obs + 1 + k * kObsStride;
        const int type = (int)o[0];
        double dx, p0, p1, p2;
        if (type == OBS_FLOOR) {                      // Floor(y)                   :32-45
            dx = q[1] - o[1];
            p0 = q[0]; p1 = o[1]; p2 = q[2];
        } else if (type == OBS_SLIDE_FLOOR) {         // SlideFloor(center, normal) :47-62
            const double l0 = q[0] - o[1], l1 = q[1] - o[2], l2 = q[2] - o[3];
            dx = l0 * o[4] + l1 * o[5] + l2 * o[6];
            p0 = q[0] - dx * o[4]; p1 = q[1] - dx * o[5]; p2 = q[2] - dx * o[6];
        } else if (type == OBS_SPHERE) {              // Sphere(center, rad)        :64-80
            double d0 = q[0] - o[1], d1 = q[1] - o[2], d2 = q[2] - o[3];
            const double z2 = sq3(d0, d1, d2), nrm = sqrt(z2);
            dx = nrm - o[4];
            if (dx > best) continue;
            if (z2 > 0.0) { d0 /= nrm; d1 /= nrm; d2 /= nrm; }
            p0 = o[1] + d0 * o[4]; p1 = o[2] + d1 * o[4]; p2 = o[3] + d2 * o[4];
        } else if (type == OBS_PLANE_HALF_SPHERE) {   // PlaneAndHalfSphere         :82-116
            const double dc = sqrt(sq3(q[0] - o[1], 0.0, q[2] - o[3])) - o[4];
            if (dc > 0) {
                dx = q[1] - o[2];
                p0 = q[0]; p1 = o[2]; p2 = q[2];
            } else {
                const double dpl = q[1] - o[2];
                double d0 = q[0] - o[1], d1 = q[1] - o[2], d2 = q[2] - o[3];
                const double z2 = sq3(d0, d1, d2), nrm = sqrt(z2);
                dx = dpl > 0 ? nrm + o[4] : o[4] - nrm;
                if (dx > best) continue;
                if (z2 > 0.0) { d0 /= nrm; d1 /= nrm; d2 /= nrm; }
                p0 = o[1] + d0 * o[4]; p1 = o[2] + d1 * o[4]; p2 = o[3] + d2 * o[4];
            }
        } else if (sizeof...(M) != 0 && type == OBS_MESH) {   // PassiveMesh            :138-178
            if constexpr (sizeof...(M) != 0) {
                const MeshObsDev& mo = mesh_table_of(meshes...)[(int)o[1]];
                if (mesh_exempts(mo, meshes...)) continue;   // the running payload stays as it is
                double c[3];
                int tri;
                if (!mesh_signed_distance(mo, q, dx, c, tri)) continue;
                best = dx;
                pt[0] = c[0]; pt[1] = c[1]; pt[2] = c[2];
            }
            continue;
        } else {                                      // Cylinder(center, rad), axis z :118-136
            double d0 = q[0] - o[1], d1 = q[1] - o[2], d2 = 0.0 - o[3];
            const double z2 = sq3(d0, d1, d2), nrm = sqrt(z2);
            dx = nrm - o[4];
            if (dx > best) continue;
            if (z2 > 0.0) { d0 /= nrm; d1 /= nrm; d2 /= nrm; }
            p0 = o[1] + d0 * o[4] + 0.0; p1 = o[2] + d1 * o[4] + 0.0; p2 = o[3] + d2 * o[4] + q[2];
        }
        if (dx > best) continue;
        best = dx;
        pt[0] = p0; pt[1] = p1; pt[2] = p2;
    }
    if (best < 0) { out[0] = pt[0]; out[1] = pt[1]; out[2] = pt[2]; }
    else { out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; }
}

// collision_prox's walk, statement for statement, which also reports the row that supplied the
// final (dx, point): contact iff the final dx < 0, then row = that obstacle's index in the shared
// insertion order and c its point in the world frame. Only the friction pass calls it
// (contact_friction.hip); collision_prox and the kernels built from it are untouched.
// collision_contact_walk also hands on the leaf triangle of the mesh hit that supplied the point
// (-1 for an analytic row): what the carry form of the pass interpolates the surface's own motion
// on. collision_contact, the plain pass's, drops it.
template <class... M>
__device__ inline bool collision_contact_walk(const double* q, const double* obs, int& row, double* c, int& tri_at,
                                              M... meshes) {
#pragma clang fp contract(off)
    double best = 1.79769313486231570815e+308;
    double pt[3] = {0.0, 0.0, 0.0};
    int at = -1, tat = -1;
    const int n = obs ? (int)obs[0] : 0;
    auto sq3 = [](double a, double b, double c) { return (a * a + b * b) + c * c; };
    for (int k = 0; k < n; ++k) {
        const double* o = obs + 1 + k * kObsStride;
        const int type = (int)o[0];
        double dx, p0, p1, p2;
        if (type == OBS_FLOOR) {
            dx = q[1] - o[1];
            p0 = q[0]; p1 = o[1]; p2 = q[2];
        } else if (type == OBS_SLIDE_FLOOR) {
            const double l0 = q[0] - o[1], l1 = q[1] - o[2], l2 = q[2] - o[3];
            dx = l0 * o[4] + l1 * o[5] + l2 * o[6];
            p0 = q[0] - dx * o[4]; p1 = q[1] - dx * o[5]; p2 = q[2] - dx * o[6];
        } else if (type == OBS_SPHERE) {
            double d0 = q[0] - o[1], d1 = q[1] - o[2], d2 = q[2] - o[3];
            const double z2 = sq3(d0, d1, d2), nrm = sqrt(z2);
            dx = nrm - o[4];
            if (dx > best) continue;
            if (z2 > 0.0) { d0 /= nrm; d1 /= nrm; d2 /= nrm; }
            p0 = o[1] + d0 * o[4]; p1 = o[2] + d1 * o[4]; p2 = o[3] + d2 * o[4];
        } else if (type == OBS_PLANE_HALF_SPHERE) {
            const double dc = sqrt(sq3(q[0] - o[1], 0.0, q[2] - o[3])) - o[4];
            if (dc > 0) {
                dx = q[1] - o[2];
                p0 = q[0]; p1 = o[2]; p2 = q[2];
            } else {
                const double dpl = q[1] - o[2];
                double d0 = q[0] - o[1], d1 = q[1] - o[2], d2 = q[2] - o[3];
                const double z2 = sq3(d0, d1, d2), nrm = sqrt(z2);
                dx = dpl > 0 ? nrm + o[4] : o[4] - nrm;
                if (dx > best) continue;
                if (z2 > 0.0) { d0 /= nrm; d1 /= nrm; d2 /= nrm; }
                p0 = o[1] + d0 * o[4]; p1 = o[2] + d1 * o[4]; p2 = o[3] + d2 * o[4];
            }
        } else if (sizeof...(M) != 0 && type == OBS_MESH) {
            if constexpr (sizeof...(M) != 0) {
                const MeshObsDev& mo = mesh_table_of(meshes...)[(int)o[1]];
                if (mesh_exempts(mo, meshes...)) continue;
                double cm[3];
                int tri;
                if (!mesh_signed_distance(mo, q, dx, cm, tri)) continue;
                best = dx;
                pt[0] = cm[0]; pt[1] = cm[1]; pt[2] = cm[2];
                at = k;
                tat = tri;
            }
            continue;
        } else {
            double d0 = q[0] - o[1], d1 = q[1] - o[2], d2 = 0.0 - o[3];
            const double z2 = sq3(d0, d1, d2), nrm = sqrt(z2);
            dx = nrm - o[4];
            if (dx > best) continue;
            if (z2 > 0.0) { d0 /= nrm; d1 /= nrm; d2 /= nrm; }
            p0 = o[1] + d0 * o[4] + 0.0; p1 = o[2] + d1 * o[4] + 0.0; p2 = o[3] + d2 * o[4] + q[2];
        }
        if (dx > best) continue;
        best = dx;
        pt[0] = p0; pt[1] = p1; pt[2] = p2;
        at = k;
        tat = -1;
    }
    row = at;
    tri_at = tat;
    c[0] = pt[0]; c[1] = pt[1]; c[2] = pt[2];
    return best < 0;
}
template <class... M>
__device__ inline bool collision_contact(const double* q, const double* obs, int& row, double* c, M... meshes) {
    int tri;
    return collision_contact_walk(q, obs, row, c, tri, meshes...);
}

// Coulomb friction of one collision term, applied once per step between the ADMM loop and the
// finalize pass (contact_friction.hpp states the model). fp64, no contraction, sums left to right.
// in:  xo / xn the node's position at the step's start / as the step writes it back, u the term's
//      dual, w its weight, m the node's mass, p the penalty, dt the time step; obs / meshes the
//      tables now, T the previous ones with the coefficients.
// out: the record (hit, row, c, n, j, rt, s) and xn moved in place when s != 0. `filter` false
//      (a pinned node): reported, s = 0.
struct FrictionRec {
    int hit, row;
    double c[3], n[3], j, rt[3], s;
};
// Carry form: the trailing pack is (the carry table, the contact's features to fill). A mesh whose
// row of the table is set carries: its displacement at c is interpolated from its vertices' own
// motion on the contact triangle (mesh_carry_displacement) and it is never still; every other row
// follows the plain rule. The features (tri, b) are written for every mesh-row contact. Without the
// pack the code is the plain pass's.
struct FrictionFeat {
    int tri;        // the caller's triangle index (MeshObsDev::orig); -1 for an analytic row
    double b[3];    // barycentric weights of c_l on its corners A, B, C
};
// b of c_l on leaf triangle v9 = (A, B, C): Cramer's rule on the edge Gram matrix, (1, 0, 0) for a
// triangle with !(den > 0)
__device__ inline void tri_barycentric(const double* v9, const double* cl, double* b) {
#pragma clang fp contract(off)
    double e1[3], e2[3], d[3];
    for (int i = 0; i < 3; ++i) { e1[i] = v9[3 + i] - v9[i]; e2[i] = v9[6 + i] - v9[i]; d[i] = cl[i] - v9[i]; }
    const double d11 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double d12 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2];
    const double d22 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    const double p1 = (d[0] * e1[0] + d[1] * e1[1]) + d[2] * e1[2];
    const double p2 = (d[0] * e2[0] + d[1] * e2[1]) + d[2] * e2[2];
    const double den = d11 * d22 - d12 * d12;
    if (!(den > 0.0)) { b[0] = 1.0; b[1] = 0.0; b[2] = 0.0; return; }
    b[1] = (d22 * p1 - d12 * p2) / den;
    b[2] = (d11 * p2 - d12 * p1) / den;
    b[0] = (1.0 - b[1]) - b[2];
}
// g of a carrying mesh at c (c_l in the obstacle frame now): the corners' displacements since the
// previous step's pass interpolated with b, taken off c_l, and the result carried by the previous
// pose. With unchanged vertices every corner difference is an exact zero and g is the rigid one.
__device__ inline void mesh_carry_displacement(const MeshObsDev& prev, const MeshCarryDev& cy, int tri, const double* v9,
                                               const double* b, const double* c, const double* cl, double* g) {
#pragma clang fp contract(off)
    const int* vid = cy.leaf_vid + 3 * (size_t)tri;
    const double *A = cy.vprev + 3 * (size_t)vid[0], *B = cy.vprev + 3 * (size_t)vid[1], *C = cy.vprev + 3 * (size_t)vid[2];
    double pl[3], cp[3];
    for (int i = 0; i < 3; ++i) {
        const double gl = (b[0] * (v9[i] - A[i]) + b[1] * (v9[3 + i] - B[i])) + b[2] * (v9[6 + i] - C[i]);
        pl[i] = cl[i] - gl;
    }
    mesh_to_world(prev, pl, cp);
    for (int i = 0; i < 3; ++i) g[i] = c[i] - cp[i];
}
__device__ __forceinline__ const MeshCarryDev* carry_table_of(const MeshCarryDev* t, FrictionFeat*) { return t; }
__device__ __forceinline__ FrictionFeat* carry_feat_of(const MeshCarryDev*, FrictionFeat* f) { return f; }

template <class... K>
__device__ inline void contact_friction(const double* xo, double* xn, const double* u, double w, double m, double p,
                                        double dt, const double* obs, const MeshObsDev* meshes, int node,
                                        const FrictionTables& T, bool filter, FrictionRec& r, K... carry) {
#pragma clang fp contract(off)
    r.hit = 0; r.row = -1; r.j = 0.0; r.s = 0.0;
    for (int i = 0; i < 3; ++i) { r.c[i] = 0.0; r.n[i] = 0.0; r.rt[i] = 0.0; }
    double q[3], c[3];
    collision_candidate(xn, u, w, q);
    int row;
    int tri = -1;
    bool in;
    if constexpr (sizeof...(K) != 0) {
        FrictionFeat* f = carry_feat_of(carry...);
        f->tri = -1; f->b[0] = 0.0; f->b[1] = 0.0; f->b[2] = 0.0;
        in = meshes ? collision_contact_walk(q, obs, row, c, tri, meshes, node) : collision_contact_walk(q, obs, row, c, tri);
    } else {
        in = meshes ? collision_contact(q, obs, row, c, meshes, node) : collision_contact(q, obs, row, c);
    }
    if (!in) return;
    const double e0 = c[0] - q[0], e1 = c[1] - q[1], e2 = c[2] - q[2];
    const double l = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    if (l == 0.0) return;
    const double n[3] = {e0 / l, e1 / l, e2 / l};
    const double un = (u[0] * n[0] + u[1] * n[1]) + u[2] * n[2];
    const double k = (((p * dt) * dt) * w) / m;
    const double j = un < 0.0 ? k * (-un) : 0.0;
    // the obstacle's displacement at c between the previous step's state and this one's
    double g[3] = {0.0, 0.0, 0.0};
    const double* o = obs + 1 + row * kObsStride;
    const int type = (int)o[0];
    const int nprev = (int)T.obs_prev[0];
    if (type == OBS_MESH) {
        const int mr = (int)o[1];
        if constexpr (sizeof...(K) != 0) {
            const MeshCarryDev cy = carry_table_of(carry...)[mr];
            FrictionFeat* f = carry_feat_of(carry...);
            const double* v9 = meshes[mr].surf.tris[tri].v;
            double cl[3], cp[3];
            mesh_to_local(meshes[mr], c, cl);
            tri_barycentric(v9, cl, f->b);
            f->tri = meshes[mr].orig[tri];
            if (cy.vprev) {
                mesh_carry_displacement(T.mesh_prev[mr], cy, tri, v9, f->b, c, cl, g);
            } else if (!T.mesh_still[mr]) {
                mesh_to_world(T.mesh_prev[mr], cl, cp);
                for (int i = 0; i < 3; ++i) g[i] = c[i] - cp[i];
            }
        } else if (!T.mesh_still[mr]) {
            double cl[3], cp[3];
            mesh_to_local(meshes[mr], c, cl);
            mesh_to_world(T.mesh_prev[mr], cl, cp);
            for (int i = 0; i < 3; ++i) g[i] = c[i] - cp[i];
        }
    } else if (row < nprev) {
        const double* op = T.obs_prev + 1 + row * kObsStride;
        if (type == OBS_FLOOR) g[1] = o[1] - op[1];
        else for (int i = 0; i < 3; ++i) g[i] = o[1 + i] - op[1 + i];
    }
    double rel[3];
    for (int i = 0; i < 3; ++i) rel[i] = (xn[i] - xo[i]) - g[i];
    const double rn = (rel[0] * n[0] + rel[1] * n[1]) + rel[2] * n[2];
    double rt[3];
    for (int i = 0; i < 3; ++i) rt[i] = rel[i] - rn * n[i];
    const double lt = sqrt((rt[0] * rt[0] + rt[1] * rt[1]) + rt[2] * rt[2]);
    const double mu = T.mu[row];
    double s = 0.0;
    if (filter && !(mu == 0.0 || j == 0.0 || !(lt > 0.0))) {
        const double a = (mu * j) / lt;
        s = a < 1.0 ? a : 1.0;
    }
    if (s != 0.0)
        for (int i = 0; i < 3; ++i) xn[i] = xn[i] - s * rt[i];
    r.hit = 1; r.row = row; r.j = j; r.s = s;
    for (int i = 0; i < 3; ++i) { r.c[i] = c[i]; r.n[i] = n[i]; r.rt[i] = rt[i]; }
}

}  // namespace dev
}  // namespace aa
