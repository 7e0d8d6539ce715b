// The friction pass on the device (gfx950): one lane per collision term, dev::contact_friction on
// the (u, x) pair the step writes back (contact_friction.hpp states the model).
//   k_contact_friction       the solver's pass: the term's node, dual, weight and mass gathered,
//                            the node's new position moved in place in the buffer the finalize pass
//                            reads, the record written;
//   k_test_contact_friction  the same device function on host-given arrays (aa_test_contact_friction).
// Each has a carry form (a trailing pack), launched only when some mesh carries.
// Every node carries at most one collision term (the terms are made from a set of nodes), so no
// two lanes write the same position. Plain vector loads and stores, no atomics.
// The arithmetic is stated operation by operation for a host restatement, so nothing may be
// contracted into an FMA:
#pragma clang fp contract(off)
#include "contact_friction.hpp"

#include "common.hpp"
#include "device_prox.hpp"

namespace aa {
namespace {

__device__ inline void store_record(const ContactRecDev& rec, size_t k, const dev::FrictionRec& r) {
    rec.hit[k] = r.hit;
    rec.row[k] = r.row;
    rec.j[k] = r.j;
    rec.s[k] = r.s;
    for (int i = 0; i < 3; ++i) {
        rec.c[3 * k + i] = r.c[i];
        rec.n[3 * k + i] = r.n[i];
        rec.rt[3 * k + i] = r.rt[i];
    }
}

__global__ __launch_bounds__(kBlock) void k_contact_friction(GroupDev g, const double* __restrict__ xold,
                                                             double* xsrc, const double* xfull,   // one buffer without Anderson
                                                             const double* __restrict__ u, const double* __restrict__ mass,
                                                             int nf, double penalty, double dt,
                                                             const MeshObsDev* __restrict__ meshes, FrictionTables T,
                                                             ContactRecDev rec, int rec_off) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.count) return;
    const int v = g.idx[e];
    const bool pinned = v >= nf;
    const double* xp = pinned ? xfull : xsrc;
    double xn[3], xo[3], uu[3];
    for (int i = 0; i < 3; ++i) {
        xn[i] = xp[3 * (size_t)v + i];
        xo[i] = xold[3 * (size_t)v + i];
        uu[i] = u[g.zoff + (size_t)i * g.count + e];
    }
    dev::FrictionRec r;
    dev::contact_friction(xo, xn, uu, g.w[e], mass[v], penalty, dt, g.obs, meshes, v, T, !pinned, r);
    if (r.s != 0.0)   // an unfiltered lane's position is not written at all
        for (int i = 0; i < 3; ++i) xsrc[3 * (size_t)v + i] = xn[i];
    store_record(rec, (size_t)rec_off + e, r);
}

__global__ __launch_bounds__(kBlock) void k_test_contact_friction(const double* __restrict__ obs,
                                                                  const MeshObsDev* __restrict__ meshes, FrictionTables T,
                                                                  const int* __restrict__ node,
                                                                  const unsigned char* __restrict__ pinned,
                                                                  const double* __restrict__ xold, double* __restrict__ xnew,
                                                                  const double* __restrict__ u, const double* __restrict__ w,
                                                                  const double* __restrict__ m, double penalty, double dt,
                                                                  int n, ContactRecDev rec) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    double xn[3], xo[3], uu[3];
    for (int i = 0; i < 3; ++i) {
        xn[i] = xnew[3 * (size_t)e + i];
        xo[i] = xold[3 * (size_t)e + i];
        uu[i] = u[3 * (size_t)e + i];
    }
    dev::FrictionRec r;
    dev::contact_friction(xo, xn, uu, w[e], m[e], penalty, dt, obs, meshes, node[e], T, pinned[e] == 0, r);
    if (r.s != 0.0)
        for (int i = 0; i < 3; ++i) xnew[3 * (size_t)e + i] = xn[i];
    store_record(rec, (size_t)e, r);
}

// The carry forms: the same kernels with the carry table and the feature arrays as a trailing
// pack, handed on to dev::contact_friction (a handful of dependent loads more on a lane in contact
// with a carrying mesh: leaf_vid, then three previous vertices). Instantiated with the pack only;
// the kernels above are what a solver without a carrying mesh launches.
__device__ inline void store_features(const ContactFeatDev& feat, size_t k, const dev::FrictionFeat& f) {
    feat.tri[k] = f.tri;
    for (int i = 0; i < 3; ++i) feat.b[3 * k + i] = f.b[i];
}
__device__ __forceinline__ const MeshCarryDev* pack_table(const MeshCarryDev* t, const ContactFeatDev&) { return t; }
__device__ __forceinline__ const ContactFeatDev& pack_feat(const MeshCarryDev*, const ContactFeatDev& f) { return f; }

template <class... K>
__global__ __launch_bounds__(kBlock) void k_contact_friction(GroupDev g, const double* __restrict__ xold, double* xsrc,
                                                             const double* xfull, const double* __restrict__ u,
                                                             const double* __restrict__ mass, int nf, double penalty, double dt,
                                                             const MeshObsDev* __restrict__ meshes, FrictionTables T,
                                                             ContactRecDev rec, int rec_off, K... carry) {
    static_assert(sizeof...(K) == 2, "the carry form takes (carry table, feature arrays)");
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.count) return;
    const int v = g.idx[e];
    const bool pinned = v >= nf;
    const double* xp = pinned ? xfull : xsrc;
    double xn[3], xo[3], uu[3];
    for (int i = 0; i < 3; ++i) {
        xn[i] = xp[3 * (size_t)v + i];
        xo[i] = xold[3 * (size_t)v + i];
        uu[i] = u[g.zoff + (size_t)i * g.count + e];
    }
    dev::FrictionRec r;
    dev::FrictionFeat f;
    dev::contact_friction(xo, xn, uu, g.w[e], mass[v], penalty, dt, g.obs, meshes, v, T, !pinned, r, pack_table(carry...), &f);
    if (r.s != 0.0)
        for (int i = 0; i < 3; ++i) xsrc[3 * (size_t)v + i] = xn[i];
    store_record(rec, (size_t)rec_off + e, r);
    store_features(pack_feat(carry...), (size_t)rec_off + e, f);
}

template <class... K>
__global__ __launch_bounds__(kBlock) void k_test_contact_friction(const double* __restrict__ obs,
                                                                  const MeshObsDev* __restrict__ meshes, FrictionTables T,
                                                                  const int* __restrict__ node,
                                                                  const unsigned char* __restrict__ pinned,
                                                                  const double* __restrict__ xold, double* __restrict__ xnew,
                                                                  const double* __restrict__ u, const double* __restrict__ w,
                                                                  const double* __restrict__ m, double penalty, double dt,
                                                                  int n, ContactRecDev rec, K... carry) {
    static_assert(sizeof...(K) == 2, "the carry form takes (carry table, feature arrays)");
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    double xn[3], xo[3], uu[3];
    for (int i = 0; i < 3; ++i) {
        xn[i] = xnew[3 * (size_t)e + i];
        xo[i] = xold[3 * (size_t)e + i];
        uu[i] = u[3 * (size_t)e + i];
    }
    dev::FrictionRec r;
    dev::FrictionFeat f;
    dev::contact_friction(xo, xn, uu, w[e], m[e], penalty, dt, obs, meshes, node[e], T, pinned[e] == 0, r, pack_table(carry...), &f);
    if (r.s != 0.0)
        for (int i = 0; i < 3; ++i) xnew[3 * (size_t)e + i] = xn[i];
    store_record(rec, (size_t)e, r);
    store_features(pack_feat(carry...), (size_t)e, f);
}

}  // namespace

void launch_contact_friction(const GroupDev& g, const double* xold, double* xsrc, const double* xfull, const double* u,
                             const double* mass, int nf, double penalty, double dt, const MeshObsDev* meshes,
                             const FrictionTables& T, const ContactRecDev& rec, int rec_off, hipStream_t s) {
    if (g.count <= 0) return;
    hipLaunchKernelGGL(k_contact_friction, dim3(blocks_for(g.count)), dim3(kBlock), 0, s, g, xold, xsrc, xfull, u, mass, nf,
                       penalty, dt, meshes, T, rec, rec_off);
    AA_CHECK_LAUNCH();
}

void launch_test_contact_friction(const double* obs, const MeshObsDev* meshes, const FrictionTables& T, const int* node,
                                  const unsigned char* pinned, const double* xold, double* xnew, const double* u,
                                  const double* w, const double* m, double penalty, double dt, int n,
                                  const ContactRecDev& rec, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_test_contact_friction, dim3(blocks_for(n)), dim3(kBlock), 0, s, obs, meshes, T, node, pinned, xold,
                       xnew, u, w, m, penalty, dt, n, rec);
    AA_CHECK_LAUNCH();
}

void launch_contact_friction_carry(const GroupDev& g, const double* xold, double* xsrc, const double* xfull, const double* u,
                                   const double* mass, int nf, double penalty, double dt, const MeshObsDev* meshes,
                                   const FrictionTables& T, const ContactRecDev& rec, int rec_off, const MeshCarryDev* carry,
                                   const ContactFeatDev& feat, hipStream_t s) {
    if (g.count <= 0) return;
    hipLaunchKernelGGL((k_contact_friction<const MeshCarryDev*, ContactFeatDev>), dim3(blocks_for(g.count)), dim3(kBlock), 0, s,
                       g, xold, xsrc, xfull, u, mass, nf, penalty, dt, meshes, T, rec, rec_off, carry, feat);
    AA_CHECK_LAUNCH();
}

void launch_test_contact_friction_carry(const double* obs, const MeshObsDev* meshes, const FrictionTables& T, const int* node,
                                        const unsigned char* pinned, const double* xold, double* xnew, const double* u,
                                        const double* w, const double* m, double penalty, double dt, int n,
                                        const ContactRecDev& rec, const MeshCarryDev* carry, const ContactFeatDev& feat,
                                        hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((k_test_contact_friction<const MeshCarryDev*, ContactFeatDev>), dim3(blocks_for(n)), dim3(kBlock), 0, s,
                       obs, meshes, T, node, pinned, xold, xnew, u, w, m, penalty, dt, n, rec, carry, feat);
    AA_CHECK_LAUNCH();
}

}  // namespace aa
