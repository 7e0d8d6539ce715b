// The triangle-surface BVH shared by the Geometry closest-point constraints and the mesh
// obstacles of the collision terms: node / triangle records and the device-side view. No HIP
// needed (the host builder, bvh_build.hpp, compiles with a plain compiler).
#pragma once

#if defined(__HIPCC__)
#define AA_HD __host__ __device__
#else
#define AA_HD
#endif

namespace aa {

// Bounding-volume hierarchy over one reference triangle surface (closest-point queries of
// PointToRefSurfaceConstraint / ReferenceSurfceConstraint). Nodes in depth-first order:
// the left child of node i is i+1; `a` is the right child (inner) or the first triangle
// (leaf), `b` = -(triangle count) for a leaf, 0 otherwise; `skip` is the first node after
// this node's subtree (the escape link of a stackless traversal).
// 64-B BVH node: box in fp32 rounded OUTWARD (never prunes a box the fp64 box would keep),
// a = right child (inner) or first triangle (leaf), sn = escape link (node after the subtree,
// low 29 bits) | leaf triangle count << 29 (0 = inner), and a slab: the subtree's mean unit
// normal n and the range [dlo, dhi] of n . v over its vertices (rounded outward). The slab
// bounds the distance to every triangle of the subtree from below like the box does, and is
// far tighter for sloped, thin patches seen from afar (a point well off the surface).
// With the two tangent axes t1, t2 (principal directions of the subtree's vertices in the plane
// normal to n) and their ranges the slab becomes an oriented box: a point far above a flat
// patch has the same normal distance to every patch around its foot point, and only the
// tangent ranges tell those patches apart. 128 B, one cache line.
struct alignas(128) BvhNode {
    float lo[3], hi[3];
    int a;
    unsigned sn;
    float nrm[3], dlo, dhi;
    float t1[3], t1lo, t1hi;
    float t2[3], t2lo, t2hi;
};
static_assert(sizeof(BvhNode) == 128, "BvhNode is one 128-B line");
AA_HD inline int bvh_skip(const BvhNode& n) { return (int)(n.sn & 0x1fffffffu); }
AA_HD inline int bvh_count(const BvhNode& n) { return (int)(n.sn >> 29); }
struct BvhTri { double v[9]; };   // triangle corners, stored in leaf order
// The same tree collapsed to `wide_g` (4 or 8) children per node for the group traversal
// (wide_g lanes per query, see bvh_closest_grp): node w's children are the records
// wide[w * wide_g + k], copies of the BvhNode of a descendant log2(wide_g) levels down (or of a
// leaf met earlier), with `a` = the child's wide node (inner) or its first triangle (leaf) and
// sn = triangle count << 29 (0 = inner); unused slots have a = -1. wide_g = 0: not built.
constexpr int kCpStack = 64;   // per-query traversal stack entries of the group traversal
struct SurfDev {
    const BvhNode* nodes;
    const BvhTri* tris;
    int n_nodes, n_tris;
    const BvhNode* wide = nullptr;
    int wide_g = 0;
};

// One mesh obstacle of the collision terms as the device sees it (a row of the solver's mesh
// table, mesh_obstacle.hpp builds it): the BVH, the per-triangle pseudonormals in leaf order
// (kPnStride doubles each: 7 features x 3, indexed by closest_on_tri's region code), the
// leaf-order -> caller's triangle index map and the root box in fp64 (the exact range of the
// vertices: a point outside it is not inside the surface).
// Kinematic obstacles: a rigid pose per row, world = R * local + t (R row-major, obstacle frame ->
// world). Everything above stays in the obstacle frame as uploaded; a posed row's candidate is
// taken into that frame, walked there, and the closest point taken back (device_prox.hpp).
// posed = 0: the row is read as before the pose existed (R, t are not looked at).
constexpr int kPnStride = 21;
struct MeshObsDev {
    SurfDev surf;
    const double* pn;
    const int* orig;
    double lo[3], hi[3];
    double R[9], t[3];
    int posed;
    // Exemption: one byte per node in the solver's internal numbering, non-zero = that node's
    // collision term skips this mesh as if it were not in the obstacle list (null = no node is exempt)
    const unsigned char* exempt;
};

}  // namespace aa
