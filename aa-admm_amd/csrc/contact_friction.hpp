// Coulomb friction of the collision terms against their obstacles, moving ones included: one pass
// per time step between the ADMM loop and the finalize pass, one lane per collision term, outside
// the captured iteration graph. It launches only when some obstacle row has a coefficient > 0 or
// contact recording is on; a scene that sets neither runs exactly what it ran before.
//
// Model (lagged, explicit; dev::contact_friction in device_prox.hpp is the arithmetic). With the
// (u, x) pair the step writes back, for a term of weight w on a node of mass m:
//   q = collision_candidate(x_new, u, w), the point the last local step's prox saw. The prox is a
//       hard projection, so at convergence x_new lies on the surface and the dual pushes q inside:
//       contact is decided on q;
//   contact query: collision_prox's walk on q (every rule unchanged), also returning the row r that
//       supplied the final (dx, point c); contact iff dx < 0;
//   n = (c - q) / |c - q|; no contact when the length is 0;
//   j = k (-u.n) for u.n < 0, else 0, k = p dt^2 w / m: the length dt^2 f_n / m, f_n the term's
//       force on the node in the step's optimality condition M (x - xbar) = -p dt^2 D^T u, D = w I;
//   g = the obstacle's displacement at c between its state during the previous step and now:
//       the floor's height or the shape's centre for an analytic row, c - (R_prev c_l + t_prev)
//       with c_l = c in the obstacle frame now for a mesh (position form, so a node stuck to a
//       turning obstacle does not drift along the tangent); 0 for a mesh whose vertices changed or
//       that is bound, unless it carries (the carry form below);
//   rel = (x_new - x_old) - g, rt its part tangential to n, lt = |rt|;
//   s = 0 if mu_r == 0, j == 0 or !(lt > 0), else min(1, mu_r j / lt); x_new -= s rt, written only
//       when s != 0. s = 1 is static friction (no slip relative to the obstacle), s < 1 kinetic.
// A term on a pinned node is reported but never filtered. The finalize pass then forms
// v = (x' - x_old) / dt as before, so position and velocity stay consistent.
#pragma once
#include <hip/hip_runtime.h>

#include "elastic_kernels.hpp"

namespace aa {

// One record per collision term, kept on the device ([count] and [count][3])
struct ContactRecDev {
    int* hit;
    int* row;
    double* c;
    double* n;
    double* j;
    double* rt;
    double* s;
};
// The contact features the carry form writes beside the record ([count] and [count][3]): the
// caller's triangle index (-1 for an analytic row) and the barycentric weights of c_l on it. Kept
// beside ContactRecDev, not in it: the plain kernel takes that struct by value before rec_off, so
// growing it would move the plain kernel's arguments.
struct ContactFeatDev {
    int* tri;
    double* b;
};
// g: a collision group (kCollision). xold: the step's start state (all nodes); xsrc: the free nodes'
// new positions, the buffer the finalize pass reads (moved in place); xfull: the pinned nodes'.
// rec_off: the group's first record.
void launch_contact_friction(const GroupDev& g, const double* xold, double* xsrc, const double* xfull, const double* u,
                             const double* mass, int nf, double penalty, double dt, const MeshObsDev* meshes,
                             const FrictionTables& T, const ContactRecDev& rec, int rec_off, hipStream_t s);

// aa_test_contact_friction: the device function on n queries (node[e] the exemption id, pinned[e]
// non-zero = reported only); xnew is moved in place
void launch_test_contact_friction(const double* obs, const MeshObsDev* meshes, const FrictionTables& T, const int* node,
                                  const unsigned char* pinned, const double* xold, double* xnew, const double* u,
                                  const double* w, const double* m, double penalty, double dt, int n,
                                  const ContactRecDev& rec, hipStream_t s);

// Carry form (aa_elastic_set_mesh_obstacle_carry): a mesh whose row of `carry` is set moves the
// nodes on it with its vertices' own motion since the previous step's pass, interpolated on the
// contact triangle:
//   A, B, C = the corners of the leaf triangle the walk found, A-, B-, C- the same vertices in the
//   mesh's previous vertex buffer; b = the barycentric weights of c_l on A, B, C (Cramer's rule on
//   the edge Gram matrix, (1, 0, 0) when !(den > 0));
//   g_l = (b0 (A - A-) + b1 (B - B-)) + b2 (C - C-), p_l = c_l - g_l, g = c - ((R_prev p_l) + t_prev).
// The displacement form: with unchanged vertices g_l is an exact zero and g the rigid one bit for
// bit, and the interpolation is continuous across shared edges and vertices. Such a mesh is never
// "still"; every other row follows the plain rule. The features are written for every mesh-row
// contact. Launched only when some mesh carries: otherwise the plain kernels above run as before.
void launch_contact_friction_carry(const GroupDev& g, const double* xold, double* xsrc, const double* xfull, const double* u,
                                   const double* mass, int nf, double penalty, double dt, const MeshObsDev* meshes,
                                   const FrictionTables& T, const ContactRecDev& rec, int rec_off, const MeshCarryDev* carry,
                                   const ContactFeatDev& feat, hipStream_t s);
void launch_test_contact_friction_carry(const double* obs, const MeshObsDev* meshes, const FrictionTables& T, const int* node,
                                        const unsigned char* pinned, const double* xold, double* xnew, const double* u,
                                        const double* w, const double* m, double penalty, double dt, int n,
                                        const ContactRecDev& rec, const MeshCarryDev* carry, const ContactFeatDev& feat,
                                        hipStream_t s);

}  // namespace aa
