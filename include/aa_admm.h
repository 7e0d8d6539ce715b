/* aa_admm.h -- C ABI of the MI355X-native Anderson-accelerated ADMM hot path.
 *
 * This is the drop-in boundary for the reference's admm-elastic plugin API
 * (bldeng/AA-ADMM, admm_anderson_{xzu,hard_zxu}/src). Plain pointers and sizes only; no
 * torch or HIP types. Every call returns AA_OK (0) or a negative status; the message of the
 * last failure on the calling thread is available from aa_last_error(). The reference
 * throws std::runtime_error / returns bool at the same points -- the C++ facade in
 * include/aa_admm.hpp re-raises these codes as std::runtime_error.
 *
 * Arrays are fp64 (the reference computes in double throughout, Types.h) and int32 indices
 * (Eigen's default StorageIndex). Node arrays are xyz-interleaved ("scaled x3" as in
 * Solver::m_x / m_masses, admm_anderson_hard_zxu/src/Solver.hpp:84-87).
 */
#ifndef AA_ADMM_H
#define AA_ADMM_H
#ifdef __cplusplus
extern "C" {
#endif

#define AA_OK 0
#define AA_ERR_ARG -1       /* bad input (reference: "Bad input" runtime_error)            */
#define AA_ERR_STATE -2     /* call order violated (e.g. step before initialize)           */
#define AA_ERR_DEVICE -3    /* HIP runtime failure                                         */
#define AA_ERR_NUMERIC -4   /* inverted element, weight <= 0, matrix not SPD              */

typedef struct aa_ctx_s* aa_ctx;          /* one GPU + one HIP stream                    */
typedef struct aa_elastic_s* aa_elastic;  /* one admm::Solver instance                   */

/* Element materials (binding::MeshFlags, samples/utils/AddMeshes.hpp:45-50). */
#define AA_LINEAR 0      /* TetEnergyTerm (corotated-linear via 3x3 SVD) / TriEnergyTerm */
#define AA_NEOHOOKEAN 1  /* NeoHookeanTet (9-D L-BFGS prox)                              */
#define AA_STVK 2        /* StVKTet       (9-D L-BFGS prox)                              */

/* Solver variants: the two reference solver copies. */
#define AA_VARIANT_Z 0   /* admm_anderson_xzu: Anderson on z (Solver.cpp:34-263)            */
#define AA_VARIANT_UX 1  /* admm_anderson_hard_zxu: Anderson on (u,x) (Solver.cpp:34-234)    */

/* Lame (EnergyTerm.hpp:35-61): mu, lambda and strain limits (tris only). */
typedef struct {
    double mu, lambda;
    double limit_min, limit_max;   /* defaults -100 / 100 = no limiting */
} aa_lame;

/* Solver::Settings (Solver.hpp:45-67) + variant selection. */
typedef struct {
    double timestep_s;      /* -dt   default 1/30                                  */
    int verbose;            /* -v                                                  */
    int admm_iters;         /* -it   default 500                                   */
    double gravity;         /* -g    default -9.8 (applied to y of free nodes)     */
    double constraint_w;    /* -ck   (unused by the LDLT path, kept for parity)    */
    int anderson_m;         /* -am   window (>0 with acceleration)                 */
    double penalty;         /* -ap   (UX variant; the Z variant uses 1)            */
    int acceleration_type;  /* 0 = NOACC, 1 = ANDERSON  (-a)                       */
    int variant;            /* AA_VARIANT_Z / AA_VARIANT_UX                        */
    double eps_rel;         /* run-to-epsilon (new, not in the reference): > 0 ends a
                               step once comb <= eps_rel * comb of its first iteration;
                               0 = the reference's loop (admm_iters, comb < 1e-20 break) */
} aa_settings;

/* RuntimeData (Solver.hpp:69-80) plus device-side counters. */
typedef struct {
    double global_ms, local_ms, acceleration_ms, initialization_ms;  /* host wall, per step */
    double step_ms;          /* wall time of the last step() (device-synchronised)  */
    double setup_ms;         /* initialize(): assembly + ordering + factorisation   */
    int iterations;          /* ADMM iterations executed in the last step (incl. a  
                                breaking one; history() holds the recorded rows)     */
    int rejects;             /* Anderson rejections in the last step                */
    long long nnz_factor;    /* scalar nnz(L) of the global factor                  */
    int n_free, n_pinned, n_elements, z_dim;
} aa_runtime;

const char* aa_last_error(void);
const char* aa_version(void);

/* ---- context --------------------------------------------------------------------- */
int aa_ctx_create(int device_id, aa_ctx* out);
int aa_ctx_destroy(aa_ctx ctx);
int aa_ctx_synchronize(aa_ctx ctx);
/* Measurement hook (no reference counterpart): GB/s of a 16-B-per-lane streaming read of `bytes`
 * on the context's stream -- the measured HBM read ceiling bench.py reports beside the spec. */
int aa_ctx_bench_read(aa_ctx ctx, long long bytes, double* gbps);
/* One-time library load, made explicit (no reference counterpart): the first rocBLAS / rocSOLVER
 * calls of a process load their code objects (seconds on a fresh box with a cold page cache),
 * which would otherwise land inside the first aa_elastic_initialize / aa_geom_setup that factors
 * a front on the GPU (SolverCommon / Solver.cpp:414-482 factor step). Runs the dense-front
 * backend once on a synthetic front of the smallest GPU order; *ms = its wall time (0 when
 * already warm or AA_DENSE_GPU=0). */
int aa_ctx_warm_dense(aa_ctx ctx, double* ms);

/* ---- admm::Solver ------------------------------------------------------------------ */
int aa_lame_from_young(double youngs, double poisson, aa_lame* out);    /* Lame(k, v)        */
int aa_settings_default(aa_settings* out);                               /* Settings()        */

int aa_elastic_create(aa_ctx ctx, aa_elastic* out);                      /* Solver()          */
int aa_elastic_destroy(aa_elastic h);
/* Solver::add_nodes(x, m, n): x and m are "scaled x3"; returns the node count in *total. */
int aa_elastic_add_nodes(aa_elastic h, const double* x3, const double* m3, int n_verts, int* total);
/* create_tets_from_mesh<IN_SCALAR,TYPE>(energyterms, verts, inds, n, lame, vertex_offset)
 * (TetEnergyTerm.hpp:36-51): rest shape from verts3[inds], node ids inds + vertex_offset. */
int aa_elastic_add_tets(aa_elastic h, const double* verts3, const int* tets4, int n_tets, int material,
                        const aa_lame* lame, int vertex_offset);
/* create_tris_from_mesh<IN_SCALAR,TriEnergyTerm> (TriEnergyTerm.hpp:33-47). */
int aa_elastic_add_tris(aa_elastic h, const double* verts3, const int* tris3, int n_tris, const aa_lame* lame,
                        int vertex_offset);
/* Per-element materials: the reference builds one EnergyTerm per tet / triangle and each term owns
 * its Lame (TetEnergyTerm.hpp:36-51, TriEnergyTerm.hpp:33-47), so a caller may loop over the elements
 * with a stiffness that varies in space. These calls take that loop as one group (one launch per kernel
 * class, one work queue): the semantics of n create_*_from_mesh calls of one element each, in element
 * order, with lame_per_*[e]. `material` stays per call; mu and lambda (and, for triangles, the strain
 * limits) vary. The scalar calls' errors apply per element with the same codes and messages, which
 * also name the first offending element; a null array with n > 0 or a non-finite mu / lambda is
 * AA_ERR_ARG. */
int aa_elastic_add_tets_var(aa_elastic h, const double* verts3, const int* tets4, int n_tets, int material,
                            const aa_lame* lame_per_tet /* [n_tets] */, int vertex_offset);
int aa_elastic_add_tris_var(aa_elastic h, const double* verts3, const int* tris3, int n_tris,
                            const aa_lame* lame_per_tri /* [n_tris] */, int vertex_offset);
/* Bending (no counterpart in the reference, whose cloth is a pure membrane): one hinge per interior
 * edge of the triangle list, i.e. an edge shared by exactly two triangles; boundary edges make none.
 * Hinge vertices (x0, x1, x2, x3): x0 < x1 the edge's endpoints, x2 the opposite vertex in the
 * triangle with the lower index, x3 the other. With cot(p; a, b) = ((a-p).(b-p)) / |(a-p)x(b-p)| on
 * the rest positions, a0 = cot(x0; x1, x2), a1 = cot(x1; x0, x2), b0 = cot(x0; x1, x3), b1 =
 * cot(x1; x0, x3), the reduction row is K = (a1 + b1, a0 + b0, -(a0 + a1), -(b0 + b1)) and z = K x in
 * R^3. Energy 1/2 kappa (|z| - r)^2, kappa = 3 k_bend / (sum of the two rest areas); flat_rest != 0:
 * r = 0 (the quadratic isometric bending model of Bergou et al. 2006), else r = |K xbar| of the rest
 * shape, so that a curved rest shape is an equilibrium. ADMM weight sqrt(kappa). Rest shape from
 * verts3[tris3], node ids tris3 + vertex_offset; *n_hinges (optional) receives the hinge count, 0 for
 * a list without an interior edge. Before initialize only (AA_ERR_STATE after). AA_ERR_ARG naming the
 * first offending element: an index out of range, a non-finite vertex, k_bend not finite or not > 0,
 * an edge in more than two triangles, two triangles running along their shared edge in the same
 * direction; AA_ERR_NUMERIC: a zero-area triangle. initialize refuses a solver with hinges in
 * AA_VARIANT_Z and one partitioned over more than one rank. */
int aa_elastic_add_bending(aa_elastic h, const double* verts3, const int* tris3, int n_tris, double k_bend,
                           int flat_rest, int vertex_offset, int* n_hinges);
/* Springs, tethers and struts (no counterpart in the reference, whose SpringPin is an infinitely hard
 * spring on one node): spring e joins nodes a != b = pairs2[2e], pairs2[2e + 1] (+ vertex_offset).
 * Its reduction row is (-1, +1), so z = x_b - x_a in R^3: two vertices, one column. Rest length
 * L = rest[e] >= 0 (rest == NULL: |verts3[b] - verts3[a]|) and stiffness k[e] > 0 per spring; ADMM
 * weight sqrt(k). One mode per call (one group per call). With n = |v| = sqrt((v0^2 + v1^2) + v2^2)
 * the prox z = argmin U(z) + 1/2 k |z - v|^2 is z = s v:
 *   AA_SPRING          U = 1/2 k (|z| - L)^2          s = 1/2 + 1/2 (L / n)
 *   AA_SPRING_TETHER   U = 1/2 k max(0, |z| - L)^2    n <= L: z = v bitwise; else as AA_SPRING
 *   AA_SPRING_STRUT    U = 1/2 k max(0, L - |z|)^2    n >= L: z = v bitwise; else as AA_SPRING
 *   ... | AA_SPRING_HARD   U the indicator of |z| = L / |z| <= L / |z| >= L, k sets the weight only:
 *                          s = L / n where the soft form would act, z = v bitwise elsewhere
 * n = 0 has no direction: z = v in every mode (stated, not derived). L = 0 is allowed: a zero-length
 * spring is a stitch, its hard two-sided form a weld. Parallel springs on one pair are allowed. An
 * endpoint may be pinned; a pinned endpoint moved by aa_elastic_set_pins every step is a soft
 * attachment. Before initialize only (AA_ERR_STATE after). AA_ERR_ARG naming the first offending
 * spring: an index out of range, a == b, k not finite or not > 0, rest negative or not finite; also
 * an unknown mode, a null array with n_springs > 0, rest == NULL together with verts3 == NULL. A
 * refused call changes nothing. initialize refuses a solver with springs in AA_VARIANT_Z and one
 * partitioned over more than one rank. */
enum { AA_SPRING = 0, AA_SPRING_TETHER = 1, AA_SPRING_STRUT = 2, AA_SPRING_HARD = 4 };
int aa_elastic_add_springs(aa_elastic h, const double* verts3, const int* pairs2, int n_springs, int mode,
                           const double* k /* [n] */, const double* rest /* [n] or NULL */, int vertex_offset);
/* Ties: springs between barycentric anchors (no counterpart in the reference). Tie e joins anchor
 * A = sum_i a_i x_{A_i}, A_i = nodes_a[na e + i], a_i = w_a[na e + i], to anchor B = sum_j b_j x_{B_j}
 * alike (node ids + vertex_offset): a node (1), a point on an edge (2), in a triangle (3) or in a tet
 * (4), with 1 <= na, nb <= 4 and 3 <= na + nb <= 6. Its reduction row over the vertices (A_0 ..
 * A_{na-1}, B_0 .. B_{nb-1}) is (-a_0 .. -a_{na-1}, +b_0 .. +b_{nb-1}), so z = p_B - p_A in R^3:
 * na + nb vertices, one column, formed as the sum over the vertices in that order, left to right
 * from 0, each term one fused multiply-add. The row sums to zero: a tie is an internal force. Rest
 * length L = rest[e] >= 0, stiffness k[e] > 0, ADMM weight sqrt(k), one mode per call (one group per
 * call); k, rest, mode and the prox are those of aa_elastic_add_springs, every mode included.
 * rest == NULL: L = |p_B - p_A| at verts3, each anchor coordinate summed left to right from its
 * first term, p = ((w_0 x_0 + w_1 x_1) + w_2 x_2) + w_3 x_3, d = p_B - p_A,
 * L = sqrt((d0 d0 + d1 d1) + d2 d2), nothing contracted.
 * Weights: finite, each side |sum w - 1| <= 1e-12, used as given (no renormalisation); a weight
 * outside [0, 1] (an extrapolated anchor) or equal to zero is allowed. No node may appear twice in
 * one tie, within an anchor or across the two. The anchors are fixed: they do not slide.
 * Before initialize only (AA_ERR_STATE after). AA_ERR_ARG naming the first offending tie: an index
 * out of range, a node twice, a weight not finite, a side not summing to 1, k not finite or not > 0,
 * rest negative or not finite; also an unknown mode, na or nb outside 1..4, na + nb = 2 (use
 * aa_elastic_add_springs), na + nb = 7 or 8 (triangle-tet, tet-tet: not provided), a null array with
 * n_ties > 0, rest == NULL together with verts3 == NULL. A refused call changes nothing. initialize
 * refuses a solver with ties in AA_VARIANT_Z and one partitioned over more than one rank. */
int aa_elastic_add_ties(aa_elastic h, const double* verts3, int na, const int* nodes_a /* [n][na] */,
                        const double* w_a /* [n][na] */, int nb, const int* nodes_b /* [n][nb] */,
                        const double* w_b /* [n][nb] */, int n_ties, int mode, const double* k /* [n] */,
                        const double* rest /* [n] or NULL */, int vertex_offset);
/* Where on a triangle list does a point land (to find a tie's anchor)? For each of the n queries
 * q3: the closest point of the surface, the caller's index of the triangle it lies on and its
 * barycentric weights on that triangle's corners (Cramer's rule on the edge Gram matrix; (1, 0, 0)
 * for a triangle whose Gram determinant is not > 0). Any triangle list: open and non-manifold ones
 * are fine, no orientation is needed. The host builds a BVH; one kernel, one lane per query, runs the
 * exact closest-point walk from a cold start, so the closest point is the exact minimum over all
 * triangles; among triangles at the same distance the walk's first found wins (the leaf its greedy
 * descent reaches, then depth-first order, strictly smaller distances replacing). AA_ERR_ARG for a
 * non-finite coordinate (vertex or query), an index out of range, a zero-area triangle, an empty
 * list. Not the mesh-obstacle path: nothing is added to a solver. closest3, tri or bary3 may be NULL. */
int aa_closest_on_triangles(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                            const double* q3, int n, double* closest3, int* tri, double* bary3);
/* Solver::set_pins(inds, points): points3 == NULL pins in place (Solver.cpp:280-315). */
int aa_elastic_set_pins(aa_elastic h, const int* inds, const double* points3, int n_pins);

/* Passive obstacles (admm_anderson_hard_zxu/src/PassiveObject.hpp:32-136), Solver::add_obstacle
 * (Solver.cpp:346-348). params: FLOOR {y}; SLIDE_FLOOR {cx,cy,cz, nx,ny,nz} (the normal is
 * normalised, as the SlideFloor constructor does); SPHERE / PLANE_HALF_SPHERE / CYLINDER
 * {cx,cy,cz, r} (the cylinder's axis is z). The collision terms test every obstacle in insertion
 * order each iteration; obstacles may be added after initialize. The z-AA variant rejects
 * obstacles at initialize (admm_anderson_xzu/src/Solver.cpp:485-489). The mesh obstacle
 * (PassiveMesh) has its own call, aa_elastic_add_mesh_obstacle below; AA_OBS_MESH names its type
 * in obstacle rows and is an "unknown obstacle type" error here. */
#define AA_OBS_FLOOR 0
#define AA_OBS_SLIDE_FLOOR 1
#define AA_OBS_SPHERE 2
#define AA_OBS_PLANE_HALF_SPHERE 3
#define AA_OBS_CYLINDER 4
#define AA_OBS_MESH 5
int aa_elastic_add_obstacle(aa_elastic h, int type, const double* params);
/* PassiveMesh (PassiveObject.hpp:138-178): a collision node inside the mesh moves to the nearest
 * surface point. The obstacle is a closed, edge-manifold, outward-oriented triangle surface
 * (verts3: 3 n_verts doubles, tris3: 3 n_tris vertex indices). For a candidate q, the closest
 * surface point c and its triangle are those of the exact fp64 closest-point walk of the
 * reference-surface constraints (same arithmetic, same tie rule); q is inside iff (q - c) . n < 0
 * for the angle-weighted pseudonormal n of the feature c lies on (face: the unit face normal; edge:
 * the sum of the two incident unit face normals; vertex: the sum over incident faces of incident
 * angle x unit face normal). Inside: dx = -|q - c|, point = c, and -- the reference's rule, whose
 * PassiveMesh::signed_distance has no `if (dx > p.dx) return;` -- the hit replaces the running
 * (dx, point) of the obstacles before it unconditionally; obstacles after it compete with their
 * own test. Not inside: the running payload is left untouched. The obstacle takes its place in
 * the insertion order shared with aa_elastic_add_obstacle, may be added after initialize (the
 * step graph is captured again at the next step when it is the first mesh), and is refused by the
 * z-AA variant at initialize like the analytic ones. *id (optional) receives the mesh's number.
 * Deviations from the reference, stated: fp64 instead of float, and the boundary surface instead
 * of point-in-any-tet of a tet mesh (for a solid tet mesh the inside set is the same; pass its
 * boundary faces). Capacity: AA_MAX_MESH_OBSTACLES meshes per solver (they also count toward the
 * 256 obstacles in all); one more is AA_ERR_ARG. AA_ERR_ARG with a message naming the first
 * offending vertex, triangle or edge for: a non-finite coordinate, an index out of range, a
 * zero-area triangle, an edge not in exactly two faces of opposite directions (open, non-manifold
 * or inconsistently oriented surfaces), a signed volume that is not positive (inward faces). */
#define AA_MAX_MESH_OBSTACLES 16
int aa_elastic_add_mesh_obstacle(aa_elastic h, const double* verts3, int n_verts, const int* tris3, int n_tris, int* id);
/* Kinematic obstacles: a rigid pose per mesh obstacle, changed as often as every step at the cost
 * of one table row (no re-validation, no BVH work, no new mesh row). pose12 = R (row-major 3x3,
 * obstacle frame -> world) then t: the surface the collision terms see is R v + t for the vertices
 * v given to aa_elastic_add_mesh_obstacle, which stay as uploaded. NULL = back to unposed. The
 * candidate q is taken into the obstacle frame, tested there by the unchanged walk, and the closest
 * point taken back, in this fixed operation order (no FMA contraction):
 *   d = q - t;  q_l[i] = (R[0][i] d0 + R[1][i] d1) + R[2][i] d2;
 *   root-box cull, closest point c_l, pseudonormal sign and dx = -|q_l - c_l| on q_l;
 *   c_w[i] = ((R[i][0] c0 + R[i][1] c1) + R[i][2] c2) + t[i].
 * A mesh that never had a pose set takes exactly the unposed arithmetic. May be called before or
 * after initialize and between steps; it writes the mesh's row of the device table on the solver's
 * stream and keeps the captured step graph. The pose holds for every ADMM iteration of every later
 * step until changed. The obstacle is kinematic; it exerts friction, and carries the nodes on it
 * along, only through aa_elastic_set_obstacle_friction (below). A node it overruns is moved to its
 * surface by the next step's prox. R is used as given (no
 * re-orthonormalisation). AA_ERR_ARG, the message naming the cause: an unknown mesh_id, a
 * non-finite entry, max|R^T R - I| > 1e-12, det R <= 0 (a reflection would turn the surface
 * inside out). Partitioned solvers: every rank makes the same call, as for add_obstacle.
 * aa_elastic_get_mesh_obstacle_pose returns the pose in force (identity when unposed) and whether
 * one is set; either output may be NULL. */
int aa_elastic_set_mesh_obstacle_pose(aa_elastic h, int mesh_id, const double pose12[12]);
int aa_elastic_get_mesh_obstacle_pose(aa_elastic h, int mesh_id, double pose12[12], int* posed);
/* Deforming obstacles: new vertex positions for mesh obstacle mesh_id -- 3 n_verts doubles, the
 * vertex count and the triangles of aa_elastic_add_mesh_obstacle, in the obstacle frame (a pose set
 * for the mesh still applies on top). Changed as often as every step without a host BVH build and
 * without a new obstacle or mesh row: the topology is not validated again and the BVH is not
 * rebuilt -- the tree keeps its node order, its leaf contents and its stored axes -- but refitted on
 * the device to the new positions V', in this order:
 *   leaf triangles: the corners read from V' in the build's leaf and corner order;
 *   pseudonormals: the formulas of aa_elastic_add_mesh_obstacle on V' (unit face normals, clamped
 *     acos corner angles), a vertex's terms added in increasing triangle index from 0, an edge's
 *     value (0 + n[t_lo]) + n[t_hi];
 *   node bounds: per node the box of the vertices of its triangles and the ranges of
 *     s = (a0 P0 + a1 P1) + a2 P2 (fp64, no FMA contraction) along its three stored axes a, each
 *     rounded outward to fp32; a range stored as unbounded stays so;
 *   the row's fp64 root box: the exact range of the referenced vertices.
 * The closest-point walk is exact for any conservative bounds, so the answers are those of a mesh
 * freshly added with V' (bit for bit where the closest triangle is unique); only the walk's cost
 * grows as the shape leaves the one the tree was built for. Measured on a 200 k triangle torus
 * (DESIGN.md section 3.7): the refit takes 0.47 ms where preparing and uploading the mesh anew
 * takes 300 ms on the host; the walk on the refitted tree costs what the fresh tree's costs for an
 * unchanged shape, 2.2 times that after a twist, bend and stretch that moves vertices by up to 15 %
 * of the torus' diameter, and 4.8 times after one that moves them by up to 31 %. More than twice the fresh
 * walk is the point where a caller should add the new shape as a new mesh (a host build and a new
 * row) rather than go on refitting -- shapes that stay near the added one, a breathing or
 * flexing body, are far from it. May be called before
 * or after initialize and between steps; the work runs on the solver's stream and is finished when
 * the call returns; every device buffer and the mesh's table row keep their addresses, so the
 * captured step graph is kept. The vertices hold for every ADMM iteration of every later step until
 * changed. The obstacle stays kinematic; the friction pass (aa_elastic_set_obstacle_friction) takes
 * no displacement from a change of shape unless the mesh carries (aa_elastic_set_mesh_obstacle_carry). Validation
 * happens on the host before anything on the device is touched, and a refused call leaves the
 * obstacle exactly as it was. AA_ERR_ARG, the message naming the cause: an unknown mesh_id, a null
 * pointer, a non-finite coordinate (the vertex named), a zero-area triangle (named; the test of
 * aa_elastic_add_mesh_obstacle), a signed volume that is not positive. Partitioned solvers: every
 * rank makes the same call, as for the pose.
 * aa_elastic_get_mesh_obstacle_vertices returns the vertices in force (verts3 may be NULL) and
 * their count (n_verts may be NULL). */
int aa_elastic_set_mesh_obstacle_vertices(aa_elastic h, int mesh_id, const double* verts3);
int aa_elastic_get_mesh_obstacle_vertices(aa_elastic h, int mesh_id, double* verts3, int* n_verts);
/* Bound obstacles: the obstacle is another simulated body. Vertex i of mesh obstacle mesh_id follows
 * solver node nodes[i] (the caller's numbering; any node, pinned ones included; n_verts = the mesh's
 * vertex count). nodes = NULL unbinds; the shape last in force stays. May be called before or after
 * initialize and between steps. From then on every aa_elastic_step begins -- before wind, before
 * the first local step -- by gathering the mesh's vertices on the device from the step's start
 * positions and running the refit of aa_elastic_set_mesh_obstacle_vertices on them, on the solver's
 * stream: no host copy, no wait. That work precedes the captured iteration graph, so binding and
 * unbinding keep the graph.
 * Coupling: the obstacle holds its start-of-step shape for every ADMM iteration of that step --
 * lagged, explicit coupling. The friction pass (aa_elastic_set_obstacle_friction) treats its surface
 * as standing still unless the mesh carries (aa_elastic_set_mesh_obstacle_carry: the surface then
 * drags the nodes on it with the body's displacement over the previous step) and applies no
 * reaction to its nodes, and it is refitted once per step, not more often. The BVH is not rebuilt when the shape drifts far from the added one: the
 * cost growth stated above for the vertex setter applies alike.
 * Validity is decided on the device, because the host never sees the gathered shape. The causes
 * are the vertex setter's, tested in this order, the lowest-numbered one reported:
 *   1  a non-finite gathered coordinate;
 *   2  a triangle with !(n . n > 0), n = (B - A) x (C - A);
 *   3  !(vol6 > 0), vol6 = the sum of A . (B x C) in a fixed shape: the triangles in the caller's
 *      order in consecutive chunks of 256, a chunk's partial the pairwise tree p[i] += p[i + w],
 *      w = 128 .. 1 (absent triangles of the last chunk count 0), the partials added in chunk order.
 * When the check fails every refit kernel and the kernel that writes the row's root box exit at
 * once (gated on a device status word) and the obstacle stays exactly as it was after its last
 * good refit; aa_elastic_step does not fail. When it passes, the tables are what
 * aa_elastic_set_mesh_obstacle_vertices writes for the same positions, bit for bit, and the root
 * box is the exact range of the gathered vertices.
 * aa_elastic_mesh_obstacle_status (every output optional): whether the mesh is bound, the refits
 * taken and skipped since binding, and the cause (above; 0 = none) of the last skipped one; the
 * counts arrive with the step's other results. aa_elastic_get_mesh_obstacle_vertices returns the
 * vertices in force, after a skipped refit the earlier ones.
 * AA_ERR_ARG, the message naming the cause: an unknown mesh_id, n_verts not the mesh's vertex
 * count, a node index out of range, a mesh that has a pose, a solver partitioned over more than one
 * rank (a rank holds only its part of the nodes: partitioned binding is out of scope).
 * aa_elastic_set_mesh_obstacle_pose and aa_elastic_set_mesh_obstacle_vertices refuse a bound mesh.
 * Not provided: self-collision (see the exemption below), partitioned solvers, a reaction of the
 * contact on the body's nodes, more than one refit per step, a BVH rebuild on drift, and the z-AA variant, which
 * refuses collision terms as before. */
int aa_elastic_bind_mesh_obstacle(aa_elastic h, int mesh_id, const int* nodes, int n_verts);
int aa_elastic_mesh_obstacle_status(aa_elastic h, int mesh_id, int* bound, int* refits, int* skipped, int* last_cause);
/* Exemption: the collision terms of the n listed nodes (caller's numbering) skip mesh obstacle
 * mesh_id as if it were not in the obstacle list -- the running (dx, point) is left untouched and
 * later obstacles compete as before. The list replaces the earlier one; n = 0 clears it. Any mesh,
 * bound or not, before or after initialize, between steps; the captured graph is kept (one byte per
 * node on the device, reached from the mesh's table row). A body whose surface is a bound obstacle
 * exempts its own nodes, or its interior nodes would be projected out of their own surface.
 * A node is exempt from a whole mesh, not from its incident triangles only, so self-collision is
 * not provided. AA_ERR_ARG: an unknown mesh_id, a null list with n > 0, a node out of range. */
int aa_elastic_set_mesh_obstacle_exempt(aa_elastic h, int mesh_id, const int* nodes, int n);
/* The number of obstacle rows, analytic and mesh, in the shared insertion order. */
int aa_elastic_num_obstacles(aa_elastic h, int* n);
/* Re-parameterises the analytic obstacle at position `index` of that order (a rising floor, a
 * rolling sphere): parameter layout and SLIDE_FLOOR normalisation of aa_elastic_add_obstacle; the
 * new parameters hold from the next step on; before or after initialize; the step graph is kept.
 * `type` must equal the row's stored type (a guard against a stale index). AA_ERR_ARG for a mesh
 * row, a type mismatch, an index out of range, null or non-finite parameters. */
int aa_elastic_set_obstacle(aa_elastic h, int index, int type, const double* params);
/* Coulomb friction of the collision terms against the obstacles, moving ones included. mu is the
 * coefficient of obstacle row `index` of the shared insertion order, analytic and mesh alike
 * (default 0). May be set before or after initialize and between steps; the captured step graph is
 * kept, because friction is one pass per step after the ADMM iterations and before the new state is
 * formed, outside that graph. The pass runs in a step iff some row has mu > 0 or recording is on; a
 * solver that uses neither launches nothing new and computes bit for bit what it did.
 * The model, per collision term on a node of mass m (term weight w, penalty p, time step dt), on
 * the pair (u, x_new) the step writes back (with Anderson acceleration the un-accelerated pair of
 * the last iteration); fp64, no FMA contraction, sums left to right:
 *   1  q = (1/w) (w x_new + u), the point the last local step's prox saw. The prox is a hard
 *      projection, so a converged x_new lies on the surface and the dual pushes q inside: contact is
 *      decided on q.
 *   2  The obstacle walk of the collision prox on q, every rule unchanged (insertion order, a later
 *      analytic obstacle wins a tie, a mesh hit replaces unconditionally, exemptions, poses, the
 *      root-box cull). Contact iff the final dx < 0; r = the row that supplied it, c = its point.
 *   3  e = c - q, l = sqrt((e0^2 + e1^2) + e2^2), n = e / l; no contact if l == 0.
 *   4  un = (u0 n0 + u1 n1) + u2 n2, k = (((p dt) dt) w) / m, j = k (-un) if un < 0, else 0: the
 *      length dt^2 f_n / m for the term's normal force f_n on the node in the step's optimality
 *      condition M (x - xbar) = -p dt^2 D^T u, D = w I.
 *   5  g = the obstacle's displacement at c between its state during the previous step and now:
 *      FLOOR (0, y_now - y_prev, 0); the other analytic shapes centre_now - centre_prev (changes of
 *      normal or radius do not count); a mesh c - ((R_prev c_l) + t_prev) with c_l = c taken into
 *      the obstacle frame of the pose now (no pose = identity) -- the position form, not omega x c,
 *      so a node stuck to a turning obstacle does not drift along the tangent. g = 0 for a mesh
 *      whose vertices changed since the previous step (aa_elastic_set_mesh_obstacle_vertices) or
 *      that is bound to solver nodes. In the first step, and in the first step after a step in
 *      which the pass did not run, previous = now.
 *      A mesh that carries (aa_elastic_set_mesh_obstacle_carry, below) is never taken as standing
 *      still, whether bound, changed or neither; its g follows its vertices' own motion, with the
 *      leaf triangle tri the walk of step 2 found c on:
 *        c_l = c in the obstacle frame of the pose now, as above;
 *        A, B, C = the corners of tri now; A-, B-, C- = the same three vertices in the vertices in
 *        force during the previous step's pass;
 *        e1 = B - A, e2 = C - A, d = c_l - A; d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, p1 = d.e1,
 *        p2 = d.e2, every dot (a0 b0 + a1 b1) + a2 b2; den = d11 d22 - d12 d12;
 *        b1 = (d22 p1 - d12 p2) / den, b2 = (d11 p2 - d12 p1) / den, b0 = (1 - b1) - b2;
 *        b = (1, 0, 0) if !(den > 0);
 *        g_l = (b0 (A - A-) + b1 (B - B-)) + b2 (C - C-) componentwise, p_l = c_l - g_l,
 *        g = c - ((R_prev p_l) + t_prev).
 *      The displacement form, not a difference of interpolated positions: with unchanged vertices
 *      every corner difference is an exact zero, p_l = c_l and g is the rigid expression bit for
 *      bit; and the interpolation is continuous across shared edges and vertices, so which of two
 *      tying triangles the walk returns does not matter beyond rounding. The state "during the
 *      previous step" is the pose path's notion: for a vertex setter's mesh the vertices set before
 *      that step, for a bound mesh the body's start-of-step shape then -- so a bound mesh carries
 *      with the body's displacement over the previous step, lagged and explicit like the rest of
 *      that coupling, and a skipped refit leaves the vertices as they were (g_l = 0). Previous =
 *      now in the first step, after a step without the pass, and when carry was switched on since.
 *   6  rel = (x_new - x_old) - g, rn = (rel0 n0 + rel1 n1) + rel2 n2, rt = rel - rn n,
 *      lt = sqrt((rt0^2 + rt1^2) + rt2^2); s = 0 if mu_r == 0, j == 0 or !(lt > 0), else
 *      min(1, (mu_r j) / lt); x_new -= s rt, written only when s != 0.
 * The velocity is then (x_new' - x_old) / dt as always. s = 1: the node does not move along the
 * surface relative to the obstacle (static friction); s < 1: it loses mu j of slip (kinetic).
 * A collision term on a pinned node is reported but never filtered.
 * What it is not: the friction is lagged and explicit, applied once per step with the normal force
 * of the solve just finished -- it is not part of the ADMM iteration; there is no rolling or
 * anisotropic friction, and no reaction on a bound obstacle's nodes. A deforming or bound mesh's
 * own surface motion enters only for a mesh that carries; partitioned solvers and the z-AA variant
 * (which refuses collision terms) are not served.
 * aa_elastic_record_contacts(on) keeps the pass running for its records even with every mu = 0.
 * aa_elastic_get_contacts returns the last step's terms in contact, in collision-term order: *n
 * their full count, at most cap entries in each given array (every array may be NULL) -- the node
 * (caller's numbering), the obstacle row r, the point c, the normal n, the push j, the slip rt
 * and the scale s. n = 0 when the pass did not run in the last step.
 * AA_ERR_ARG, the message naming the cause: an index out of range, a negative or non-finite mu, a
 * null mu or n output, and mu > 0 or recording on in a solver partitioned over more than one rank
 * (a rank holds only its part of the terms), raised by the setter after initialize and by
 * aa_elastic_initialize otherwise. */
int aa_elastic_set_obstacle_friction(aa_elastic h, int index, double mu);
int aa_elastic_get_obstacle_friction(aa_elastic h, int index, double* mu);
int aa_elastic_record_contacts(aa_elastic h, int on);
int aa_elastic_get_contacts(aa_elastic h, int cap, int* n, int* node, int* obstacle, double* point3, double* normal3,
                            double* push, double* slip3, double* scale);
/* Carry, per mesh obstacle, default off: the friction pass takes the mesh's displacement at a
 * contact from its vertices' own motion (step 5 above), so a surface moved through
 * aa_elastic_set_mesh_obstacle_vertices or bound to solver nodes drags the nodes on it as one moved
 * through its pose does. May be switched before or after initialize and between steps; the captured
 * step graph is kept, because the pass is outside it. A mesh with carry off behaves exactly as
 * before, and a solver in which no mesh carries launches the pass it always launched and computes
 * bit for bit what it did; with some mesh carrying, the pass runs in its carry form for every row.
 * The previous vertices are one more device buffer per carrying mesh, refreshed by a device-to-
 * device copy on the solver's stream after the pass: no host copy, no wait.
 * aa_elastic_get_contact_features returns, in the order of aa_elastic_get_contacts, the triangle
 * (the caller's index; -1 for an analytic row) and the barycentric weights b of step 5 for the
 * last step's contacts, filled for every mesh-row contact, carrying mesh or not: *n their count, at
 * most cap entries per array (either may be NULL); *n = 0 when the last step's pass was not the
 * carry form.
 * AA_ERR_ARG: an unknown mesh_id, a null output (on, n), and switching on after initialize in a
 * solver partitioned over more than one rank. */
int aa_elastic_set_mesh_obstacle_carry(aa_elastic h, int mesh_id, int on);
int aa_elastic_get_mesh_obstacle_carry(aa_elastic h, int mesh_id, int* on);
int aa_elastic_get_contact_features(aa_elastic h, int cap, int* n, int* tri, double* bary3);
/* Solver::set_collisions(inds, points) (admm_anderson_hard_zxu/src/Solver.cpp:318-344): one
 * Collision energy term (CollisionEnergyTerm.hpp:41-117: identity reduction, weight
 * sqrt(2 k(soft rubber)), prox = closest obstacle surface point when inside one) per listed node,
 * created at initialize after the other terms in node order. The reference's points are never read
 * by the prox and are not taken here. (u,x) variant only; after initialize it changes nothing. */
int aa_elastic_set_collisions(aa_elastic h, const int* inds, int n);
/* WindForce (ExplicitForce.hpp:39-47, ExplicitForce.cpp:47-104) pushed to Solver::ext_forces:
 * every step, before gravity, v += 0.33 dt f_n on the vertices of each listed triangle (the
 * Wejchert-Haumann normal force of the relative velocity v - dir), triangles in the given order
 * (the reference's loop run on one thread). *id names it for aa_elastic_set_wind. */
int aa_elastic_add_wind(aa_elastic h, const int* tris3, int n_tris, const double dir3[3], int* id);
int aa_elastic_set_wind(aa_elastic h, int id, const double dir3[3]);   /* WindForce::direction */
int aa_elastic_initialize(aa_elastic h, const aa_settings* settings);    /* Solver::initialize */
int aa_elastic_step(aa_elastic h);                                       /* Solver::step       */
int aa_elastic_num_nodes(aa_elastic h, int* n);
int aa_elastic_get_x(aa_elastic h, double* x3);                          /* Solver::m_x        */
int aa_elastic_get_v(aa_elastic h, double* v3);                          /* Solver::m_v        */
int aa_elastic_set_v(aa_elastic h, const double* v3);
int aa_elastic_set_x(aa_elastic h, const double* x3);                    /* Solver::m_x = x   */
/* Per-iteration (prim, comb, reject) of the last step -- the rows Solver::save() writes
 * (Solver.hpp:130-155). Returns the count in *n (<= cap copied). */
int aa_elastic_get_history(aa_elastic h, double* prim, double* comb, int* reject, int cap, int* n);
/* Change Settings::admm_iters / eps_rel of later steps without re-initialising (no refactor). */
int aa_elastic_set_iterations(aa_elastic h, int admm_iters, double eps_rel);
/* Device-clock time (ms) from the start of the last step() to the end of each recorded
 * iteration (the reference's per-iteration elapsed times; time-to-epsilon). */
int aa_elastic_get_times(aa_elastic h, double* time_ms, int cap, int* n);
int aa_elastic_runtime(aa_elastic h, aa_runtime* out);                   /* runtime_data()    */

/* ---- multi-GPU: mesh partitioned over the GPUs of one node -----------
 * The reference is one OpenMP process (no MPI/NCCL); this is new surface. One process per GPU;
 * every rank builds the SAME scene through the calls above, attaches a communicator, then
 * initialize() partitions the free nodes by nested dissection into `size` parts (any count
 * >= 1: an odd count is split floor/ceil by vertex count at each forced bisection) plus the
 * shared separator rows, and each rank keeps the elements of its part. step()
 * runs the identical reference iteration on all ranks (all-reduced residuals, Anderson dot
 * products and separator rows of the global solve); afterwards every rank holds the full
 * x and v. */
typedef struct aa_comm_s* aa_comm;
/* Host transport callback: in-place SUM of n doubles over all ranks; return 0 on success. */
typedef int (*aa_host_allreduce_fn)(double* buf, long long n, void* user);
/* Which ROCm runtime this process is bound to (no reference counterpart): "name=path\n" for the
 * objects defining hipMalloc, hsa_init, rocblas_create_handle, rocsolver_dpotrf and ncclAllReduce
 * (librccl is loaded from the HIP runtime's directory first). Needs no GPU. A process that loaded
 * another ROCm build's libamdhip64 before this library (e.g. a framework's bundled runtime) shows
 * it here; the multi-rank launchers check it. Copies at most cap-1 bytes; *len = full length. */
int aa_runtime_libraries(char* buf, long long cap, long long* len);
/* ncclGetUniqueId: called on rank 0, the 128 bytes are broadcast by the caller. */
int aa_comm_unique_id(unsigned char id[128]);
/* RCCL communicator over xGMI on ctx's GPU (ncclCommInitRank; collective over all ranks). */
int aa_comm_create_rccl(aa_ctx ctx, const unsigned char id[128], int rank, int size, aa_comm* out);
/* Host-staged transport through a caller callback (e.g. torch.distributed/gloo); lets several
 * ranks share one GPU (tests). Never captured into a hipGraph. */
int aa_comm_create_host(aa_host_allreduce_fn fn, void* user, int rank, int size, aa_comm* out);
/* Timing rehearsal (no reference counterpart): rank `rank` of a `size`-way partition alone on
 * its GPU -- device all-reduces keep the local values, host all-reduces multiply by size. The
 * results are NOT a solution; it times one rank's share of a multi-GPU step (bench.py --rehearse). */
int aa_comm_create_solo(int rank, int size, aa_comm* out);
int aa_comm_destroy(aa_comm c);
int aa_comm_info(aa_comm c, int* rank, int* size);
/* In-place SUM of a host array over the ranks (blocking; setup-time agreements, tests). */
int aa_comm_allreduce_host(aa_comm c, double* buf, long long n);
/* Attach before aa_elastic_initialize; the communicator must outlive the solver. */
int aa_elastic_set_comm(aa_elastic h, aa_comm c);

/* ---- benchmarking hooks (device-resident inputs, no host traffic) ------------------ */
/* Enqueue `iters` iterations of the ADMM loop of the current time step without the
 * per-step prologue/epilogue; used by bench.py to time the hot loop alone. */
int aa_elastic_bench_iterations(aa_elastic h, int iters, double* ms);
/* Average device time (ms) per launch of the named kernel class over the last bench call,
 * measured with HIP events on the solver's stream; and its algorithmic bytes per launch. */
int aa_elastic_kernel_stats(aa_elastic h, const char* name, double* avg_ms, double* bytes, int* launches);
/* Diagnostics of the hyperelastic local step's work queue, summed over its launches since the
 * last reset (enabled by AA_LQ_STATS=1 in the environment at aa_elastic_initialize; zeros
 * otherwise): out[0..100] elements by L-BFGS iteration count (mcloptlib LBFGS.hpp:205-305 outer
 * iterations; 0 = the start point passed the gradient test), out[101] trips (one L-BFGS
 * iteration for every busy lane of a wave), out[102] queue refills, out[103] waves. Writes
 * min(cap, 104) counters into *count. */
int aa_elastic_local_stats(aa_elastic h, long long* out, int cap, int reset, int* count);
/* Wall-clock phases of the last aa_elastic_initialize (Solver::initialize, Solver.cpp:373-498):
 * names '\n'-separated into names[0..names_cap) (NUL-terminated), milliseconds into
 * ms[0..cap); *count = number of phases. */
int aa_elastic_setup_phases(aa_elastic h, char* names, int names_cap, double* ms, int cap, int* count);

/* ==== Geometry: ALMGeometrySolver<3> + Constraint<3> (bldeng/AA-ADMM Geometry/) ============= */
typedef struct aa_geom_s* aa_geom;        /* one ALMGeometrySolver<3> instance             */

/* Constraint types (Geometry/Constraint.h). Index count k per constraint and the per-constraint
 * parameters each type takes (params is [count][P], row-major):
 *   AA_CON_PLANE        PlaneConstraint(idI, w)                     k >= 3    P = 0  (:396-414)
 *   AA_CON_ANGLE        AngleConstraint<3>(tip, s1, s2, w, min, max) k = 3     P = 2  (:220-296)
 *   AA_CON_EDGE         EdgeLengthConstraint<3>(i1, i2, w, length)   k = 2     P = 1  (:194-218)
 *   AA_CON_CLOSENESS    ClosenessConstraint<3>(i, w, target)         k = 1     P = 3  (:299-326;
 *                       its projection is the identity in the reference, kept as such)
 *   AA_CON_POINT_TO_REF PointToRefSurfaceConstraint(i, w, aabb)      k = 1     P = 1 = surface id (:328-349)
 *   AA_CON_REF_SURFACE  ReferenceSurfceConstraint(n, w, V, F): one   k = 1     P = 1 = surface id (:351-394)
 *                       constraint over points 0..count-1 (idx may be NULL)                    */
#define AA_CON_PLANE 0
#define AA_CON_ANGLE 1
#define AA_CON_EDGE 2
#define AA_CON_CLOSENESS 3
#define AA_CON_POINT_TO_REF 4
#define AA_CON_REF_SURFACE 5

/* SPDSolverType (Geometry/SolverCommon.h:34-38); both factorisations are a Cholesky here. */
#define AA_SPD_LDLT 0
#define AA_SPD_LLT 1

typedef struct {
    double setup_ms;         /* setup_ADMM: assembly of the global matrix and rhs_fixed       */
    double factor_ms;        /* nested-dissection ordering + factorisation (first solve)     */
    double solve_ms;         /* wall time of the last solve_ADMM (device-synchronised)       */
    int iterations;          /* x-updates of the last solve (accepted + rejected)            */
    int accepted;            /* accepted iterations (= function_values_.size())              */
    int rejects;             /* Anderson rejections                                          */
    int n_points;
    long long nnz_factor;    /* scalar nnz(L) of the global factor                           */
    long long hard_cols, soft_cols, n_constraints;
} aa_geom_runtime;

int aa_geom_create(aa_ctx ctx, aa_geom* out);                                  /* ALMGeometrySolver() */
/* Solver kinds: AA_GEOM_ALM = ALMGeometrySolver<3> (Geometry/ALMGeometrySolver.h);
 * AA_GEOM_PLAIN = GeometrySolver<3> (Geometry/GeometrySolver.h:85-263): every constraint row
 * unweighted and scaled by the penalty, u on every column, soft constraints projected with
 * Constraint::project_and_combine (Constraint.h:118-130), residual |Dx - z|, Anderson on (u, x)
 * with u the effective part and `replace` (no history reset) when the residual increases;
 * get_solution() = current_x_. Same calls otherwise.                                         */
#define AA_GEOM_ALM 0
#define AA_GEOM_PLAIN 1
int aa_geom_create_kind(aa_ctx ctx, int kind, aa_geom* out);
int aa_geom_destroy(aa_geom h);                                                /* ~ALMGeometrySolver  */
/* Reference surface (TriMeshAABB / igl::AABB over V (nv x 3), F (nf x 3)); returns its id. */
int aa_geom_add_ref_surface(aa_geom h, const double* V3, int nv, const int* F3, int nf, int* id);
/* add_hard_constraint (hard = 1) / add_soft_constraint (hard = 0) of `count` constraints of one
 * type: idx is [count][k] point ids, weight the constructor weight, params [count][P]. */
int aa_geom_add_constraints(aa_geom h, int hard, int type, const int* idx, int k, int count, double weight,
                            const double* params);
/* add_laplacian / add_uniform_laplacian (coefs as given; ref_points3 == NULL) and
 * add_relative_laplacian / add_relative_uniform_laplacian (ref_points3 = 3 x n points). */
int aa_geom_add_laplacian(aa_geom h, const int* idx, const double* coefs, int k, double weight,
                          const double* ref_points3);
int aa_geom_add_closeness(aa_geom h, int idx, double weight, const double* target3);   /* add_closeness */
/* Batched forms for bindings whose per-call overhead dominates (one call per point is ~10 us from
 * Python): the same rows in the same order as n_rows aa_geom_add_laplacian calls (row r: indices
 * idx[row_ptr[r] .. row_ptr[r+1]), coefficients coefs[same range], weight weights[r]; relative[r]
 * != 0 -- relative may be NULL -- passes ref_points3 as add_relative_laplacian does), and as n
 * aa_geom_add_closeness calls (targets3: n x 3). Reference: the per-point loops of
 * Geometry/PlanarityOpt.cpp / WireMeshOpt.cpp over LinearRegularization.h:91-117. */
int aa_geom_add_laplacians(aa_geom h, int n_rows, const int* row_ptr, const int* idx, const double* coefs,
                           const double* weights, const int* relative, const double* ref_points3);
int aa_geom_add_closenesses(aa_geom h, int n, const int* idx, const double* weights, const double* targets3);
int aa_geom_setup(aa_geom h, int n_points, double penalty, int spd_solver_type);       /* setup_ADMM    */
/* solve_ADMM(init_x (3 x n), rel_residual_eps, max_iter, Anderson_m): max_iter accepted
 * iterations; Anderson_m = 0 runs plain ADMM. */
int aa_geom_solve(aa_geom h, const double* init_x3, double rel_residual_eps, int max_iter, int anderson_m);
int aa_geom_get_solution(aa_geom h, double* x3);                               /* get_solution()      */
/* Run-to-epsilon for later solves (new surface; the reference computes residual_eps at
 * ALMGeometrySolver.h:172 but its stopping test is commented out at :258-260). stop_at_eps = 1
 * ends the loop after the first accepted iteration whose combined residual is below
 * rel_residual_eps^2 * hard_cols^2 * 2; eps_rel > 0 also ends it once comb <= eps_rel * comb of
 * the first accepted iteration. (0, 0) = the reference loop (max_iter accepted iterations).
 * ALMGeometrySolver only. */
int aa_geom_set_stop(aa_geom h, int stop_at_eps, double eps_rel);
/* function_values_ (combined residual per accepted iteration) and elapsed_time_ (s since the
 * loop started, device clock). Returns the count in *n (<= cap copied). */
int aa_geom_get_history(aa_geom h, double* comb, double* time_s, int cap, int* n);
int aa_geom_runtime_info(aa_geom h, aa_geom_runtime* out);
/* closest points on a reference surface (PointToRefSurfaceConstraint's projection) */
int aa_geom_closest_points(aa_geom h, int surface, const double* p3, int n, double* out3);
int aa_geom_bench_iterations(aa_geom h, int iters, double* ms);
int aa_geom_kernel_stats(aa_geom h, const char* name, double* avg_ms, double* bytes, int* launches);
/* Multi-GPU (see aa_comm above): attach before the first aa_geom_solve; every rank adds the same
 * constraints; the first solve partitions the points (nested dissection of the global matrix on
 * the initial positions) and each rank projects the constraints of its part. */
int aa_geom_set_comm(aa_geom h, aa_comm c);

/* ---- element-level test hooks (parity tests only; not part of the reference API) ----------
 * The device functions of the local step / Anderson solve / projections applied to host arrays
 * (uploaded, one device thread per element), so tests can pin them to the reference's element
 * tables (tests/golden/elements.npz, geom_elements.npz) directly:
 *   aa_test_prox: op 0 TetEnergyTerm::prox (in/out 9 per tet, TetEnergyTerm.cpp:74-96),
 *     1 NeoHookeanTet / 2 StVKTet prox (L-BFGS, TetEnergyTerm.cpp:151-162; prm4 = E, nu, h with
 *     vol = h^3/6; iters = L-BFGS iterations, -1 on a line-search failure), 3 / 4 TriEnergyTerm
 *     prox of the H / X solver copy (6 per tri; prm4[2..3] = limit_min, limit_max), 5 the bending
 *     hinge's prox (3 per hinge; prm4[0] = r), 6 the spring's prox (3 per spring; prm4 = L, mode)
 *   aa_test_cod_solve: the Anderson normal-equation solve (Eigen CompleteOrthogonalDecomposition,
 *     AndersonAcceleration.h:186-188) of a k x k column-major M
 *   aa_test_geom_project: Constraint::project_impl of plane (k 3..8) / angle (k 3) / edge (k 2)
 *     on n transformed point sets (3 x cols each, column-major); prm2 = angle min, max / edge length
 *   aa_test_mesh_sdf: the mesh obstacle's signed distance on n queries q3: the closest surface
 *     point, dx (-|q - c| inside; +|q - c| otherwise, reported by this hook only) and the closest
 *     triangle in the caller's numbering
 *   aa_test_collision_prox: Collision::prox on n candidates q3 against an obstacle list in
 *     insertion order: obs_rows = n_obs rows of 8 doubles {type, parameters as stored: a
 *     SLIDE_FLOOR normal is taken as given}, a row {AA_OBS_MESH, m} naming mesh m of the n_meshes
 *     meshes given concatenated (mesh m: vertices mesh_vert_ptr[m]..mesh_vert_ptr[m+1] of
 *     mesh_verts3, triangles mesh_tri_ptr[m]..mesh_tri_ptr[m+1] of mesh_tris3 with indices local
 *     to the mesh)
 *   aa_test_mesh_sdf_posed / aa_test_collision_prox_posed: the same with kinematic poses
 *     (aa_elastic_set_mesh_obstacle_pose; validated alike): pose12 for the one mesh, mesh_poses =
 *     12 doubles per mesh (twelve NaNs: that mesh unposed); NULL = unposed. Queries and the reported closest point are in the
 *     world frame, dx is the obstacle-frame distance.
 *   aa_test_mesh_refit_tables: the tables of a mesh obstacle built from verts3 / tris3 and, when
 *     new_verts3 is given, refitted to it (aa_elastic_set_mesh_obstacle_vertices; validated alike):
 *     device = 0 the host restatement (ctx may be NULL), 1 what the kernels wrote, downloaded.
 *     Outputs, each optional: the n_nodes 128-byte node records, the leaf triangles (9 doubles
 *     each), the pseudonormal table (21 each), the leaf order -> caller triangle map, the root box
 *     (lo then hi) and the node count (at most n_tris).
 *   aa_test_mesh_sdf_deformed: aa_test_mesh_sdf_posed on the mesh built from verts3 and refitted on
 *     the device to new_verts3. ms4 (optional) receives four times in ms: host preparation plus
 *     upload of the deformed mesh from scratch (wall), the device refit, the signed-distance kernel
 *     on the refitted tree and on a freshly built tree of the same shape (the last three by device
 *     events, the median of 5 runs after a warm-up).
 *   aa_test_bound_refit: the mesh built from verts3 / tris3, its vertices gathered from the n_nodes_x
 *     positions x3 through nodes (vertex i = x3[nodes[i]]), then checked and -- if the check passes --
 *     refitted (aa_elastic_bind_mesh_obstacle); x3_first (optional): a bound refit from these
 *     positions runs before it, as an earlier step's would. device = 0 the host restatement (ctx
 *     may be NULL), 1 what the kernels wrote. Outputs of aa_test_mesh_refit_tables plus status2 = {taken, cause}
 *     and vol6, the check's chunked sum; ms (optional, device = 1): the device time of gather +
 *     check + refit by device events, the median of 5 runs after a warm-up.
 *   aa_test_collision_prox_exempt: aa_test_collision_prox_posed with a node id per query (q_node)
 *     and per mesh a list of exempt nodes (mesh m: exempt_nodes[exempt_ptr[m]..exempt_ptr[m+1])).
 *   aa_test_contact_friction: the friction pass's device function (aa_elastic_set_obstacle_friction)
 *     on n queries. Obstacle rows now and previous (8 doubles each, same types) with mu per row; the
 *     concatenated meshes with poses now and previous (12 doubles per mesh, a row of NaNs = no
 *     pose) and mesh_still (optional; non-zero = g is 0 for that mesh); per query the exemption
 *     node id, a pinned flag, x_old, x_new, u, w, m; p and dt. Outputs per query: x' (x_new's bits
 *     where s = 0), the contact flag, the row, c, n, j, rt, s.
 *   aa_test_contact_friction_carry: the carry form of the same on the same arguments plus, per
 *     mesh, the previous vertices (concatenated like mesh_verts3) and a carry flag; it also returns
 *     per query the triangle (the caller's index, -1 = none) and the barycentric weights. */
int aa_test_prox(aa_ctx ctx, int op, const double* prm4, const double* in, int n, double* out, int* iters);
int aa_test_cod_solve(aa_ctx ctx, int k, const double* M, const double* b, double* theta);
int aa_test_geom_project(aa_ctx ctx, int type, int k, const double* prm2, const double* in, int n, double* out);
int aa_test_mesh_sdf(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris, const double* q3, int n,
                     double* closest3, double* dx, int* tri);
int aa_test_collision_prox(aa_ctx ctx, const double* obs_rows, int n_obs, const double* mesh_verts3,
                           const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr, int n_meshes,
                           const double* q3, int n, double* out3);
int aa_test_mesh_sdf_posed(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                           const double* pose12, const double* q3, int n, double* closest3, double* dx, int* tri);
int aa_test_collision_prox_posed(aa_ctx ctx, const double* obs_rows, int n_obs, const double* mesh_verts3,
                                 const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr, int n_meshes,
                                 const double* mesh_poses, const double* q3, int n, double* out3);
int aa_test_mesh_refit_tables(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                              const double* new_verts3, int device, void* nodes_bytes, double* tris9, double* pn21,
                              int* orig, double* lohi6, int* n_nodes);
int aa_test_mesh_sdf_deformed(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                              const double* new_verts3, const double* pose12, const double* q3, int n,
                              double* closest3, double* dx, int* tri, double* ms4);
int aa_test_bound_refit(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris, const double* x3,
                        int n_nodes_x, const int* nodes, int device, void* nodes_bytes, double* tris9, double* pn21,
                        int* orig, double* lohi6, int* n_nodes, int* status2, double* vol6, double* ms,
                        const double* x3_first);
int aa_test_collision_prox_exempt(aa_ctx ctx, const double* obs_rows, int n_obs, const double* mesh_verts3,
                                  const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr, int n_meshes,
                                  const double* mesh_poses, const double* q3, const int* q_node, int n,
                                  const int* exempt_ptr, const int* exempt_nodes, double* out3);
int aa_test_contact_friction(aa_ctx ctx, const double* obs_rows, const double* obs_rows_prev, const double* mu, int n_obs,
                             const double* mesh_verts3, const int* mesh_vert_ptr, const int* mesh_tris3,
                             const int* mesh_tri_ptr, int n_meshes, const double* mesh_poses,
                             const double* mesh_poses_prev, const unsigned char* mesh_still, const int* q_node,
                             const unsigned char* q_pinned, int n, const int* exempt_ptr, const int* exempt_nodes,
                             const double* x_old3, const double* x_new3, const double* u3, const double* w,
                             const double* m, double penalty, double dt, double* x_out3, int* hit, int* row,
                             double* point3, double* normal3, double* push, double* slip3, double* scale);
int aa_test_contact_friction_carry(aa_ctx ctx, const double* obs_rows, const double* obs_rows_prev, const double* mu, int n_obs,
                                   const double* mesh_verts3, const int* mesh_vert_ptr, const int* mesh_tris3,
                                   const int* mesh_tri_ptr, int n_meshes, const double* mesh_poses,
                                   const double* mesh_poses_prev, const unsigned char* mesh_still, const int* q_node,
                                   const unsigned char* q_pinned, int n, const int* exempt_ptr, const int* exempt_nodes,
                                   const double* x_old3, const double* x_new3, const double* u3, const double* w,
                                   const double* m, double penalty, double dt, const double* mesh_verts_prev3,
                                   const unsigned char* mesh_carry, double* x_out3, int* hit, int* row, double* point3,
                                   double* normal3, double* push, double* slip3, double* scale, int* tri, double* bary3);
/* The global step's sparse triangular solve alone (DirectSolver, csrc/direct_solve.hpp), on a
 * caller-given SPD matrix: full-pattern symmetric CSR (ptr, col, val; sorted columns, every
 * diagonal stored) of order n in the caller's ordering, node coordinates xyz3.
 *   tree: n_tree = 0 runs nested_dissection(leaf_size, top_rows); n_tree > 0 gives the supernode
 *     tree itself -- pivot ranges [tree_beg[s], tree_end[s]) in postorder covering [0, n), parent
 *     (-1 = root) -- with the identity permutation; every off-diagonal entry of a supernode's
 *     columns must lie in the supernode or in one of its ancestors.
 *   build: wave_p, wave_r, max_sets (1 | 2), wide, default_branches as DirectSolver::build takes
 *     them; the AA_SOLVE_* / AA_SUB_* / AA_FACTOR_NT* knobs are read from the environment by
 *     build() as always (a fresh solver is built on every call).
 *   device_factor: 0 = multifrontal_cholesky on the host, 1 = factor_on_device (AA_DENSE_MIN_FRONT).
 *   script: n_script entries run in order on the one solver: AA_SOLVE_B0 / _B1 = solve(b),
 *     AA_SOLVE_BOTH = solve2(b0, b1), AA_SOLVE_GATED_SKIP_* = gated solve with ctrl->reject = 0
 *     (skipped), AA_SOLVE_GATED_TAKE_* = gated with reject = 1 (taken), AA_SOLVE_DONE_* = solve
 *     with ctrl->done = 1 (skipped). b1 may be NULL when no entry names it. Both output buffers
 *     are filled with `sentinel` before every entry.
 *   x_out: n_script x 2 x n x 3, per entry the two output buffers (the second is written by
 *     AA_SOLVE_BOTH only) un-permuted to the caller's ordering; x_host: 2 x n x 3,
 *     factor_solve_host of b0 and b1 with the same factor; row_info: n x 2 (may be NULL), per node
 *     the height and the depth (root = 0) of the supernode that owns it; plan: the
 *     DirectSolver::PlanSummary as ints (plan_cap of them at most; *plan_count = how many there are). */
enum { AA_SOLVE_B0 = 0, AA_SOLVE_B1 = 1, AA_SOLVE_BOTH = 2, AA_SOLVE_GATED_SKIP_B0 = 3, AA_SOLVE_GATED_SKIP_B1 = 4,
       AA_SOLVE_GATED_TAKE_B0 = 5, AA_SOLVE_GATED_TAKE_B1 = 6, AA_SOLVE_DONE_B0 = 7, AA_SOLVE_DONE_B1 = 8 };
int aa_test_direct_solve(aa_ctx ctx, int n, const double* xyz3, const int* ptr, const int* col, const double* val,
                         int n_tree, const int* tree_beg, const int* tree_end, const int* tree_parent, int leaf_size,
                         int top_rows, int wave_p, int wave_r, int max_sets, int wide, int default_branches,
                         int device_factor, const double* b0, const double* b1, int n_script, const int* script,
                         double sentinel, double* x_out, double* x_host, int* row_info, int* plan, int plan_cap,
                         int* plan_count);
/* One Anderson step (AndersonAcceleration::compute_impl, AndersonAcceleration.h:154-211) from a
 * caller-given state: the solvers' own launch_aa_reduce -> launch_aa_solve -> launch_aa_mix on
 * uploaded arrays, without the fused combined-residual head, and everything they can write handed
 * back. The two segments of G (na then nb entries; dim = na + nb), of out and of copy_to are
 * separate device allocations.
 *   in/out: cur (dim), dF (m x eff, column stride eff), dG (m x dim), ctl9 = {aa_iter, aa_col,
 *     aa_skip, aa_active, done, aa_mk, aa_j, aa_jn, aa_first}, scale (m), M (m x m column-major),
 *     coef (m), aa_s, out (dim; what it holds on entry is uploaded, so an untouched out shows;
 *     ignored with AA_STEP_INPLACE), copy_to (dim, likewise; read with AA_STEP_COPY_TO only)
 *   mask4 = {lo1, hi1, lo2, hi2}: the AAMask windows in the second segment
 *   nblocks: blocks of the reduce, 0 = what the solvers take for this dim
 *   flags: AA_STEP_COPY_TO the reduce copies G; AA_STEP_INPLACE out.a == cur (nb must be 0);
 *     AA_STEP_NARROW launch_aa_mix's narrow instantiations for m <= 7; AA_STEP_ROWS the
 *     row-parallel reduce for m > 16 (default there: the column-parallel one)
 *   red: the reduce's block partials, info3[1] x (2 + 2 info3[0]) doubles (red_cap = its capacity;
 *     zero where the kernels wrote nothing); info3 = {aa_window_bucket(m), blocks, 1 cols / 0 rows /
 *     -1 not the 32 bucket} */
enum { AA_STEP_COPY_TO = 1, AA_STEP_INPLACE = 2, AA_STEP_NARROW = 4, AA_STEP_ROWS = 8 };
int aa_test_anderson_step(aa_ctx ctx, int m, long long na, long long nb, long long eff, const double* G, double* cur,
                          double* dF, double* dG, int* ctl9, double* scale, double* M, double* coef, double* aa_s,
                          const long long* mask4, int nblocks, int flags, double* red, long long red_cap, double* out,
                          double* copy_to, int* info3);

#ifdef __cplusplus
}
#endif
#endif /* AA_ADMM_H */
