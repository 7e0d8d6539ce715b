// Device data structures and kernel launchers of the admm-elastic hot path.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh.hpp"

namespace aa {

constexpr int kMaxM = 32;          // largest Anderson window supported on device
constexpr double kCombEps = 1e-20; // Solver.cpp:93 eps

// The kinds of energy term (kCollision: CollisionEnergyTerm.hpp:41-117). The values are fixed: the
// C ABI's add_tets / add_tris mean 0 and 1. What each kind is stands in kind_traits below.
enum ElemKind : int { kTet = 0, kTri = 1, kCollision = 2, kHinge = 3, kSpring = 4, kTie = 5 };
constexpr int kNumKinds = 6;

// One homogeneous block of energy terms (same kind / material / Lame), SoA on device.
struct GroupDev {
    ElemKind kind;       // an int in size and place: every element kernel takes GroupDev first, by value
    int mat;             // 0 linear, 1 NeoHookean, 2 StVK; KindTraits::mode_in_mat: the spring mode
    int count;           // elements
    int nv, ncol, dim;   // 4/3/9 for tets, 3/2/6 for tris
    int pinned;          // some element of the group has a pinned node (C_fix terms exist)
    long long zoff;      // z/u offset: component c of element e at zoff + c*count + e
    long long yrow;      // first vertex slot of this group in the slot array y (slot e*nv + a, 3 doubles)
    const int* idx;      // [nv][count] internal node ids
    const int* spos;     // [nv][count] position of the vertex's rhs slot (node order), -1 = pinned
    const double* G;     // [(c*nv + a)][count]  F[:,c] = sum_a G[c][a] x_a
    const double* w;     // [count] ADMM weights sqrt(k*vol)
    const double* vol;   // [count]; KindTraits::rest_in_vol: the rest length
    double mu, lambda, k, lmin, lmax;
    const double* obs;   // collision points: the obstacle table (obs[0] = count, then kObsStride per obstacle)
};
// Per-element material parameters of a group (aa_elastic_add_*_var; the reference's one Lame per
// EnergyTerm, TetEnergyTerm.hpp:36-51 / TriEnergyTerm.hpp:33-47), [count] each like w and vol;
// all null = a uniform group, whose kernels read GroupDev's scalars. Kept beside GroupDev, not in
// it, and handed only to the per-element instantiations (as their last argument): GroupDev is the
// first argument of every element kernel, so growing it would move every uniform kernel's
// arguments. k = lambda + (2/3) mu is formed on the host with the uniform path's expression.
struct GroupVar {
    const double* mu = nullptr;
    const double* lambda = nullptr;
    const double* k = nullptr;
    const double* lmin = nullptr;    // triangles only
    const double* lmax = nullptr;
    explicit operator bool() const { return k != nullptr; }
};
// passive obstacles of the collision terms (PassiveObject.hpp:32-136): type, then up to 7 parameters
// OBS_MESH (PassiveMesh, :138-178): a triangle-mesh obstacle, parameter 1 = its row in the mesh table
enum ObsType { OBS_FLOOR = 0, OBS_SLIDE_FLOOR = 1, OBS_SPHERE = 2, OBS_PLANE_HALF_SPHERE = 3, OBS_CYLINDER = 4, OBS_MESH = 5 };
constexpr int kObsStride = 8, kMaxObstacles = 256;
// What the friction pass reads beside the tables in force (contact_friction.hpp)
struct FrictionTables {
    const double* obs_prev;           // the obstacle table in force during the previous step
    const MeshObsDev* mesh_prev;      // the mesh table's rows then (R and t are read)
    const double* mu;                 // [rows] coefficient per obstacle row, shared insertion order
    const unsigned char* mesh_still;  // [mesh rows] non-zero: g = 0 (vertices changed, bound mesh)
};
// A mesh that carries (aa_elastic_set_mesh_obstacle_carry): one row per mesh row, both null for a
// mesh that does not. Kept beside FrictionTables, not in it, and handed only to the carry form of
// the pass as its trailing pack (as GroupVar is): growing FrictionTables would move the plain
// kernel's arguments.
struct MeshCarryDev {
    const double* vprev;     // [nv][3] the vertices in force during the previous step's pass
    const int* leaf_vid;     // [tris][3] vertex ids of leaf triangle k (MeshRefitTables::leaf_vid)
};
__host__ __device__ constexpr int ncol_of(int nv) { return nv - 1; }   // a simplex: its edge columns

// What a kind is, in one place. Host messages, the byte model, initialize's refusals, the shape
// below and the kernels' branches all read this table; a new kind is a row here (DESIGN.md §3.3,
// "Element kinds").
struct KindTraits {
    const char* noun;      // "the solver has <noun>", "<noun> exist in the (u,x) variant only"
    const char* term;      // one element, and "no <term> term"
    const char* needs;     // "(<needs> one rank)"
    int nv_min, nv_max;    // admissible vertex counts
    bool one_col;          // one column z (3 doubles) per element; false: the simplex's nv - 1 columns
    bool rest_in_vol;      // GroupDev::vol holds a rest length (the hinge's r, a spring's or tie's L)
    bool mode_in_mat;      // GroupDev::mat holds the spring mode (AA_SPRING_*), not a material
    bool z_and_ranks;      // the z variant and partitioned solvers take it; false: initialize refuses both
};
__host__ __device__ constexpr KindTraits kind_traits(ElemKind k) {
    switch (k) {
    case kTet:       return {"tets", "tet", "tets need", 4, 4, false, false, false, true};
    case kTri:       return {"triangles", "triangle", "triangles need", 3, 3, false, false, false, true};
    // (the z variant refuses collision points in the reference's own words, before this table is asked)
    case kCollision: return {"collision points", "collision", "collisions need", 1, 1, true, false, false, true};
    // G holds K (bending.hpp), the one column is z = K x
    case kHinge:     return {"bending hinges", "hinge", "bending needs", 4, 4, true, true, false, false};
    // G = (-1, +1), z = x_b - x_a (springs.hpp)
    case kSpring:    return {"springs", "spring", "springs need", 2, 2, true, true, true, false};
    // nv = na + nb, G = (-a, +b), z = sum_j b_j x_Bj - sum_i a_i x_Ai (ties.hpp); else as a spring
    case kTie:       return {"ties", "tie", "ties need", 3, 6, true, true, true, false};
    }
    return {"", "", "", 0, 0, false, false, false, false};
}
__host__ __device__ constexpr int kind_ncol(ElemKind k, int nv) { return kind_traits(k).one_col ? 1 : nv - 1; }

// The element kernels' shape parameter S says the kind and the vertex count: 100 kind + nv, so a
// kernel's name in a profile reads e.g. <503, 0> = a three-vertex tie.
__host__ __device__ constexpr int shape(ElemKind k, int nv) { return 100 * (int)k + nv; }
__host__ __device__ constexpr ElemKind shape_kind(int s) { return (ElemKind)(s / 100); }
__host__ __device__ constexpr int shape_nv(int s) { return s % 100; }
__host__ __device__ constexpr int shape_nc(int s) { return kind_ncol(shape_kind(s), shape_nv(s)); }
// every kind and admissible nv: the shape gives back what made it, and no two pairs share one
constexpr bool shapes_ok() {
    for (int k = 0; k < kNumKinds; ++k) {
        const KindTraits t = kind_traits((ElemKind)k);
        for (int nv = t.nv_min; nv <= t.nv_max; ++nv) {
            const int s = shape((ElemKind)k, nv);
            if (shape_kind(s) != k || shape_nv(s) != nv || shape_nc(s) != (t.one_col ? 1 : nv - 1)) return false;
            for (int k2 = 0; k2 < k; ++k2)
                for (int nv2 = kind_traits((ElemKind)k2).nv_min; nv2 <= kind_traits((ElemKind)k2).nv_max; ++nv2)
                    if (shape((ElemKind)k2, nv2) == s) return false;
        }
    }
    return true;
}
static_assert(shapes_ok(), "shape(kind, nv) must round-trip, give the traits' column count and be unique");

// Device-side control block: residual bookkeeping, reject/done flags, Anderson state.
struct Ctrl {
    double prim, prev_prim, comb, prim2, dual2;
    int reject, done, nrec, nrej;
    int cap, fail, iters_run, aa_skip;   // aa_skip: ALM reject -> no Anderson step this iteration
    // Anderson acceleration (AndersonAcceleration.h state)
    int aa_m, aa_iter, aa_col, aa_mk;
    int aa_j, aa_jn, aa_first, aa_active;
    double aa_s;
    double scale[kMaxM], coef[kMaxM];
    double M[kMaxM * kMaxM];      // normal-equation matrix, column-major m x m
    // Geometry ALM loop (ALMGeometrySolver.h:186-263): `reset` flag and accepted-iteration cap
    int alm_reset, max_iter;
    // time-to-epsilon: device clock (wall_clock64) of every recorded iteration and
    // of the step's start; optional stop once comb <= eps_rel * comb of the first recorded
    // iteration (eps_rel = 0: the reference's loop, only the comb < 1e-20 break).
    long long* hist_clock;
    long long clock0;
    double eps_rel, eps_abs;
    int eps_hit, pad_;
};
// device stamp of the step's start (ctrl->clock0)
void launch_stamp(Ctrl* ctrl, hipStream_t s);

// A vector seen as two concatenated segments (e.g. (u, x) of the UX variant).
struct Seg2 {
    double* a; long long na;
    double* b; long long nb;
};

// Entries of the second segment that enter the Anderson dot products (partitioned solvers: the
// x entries this rank owns -- its part and, on rank 0, the shared separators); the first
// segment always counts. Default: everything.
struct AAMask {
    long long lo1 = 0, hi1 = 0x7fffffffffffffffLL, lo2 = 0, hi2 = 0;
};

struct ElasticLaunch;  // fwd

// ---- launchers (elastic_kernels.hip) ---------------------------------------------------
enum LocalMode { LZ_NORMAL = 0, LZ_REDO = 1, LZ_INIT = 2 };

// Work queue of the hyperelastic local step: a device counter, the resident grid on the solver's
// device and the refill threshold (computed once per solver, make_local_queue)
struct LocalQueue {
    int* counter = nullptr;
    int resident = 0, refill = 60;
    int refill_lanes = 60;   // refill before the split queue halves it (per-element groups never split)
    // k_local_z_hqf (the refill's loads regrouped; groups without pins) instead of the plain
    // k_local_z_hq: the default, AA_LQ_FUSED=0 turns it off
    bool fused = false;
    bool split = false;  // AA_LQ_SPLIT=1: k_local_z_hq2 (each element's L-BFGS over a lane pair)
    // optional diagnostics (AA_LQ_STATS=1): [0..100] elements by L-BFGS iterations (0 = the start
    // point passed the gradient test), [101] trips, [102] refills, [103] waves; summed over launches
    unsigned long long* stats = nullptr;
};
constexpr int kLqStats = 104;
LocalQueue make_local_queue(int device, int* counter);
// z = prox(P x + u/w); prim partials; optional y = w(w z + c - u). gate: !done (and reject for REDO)
// queue given: hyperelastic groups without partials run as a persistent work queue
// var given (launch_u_and_y too): the group's per-element material instantiation of the same kernel
// meshes given: the collision group's mesh-aware instantiation (obstacle rows of type OBS_MESH
// index this table); null: the analytic shapes' instantiation
void launch_local_z(const GroupDev& g, const double* xfull, const double* u, double* z, double* y, int nf,
                    int variant, int mode, Ctrl* ctrl, double* red, int red_off, hipStream_t s,
                    const LocalQueue* queue = nullptr, const GroupVar& var = GroupVar(),
                    const MeshObsDev* meshes = nullptr);
// The combined-residual pass's local step with its residual folded in (k_local_z_hqf<4, false, ResArgs>):
// per element |w(P x - z_c)|^2 to pe[zoff + e] and |w(z_c - zref)|^2 to pe[zoff + count + e], with
// k_prim_z's statements; z_c itself is not stored. local_z_res_ok: the groups that take it -- those
// the fused-refill queue serves (hyperelastic tets without pins, AA_LQ_FUSED on, no AA_LQ_SPLIT).
// launch_prim_sum: k_prim_z's block partials from pe (same layout, block sum and gate: same bits)
bool local_z_res_ok(const GroupDev& g, const LocalQueue* queue);
void launch_local_z_res(const GroupDev& g, const double* xfull, const double* u, const double* zref, double* pe, int nf,
                        Ctrl* ctrl, hipStream_t s, const LocalQueue* queue, const GroupVar& var = GroupVar());
void launch_prim_sum(const GroupDev& g, const double* pe, Ctrl* ctrl, double* red_a, double* red_b, int red_off,
                     hipStream_t s);
// r = w(P x - z); prim2/dual2 partials; u += r (UX variant update_u fused with the residual)
void launch_resid_update_u(const GroupDev& g, const double* xfull, const double* xlast, const double* z, double* u,
                           int nf, Ctrl* ctrl, double* red_a, double* red_b, int red_off, hipStream_t s);
// Z variant: u = uin + w(Px - z) [mode 0] or u = grad E(z)/w [mode 1]; then y = w(w z + c - u) (mode 2: of uin,
// nothing written to u). uin may be u. gate !done (+reject if redo)
void launch_u_and_y(const GroupDev& g, const double* xfull, const double* z, const double* uin, double* u, double* y,
                    int nf, int mode, int redo, Ctrl* ctrl, hipStream_t s, const GroupVar& var = GroupVar());
// prim2 partials of |w(Px - z)|^2 and optionally dual2 partials of |w(z - zref)|^2. gate !done (+reject if redo)
void launch_prim_z(const GroupDev& g, const double* xfull, const double* z, const double* zref, int nf, int redo,
                   Ctrl* ctrl, double* red_a, double* red_b, int red_off, hipStream_t s);
// b = Mxbar + pdt2 * (D^T rows) . y ; optionally xlast = xsrc (free part) in the same pass
// red_final: UX "prim final" fused in block 0 (prim recomputed after a reject; prev_prim = prim)
void launch_rhs(int nf, const int* ptr, const int* row, const double* val, const double* y, const double* Mxbar,
                double pdt2, double* b, Ctrl* ctrl, int gate_reject, hipStream_t s,
                const double* xsrc = nullptr, double* xlast = nullptr, const double* red_final = nullptr,
                int nb_final = 0);
// UX reject test + restore fused (replaces CTL_PRIM_CHECK + launch_restore_ux)
// Z variant: k_control's CTL_PRIM_CHECK_Z and the reject branch's three restores in one launch
// (u null: x and z only)
void launch_check_restore_z(Ctrl* ctrl, const double* red, int nb, int accel, double* u, double* x, double* z,
                            const double* du, const double* dx, const double* dz, long long nz, long long nx,
                            hipStream_t s);
void launch_check_restore_ux(Ctrl* ctrl, const double* red, int nb, int accel, double* u, double* x, double* cur,
                             const double* du, const double* dx, long long nz, long long nx, hipStream_t s);
// UX reject: u = du, x = dx, cur = (du, dx) (gate: reject)
void launch_restore_ux(double* u, double* x, double* cur, const double* du, const double* dx, long long nz,
                       long long nx, const Ctrl* ctrl, hipStream_t s);
// control steps
enum CtlOp { CTL_PRIM_CHECK = 0, CTL_PRIM_FINAL = 1, CTL_COMB_UX = 2, CTL_PRIM_CHECK_Z = 3, CTL_PRIM_FINAL_Z = 4,
             CTL_COMB_Z = 5, CTL_COMB_ZP = 6 };
void launch_control(int op, Ctrl* ctrl, const double* red_a, const double* red_b, int nblocks, int accel,
                    double* hist_prim, double* hist_comb, int* hist_rej, hipStream_t s);
// concurrent combined-residual pass: side = *ctrl (fork); records merged back, a break taken
// as done = 2 with x = dx and the later iterations' reject count / failure flag restored, once (join)
void launch_ctrl_fork(const Ctrl* ctrl, Ctrl* side, hipStream_t s);
void launch_ctrl_join(Ctrl* ctrl, const Ctrl* side, double* x, const double* dx, long long n, hipStream_t s);
// dst = src (gate: !done, and reject if gate_reject)
void launch_copy(double* dst, const double* src, long long n, const Ctrl* ctrl, int gate_reject, hipStream_t s);
// GB/s of a 16-B/lane streaming read of `bytes` (the measured HBM read ceiling; bench.py)
double bench_stream_read(long long bytes, int reps, hipStream_t s);
// predictor: v_y += dt g (free); xbar = x + dt v; Mxbar = m xbar; xfull = xbar (free) / xpin (pinned)
void launch_predict(int n, int nf, double* xstate, double* vstate, const double* mass, double dt, double gravity,
                    double* xbar, double* Mxbar, double* xfull, hipStream_t s);
// z = P xbar (initial z = W^-1 (D xbar - C))
void launch_init_z(const GroupDev& g, const double* xfull, double* z, hipStream_t s);
// new state: x = xsrc (free) / xfull (pinned); v = (x_new - x_old)/dt
void launch_finalize(int n, int nf, const double* xsrc, const double* xfull, double* xstate, double* vstate, double dt,
                     hipStream_t s);
// WindForce::project (ExplicitForce.cpp:47-104) on the step's start state: v += dt 0.33 f_n per
// triangle vertex, triangles in the given order. lvl_ptr[l]..lvl_ptr[l+1] index tri_ord: a level's
// triangles share no vertex with each other, and every earlier triangle sharing a vertex with one
// of them sits in an earlier level -- so one workgroup sweeping the levels reproduces the
// sequential loop (the reference's single-thread order) exactly.
void launch_wind(const int* tris3, const int* tri_ord, const int* lvl_ptr, int nlvl, const double* x, double* v,
                 double dir0, double dir1, double dir2, double dt, hipStream_t s);

// ---- Anderson acceleration (device-side AndersonAcceleration::compute_impl) -----------
// G: the fixed-point map output (2 segments); cur: the stored current iterate (current_u_);
// dF/dG: history (column-major, eff x m / dim x m); copy_to: optional copy of G (the
// "default" iterate kept for the reject test); out: where the accelerated iterate goes.
// m: window (selects the register-resident accumulator bucket 8/12/16/32, aa_window_bucket;
// the block partials hold 2 + 2 aa_window_bucket(m) values).
int aa_window_bucket(int m);
int aa_reduce_blocks(long long dim);
// comb_a/comb_b given: the UX combined residual, break test and record are fused in front
// cols: the 32 bucket's kernel, 1 column-parallel, 0 row-parallel, -1 (every solver) as AA_AA_COLS
// says; aa_test_anderson_step alone names one
void launch_aa_reduce(Seg2 G, const double* cur, long long eff, double* dF, double* dG, Ctrl* ctrl, double* red,
                      int nblocks, Seg2 copy_to, int m, hipStream_t s, const double* comb_a = nullptr,
                      const double* comb_b = nullptr, int comb_nb = 0, double* hist_prim = nullptr,
                      double* hist_comb = nullptr, int* hist_rej = nullptr, AAMask mask = AAMask(), int cols = -1);
void launch_aa_solve(Ctrl* ctrl, const double* red, int nblocks, int m, hipStream_t s);
void launch_aa_mix(Seg2 G, double* cur, long long eff, double* dF, double* dG, Ctrl* ctrl, Seg2 out, int m,
                   hipStream_t s, bool narrow = true);

// ---- element-level test hooks (aa_test_* in the C ABI; tests only)
void launch_test_prox(int op, const double* prm4, const double* in, int n, double* out, int* iters, hipStream_t s);
void launch_test_cod(int n, const double* M, const double* b, double* x, hipStream_t s);
// aa_test_mesh_sdf: per query the closest point, dx (-|q - c| inside, +|q - c| otherwise) and the
// triangle in the caller's numbering; aa_test_collision_prox: collision_prox on n candidates
void launch_test_mesh_sdf(const MeshObsDev* mesh, const double* q, int n, double* closest, double* dx, int* tri,
                          hipStream_t s);
void launch_test_collision_prox(const double* obs, const MeshObsDev* meshes, const double* q, int n, double* out,
                                hipStream_t s);
void launch_test_collision_prox_exempt(const double* obs, const MeshObsDev* meshes, const double* q, const int* node, int n,
                                       double* out, hipStream_t s);

}  // namespace aa
