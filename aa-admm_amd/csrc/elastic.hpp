// Host orchestration of the admm-elastic hot path on one MI355X (the reference's
// admm::Solver, admm_anderson_hard_zxu/src/Solver.{hpp,cpp} and admm_anderson_xzu/src/...).
#pragma once
#include <array>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/aa_admm.h"
#include "bending.hpp"
#include "comm.hpp"
#include "common.hpp"
#include "contact_friction.hpp"
#include "direct_solve.hpp"
#include "elastic_kernels.hpp"
#include "mesh_obstacle.hpp"
#include "mesh_refit.hpp"
#include "springs.hpp"
#include "ties.hpp"

namespace aa {

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
};

// Device storage of one prepared mesh obstacle; upload returns the view the kernels read
struct MeshObsBuffers {
    DevBuf<BvhNode> nodes;
    DevBuf<BvhTri> tris;
    DevBuf<double> pn;
    DevBuf<int> orig;
    MeshObsDev upload(const MeshObstacleHost& M, hipStream_t s) {
        nodes.upload(M.nodes, s);
        tris.upload(M.tris, s);
        pn.upload(M.pn, s);
        orig.upload(M.orig, s);
        MeshObsDev d{};
        d.surf.nodes = nodes.p; d.surf.tris = tris.p;
        d.surf.n_nodes = (int)M.nodes.size(); d.surf.n_tris = (int)M.tris.size();
        d.pn = pn.p; d.orig = orig.p;
        for (int k = 0; k < 3; ++k) { d.lo[k] = M.lo[k]; d.hi[k] = M.hi[k]; }
        return d;
    }
    // Deforming obstacles: what a refit to new vertices needs (mesh_refit.hpp), kept from add time
    // on, and the vertices in force. refit() enqueues the kernels on s and waits for nothing.
    MeshRefitTables tables;
    MeshRefitBuffers rf;
    std::vector<double> verts;
    void keep_for_refit(const MeshObstacleHost& M, const double* V3, int nv, const int* F3, int nf, hipStream_t s) {
        tables = make_refit_tables(M, nv, F3, nf);
        rf.upload(tables, s);
        verts.assign(V3, V3 + 3 * (size_t)nv);
    }
    void refit(const double* V3, hipStream_t s) { rf.refit(V3, nodes.p, (int)nodes.n, tris.p, pn.p, s); }
    // Bound obstacles: vertex i follows solver node bound_nodes[i] (caller's numbering). Exemption:
    // the caller's list and its byte array over the internal numbering (allocated at first use).
    bool bound = false;
    std::vector<int> bound_nodes, exempt_nodes;
    DevBuf<unsigned char> exempt;
    // Carry: the friction pass takes this mesh's displacement from its vertices' own motion
    // (contact_friction.hpp); carry_fresh = switched on since the last pass, whose previous vertices
    // are made equal to the ones in force before the next pass reads them
    bool carry = false, carry_fresh = false;
};

class ElasticSolver {
public:
    explicit ElasticSolver(Context* ctx) : ctx_(ctx) {}
    ~ElasticSolver();

    int add_nodes(const double* x3, const double* m3, int n);
    // per_element given: [count] Lame parameters, one per element (aa_elastic_add_*_var); `lame` is then unused
    void add_elements(ElemKind kind, int material, const double* verts3, const int* idx, int count, const aa_lame& lame,
                      int vertex_offset, const aa_lame* per_element = nullptr);
    // bending hinges on the interior edges of a triangle list (bending.hpp); returns their count
    int add_bending(const double* verts3, const int* tris3, int n_tris, double k_bend, bool flat_rest, int vertex_offset);
    // two-node springs (springs.hpp): one kSpring group per call; node ids pairs2 + vertex_offset
    void add_springs(const double* verts3, const int* pairs2, int n_springs, int mode, const double* k, const double* rest,
                     int vertex_offset);
    // ties between barycentric anchors (ties.hpp): one kTie group per call; node ids + vertex_offset
    void add_ties(const double* verts3, int na, const int* nodes_a, const double* w_a, int nb, const int* nodes_b,
                  const double* w_b, int n_ties, int mode, const double* k, const double* rest, int vertex_offset);
    void set_pins(const int* inds, const double* pts3, int n);
    // energy-based collisions of the (u,x) variant (admm_anderson_hard_zxu Solver.cpp:318-348)
    void add_obstacle(int type, const double* params);
    void set_collisions(const int* inds, int n);
    // PassiveMesh (PassiveObject.hpp:138-178) as a closed triangle surface (mesh_obstacle.hpp);
    // takes its place in add_obstacle's insertion order. Returns the mesh's row in the table.
    int add_mesh_obstacle(const double* verts3, int n_verts, const int* tris3, int n_tris);
    // Kinematic obstacles. A mesh's rigid pose (R row-major then t, null = unposed) for every
    // later iteration: one row of the device mesh table rewritten on the solver's stream, which
    // the captured graph reads at replay, so the graph stays. An analytic row re-parameterised in
    // place (index in the shared insertion order; type must match the stored one).
    void set_mesh_obstacle_pose(int mesh_id, const double* pose12);
    bool mesh_obstacle_pose(int mesh_id, double* pose12) const;
    // Deforming obstacles. New vertex positions for a mesh (same count, same triangles, obstacle
    // frame): validated on the host, then the BVH's bounds, the leaf triangles and the
    // pseudonormals refitted in place on the solver's stream (mesh_refit.hip) and the row's root
    // box rewritten; no buffer moves, so the graph stays. A refused call changes nothing.
    void set_mesh_obstacle_vertices(int mesh_id, const double* verts3);
    int mesh_obstacle_vertices(int mesh_id, double* verts3) const;   // returns the vertex count
    // Bound obstacles: vertex i of the mesh follows solver node nodes[i] (null = unbind, the shape
    // last in force stays). From then on every step() starts by gathering the vertices from the
    // step's start state on the device, checking them there (check_bound_refit) and, gated on the
    // outcome, refitting; the obstacle holds that shape for all iterations of the step. Nothing is
    // copied to or from the host and nothing waited for; the prologue is outside the graph.
    void bind_mesh_obstacle(int mesh_id, const int* nodes, int n_verts);
    void mesh_obstacle_status(int mesh_id, int* bound, int* refits, int* skipped, int* last_cause) const;
    // Exemption: the collision terms of the listed nodes skip this mesh (replaces the earlier list)
    void set_mesh_obstacle_exempt(int mesh_id, const int* nodes, int n);
    int num_obstacles() const { return (int)obstacles_.size(); }
    void set_obstacle(int index, int type, const double* params);
    // Coulomb friction against the obstacles (contact_friction.hpp): a coefficient per obstacle row
    // (index in the shared insertion order; before or after initialize, between steps: the pass is
    // outside the captured graph, which stays) and the per-term contact records of the last step.
    // The pass runs in a step iff some row has mu > 0 or recording is on. One rank only.
    void set_obstacle_friction(int index, double mu);
    double obstacle_friction(int index) const;
    void record_contacts(bool on);
    // Carry, per mesh, default off: the pass derives a carrying mesh's displacement at a contact from
    // its vertices' own motion since the previous step's pass (a deforming or bound mesh then drags
    // the nodes on it as a posed one does). Before or after initialize, between steps; the graph
    // stays. A solver in which no mesh carries launches the plain pass. One rank only.
    void set_mesh_obstacle_carry(int mesh_id, bool on);
    bool mesh_obstacle_carry(int mesh_id) const;
    // the last step's contact features, in contacts()'s order: the caller's triangle index (-1 for an
    // analytic row) and the barycentric weights; 0 when that step's pass was not the carry form
    int contact_features(int cap, int* tri, double* bary3);
    // the last step's terms in contact, in collision-term order; returns their count (every output
    // optional, at most cap entries written)
    int contacts(int cap, int* node, int* obstacle, double* point3, double* normal3, double* push, double* slip3,
                 double* scale);
    // WindForce (ExplicitForce.hpp:39-47) on the given triangles; returns its id
    int add_wind(const int* tris3, int ntris, const double* dir3);
    void set_wind(int id, const double* dir3);
    // multi-GPU: partition the mesh over comm's ranks at initialize(); every
    // rank passes the same scene. Not owned; must outlive the solver.
    void set_comm(Comm* c);
    void initialize(const aa_settings& s);
    void step();

    int num_nodes() const { return (int)x_.size() / 3; }
    void get_x(double* out);
    void get_v(double* out);
    void set_v(const double* v3);
    void set_x(const double* x3);
    int history(double* prim, double* comb, int* rej, int cap) const;
    int times(double* time_ms, int cap) const;
    void set_iterations(int admm_iters, double eps_rel);
    aa_runtime runtime() const { return rt_; }

    // benchmarking: run `iters` iterations of the ADMM loop body of a fresh time step;
    // returns device-synchronised wall ms. Per-kernel-class event timings are collected.
    double bench_iterations(int iters);
    bool kernel_stats(const std::string& name, double* avg_ms, double* bytes, int* launches) const;
    // the local-step work queue's diagnostics (kLqStats counters; 0 when not enabled); reset after
    int local_stats(long long* out, int cap, bool reset);
    const std::vector<std::pair<std::string, double>>& setup_phases() const { return setup_phases_; }

private:
    struct HostGroup {
        ElemKind kind;              // what G, vol and material hold for it: kind_traits (elastic_kernels.hpp)
        int material, nv, ncol;
        aa_lame lame;
        std::vector<int> idx;       // [count][nv] global node ids
        std::vector<double> G;      // [count][ncol][nv]
        std::vector<double> vol, w;
        // per-element materials ([count] each; empty = uniform, `lame` holds): k_e = lambda_e + (2/3) mu_e
        std::vector<double> mu_e, lambda_e, k_e, lmin_e, lmax_e;
        bool per_element() const { return !k_e.empty(); }
        // element t of `from` appended (the partitioned solver's split by owner)
        void append_element(const HostGroup& from, size_t t);
    };
    struct DevGroup {
        DevBuf<int> idx, spos;
        DevBuf<double> G, w, vol;
        DevBuf<double> mu_e, lambda_e, k_e, lmin_e, lmax_e;
        GroupDev d{};
        GroupVar var{};   // the arrays above; all null for a uniform group
    };
    Context* ctx_;
    hipStream_t s() const { return ctx_->stream; }

    // host model
    std::vector<double> x_, v_, m3_;
    std::vector<HostGroup> hgroups_;
    std::map<int, std::array<double, 3>> pins_;
    std::vector<std::array<double, kObsStride>> obstacles_;
    std::vector<int> coll_nodes_;   // collision-checked nodes (sorted, as the reference's map)
    struct Wind {
        std::vector<int> tris;      // user node ids
        double dir[3];
        DevBuf<int> dtris, dord, dlvl;
        int nlvl = 0;
    };
    std::vector<std::unique_ptr<Wind>> winds_;
    DevBuf<double> obs_dev_;
    // the tail of add_bending / add_springs / add_ties: the caller-numbered idx checked and offset,
    // G / vol / w moved into one new group; `who` is the caller's name in the message
    void add_one_col_group(ElemKind kind, int material, int nv, const std::vector<int>& idx, std::vector<double>&& G,
                           std::vector<double>&& vol, std::vector<double>&& w, int vertex_offset, const char* who);
    void upload_obstacles();
    // mesh obstacles: each one's BVH and pseudonormals, and the table of their device views the
    // mesh-aware collision prox indexes (kMaxMeshObstacles rows, allocated once: a fixed address,
    // so a captured graph stays valid when a later mesh fills another row)
    std::vector<std::unique_ptr<MeshObsBuffers>> meshes_;
    DevBuf<MeshObsDev> mesh_dev_;
    std::vector<MeshObsDev> mesh_rows_;   // the table's rows as last written
    // bound meshes: the device status words (one per row; the gate of that mesh's refit kernels)
    // and their host copies, fetched with the control block
    DevBuf<MeshBoundStatus> mesh_status_;
    std::vector<MeshBoundStatus> h_mesh_status_;
    MeshObsBuffers& mesh_at(int mesh_id, const std::string& who) const;
    void upload_mesh_binding(int mesh_id);
    void upload_mesh_exempt(int mesh_id);
    void refresh_bound_mesh(int mesh_id);   // host row lo / hi and host vertices from the device
    bool any_bound() const { for (auto& m : meshes_) if (m->bound) return true; return false; }
    const MeshObsDev* mesh_table(const GroupDev& d) const { return d.kind == kCollision && !meshes_.empty() ? mesh_dev_.p : nullptr; }
    void build_wind(Wind& w);
    // friction: the coefficients, the obstacle state in force during the previous step (host
    // snapshots, uploaded before the pass; valid once the pass has run in the step before), the
    // meshes whose vertices changed since, and the device records
    std::vector<double> fr_mu_;
    bool fr_record_ = false, fr_prev_valid_ = false, fr_ran_ = false;
    int fr_count_ = 0;
    std::vector<std::array<double, kObsStride>> obs_prev_;
    std::vector<MeshObsDev> mesh_rows_prev_;
    std::vector<unsigned char> mesh_changed_;
    std::vector<double> fr_h_obs_, fr_h_mu_;
    std::vector<MeshObsDev> fr_h_mesh_;
    std::vector<unsigned char> fr_h_still_;
    DevBuf<double> fr_obs_prev_, fr_mu_dev_;
    DevBuf<MeshObsDev> fr_mesh_prev_;
    DevBuf<unsigned char> fr_still_;
    DevBuf<int> rec_hit_, rec_row_;
    DevBuf<double> rec_c_, rec_n_, rec_j_, rec_rt_, rec_s_;
    // carry: the table the carry form reads (host snapshot and device copy), its feature records,
    // and whether the last step's pass was that form
    std::vector<MeshCarryDev> fr_h_carry_;
    DevBuf<MeshCarryDev> fr_carry_;
    DevBuf<int> rec_tri_;
    DevBuf<double> rec_b_;
    bool fr_carry_ran_ = false;
    bool any_carry() const { for (auto& m : meshes_) if (m->carry) return true; return false; }
    hipEvent_t fr_ev0_ = nullptr, fr_ev1_ = nullptr;   // around the pass (kernel_stats("friction"))
    hipEvent_t fr_ev2_ = nullptr;                      // after the carry snapshot copies (kernel_stats("carry_copy"))
    bool friction_active() const;
    void friction_enqueue(bool accel);
    std::vector<int> pin_order_;
    aa_settings st_{};
    bool initialized_ = false;

    // internal numbering: free nodes in nested-dissection order, then pinned (sorted)
    int n_ = 0, nf_ = 0, np_ = 0;
    long long Z_ = 0, Yslots_ = 0;
    std::vector<int> node2int_, int2node_;
    double pdt2_ = 0;

    // device
    std::vector<DevGroup> groups_;
    DirectSolver solver_;
    DevBuf<int> dt_ptr_;
    DevBuf<double> xs_, vs_, mass_, xfull_, xlast_, xbar_, Mxbar_, b_, b2_, cxfull_;
    DevBuf<double> z_, u_, y_, du_, dz_, dx_, lastz_, cz_;
    DevBuf<double> aa_cur_, aa_dF_, aa_dG_, aa_red_, aa_red_g_;
    // residual block partials: this rank's [a | b] (pa_, pb_) and their sums over the ranks
    // (ga_, gb_; aliases of pa_, pb_ on one GPU); nbg_ = the largest rank's block count
    DevBuf<double> red_ab_, red_gab_;
    double *pa_ = nullptr, *pb_ = nullptr, *ga_ = nullptr, *gb_ = nullptr, *aag_ = nullptr;
    int nbg_ = 0;
    DevBuf<Ctrl> ctrl_;
    DevBuf<int> lzq_;          // work-queue counter of the hyperelastic local step
    DevBuf<unsigned long long> lq_stats_;   // its diagnostics (AA_LQ_STATS=1)
    LocalQueue lq_;
    bool use_queue_ = true;
    DevBuf<double> hist_prim_, hist_comb_;
    DevBuf<int> hist_rej_;
    DevBuf<long long> hist_clock_;
    double clock_khz_ = 100000.0;
    std::vector<double> h_time_;
    int red_blocks_ = 0, aa_blocks_ = 0, hist_cap_ = 0;
    // partition: own free nodes [own_beg_, own_end_), shared top [top_beg_, nf_)
    Comm* comm_ = nullptr;
    int rank_ = 0, own_beg_ = 0, own_end_ = 0, top_beg_ = 0;
    void reduce_partials();
    void reduce_aa();
    void gather_state(DevBuf<double>& v);
    std::vector<double> h_prim_, h_comb_;
    std::vector<int> h_rej_;
    int nrec_ = 0;
    aa_runtime rt_{};
    std::vector<std::pair<std::string, double>> setup_phases_;   // last initialize(): (phase, ms)
    bool pins_dirty_ = true;

    // the whole ADMM loop of a time step, captured once into a hipGraph and replayed per step
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t gexec_ = nullptr;
    bool use_graph_ = true;
    bool pipe_z_ = false;   // Z variant + Anderson: comb solve batched with the next solve
    void drop_graph();
    // Concurrent combined-residual pass (pipelined Z variant, one GPU; AA_CONCURRENT=0 turns it
    // off): iteration k-1's pass runs on side_ beside iteration k, with its own control block,
    // partials and work-queue counter; default_{u,z,x} alternate between two buffers by
    // iteration parity so the pass reads k-1's while iteration k writes its own.
    bool conc_ = false;
    bool join_wait_ = false;
    double* join_dx_ = nullptr;
    void join_side();
    hipStream_t side_ = nullptr;
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
    DevBuf<Ctrl> ctrl_c_;
    DevBuf<int> lzq2_;
    LocalQueue lq2_;
    DevBuf<double> red_c_, du2_, dz2_, dx2_;
    double* du_at(int it) { return conc_ && (it & 1) ? du2_.p : du_.p; }
    double* dz_at(int it) { return conc_ && (it & 1) ? dz2_.p : dz_.p; }
    double* dx_at(int it) { return conc_ && (it & 1) ? dx2_.p : dx_.p; }
    // win_u_ (with conc_; AA_Z_WINDOW=0 turns it off): iteration `it` keeps its working u in
    // du_at(it) itself -- no default_u copy in the window beside the pass's local step, no restore
    // of u on a reject (the reject branch reads du_at(it - 1) where it lies); u_ is then unused
    bool win_u_ = false;
    double* u_at(int it) { return win_u_ ? du_at(it) : u_.p; }
    // the combined-residual pass forms its two residual sums per element inside its local step
    // (no z_c round trip through cz_); AA_COMB_FUSED=0: local step, then k_prim_z
    bool comb_fused_ = true;

    // kernel-class event timing (bench only)
    bool instrument_ = false;
    struct KStat { std::vector<hipEvent_t> ev; double bytes = 0; double total_ms = 0; int launches = 0; };
    std::map<std::string, KStat> kstats_;
    void ev_begin(const char* name);
    void ev_end(const char* name);

    void upload_pins();
    void prologue();
    void enqueue_iteration_ux(bool accel);
    void enqueue_iteration_z(bool accel, int it);
    void comb_finish_z(int op, hipStream_t st, Ctrl* c, double* pa, double* pb, const LocalQueue* q,
                       const double* du, const double* dz);
    void enqueue_comb_tail_z(int iters);
    void enqueue_iterations(int iters, bool accel);
    void epilogue_enqueue(bool accel);
    void fetch_results();
    int nb_elems() const { return red_blocks_; }
    void local_z_all(const double* xfull, const double* u, double* z, double* y, int mode, bool red);
};

}  // namespace aa
