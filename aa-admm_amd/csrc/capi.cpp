// extern "C" boundary (include/aa_admm.h). Every entry point catches and maps exceptions to
// status codes; the message is kept per thread for aa_last_error().
#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../../include/aa_admm.h"
#include "closest_query.hpp"
#include "comm.hpp"
#include "dense_gpu.hpp"
#include "elastic.hpp"
#include "geom.hpp"

struct aa_ctx_s { aa::Context c; };
struct aa_elastic_s { aa::ElasticSolver* s; aa_ctx_s* ctx; };
struct aa_geom_s { aa::GeomSolver* s; aa_ctx_s* ctx; };
struct aa_comm_s { std::unique_ptr<aa::Comm> c; };

static_assert(AA_MAX_MESH_OBSTACLES == aa::kMaxMeshObstacles && AA_OBS_MESH == aa::OBS_MESH, "aa_admm.h and the library agree");

namespace {
thread_local std::string g_err;

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return AA_OK;
    } catch (const aa::Error& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "out of host memory";
        return AA_ERR_DEVICE;
    } catch (const std::exception& e) {
        g_err = e.what();
        return AA_ERR_ARG;
    }
}

#define NEED(p, what) do { if (!(p)) throw aa::Error(AA_ERR_ARG, what); } while (0)
}  // namespace

extern "C" {

const char* aa_last_error(void) { return g_err.c_str(); }
const char* aa_version(void) { return "aa_admm 0.1 (gfx950)"; }

int aa_ctx_create(int device_id, aa_ctx* out) {
    return guarded([&] {
        NEED(out, "aa_ctx_create: null out");
        int n = 0;
        AA_HIP(hipGetDeviceCount(&n));
        if (device_id < 0 || device_id >= n) throw aa::Error(AA_ERR_ARG, "aa_ctx_create: no such device");
        AA_HIP(hipSetDevice(device_id));
        auto* c = new aa_ctx_s;
        c->c.device = device_id;
        AA_HIP(hipStreamCreateWithFlags(&c->c.stream, hipStreamNonBlocking));
        *out = c;
    });
}

int aa_ctx_destroy(aa_ctx ctx) {
    return guarded([&] {
        if (!ctx) return;
        (void)hipStreamSynchronize(ctx->c.stream);
        (void)hipStreamDestroy(ctx->c.stream);
        delete ctx;
    });
}

int aa_ctx_synchronize(aa_ctx ctx) {
    return guarded([&] { NEED(ctx, "null ctx"); AA_HIP(hipStreamSynchronize(ctx->c.stream)); });
}

int aa_ctx_bench_read(aa_ctx ctx, long long bytes, double* gbps) {
    return guarded([&] {
        NEED(ctx && gbps && bytes >= 16, "aa_ctx_bench_read: bad argument");
        AA_HIP(hipSetDevice(ctx->c.device));
        *gbps = aa::bench_stream_read(bytes, 10, ctx->c.stream);
    });
}

int aa_ctx_warm_dense(aa_ctx ctx, double* ms) {
    return guarded([&] {
        NEED(ctx && ms, "aa_ctx_warm_dense: bad argument");
        AA_HIP(hipSetDevice(ctx->c.device));
        *ms = aa::warm_gpu_front_backend(ctx->c.stream);
    });
}

int aa_lame_from_young(double k, double v, aa_lame* out) {
    return guarded([&] {
        NEED(out, "null out");
        out->mu = k / (2.0 * (1.0 + v));
        out->lambda = k * v / ((1.0 + v) * (1.0 - 2.0 * v));
        out->limit_min = -100.0;
        out->limit_max = 100.0;
    });
}

int aa_settings_default(aa_settings* s) {
    return guarded([&] {
        NEED(s, "null out");
        s->timestep_s = 1.0 / 30.0;
        s->verbose = 1;
        s->admm_iters = 500;
        s->gravity = -9.8;
        s->constraint_w = -1;
        s->anderson_m = 2;
        s->penalty = 1.0;
        s->acceleration_type = 0;
        s->variant = AA_VARIANT_UX;
        s->eps_rel = 0.0;
    });
}

int aa_elastic_create(aa_ctx ctx, aa_elastic* out) {
    return guarded([&] {
        NEED(ctx && out, "aa_elastic_create: null argument");
        AA_HIP(hipSetDevice(ctx->c.device));
        auto* h = new aa_elastic_s;
        h->ctx = ctx;
        h->s = new aa::ElasticSolver(&ctx->c);
        *out = h;
    });
}

int aa_elastic_destroy(aa_elastic h) {
    return guarded([&] {
        if (!h) return;
        (void)hipSetDevice(h->ctx->c.device);
        delete h->s;
        delete h;
    });
}

int aa_elastic_add_nodes(aa_elastic h, const double* x3, const double* m3, int n, int* total) {
    return guarded([&] {
        NEED(h, "null handle");
        int t = h->s->add_nodes(x3, m3, n);
        if (total) *total = t;
    });
}

int aa_elastic_add_tets(aa_elastic h, const double* verts3, const int* tets4, int n, int material, const aa_lame* lame,
                        int vertex_offset) {
    return guarded([&] {
        NEED(h && lame, "null argument");
        h->s->add_elements(aa::kTet, material, verts3, tets4, n, *lame, vertex_offset);
    });
}

int aa_elastic_add_tris(aa_elastic h, const double* verts3, const int* tris3, int n, const aa_lame* lame,
                        int vertex_offset) {
    return guarded([&] {
        NEED(h && lame, "null argument");
        h->s->add_elements(aa::kTri, AA_LINEAR, verts3, tris3, n, *lame, vertex_offset);
    });
}

int aa_elastic_add_tets_var(aa_elastic h, const double* verts3, const int* tets4, int n, int material,
                            const aa_lame* lame_per_tet, int vertex_offset) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(lame_per_tet || n <= 0, "add_tets_var: null material array");
        h->s->add_elements(aa::kTet, material, verts3, tets4, n, aa_lame{}, vertex_offset, n > 0 ? lame_per_tet : nullptr);
    });
}

int aa_elastic_add_tris_var(aa_elastic h, const double* verts3, const int* tris3, int n, const aa_lame* lame_per_tri,
                            int vertex_offset) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(lame_per_tri || n <= 0, "add_tris_var: null material array");
        h->s->add_elements(aa::kTri, AA_LINEAR, verts3, tris3, n, aa_lame{}, vertex_offset, n > 0 ? lame_per_tri : nullptr);
    });
}

int aa_elastic_add_bending(aa_elastic h, const double* verts3, const int* tris3, int n_tris, double k_bend,
                           int flat_rest, int vertex_offset, int* n_hinges) {
    return guarded([&] {
        NEED(h, "null handle");
        const int k = h->s->add_bending(verts3, tris3, n_tris, k_bend, flat_rest != 0, vertex_offset);
        if (n_hinges) *n_hinges = k;
    });
}

int aa_elastic_add_springs(aa_elastic h, const double* verts3, const int* pairs2, int n_springs, int mode, const double* k,
                           const double* rest, int vertex_offset) {
    return guarded([&] {
        NEED(h, "null handle");
        h->s->add_springs(verts3, pairs2, n_springs, mode, k, rest, vertex_offset);
    });
}

int aa_elastic_add_ties(aa_elastic h, const double* verts3, int na, const int* nodes_a, const double* w_a, int nb,
                        const int* nodes_b, const double* w_b, int n_ties, int mode, const double* k, const double* rest,
                        int vertex_offset) {
    return guarded([&] {
        NEED(h, "null handle");
        h->s->add_ties(verts3, na, nodes_a, w_a, nb, nodes_b, w_b, n_ties, mode, k, rest, vertex_offset);
    });
}

int aa_elastic_set_pins(aa_elastic h, const int* inds, const double* pts3, int n) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_pins(inds, pts3, n); });
}

int aa_elastic_add_obstacle(aa_elastic h, int type, const double* params) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->add_obstacle(type, params);
    });
}

int aa_elastic_add_mesh_obstacle(aa_elastic h, const double* verts3, int n_verts, const int* tris3, int n_tris, int* id) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        const int k = h->s->add_mesh_obstacle(verts3, n_verts, tris3, n_tris);
        if (id) *id = k;
    });
}

int aa_elastic_set_mesh_obstacle_pose(aa_elastic h, int mesh_id, const double pose12[12]) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->set_mesh_obstacle_pose(mesh_id, pose12);
    });
}

int aa_elastic_get_mesh_obstacle_pose(aa_elastic h, int mesh_id, double pose12[12], int* posed) {
    return guarded([&] {
        NEED(h, "null handle");
        const bool p = h->s->mesh_obstacle_pose(mesh_id, pose12);
        if (posed) *posed = p ? 1 : 0;
    });
}

int aa_elastic_set_mesh_obstacle_vertices(aa_elastic h, int mesh_id, const double* verts3) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->set_mesh_obstacle_vertices(mesh_id, verts3);
    });
}

int aa_elastic_get_mesh_obstacle_vertices(aa_elastic h, int mesh_id, double* verts3, int* n_verts) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        const int n = h->s->mesh_obstacle_vertices(mesh_id, verts3);
        if (n_verts) *n_verts = n;
    });
}

int aa_elastic_bind_mesh_obstacle(aa_elastic h, int mesh_id, const int* nodes, int n_verts) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->bind_mesh_obstacle(mesh_id, nodes, n_verts);
    });
}

int aa_elastic_mesh_obstacle_status(aa_elastic h, int mesh_id, int* bound, int* refits, int* skipped, int* last_cause) {
    return guarded([&] {
        NEED(h, "null handle");
        h->s->mesh_obstacle_status(mesh_id, bound, refits, skipped, last_cause);
    });
}

int aa_elastic_set_mesh_obstacle_exempt(aa_elastic h, int mesh_id, const int* nodes, int n) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->set_mesh_obstacle_exempt(mesh_id, nodes, n);
    });
}

int aa_elastic_num_obstacles(aa_elastic h, int* n) {
    return guarded([&] { NEED(h && n, "null argument"); *n = h->s->num_obstacles(); });
}

int aa_elastic_set_obstacle(aa_elastic h, int index, int type, const double* params) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->set_obstacle(index, type, params);
    });
}

int aa_elastic_set_obstacle_friction(aa_elastic h, int index, double mu) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_obstacle_friction(index, mu); });
}

int aa_elastic_get_obstacle_friction(aa_elastic h, int index, double* mu) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(mu, "aa_elastic_get_obstacle_friction: null mu");
        *mu = h->s->obstacle_friction(index);
    });
}

int aa_elastic_record_contacts(aa_elastic h, int on) {
    return guarded([&] { NEED(h, "null handle"); h->s->record_contacts(on != 0); });
}

int aa_elastic_get_contacts(aa_elastic h, int cap, int* n, int* node, int* obstacle, double* point3, double* normal3,
                            double* push, double* slip3, double* scale) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(n, "aa_elastic_get_contacts: null n");
        NEED(cap >= 0, "aa_elastic_get_contacts: negative cap");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        *n = h->s->contacts(cap, node, obstacle, point3, normal3, push, slip3, scale);
    });
}

int aa_elastic_set_mesh_obstacle_carry(aa_elastic h, int mesh_id, int on) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->set_mesh_obstacle_carry(mesh_id, on != 0);
    });
}

int aa_elastic_get_mesh_obstacle_carry(aa_elastic h, int mesh_id, int* on) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(on, "aa_elastic_get_mesh_obstacle_carry: null on");
        *on = h->s->mesh_obstacle_carry(mesh_id) ? 1 : 0;
    });
}

int aa_elastic_get_contact_features(aa_elastic h, int cap, int* n, int* tri, double* bary3) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(n, "aa_elastic_get_contact_features: null n");
        NEED(cap >= 0, "aa_elastic_get_contact_features: negative cap");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        *n = h->s->contact_features(cap, tri, bary3);
    });
}

int aa_elastic_set_collisions(aa_elastic h, const int* inds, int n) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_collisions(inds, n); });
}

int aa_elastic_add_wind(aa_elastic h, const int* tris3, int n_tris, const double dir3[3], int* id) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        const int k = h->s->add_wind(tris3, n_tris, dir3);
        if (id) *id = k;
    });
}

int aa_elastic_set_wind(aa_elastic h, int id, const double dir3[3]) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_wind(id, dir3); });
}

int aa_elastic_initialize(aa_elastic h, const aa_settings* s) {
    return guarded([&] {
        NEED(h && s, "null argument");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->initialize(*s);
    });
}

int aa_elastic_step(aa_elastic h) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->step();
    });
}

int aa_elastic_num_nodes(aa_elastic h, int* n) {
    return guarded([&] { NEED(h && n, "null argument"); *n = h->s->num_nodes(); });
}

int aa_elastic_get_x(aa_elastic h, double* x3) {
    return guarded([&] { NEED(h && x3, "null argument"); h->s->get_x(x3); });
}

int aa_elastic_get_v(aa_elastic h, double* v3) {
    return guarded([&] { NEED(h && v3, "null argument"); h->s->get_v(v3); });
}

int aa_elastic_set_v(aa_elastic h, const double* v3) {
    return guarded([&] { NEED(h && v3, "null argument"); h->s->set_v(v3); });
}

int aa_elastic_set_x(aa_elastic h, const double* x3) {
    return guarded([&] { NEED(h && x3, "null argument"); h->s->set_x(x3); });
}

int aa_elastic_get_history(aa_elastic h, double* prim, double* comb, int* reject, int cap, int* n) {
    return guarded([&] {
        NEED(h, "null handle");
        int k = h->s->history(prim, comb, reject, cap);
        if (n) *n = k;
    });
}

int aa_elastic_set_iterations(aa_elastic h, int admm_iters, double eps_rel) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_iterations(admm_iters, eps_rel); });
}

int aa_elastic_get_times(aa_elastic h, double* time_ms, int cap, int* n) {
    return guarded([&] {
        NEED(h, "null handle");
        int k = h->s->times(time_ms, cap);
        if (n) *n = k;
    });
}

int aa_elastic_runtime(aa_elastic h, aa_runtime* out) {
    return guarded([&] { NEED(h && out, "null argument"); *out = h->s->runtime(); });
}

int aa_runtime_libraries(char* buf, long long cap, long long* len) {
    return guarded([&] {
        std::string s = aa::runtime_libraries();
        if (len) *len = (long long)s.size();
        if (buf && cap > 0) {
            size_t k = std::min((size_t)(cap - 1), s.size());
            std::memcpy(buf, s.data(), k);
            buf[k] = 0;
        }
    });
}

int aa_comm_unique_id(unsigned char id[128]) {
    return guarded([&] { NEED(id, "null argument"); aa::rccl_unique_id(id); });
}

int aa_comm_create_rccl(aa_ctx ctx, const unsigned char id[128], int rank, int size, aa_comm* out) {
    return guarded([&] {
        NEED(ctx && id && out, "null argument");
        NEED(size >= 1 && rank >= 0 && rank < size, "aa_comm_create_rccl: bad rank/size");
        AA_HIP(hipSetDevice(ctx->c.device));
        auto* c = new aa_comm_s;
        try { c->c = aa::make_rccl_comm(id, rank, size); } catch (...) { delete c; throw; }
        *out = c;
    });
}

int aa_comm_create_host(aa_host_allreduce_fn fn, void* user, int rank, int size, aa_comm* out) {
    return guarded([&] {
        NEED(fn && out, "null argument");
        NEED(size >= 1 && rank >= 0 && rank < size, "aa_comm_create_host: bad rank/size");
        auto* c = new aa_comm_s;
        c->c = aa::make_host_comm(fn, user, rank, size);
        *out = c;
    });
}

int aa_comm_create_solo(int rank, int size, aa_comm* out) {
    return guarded([&] {
        NEED(out, "aa_comm_create_solo: null out");
        NEED(size >= 1 && rank >= 0 && rank < size, "aa_comm_create_solo: bad rank/size");
        auto* c = new aa_comm_s;
        c->c = aa::make_solo_comm(rank, size);
        *out = c;
    });
}

int aa_comm_destroy(aa_comm c) {
    return guarded([&] { delete c; });
}

int aa_comm_info(aa_comm c, int* rank, int* size) {
    return guarded([&] {
        NEED(c, "null handle");
        if (rank) *rank = c->c->rank();
        if (size) *size = c->c->size();
    });
}

int aa_comm_allreduce_host(aa_comm c, double* buf, long long n) {
    return guarded([&] {
        NEED(c && (n == 0 || buf) && n >= 0, "bad argument");
        c->c->allreduce_sum_host(buf, (size_t)n);
    });
}

int aa_elastic_set_comm(aa_elastic h, aa_comm c) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_comm(c ? c->c.get() : nullptr); });
}

int aa_geom_set_comm(aa_geom h, aa_comm c) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_comm(c ? c->c.get() : nullptr); });
}

int aa_elastic_bench_iterations(aa_elastic h, int iters, double* ms) {
    return guarded([&] {
        NEED(h && iters >= 0, "bad argument");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        double t = h->s->bench_iterations(iters);
        if (ms) *ms = t;
    });
}

int aa_elastic_kernel_stats(aa_elastic h, const char* name, double* avg_ms, double* bytes, int* launches) {
    return guarded([&] {
        NEED(h && name, "null argument");
        if (!h->s->kernel_stats(name, avg_ms, bytes, launches)) throw aa::Error(AA_ERR_ARG, std::string("no kernel class ") + name);
    });
}

int aa_elastic_local_stats(aa_elastic h, long long* out, int cap, int reset, int* count) {
    return guarded([&] {
        NEED(h && out && cap >= 0, "bad argument");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        const int n = h->s->local_stats(out, cap, reset != 0);
        if (count) *count = n;
    });
}

int aa_elastic_setup_phases(aa_elastic h, char* names, int names_cap, double* ms, int cap, int* count) {
    return guarded([&] {
        NEED(h && cap >= 0 && names_cap >= 0, "bad argument");
        const auto& ph = h->s->setup_phases();
        std::string all;
        for (size_t i = 0; i < ph.size(); ++i) {
            if (i) all += '\n';
            all += ph[i].first;
            if ((int)i < cap && ms) ms[i] = ph[i].second;
        }
        if (names && names_cap > 0) {
            const size_t k = std::min(all.size(), (size_t)names_cap - 1);
            std::memcpy(names, all.data(), k);
            names[k] = 0;
        }
        if (count) *count = (int)ph.size();
    });
}

// ---- Geometry (ALMGeometrySolver<3>) -------------------------------------------------------
int aa_geom_create(aa_ctx ctx, aa_geom* out) { return aa_geom_create_kind(ctx, AA_GEOM_ALM, out); }

int aa_geom_create_kind(aa_ctx ctx, int kind, aa_geom* out) {
    return guarded([&] {
        NEED(ctx && out, "aa_geom_create: null argument");
        NEED(kind == AA_GEOM_ALM || kind == AA_GEOM_PLAIN, "aa_geom_create_kind: unknown solver kind");
        AA_HIP(hipSetDevice(ctx->c.device));
        auto* h = new aa_geom_s;
        h->ctx = ctx;
        h->s = new aa::GeomSolver(&ctx->c, kind == AA_GEOM_PLAIN);
        *out = h;
    });
}

int aa_geom_destroy(aa_geom h) {
    return guarded([&] {
        if (!h) return;
        (void)hipSetDevice(h->ctx->c.device);
        delete h->s;
        delete h;
    });
}

int aa_geom_add_ref_surface(aa_geom h, const double* V3, int nv, const int* F3, int nf, int* id) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        const int i = h->s->add_ref_surface(V3, nv, F3, nf);
        if (id) *id = i;
    });
}

int aa_geom_add_constraints(aa_geom h, int hard, int type, const int* idx, int k, int count, double weight,
                            const double* params) {
    return guarded([&] { NEED(h, "null handle"); h->s->add_constraints(hard, type, idx, k, count, weight, params); });
}

int aa_geom_add_laplacian(aa_geom h, const int* idx, const double* coefs, int k, double weight, const double* ref3) {
    return guarded([&] { NEED(h, "null handle"); h->s->add_laplacian(idx, coefs, k, weight, ref3); });
}

int aa_geom_add_closeness(aa_geom h, int idx, double weight, const double* target3) {
    return guarded([&] { NEED(h, "null handle"); h->s->add_closeness(idx, weight, target3); });
}

int aa_geom_add_laplacians(aa_geom h, int n_rows, const int* row_ptr, const int* idx, const double* coefs,
                           const double* weights, const int* relative, const double* ref_points3) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(n_rows >= 0 && (n_rows == 0 || (row_ptr && idx && coefs && weights)), "bad laplacian rows");
        for (int r = 0; r < n_rows; ++r) {
            const int a = row_ptr[r], k = row_ptr[r + 1] - a;
            NEED(k > 0, "empty laplacian row");
            const bool rel = relative && relative[r];
            NEED(!rel || ref_points3, "relative laplacian row without reference points");
            h->s->add_laplacian(idx + a, coefs + a, k, weights[r], rel ? ref_points3 : nullptr);
        }
    });
}

int aa_geom_add_closenesses(aa_geom h, int n, const int* idx, const double* weights, const double* targets3) {
    return guarded([&] {
        NEED(h, "null handle");
        NEED(n >= 0 && (n == 0 || (idx && weights && targets3)), "bad closeness rows");
        for (int r = 0; r < n; ++r) h->s->add_closeness(idx[r], weights[r], targets3 + 3 * (size_t)r);
    });
}

int aa_geom_setup(aa_geom h, int n_points, double penalty, int spd_solver_type) {
    return guarded([&] { NEED(h, "null handle"); h->s->setup(n_points, penalty, spd_solver_type); });
}

int aa_geom_solve(aa_geom h, const double* init_x3, double rel_eps, int max_iter, int m) {
    return guarded([&] {
        NEED(h, "null handle");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->solve(init_x3, rel_eps, max_iter, m);
    });
}

int aa_geom_set_stop(aa_geom h, int stop_at_eps, double eps_rel) {
    return guarded([&] { NEED(h, "null handle"); h->s->set_stop(stop_at_eps, eps_rel); });
}

int aa_geom_get_solution(aa_geom h, double* x3) {
    return guarded([&] { NEED(h && x3, "null argument"); h->s->get_solution(x3); });
}

int aa_geom_get_history(aa_geom h, double* comb, double* time_s, int cap, int* n) {
    return guarded([&] {
        NEED(h, "null handle");
        const int k = h->s->history(comb, time_s, cap);
        if (n) *n = k;
    });
}

int aa_geom_runtime_info(aa_geom h, aa_geom_runtime* out) {
    return guarded([&] { NEED(h && out, "null argument"); *out = h->s->runtime(); });
}

int aa_geom_closest_points(aa_geom h, int surface, const double* p3, int n, double* out3) {
    return guarded([&] {
        NEED(h && (n == 0 || (p3 && out3)), "null argument");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        h->s->closest_points(surface, p3, n, out3);
    });
}

int aa_geom_bench_iterations(aa_geom h, int iters, double* ms) {
    return guarded([&] {
        NEED(h && iters >= 0, "bad argument");
        AA_HIP(hipSetDevice(h->ctx->c.device));
        const double t = h->s->bench_iterations(iters);
        if (ms) *ms = t;
    });
}

int aa_geom_kernel_stats(aa_geom h, const char* name, double* avg_ms, double* bytes, int* launches) {
    return guarded([&] {
        NEED(h && name, "null argument");
        if (!h->s->kernel_stats(name, avg_ms, bytes, launches)) throw aa::Error(AA_ERR_ARG, std::string("no kernel class ") + name);
    });
}

int aa_closest_on_triangles(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris, const double* q3,
                            int n, double* closest3, int* tri, double* bary3) {
    return guarded([&] {
        NEED(ctx, "null context");
        NEED(n >= 0 && (n == 0 || q3), "closest_on_triangles: bad argument");
        const aa::ClosestSurfaceHost M = aa::prepare_closest_surface(verts3, n_verts, tris3, n_tris);
        aa::validate_closest_queries(q3, n);
        if (n == 0) return;
        AA_HIP(hipSetDevice(ctx->c.device));
        hipStream_t s = ctx->c.stream;
        aa::DevBuf<aa::BvhNode> nodes;
        aa::DevBuf<aa::BvhTri> tris;
        aa::DevBuf<int> orig, dt(n);
        aa::DevBuf<double> dq, dc((size_t)3 * n), db((size_t)3 * n);
        nodes.upload(M.nodes, s);
        tris.upload(M.tris, s);
        orig.upload(M.orig, s);
        dq.upload(q3, (size_t)3 * n, s);
        aa::SurfDev S{};
        S.nodes = nodes.p; S.tris = tris.p;
        S.n_nodes = (int)M.nodes.size(); S.n_tris = (int)M.tris.size();
        aa::launch_closest_on_triangles(S, orig.p, dq.p, n, dc.p, dt.p, db.p, s);
        if (closest3) AA_HIP(hipMemcpyAsync(closest3, dc.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        if (tri) AA_HIP(hipMemcpyAsync(tri, dt.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        if (bary3) AA_HIP(hipMemcpyAsync(bary3, db.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"

// ---- element-level test hooks (tests only): device prox / COD / projections on host arrays ----
namespace {
template <class F>
int with_device_arrays(aa_ctx ctx, F&& f) {
    return guarded([&] {
        NEED(ctx, "null context");
        AA_HIP(hipSetDevice(ctx->c.device));
        f(ctx->c.stream);
        AA_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}
}  // namespace

extern "C" int aa_test_prox(aa_ctx ctx, int op, const double* prm4, const double* in, int n, double* out, int* iters) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        NEED(prm4 && in && out && n >= 0 && op >= 0 && op <= 6, "aa_test_prox: bad argument");
        const int D = op >= 5 ? 3 : op >= 3 ? 6 : 9;
        aa::DevBuf<double> di, dout((size_t)D * std::max(n, 1));
        aa::DevBuf<int> dit(std::max(n, 1));
        di.upload(in, (size_t)D * n, s);
        if (op >= 5) AA_HIP(hipMemsetAsync(dit.p, 0, sizeof(int) * std::max(n, 1), s));   // closed form: no iterations
        aa::launch_test_prox(op, prm4, di.p, n, dout.p, dit.p, s);
        AA_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * D * n, hipMemcpyDeviceToHost, s));
        if (iters) AA_HIP(hipMemcpyAsync(iters, dit.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int aa_test_mesh_sdf(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                               const double* q3, int n, double* closest3, double* dx, int* tri) {
    return aa_test_mesh_sdf_posed(ctx, verts3, n_verts, tris3, n_tris, nullptr, q3, n, closest3, dx, tri);
}

extern "C" int aa_test_mesh_sdf_posed(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                                     const double* pose12, const double* q3, int n, double* closest3, double* dx,
                                     int* tri) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        NEED(q3 && closest3 && dx && tri && n >= 0, "aa_test_mesh_sdf: bad argument");
        const aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(verts3, n_verts, tris3, n_tris);
        if (pose12) aa::validate_mesh_pose(pose12, "aa_test_mesh_sdf_posed: ");
        aa::MeshObsBuffers buf;
        aa::MeshObsDev d = buf.upload(M, s);
        aa::apply_mesh_pose(d, pose12);
        aa::DevBuf<aa::MeshObsDev> dd;
        dd.upload(&d, 1, s);
        aa::DevBuf<double> dq, dc((size_t)3 * std::max(n, 1)), ddx(std::max(n, 1));
        aa::DevBuf<int> dt(std::max(n, 1));
        dq.upload(q3, (size_t)3 * n, s);
        aa::launch_test_mesh_sdf(dd.p, dq.p, n, dc.p, ddx.p, dt.p, s);
        AA_HIP(hipMemcpyAsync(closest3, dc.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(dx, ddx.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(tri, dt.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int aa_test_mesh_refit_tables(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                                        const double* new_verts3, int device, void* nodes_bytes, double* tris9,
                                        double* pn21, int* orig, double* lohi6, int* n_nodes) {
    auto give = [&](const aa::MeshObstacleHost& M) {
        if (nodes_bytes) std::memcpy(nodes_bytes, M.nodes.data(), sizeof(aa::BvhNode) * M.nodes.size());
        if (tris9) std::memcpy(tris9, M.tris.data(), sizeof(aa::BvhTri) * M.tris.size());
        if (pn21) std::copy(M.pn.begin(), M.pn.end(), pn21);
        if (orig) std::copy(M.orig.begin(), M.orig.end(), orig);
        if (lohi6) for (int d = 0; d < 3; ++d) { lohi6[d] = M.lo[d]; lohi6[3 + d] = M.hi[d]; }
        if (n_nodes) *n_nodes = (int)M.nodes.size();
    };
    const std::string who = "aa_test_mesh_refit_tables: ";
    if (!device)
        return guarded([&] {
            aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(verts3, n_verts, tris3, n_tris);
            if (new_verts3) {
                const aa::MeshRefitTables T = aa::make_refit_tables(M, n_verts, tris3, n_tris);
                double lo[3], hi[3];
                aa::validate_mesh_refit(T, new_verts3, who, lo, hi);
                aa::refit_mesh_obstacle_host(M, T, new_verts3);
            }
            give(M);
        });
    return with_device_arrays(ctx, [&](hipStream_t s) {
        aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(verts3, n_verts, tris3, n_tris);
        aa::MeshObsBuffers buf;
        buf.upload(M, s);
        if (new_verts3) {
            buf.keep_for_refit(M, verts3, n_verts, tris3, n_tris, s);
            validate_mesh_refit(buf.tables, new_verts3, who, M.lo, M.hi);
            buf.refit(new_verts3, s);
        }
        AA_HIP(hipMemcpyAsync(M.nodes.data(), buf.nodes.p, buf.nodes.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(M.tris.data(), buf.tris.p, buf.tris.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(M.pn.data(), buf.pn.p, buf.pn.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(M.orig.data(), buf.orig.p, buf.orig.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
        give(M);
    });
}

namespace {
// median of 5 event-timed runs of f on s after one warm-up, in ms
template <class F>
double median5_ms(hipStream_t s, F&& f) {
    hipEvent_t e0, e1;
    AA_HIP(hipEventCreate(&e0));
    AA_HIP(hipEventCreate(&e1));
    float t[5];
    f();
    AA_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < 5; ++r) {
        AA_HIP(hipEventRecord(e0, s));
        f();
        AA_HIP(hipEventRecord(e1, s));
        AA_HIP(hipEventSynchronize(e1));
        AA_HIP(hipEventElapsedTime(&t[r], e0, e1));
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    std::sort(t, t + 5);
    return t[2];
}
}  // namespace

extern "C" int aa_test_bound_refit(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                                  const double* x3, int n_nodes_x, const int* nodes, int device, void* nodes_bytes,
                                  double* tris9, double* pn21, int* orig, double* lohi6, int* n_nodes, int* status2,
                                  double* vol6, double* ms, const double* x3_first) {
    auto give = [&](const aa::MeshObstacleHost& M) {
        if (nodes_bytes) std::memcpy(nodes_bytes, M.nodes.data(), sizeof(aa::BvhNode) * M.nodes.size());
        if (tris9) std::memcpy(tris9, M.tris.data(), sizeof(aa::BvhTri) * M.tris.size());
        if (pn21) std::copy(M.pn.begin(), M.pn.end(), pn21);
        if (orig) std::copy(M.orig.begin(), M.orig.end(), orig);
        if (lohi6) for (int d = 0; d < 3; ++d) { lohi6[d] = M.lo[d]; lohi6[3 + d] = M.hi[d]; }
        if (n_nodes) *n_nodes = (int)M.nodes.size();
    };
    auto check_args = [&] {
        NEED(x3 && nodes && n_nodes_x > 0, "aa_test_bound_refit: null argument");
        for (int i = 0; i < n_verts; ++i)
            NEED(nodes[i] >= 0 && nodes[i] < n_nodes_x, "aa_test_bound_refit: node index out of range");
    };
    if (!device)
        return guarded([&] {
            aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(verts3, n_verts, tris3, n_tris);
            check_args();
            const aa::MeshRefitTables T = aa::make_refit_tables(M, n_verts, tris3, n_tris);
            double v6 = 0;
            if (x3_first) aa::bound_refit_host(M, T, x3_first, nodes, &v6);   // an earlier step's refit, taken or refused
            const int cause = aa::bound_refit_host(M, T, x3, nodes, &v6);
            if (status2) { status2[0] = cause == aa::BOUND_OK; status2[1] = cause; }
            if (vol6) *vol6 = v6;
            give(M);
        });
    return with_device_arrays(ctx, [&](hipStream_t s) {
        aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(verts3, n_verts, tris3, n_tris);
        check_args();
        aa::MeshObsBuffers buf;
        aa::MeshObsDev d = buf.upload(M, s);
        aa::apply_mesh_pose(d, nullptr);
        buf.keep_for_refit(M, verts3, n_verts, tris3, n_tris, s);
        buf.rf.bind(buf.tables, nodes, verts3, s);   // the caller's numbering is the internal one here
        aa::DevBuf<aa::MeshObsDev> row;
        row.upload(&d, 1, s);
        aa::DevBuf<aa::MeshBoundStatus> st(1);
        st.zero(s);
        aa::DevBuf<double> xs, xs_first;
        if (x3_first) {   // an earlier step's refit, taken or refused
            xs_first.upload(x3_first, 3 * (size_t)n_nodes_x, s);
            buf.rf.bound_refit(xs_first.p, row.p, st.p, buf.nodes.p, (int)buf.nodes.n, buf.tris.p, buf.pn.p, s);
        }
        xs.upload(x3, 3 * (size_t)n_nodes_x, s);
        buf.rf.bound_refit(xs.p, row.p, st.p, buf.nodes.p, (int)buf.nodes.n, buf.tris.p, buf.pn.p, s);
        aa::MeshBoundStatus hs;
        AA_HIP(hipMemcpyAsync(M.nodes.data(), buf.nodes.p, buf.nodes.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(M.tris.data(), buf.tris.p, buf.tris.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(M.pn.data(), buf.pn.p, buf.pn.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(M.orig.data(), buf.orig.p, buf.orig.bytes(), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(&d, row.p, sizeof(d), hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(&hs, st.p, sizeof(hs), hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < 3; ++k) { M.lo[k] = d.lo[k]; M.hi[k] = d.hi[k]; }
        if (status2) { status2[0] = hs.skip ? 0 : 1; status2[1] = hs.cause; }
        if (vol6) *vol6 = hs.vol6;
        give(M);
        if (ms) *ms = median5_ms(s, [&] { buf.rf.bound_refit(xs.p, row.p, st.p, buf.nodes.p, (int)buf.nodes.n, buf.tris.p, buf.pn.p, s); });
    });
}

extern "C" int aa_test_mesh_sdf_deformed(aa_ctx ctx, const double* verts3, int n_verts, const int* tris3, int n_tris,
                                        const double* new_verts3, const double* pose12, const double* q3, int n,
                                        double* closest3, double* dx, int* tri, double* ms4) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        const std::string who = "aa_test_mesh_sdf_deformed: ";
        NEED(new_verts3 && q3 && closest3 && dx && tri && n >= 0, "aa_test_mesh_sdf_deformed: bad argument");
        const aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(verts3, n_verts, tris3, n_tris);
        if (pose12) aa::validate_mesh_pose(pose12, who);
        aa::MeshObsBuffers buf;
        aa::MeshObsDev d = buf.upload(M, s);
        buf.keep_for_refit(M, verts3, n_verts, tris3, n_tris, s);
        validate_mesh_refit(buf.tables, new_verts3, who, d.lo, d.hi);
        buf.refit(new_verts3, s);
        aa::apply_mesh_pose(d, pose12);
        aa::DevBuf<aa::MeshObsDev> dd;
        dd.upload(&d, 1, s);
        aa::DevBuf<double> dq, dc((size_t)3 * std::max(n, 1)), ddx(std::max(n, 1));
        aa::DevBuf<int> dt(std::max(n, 1));
        dq.upload(q3, (size_t)3 * n, s);
        aa::launch_test_mesh_sdf(dd.p, dq.p, n, dc.p, ddx.p, dt.p, s);
        AA_HIP(hipMemcpyAsync(closest3, dc.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(dx, ddx.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipMemcpyAsync(tri, dt.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
        if (!ms4) return;
        // 1: what the parent offers instead -- prepare on the host and upload, from scratch (wall)
        aa::MeshObsBuffers fresh;
        aa::MeshObsDev df;
        const auto t0 = std::chrono::steady_clock::now();
        {
            const aa::MeshObstacleHost Mf = aa::prepare_mesh_obstacle(new_verts3, n_verts, tris3, n_tris);
            df = fresh.upload(Mf, s);
            AA_HIP(hipStreamSynchronize(s));
        }
        ms4[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        aa::apply_mesh_pose(df, pose12);
        aa::DevBuf<aa::MeshObsDev> ddf;
        ddf.upload(&df, 1, s);
        // 2: the device refit (staging copy included); 3, 4: the walk on the refitted / the fresh tree
        ms4[1] = median5_ms(s, [&] { buf.refit(new_verts3, s); });
        ms4[2] = median5_ms(s, [&] { aa::launch_test_mesh_sdf(dd.p, dq.p, n, dc.p, ddx.p, dt.p, s); });
        ms4[3] = median5_ms(s, [&] { aa::launch_test_mesh_sdf(ddf.p, dq.p, n, dc.p, ddx.p, dt.p, s); });
    });
}

extern "C" int aa_test_collision_prox(aa_ctx ctx, const double* obs_rows, int n_obs, const double* mesh_verts3,
                                     const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr,
                                     int n_meshes, const double* q3, int n, double* out3) {
    return aa_test_collision_prox_posed(ctx, obs_rows, n_obs, mesh_verts3, mesh_vert_ptr, mesh_tris3, mesh_tri_ptr,
                                        n_meshes, nullptr, q3, n, out3);
}

extern "C" int aa_test_collision_prox_posed(aa_ctx ctx, const double* obs_rows, int n_obs, const double* mesh_verts3,
                                           const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr,
                                           int n_meshes, const double* mesh_poses, const double* q3, int n,
                                           double* out3) {
    return aa_test_collision_prox_exempt(ctx, obs_rows, n_obs, mesh_verts3, mesh_vert_ptr, mesh_tris3, mesh_tri_ptr, n_meshes,
                                         mesh_poses, q3, nullptr, n, nullptr, nullptr, out3);
}

extern "C" int aa_test_collision_prox_exempt(aa_ctx ctx, const double* obs_rows, int n_obs, const double* mesh_verts3,
                                            const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr,
                                            int n_meshes, const double* mesh_poses, const double* q3, const int* q_node,
                                            int n, const int* exempt_ptr, const int* exempt_nodes, double* out3) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        // q_node null: the form without nodes (aa_test_collision_prox_posed), no exemption
        NEED(!q_node || (exempt_ptr && (exempt_nodes || exempt_ptr[std::max(n_meshes, 0)] == 0)), "aa_test_collision_prox_exempt: null exempt lists");
        int n_ids = 1;
        if (q_node) {
            for (int e = 0; e < n; ++e) {
                NEED(q_node[e] >= 0, "aa_test_collision_prox_exempt: negative node id");
                n_ids = std::max(n_ids, q_node[e] + 1);
            }
            for (int m = 0; m < n_meshes; ++m) NEED(exempt_ptr[m + 1] >= exempt_ptr[m], "aa_test_collision_prox_exempt: bad exempt_ptr");
            for (int j = 0; j < exempt_ptr[n_meshes]; ++j) {
                NEED(exempt_nodes[j] >= 0, "aa_test_collision_prox_exempt: negative node id");
                n_ids = std::max(n_ids, exempt_nodes[j] + 1);
            }
        }
        std::vector<std::unique_ptr<aa::DevBuf<unsigned char>>> ebufs;
        NEED(q3 && out3 && n >= 0 && n_obs >= 0 && n_obs <= aa::kMaxObstacles && (obs_rows || n_obs == 0),
             "aa_test_collision_prox: bad argument");
        NEED(n_meshes >= 0 && n_meshes <= aa::kMaxMeshObstacles, "aa_test_collision_prox: too many mesh obstacles");
        NEED(n_meshes == 0 || (mesh_verts3 && mesh_vert_ptr && mesh_tris3 && mesh_tri_ptr), "aa_test_collision_prox: null mesh arrays");
        std::vector<std::unique_ptr<aa::MeshObsBuffers>> bufs;
        std::vector<aa::MeshObsDev> table((size_t)std::max(n_meshes, 1));
        for (int m = 0; m < n_meshes; ++m) {
            const aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(
                mesh_verts3 + 3 * (size_t)mesh_vert_ptr[m], mesh_vert_ptr[m + 1] - mesh_vert_ptr[m],
                mesh_tris3 + 3 * (size_t)mesh_tri_ptr[m], mesh_tri_ptr[m + 1] - mesh_tri_ptr[m]);
            bufs.push_back(std::make_unique<aa::MeshObsBuffers>());
            table[m] = bufs.back()->upload(M, s);
            const double* pose = mesh_poses ? mesh_poses + 12 * (size_t)m : nullptr;
            if (pose && std::all_of(pose, pose + 12, [](double v) { return std::isnan(v); })) pose = nullptr;   // this mesh unposed
            if (pose) aa::validate_mesh_pose(pose, "aa_test_collision_prox_posed: ");
            aa::apply_mesh_pose(table[m], pose);
            if (q_node && exempt_ptr[m + 1] > exempt_ptr[m]) {
                std::vector<unsigned char> bytes((size_t)n_ids, 0);
                for (int j = exempt_ptr[m]; j < exempt_ptr[m + 1]; ++j) bytes[exempt_nodes[j]] = 1;
                ebufs.push_back(std::make_unique<aa::DevBuf<unsigned char>>());
                ebufs.back()->upload(bytes, s);
                AA_HIP(hipStreamSynchronize(s));
                table[m].exempt = ebufs.back()->p;
            }
        }
        std::vector<double> h(1 + (size_t)aa::kObsStride * n_obs, 0.0);
        h[0] = n_obs;
        for (int k = 0; k < n_obs; ++k) {
            const double* o = obs_rows + (size_t)aa::kObsStride * k;
            const int type = (int)o[0];
            NEED(type >= aa::OBS_FLOOR && type <= aa::OBS_MESH, "aa_test_collision_prox: unknown obstacle type");
            NEED(type != aa::OBS_MESH || (o[1] >= 0 && o[1] < n_meshes && o[1] == (int)o[1]), "aa_test_collision_prox: mesh id out of range");
            std::copy(o, o + aa::kObsStride, h.begin() + 1 + (size_t)aa::kObsStride * k);
        }
        aa::DevBuf<aa::MeshObsDev> dtab;
        dtab.upload(table, s);
        aa::DevBuf<double> dobs, dq, dout((size_t)3 * std::max(n, 1));
        dobs.upload(h, s);
        dq.upload(q3, (size_t)3 * n, s);
        aa::DevBuf<int> dnode;
        if (q_node) {
            dnode.upload(q_node, (size_t)n, s);
            aa::launch_test_collision_prox_exempt(dobs.p, dtab.p, dq.p, dnode.p, n, dout.p, s);
        } else {
            aa::launch_test_collision_prox(dobs.p, dtab.p, dq.p, n, dout.p, s);
        }
        AA_HIP(hipMemcpyAsync(out3, dout.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
    });
}

// aa_test_contact_friction and its carry form (carry_form: mesh_verts_prev3, mesh_carry, tri and
// bary3 are read / written and the carry kernel is launched; otherwise the plain one, as ever)
static int test_contact_friction(const char* who, bool carry_form, aa_ctx ctx, const double* obs_rows,
                                 const double* obs_rows_prev, const double* mu, int n_obs, const double* mesh_verts3,
                                 const int* mesh_vert_ptr, const int* mesh_tris3, const int* mesh_tri_ptr, int n_meshes,
                                 const double* mesh_poses, const double* mesh_poses_prev, const unsigned char* mesh_still,
                                 const int* q_node, const unsigned char* q_pinned, int n, const int* exempt_ptr,
                                 const int* exempt_nodes, const double* x_old3, const double* x_new3, const double* u3,
                                 const double* w, const double* m, double penalty, double dt, double* x_out3, int* hit,
                                 int* row, double* point3, double* normal3, double* push, double* slip3, double* scale,
                                 const double* mesh_verts_prev3, const unsigned char* mesh_carry, int* tri, double* bary3) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        NEED(!carry_form || ((n_meshes == 0 || (mesh_verts_prev3 && mesh_carry)) && tri && bary3),
             std::string(who) + "null carry arguments");
        NEED(n >= 0 && n_obs >= 0 && n_obs <= aa::kMaxObstacles && (n_obs == 0 || (obs_rows && obs_rows_prev && mu)),
             std::string(who) + "bad obstacle arguments");
        NEED(n_meshes >= 0 && n_meshes <= aa::kMaxMeshObstacles, std::string(who) + "too many mesh obstacles");
        NEED(n_meshes == 0 || (mesh_verts3 && mesh_vert_ptr && mesh_tris3 && mesh_tri_ptr && exempt_ptr), std::string(who) + "null mesh arrays");
        NEED(n == 0 || (q_node && q_pinned && x_old3 && x_new3 && u3 && w && m), std::string(who) + "null query arrays");
        NEED(x_out3 && hit && row && point3 && normal3 && push && slip3 && scale, std::string(who) + "null output");
        int n_ids = 1;
        for (int e = 0; e < n; ++e) {
            NEED(q_node[e] >= 0, std::string(who) + "negative node id");
            NEED(w[e] > 0.0 && m[e] > 0.0, std::string(who) + "weights and masses must be positive");
            n_ids = std::max(n_ids, q_node[e] + 1);
        }
        for (int k = 0; k < n_meshes; ++k) NEED(exempt_ptr[k + 1] >= exempt_ptr[k], std::string(who) + "bad exempt_ptr");
        if (n_meshes > 0) {
            NEED(exempt_ptr[n_meshes] == 0 || exempt_nodes, std::string(who) + "null exempt list");
            for (int j = 0; j < exempt_ptr[n_meshes]; ++j) {
                NEED(exempt_nodes[j] >= 0, std::string(who) + "negative node id");
                n_ids = std::max(n_ids, exempt_nodes[j] + 1);
            }
        }
        std::vector<std::unique_ptr<aa::DevBuf<unsigned char>>> ebufs;
        std::vector<std::unique_ptr<aa::MeshObsBuffers>> bufs;
        std::vector<aa::MeshObsDev> table((size_t)aa::kMaxMeshObstacles), prev((size_t)aa::kMaxMeshObstacles);
        std::vector<unsigned char> still((size_t)aa::kMaxMeshObstacles, 0);
        std::vector<aa::MeshCarryDev> ctab((size_t)aa::kMaxMeshObstacles, aa::MeshCarryDev{nullptr, nullptr});
        std::vector<std::unique_ptr<aa::DevBuf<double>>> vprev;
        std::vector<std::unique_ptr<aa::DevBuf<int>>> lvid;
        auto pose_of = [&](const double* poses, int k) -> const double* {
            const double* pose = poses ? poses + 12 * (size_t)k : nullptr;
            if (pose && std::all_of(pose, pose + 12, [](double v) { return std::isnan(v); })) pose = nullptr;
            if (pose) aa::validate_mesh_pose(pose, who);
            return pose;
        };
        for (int k = 0; k < n_meshes; ++k) {
            const aa::MeshObstacleHost M = aa::prepare_mesh_obstacle(
                mesh_verts3 + 3 * (size_t)mesh_vert_ptr[k], mesh_vert_ptr[k + 1] - mesh_vert_ptr[k],
                mesh_tris3 + 3 * (size_t)mesh_tri_ptr[k], mesh_tri_ptr[k + 1] - mesh_tri_ptr[k]);
            bufs.push_back(std::make_unique<aa::MeshObsBuffers>());
            table[k] = bufs.back()->upload(M, s);
            prev[k] = table[k];
            aa::apply_mesh_pose(table[k], pose_of(mesh_poses, k));
            aa::apply_mesh_pose(prev[k], pose_of(mesh_poses_prev, k));
            still[k] = mesh_still ? mesh_still[k] : 0;
            if (exempt_ptr[k + 1] > exempt_ptr[k]) {
                std::vector<unsigned char> bytes((size_t)n_ids, 0);
                for (int j = exempt_ptr[k]; j < exempt_ptr[k + 1]; ++j) bytes[exempt_nodes[j]] = 1;
                ebufs.push_back(std::make_unique<aa::DevBuf<unsigned char>>());
                ebufs.back()->upload(bytes, s);
                AA_HIP(hipStreamSynchronize(s));
                table[k].exempt = ebufs.back()->p;
            }
            if (carry_form && mesh_carry[k]) {   // the previous vertices and the leaf triangles' vertex ids
                const int nv = mesh_vert_ptr[k + 1] - mesh_vert_ptr[k], nf = mesh_tri_ptr[k + 1] - mesh_tri_ptr[k];
                const aa::MeshRefitTables RT = aa::make_refit_tables(M, nv, mesh_tris3 + 3 * (size_t)mesh_tri_ptr[k], nf);
                vprev.push_back(std::make_unique<aa::DevBuf<double>>());
                lvid.push_back(std::make_unique<aa::DevBuf<int>>());
                vprev.back()->upload(mesh_verts_prev3 + 3 * (size_t)mesh_vert_ptr[k], 3 * (size_t)nv, s);
                lvid.back()->upload(RT.leaf_vid, s);
                AA_HIP(hipStreamSynchronize(s));   // RT is a temporary
                ctab[k] = aa::MeshCarryDev{vprev.back()->p, lvid.back()->p};
            }
        }
        std::vector<double> h(1 + (size_t)aa::kObsStride * aa::kMaxObstacles, 0.0), hp(h.size(), 0.0), hmu((size_t)aa::kMaxObstacles, 0.0);
        h[0] = hp[0] = n_obs;
        for (int k = 0; k < n_obs; ++k) {
            const double* o = obs_rows + (size_t)aa::kObsStride * k;
            const double* op = obs_rows_prev + (size_t)aa::kObsStride * k;
            const int type = (int)o[0];
            NEED(type >= aa::OBS_FLOOR && type <= aa::OBS_MESH && (int)op[0] == type, std::string(who) + "unknown obstacle type, or one that differs from the previous row's");
            NEED(type != aa::OBS_MESH || (o[1] >= 0 && o[1] < n_meshes && o[1] == (int)o[1]), std::string(who) + "mesh id out of range");
            NEED(std::isfinite(mu[k]) && mu[k] >= 0.0, std::string(who) + "the coefficient must be finite and >= 0");
            std::copy(o, o + aa::kObsStride, h.begin() + 1 + (size_t)aa::kObsStride * k);
            std::copy(op, op + aa::kObsStride, hp.begin() + 1 + (size_t)aa::kObsStride * k);
            hmu[k] = mu[k];
        }
        const size_t nn = (size_t)std::max(n, 1);
        aa::DevBuf<aa::MeshObsDev> dtab, dprev;
        dtab.upload(table, s);
        dprev.upload(prev, s);
        aa::DevBuf<unsigned char> dstill, dpin;
        dstill.upload(still, s);
        aa::DevBuf<double> dobs, dobsp, dmu, dxo, dxn, du, dw, dm;
        dobs.upload(h, s); dobsp.upload(hp, s); dmu.upload(hmu, s);
        aa::DevBuf<int> dnode, dhit(nn), drow(nn);
        aa::DevBuf<double> dc(3 * nn), dn(3 * nn), dj(nn), drt(3 * nn), ds(nn);
        if (n > 0) {
            dpin.upload(q_pinned, (size_t)n, s);
            dnode.upload(q_node, (size_t)n, s);
            dxo.upload(x_old3, 3 * (size_t)n, s); dxn.upload(x_new3, 3 * (size_t)n, s); du.upload(u3, 3 * (size_t)n, s);
            dw.upload(w, (size_t)n, s); dm.upload(m, (size_t)n, s);
            const aa::FrictionTables T{dobsp.p, dprev.p, dmu.p, dstill.p};
            const aa::ContactRecDev rec{dhit.p, drow.p, dc.p, dn.p, dj.p, drt.p, ds.p};
            aa::DevBuf<aa::MeshCarryDev> dcarry;
            aa::DevBuf<int> dtri;
            aa::DevBuf<double> db;
            if (carry_form) {
                dcarry.upload(ctab, s);
                dtri.alloc(nn); db.alloc(3 * nn);
                aa::launch_test_contact_friction_carry(dobs.p, n_meshes > 0 ? dtab.p : nullptr, T, dnode.p, dpin.p, dxo.p, dxn.p,
                                                       du.p, dw.p, dm.p, penalty, dt, n, rec, dcarry.p,
                                                       aa::ContactFeatDev{dtri.p, db.p}, s);
                AA_HIP(hipMemcpyAsync(tri, dtri.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
                AA_HIP(hipMemcpyAsync(bary3, db.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
            } else {
                aa::launch_test_contact_friction(dobs.p, n_meshes > 0 ? dtab.p : nullptr, T, dnode.p, dpin.p, dxo.p, dxn.p, du.p,
                                                 dw.p, dm.p, penalty, dt, n, rec, s);
            }
            AA_HIP(hipMemcpyAsync(x_out3, dxn.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(hit, dhit.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(row, drow.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(point3, dc.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(normal3, dn.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(push, dj.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(slip3, drt.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipMemcpyAsync(scale, ds.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
            AA_HIP(hipStreamSynchronize(s));   // the carry form's buffers live in this block
        }
        AA_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int aa_test_contact_friction(aa_ctx ctx, const double* obs_rows, const double* obs_rows_prev, const double* mu,
                                       int n_obs, const double* mesh_verts3, const int* mesh_vert_ptr, const int* mesh_tris3,
                                       const int* mesh_tri_ptr, int n_meshes, const double* mesh_poses,
                                       const double* mesh_poses_prev, const unsigned char* mesh_still, const int* q_node,
                                       const unsigned char* q_pinned, int n, const int* exempt_ptr, const int* exempt_nodes,
                                       const double* x_old3, const double* x_new3, const double* u3, const double* w,
                                       const double* m, double penalty, double dt, double* x_out3, int* hit, int* row,
                                       double* point3, double* normal3, double* push, double* slip3, double* scale) {
    return test_contact_friction("aa_test_contact_friction: ", false, ctx, obs_rows, obs_rows_prev, mu, n_obs, mesh_verts3,
                                 mesh_vert_ptr, mesh_tris3, mesh_tri_ptr, n_meshes, mesh_poses, mesh_poses_prev, mesh_still, q_node,
                                 q_pinned, n, exempt_ptr, exempt_nodes, x_old3, x_new3, u3, w, m, penalty, dt, x_out3, hit, row,
                                 point3, normal3, push, slip3, scale, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int aa_test_contact_friction_carry(aa_ctx ctx, const double* obs_rows, const double* obs_rows_prev, const double* mu,
                                             int n_obs, const double* mesh_verts3, const int* mesh_vert_ptr,
                                             const int* mesh_tris3, const int* mesh_tri_ptr, int n_meshes,
                                             const double* mesh_poses, const double* mesh_poses_prev,
                                             const unsigned char* mesh_still, const int* q_node, const unsigned char* q_pinned,
                                             int n, const int* exempt_ptr, const int* exempt_nodes, const double* x_old3,
                                             const double* x_new3, const double* u3, const double* w, const double* m,
                                             double penalty, double dt, const double* mesh_verts_prev3,
                                             const unsigned char* mesh_carry, double* x_out3, int* hit, int* row, double* point3,
                                             double* normal3, double* push, double* slip3, double* scale, int* tri,
                                             double* bary3) {
    return test_contact_friction("aa_test_contact_friction_carry: ", true, ctx, obs_rows, obs_rows_prev, mu, n_obs, mesh_verts3,
                                 mesh_vert_ptr, mesh_tris3, mesh_tri_ptr, n_meshes, mesh_poses, mesh_poses_prev, mesh_still, q_node,
                                 q_pinned, n, exempt_ptr, exempt_nodes, x_old3, x_new3, u3, w, m, penalty, dt, x_out3, hit, row,
                                 point3, normal3, push, slip3, scale, mesh_verts_prev3, mesh_carry, tri, bary3);
}

extern "C" int aa_test_direct_solve(aa_ctx ctx, int n, const double* xyz3, const int* ptr, const int* col,
                                    const double* val, int n_tree, const int* tree_beg, const int* tree_end,
                                    const int* tree_parent, int leaf_size, int top_rows, int wave_p, int wave_r,
                                    int max_sets, int wide, int default_branches, int device_factor, const double* b0,
                                    const double* b1, int n_script, const int* script, double sentinel, double* x_out,
                                    double* x_host, int* row_info, int* plan, int plan_cap, int* plan_count) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        NEED(n >= 1 && xyz3 && ptr && col && val && b0 && x_out && x_host, "aa_test_direct_solve: null argument");
        NEED(n_tree >= 0 && (n_tree == 0 || (tree_beg && tree_end && tree_parent)), "aa_test_direct_solve: bad tree");
        NEED(n_tree > 0 || leaf_size >= 1, "aa_test_direct_solve: leaf_size must be positive");
        NEED((max_sets == 1 || max_sets == 2) && wave_p >= 0 && wave_r >= 0 && n_script >= 0 && (n_script == 0 || script),
             "aa_test_direct_solve: bad argument");
        NEED(ptr[0] == 0, "aa_test_direct_solve: bad CSR");
        for (int i = 0; i < n; ++i) {
            NEED(ptr[i + 1] >= ptr[i], "aa_test_direct_solve: bad CSR");
            bool diag = false;
            for (int k = ptr[i]; k < ptr[i + 1]; ++k) {
                NEED(col[k] >= 0 && col[k] < n && (k == ptr[i] || col[k] > col[k - 1]), "aa_test_direct_solve: CSR columns must be sorted and in range");
                diag = diag || col[k] == i;
            }
            NEED(diag, "aa_test_direct_solve: every diagonal entry must be stored");
        }
        for (int k = 0; k < n_script; ++k) {
            const int op = script[k];
            NEED(op >= AA_SOLVE_B0 && op <= AA_SOLVE_DONE_B1, "aa_test_direct_solve: unknown script entry");
            const bool uses_b1 = op == AA_SOLVE_B1 || op == AA_SOLVE_BOTH || op == AA_SOLVE_GATED_SKIP_B1 ||
                                 op == AA_SOLVE_GATED_TAKE_B1 || op == AA_SOLVE_DONE_B1;
            NEED(!uses_b1 || b1, "aa_test_direct_solve: a script entry names b1, which was not given");
            NEED(op != AA_SOLVE_BOTH || max_sets == 2, "aa_test_direct_solve: solve2 needs max_sets = 2");
        }
        // the tree and the matrix in its ordering
        aa::NdTree tree;
        if (n_tree > 0) {
            tree = aa::explicit_tree(n, std::vector<int>(tree_beg, tree_beg + n_tree), std::vector<int>(tree_end, tree_end + n_tree),
                                     std::vector<int>(tree_parent, tree_parent + n_tree));
        } else {
            std::vector<int> aptr(n + 1, 0), aj;
            for (int i = 0; i < n; ++i) {
                for (int k = ptr[i]; k < ptr[i + 1]; ++k) if (col[k] != i) aj.push_back(col[k]);
                aptr[i + 1] = (int)aj.size();
            }
            tree = aa::nested_dissection(n, xyz3, aptr, aj, leaf_size, top_rows);
        }
        NEED((int)tree.perm.size() == n, "aa_test_direct_solve: the ordering lost nodes");
        std::vector<int> inv(n);
        for (int q = 0; q < n; ++q) inv[tree.perm[q]] = q;
        aa::CsrMatrix A;
        A.n = n;
        A.ptr.assign(n + 1, 0);
        A.col.reserve(ptr[n]);
        A.val.reserve(ptr[n]);
        std::vector<std::pair<int, double>> r;
        for (int q = 0; q < n; ++q) {
            const int i = tree.perm[q];
            r.clear();
            for (int k = ptr[i]; k < ptr[i + 1]; ++k) r.push_back({inv[col[k]], val[k]});
            std::sort(r.begin(), r.end());
            for (const auto& e : r) { A.col.push_back(e.first); A.val.push_back(e.second); }
            A.ptr[q + 1] = (int)A.col.size();
        }
        aa::check_tree_covers(A, tree);
        aa::SupernodalFactor F = device_factor ? aa::factor_on_device(A, tree, s) : aa::multifrontal_cholesky(A, tree);
        // host yardstick with the same factor
        const int nrhs = b1 ? 2 : 1;
        std::vector<double> hb(3 * (size_t)n), bperm[2];
        for (int k = 0; k < nrhs; ++k) {
            const double* b = k ? b1 : b0;
            bperm[k].resize(3 * (size_t)n);
            for (int q = 0; q < n; ++q) for (int c = 0; c < 3; ++c) bperm[k][3 * (size_t)q + c] = b[3 * (size_t)tree.perm[q] + c];
            hb = bperm[k];
            aa::factor_solve_host(F, hb);
            for (int q = 0; q < n; ++q)
                for (int c = 0; c < 3; ++c) x_host[3 * ((size_t)k * n + tree.perm[q]) + c] = hb[3 * (size_t)q + c];
        }
        if (!b1) std::fill(x_host + 3 * (size_t)n, x_host + 6 * (size_t)n, sentinel);
        if (row_info) {
            std::vector<int> depth(F.n_nodes, 0);
            for (int sn = F.n_nodes - 1; sn >= 0; --sn) depth[sn] = F.parent[sn] >= 0 ? depth[F.parent[sn]] + 1 : 0;
            for (int sn = 0; sn < F.n_nodes; ++sn)
                for (int q = F.beg[sn]; q < F.end[sn]; ++q) { row_info[2 * tree.perm[q]] = F.height[sn]; row_info[2 * tree.perm[q] + 1] = depth[sn]; }
        }
        // the device solver, built once, then the script
        aa::DirectSolver solver;
        solver.default_branches = default_branches;
        solver.build(F, s, nullptr, -1, -1, nullptr, max_sets, wide != 0, wave_p, wave_r);
        const aa::DirectSolver::PlanSummary P = solver.plan_summary();
        static_assert(sizeof(P) % sizeof(int) == 0, "PlanSummary is ints only");
        const int np = (int)(sizeof(P) / sizeof(int));
        if (plan_count) *plan_count = np;
        if (plan) std::memcpy(plan, &P, sizeof(int) * std::min(np, std::max(plan_cap, 0)));
        aa::DevBuf<double> db[2], dx[2];
        for (int k = 0; k < 2; ++k) {
            dx[k].alloc(3 * (size_t)n);
            if (k < nrhs) db[k].upload(bperm[k], s);
        }
        aa::DevBuf<aa::Ctrl> dctrl(1);
        const std::vector<double> fill(3 * (size_t)n, sentinel);
        std::vector<double> hx(3 * (size_t)n);
        for (int k = 0; k < n_script; ++k) {
            const int op = script[k];
            for (int o = 0; o < 2; ++o) AA_HIP(hipMemcpyAsync(dx[o].p, fill.data(), sizeof(double) * fill.size(), hipMemcpyHostToDevice, s));
            aa::Ctrl hc;
            std::memset(&hc, 0, sizeof(hc));
            int gate = 0, rhs = 0;
            switch (op) {
                case AA_SOLVE_B0: break;
                case AA_SOLVE_B1: rhs = 1; break;
                case AA_SOLVE_BOTH: break;
                case AA_SOLVE_GATED_SKIP_B0: gate = 1; break;
                case AA_SOLVE_GATED_SKIP_B1: gate = 1; rhs = 1; break;
                case AA_SOLVE_GATED_TAKE_B0: gate = 1; hc.reject = 1; break;
                case AA_SOLVE_GATED_TAKE_B1: gate = 1; hc.reject = 1; rhs = 1; break;
                case AA_SOLVE_DONE_B0: hc.done = 1; break;
                default: hc.done = 1; rhs = 1; break;
            }
            AA_HIP(hipMemcpyAsync(dctrl.p, &hc, sizeof(hc), hipMemcpyHostToDevice, s));
            AA_HIP(hipStreamSynchronize(s));   // (hc and fill are pageable host memory)
            if (op == AA_SOLVE_BOTH) solver.solve2(db[0].p, dx[0].p, db[1].p, dx[1].p, dctrl.p, 0, s);
            else solver.solve(db[rhs].p, dx[0].p, dctrl.p, gate, s);
            AA_HIP(hipStreamSynchronize(s));
            for (int o = 0; o < 2; ++o) {
                AA_HIP(hipMemcpy(hx.data(), dx[o].p, sizeof(double) * hx.size(), hipMemcpyDeviceToHost));
                double* out = x_out + 3 * (size_t)n * (2 * (size_t)k + o);
                for (int q = 0; q < n; ++q) for (int c = 0; c < 3; ++c) out[3 * (size_t)tree.perm[q] + c] = hx[3 * (size_t)q + c];
            }
        }
    });
}

extern "C" int aa_test_cod_solve(aa_ctx ctx, int k, const double* M, const double* b, double* theta) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        NEED(M && b && theta && k >= 1 && k <= aa::kMaxM, "aa_test_cod_solve: bad argument");
        aa::DevBuf<double> dM, db, dx(k);
        dM.upload(M, (size_t)k * k, s);
        db.upload(b, k, s);
        aa::launch_test_cod(k, dM.p, db.p, dx.p, s);
        AA_HIP(hipMemcpyAsync(theta, dx.p, sizeof(double) * k, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int aa_test_geom_project(aa_ctx ctx, int type, int k, const double* prm2, const double* in, int n,
                                    double* out) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        NEED(prm2 && in && out && n >= 0 && k >= 2, "aa_test_geom_project: bad argument");
        const int C = (type == aa::GEO_ANGLE || type == aa::GEO_EDGE) ? k - 1 : k;
        aa::DevBuf<double> di, dout((size_t)3 * C * std::max(n, 1));
        di.upload(in, (size_t)3 * C * n, s);
        aa::launch_test_geo_project(type, k, prm2, di.p, n, dout.p, s);
        AA_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * 3 * C * n, hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
    });
}


extern "C" int aa_test_anderson_step(aa_ctx ctx, int m, long long na, long long nb, long long eff, const double* G,
                                     double* cur, double* dF, double* dG, int* ctl9, double* scale, double* M,
                                     double* coef, double* aa_s, const long long* mask4, int nblocks, int flags,
                                     double* red, long long red_cap, double* out, double* copy_to, int* info3) {
    return with_device_arrays(ctx, [&](hipStream_t s) {
        const long long dim = na + nb;
        NEED(G && cur && dF && dG && ctl9 && scale && M && coef && aa_s && mask4 && red && info3,
             "aa_test_anderson_step: null argument");
        NEED(m >= 1 && m <= aa::kMaxM, "aa_test_anderson_step: m must lie in 1..32");
        NEED(na >= 0 && nb >= 0 && dim >= 1 && dim < (1LL << 31), "aa_test_anderson_step: bad segment lengths");
        NEED(eff > 0 && eff <= dim, "aa_test_anderson_step: eff must lie in 1..dim");
        NEED(ctl9[0] >= 0, "aa_test_anderson_step: aa_iter must not be negative");
        NEED(ctl9[1] >= 0 && ctl9[1] < m, "aa_test_anderson_step: aa_col must lie in 0..m-1");
        NEED(nblocks >= 0 && nblocks <= 2048, "aa_test_anderson_step: nblocks must lie in 0..2048");
        const bool want_copy = flags & AA_STEP_COPY_TO, inplace = flags & AA_STEP_INPLACE;
        NEED(!(flags & ~(AA_STEP_COPY_TO | AA_STEP_INPLACE | AA_STEP_NARROW | AA_STEP_ROWS)), "aa_test_anderson_step: unknown flag");
        NEED(!inplace || nb == 0, "aa_test_anderson_step: the in-place form has one segment");
        NEED(inplace || out, "aa_test_anderson_step: out is null");
        NEED(!want_copy || copy_to, "aa_test_anderson_step: copy_to is null");
        const int nbl = nblocks > 0 ? nblocks : aa::aa_reduce_blocks(dim);
        const int bucket = aa::aa_window_bucket(m);
        const size_t nred = (size_t)nbl * (2 + 2 * bucket);
        NEED(red_cap >= (long long)nred, "aa_test_anderson_step: red is too short");

        aa::Ctrl hc{};
        hc.aa_m = m;
        hc.aa_iter = ctl9[0]; hc.aa_col = ctl9[1]; hc.aa_skip = ctl9[2]; hc.aa_active = ctl9[3]; hc.done = ctl9[4];
        hc.aa_mk = ctl9[5]; hc.aa_j = ctl9[6]; hc.aa_jn = ctl9[7]; hc.aa_first = ctl9[8];
        hc.aa_s = *aa_s;
        std::copy(scale, scale + m, hc.scale);
        std::copy(coef, coef + m, hc.coef);
        std::copy(M, M + (size_t)m * m, hc.M);
        aa::DevBuf<aa::Ctrl> dctrl(1);
        // the two segments live apart, as the solvers' do
        aa::DevBuf<double> dGa, dGb, dcur, ddF, ddG, dred(nred), douta, doutb, dcpa, dcpb;
        dGa.upload(G, (size_t)na, s);
        dGb.upload(G + na, (size_t)nb, s);
        dcur.upload(cur, (size_t)dim, s);
        ddF.upload(dF, (size_t)m * eff, s);
        ddG.upload(dG, (size_t)m * dim, s);
        dred.zero(s);
        if (!inplace) { douta.upload(out, (size_t)na, s); doutb.upload(out + na, (size_t)nb, s); }
        if (want_copy) { dcpa.upload(copy_to, (size_t)na, s); dcpb.upload(copy_to + na, (size_t)nb, s); }
        AA_HIP(hipMemcpyAsync(dctrl.p, &hc, sizeof(hc), hipMemcpyHostToDevice, s));
        AA_HIP(hipStreamSynchronize(s));   // (hc is pageable host memory)

        // a segment of no entries is still a pointer the kernels may form addresses from
        const aa::Seg2 g{na ? dGa.p : dGb.p, na, dGb.p, nb};
        const aa::Seg2 o = inplace ? aa::Seg2{dcur.p, dim, nullptr, 0} : aa::Seg2{na ? douta.p : doutb.p, na, doutb.p, nb};
        const aa::Seg2 cp = want_copy ? aa::Seg2{na ? dcpa.p : dcpb.p, na, dcpb.p, nb} : aa::Seg2{nullptr, 0, nullptr, 0};
        aa::AAMask mask;
        mask.lo1 = mask4[0]; mask.hi1 = mask4[1]; mask.lo2 = mask4[2]; mask.hi2 = mask4[3];
        const int cols = (flags & AA_STEP_ROWS) ? 0 : 1;
        aa::launch_aa_reduce(g, dcur.p, eff, ddF.p, ddG.p, dctrl.p, dred.p, nbl, cp, m, s, nullptr, nullptr, 0, nullptr,
                             nullptr, nullptr, mask, cols);
        aa::launch_aa_solve(dctrl.p, dred.p, nbl, m, s);
        aa::launch_aa_mix(g, dcur.p, eff, ddF.p, ddG.p, dctrl.p, o, m, s, (flags & AA_STEP_NARROW) != 0);

        auto down = [&](double* h, const aa::DevBuf<double>& d) {
            if (d.n) AA_HIP(hipMemcpyAsync(h, d.p, d.bytes(), hipMemcpyDeviceToHost, s));
        };
        down(red, dred); down(cur, dcur); down(dF, ddF); down(dG, ddG);
        if (!inplace) { down(out, douta); down(out + na, doutb); }
        if (want_copy) { down(copy_to, dcpa); down(copy_to + na, dcpb); }
        AA_HIP(hipMemcpyAsync(&hc, dctrl.p, sizeof(hc), hipMemcpyDeviceToHost, s));
        AA_HIP(hipStreamSynchronize(s));
        ctl9[0] = hc.aa_iter; ctl9[1] = hc.aa_col; ctl9[2] = hc.aa_skip; ctl9[3] = hc.aa_active; ctl9[4] = hc.done;
        ctl9[5] = hc.aa_mk; ctl9[6] = hc.aa_j; ctl9[7] = hc.aa_jn; ctl9[8] = hc.aa_first;
        *aa_s = hc.aa_s;
        std::copy(hc.scale, hc.scale + m, scale);
        std::copy(hc.coef, hc.coef + m, coef);
        std::copy(hc.M, hc.M + (size_t)m * m, M);
        info3[0] = bucket; info3[1] = nbl; info3[2] = bucket == 32 ? cols : -1;
    });
}
