// aa_admm.hpp -- header-only C++ facade over the C ABI (aa_admm.h) that keeps the reference's
// admm-elastic plugin API shape (admm_anderson_hard_zxu/src/Solver.hpp:39-262,
// EnergyTerm.hpp:35-129, TetEnergyTerm.hpp:36-51, TriEnergyTerm.hpp:33-47) so existing scene
// code ports by changing includes:
//
//   admm::Solver solver;                               // one MI355X (device 0) by default
//   solver.add_nodes(x, m, n);                         // Solver::add_nodes
//   admm::create_tets_from_mesh<float, admm::NeoHookeanTet>(solver.energyterms, verts, inds, n, lame, off);
//   admm::create_tris_from_mesh<float, admm::TriEnergyTerm>(solver.energyterms, verts, inds, n, lame, off);
//   solver.set_pins(pins, points);                     // Solver::set_pins
//   solver.add_obstacle(std::make_shared<admm::Floor>(-1.0)); solver.set_collisions(inds);  // (u,x) variant
//   solver.add_obstacle(std::make_shared<admm::PassiveMesh>(admm::PassiveMesh::from_tets(v, nv, tets, nt)));
//   solver.ext_forces.push_back(std::make_shared<admm::WindForce>(faces));                    // wind
//   solver.initialize(settings);                       // Solver::initialize (returns bool)
//   solver.step();                                     // Solver::step; solver.m_x / m_v updated
//   solver.set_obstacle_pose(mesh, R, t); solver.update_obstacle(floor);   // kinematic obstacles, between steps
//   solver.set_obstacle_vertices(mesh, new_verts);                         // a mesh that changes shape
//   solver.bind_obstacle(mesh, surface_nodes); solver.exempt_from_obstacle(mesh, body_nodes);   // body-to-body contact
//   solver.set_obstacle_friction(floor, 0.4); solver.record_contacts(); solver.contacts();      // Coulomb friction
//
// Energy terms are descriptors of the built-in element kinds (batched SoA on the device);
// user-defined EnergyTerm subclasses with arbitrary prox() are not supported (no host
// callbacks on the GPU path). Errors are re-raised as std::runtime_error like the reference.
#ifndef AA_ADMM_HPP
#define AA_ADMM_HPP

#include <algorithm>
#include <array>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "aa_admm.h"

namespace admm {

inline void check(int rc) {
    if (rc != AA_OK) throw std::runtime_error(aa_last_error());
}

// EnergyTerm.hpp:35-61
class Lame {
public:
    static Lame rubber() { return Lame(10000000, 0.499); }
    static Lame soft_rubber() { return Lame(10000000, 0.399); }
    static Lame very_soft_rubber() { return Lame(1000000, 0.299); }
    double mu = 0, lambda = 0;
    double limit_min = -100.0, limit_max = 100.0;
    double bulk_modulus() const { return lambda + (2.0 / 3.0) * mu; }
    Lame(double k, double v) : mu(k / (2.0 * (1.0 + v))), lambda(k * v / ((1.0 + v) * (1.0 - 2.0 * v))) {}
    Lame() {}
    aa_lame c() const { return aa_lame{mu, lambda, limit_min, limit_max}; }
};

// Descriptors of the built-in energy terms (one per create_*_from_mesh call).
class EnergyTerm {
public:
    virtual ~EnergyTerm() {}
    int kind = 0, material = AA_LINEAR;   // kind 0 tet, 1 tri, 3 bending hinges (BendingEnergyTerm), 4 springs (SpringEnergyTerm), 5 ties (TieEnergyTerm)
    Lame lame;
    std::vector<Lame> lames;     // per-element materials ([count]); empty: `lame` for every element
    std::vector<double> verts;   // rest shape (as given to create_*_from_mesh)
    std::vector<int> inds;
    int count = 0, vertex_offset = 0;
};
struct TetEnergyTerm { static constexpr int material = AA_LINEAR; };
struct NeoHookeanTet { static constexpr int material = AA_NEOHOOKEAN; };
struct StVKTet { static constexpr int material = AA_STVK; };
struct TriEnergyTerm { static constexpr int material = AA_LINEAR; };

// TetEnergyTerm.hpp:36-51 (one descriptor holds the whole mesh instead of n objects)
template <typename IN_SCALAR, typename TYPE>
inline void create_tets_from_mesh(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts,
                                  const int* inds, int n_tets, const Lame& lame, const int vertex_offset) {
    auto e = std::make_shared<EnergyTerm>();
    e->kind = 0;
    e->material = TYPE::material;
    e->lame = lame;
    int nv = 0;
    for (int i = 0; i < 4 * n_tets; ++i) nv = std::max(nv, inds[i] + 1);
    e->verts.assign(verts, verts + 3 * (size_t)nv);
    e->inds.assign(inds, inds + 4 * (size_t)n_tets);
    e->count = n_tets;
    e->vertex_offset = vertex_offset;
    energyterms.push_back(e);
}

// TriEnergyTerm.hpp:33-47
template <typename IN_SCALAR, typename TYPE>
inline void create_tris_from_mesh(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts,
                                  const int* inds, int n_tris, const Lame& lame, const int vertex_offset) {
    auto e = std::make_shared<EnergyTerm>();
    e->kind = 1;
    e->material = AA_LINEAR;
    e->lame = lame;
    int nv = 0;
    for (int i = 0; i < 3 * n_tris; ++i) nv = std::max(nv, inds[i] + 1);
    e->verts.assign(verts, verts + 3 * (size_t)nv);
    e->inds.assign(inds, inds + 3 * (size_t)n_tris);
    e->count = n_tris;
    e->vertex_offset = vertex_offset;
    energyterms.push_back(e);
}

// Per-element materials: lames[e] is element e's Lame -- the reference caller's loop of one-element
// create_*_from_mesh calls (each EnergyTerm owns its Lame, TetEnergyTerm.hpp:36-51 /
// TriEnergyTerm.hpp:33-47) as one descriptor and one device group.
template <typename IN_SCALAR, typename TYPE>
inline void create_tets_from_mesh(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts,
                                  const int* inds, int n_tets, const std::vector<Lame>& lames, const int vertex_offset) {
    if ((int)lames.size() != n_tets) throw std::runtime_error("create_tets_from_mesh: one Lame per tet expected");
    create_tets_from_mesh<IN_SCALAR, TYPE>(energyterms, verts, inds, n_tets, Lame(), vertex_offset);
    energyterms.back()->lames = lames;
}
template <typename IN_SCALAR, typename TYPE>
inline void create_tris_from_mesh(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts,
                                  const int* inds, int n_tris, const std::vector<Lame>& lames, const int vertex_offset) {
    if ((int)lames.size() != n_tris) throw std::runtime_error("create_tris_from_mesh: one Lame per triangle expected");
    create_tris_from_mesh<IN_SCALAR, TYPE>(energyterms, verts, inds, n_tris, Lame(), vertex_offset);
    energyterms.back()->lames = lames;
}

// Bending (aa_elastic_add_bending; the reference has no such term): hinges on the interior edges of
// a triangle list, stiffness k_bend; flat_rest false keeps the rest shape's curvature as the equilibrium.
class BendingEnergyTerm : public EnergyTerm {
public:
    double k_bend = 0;
    bool flat_rest = true;
};
template <typename IN_SCALAR>
inline void create_bending_from_mesh(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts,
                                     const int* inds, int n_tris, double k_bend, bool flat_rest, const int vertex_offset) {
    auto e = std::make_shared<BendingEnergyTerm>();
    e->kind = 3;
    e->k_bend = k_bend;
    e->flat_rest = flat_rest;
    int nv = 0;
    for (int i = 0; i < 3 * n_tris; ++i) nv = std::max(nv, inds[i] + 1);
    e->verts.assign(verts, verts + 3 * (size_t)nv);
    e->inds.assign(inds, inds + 3 * (size_t)n_tris);
    e->count = n_tris;
    e->vertex_offset = vertex_offset;
    energyterms.push_back(e);
}

// Springs, tethers and struts (aa_elastic_add_springs; the reference's SpringPin is a hard spring on
// one node): n two-node springs pairs[2e], pairs[2e + 1] with stiffness k[e] and rest length rest[e];
// rest null takes the distance of the pair in verts (verts may be null when rest is given). mode:
// AA_SPRING / AA_SPRING_TETHER / AA_SPRING_STRUT, | AA_SPRING_HARD.
class SpringEnergyTerm : public EnergyTerm {
public:
    std::vector<double> k, rest;   // rest empty: lengths from verts
    int mode = AA_SPRING;
    bool has_verts = false;
};
template <typename IN_SCALAR>
inline void create_springs(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts, const int* pairs,
                           int n, const double* k, const double* rest, int mode, const int vertex_offset) {
    auto e = std::make_shared<SpringEnergyTerm>();
    e->kind = 4;
    e->mode = mode;
    e->k.assign(k, k + n);
    if (rest) e->rest.assign(rest, rest + n);
    if (verts) {
        int nv = 0;
        for (int i = 0; i < 2 * n; ++i) nv = std::max(nv, pairs[i] + 1);
        e->verts.assign(verts, verts + 3 * (size_t)nv);
        e->has_verts = true;
    }
    e->inds.assign(pairs, pairs + 2 * (size_t)n);
    e->count = n;
    e->vertex_offset = vertex_offset;
    energyterms.push_back(e);
}

// Ties (aa_elastic_add_ties): n springs between barycentric anchors, anchor A of tie e the nodes
// nodes_a[na e ..] with the weights w_a[na e ..], anchor B alike over nb nodes; stiffness k[e] and rest
// length rest[e]; rest null takes the anchors' distance in verts (verts may be null when rest is
// given). mode as for create_springs.
class TieEnergyTerm : public EnergyTerm {
public:
    int na = 0, nb = 0;
    std::vector<int> nodes_a, nodes_b;
    std::vector<double> w_a, w_b, k, rest;   // rest empty: lengths from verts
    int mode = AA_SPRING;
    bool has_verts = false;
};
template <typename IN_SCALAR>
inline void create_ties(std::vector<std::shared_ptr<EnergyTerm>>& energyterms, const IN_SCALAR* verts, int na, const int* nodes_a,
                        const double* w_a, int nb, const int* nodes_b, const double* w_b, int n, const double* k,
                        const double* rest, int mode, const int vertex_offset) {
    auto e = std::make_shared<TieEnergyTerm>();
    e->kind = 5;
    e->mode = mode;
    e->na = na; e->nb = nb;
    e->nodes_a.assign(nodes_a, nodes_a + (size_t)na * n);
    e->nodes_b.assign(nodes_b, nodes_b + (size_t)nb * n);
    e->w_a.assign(w_a, w_a + (size_t)na * n);
    e->w_b.assign(w_b, w_b + (size_t)nb * n);
    e->k.assign(k, k + n);
    if (rest) e->rest.assign(rest, rest + n);
    if (verts) {
        int nv = 0;
        for (int i : e->nodes_a) nv = std::max(nv, i + 1);
        for (int i : e->nodes_b) nv = std::max(nv, i + 1);
        e->verts.assign(verts, verts + 3 * (size_t)nv);
        e->has_verts = true;
    }
    e->count = n;
    e->vertex_offset = vertex_offset;
    energyterms.push_back(e);
}

typedef std::array<double, 3> Vec3d;

// Passive obstacles (admm_anderson_hard_zxu/src/PassiveObject.hpp:32-136, Collider.hpp:63-82):
// shape descriptors, tested on the device by the collision terms
class PassiveCollision {
public:
    virtual ~PassiveCollision() {}
    int type = AA_OBS_FLOOR;
    double params[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
class Floor : public PassiveCollision {
public:
    explicit Floor(double y) { type = AA_OBS_FLOOR; params[0] = y; }
};
class SlideFloor : public PassiveCollision {
public:
    SlideFloor(const Vec3d& c, const Vec3d& n) {
        type = AA_OBS_SLIDE_FLOOR;
        for (int i = 0; i < 3; ++i) { params[i] = c[i]; params[3 + i] = n[i]; }
    }
};
class Sphere : public PassiveCollision {
public:
    Sphere(const Vec3d& c, double r) { type = AA_OBS_SPHERE; for (int i = 0; i < 3; ++i) params[i] = c[i]; params[3] = r; }
};
class PlaneAndHalfSphere : public PassiveCollision {
public:
    PlaneAndHalfSphere(const Vec3d& c, double r) {
        type = AA_OBS_PLANE_HALF_SPHERE;
        for (int i = 0; i < 3; ++i) params[i] = c[i];
        params[3] = r;
    }
};
class Cylinder : public PassiveCollision {
public:
    Cylinder(const Vec3d& c, double r) { type = AA_OBS_CYLINDER; for (int i = 0; i < 3; ++i) params[i] = c[i]; params[3] = r; }
};

// PassiveMesh (PassiveObject.hpp:138-178): a collision node inside the mesh moves to the nearest
// surface point. Here the obstacle is a closed, outward-oriented triangle surface (aa_admm.h,
// aa_elastic_add_mesh_obstacle): built from one directly, or from a tet mesh as the reference's is
// -- then the boundary faces are taken, the faces used by exactly one tet, oriented outward.
class PassiveMesh : public PassiveCollision {
public:
    std::vector<double> verts;   // 3 per vertex
    std::vector<int> tris;       // 3 per triangle
    int mesh_id = -1;            // its number in the solver it was added to (Solver::set_obstacle_pose)
    static PassiveMesh from_surface(const double* verts3, int n_verts, const int* tris3, int n_tris) {
        PassiveMesh m;
        m.verts.assign(verts3, verts3 + 3 * (size_t)n_verts);
        m.tris.assign(tris3, tris3 + 3 * (size_t)n_tris);
        return m;
    }
    static PassiveMesh from_tets(const double* verts3, int n_verts, const int* tets4, int n_tets) {
        PassiveMesh m;
        m.verts.assign(verts3, verts3 + 3 * (size_t)n_verts);
        // face k of a tet lies opposite its vertex k; keyed by its sorted vertex ids
        static const int loc[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
        struct Face { std::array<int, 3> key, f; int opp; };
        std::vector<Face> faces;
        faces.reserve(4 * (size_t)n_tets);
        for (int t = 0; t < n_tets; ++t)
            for (int k = 0; k < 4; ++k) {
                Face fc;
                for (int a = 0; a < 3; ++a) fc.f[a] = tets4[4 * (size_t)t + loc[k][a]];
                fc.key = fc.f;
                std::sort(fc.key.begin(), fc.key.end());
                fc.opp = tets4[4 * (size_t)t + k];
                faces.push_back(fc);
            }
        std::vector<int> order(faces.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return faces[a].key < faces[b].key || (faces[a].key == faces[b].key && a < b); });
        std::vector<char> boundary(faces.size(), 0);
        for (size_t i = 0; i < order.size();) {
            size_t j = i + 1;
            while (j < order.size() && faces[order[j]].key == faces[order[i]].key) ++j;
            if (j - i == 1) boundary[order[i]] = 1;
            i = j;
        }
        for (size_t i = 0; i < faces.size(); ++i) {   // tet order
            if (!boundary[i]) continue;
            Face fc = faces[i];
            const double *A = verts3 + 3 * (size_t)fc.f[0], *B = verts3 + 3 * (size_t)fc.f[1], *C = verts3 + 3 * (size_t)fc.f[2],
                         *O = verts3 + 3 * (size_t)fc.opp;
            const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, w[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
            const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            if (n[0] * (O[0] - A[0]) + n[1] * (O[1] - A[1]) + n[2] * (O[2] - A[2]) > 0) std::swap(fc.f[1], fc.f[2]);   // away from the fourth vertex
            m.tris.insert(m.tris.end(), fc.f.begin(), fc.f.end());
        }
        return m;
    }

private:
    PassiveMesh() { type = AA_OBS_MESH; }
};

// Explicit forces (ExplicitForce.hpp:33-47): WindForce on a list of triangles (flat, 3 per face);
// `direction` may be changed between steps (windyflag.cpp's intensity keys)
class ExplicitForce {
public:
    virtual ~ExplicitForce() {}
};
class WindForce : public ExplicitForce {
public:
    explicit WindForce(std::vector<int>& tris_) : tris(tris_), direction{{0, 0, 0}} {}
    std::vector<int> tris;
    Vec3d direction;
    int id = -1;   // device handle once registered
};

class Solver {
public:
    typedef std::vector<double> VecX;      // Eigen::VectorXd in the reference (no Eigen dependency here)
    typedef std::array<double, 3> Vec3;

    // Solver::Settings (Solver.hpp:45-67); `variant` selects the reference copy
    struct Settings {
        enum AccelationType { NOACC = 0, ANDERSON = 1 };
        double timestep_s;
        int verbose;
        int admm_iters;
        double gravity;
        double constraint_w;
        int Anderson_m;
        double penalty;
        AccelationType acceleration_type;
        int variant;
        Settings() : timestep_s(1.0 / 30.0), verbose(1), admm_iters(500), gravity(-9.8), constraint_w(-1),
                     Anderson_m(2), penalty(1.0), acceleration_type(NOACC), variant(AA_VARIANT_UX) {}
    };
    struct RuntimeData : aa_runtime {};

    VecX m_x, m_v, m_masses;   // scaled x3, as the reference
    std::vector<std::shared_ptr<EnergyTerm>> energyterms;
    std::vector<std::shared_ptr<ExplicitForce>> ext_forces;   // Solver.hpp:90

    explicit Solver(int device = 0) {
        check(aa_ctx_create(device, &ctx_));
        check(aa_elastic_create(ctx_, &h_));
    }
    ~Solver() {
        if (h_) aa_elastic_destroy(h_);
        if (ctx_) aa_ctx_destroy(ctx_);
    }
    Solver(const Solver&) = delete;
    Solver& operator=(const Solver&) = delete;

    template <typename T>
    int add_nodes(T* x, T* m, int n_verts) {
        const int prev = (int)m_x.size();
        m_x.resize(prev + 3 * n_verts);
        m_v.resize(prev + 3 * n_verts);
        m_masses.resize(prev + 3 * n_verts);
        for (int i = 0; i < 3 * n_verts; ++i) { m_x[prev + i] = x[i]; m_v[prev + i] = 0; m_masses[prev + i] = m[i]; }
        return (prev + 3 * n_verts) / 3;
    }

    void set_pins(const std::vector<int>& inds, const std::vector<Vec3>& points = std::vector<Vec3>()) {
        pins_ = inds;
        pin_pts_.clear();
        if (points.size() == inds.size())
            for (auto& p : points) { pin_pts_.push_back(p[0]); pin_pts_.push_back(p[1]); pin_pts_.push_back(p[2]); }
        if (initialized_) push_pins();
    }

    // Solver::add_obstacle (Solver.cpp:346-348): takes effect at once, also between steps
    void add_obstacle(std::shared_ptr<PassiveCollision> obj) {
        if (PassiveMesh* m = dynamic_cast<PassiveMesh*>(obj.get()))
            check(aa_elastic_add_mesh_obstacle(h_, m->verts.data(), (int)m->verts.size() / 3, m->tris.data(), (int)m->tris.size() / 3, &m->mesh_id));
        else
            check(aa_elastic_add_obstacle(h_, obj->type, obj->params));
        obstacles_.push_back(obj);   // its row in the insertion order
    }
    // Kinematic obstacles (no reference counterpart; aa_admm.h, aa_elastic_set_mesh_obstacle_pose):
    // the mesh as added, turned by R (row-major 3x3, a rotation) and moved by t, for every later
    // step until changed -- a paddle, a drum, a rising floor. R == nullptr: back to unposed.
    void set_obstacle_pose(const std::shared_ptr<PassiveMesh>& mesh, const double R[9], const double t[3]) {
        if (!mesh || mesh->mesh_id < 0 || row_of(mesh.get()) < 0) throw std::runtime_error("set_obstacle_pose: the mesh was not added to this solver");
        if (!R) { check(aa_elastic_set_mesh_obstacle_pose(h_, mesh->mesh_id, nullptr)); return; }
        double p[12];
        for (int i = 0; i < 9; ++i) p[i] = R[i];
        for (int i = 0; i < 3; ++i) p[9 + i] = t ? t[i] : 0.0;
        check(aa_elastic_set_mesh_obstacle_pose(h_, mesh->mesh_id, p));
    }
    // Deforming obstacles (no reference counterpart; aa_admm.h, aa_elastic_set_mesh_obstacle_vertices):
    // new positions for the mesh's vertices (same count, same triangles, obstacle frame) for every
    // later step until changed -- a breathing body under a cloth. mesh->verts is updated too.
    void set_obstacle_vertices(const std::shared_ptr<PassiveMesh>& mesh, const std::vector<double>& verts3) {
        if (!mesh || mesh->mesh_id < 0 || row_of(mesh.get()) < 0) throw std::runtime_error("set_obstacle_vertices: the mesh was not added to this solver");
        if (verts3.size() != mesh->verts.size()) throw std::runtime_error("set_obstacle_vertices: the vertex count differs from the mesh's");
        check(aa_elastic_set_mesh_obstacle_vertices(h_, mesh->mesh_id, verts3.data()));
        mesh->verts = verts3;
    }
    // Bound obstacles (no reference behaviour: add_dynamic_collider / surface_inds are registered
    // there but never asked; aa_admm.h, aa_elastic_bind_mesh_obstacle): the mesh is the surface of
    // another simulated body -- vertex i follows node nodes[i] from every step's start state, gathered
    // and refitted on the device; an empty list unbinds. exempt_from_obstacle: the collision terms of
    // `nodes` skip the mesh (a body's own nodes; an empty list clears). Before the first
    // initialize() the device solver has no nodes yet: both are kept and handed over with them.
    void bind_obstacle(const std::shared_ptr<PassiveMesh>& mesh, const std::vector<int>& nodes) {
        if (!mesh || mesh->mesh_id < 0 || row_of(mesh.get()) < 0) throw std::runtime_error("bind_obstacle: the mesh was not added to this solver");
        if (!nodes.empty() && 3 * nodes.size() != mesh->verts.size()) throw std::runtime_error("bind_obstacle: one node per vertex of the mesh");
        if (!bound_) { pending_.push_back({0, mesh->mesh_id, nodes}); return; }
        check(aa_elastic_bind_mesh_obstacle(h_, mesh->mesh_id, nodes.empty() ? nullptr : nodes.data(), (int)nodes.size()));
    }
    void exempt_from_obstacle(const std::shared_ptr<PassiveMesh>& mesh, const std::vector<int>& nodes) {
        if (!mesh || mesh->mesh_id < 0 || row_of(mesh.get()) < 0) throw std::runtime_error("exempt_from_obstacle: the mesh was not added to this solver");
        if (!bound_) { pending_.push_back({1, mesh->mesh_id, nodes}); return; }
        check(aa_elastic_set_mesh_obstacle_exempt(h_, mesh->mesh_id, nodes.data(), (int)nodes.size()));
    }
    // refits taken / skipped since the mesh was bound, and the cause of the last skipped one
    void obstacle_status(const std::shared_ptr<PassiveMesh>& mesh, int& refits, int& skipped, int& last_cause) const {
        if (!mesh || mesh->mesh_id < 0) throw std::runtime_error("obstacle_status: the mesh was not added to this solver");
        check(aa_elastic_mesh_obstacle_status(h_, mesh->mesh_id, nullptr, &refits, &skipped, &last_cause));
    }
    // ... and the analytic shapes: change obj->params, then call this to re-send them to the row
    // the obstacle was added as
    void update_obstacle(std::shared_ptr<PassiveCollision> obj) {
        const int row = row_of(obj.get());
        if (row < 0) throw std::runtime_error("update_obstacle: the obstacle was not added to this solver");
        check(aa_elastic_set_obstacle(h_, row, obj->type, obj->params));
    }
    // Coulomb friction against an obstacle (no reference counterpart: Collision::prox only projects;
    // aa_admm.h, aa_elastic_set_obstacle_friction): the coefficient of the obstacle's row, moving
    // obstacles included -- a block stays on an incline, a cloth turns with the drum under it. Lagged
    // and explicit, one pass per step. record_contacts keeps the per-term records with every mu = 0.
    void set_obstacle_friction(const std::shared_ptr<PassiveCollision>& obj, double mu) {
        const int row = row_of(obj.get());
        if (row < 0) throw std::runtime_error("set_obstacle_friction: the obstacle was not added to this solver");
        check(aa_elastic_set_obstacle_friction(h_, row, mu));
    }
    double obstacle_friction(const std::shared_ptr<PassiveCollision>& obj) const {
        const int row = row_of(obj.get());
        if (row < 0) throw std::runtime_error("obstacle_friction: the obstacle was not added to this solver");
        double mu = 0;
        check(aa_elastic_get_obstacle_friction(h_, row, &mu));
        return mu;
    }
    // Carry (aa_admm.h, aa_elastic_set_mesh_obstacle_carry), per mesh, default off: the friction pass
    // takes the mesh's displacement at a contact from its vertices' own motion, so a mesh moved
    // through set_obstacle_vertices or bound to a body drags the nodes on it as a posed one does.
    void set_obstacle_carry(const std::shared_ptr<PassiveMesh>& mesh, bool on = true) {
        if (!mesh || mesh->mesh_id < 0 || row_of(mesh.get()) < 0) throw std::runtime_error("set_obstacle_carry: the mesh was not added to this solver");
        check(aa_elastic_set_mesh_obstacle_carry(h_, mesh->mesh_id, on ? 1 : 0));
    }
    bool obstacle_carry(const std::shared_ptr<PassiveMesh>& mesh) const {
        if (!mesh || mesh->mesh_id < 0 || row_of(mesh.get()) < 0) throw std::runtime_error("obstacle_carry: the mesh was not added to this solver");
        int on = 0;
        check(aa_elastic_get_mesh_obstacle_carry(h_, mesh->mesh_id, &on));
        return on != 0;
    }
    void record_contacts(bool on = true) { check(aa_elastic_record_contacts(h_, on ? 1 : 0)); }
    // the last step's collision terms in contact, in term order
    struct Contact {
        int node, obstacle;         // the caller's node, the obstacle's row in the insertion order
        Vec3 point, normal, slip;   // c, n, and the tangential slip rt relative to the obstacle
        double push, scale;         // j = dt^2 f_n / m, and the share s of the slip taken away
    };
    std::vector<Contact> contacts() const {
        int n = 0;
        check(aa_elastic_get_contacts(h_, 0, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<int> node(n), obs(n);
        std::vector<double> pt(3 * (size_t)n), nr(3 * (size_t)n), sl(3 * (size_t)n), push(n), sc(n);
        if (n) check(aa_elastic_get_contacts(h_, n, &n, node.data(), obs.data(), pt.data(), nr.data(), push.data(), sl.data(), sc.data()));
        std::vector<Contact> out(n);
        for (int k = 0; k < n; ++k) {
            out[k].node = node[k]; out[k].obstacle = obs[k]; out[k].push = push[k]; out[k].scale = sc[k];
            for (int i = 0; i < 3; ++i) { out[k].point[i] = pt[3 * k + i]; out[k].normal[i] = nr[3 * k + i]; out[k].slip[i] = sl[3 * k + i]; }
        }
        return out;
    }
    // Solver::set_collisions (Solver.cpp:318-344): the points are not used by the prox
    // Before the first initialize() the device solver has no nodes yet (see below): the list is
    // kept and handed over with them
    void set_collisions(const std::vector<int>& inds, const std::vector<Vec3>& points = std::vector<Vec3>()) {
        (void)points;
        if (!bound_) { collisions_ = inds; return; }
        check(aa_elastic_set_collisions(h_, inds.data(), (int)inds.size()));
    }

    // Nodes and energy terms are handed to the device solver on the FIRST initialize(); a later
    // initialize() re-runs only the device setup with the new settings (the reference rebuilds
    // its matrices from the same members).
    bool initialize(const Settings& s) {
        settings_ = s;
        if (!bound_) {
            int total = 0;
            if (aa_elastic_add_nodes(h_, m_x.data(), m_masses.data(), (int)m_x.size() / 3, &total) != AA_OK) return false;
            for (auto& e : energyterms) {
                aa_lame l = e->lame.c();
                int rc;
                if (const BendingEnergyTerm* b = dynamic_cast<const BendingEnergyTerm*>(e.get())) {
                    rc = aa_elastic_add_bending(h_, b->verts.data(), b->inds.data(), b->count, b->k_bend, b->flat_rest ? 1 : 0,
                                                b->vertex_offset, nullptr);
                } else if (const SpringEnergyTerm* sp = dynamic_cast<const SpringEnergyTerm*>(e.get())) {
                    rc = aa_elastic_add_springs(h_, sp->has_verts ? sp->verts.data() : nullptr, sp->inds.data(), sp->count, sp->mode,
                                                sp->k.data(), sp->rest.empty() ? nullptr : sp->rest.data(), sp->vertex_offset);
                } else if (const TieEnergyTerm* ti = dynamic_cast<const TieEnergyTerm*>(e.get())) {
                    rc = aa_elastic_add_ties(h_, ti->has_verts ? ti->verts.data() : nullptr, ti->na, ti->nodes_a.data(), ti->w_a.data(),
                                             ti->nb, ti->nodes_b.data(), ti->w_b.data(), ti->count, ti->mode, ti->k.data(),
                                             ti->rest.empty() ? nullptr : ti->rest.data(), ti->vertex_offset);
                } else if (!e->lames.empty()) {   // per-element materials: the _var calls
                    std::vector<aa_lame> ls;
                    for (auto& le : e->lames) ls.push_back(le.c());
                    rc = e->kind == 0
                        ? aa_elastic_add_tets_var(h_, e->verts.data(), e->inds.data(), e->count, e->material, ls.data(), e->vertex_offset)
                        : aa_elastic_add_tris_var(h_, e->verts.data(), e->inds.data(), e->count, ls.data(), e->vertex_offset);
                } else {
                    rc = e->kind == 0
                        ? aa_elastic_add_tets(h_, e->verts.data(), e->inds.data(), e->count, e->material, &l, e->vertex_offset)
                        : aa_elastic_add_tris(h_, e->verts.data(), e->inds.data(), e->count, &l, e->vertex_offset);
                }
                if (rc != AA_OK) return false;
            }
            bound_ = true;
            if (!collisions_.empty() && aa_elastic_set_collisions(h_, collisions_.data(), (int)collisions_.size()) != AA_OK) return false;
            for (auto& p : pending_) {   // bind_obstacle / exempt_from_obstacle calls made before the nodes existed
                const int rc = p.kind == 0
                    ? aa_elastic_bind_mesh_obstacle(h_, p.mesh_id, p.nodes.empty() ? nullptr : p.nodes.data(), (int)p.nodes.size())
                    : aa_elastic_set_mesh_obstacle_exempt(h_, p.mesh_id, p.nodes.data(), (int)p.nodes.size());
                if (rc != AA_OK) return false;
            }
            pending_.clear();
        }
        push_pins();
        aa_settings cs{s.timestep_s, s.verbose, s.admm_iters, s.gravity, s.constraint_w, s.Anderson_m, s.penalty,
                       (int)s.acceleration_type, s.variant, 0.0};
        if (aa_elastic_initialize(h_, &cs) != AA_OK) return false;
        initialized_ = true;
        x_seen_.clear();
        v_seen_.clear();
        return true;
    }

    // m_x / m_v edited by the caller between steps (the reference reads them directly) are pushed
    // to the device first.
    void step() {
        for (auto& f : ext_forces) {   // register new forces, push the current wind directions
            auto w = std::dynamic_pointer_cast<WindForce>(f);
            if (!w) throw std::runtime_error("ext_forces: only WindForce is provided");
            if (w->id < 0) check(aa_elastic_add_wind(h_, w->tris.data(), (int)w->tris.size() / 3, w->direction.data(), &w->id));
            else check(aa_elastic_set_wind(h_, w->id, w->direction.data()));
        }
        if (!x_seen_.empty() && x_seen_ != m_x) check(aa_elastic_set_x(h_, m_x.data()));
        if (!v_seen_.empty() && v_seen_ != m_v) check(aa_elastic_set_v(h_, m_v.data()));
        check(aa_elastic_step(h_));
        check(aa_elastic_get_x(h_, m_x.data()));
        check(aa_elastic_get_v(h_, m_v.data()));
        x_seen_ = m_x;
        v_seen_ = m_v;
        save(true);
    }

    // Solver::save() (Solver.hpp:130-155, called at the end of every step, Solver.cpp:232/262):
    // ./result/residual-<m>.txt (or residual-no.txt) with one row per iteration of the last step:
    // time (ms since the step started; device clock), prim, comb and -- (u,x) variant
    // (admm_anderson_hard_zxu) only -- the reject flag, %.16g as `ofs << setprecision(16)`.
    // quiet: skip silently when ./result does not exist (the reference prints "Cannot open").
    bool save(bool quiet = false) const {
        const std::string file = settings_.acceleration_type ? "./result/residual-" + std::to_string(settings_.Anderson_m) + ".txt"
                                                             : std::string("./result/residual-no.txt");
        std::FILE* f = std::fopen(file.c_str(), "w");
        if (!f) {
            if (!quiet) std::printf("Cannot open: %s\n", file.c_str());
            return false;
        }
        std::vector<double> prim, comb, t;
        std::vector<int> rej;
        const int n = history(prim, comb, rej);
        int nt = 0;
        check(aa_elastic_get_times(h_, nullptr, 0, &nt));
        t.assign(std::max(n, nt), 0.0);
        if (nt) check(aa_elastic_get_times(h_, t.data(), nt, &nt));
        for (int i = 0; i < n; ++i) {
            if (settings_.variant == AA_VARIANT_UX) std::fprintf(f, "%.16g\t%.16g\t%.16g\t%d\n", t[i], prim[i], comb[i], rej[i]);
            else std::fprintf(f, "%.16g\t%.16g\t%.16g\n", t[i], prim[i], comb[i]);
        }
        std::fclose(f);
        return true;
    }

    const Settings& settings() const { return settings_; }
    RuntimeData runtime_data() const {
        RuntimeData r;
        check(aa_elastic_runtime(h_, &r));
        return r;
    }
    // the (prim, comb, reject) rows Solver::save() writes (Solver.hpp:130-155)
    int history(std::vector<double>& prim, std::vector<double>& comb, std::vector<int>& rej) const {
        int n = 0;
        check(aa_elastic_get_history(h_, nullptr, nullptr, nullptr, 0, &n));
        prim.resize(n); comb.resize(n); rej.resize(n);
        check(aa_elastic_get_history(h_, prim.data(), comb.data(), rej.data(), n, &n));
        return n;
    }

private:
    void push_pins() {
        check(aa_elastic_set_pins(h_, pins_.data(), pin_pts_.empty() ? nullptr : pin_pts_.data(), (int)pins_.size()));
    }
    aa_ctx ctx_ = nullptr;
    aa_elastic h_ = nullptr;
    Settings settings_;
    bool initialized_ = false, bound_ = false;
    VecX x_seen_, v_seen_;
    std::vector<int> pins_, collisions_;
    std::vector<double> pin_pts_;
    std::vector<std::shared_ptr<PassiveCollision>> obstacles_;   // by row of the insertion order
    struct PendingNodes { int kind, mesh_id; std::vector<int> nodes; };   // kind 0 bind, 1 exempt
    std::vector<PendingNodes> pending_;
    int row_of(const PassiveCollision* o) const {
        for (size_t k = 0; k < obstacles_.size(); ++k)
            if (obstacles_[k].get() == o) return (int)k;
        return -1;
    }
};

}  // namespace admm

#endif  // AA_ADMM_HPP
