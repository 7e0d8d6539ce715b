// C++ caller of the drop-in facade (include/aa_admm.hpp) for a carrying mesh obstacle: the tet block
// on a slab whose vertices are translated in x before every step (scenes.block_on_conveyor_mesh),
// the slab's friction set through Solver::set_obstacle_friction and its carry through
// Solver::set_obstacle_carry, the contacts read through Solver::contacts().
// usage: facade_carry scene.bin out.bin
// scene.bin: int32 n, nt, nb, steps, iters, aa_m, nv, nf; float64 shift, mu, dt, E, nu; then x (3 n),
//            rest (3 n), masses (n) as float64; tets (4 nt), bottom nodes (nb) as int32; the slab's
//            vertices (3 nv) as float64 and triangles (3 nf) as int32.
// out.bin:   int32 contacts of the last step, sticking ones (scale == 1); float64 x (3 n).
#include <cstdio>
#include <memory>
#include <vector>

#include "aa_admm.hpp"

template <typename T>
static bool get(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int> hd, tets, bottom, F;
    std::vector<double> pr, x, rest, mass, V;
    if (!get(f, hd, 8) || !get(f, pr, 5)) return 2;
    const int n = hd[0], nt = hd[1], nb = hd[2], steps = hd[3], nv = hd[6], nf = hd[7];
    if (!get(f, x, 3 * (size_t)n) || !get(f, rest, 3 * (size_t)n) || !get(f, mass, (size_t)n) || !get(f, tets, 4 * (size_t)nt) ||
        !get(f, bottom, (size_t)nb) || !get(f, V, 3 * (size_t)nv) || !get(f, F, 3 * (size_t)nf))
        return 2;
    std::fclose(f);
    std::vector<double> m3(3 * (size_t)n);
    for (int i = 0; i < 3 * n; ++i) m3[i] = mass[i / 3];

    admm::Solver solver;
    solver.add_nodes(x.data(), m3.data(), n);
    admm::create_tets_from_mesh<double, admm::TetEnergyTerm>(solver.energyterms, rest.data(), tets.data(), nt, admm::Lame(pr[3], pr[4]), 0);
    auto slab = std::make_shared<admm::PassiveMesh>(admm::PassiveMesh::from_surface(V.data(), nv, F.data(), nf));
    {   // a mesh that was never added
        bool threw = false;
        try { solver.set_obstacle_carry(slab); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("set_obstacle_carry took a mesh that was never added\n"); return 1; }
    }
    solver.add_obstacle(slab);
    solver.set_collisions(bottom);
    solver.set_obstacle_friction(slab, pr[1]);
    solver.record_contacts();
    if (solver.obstacle_carry(slab)) { std::printf("carry is on by default\n"); return 1; }
    solver.set_obstacle_carry(slab);
    if (!solver.obstacle_carry(slab)) { std::printf("the switch did not come back\n"); return 1; }
    admm::Solver::Settings st;
    st.timestep_s = pr[2];
    st.admm_iters = hd[4];
    st.acceleration_type = admm::Solver::Settings::ANDERSON;
    st.Anderson_m = hd[5];
    st.verbose = 0;
    if (!solver.initialize(st)) { std::printf("initialize failed: %s\n", aa_last_error()); return 1; }
    std::vector<double> W(V);
    for (int k = 1; k <= steps; ++k) {
        for (int i = 0; i < nv; ++i) W[3 * (size_t)i] = V[3 * (size_t)i] + k * pr[0];
        solver.set_obstacle_vertices(slab, W);
        solver.step();
    }
    const std::vector<admm::Solver::Contact> cs = solver.contacts();
    int out[2] = {(int)cs.size(), 0};
    for (auto& c : cs) out[1] += c.scale == 1.0 ? 1 : 0;
    std::FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 2;
    std::fwrite(out, sizeof(int), 2, g);
    std::fwrite(solver.m_x.data(), sizeof(double), solver.m_x.size(), g);
    std::fclose(g);
    return 0;
}
