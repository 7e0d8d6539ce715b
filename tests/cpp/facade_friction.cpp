// C++ caller of the drop-in facade (include/aa_admm.hpp) for obstacle friction: a tet block on a
// tilted SlideFloor (scenes.block_on_incline), the coefficient set through
// Solver::set_obstacle_friction, the contacts read through Solver::contacts().
// usage: facade_friction scene.bin out.bin
// scene.bin: int32 n, nt, nb, steps, iters, aa_m; float64 nx, ny, mu, dt, E, nu; then x (3 n),
//            rest (3 n), masses (n) as float64; tets (4 nt), bottom nodes (nb) as int32.
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
    std::vector<int> hd, tets, bottom;
    std::vector<double> pr, x, rest, mass;
    if (!get(f, hd, 6) || !get(f, pr, 6)) return 2;
    const int n = hd[0], nt = hd[1], nb = hd[2], steps = hd[3];
    if (!get(f, x, 3 * (size_t)n) || !get(f, rest, 3 * (size_t)n) || !get(f, mass, (size_t)n) || !get(f, tets, 4 * (size_t)nt) ||
        !get(f, bottom, (size_t)nb))
        return 2;
    std::fclose(f);
    std::vector<double> m3(3 * (size_t)n);
    for (int i = 0; i < 3 * n; ++i) m3[i] = mass[i / 3];

    admm::Solver solver;
    solver.add_nodes(x.data(), m3.data(), n);
    admm::create_tets_from_mesh<double, admm::TetEnergyTerm>(solver.energyterms, rest.data(), tets.data(), nt, admm::Lame(pr[4], pr[5]), 0);
    auto incline = std::make_shared<admm::SlideFloor>(admm::Vec3d{{0.0, 0.0, 0.0}}, admm::Vec3d{{pr[0], pr[1], 0.0}});
    solver.add_obstacle(incline);
    solver.set_collisions(bottom);
    solver.set_obstacle_friction(incline, pr[2]);
    solver.record_contacts();
    if (solver.obstacle_friction(incline) != pr[2]) { std::printf("the coefficient did not come back\n"); return 1; }
    admm::Solver::Settings st;
    st.timestep_s = pr[3];
    st.admm_iters = hd[4];
    st.acceleration_type = admm::Solver::Settings::ANDERSON;
    st.Anderson_m = hd[5];
    st.verbose = 0;
    if (!solver.initialize(st)) { std::printf("initialize failed: %s\n", aa_last_error()); return 1; }
    for (int k = 0; k < steps; ++k) solver.step();
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
