// C++ caller of the drop-in facade (include/aa_admm.hpp) with springs: tests/test_facade_springs.py's
// scene -- a 5 x 5 net of nodes 0.25 apart in the x-z plane, node mass 0.01, corners pinned; its 40
// structural springs through one create_springs call (k = 50, rest lengths derived from the
// vertices, AA_SPRING), its 32 shear springs through a second (k = 20 + e, rest = 1.1 x 0.25 sqrt 2
// given, AA_SPRING_TETHER). (u,x)-Anderson m=4, 30 iterations, three steps. Writes
// "<n nodes (int32)> <x (3n doubles)> <v (3n doubles)>" to argv[1].
#include <cmath>
#include <cstdio>
#include <vector>

#include "aa_admm.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: facade_springs out.bin\n"); return 2; }
    const int nx = 5, ny = 5;
    std::vector<double> v, m;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) { v.push_back(i * 0.25); v.push_back(0.0); v.push_back(j * 0.25); }
    const int n = nx * ny;
    for (int q = 0; q < 3 * n; ++q) m.push_back(0.01);
    std::vector<int> st, sh;   // scenes.net_pairs' order
    for (int j = 0; j < ny; ++j) for (int i = 0; i + 1 < nx; ++i) { st.push_back(j * nx + i); st.push_back(j * nx + i + 1); }
    for (int j = 0; j + 1 < ny; ++j) for (int i = 0; i < nx; ++i) { st.push_back(j * nx + i); st.push_back((j + 1) * nx + i); }
    for (int j = 0; j + 1 < ny; ++j)
        for (int i = 0; i + 1 < nx; ++i) {
            sh.push_back(j * nx + i); sh.push_back((j + 1) * nx + i + 1);
            sh.push_back(j * nx + i + 1); sh.push_back((j + 1) * nx + i);
        }
    const int n_st = (int)st.size() / 2, n_sh = (int)sh.size() / 2;
    std::vector<double> k_st(n_st, 50.0), k_sh(n_sh), rest_sh(n_sh, 1.1 * (0.25 * std::sqrt(2.0)));
    for (int e = 0; e < n_sh; ++e) k_sh[e] = 20.0 + e;
    admm::Solver solver;
    solver.add_nodes(v.data(), m.data(), n);
    admm::create_springs<double>(solver.energyterms, v.data(), st.data(), n_st, k_st.data(), nullptr, AA_SPRING, 0);
    admm::create_springs<double>(solver.energyterms, nullptr, sh.data(), n_sh, k_sh.data(), rest_sh.data(), AA_SPRING_TETHER, 0);
    solver.set_pins({0, nx - 1, (ny - 1) * nx, ny * nx - 1});
    admm::Solver::Settings s;
    s.admm_iters = 30;
    s.acceleration_type = admm::Solver::Settings::ANDERSON;
    s.Anderson_m = 4;
    s.verbose = 0;
    if (!solver.initialize(s)) { std::printf("initialize failed: %s\n", aa_last_error()); return 1; }
    for (int k = 0; k < 3; ++k) solver.step();
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 1;
    std::fwrite(&n, sizeof(int), 1, f);
    std::fwrite(solver.m_x.data(), sizeof(double), solver.m_x.size(), f);
    std::fwrite(solver.m_v.data(), sizeof(double), solver.m_v.size(), f);
    std::fclose(f);
    return 0;
}
