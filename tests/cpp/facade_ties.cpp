// C++ caller of the drop-in facade (include/aa_admm.hpp) with ties: tests/test_facade_ties.py's scene
// -- the triangle (-0.3, 0, -0.2), (0.4, 0, -0.1), (0, 0, 0.5) pinned in place and three masses of 0.01
// below it, joined in a ring by springs (k = 30, derived lengths). One create_ties call hangs each
// mass from a point of the triangle (na = 3, nb = 1, k = 50 + e, rest = 0.3 given, vertices null,
// AA_SPRING_TETHER); a second ties the point (0.5, 0.5) of the free edge (4, 5) to the point (0.25,
// 0.75) of the pinned edge (0, 1) (na = nb = 2, k = 20, rest derived from the vertices, AA_SPRING).
// (u,x)-Anderson m=4, 30 iterations, three steps. Writes "<n nodes (int32)> <x (3n doubles)>
// <v (3n doubles)>" to argv[1].
#include <cstdio>
#include <vector>

#include "aa_admm.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: facade_ties out.bin\n"); return 2; }
    const double T[3][3] = {{-0.3, 0.0, -0.2}, {0.4, 0.0, -0.1}, {0.0, 0.0, 0.5}};
    const double W[3][3] = {{0.2, 0.3, 0.5}, {0.6, 0.3, 0.1}, {0.15, 0.7, 0.15}};
    const double off[3][3] = {{0.1, -0.35, 0.05}, {-0.05, -0.3, 0.1}, {0.0, -0.4, -0.1}};
    std::vector<double> v, m;
    for (int i = 0; i < 3; ++i) for (int d = 0; d < 3; ++d) v.push_back(T[i][d]);
    for (int e = 0; e < 3; ++e)
        for (int d = 0; d < 3; ++d) v.push_back(((W[e][0] * T[0][d] + W[e][1] * T[1][d]) + W[e][2] * T[2][d]) + off[e][d]);
    const int n = 6;
    for (int q = 0; q < 3 * n; ++q) m.push_back(0.01);
    const std::vector<int> ring = {3, 4, 4, 5, 5, 3};
    const std::vector<double> k_ring(3, 30.0);
    const std::vector<int> a1 = {0, 1, 2, 0, 1, 2, 0, 1, 2}, b1 = {3, 4, 5};
    const std::vector<double> wa1 = {0.2, 0.3, 0.5, 0.6, 0.3, 0.1, 0.15, 0.7, 0.15}, wb1(3, 1.0), k1 = {50.0, 51.0, 52.0}, rest1(3, 0.3);
    const std::vector<int> a2 = {0, 1}, b2 = {4, 5};
    const std::vector<double> wa2 = {0.25, 0.75}, wb2 = {0.5, 0.5}, k2 = {20.0};
    admm::Solver solver;
    solver.add_nodes(v.data(), m.data(), n);
    admm::create_springs<double>(solver.energyterms, v.data(), ring.data(), 3, k_ring.data(), nullptr, AA_SPRING, 0);
    admm::create_ties<double>(solver.energyterms, nullptr, 3, a1.data(), wa1.data(), 1, b1.data(), wb1.data(), 3, k1.data(), rest1.data(),
                              AA_SPRING_TETHER, 0);
    admm::create_ties<double>(solver.energyterms, v.data(), 2, a2.data(), wa2.data(), 2, b2.data(), wb2.data(), 1, k2.data(), nullptr,
                              AA_SPRING, 0);
    solver.set_pins({0, 1, 2});
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
