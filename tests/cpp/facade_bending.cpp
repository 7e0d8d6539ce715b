// C++ caller of the drop-in facade (include/aa_admm.hpp) with bending: the 3 x 3-vertex sheet of
// tests/bending_cases.py grid3_scene -- cloth membrane (Lame(50, 0.1), limits [0.95, 1.05]) through
// create_tris_from_mesh plus hinges of stiffness 1e-2 through create_bending_from_mesh, the centre
// node and a corner pinned, (u,x)-Anderson m=4, 30 iterations, three steps. Writes
// "<n nodes (int32)> <x (3n doubles)> <v (3n doubles)>" to argv[1].
#include <cmath>
#include <cstdio>
#include <vector>

#include "aa_admm.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: facade_bending out.bin\n"); return 2; }
    const int nx = 2, ny = 2;
    std::vector<double> v;
    std::vector<int> t;
    for (int j = 0; j <= ny; ++j)
        for (int i = 0; i <= nx; ++i) { v.push_back(i * 0.5); v.push_back(0.0); v.push_back(j * 0.5); }
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const int a = j * (nx + 1) + i, b = a + 1, c = a + nx + 1, d = c + 1;
            const int tri[6] = {a, b, d, a, d, c};
            t.insert(t.end(), tri, tri + 6);
        }
    const int n = (int)v.size() / 3, nt = (int)t.size() / 3;
    // area density 1, a third of each triangle's area to each corner (scenes.tri_masses' order of sums)
    std::vector<double> mass(n, 0.0), m;
    for (int k = 0; k < 3; ++k)
        for (int e = 0; e < nt; ++e) {
            const double *A = &v[3 * t[3 * e]], *B = &v[3 * t[3 * e + 1]], *C = &v[3 * t[3 * e + 2]];
            const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, w[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
            const double cr[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double area = 0.5 * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
            mass[t[3 * e + k]] += 1.0 * area / 3.0;
        }
    for (int q = 0; q < n; ++q) for (int d = 0; d < 3; ++d) m.push_back(mass[q]);
    admm::Solver solver;
    solver.add_nodes(v.data(), m.data(), n);
    admm::Lame lame(50, 0.1);
    lame.limit_min = 0.95;
    lame.limit_max = 1.05;
    admm::create_tris_from_mesh<double, admm::TriEnergyTerm>(solver.energyterms, v.data(), t.data(), nt, lame, 0);
    admm::create_bending_from_mesh<double>(solver.energyterms, v.data(), t.data(), nt, 1e-2, true, 0);
    solver.set_pins({4, 0});
    admm::Solver::Settings st;
    st.admm_iters = 30;
    st.acceleration_type = admm::Solver::Settings::ANDERSON;
    st.Anderson_m = 4;
    st.verbose = 0;
    if (!solver.initialize(st)) { std::printf("initialize failed: %s\n", aa_last_error()); return 1; }
    for (int k = 0; k < 3; ++k) solver.step();
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 1;
    std::fwrite(&n, sizeof(int), 1, f);
    std::fwrite(solver.m_x.data(), sizeof(double), solver.m_x.size(), f);
    std::fwrite(solver.m_v.data(), sizeof(double), solver.m_v.size(), f);
    std::fclose(f);
    return 0;
}
