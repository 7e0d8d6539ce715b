// C++ caller of the drop-in facade (include/aa_admm.hpp) with per-element materials: a graded
// make_tet_blocks(8, 2, 2) NeoHookean cantilever whose stiffness rises along x, bound the way a
// reference caller would loop over the tets with one Lame each -- here through the
// std::vector<Lame> overload of create_tets_from_mesh, i.e. as one group. z-Anderson m=6, two
// steps. Writes "<n nodes (int32)> <x (3n doubles)> <v (3n doubles)>" to argv[1].
#include <cstdio>
#include <vector>

#include "aa_admm.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: facade_varmat out.bin\n"); return 2; }
    const int cx = 8, cy = 2, cz = 2;
    std::vector<double> v;
    std::vector<int> t;
    std::vector<admm::Lame> lames;
    for (int i = 0; i <= cx; ++i)
        for (int j = 0; j <= cy; ++j)
            for (int k = 0; k <= cz; ++k) { v.push_back(i / 2.0); v.push_back(j / 2.0); v.push_back(k / 2.0); }
    auto node = [&](int i, int j, int k) { return (i * (cy + 1) + j) * (cz + 1) + k; };
    const int table[5][4] = {{0, 5, 7, 4}, {5, 7, 2, 0}, {5, 0, 2, 1}, {7, 2, 0, 3}, {5, 2, 7, 6}};
    for (int X = 0; X < cx; ++X)
        for (int Y = 0; Y < cy; ++Y)
            for (int Z = 0; Z < cz; ++Z) {
                // corner labels a..h of make_tet_blocks (ShapeFactory.hpp:436-496)
                const int lab[8] = {node(X + 1, Y + 1, Z + 1), node(X, Y + 1, Z + 1), node(X, Y + 1, Z), node(X + 1, Y + 1, Z),
                                    node(X + 1, Y, Z + 1), node(X, Y, Z + 1), node(X, Y, Z), node(X + 1, Y, Z)};
                for (auto& row : table) {
                    for (int a = 0; a < 4; ++a) t.push_back(lab[row[a]]);
                    lames.push_back(admm::Lame(1e5 + 9.9e6 * X / 7.0, 0.30 + 0.15 * X / 7.0));   // graded along x
                }
            }
    const int n = (int)v.size() / 3;
    std::vector<double> m(3 * n, 0.05);
    admm::Solver solver;
    solver.add_nodes(v.data(), m.data(), n);
    admm::create_tets_from_mesh<double, admm::NeoHookeanTet>(solver.energyterms, v.data(), t.data(), (int)t.size() / 4, lames, 0);
    std::vector<int> pins;
    for (int q = 0; q < n; ++q) if (v[3 * q] == 0.0) pins.push_back(q);
    solver.set_pins(pins);
    admm::Solver::Settings st;
    st.admm_iters = 30;
    st.acceleration_type = admm::Solver::Settings::ANDERSON;
    st.Anderson_m = 6;
    st.variant = AA_VARIANT_Z;
    st.verbose = 0;
    if (!solver.initialize(st)) { std::printf("initialize failed: %s\n", aa_last_error()); return 1; }
    solver.step();
    solver.step();
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 1;
    std::fwrite(&n, sizeof(int), 1, f);
    std::fwrite(solver.m_x.data(), sizeof(double), solver.m_x.size(), f);
    std::fwrite(solver.m_v.data(), sizeof(double), solver.m_v.size(), f);
    std::fclose(f);
    return 0;
}
