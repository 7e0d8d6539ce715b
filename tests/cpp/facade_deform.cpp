// Deforming obstacles of the drop-in facade (include/aa_admm.hpp): admm::Solver::set_obstacle_vertices.
// With "run" (GPU): a small unpinned cloth falls on a box given as five tets (top face at y = 0)
// whose four top vertices set_obstacle_vertices lifts by 0.02 before every step, the bottom staying
// where it is. Prints the height of the box's top face after 12 steps and the lowest node height.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "aa_admm.hpp"

namespace {
// the box [lo, hi] as five tets (corner index = 4 x + 2 y + z)
void box_tets(const double lo[3], const double hi[3], std::vector<double>& v, std::vector<int>& t) {
    for (int x = 0; x < 2; ++x) for (int y = 0; y < 2; ++y) for (int z = 0; z < 2; ++z) {
        v.push_back(x ? hi[0] : lo[0]); v.push_back(y ? hi[1] : lo[1]); v.push_back(z ? hi[2] : lo[2]);
    }
    const int tets[20] = {0, 3, 5, 6,  0, 1, 3, 5,  0, 2, 6, 3,  0, 4, 5, 6,  7, 6, 5, 3};
    t.assign(tets, tets + 20);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "run") != 0) return 2;
    try {
        const int nx = 6, ny = 6;
        const double h = 0.1, y_start = 0.05;
        std::vector<double> v;
        std::vector<int> t;
        auto corner = [&](int i, int j) { return i * (ny + 1) + j; };
        for (int i = 0; i <= nx; ++i) for (int j = 0; j <= ny; ++j) { v.push_back(i * h); v.push_back(y_start); v.push_back(j * h); }
        const int c0 = (nx + 1) * (ny + 1);
        for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) { v.push_back((i + 0.5) * h); v.push_back(y_start); v.push_back((j + 0.5) * h); }
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j) {
                const int a = corner(i, j), b = corner(i + 1, j), c = corner(i + 1, j + 1), d = corner(i, j + 1), e = c0 + i * ny + j;
                const int tri[12] = {d, a, e, a, b, e, b, c, e, c, d, e};
                t.insert(t.end(), tri, tri + 12);
            }
        const int n = (int)v.size() / 3;
        std::vector<double> m(3 * n, 1e-3);
        admm::Solver solver;
        solver.add_nodes(v.data(), m.data(), n);
        admm::Lame lame(50, 0.1);
        admm::create_tris_from_mesh<double, admm::TriEnergyTerm>(solver.energyterms, v.data(), t.data(), (int)t.size() / 3, lame, 0);
        const double lo[3] = {-1, -1, -1}, hi[3] = {2, 0, 2};
        std::vector<double> bv;
        std::vector<int> bt;
        box_tets(lo, hi, bv, bt);
        auto box = std::make_shared<admm::PassiveMesh>(admm::PassiveMesh::from_tets(bv.data(), 8, bt.data(), 5));
        bool threw = false;
        try { solver.set_obstacle_vertices(box, box->verts); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("set_obstacle_vertices took a mesh that was never added\n"); return 1; }
        solver.add_obstacle(box);
        threw = false;
        try { solver.set_obstacle_vertices(box, std::vector<double>(3)); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("set_obstacle_vertices took a wrong vertex count\n"); return 1; }
        std::vector<int> all(n);
        for (int i = 0; i < n; ++i) all[i] = i;
        solver.set_collisions(all);
        admm::Solver::Settings st;
        st.admm_iters = 30;
        st.verbose = 0;
        if (!solver.initialize(st)) { std::printf("initialize failed\n"); return 1; }
        const std::vector<double> rest = box->verts;
        const double lift = 0.02;
        double top = 0;
        for (int k = 1; k <= 12; ++k) {
            top = lift * k;
            std::vector<double> w = rest;
            for (size_t i = 0; i < w.size() / 3; ++i)
                if (rest[3 * i + 1] == hi[1]) w[3 * i + 1] = top;
            solver.set_obstacle_vertices(box, w);
            if (box->verts != w) { std::printf("mesh->verts not updated\n"); return 1; }
            solver.step();
        }
        double ymin = 1e300;
        for (int i = 0; i < n; ++i) ymin = std::fmin(ymin, solver.m_x[3 * i + 1]);
        std::printf("%.17g %.17g\n", top, ymin);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
