// admm::PassiveMesh of the drop-in facade (include/aa_admm.hpp).
// Without arguments (no GPU): PassiveMesh::from_tets takes the boundary faces of a tet mesh, the
// faces used by exactly one tet, oriented outward -- checked on one tet of either orientation and
// on a cube of five tets. Prints "ok".
// With "run" (GPU): a small unpinned cloth falls on a box given as those five tets; prints the
// lowest node height after 12 steps (the box's top is at y = 0).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "aa_admm.hpp"

namespace {
double signed_volume(const admm::PassiveMesh& m) {
    double s = 0;
    for (size_t t = 0; t + 2 < m.tris.size(); t += 3) {
        const double *a = &m.verts[3 * m.tris[t]], *b = &m.verts[3 * m.tris[t + 1]], *c = &m.verts[3 * m.tris[t + 2]];
        s += a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    }
    return s / 6.0;
}
bool closed(const admm::PassiveMesh& m) {   // every directed edge once, its reverse once
    std::map<std::pair<int, int>, int> dir;
    for (size_t t = 0; t + 2 < m.tris.size(); t += 3)
        for (int a = 0; a < 3; ++a) ++dir[{m.tris[t + a], m.tris[t + (a + 1) % 3]}];
    for (auto& kv : dir)
        if (kv.second != 1 || dir.count({kv.first.second, kv.first.first}) == 0) return false;
    return true;
}
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
    if (argc < 2) {
        const double v[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
        const int pos[4] = {0, 1, 2, 3}, neg[4] = {0, 2, 1, 3};
        for (const int* tet : {pos, neg}) {
            const admm::PassiveMesh m = admm::PassiveMesh::from_tets(v, 4, tet, 1);
            if (m.tris.size() != 12 || !closed(m) || std::fabs(signed_volume(m) - 1.0 / 6.0) > 1e-15) { std::printf("FAIL one tet\n"); return 1; }
        }
        const double lo[3] = {-1, -2, -3}, hi[3] = {1, 0, 2};
        std::vector<double> bv;
        std::vector<int> bt;
        box_tets(lo, hi, bv, bt);
        const admm::PassiveMesh m = admm::PassiveMesh::from_tets(bv.data(), 8, bt.data(), 5);
        if (m.tris.size() != 36 || !closed(m) || std::fabs(signed_volume(m) - 20.0) > 1e-13) { std::printf("FAIL box: %zu faces, volume %g\n", m.tris.size() / 3, signed_volume(m)); return 1; }
        const admm::PassiveMesh s = admm::PassiveMesh::from_surface(m.verts.data(), 8, m.tris.data(), 12);
        if (s.type != AA_OBS_MESH || s.tris != m.tris) { std::printf("FAIL from_surface\n"); return 1; }
        std::printf("ok\n");
        return 0;
    }
    if (std::strcmp(argv[1], "run") != 0) return 2;
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
        solver.add_obstacle(std::make_shared<admm::PassiveMesh>(admm::PassiveMesh::from_tets(bv.data(), 8, bt.data(), 5)));
        std::vector<int> all(n);
        for (int i = 0; i < n; ++i) all[i] = i;
        solver.set_collisions(all);
        admm::Solver::Settings st;
        st.admm_iters = 30;
        st.verbose = 0;
        if (!solver.initialize(st)) { std::printf("initialize failed\n"); return 1; }
        for (int k = 0; k < 12; ++k) solver.step();
        double ymin = 1e300;
        for (int i = 0; i < n; ++i) ymin = std::fmin(ymin, solver.m_x[3 * i + 1]);
        std::printf("%.17g\n", ymin);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
