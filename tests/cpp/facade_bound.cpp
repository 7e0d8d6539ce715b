// Bound obstacles of the drop-in facade (include/aa_admm.hpp): admm::Solver::bind_obstacle and
// exempt_from_obstacle. With "run" (GPU): a soft linear-tet block (3 x 2 x 3 cubes of side 0.3 cut
// into six tets each, bottom face pinned, top face at y = 0.6) sags under its own weight; its boundary
// is a PassiveMesh bound to its nodes. A small unpinned cloth starts 0.05 above the top face; its
// nodes are the collision nodes. Prints, after 8 steps: the lowest and highest node of the block's top
// face, the height of the cloth's middle node, and the refits taken and skipped.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "aa_admm.hpp"

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "run") != 0) return 2;
    try {
        // the block: lattice nodes, six tets per cube around the cube's main diagonal (conforming)
        const int cx = 3, cy = 2, cz = 3;
        const double cell = 0.3, density = 1522.0;
        auto node = [&](int i, int j, int k) { return (i * (cy + 1) + j) * (cz + 1) + k; };
        std::vector<double> bv;
        for (int i = 0; i <= cx; ++i) for (int j = 0; j <= cy; ++j) for (int k = 0; k <= cz; ++k) { bv.push_back(i * cell); bv.push_back(j * cell); bv.push_back(k * cell); }
        const int nb = (int)bv.size() / 3;
        const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        const bool odd[6] = {false, true, true, false, false, true};
        std::vector<int> bt;
        for (int i = 0; i < cx; ++i) for (int j = 0; j < cy; ++j) for (int k = 0; k < cz; ++k)
            for (int p = 0; p < 6; ++p) {
                int c[3] = {i, j, k}, q[4];
                q[0] = node(c[0], c[1], c[2]);
                for (int a = 0; a < 3; ++a) { ++c[perms[p][a]]; q[a + 1] = node(c[0], c[1], c[2]); }
                if (odd[p]) std::swap(q[1], q[2]);
                bt.insert(bt.end(), q, q + 4);
            }
        std::vector<double> bm(3 * nb, 0.0);
        for (size_t t = 0; t < bt.size() / 4; ++t)
            for (int a = 0; a < 4; ++a)
                for (int d = 0; d < 3; ++d) bm[3 * bt[4 * t + a] + d] += density * (cell * cell * cell / 6.0) / 4.0;
        // the cloth: n x n cells with a centre node each, a little wider than the block
        const int n = 8;
        const double side = 1.08, h = side / n, top0 = cy * cell, y_start = top0 + 0.05, off = 0.5 * (cx * cell - side);
        std::vector<double> cv;
        std::vector<int> ct;
        auto corner = [&](int i, int j) { return i * (n + 1) + j; };
        for (int i = 0; i <= n; ++i) for (int j = 0; j <= n; ++j) { cv.push_back(off + i * h); cv.push_back(y_start); cv.push_back(off + j * h); }
        const int c0 = (n + 1) * (n + 1);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { cv.push_back(off + (i + 0.5) * h); cv.push_back(y_start); cv.push_back(off + (j + 0.5) * h); }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const int a = corner(i, j), b = corner(i + 1, j), c = corner(i + 1, j + 1), d = corner(i, j + 1), e = c0 + i * n + j;
                const int tri[12] = {d, a, e, a, b, e, b, c, e, c, d, e};
                ct.insert(ct.end(), tri, tri + 12);
            }
        const int nc = (int)cv.size() / 3;
        std::vector<double> cm(3 * nc, 4e-3);

        admm::Solver solver;
        solver.add_nodes(bv.data(), bm.data(), nb);
        solver.add_nodes(cv.data(), cm.data(), nc);
        admm::create_tets_from_mesh<double, admm::TetEnergyTerm>(solver.energyterms, bv.data(), bt.data(), (int)bt.size() / 4, admm::Lame(5e4, 0.3), 0);
        admm::create_tris_from_mesh<double, admm::TriEnergyTerm>(solver.energyterms, cv.data(), ct.data(), (int)ct.size() / 3, admm::Lame(50, 0.1), nb);
        std::vector<int> pins, top, block_nodes(nb), cloth_nodes(nc);
        std::vector<admm::Solver::Vec3> pin_pts;
        for (int i = 0; i < nb; ++i) {
            block_nodes[i] = i;
            if (bv[3 * i + 1] == 0.0) { pins.push_back(i); pin_pts.push_back({bv[3 * i], bv[3 * i + 1], bv[3 * i + 2]}); }
            if (bv[3 * i + 1] == top0) top.push_back(i);
        }
        for (int i = 0; i < nc; ++i) cloth_nodes[i] = nb + i;
        solver.set_pins(pins, pin_pts);

        auto skin = std::make_shared<admm::PassiveMesh>(admm::PassiveMesh::from_tets(bv.data(), nb, bt.data(), (int)bt.size() / 4));
        bool threw = false;
        try { solver.bind_obstacle(skin, block_nodes); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("bind_obstacle took a mesh that was never added\n"); return 1; }
        solver.add_obstacle(skin);
        threw = false;
        try { solver.bind_obstacle(skin, std::vector<int>(3, 0)); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("bind_obstacle took a wrong node count\n"); return 1; }
        solver.bind_obstacle(skin, block_nodes);            // vertex i of the skin is block node i
        solver.exempt_from_obstacle(skin, block_nodes);     // the body's own nodes (none of them is a collision node here)
        solver.set_collisions(cloth_nodes);
        admm::Solver::Settings st;
        st.admm_iters = 30;
        st.verbose = 0;
        st.acceleration_type = admm::Solver::Settings::ANDERSON;
        st.Anderson_m = 6;
        if (!solver.initialize(st)) { std::printf("initialize failed: %s\n", aa_last_error()); return 1; }
        for (int k = 1; k <= 8; ++k) solver.step();
        int refits = -1, skipped = -1, cause = -1;
        solver.obstacle_status(skin, refits, skipped, cause);
        double tmin = 1e300, tmax = -1e300;
        for (int i : top) { tmin = std::fmin(tmin, solver.m_x[3 * i + 1]); tmax = std::fmax(tmax, solver.m_x[3 * i + 1]); }
        const int mid = nb + corner(n / 2, n / 2);
        std::printf("%.17g %.17g %.17g %d %d\n", tmin, tmax, solver.m_x[3 * mid + 1], refits, skipped);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
