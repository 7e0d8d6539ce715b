// Host restatement of the deforming-obstacle refit (csrc/mesh_obstacle.hpp:
// refit_mesh_obstacle_host), no GPU. argv[1] (tests/test_deforming_obstacle.py writes it) holds per
// case "name nv nf", nv vertex rows V, nf triangle rows, nv rows of the deformed vertices V' and nf
// rows of 21 doubles: the pseudonormals of tests/mesh_obs_cases.py on V' per caller triangle in
// the table's feature order (a, b, ab, c, ca, bc, face). Checked on every case:
//   * the refit to V itself reproduces the built node, triangle and pseudonormal tables and the
//     root box bit for bit;
//   * after the refit to V' the leaf triangles hold V', every vertex of a node's triangles lies
//     inside that node's box and its three axis ranges, the axes, `a` and `sn` are untouched, and
//     the root box is the exact range of V';
//   * pn matches the given pseudonormals to 1e-13;
//   * a null array, a NaN vertex, a vertex collapsed onto its neighbour and V' = -V are refused
//     with ERR_ARG naming the cause, before anything changes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "mesh_obstacle.hpp"

namespace {
int fails = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) { std::printf("FAIL %s\n", what.c_str()); ++fails; }
}
void refused(const aa::MeshRefitTables& T, const double* W, const std::string& needle, const std::string& what) {
    double lo[3], hi[3];
    try {
        aa::validate_mesh_refit(T, W, "refit: ", lo, hi);
        expect(false, what + ": accepted");
    } catch (const aa::Error& e) {
        expect(e.code == aa::ERR_ARG, what + ": not ERR_ARG");
        expect(std::string(e.what()).find(needle) != std::string::npos, what + ": message '" + e.what() + "' lacks '" + needle + "'");
    }
}
template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: mesh_refit cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string name;
    int nv, nf, n_cases = 0, n_big = 0;
    double worst_pn = 0;
    while (in >> name >> nv >> nf) {
        std::vector<double> V(3 * (size_t)nv), W(3 * (size_t)nv), PN((size_t)aa::kPnStride * nf);
        std::vector<int> F(3 * (size_t)nf);
        for (auto& v : V) in >> v;
        for (auto& f : F) in >> f;
        for (auto& v : W) in >> v;
        for (auto& v : PN) in >> v;
        ++n_cases;
        const aa::MeshObstacleHost M0 = aa::prepare_mesh_obstacle(V.data(), nv, F.data(), nf);
        const aa::MeshRefitTables T = aa::make_refit_tables(M0, nv, F.data(), nf);
        n_big += (int)T.big_node.size();
        const int nn = (int)M0.nodes.size();
        expect(T.node_beg[0] == 0 && T.node_cnt[0] == nf, name + ": the root's range is every triangle");

        double lo[3], hi[3];
        {   // identity
            aa::MeshObstacleHost M = M0;
            aa::validate_mesh_refit(T, V.data(), "refit: ", lo, hi);
            aa::refit_mesh_obstacle_host(M, T, V.data());
            expect(same_bytes(M.nodes, M0.nodes), name + ": identity refit changes the nodes");
            expect(same_bytes(M.tris, M0.tris), name + ": identity refit changes the triangles");
            expect(same_bytes(M.pn, M0.pn), name + ": identity refit changes the pseudonormals");
            for (int d = 0; d < 3; ++d)
                expect(M.lo[d] == M0.lo[d] && M.hi[d] == M0.hi[d] && lo[d] == M0.lo[d] && hi[d] == M0.hi[d], name + ": identity refit changes the root box");
        }

        aa::MeshObstacleHost M = M0;
        try {
            aa::validate_mesh_refit(T, W.data(), "refit: ", lo, hi);
        } catch (const aa::Error& e) {
            expect(false, name + ": refused: " + e.what());
            continue;
        }
        aa::refit_mesh_obstacle_host(M, T, W.data());
        for (int k = 0; k < nf; ++k)
            for (int a = 0; a < 3; ++a)
                for (int d = 0; d < 3; ++d)
                    expect(M.tris[k].v[3 * a + d] == W[3 * (size_t)F[3 * (size_t)M.orig[k] + a] + d], name + ": leaf triangles hold V'");
        for (int d = 0; d < 3; ++d) {
            double l = 1e300, h = -1e300;
            for (int i = 0; i < nv; ++i) { l = std::min(l, W[3 * (size_t)i + d]); h = std::max(h, W[3 * (size_t)i + d]); }
            expect(M.lo[d] == l && M.hi[d] == h && lo[d] == l && hi[d] == h, name + ": root box of V'");
        }
        for (int i = 0; i < nn; ++i) {
            const aa::BvhNode &nd = M.nodes[i], &n0 = M0.nodes[i];
            expect(nd.a == n0.a && nd.sn == n0.sn && !std::memcmp(nd.nrm, n0.nrm, 12) && !std::memcmp(nd.t1, n0.t1, 12) && !std::memcmp(nd.t2, n0.t2, 12),
                   name + ": the refit touched a, sn or an axis");
            const float* ax[3] = {nd.nrm, nd.t1, nd.t2};
            const float rl[3] = {nd.dlo, nd.t1lo, nd.t2lo}, rh[3] = {nd.dhi, nd.t1hi, nd.t2hi};
            const float r0l[3] = {n0.dlo, n0.t1lo, n0.t2lo}, r0h[3] = {n0.dhi, n0.t1hi, n0.t2hi};
            for (int x = 0; x < 3; ++x)
                if (r0l[x] == -FLT_MAX && r0h[x] == FLT_MAX) expect(rl[x] == -FLT_MAX && rh[x] == FLT_MAX, name + ": an unbounded range got bounds");
            bool inside = true, tight = true;
            double mn[6], mx[6];
            for (int c = 0; c < 6; ++c) { mn[c] = 1e300; mx[c] = -1e300; }
            for (int k = T.node_beg[i]; k < T.node_beg[i] + T.node_cnt[i]; ++k)
                for (int a = 0; a < 3; ++a) {
                    const double* P = M.tris[k].v + 3 * a;
                    for (int d = 0; d < 3; ++d) {
                        inside = inside && (double)nd.lo[d] <= P[d] && P[d] <= (double)nd.hi[d];
                        mn[d] = std::min(mn[d], P[d]); mx[d] = std::max(mx[d], P[d]);
                    }
                    for (int x = 0; x < 3; ++x) {
                        const double s = ((double)ax[x][0] * P[0] + (double)ax[x][1] * P[1]) + (double)ax[x][2] * P[2];
                        inside = inside && (double)rl[x] <= s && s <= (double)rh[x];
                        mn[3 + x] = std::min(mn[3 + x], s); mx[3 + x] = std::max(mx[3 + x], s);
                    }
                }
            expect(inside, name + ": node " + std::to_string(i) + " does not bound its vertices");
            // ... and no looser than one fp32 step
            for (int d = 0; d < 3; ++d)
                tight = tight && std::nextafterf(nd.lo[d], INFINITY) > mn[d] && std::nextafterf(nd.hi[d], -INFINITY) < mx[d];
            for (int x = 0; x < 3; ++x)
                if (rl[x] != -FLT_MAX || rh[x] != FLT_MAX)
                    tight = tight && std::nextafterf(rl[x], INFINITY) > mn[3 + x] && std::nextafterf(rh[x], -INFINITY) < mx[3 + x];
            expect(tight, name + ": node " + std::to_string(i) + " is looser than outward rounding");
        }
        for (int k = 0; k < nf; ++k)
            for (int c = 0; c < aa::kPnStride; ++c)
                worst_pn = std::max(worst_pn, std::fabs(M.pn[(size_t)aa::kPnStride * k + c] - PN[(size_t)aa::kPnStride * M.orig[k] + c]));

        // refusals; M0's tables are what a refused call leaves
        refused(T, nullptr, "null", name + " with a null array");
        {
            std::vector<double> X = W;
            X[3 * 1 + 2] = std::numeric_limits<double>::quiet_NaN();
            refused(T, X.data(), "vertex 1 has a non-finite coordinate", name + " with a NaN coordinate");
        }
        {
            std::vector<double> X = W;   // the second corner of triangle 2 collapsed onto its first
            for (int d = 0; d < 3; ++d) X[3 * (size_t)F[3 * 2 + 1] + d] = X[3 * (size_t)F[3 * 2] + d];
            refused(T, X.data(), "has zero area", name + " with a collapsed vertex");
        }
        {
            std::vector<double> X = W;
            for (auto& v : X) v = -v;
            refused(T, X.data(), "signed volume", name + " turned inside out");
        }
    }
    std::printf("max |pn - expected| %.3e, %d split nodes\n", worst_pn, n_big);
    expect(worst_pn <= 1e-13, "pseudonormals to 1e-13");
    expect(n_big >= 1, "a case with split nodes");
    if (fails) return 1;
    std::printf("ok %d cases\n", n_cases);
    return 0;
}
