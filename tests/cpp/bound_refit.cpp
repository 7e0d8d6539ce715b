// Host restatement of the bound-obstacle refit (csrc/mesh_obstacle.hpp: gather_bound_vertices,
// check_bound_refit, bound_refit_host), no GPU. argv[1] (tests/test_bound_obstacle.py writes it)
// holds per case "name nv nf nx", nv vertex rows V, nf triangle rows, nx node rows X, nv node
// indices and the expected vol6 of X[nodes] as a hexadecimal double. Checked on every case:
//   * the tables after the bound refit equal refit_mesh_obstacle_host on X[nodes] bit for bit, the
//     root box is the exact range of X[nodes], the cause is 0;
//   * vol6 has the bits of the given value (a numpy restatement of the stated chunked sum);
//   * a NaN in a bound node, a vertex collapsed onto its neighbour and X = -X are causes 1, 2 and 3
//     and leave the built tables untouched; a NaN in a node the mesh does not name changes nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0;
}
bool same_tables(const aa::MeshObstacleHost& a, const aa::MeshObstacleHost& b) {
    return same_bytes(a.nodes, b.nodes) && same_bytes(a.tris, b.tris) && same_bytes(a.pn, b.pn) && a.orig == b.orig &&
           !std::memcmp(a.lo, b.lo, sizeof(a.lo)) && !std::memcmp(a.hi, b.hi, sizeof(a.hi));
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: bound_refit cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string name, hex;
    int nv, nf, nx, n_cases = 0;
    while (in >> name >> nv >> nf >> nx) {
        std::vector<double> V(3 * (size_t)nv), X(3 * (size_t)nx);
        std::vector<int> F(3 * (size_t)nf), nodes(nv);
        for (auto& v : V) in >> v;
        for (auto& f : F) in >> f;
        for (auto& v : X) in >> v;
        for (auto& i : nodes) in >> i;
        in >> hex;
        const double want_vol6 = std::strtod(hex.c_str(), nullptr);
        ++n_cases;
        expect(nx >= nv + 30, name + ": at least 30 decoy nodes");
        const aa::MeshObstacleHost M0 = aa::prepare_mesh_obstacle(V.data(), nv, F.data(), nf);
        const aa::MeshRefitTables T = aa::make_refit_tables(M0, nv, F.data(), nf);

        std::vector<double> W(3 * (size_t)nv);   // X[nodes], gathered here independently
        for (int i = 0; i < nv; ++i)
            for (int d = 0; d < 3; ++d) W[3 * (size_t)i + d] = X[3 * (size_t)nodes[i] + d];
        aa::MeshObstacleHost want = M0;
        double lo[3], hi[3];
        aa::validate_mesh_refit(T, W.data(), "refit: ", lo, hi);
        aa::refit_mesh_obstacle_host(want, T, W.data());

        aa::MeshObstacleHost M = M0;
        double vol6 = -1;
        const int cause = aa::bound_refit_host(M, T, X.data(), nodes.data(), &vol6);
        expect(cause == aa::BOUND_OK, name + ": cause " + std::to_string(cause));
        expect(same_tables(M, want), name + ": tables differ from refit_mesh_obstacle_host on X[nodes]");
        for (int d = 0; d < 3; ++d) expect(M.lo[d] == lo[d] && M.hi[d] == hi[d], name + ": root box");
        expect(!std::memcmp(&vol6, &want_vol6, sizeof(double)), name + ": vol6 bits differ from the restated chunked sum");

        {   // a decoy holding NaN is not looked at
            std::vector<char> named(nx, 0);
            for (int i : nodes) named[i] = 1;
            std::vector<double> Y = X;
            for (int i = 0; i < nx; ++i)
                if (!named[i]) Y[3 * (size_t)i + 1] = std::numeric_limits<double>::quiet_NaN();
            aa::MeshObstacleHost M2 = M0;
            double v2 = -1;
            expect(aa::bound_refit_host(M2, T, Y.data(), nodes.data(), &v2) == aa::BOUND_OK && same_tables(M2, want) &&
                       !std::memcmp(&v2, &vol6, sizeof(double)), name + ": a NaN decoy changed the result");
        }
        auto refused = [&](const std::vector<double>& Y, int want_cause, const std::string& what) {
            aa::MeshObstacleHost M2 = M0;
            double v2 = 0;
            const int c = aa::bound_refit_host(M2, T, Y.data(), nodes.data(), &v2);
            expect(c == want_cause, name + " " + what + ": cause " + std::to_string(c));
            expect(same_tables(M2, M0), name + " " + what + ": the built tables changed");
        };
        {
            std::vector<double> Y = X;
            Y[3 * (size_t)nodes[1] + 2] = std::numeric_limits<double>::quiet_NaN();
            refused(Y, aa::BOUND_NONFINITE, "with a NaN in a bound node");
        }
        {
            std::vector<double> Y = X;   // the second corner of triangle 2 collapsed onto its first
            for (int d = 0; d < 3; ++d) Y[3 * (size_t)nodes[F[3 * 2 + 1]] + d] = Y[3 * (size_t)nodes[F[3 * 2]] + d];
            refused(Y, aa::BOUND_ZERO_AREA, "with a collapsed vertex");
        }
        {
            std::vector<double> Y = X;
            for (auto& v : Y) v = -v;
            refused(Y, aa::BOUND_VOLUME, "turned inside out");
        }
        {   // the lowest-numbered cause wins: inside out and a NaN
            std::vector<double> Y = X;
            for (auto& v : Y) v = -v;
            Y[3 * (size_t)nodes[0]] = std::numeric_limits<double>::infinity();
            refused(Y, aa::BOUND_NONFINITE, "inside out with an infinite coordinate");
        }
    }
    if (fails) return 1;
    std::printf("ok %d cases\n", n_cases);
    return 0;
}
