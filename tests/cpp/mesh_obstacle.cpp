// Host preparation of the triangle-mesh obstacle (csrc/mesh_obstacle.hpp), no GPU:
//   * validation accepts the closed test meshes given in argv[1] (tests/mesh_obs_cases.py writes
//     them: per mesh "name nv nf", nv vertex rows, nf triangle rows; the cube comes first) and
//     refuses, with ERR_ARG naming the element, each of them with one face removed, one face
//     flipped, all faces flipped, a zero-area face, an index out of range, a non-finite vertex;
//   * the tables are in the BVH's leaf order (tris[k] = the corners of triangle orig[k]);
//   * on the cube the pseudonormals are, up to scale, the diagonal at the 8 vertices, the sum of
//     the two face normals on the 12 cube edges and the face normal on the 6 face diagonals.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "mesh_obstacle.hpp"

namespace {
int fails = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) { std::printf("FAIL %s\n", what.c_str()); ++fails; }
}
// validation must throw ERR_ARG with a message containing `needle`
void refused(const std::vector<double>& V, const std::vector<int>& F, const std::string& needle, const std::string& what) {
    try {
        aa::validate_mesh_obstacle(V.data(), (int)V.size() / 3, F.data(), (int)F.size() / 3);
        expect(false, what + ": accepted");
    } catch (const aa::Error& e) {
        expect(e.code == aa::ERR_ARG, what + ": not ERR_ARG");
        expect(std::string(e.what()).find(needle) != std::string::npos, what + ": message '" + e.what() + "' lacks '" + needle + "'");
    }
}
bool parallel(const double* a, const double* b) {   // same direction, up to scale
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double la = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), lb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    return std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) <= 1e-14 * la * lb && a[0] * b[0] + a[1] * b[1] + a[2] * b[2] > 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: mesh_obstacle meshes.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string name;
    int nv, nf, n_meshes = 0;
    while (in >> name >> nv >> nf) {
        std::vector<double> V(3 * (size_t)nv);
        std::vector<int> F(3 * (size_t)nf);
        for (auto& v : V) in >> v;
        for (auto& f : F) in >> f;
        ++n_meshes;
        aa::MeshObstacleHost M;
        try {
            M = aa::prepare_mesh_obstacle(V.data(), nv, F.data(), nf);
        } catch (const aa::Error& e) {
            expect(false, name + ": refused: " + e.what());
            continue;
        }
        // leaf order
        expect((int)M.tris.size() == nf && (int)M.orig.size() == nf && (int)M.pn.size() == aa::kPnStride * nf, name + ": table sizes");
        std::set<int> seen(M.orig.begin(), M.orig.end());
        expect((int)seen.size() == nf, name + ": orig is a permutation");
        for (int k = 0; k < nf; ++k)
            for (int a = 0; a < 3; ++a)
                for (int d = 0; d < 3; ++d)
                    expect(M.tris[k].v[3 * a + d] == V[3 * (size_t)F[3 * (size_t)M.orig[k] + a] + d], name + ": leaf order of tris");
        for (int d = 0; d < 3; ++d) {
            double lo = 1e300, hi = -1e300;
            for (int i = 0; i < nv; ++i) { lo = std::min(lo, V[3 * (size_t)i + d]); hi = std::max(hi, V[3 * (size_t)i + d]); }
            expect(M.lo[d] == lo && M.hi[d] == hi, name + ": root box");
        }
        if (nf <= 4) expect(M.nodes.size() == 1, name + ": single-leaf BVH");

        // refusals
        {
            std::vector<int> G(F.begin() + 3, F.end());
            refused(V, G, "edge (", name + " with face 0 removed");
            refused(V, G, "open", name + " with face 0 removed");
        }
        {
            std::vector<int> G = F;
            std::swap(G[3 * 1 + 1], G[3 * 1 + 2]);
            refused(V, G, "edge (", name + " with face 1 flipped");
            refused(V, G, "orientation", name + " with face 1 flipped");
        }
        {
            std::vector<int> G = F;
            for (int t = 0; t < nf; ++t) std::swap(G[3 * t + 1], G[3 * t + 2]);
            refused(V, G, "signed volume", name + " with all faces flipped");
        }
        {
            std::vector<int> G = F;
            G[3 * 2 + 2] = G[3 * 2 + 1];
            refused(V, G, "triangle 2 has zero area", name + " with a zero-area face");
        }
        {
            std::vector<int> G = F;
            G[3 * 3] = nv;
            refused(V, G, "triangle 3 has a vertex index out of range", name + " with an index out of range");
            G[3 * 3] = -1;
            refused(V, G, "triangle 3 has a vertex index out of range", name + " with a negative index");
        }
        {
            std::vector<double> W = V;
            W[3 * 1 + 2] = std::numeric_limits<double>::quiet_NaN();
            refused(W, F, "vertex 1 has a non-finite coordinate", name + " with a NaN coordinate");
        }

        if (n_meshes == 1) {   // the unit cube
            expect(name == "cube" && nv == 8 && nf == 12, "the cube comes first");
            std::set<std::pair<int, int>> cube_edges, diagonals;
            static const int corner_slot[3] = {0, 1, 3}, edge_slot[3] = {2, 5, 4};   // a b c; ab bc ca
            for (int k = 0; k < nf; ++k) {
                const int t = M.orig[k];
                const double* P = M.pn.data() + (size_t)aa::kPnStride * k;
                const double* fn = P + 3 * 6;
                expect(std::fabs(fn[0] * fn[0] + fn[1] * fn[1] + fn[2] * fn[2] - 1.0) < 1e-15, "cube: unit face normal");
                int axis = -1;
                for (int d = 0; d < 3; ++d) if (std::fabs(fn[d]) > 0.5) axis = d;
                for (int a = 0; a < 3; ++a) {
                    const int p = F[3 * t + a], q = F[3 * t + (a + 1) % 3];
                    const double* vp = V.data() + 3 * (size_t)p;
                    const double* vq = V.data() + 3 * (size_t)q;
                    const double diag[3] = {2 * vp[0] - 1, 2 * vp[1] - 1, 2 * vp[2] - 1};
                    expect(parallel(P + 3 * corner_slot[a], diag), "cube: vertex pseudonormal is the diagonal");
                    int differ = 0;
                    for (int d = 0; d < 3; ++d) differ += vp[d] != vq[d];
                    const double* en = P + 3 * edge_slot[a];
                    if (differ == 1) {   // a cube edge: the sum of the two face normals = the mid-point's direction from the centre
                        const double want[3] = {vp[0] + vq[0] - 1, vp[1] + vq[1] - 1, vp[2] + vq[2] - 1};
                        expect(parallel(en, want), "cube: edge pseudonormal is the sum of the two face normals");
                        expect(std::fabs(en[0] * en[0] + en[1] * en[1] + en[2] * en[2] - 2.0) < 1e-14, "cube: edge pseudonormal is unnormalised");
                        cube_edges.insert({std::min(p, q), std::max(p, q)});
                    } else {             // a face diagonal: two coplanar faces
                        expect(differ == 2, "cube: diagonal");
                        expect(parallel(en, fn) && axis >= 0, "cube: diagonal pseudonormal is the face normal");
                        diagonals.insert({std::min(p, q), std::max(p, q)});
                    }
                }
            }
            expect(cube_edges.size() == 12 && diagonals.size() == 6, "cube: 12 edges and 6 diagonals");
        }
    }
    expect(n_meshes == 4, "four meshes read");
    if (fails) return 1;
    std::printf("ok %d meshes\n", n_meshes);
    return 0;
}
