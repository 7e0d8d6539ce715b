// Host construction of the bending hinges of a triangle list (aa_elastic_add_bending). Host only,
// no HIP: builds with a plain compiler (tests/cpp/bending.cpp).
//
// One hinge per interior edge, i.e. an edge shared by exactly two triangles; a boundary edge makes
// none. Its vertices (x0, x1, x2, x3): x0 < x1 the edge's endpoints, x2 the opposite vertex in the
// triangle with the lower index, x3 the one in the other. With the rest-shape cotangents
//   cot(p; a, b) = ((a - p) . (b - p)) / |(a - p) x (b - p)|
//   a0 = cot(x0; x1, x2), a1 = cot(x1; x0, x2), b0 = cot(x0; x1, x3), b1 = cot(x1; x0, x3)
// the reduction row is K = (a1 + b1, a0 + b0, -(a0 + a1), -(b0 + b1)) (entries sum to zero), the
// reduction D_e = K (x) I3, so z_e = K x in R^3 -- the row of the quadratic isometric bending model
// (Bergou, Wardetzky, Harmon, Zorin, Grinspun, "A quadratic bending model for inextensible
// surfaces", SGP 2006). Energy U(z) = 1/2 kappa (|z| - r)^2 with kappa = 3 k_bend / (A_lo + A_hi)
// of the two rest areas; r = 0 with flat_rest, else |K xbar| of the rest positions, so that a
// curved rest shape is an equilibrium. Hinges come in increasing (x0, x1).
#pragma once
#include <array>
#include <cmath>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "error.hpp"

namespace aa {

struct HingeSet {
    std::vector<int> idx;        // [count][4] indices into the caller's vertex array
    std::vector<double> K;       // [count][4]
    std::vector<double> kappa;   // [count]
    std::vector<double> r;       // [count] rest length of z (0 with flat_rest)
    int count() const { return (int)kappa.size(); }
};

namespace bend_detail {
inline void sub3(const double* a, const double* b, double* r) { r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; }
inline void cross3(const double* u, const double* w, double* r) {
    r[0] = u[1] * w[2] - u[2] * w[1]; r[1] = u[2] * w[0] - u[0] * w[2]; r[2] = u[0] * w[1] - u[1] * w[0];
}
inline double dot3(const double* u, const double* w) { return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]; }
inline double norm3(const double* u) { return std::sqrt(dot3(u, u)); }
inline double cot(const double* p, const double* a, const double* b) {
    double u[3], w[3], n[3];
    sub3(a, p, u); sub3(b, p, w); cross3(u, w, n);
    return dot3(u, w) / norm3(n);
}
}  // namespace bend_detail

// V: [n_verts][3] rest positions, F: [n_tris][3]. Throws Error naming the first offending element:
// ERR_ARG for an index out of range, a non-finite vertex, k_bend not finite or not > 0, an edge in
// more than two triangles, two triangles running along their shared edge in the same direction;
// ERR_NUMERIC for a zero-area triangle.
inline HingeSet build_hinges(const double* V, int n_verts, const int* F, int n_tris, double k_bend, bool flat_rest) {
    using namespace bend_detail;
    const std::string who = "add_bending: ";
    if (n_tris < 0 || (n_tris > 0 && (!V || !F))) throw Error(ERR_ARG, who + "bad input");
    for (int t = 0; t < n_tris; ++t)
        for (int a = 0; a < 3; ++a)
            if (F[3 * (size_t)t + a] < 0 || F[3 * (size_t)t + a] >= n_verts)
                throw Error(ERR_ARG, who + "triangle " + std::to_string(t) + " has a vertex index out of range");
    for (int t = 0; t < n_tris; ++t)
        for (int a = 0; a < 3; ++a)
            for (int d = 0; d < 3; ++d)
                if (!std::isfinite(V[3 * (size_t)F[3 * (size_t)t + a] + d]))
                    throw Error(ERR_ARG, who + "vertex " + std::to_string(F[3 * (size_t)t + a]) + " (triangle " + std::to_string(t) + ") has a non-finite coordinate");
    if (!std::isfinite(k_bend) || !(k_bend > 0.0)) throw Error(ERR_ARG, who + "k_bend must be finite and > 0");
    std::vector<double> area(n_tris);
    for (int t = 0; t < n_tris; ++t) {
        const double *A = V + 3 * (size_t)F[3 * (size_t)t], *B = V + 3 * (size_t)F[3 * (size_t)t + 1],
                     *C = V + 3 * (size_t)F[3 * (size_t)t + 2];
        double u[3], w[3], n[3];
        sub3(B, A, u); sub3(C, A, w); cross3(u, w, n);
        area[t] = 0.5 * norm3(n);
        if (!(area[t] > 0.0)) throw Error(ERR_NUMERIC, who + "triangle " + std::to_string(t) + " has zero area");
    }
    // edge map: per undirected edge (lower index first) its triangles in increasing index, each
    // with its opposite vertex and whether it runs the edge from the lower to the higher index
    struct Edge { int n = 0; int tri[2], opp[2]; bool fwd[2]; };
    std::map<std::pair<int, int>, Edge> edges;
    for (int t = 0; t < n_tris; ++t)
        for (int a = 0; a < 3; ++a) {
            const int p = F[3 * (size_t)t + a], q = F[3 * (size_t)t + (a + 1) % 3], o = F[3 * (size_t)t + (a + 2) % 3];
            const std::string e = "edge (" + std::to_string(p < q ? p : q) + ", " + std::to_string(p < q ? q : p) + ") of triangle " + std::to_string(t);
            if (p == q) throw Error(ERR_NUMERIC, who + "triangle " + std::to_string(t) + " has zero area");
            Edge& E = edges[{p < q ? p : q, p < q ? q : p}];
            if (E.n == 2) throw Error(ERR_ARG, who + e + " lies in more than two triangles: the list is not edge-manifold");
            if (E.n == 1 && E.fwd[0] == (p < q))
                throw Error(ERR_ARG, who + e + " is run in the same direction by triangle " + std::to_string(E.tri[0]) + ": inconsistent orientation");
            E.tri[E.n] = t; E.opp[E.n] = o; E.fwd[E.n] = p < q;
            ++E.n;
        }
    HingeSet H;
    for (auto& kv : edges) {
        const Edge& E = kv.second;
        if (E.n != 2) continue;   // boundary
        const int id[4] = {kv.first.first, kv.first.second, E.opp[0], E.opp[1]};
        const double* x[4];
        for (int a = 0; a < 4; ++a) x[a] = V + 3 * (size_t)id[a];
        const double a0 = cot(x[0], x[1], x[2]), a1 = cot(x[1], x[0], x[2]);
        const double b0 = cot(x[0], x[1], x[3]), b1 = cot(x[1], x[0], x[3]);
        const double K[4] = {a1 + b1, a0 + b0, -(a0 + a1), -(b0 + b1)};
        double r = 0.0;
        if (!flat_rest) {
            double z[3];
            for (int d = 0; d < 3; ++d) z[d] = ((K[0] * x[0][d] + K[1] * x[1][d]) + K[2] * x[2][d]) + K[3] * x[3][d];
            r = norm3(z);
        }
        for (int a = 0; a < 4; ++a) { H.idx.push_back(id[a]); H.K.push_back(K[a]); }
        H.kappa.push_back(3.0 * k_bend / (area[E.tri[0]] + area[E.tri[1]]));
        H.r.push_back(r);
    }
    return H;
}

}  // namespace aa
