// Host construction of ties (aa_elastic_add_ties). Host only, no HIP: builds with a plain compiler
// (tests/cpp/ties.cpp).
//
// A tie is a spring between two anchors, each a fixed weighted combination of nodes: anchor A =
// sum_i a_i x_{A_i} over na nodes, anchor B = sum_j b_j x_{B_j} over nb nodes, 1 <= na, nb <= 4 and
// 3 <= na + nb <= 6 (a node, a point on an edge, in a triangle, in a tet). Its reduction row is
// (-a_0 .. -a_{na-1}, +b_0 .. +b_{nb-1}) over the vertices (A_0 .. A_{na-1}, B_0 .. B_{nb-1}), so
// z = p_B - p_A in R^3: na + nb vertices, one column. The kernels form z as the sum over the
// vertices in this stored order, left to right from 0, each term one fused multiply-add:
// z = fma(g_{nv-1}, x_{nv-1}, ... fma(g_1, x_1, g_0 x_0)). Rest length L >= 0 and stiffness k > 0 per
// tie; ADMM weight sqrt(k). The mode is one per call and means what it means for a spring
// (springs.hpp); the prox is dev::spring_prox. The weights are used as given: each side must sum to
// 1 within 1e-12 and is not renormalised; weights outside [0, 1] (an extrapolated anchor) and zero
// weights are allowed. rest == NULL: L = |p_B - p_A| at verts3, with each anchor's coordinate summed
// left to right from its first term, p = ((w_0 x_0 + w_1 x_1) + w_2 x_2) + w_3 x_3, d = p_B - p_A
// and L = sqrt((d0 d0 + d1 d1) + d2 d2), nothing contracted.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "error.hpp"
#include "springs.hpp"

namespace aa {

struct TieSet {
    int nv = 0;                // na + nb
    std::vector<int> idx;      // [count][nv] indices into the caller's vertex array: A's nodes, then B's
    std::vector<double> G;     // [count][nv] = (-a, +b)
    std::vector<double> L;     // [count] rest length
    std::vector<double> w;     // [count] sqrt(k)
    int count() const { return (int)L.size(); }
};

// V: [n_verts][3] (may be null when rest is given); nodes_a / w_a: [n][na], nodes_b / w_b: [n][nb],
// indices < n_verts. Throws Error(ERR_ARG) naming the first offending tie; builds nothing then.
inline TieSet build_ties(const double* V, int n_verts, int na, const int* nodes_a, const double* w_a, int nb,
                         const int* nodes_b, const double* w_b, int n, int mode, const double* k, const double* rest) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const std::string who = "add_ties: ";
    if (!spring_mode_ok(mode)) throw Error(ERR_ARG, who + "unknown mode " + std::to_string(mode));
    if (na < 1 || nb < 1 || na > 4 || nb > 4)
        throw Error(ERR_ARG, who + "na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ": an anchor has 1 to 4 nodes");
    if (na + nb == 2) throw Error(ERR_ARG, who + "na = nb = 1 is a two-node spring: use aa_elastic_add_springs");
    if (na + nb > 6)
        throw Error(ERR_ARG, who + "na + nb = " + std::to_string(na + nb) + ": ties of 7 or 8 nodes (triangle-tet, tet-tet) are not provided");
    if (n < 0) throw Error(ERR_ARG, who + "n_ties < 0");
    if (n > 0 && (!nodes_a || !w_a || !nodes_b || !w_b || !k)) throw Error(ERR_ARG, who + "null nodes, weights or k with n_ties > 0");
    if (n > 0 && !rest && !V) throw Error(ERR_ARG, who + "rest == NULL needs verts3 for the rest lengths");
    const int nv = na + nb;
    TieSet S;
    S.nv = nv;
    S.idx.reserve((size_t)nv * n); S.G.reserve((size_t)nv * n); S.L.reserve(n); S.w.reserve(n);
    for (int e = 0; e < n; ++e) {
        const std::string tp = who + "tie " + std::to_string(e);
        int id[8];
        double g[8];
        for (int i = 0; i < na; ++i) { id[i] = nodes_a[(size_t)na * e + i]; g[i] = w_a[(size_t)na * e + i]; }
        for (int j = 0; j < nb; ++j) { id[na + j] = nodes_b[(size_t)nb * e + j]; g[na + j] = w_b[(size_t)nb * e + j]; }
        for (int i = 0; i < nv; ++i)
            if (id[i] < 0 || id[i] >= n_verts) throw Error(ERR_ARG, tp + " has a node index out of range");
        for (int i = 0; i < nv; ++i)
            for (int j = i + 1; j < nv; ++j)
                if (id[i] == id[j]) throw Error(ERR_ARG, tp + " has node " + std::to_string(id[i]) + " twice");
        for (int i = 0; i < nv; ++i)
            if (!std::isfinite(g[i])) throw Error(ERR_ARG, tp + " has a non-finite weight");
        double sa = 0.0, sb = 0.0;
        for (int i = 0; i < na; ++i) sa += g[i];
        for (int j = 0; j < nb; ++j) sb += g[na + j];
        if (!(std::fabs(sa - 1.0) <= 1e-12)) throw Error(ERR_ARG, tp + ": the weights of anchor A do not sum to 1 within 1e-12");
        if (!(std::fabs(sb - 1.0) <= 1e-12)) throw Error(ERR_ARG, tp + ": the weights of anchor B do not sum to 1 within 1e-12");
        if (!std::isfinite(k[e]) || !(k[e] > 0.0)) throw Error(ERR_ARG, tp + ": k must be finite and > 0");
        double L;
        if (rest) {
            L = rest[e];
            if (!std::isfinite(L) || L < 0.0) throw Error(ERR_ARG, tp + ": rest must be finite and >= 0");
        } else {
            double d[3];
            for (int c = 0; c < 3; ++c) {
                double pa = g[0] * V[3 * (size_t)id[0] + c], pb = g[na] * V[3 * (size_t)id[na] + c];
                for (int i = 1; i < na; ++i) pa = pa + g[i] * V[3 * (size_t)id[i] + c];
                for (int j = 1; j < nb; ++j) pb = pb + g[na + j] * V[3 * (size_t)id[na + j] + c];
                d[c] = pb - pa;
            }
            L = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            if (!std::isfinite(L)) throw Error(ERR_ARG, tp + " has a node with a non-finite coordinate");
        }
        const double w = std::sqrt(k[e]);
        if (!std::isfinite(w) || !(w > 0.0)) throw Error(ERR_ARG, tp + ": k must be finite and > 0");
        for (int i = 0; i < nv; ++i) { S.idx.push_back(id[i]); S.G.push_back(i < na ? -g[i] : g[i]); }
        S.L.push_back(L);
        S.w.push_back(w);
    }
    return S;
}

}  // namespace aa
