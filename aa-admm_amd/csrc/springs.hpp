// Host construction of two-node springs (aa_elastic_add_springs). Host only, no HIP: builds with a
// plain compiler (tests/cpp/springs.cpp).
//
// A spring joins nodes a != b. Its reduction row is (-1, +1), so z = x_b - x_a in R^3: two
// vertices, one column. Rest length L >= 0 and stiffness k > 0 per spring; ADMM weight sqrt(k).
// The mode is one per call: AA_SPRING (0) U = 1/2 k (|z| - L)^2, AA_SPRING_TETHER (1) U = 1/2 k
// max(0, |z| - L)^2 (slack below L), AA_SPRING_STRUT (2) U = 1/2 k max(0, L - |z|)^2 (slack above
// L); | AA_SPRING_HARD (4) makes U the indicator of |z| = L / <= L / >= L and leaves k the weight
// alone. The prox is dev::spring_prox (device_prox.hpp). rest == NULL: L = |verts3[b] - verts3[a]|.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "error.hpp"

namespace aa {

constexpr int kSpringTether = 1, kSpringStrut = 2, kSpringHard = 4;   // AA_SPRING_* of aa_admm.h

struct SpringSet {
    std::vector<int> idx;      // [count][2] indices into the caller's vertex array: (a, b)
    std::vector<double> G;     // [count][2] = (-1, +1)
    std::vector<double> L;     // [count] rest length
    std::vector<double> w;     // [count] sqrt(k)
    int count() const { return (int)L.size(); }
};

inline bool spring_mode_ok(int mode) { return mode >= 0 && mode <= 6 && (mode & 3) != 3; }

// V: [n_verts][3] (may be null when rest is given), pairs: [n][2] indices < n_verts. Throws
// Error(ERR_ARG) naming the first offending spring; builds nothing in that case.
inline SpringSet build_springs(const double* V, int n_verts, const int* pairs, int n, int mode, const double* k,
                               const double* rest) {
    const std::string who = "add_springs: ";
    if (!spring_mode_ok(mode)) throw Error(ERR_ARG, who + "unknown mode " + std::to_string(mode));
    if (n < 0) throw Error(ERR_ARG, who + "n_springs < 0");
    if (n > 0 && (!pairs || !k)) throw Error(ERR_ARG, who + "null pairs or k with n_springs > 0");
    if (n > 0 && !rest && !V) throw Error(ERR_ARG, who + "rest == NULL needs verts3 for the rest lengths");
    SpringSet S;
    S.idx.reserve(2 * (size_t)n); S.G.reserve(2 * (size_t)n); S.L.reserve(n); S.w.reserve(n);
    for (int e = 0; e < n; ++e) {
        const std::string sp = who + "spring " + std::to_string(e);
        const int a = pairs[2 * (size_t)e], b = pairs[2 * (size_t)e + 1];
        if (a < 0 || a >= n_verts || b < 0 || b >= n_verts) throw Error(ERR_ARG, sp + " has a node index out of range");
        if (a == b) throw Error(ERR_ARG, sp + " joins node " + std::to_string(a) + " to itself");
        if (!std::isfinite(k[e]) || !(k[e] > 0.0)) throw Error(ERR_ARG, sp + ": k must be finite and > 0");
        double L;
        if (rest) {
            L = rest[e];
            if (!std::isfinite(L) || L < 0.0) throw Error(ERR_ARG, sp + ": rest must be finite and >= 0");
        } else {
            const double *A = V + 3 * (size_t)a, *B = V + 3 * (size_t)b;
            const double d0 = B[0] - A[0], d1 = B[1] - A[1], d2 = B[2] - A[2];
            L = std::sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            if (!std::isfinite(L)) throw Error(ERR_ARG, sp + " has an endpoint with a non-finite coordinate");
        }
        const double w = std::sqrt(k[e]);
        if (!std::isfinite(w) || !(w > 0.0)) throw Error(ERR_ARG, sp + ": k must be finite and > 0");
        S.idx.push_back(a); S.idx.push_back(b);
        S.G.push_back(-1.0); S.G.push_back(1.0);
        S.L.push_back(L);
        S.w.push_back(w);
    }
    return S;
}

}  // namespace aa
