// CPU check of the explicit supernode tree (aa::explicit_tree, spd_direct.hpp) that the solver
// test hook aa_test_direct_solve hands to multifrontal_cholesky instead of a dissection.
//
// Block systems as tests/direct_solve_cases.py builds them: dense SPD blocks in postorder, each
// coupled densely to all of its ancestors, so supernode s must come out with exactly its block's
// pivots and a boundary of all its ancestors' pivots:
//  * an arrow (k leaves of p under a root of q): leaves p pivots, nb = q; root nb = 0;
//  * a chain (k leaves -> middle -> root): the middle has children and a boundary.
// Each is factored through the explicit tree; factor_solve_host must satisfy A x = b at the 1e-10
// of part_solve.cpp and bnd must have exactly the intended sizes. A tree that A does not respect
// (two coupled siblings) and malformed arrays must be refused. Last, the degenerate graphs of the
// solver tests (n = 1, a diagonal matrix, an isolated vertex) go through nested_dissection.
//   g++ -O2 -std=c++17 -fopenmp tests/cpp/explicit_tree.cpp aa-admm_amd/csrc/spd_direct.cpp
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <vector>

#include "../../aa-admm_amd/csrc/spd_direct.hpp"

namespace {

struct Blocks {
    std::vector<int> size, parent, beg, end;
    int n = 0;
    std::vector<double> D;   // dense n x n
    std::vector<char> mask;
};

Blocks make_blocks(const std::vector<int>& size, const std::vector<int>& parent, unsigned seed, bool couple_siblings = false) {
    Blocks B;
    B.size = size; B.parent = parent;
    for (int m : size) { B.beg.push_back(B.n); B.n += m; B.end.push_back(B.n); }
    const int n = B.n, nn = (int)size.size();
    B.D.assign((size_t)n * n, 0.0);
    B.mask.assign((size_t)n * n, 0);
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N01;
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    long long ncpl = 0;
    for (int s = 0; s < nn; ++s) for (int a = parent[s]; a >= 0; a = parent[a]) ncpl += (long long)size[s] * size[a];
    const double scale = 0.7 / std::sqrt(2.0 * std::max<long long>(ncpl + (couple_siblings ? 1 : 0), 1));
    for (int s = 0; s < nn; ++s) {
        const int m = size[s], b0 = B.beg[s];
        std::vector<double> G((size_t)m * m);
        for (auto& v : G) v = N01(rng);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                double acc = 0;
                for (int k = 0; k < m; ++k) acc += G[(size_t)i * m + k] * G[(size_t)j * m + k];
                B.D[(size_t)(b0 + i) * n + b0 + j] = acc / m + (i == j ? 1.0 : 0.0);
                B.mask[(size_t)(b0 + i) * n + b0 + j] = 1;
            }
        for (int a = parent[s]; a >= 0; a = parent[a])
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < size[a]; ++j) {
                    const double c = U(rng) * scale;
                    const size_t r = b0 + i, q = B.beg[a] + j;
                    B.D[r * n + q] = B.D[q * n + r] = c;
                    B.mask[r * n + q] = B.mask[q * n + r] = 1;
                }
    }
    if (couple_siblings) {   // first pivots of supernodes 0 and 1 (siblings in every tree used here)
        const size_t r = B.beg[0], q = B.beg[1];
        B.D[r * n + q] = B.D[q * n + r] = scale;
        B.mask[r * n + q] = B.mask[q * n + r] = 1;
    }
    return B;
}

aa::CsrMatrix to_csr(const Blocks& B) {
    aa::CsrMatrix A;
    A.n = B.n;
    A.ptr.assign(B.n + 1, 0);
    for (int i = 0; i < B.n; ++i) {
        for (int j = 0; j < B.n; ++j)
            if (B.mask[(size_t)i * B.n + j]) { A.col.push_back(j); A.val.push_back(B.D[(size_t)i * B.n + j]); }
        A.ptr[i + 1] = (int)A.col.size();
    }
    return A;
}

// |A x - b|_inf / |b|_inf of factor_solve_host
double solve_residual(const aa::CsrMatrix& A, const aa::SupernodalFactor& F, const std::vector<int>& perm, unsigned seed) {
    const int n = A.n;
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N01;
    std::vector<double> b(3 * (size_t)n);
    for (auto& v : b) v = N01(rng);
    std::vector<double> x = b;
    aa::factor_solve_host(F, x);
    (void)perm;   // A is given in the tree's ordering already
    double rmax = 0, bmax = 0;
    for (int q = 0; q < n; ++q)
        for (int c = 0; c < 3; ++c) {
            double s = 0;
            for (int k = A.ptr[q]; k < A.ptr[q + 1]; ++k) s += A.val[k] * x[3 * (size_t)A.col[k] + c];
            rmax = std::max(rmax, std::fabs(s - b[3 * (size_t)q + c]));
            bmax = std::max(bmax, std::fabs(b[3 * (size_t)q + c]));
        }
    return rmax / bmax;
}

int check_blocks(const char* name, const std::vector<int>& size, const std::vector<int>& parent, unsigned seed) {
    const Blocks B = make_blocks(size, parent, seed);
    const aa::CsrMatrix A = to_csr(B);
    const aa::NdTree T = aa::explicit_tree(B.n, B.beg, B.end, parent);
    aa::check_tree_covers(A, T);
    const aa::SupernodalFactor F = aa::multifrontal_cholesky(A, T);
    bool ok = F.n_nodes == (int)size.size();
    for (int s = 0; s < F.n_nodes && ok; ++s) {
        std::vector<int> want;   // all ancestors' pivots, ascending
        for (int a = parent[s]; a >= 0; a = parent[a]) for (int i = B.beg[a]; i < B.end[a]; ++i) want.push_back(i);
        std::sort(want.begin(), want.end());
        ok = ok && F.end[s] - F.beg[s] == size[s] && F.bnd[s] == want;
    }
    const double res = solve_residual(A, F, T.perm, seed + 1);
    ok = ok && res <= 1e-10;
    std::printf("%s: n=%d supernodes=%d |Ax-b|=%.2e %s\n", name, B.n, F.n_nodes, res, ok ? "TREE_OK" : "TREE_FAIL");
    return ok ? 0 : 1;
}

template <class Fn>
int must_throw(const char* name, Fn&& f) {
    bool threw = false;
    try {
        f();
    } catch (const std::runtime_error&) {
        threw = true;
    }
    std::printf("%s: %s\n", name, threw ? "REFUSED_OK" : "REFUSED_FAIL");
    return threw ? 0 : 1;
}

// a graph through nested_dissection (leaf 8), factored and solved
int check_nd(const char* name, int n, const std::vector<std::vector<std::pair<int, double>>>& rows, int want_roots_min) {
    std::vector<double> xyz(3 * (size_t)n);
    for (int i = 0; i < n; ++i) { xyz[3 * i] = 0.1 * (i % 5); xyz[3 * i + 1] = 0.1 * ((i / 5) % 4); xyz[3 * i + 2] = 0.1 * (i / 20); }
    std::vector<int> aptr(n + 1, 0), aj;
    for (int i = 0; i < n; ++i) {
        for (auto& e : rows[i]) if (e.first != i) aj.push_back(e.first);
        aptr[i + 1] = (int)aj.size();
    }
    const aa::NdTree T = aa::nested_dissection(n, xyz.data(), aptr, aj, 8, 0);
    std::vector<int> inv(n);
    for (int q = 0; q < n; ++q) inv[T.perm[q]] = q;
    aa::CsrMatrix A;
    A.n = n;
    A.ptr.assign(n + 1, 0);
    for (int q = 0; q < n; ++q) {
        std::vector<std::pair<int, double>> r;
        for (auto& e : rows[T.perm[q]]) r.push_back({inv[e.first], e.second});
        std::sort(r.begin(), r.end());
        for (auto& e : r) { A.col.push_back(e.first); A.val.push_back(e.second); }
        A.ptr[q + 1] = (int)A.col.size();
    }
    aa::check_tree_covers(A, T);
    const aa::SupernodalFactor F = aa::multifrontal_cholesky(A, T);
    int roots = 0;
    for (int s = 0; s < F.n_nodes; ++s) roots += F.parent[s] < 0;
    const double res = solve_residual(A, F, T.perm, 99);
    const bool ok = res <= 1e-10 && roots >= want_roots_min;
    std::printf("%s: n=%d supernodes=%d roots=%d |Ax-b|=%.2e %s\n", name, n, F.n_nodes, roots, res, ok ? "ND_OK" : "ND_FAIL");
    return ok ? 0 : 1;
}

}  // namespace

int main() {
    int fails = 0;
    fails += check_blocks("arrow k=3 p=5 q=7", {5, 5, 5, 7}, {3, 3, 3, -1}, 1);
    fails += check_blocks("arrow k=2 p=1 q=40", {1, 1, 40}, {2, 2, -1}, 2);
    fails += check_blocks("single p=33", {33}, {-1}, 3);
    fails += check_blocks("chain k=3 7/13/19", {7, 7, 7, 13, 19}, {3, 3, 3, 4, -1}, 4);
    fails += check_blocks("two roots", {4, 6, 5}, {1, -1, -1}, 5);
    fails += must_throw("coupled siblings", [] {
        const Blocks B = make_blocks({5, 5, 7}, {2, 2, -1}, 6, true);
        aa::check_tree_covers(to_csr(B), aa::explicit_tree(B.n, B.beg, B.end, B.parent));
    });
    fails += must_throw("not a postorder", [] { aa::explicit_tree(6, {0, 3}, {3, 6}, {-1, 0}); });
    fails += must_throw("gap in the ranges", [] { aa::explicit_tree(6, {0, 4}, {3, 6}, {1, -1}); });
    fails += must_throw("ranges short of n", [] { aa::explicit_tree(7, {0, 3}, {3, 6}, {1, -1}); });
    {   // n = 1
        std::vector<std::vector<std::pair<int, double>>> rows(1);
        rows[0].push_back({0, 2.5});
        fails += check_nd("n=1", 1, rows, 1);
    }
    {   // diagonal matrix: every separator empty
        std::vector<std::vector<std::pair<int, double>>> rows(40);
        for (int i = 0; i < 40; ++i) rows[i].push_back({i, 0.5 + 0.1 * i});
        fails += check_nd("diagonal n=40", 40, rows, 2);
    }
    {   // a 5 x 4 x 3 grid (6-point) whose node 17 is isolated
        const int n = 60;
        std::vector<std::vector<std::pair<int, double>>> rows(n);
        std::vector<double> diag(n, 0.3);
        auto edge = [&](int a, int b) {
            if (a == 17 || b == 17) return;
            rows[a].push_back({b, -1.0}); rows[b].push_back({a, -1.0});
            diag[a] += 1.0; diag[b] += 1.0;
        };
        for (int i = 0; i < n; ++i) {
            if (i % 5 != 4) edge(i, i + 1);
            if ((i / 5) % 4 != 3) edge(i, i + 5);
            if (i / 20 != 2) edge(i, i + 20);
        }
        for (int i = 0; i < n; ++i) rows[i].push_back({i, diag[i]});
        fails += check_nd("isolated vertex", n, rows, 1);
    }
    return fails ? 1 : 0;
}
