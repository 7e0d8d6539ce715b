// CPU test of the solve plan (aa-admm_amd/csrc/solve_plan.hpp / .cpp): everything the GPU does in a
// DirectSolver solve is decided by the arrays plan_solve() emits, so their invariants are checked
// here, without a GPU. An SPD 27-point grid matrix goes through nested_dissection ->
// multifrontal_cholesky -> plan_solve for settings modelled on tests/test_gpu_direct_solve.py:
// 24 x 10 x 12 (leaf 8, wave 16 / 32, min_subtrees 8 and 4096) with tile widths 64 / 128 / 256,
// packed on / off, streams off / gated / all, branches 1 / 2 / 4, one and two sets; 12 x 6 x 6; and
// 24 x 10 x 12 dissected for 2 and 3 parts with the dense top. Per plan: membership, level order,
// forward / backward coverage by row tasks or split-K tiles, the dense-top split over the ranks,
// branch ranges, the streamed runs' counters and queue order (a wrong `need` is a hang on the
// GPU), the fused subtrees' items and LDS offsets, the packed offsets; and a one-set plan built
// `wide` equals the two-set plan array by array.
//
//   g++ -O2 -std=c++17 -fopenmp -I aa-admm_amd/csrc tests/cpp/solve_plan.cpp aa-admm_amd/csrc/solve_plan.cpp
//       aa-admm_amd/csrc/spd_direct.cpp -o solve_plan && ./solve_plan
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "solve_plan.hpp"

namespace {

using namespace aa;

int g_fails = 0;
std::string g_label;
#define CHECK(cond, what)                                                                       \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            if (g_fails++ < 20) std::printf("FAIL [%s] %s (line %d)\n", g_label.c_str(), what, __LINE__); \
        }                                                                                       \
    } while (0)

struct Sys {
    int n = 0;
    std::vector<double> xyz;
    std::vector<int> aptr, aj;
    std::vector<std::vector<std::pair<int, double>>> rows;
};

// lumped mass + 27-point stiffness pattern on an nx x ny x nz block, weights from a seeded rng
Sys grid(int nx, int ny, int nz) {
    Sys S;
    const int n = nx * ny * nz;
    S.n = n;
    auto id = [&](int i, int j, int k) { return (i * ny + j) * nz + k; };
    S.xyz.resize(3 * (size_t)n);
    std::mt19937_64 rng(20191015);
    std::uniform_real_distribution<double> U(0.5, 1.5);
    S.rows.resize(n);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k) {
                const int a = id(i, j, k);
                S.xyz[3 * a] = 0.1 * i; S.xyz[3 * a + 1] = 0.1 * j + 0.001 * i; S.xyz[3 * a + 2] = 0.1 * k;
                for (int di = 0; di <= 1; ++di)
                    for (int dj = -1; dj <= 1; ++dj)
                        for (int dk = -1; dk <= 1; ++dk) {
                            if (di == 0 && (dj < 0 || (dj == 0 && dk <= 0))) continue;
                            const int i2 = i + di, j2 = j + dj, k2 = k + dk;
                            if (i2 >= nx || j2 < 0 || j2 >= ny || k2 < 0 || k2 >= nz) continue;
                            const int b = id(i2, j2, k2);
                            const double w = U(rng);
                            S.rows[a].push_back({b, -w}); S.rows[b].push_back({a, -w});
                            S.rows[a].push_back({a, w}); S.rows[b].push_back({b, w});
                        }
                S.rows[a].push_back({a, 0.05 * U(rng)});   // mass
            }
    S.aptr.assign(n + 1, 0);
    for (int v = 0; v < n; ++v) {
        std::vector<int> l;
        for (auto& e : S.rows[v]) if (e.first != v) l.push_back(e.first);
        std::sort(l.begin(), l.end());
        l.erase(std::unique(l.begin(), l.end()), l.end());
        S.aj.insert(S.aj.end(), l.begin(), l.end());
        S.aptr[v + 1] = (int)S.aj.size();
    }
    return S;
}

SupernodalFactor factor(const Sys& S, const NdTree& T) {
    const int n = S.n;
    std::vector<int> inv(n);
    for (int q = 0; q < n; ++q) inv[T.perm[q]] = q;
    CsrMatrix A;
    A.n = n;
    A.ptr.assign(n + 1, 0);
    for (int q = 0; q < n; ++q) {
        std::vector<std::pair<int, double>> r;
        for (auto& e : S.rows[T.perm[q]]) r.push_back({inv[e.first], e.second});
        std::sort(r.begin(), r.end());
        for (size_t k = 0; k < r.size();) {
            size_t k2 = k;
            double s = 0;
            while (k2 < r.size() && r[k2].first == r[k].first) s += r[k2++].second;
            A.col.push_back(r[k].first); A.val.push_back(s);
            k = k2;
        }
        A.ptr[q + 1] = (int)A.col.size();
    }
    return multifrontal_cholesky(A, T);
}

// what the settings exercised, over the whole run: a test that checked no streamed run, no branch,
// no dense top ... would prove nothing
struct Seen {
    int fstreams = 0, bstreams = 0, branched = 0, sub_u = 0, sub_x = 0, tops = 0, row_tasks = 0, waits = 0, xs_reads = 0;
    int tile_w[3] = {0, 0, 0};
} seen;

// rows [lo, hi) marked once each
struct Cover {
    std::vector<int> c;
    explicit Cover(int n) : c(n, 0) {}
    void add(int lo, int hi) { for (int i = std::max(lo, 0); i < hi && i < (int)c.size(); ++i) ++c[i]; if (lo < 0 || hi > (int)c.size()) c.assign(c.size(), 99); }
    bool exactly_once(int lo, int hi) const {
        for (int i = 0; i < (int)c.size(); ++i) if (c[i] != (i >= lo && i < hi ? 1 : 0)) return false;
        return true;
    }
};

// (offset, size) blocks are disjoint and lie in [0, total); returns their sum
long long disjoint_sum(std::vector<std::pair<long long, long long>> blk, long long total, bool& ok) {
    std::sort(blk.begin(), blk.end());
    long long end = 0, sum = 0;
    ok = true;
    for (const auto& b : blk) {
        if (b.first < end || b.second <= 0) ok = false;
        end = b.first + b.second;
        sum += b.second;
    }
    if (end > total) ok = false;
    return sum;
}

void check_membership_and_order(const SolvePlan& P, const SupernodalFactor& F) {
    for (int sn = 0; sn < P.nn; ++sn) {
        const int where = (P.fused[sn] != 0) + (P.lev_of[sn] >= 0) + (sn == P.top_sn);
        CHECK(where == (P.inc[sn] ? 1 : 0), "a held supernode is in exactly one of: fused subtree, level, dense top");
        const int par = F.parent[sn];
        if (P.lev_of[sn] < 0 || par < 0) continue;
        CHECK(P.inc[par] && !P.fused[par], "a level-scheduled supernode's parent is above it");
        CHECK(par == P.top_sn || P.lev_of[par] > P.lev_of[sn], "a child's level precedes its parent's");
    }
    // every fused supernode has one forward and one backward record, in one subtree
    std::map<int, int> by_beg;
    for (int sn = 0; sn < P.nn; ++sn) if (P.fused[sn]) by_beg[P.beg[sn]] = sn;
    std::vector<int> recs(P.nn, 0), tree_of(P.nn, -1);
    for (size_t t = 0; t < P.strees.size(); ++t) {
        const SubTree& T = P.strees[t];
        for (int k = T.node0; k < T.node0 + T.nnode; ++k) {
            const SubNode& nd = P.snodes[k];
            auto it = by_beg.find(nd.beg);
            CHECK(it != by_beg.end(), "a subtree record names a fused supernode");
            if (it == by_beg.end()) continue;
            const int sn = it->second;
            CHECK(nd.p == P.p[sn] && nd.nb == P.nb[sn] && nd.goff == P.goff[sn] && nd.uoff == P.uoff[sn] && nd.ldr == P.ldr[sn] &&
                  nd.bnd_off == P.bnd_off[sn] && nd.ell_off == P.ell_off[sn] && nd.ell_w == P.ell_w[sn], "a subtree record copies its supernode's layout");
            CHECK(tree_of[sn] < 0 || tree_of[sn] == (int)t, "a fused supernode is in one subtree");
            tree_of[sn] = (int)t;
            ++recs[sn];
        }
    }
    for (int sn = 0; sn < P.nn; ++sn) CHECK(recs[sn] == (P.fused[sn] ? 2 : 0), "two records per fused supernode");
}

// the FReds [fr0, fr0 + nfr) of supernode rows: each row block's tiles are its column blocks
// 0, w, 2w, ... up to the diagonal block
void check_freds(const SolvePlan& P, int fr0, int nfr, int w, std::vector<Cover>& cover, bool top) {
    std::vector<std::vector<int>> tiles_of(nfr);
    for (size_t k = 0; k < P.ftiles.size(); ++k) {
        const int rid = P.ftiles[k].rid;
        if (rid >= fr0 && rid < fr0 + nfr) tiles_of[rid - fr0].push_back((int)k);
    }
    for (int i = 0; i < nfr; ++i) {
        const FRed& rd = P.freds[fr0 + i];
        const int sn = P.fr_sn[fr0 + i], p = P.p[sn], R = p + P.nb[sn];
        CHECK(rd.beg == P.beg[sn] && rd.p == p && rd.uoff == P.uoff[sn], "FRed names its supernode");
        CHECK(rd.ell_w == (top ? 0 : P.ell_w[sn]) && rd.ell_off == (top ? 0 : P.ell_off[sn]), "FRed pull list");
        CHECK(rd.nr >= 1 && rd.nr <= 64 && rd.r0 + rd.nr <= R, "FRed rows");
        cover[sn].add(rd.r0, rd.r0 + rd.nr);
        int want = 0;
        for (int c0 = 0; c0 < p && c0 <= rd.r0 + 63; c0 += w) ++want;
        CHECK(rd.nt == want && (int)tiles_of[i].size() == want, "FRed tile count: column blocks up to the diagonal");
        for (size_t k = 0; k < tiles_of[i].size(); ++k) {
            const FTile& ft = P.ftiles[tiles_of[i][k]];
            CHECK(P.ft_sn[tiles_of[i][k]] == sn && P.fwid[tiles_of[i][k]] == w, "forward tile's supernode and width");
            CHECK(ft.c0 == (int)k * w && ft.nc == std::min(w, p - ft.c0) && ft.r0 == rd.r0, "forward tile column block and clip");
            CHECK(ft.beg == P.beg[sn] && ft.p == p && ft.R == R && ft.goff == P.goff[sn], "forward tile names its supernode");
            CHECK(ft.ell_w == rd.ell_w && ft.ell_off == rd.ell_off, "forward tile pull list");
            CHECK(ft.poff == rd.poff + 192LL * (long long)k, "forward partials follow the reduction's first");
        }
    }
}

// the BReds [br0, br0 + nbr) over rows [r_lo, r_hi) of their supernode: each column block's
// tiles are its row blocks from the diagonal (or r_lo) down
void check_breds(const SolvePlan& P, int br0, int nbr, int w, std::vector<Cover>& cover, int top_lo, int top_hi) {
    std::vector<std::vector<int>> tiles_of(nbr);
    for (size_t k = 0; k < P.btiles.size(); ++k) {
        const int rid = P.btiles[k].rid;
        if (rid >= br0 && rid < br0 + nbr) tiles_of[rid - br0].push_back((int)k);
    }
    for (int i = 0; i < nbr; ++i) {
        const BRed& rd = P.breds[br0 + i];
        const int sn = P.br_sn[br0 + i], p = P.p[sn], R = p + P.nb[sn];
        const int r_lo = top_hi > 0 ? top_lo : 0, r_hi = top_hi > 0 ? top_hi : R;
        CHECK(rd.beg == P.beg[sn] && rd.c0 % 128 == 0 && rd.c0 < p && rd.nc == std::min(128, p - rd.c0), "BRed column block");
        cover[sn].add(rd.c0, rd.c0 + rd.nc);
        const int rs = std::max(rd.c0, r_lo);
        const int want = (r_hi - rs + w - 1) / w;
        CHECK(rs < r_hi && rd.nt == want && (int)tiles_of[i].size() == want, "BRed tile count: row blocks from the diagonal down");
        for (size_t k = 0; k < tiles_of[i].size(); ++k) {
            const BTile& bt = P.btiles[tiles_of[i][k]];
            CHECK(P.bt_sn[tiles_of[i][k]] == sn && P.bwid[tiles_of[i][k]] == w, "backward tile's supernode and width");
            CHECK(bt.c0 == rd.c0 && bt.r0 == rs + (int)k * w && bt.nr == std::min(w, r_hi - bt.r0), "backward tile row block and clip");
            CHECK(bt.beg == P.beg[sn] && bt.p == p && bt.nb == P.nb[sn] && bt.goff == P.goff[sn] && bt.ldr == P.ldr[sn] &&
                  bt.bnd_off == P.bnd_off[sn], "backward tile names its supernode");
            CHECK(bt.poff == rd.poff + 384LL * (long long)k, "backward partials follow the reduction's first");
        }
    }
}

void check_coverage(const SolvePlan& P) {
    std::vector<Cover> fcov, bcov;
    for (int sn = 0; sn < P.nn; ++sn) { fcov.emplace_back(P.p[sn] + P.nb[sn]); bcov.emplace_back(P.p[sn]); }
    for (size_t li = 0; li < P.levels.size(); ++li) {
        const Level& L = P.levels[li];
        for (int k = L.fwd_first; k < L.fwd_first + L.fwd_count; ++k) {
            const Task& t = P.tasks[k];
            CHECK(P.lev_of[t.node] == (int)li && t.p <= P.wave_p && t.nr >= 1 && t.nr <= L.fblock, "forward row task");
            CHECK(t.p == P.p[t.node] && t.nb == P.nb[t.node] && t.beg == P.beg[t.node] && t.goff == P.goff[t.node] &&
                  t.uoff == P.uoff[t.node] && t.ldr == P.ldr[t.node] && t.ell_off == P.ell_off[t.node] && t.ell_w == P.ell_w[t.node] &&
                  t.bnd_off == P.bnd_off[t.node], "a task copies its supernode's layout");
            CHECK(24 * t.p <= L.lds_fwd, "forward task's front fits the level's LDS");
            fcov[t.node].add(t.r0, t.r0 + t.nr);
            ++seen.row_tasks;
        }
        for (int k = L.bwd_first; k < L.bwd_first + L.bwd_count; ++k) {
            const Task& t = P.tasks[k];
            CHECK(P.lev_of[t.node] == (int)li && t.p + t.nb <= P.wave_r && t.nr >= 1 && t.nr <= L.bblock, "backward row task");
            CHECK(24 * (t.p + t.nb) <= L.lds_bwd, "backward task's vector fits the level's LDS");
            bcov[t.node].add(t.r0, t.r0 + t.nr);
        }
        for (int k = L.fr_first; k < L.fr_first + L.frd_count; ++k)
            CHECK(P.lev_of[P.fr_sn[k]] == (int)li && P.p[P.fr_sn[k]] > P.wave_p, "forward reduction's supernode is tiled in this level");
        for (int k = L.br_first; k < L.br_first + L.br_count; ++k)
            CHECK(P.lev_of[P.br_sn[k]] == (int)li && P.p[P.br_sn[k]] + P.nb[P.br_sn[k]] > P.wave_r, "backward reduction's supernode is tiled in this level");
        for (int k = L.ft_first; k < L.ft_first + L.ft_count; ++k)
            CHECK(P.ftiles[k].rid >= L.fr_first && P.ftiles[k].rid < L.fr_first + L.frd_count, "a level's forward tiles reduce in the level");
        for (int k = L.bt_first; k < L.bt_first + L.bt_count; ++k)
            CHECK(P.btiles[k].rid >= L.br_first && P.btiles[k].rid < L.br_first + L.br_count, "a level's backward tiles reduce in the level");
        check_freds(P, L.fr_first, L.frd_count, L.ftw, fcov, false);
        check_breds(P, L.br_first, L.br_count, L.btw, bcov, 0, 0);
        if (L.ft_count) ++seen.tile_w[L.ftw == 64 ? 0 : (L.ftw == 128 ? 1 : 2)];
    }
    for (int sn = 0; sn < P.nn; ++sn) {
        if (P.lev_of[sn] < 0) continue;
        CHECK(fcov[sn].exactly_once(0, P.p[sn] + P.nb[sn]), "forward rows [0, p + nb) covered exactly once");
        CHECK(bcov[sn].exactly_once(0, P.p[sn]), "backward columns [0, p) covered exactly once");
    }
    if (P.top_sn >= 0) {   // this rank's slice of the dense top
        const int sn = P.top_sn;
        ++seen.tops;
        int fr0 = (int)P.freds.size(), nfr = 0, br0 = (int)P.breds.size(), nbr = 0;
        for (int k = 0; k < (int)P.freds.size(); ++k) if (P.fr_sn[k] == sn) { fr0 = std::min(fr0, k); ++nfr; }
        for (int k = 0; k < (int)P.breds.size(); ++k) if (P.br_sn[k] == sn) { br0 = std::min(br0, k); ++nbr; }
        check_freds(P, fr0, nfr, P.top_ftw, fcov, true);
        CHECK(fcov[sn].exactly_once(P.top_r0, P.top_r1), "the top's forward tiles cover exactly this rank's rows");
        check_breds(P, br0, nbr, P.top_btw, bcov, P.top_r0, P.top_r1);
        // (whole 128-column blocks: the last one may run past r1, its columns >= r1 get zeros)
        CHECK(bcov[sn].exactly_once(0, P.top_r1 > P.top_r0 ? std::min(P.top_p, (P.top_r1 + 127) / 128 * 128) : 0),
              "the top's backward tiles reach the column blocks of [0, r1)");
        for (int k = 0; k < (int)P.ftiles.size(); ++k)
            CHECK((P.ft_sn[k] == sn) == (k >= P.top_ft_first && k < P.top_ft_first + P.top_ft_count), "the top's forward tile range");
        for (int k = 0; k < (int)P.btiles.size(); ++k)
            CHECK((P.bt_sn[k] == sn) == (k >= P.top_bt_first && k < P.top_bt_first + P.top_bt_count), "the top's backward tile range");
        CHECK(P.top_task.node == sn && P.top_task.r0 == 0 && P.top_task.nr == P.top_p && P.top_p == P.p[sn], "the top's task");
    }
    // partial buffer: every tile's block disjoint, inside the buffer
    std::vector<std::pair<long long, long long>> blk;
    for (const FTile& t : P.ftiles) blk.push_back({t.poff, 192});
    for (const BTile& t : P.btiles) blk.push_back({t.poff, 384});
    bool ok;
    const long long sum = disjoint_sum(blk, P.part_doubles, ok);
    CHECK(ok && sum == P.part_doubles, "tile partials disjoint and inside the partial buffer");
    // packed offsets
    if (P.packed) {
        blk.clear();
        for (size_t k = 0; k < P.ftiles.size(); ++k) blk.push_back({P.ftiles[k].toff, 64LL * P.fwid[k]});
        for (size_t k = 0; k < P.btiles.size(); ++k)
            blk.push_back({P.btiles[k].toff, (P.btiles[k].p - P.btiles[k].c0 <= 64 ? 64LL : 128LL) * P.bwid[k]});
        const long long s2 = disjoint_sum(blk, P.gt_doubles, ok);
        CHECK(ok && s2 == P.gt_doubles, "packed tile blocks disjoint, summing to the Gt size");
    } else {
        CHECK(P.gt_doubles == 0 && !P.stream_plan, "no packed tiles: no Gt, no streamed runs");
    }
}

void check_branches(const SolvePlan& P, const SupernodalFactor& F) {
    const int B = P.nbr;
    CHECK(B >= 1 && B <= kMaxBranches && P.lbr.size() == P.levels.size() * (size_t)(B + 1), "branch ranges per level");
    if (B > 1) ++seen.branched;
    for (size_t li = 0; li < P.levels.size(); ++li) {
        const Level& L = P.levels[li];
        const BrRange* r = &P.lbr[li * (B + 1)];
        struct Q { int first, count; int BrRange::*f; int BrRange::*c; int kind; };
        const Q q[4] = {{L.fwd_first, L.fwd_count, &BrRange::fwd_first, &BrRange::fwd_count, 0},
                        {L.ft_first, L.ft_count, &BrRange::ft_first, &BrRange::ft_count, 1},
                        {L.bwd_first, L.bwd_count, &BrRange::bwd_first, &BrRange::bwd_count, 0},
                        {L.bt_first, L.bt_count, &BrRange::bt_first, &BrRange::bt_count, 2}};
        for (const Q& x : q) {
            int next = x.first;
            for (int b = 0; b <= B; ++b) {
                if (r[b].*x.c == 0) continue;
                CHECK(r[b].*x.f == next, "a level's branch ranges are contiguous, in branch order");
                for (int k = r[b].*x.f; k < r[b].*x.f + r[b].*x.c; ++k) {
                    const int sn = x.kind == 0 ? P.tasks[k].node : (x.kind == 1 ? P.ft_sn[k] : P.bt_sn[k]);
                    CHECK((B > 1 ? P.brn[sn] : 0) == b, "a launch range holds its branch's supernodes only");
                }
                next = r[b].*x.f + r[b].*x.c;
            }
            CHECK(next == x.first + x.count, "the branch ranges partition the launch");
        }
    }
    if (B > 1)
        for (int sn = 0; sn < P.nn; ++sn) {
            if (!P.inc[sn]) continue;
            CHECK(P.brn[sn] >= 0 && P.brn[sn] <= B, "branch in range");
            const int par = F.parent[sn];
            if (par >= 0) CHECK(P.brn[sn] == P.brn[par] || P.brn[par] == B, "a supernode has its parent's branch unless the parent is in the top set");
            CHECK(!(P.fused[sn] && P.brn[sn] == B), "fused supernodes lie below the top set");
        }
    // sub_rng partitions the subtrees; a subtree's records are all of its branch
    CHECK((int)P.sub_rng.size() == B + 1, "subtree ranges per branch");
    std::map<int, int> by_beg;
    for (int sn = 0; sn < P.nn; ++sn) if (P.fused[sn]) by_beg[P.beg[sn]] = sn;
    int next = 0;
    for (int b = 0; b < (int)P.sub_rng.size(); ++b) {
        if (P.sub_rng[b].second == 0) continue;
        CHECK(P.sub_rng[b].first == next, "subtree ranges contiguous");
        for (int t = P.sub_rng[b].first; t < P.sub_rng[b].first + P.sub_rng[b].second && t < (int)P.strees.size(); ++t)
            for (int k = P.strees[t].node0; k < P.strees[t].node0 + P.strees[t].nnode; ++k) {
                auto it = by_beg.find(P.snodes[k].beg);
                if (it != by_beg.end()) CHECK((B > 1 ? P.brn[it->second] : 0) == b, "a subtree is in its branch's range");
            }
        next = P.sub_rng[b].first + P.sub_rng[b].second;
    }
    CHECK(next == (int)P.strees.size(), "the subtree ranges partition the subtrees");
}

// One streamed run: tiles (dep, need), reductions (sig) and the queue. TileT / RedT: forward or backward.
template <class TileT, class RedT>
void check_run(const SolvePlan& P, const Stream& S, const std::vector<TileT>& tiles, const std::vector<RedT>& reds,
               const std::vector<int>& red_sn, const std::vector<int>& order, int counters0) {
    CHECK(S.l0 >= 0 && S.l1 - S.l0 >= 2 && S.l1 <= (int)P.levels.size() && S.head >= 0 && S.head < P.n_heads, "run levels and head");
    CHECK(S.first >= 0 && S.count > 0 && S.first + S.count <= (int)order.size(), "run queue range");
    std::vector<int> pos(tiles.size(), -1);
    for (int k = S.first; k < S.first + S.count; ++k) {
        CHECK(order[k] >= 0 && order[k] < (int)tiles.size() && pos[order[k]] < 0, "a queue names each tile once");
        pos[order[k]] = k;
    }
    std::map<int, int> signals;         // counter -> reductions of the run that add to it
    std::map<int, int> last_signaller;  // counter -> the last queue position of a tile feeding such a reduction
    std::vector<int> run_reds;
    for (size_t i = 0; i < reds.size(); ++i) {
        const int l = P.lev_of[red_sn[i]];
        if (l < S.l0 || l >= S.l1) continue;
        run_reds.push_back((int)i);
        if (reds[i].sig >= 0) ++signals[reds[i].sig];
        else CHECK(reds[i].sig == -1, "sig is a counter or -1");
    }
    int ntiles = 0;
    for (size_t k = 0; k < tiles.size(); ++k) {
        const int rid = tiles[k].rid;
        const int l = P.lev_of[red_sn[rid]];
        if (l < S.l0 || l >= S.l1) continue;
        ++ntiles;
        CHECK(pos[k] >= 0, "every tile of the run's levels is queued");
        const int sig = reds[rid].sig;
        if (sig >= 0) last_signaller[sig] = std::max(last_signaller.count(sig) ? last_signaller[sig] : -1, pos[k]);
    }
    CHECK(ntiles == S.count, "the queue holds the run's tiles only");
    std::map<int, int> waited;
    for (int k = S.first; k < S.first + S.count; ++k) {
        const TileT& t = tiles[order[k]];
        if (t.dep < 0) { CHECK(t.dep == -1 && t.need == 0, "no counter: nothing to wait for"); continue; }
        CHECK(t.dep >= counters0 && t.dep < counters0 + P.nn, "dep is one of the sweep's counters");
        CHECK(t.need == (signals.count(t.dep) ? signals[t.dep] : 0), "need = the run's reductions that signal the tile's counter");
        ++waited[t.dep];
        if (t.need > 0) {
            ++seen.waits;
            CHECK(last_signaller.count(t.dep) && last_signaller[t.dep] < k, "a tile is queued after the tiles whose reductions it waits for");
        }
    }
    for (const auto& s : signals) CHECK(waited.count(s.first), "every sig names a counter some tile of the run waits on");
}

void check_streams(const SolvePlan& P) {
    CHECK(P.stream_plan == (P.stream || P.stream_gated), "stream flags");
    if (!P.stream_plan) { CHECK(P.fstreams.empty() && P.bstreams.empty(), "no runs unless planned"); return; }
    CHECK(!P.fstreams.empty() || !P.bstreams.empty(), "a stream plan has runs");
    CHECK(P.n_heads == (int)(P.fstreams.size() + P.bstreams.size()), "one queue head per run");
    seen.fstreams += (int)P.fstreams.size();
    seen.bstreams += (int)P.bstreams.size();
    std::vector<char> head(P.n_heads, 0);
    for (const Stream& S : P.fstreams) {
        check_run(P, S, P.ftiles, P.freds, P.fr_sn, P.forder, P.n_heads);
        if (S.head >= 0 && S.head < P.n_heads) { CHECK(!head[S.head], "queue heads are distinct"); head[S.head] = 1; }
        for (int l = S.l0; l < S.l1; ++l) CHECK(P.levels[l].fwd_count == 0 && P.levels[l].ftw == P.levels[S.l0].ftw, "a forward run: tiles only, one width");
    }
    for (const Stream& S : P.bstreams) {
        check_run(P, S, P.btiles, P.breds, P.br_sn, P.border, P.n_heads + P.nn);
        if (S.head >= 0 && S.head < P.n_heads) { CHECK(!head[S.head], "queue heads are distinct"); head[S.head] = 1; }
        for (int l = S.l0; l < S.l1; ++l) CHECK(P.levels[l].bwd_count == 0 && P.levels[l].btw == P.levels[S.l0].btw, "a backward run: tiles only, one width");
    }
    CHECK(P.bndx.size() == P.bnd.size(), "one Xs row per boundary entry");
    for (int v : P.bndx) { CHECK(v == -1 || (v >= 0 && v < P.xs_rows), "a bndx entry is -1 or inside Xs"); seen.xs_reads += v >= 0; }
    for (size_t i = 0; i < P.breds.size(); ++i) {
        const int sn = P.br_sn[i], l = P.lev_of[sn];
        bool in_run = false;
        for (const Stream& S : P.bstreams) in_run = in_run || (l >= S.l0 && l < S.l1);
        if (!in_run) continue;
        const BRed& rd = P.breds[i];
        CHECK(rd.xso == -1 || (rd.xso >= 0 && rd.xso % 16 == 0 && rd.xso + P.p[sn] <= P.xs_rows), "a streamed supernode's Xs rows");
        CHECK((rd.sig >= 0) == (rd.xso >= 0), "a reduction publishes x rows iff it signals");
    }
}

void check_subtrees(const SolvePlan& P) {
    CHECK(P.sub_lds_bytes(P.KS, true) <= 160 * 1024 && P.sub_lds_bytes(P.KS, false) <= 160 * 1024, "fused launch LDS within 160 KiB");
    const long long u0 = P.sub_lds_f / 8, u1 = u0 + P.sub_lds_u / 8, x0 = P.sub_lds_b / 8, x1 = x0 + P.sub_lds_x / 8;
    for (const SubTree& T : P.strees) {
        CHECK(T.nnode <= P.sub_nodes_max && T.node0 >= 0 && T.node0 + T.nnode <= (int)P.snodes.size(), "subtree records");
        CHECK(T.lvl0 >= 0 && T.nlvl >= 1 && T.lvl0 + T.nlvl <= (int)P.slevels.size() && T.nlvl <= P.cut_height + 1, "subtree levels");
        const bool ul = (T.flags & kSubU) != 0, xl = (T.flags & kSubX) != 0;
        seen.sub_u += ul; seen.sub_x += xl;
        for (int l = T.lvl0; l < T.lvl0 + T.nlvl; ++l) {
            const SubLevel& L = P.slevels[l];
            auto node = [&](int idx) -> const SubNode* {
                const int k = L.n0 + idx;
                const bool ok = idx >= 0 && k >= T.node0 && k < T.node0 + T.nnode;
                CHECK(ok, "an item's node lies in its subtree");
                return ok ? &P.snodes[k] : nullptr;
            };
            auto range = [&](int first, int count, size_t size) {
                const bool ok = first >= 0 && count >= 0 && (size_t)first + (size_t)count <= size;
                CHECK(ok, "item range");
                return ok;
            };
            // kind: rows the item may name (0: p, 1: p + nb)
            auto items = [&](int first, int count, int kind, bool fwd) {
                if (!range(first, count, P.items.size())) return;
                for (int i = first; i < first + count; ++i) {
                    const SubNode* nd = node(P.items[i] >> 16);
                    if (!nd) continue;
                    const int r = P.items[i] & 0xffff;
                    CHECK(r < (kind ? nd->p + nd->nb : nd->p), "an item's row is in range");
                    // the level vectors: forward p entries from lds, backward p + nb, inside the level budget
                    CHECK(nd->lds >= 0 && 8LL * (nd->lds + 3LL * (fwd ? nd->p : nd->p + nd->nb)) <= (fwd ? P.sub_lds_f : P.sub_lds_b), "a node's level vector lies in LDS");
                }
            };
            items(L.fa0, L.nfa, 0, true);
            items(L.fr0, L.nfr, 1, true);
            items(L.bv0, L.nbv, 1, false);
            items(L.bc0, L.nbc, 0, false);
            if (range(L.bs0, L.nbs, P.items2.size()))
                for (int i = L.bs0; i < L.bs0 + L.nbs; ++i) {
                    const long long it = P.items2[i];
                    const SubNode* nd = node((int)(it >> 40));
                    if (!nd) continue;
                    const int seg = (int)((it >> 20) & 0xfffff), j = (int)(it & 0xfffff), R = nd->p + nd->nb;
                    CHECK(seg * kSubSegRows < R && j < std::min(nd->p, (seg + 1) * kSubSegRows), "a segment item's segment and column");
                    long long slots = 0;
                    for (int sg = 0; sg * kSubSegRows < R; ++sg) slots += std::min(nd->p, (sg + 1) * kSubSegRows);
                    CHECK(nd->slot >= 0 && 8LL * (nd->slot + 3 * slots) <= P.sub_lds_b, "segment partials lie in LDS");
                }
        }
        // forward records first in every level, then the backward copies: tell them by the pull / boundary use
        for (int l = T.lvl0; l < T.lvl0 + T.nlvl; ++l) {
            const SubLevel& L = P.slevels[l];
            const int nlv = (l + 1 < T.lvl0 + T.nlvl ? P.slevels[l + 1].n0 : T.node0 + T.nnode) - L.n0;
            for (int k = 0; k < nlv / 2; ++k) {
                const SubNode& f = P.snodes[L.n0 + k];
                const SubNode& b = P.snodes[L.n0 + nlv / 2 + k];
                CHECK(f.beg == b.beg && f.p == b.p, "a level's backward records mirror its forward records");
                if (ul) CHECK(f.slot == -1 || (f.slot >= u0 && f.slot + 3LL * f.nb <= u1), "an update-vector slot lies in the kSubU region");
                else CHECK(f.slot == -1, "no slot without kSubU");
                for (long long i = f.ell_off; i < f.ell_off + (long long)(f.p + f.nb) * f.ell_w; ++i) {
                    const long long e = P.ell[i];
                    if (e < 0) { CHECK(e == -1, "pull entry"); continue; }
                    if (ul) CHECK(e >= u0 && e + 3 <= u1, "a rewritten pull offset lies in the kSubU region");
                    else CHECK(e + 3 <= P.u_doubles, "a pull offset lies in U");
                }
                if (xl) CHECK(b.xo == -1 || (b.xo >= x0 && b.xo + 3LL * b.p <= T.xst), "a supernode's x rows lie in the kSubX region, before the root's boundary");
                else CHECK(b.xo == -1, "no x rows without kSubX");
                for (int a = 0; a < b.nb; ++a) {
                    const int o = P.bnd[b.bnd_off + a];
                    if (xl) CHECK(o >= x0 && o + 3 <= x1, "a rewritten boundary offset lies in the kSubX region");
                    else CHECK(o >= 0 && o < P.n, "a boundary entry is a row of x");
                }
            }
        }
        if (xl) {
            CHECK(T.xst >= x0 && T.xst + 3LL * T.nxg <= x1 && T.xg_off >= 0 && T.xg_off + T.nxg <= (int)P.xg.size(), "the staged root boundary");
            for (int a = 0; a < T.nxg; ++a) CHECK(P.xg[T.xg_off + a] >= 0 && P.xg[T.xg_off + a] < P.n, "a staged boundary entry is a row of x");
        }
    }
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// the one-set plan built `wide` against the two-set plan: identical apart from the set count
void check_wide(const SolvePlan& A, const SolvePlan& B) {
    CHECK(A.max_sets == 1 && B.max_sets == 2 && A.KS == 2 && B.KS == 2, "wide plans for two sets");
    CHECK(same(A.inc, B.inc) && same(A.beg, B.beg) && same(A.p, B.p) && same(A.nb, B.nb) && same(A.bnd_off, B.bnd_off) &&
          same(A.ldr, B.ldr) && same(A.ell_w, B.ell_w) && same(A.goff, B.goff) && same(A.uoff, B.uoff) && same(A.ell_off, B.ell_off), "wide: layout");
    CHECK(same(A.bnd, B.bnd) && same(A.ell, B.ell), "wide: bnd, ell");
    CHECK(same(A.fused, B.fused) && same(A.snodes, B.snodes) && same(A.slevels, B.slevels) && same(A.strees, B.strees) &&
          same(A.items, B.items) && same(A.items2, B.items2) && same(A.xg, B.xg), "wide: fused subtrees");
    CHECK(A.cut_height == B.cut_height && A.sub_lds_f == B.sub_lds_f && A.sub_lds_b == B.sub_lds_b && A.sub_lds_u == B.sub_lds_u &&
          A.sub_lds_x == B.sub_lds_x && A.sub_nodes_max == B.sub_nodes_max && A.sub_block == B.sub_block, "wide: LDS figures");
    CHECK(A.nbr == B.nbr && same(A.brn, B.brn) && same(A.lbr, B.lbr) && A.sub_rng == B.sub_rng && A.branch_reject == B.branch_reject, "wide: branches");
    CHECK(same(A.levels, B.levels) && same(A.lev_of, B.lev_of) && same(A.tasks, B.tasks) && same(A.ftiles, B.ftiles) && same(A.freds, B.freds) &&
          same(A.btiles, B.btiles) && same(A.breds, B.breds) && same(A.fwid, B.fwid) && same(A.bwid, B.bwid), "wide: levels and tiles");
    CHECK(same(A.fstreams, B.fstreams) && same(A.bstreams, B.bstreams) && same(A.forder, B.forder) && same(A.border, B.border) &&
          same(A.bndx, B.bndx) && A.n_heads == B.n_heads && A.xs_rows == B.xs_rows, "wide: streamed runs");
    CHECK(A.g_doubles == B.g_doubles && A.u_doubles == B.u_doubles && A.part_doubles == B.part_doubles && A.gt_doubles == B.gt_doubles, "wide: buffer sizes");
    CHECK(A.packed == B.packed && A.nt == B.nt && A.nt_rows == B.nt_rows && A.stream == B.stream && A.stream_gated == B.stream_gated &&
          A.stream_plan == B.stream_plan && A.kernels == B.kernels && A.bytes == B.bytes && A.bytes2 == B.bytes2 && A.max_lds == B.max_lds, "wide: switches and counts");
    PlanSummary sa = A.summary, sb = B.summary;
    sa.max_sets = sb.max_sets = 0;
    CHECK(std::memcmp(&sa, &sb, sizeof(sa)) == 0, "wide: summary apart from max_sets");
}

void check_summary(const SolvePlan& P) {
    const PlanSummary& S = P.summary;
    int nfused = 0, ft = 0, bt = 0, tasks_f = 0, tasks_b = 0;
    for (int sn = 0; sn < P.nn; ++sn) nfused += P.fused[sn] != 0;
    for (const Level& L : P.levels) { ft += L.ft_count; bt += L.bt_count; tasks_f += L.fwd_count; tasks_b += L.bwd_count; }
    CHECK(S.supernodes == P.nn && S.levels == (int)P.levels.size() && S.fused_subtrees == (int)P.strees.size() && S.fused_supernodes == nfused, "summary: tree");
    CHECK(S.fwd_tiles == ft && S.bwd_tiles == bt && S.fwd_tasks == tasks_f && S.bwd_tasks == tasks_b, "summary: tasks and tiles");
    CHECK(S.branches == P.nbr && S.packed == (int)P.packed && S.fwd_streams == (int)P.fstreams.size() && S.bwd_streams == (int)P.bstreams.size() &&
          S.stream_all == (int)P.stream && S.stream_gated == (int)P.stream_gated && S.max_sets == P.max_sets, "summary: switches");
    CHECK(tasks_f + tasks_b == (int)P.tasks.size(), "every task belongs to a level");
}

SolvePlan plan_and_check(const std::string& label, const SupernodalFactor& F, const SolvePlanIn& in, const SolveKnobs& K) {
    g_label = label;
    SolvePlan P = plan_solve(in, K);
    check_membership_and_order(P, F);
    check_coverage(P);
    check_branches(P, F);
    check_streams(P);
    check_subtrees(P);
    check_summary(P);
    return P;
}

}  // namespace

int main() {
    const Sys g24 = grid(24, 10, 12), g12 = grid(12, 6, 6);
    int plans = 0;
    {   // one GPU: the kernel-family matrix on 24 x 10 x 12
        const NdTree T = nested_dissection(g24.n, g24.xyz.data(), g24.aptr, g24.aj, 8, 0);
        const SupernodalFactor F = factor(g24, T);
        for (int min_sub : {8, 4096})
            for (int tile : {64, 128, 256})
                for (int packed = 1; packed >= 0; --packed)
                    for (int st = 0; st < 3; ++st)        // streams off, gated, all
                        for (int br : {1, 2, 4}) {
                            SolveKnobs K;
                            K.min_subtrees = min_sub; K.tile = tile; K.packed = packed != 0;
                            K.stream = st == 2; K.stream_gated = st == 0 ? 0 : -1;
                            SolvePlanIn in;
                            in.F = &F; in.wave_p = 16; in.wave_r = 32; in.default_branches = br;
                            char label[128];
                            std::snprintf(label, sizeof label, "g24 min_sub %d tile %d packed %d stream %d branches %d", min_sub, tile, packed, st, br);
                            in.max_sets = 1;
                            const SolvePlan one = plan_and_check(std::string(label) + " sets 1", F, in, K);
                            in.max_sets = 2;
                            const SolvePlan two = plan_and_check(std::string(label) + " sets 2", F, in, K);
                            in.max_sets = 1; in.wide = true;
                            const SolvePlan wide = plan_and_check(std::string(label) + " wide", F, in, K);
                            check_wide(wide, two);
                            CHECK(one.KS == 1 && one.max_sets == 1, "one set");
                            CHECK(one.nbr == (st == 2 ? 1 : one.nbr) && (br == 1 ? one.nbr == 1 : true), "branches off with AA_SOLVE_STREAM, or when not asked");
                            plans += 3;
                        }
        // per-level widths by a tile target, and the LDS residency switched off
        SolvePlanIn in;
        in.F = &F; in.wave_p = 16; in.wave_r = 32; in.max_sets = 2; in.default_branches = 2;
        SolveKnobs K;
        K.min_subtrees = 4096; K.min_tiles = 40;
        plan_and_check("g24 min_tiles 40", F, in, K);
        K = SolveKnobs{};
        K.min_subtrees = 8; K.sub_lds_u = false;
        const SolvePlan nu = plan_and_check("g24 no kSubU", F, in, K);
        K.sub_lds_u = true; K.sub_lds_x = false;
        const SolvePlan nx = plan_and_check("g24 no kSubX", F, in, K);
        g_label = "LDS residency switches";
        CHECK(nu.summary.sub_u == 0 && nu.summary.sub_x > 0 && nx.summary.sub_x == 0 && nx.summary.sub_u > 0, "AA_SUB_LDS_U / _X = 0");
        plans += 3;
    }
    {   // 12 x 6 x 6
        const NdTree T = nested_dissection(g12.n, g12.xyz.data(), g12.aptr, g12.aj, 8, 0);
        const SupernodalFactor F = factor(g12, T);
        for (int sets = 1; sets <= 2; ++sets) {
            SolvePlanIn in;
            in.F = &F; in.wave_p = 16; in.wave_r = 32; in.max_sets = sets;
            SolveKnobs K;
            K.min_subtrees = 4;
            const SolvePlan P = plan_and_check("g12 sets " + std::to_string(sets), F, in, K);
            CHECK(P.summary.fused_subtrees >= 4, "g12 fuses its bottom subtrees");
            ++plans;
        }
    }
    for (int parts : {2, 3}) {   // partitioned with the dense top: every rank's plan, and the split over the ranks
        const NdTree T = nested_dissection(g24.n, g24.xyz.data(), g24.aptr, g24.aj, 8, 0, parts, true, 0);
        const SupernodalFactor F = factor(g24, T);
        for (int tile : {0, 64}) {
            int next = 0, p_top = -1;
            for (int r = 0; r < parts; ++r) {
                SolvePlanIn in;
                in.F = &F; in.node_part = &T.part; in.my_part = r; in.top_beg = T.top_beg; in.comm_size = parts; in.comm_rank = r;
                in.wave_p = 16; in.wave_r = 32; in.max_sets = 2;
                SolveKnobs K;
                K.min_subtrees = 8; K.tile = tile;
                const SolvePlan P = plan_and_check("parts " + std::to_string(parts) + " rank " + std::to_string(r) + " tile " + std::to_string(tile), F, in, K);
                CHECK(P.top_sn >= 0 && P.partitioned && !P.stream_plan && P.nbr >= 1, "the dense top is planned");
                CHECK(P.top_r0 == next && P.top_r1 >= P.top_r0 && (P.top_r1 % kTopBlk == 0 || P.top_r1 == P.top_p), "row slices abut on 64-row boundaries");
                const std::pair<int, int> rows = top_row_split(P.top_p, parts, r);
                CHECK(rows.first == P.top_r0 && rows.second == P.top_r1, "the plan takes top_row_split's rows");
                next = P.top_r1;
                p_top = P.top_p;
                ++plans;
            }
            g_label = "dense top split";
            CHECK(next == p_top && p_top == g24.n - T.top_beg, "the ranks' slices tile [0, p_top)");
        }
    }
    g_label = "what the settings exercised";
    CHECK(seen.fstreams > 0 && seen.bstreams > 0 && seen.waits > 0 && seen.xs_reads > 0, "streamed runs with real waits were checked");
    CHECK(seen.branched > 0 && seen.sub_u > 0 && seen.sub_x > 0 && seen.tops > 0 && seen.row_tasks > 0, "branches, LDS-resident subtrees, dense tops, row tasks were checked");
    CHECK(seen.tile_w[0] > 0 && seen.tile_w[1] > 0 && seen.tile_w[2] > 0, "all three tile widths were checked");
    std::printf("plans %d, streamed runs %d + %d (waits %d, Xs reads %d), branched %d, kSubU %d, kSubX %d, dense tops %d: %s\n", plans,
                seen.fstreams, seen.bstreams, seen.waits, seen.xs_reads, seen.branched, seen.sub_u, seen.sub_x, seen.tops,
                g_fails ? "FAIL" : "PLAN_OK");
    return g_fails ? 1 : 0;
}
