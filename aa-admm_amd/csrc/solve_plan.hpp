// Host-only plan of a DirectSolver solve (no HIP dependency: g++ compiles it, and the CPU tests
// tests/cpp/solve_plan.cpp, cut_height.cpp and update_slots.cpp check it without a GPU).
//
// Everything the GPU does in a solve is decided by the arrays planned here: plan_solve() takes the
// host factor's structure and the knobs (SolveKnobs, the environment read once) and returns a
// SolvePlan -- the factor layout, the pull lists, the fused bottom subtrees, the branches, the
// levels with their row tasks and split-K tiles, the dense-top split, the packed-tile offsets and
// the streamed runs. DirectSolver::build (direct_solve.hip) forms the factor values, uploads the
// plan and runs the transpose / pack kernels; it decides nothing. The stages are in solve_plan.cpp.
//
// The fused kernels (k_fwd_sub / k_bwd_sub) take their dynamic LDS from maxima over ALL
// subtrees: the widest level vectors of any subtree (16-B aligned) plus the node records of the
// largest subtree (SolvePlan::sub_lds_bytes). Those two maxima may come from different
// subtrees, so the cut height is chosen against the same aggregates (a per-subtree
// check let subtree A's wide level and subtree B's many records exceed 160 KiB together).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "spd_direct.hpp"

namespace aa {

// ---- the records the kernels read (device layouts: every field and its place is fixed) ----

// One workgroup's share of a level: rows [r0, r0 + nr) of supernode `node` (forward) or
// its columns (backward), a thread per row. The supernode's metadata rides along so a
// workgroup needs one (scalar) load before its first product.
struct Task {
    int node, r0, nr, pad0;
    int p, nb, beg, bnd_off;
    int ell_w, ldr, pad1, pad2;   // ldr: row stride of the row-major G (p padded to even)
    long long goff, uoff, ell_off, pad3;
};

// Bottom subtrees (all supernodes up to a cut height) are solved whole by one workgroup
// each: their levels are separated by workgroup barriers instead of kernel boundaries.
struct SubNode {   // a supernode inside a fused subtree; lds = its vector's offset in LDS,
    int p, nb, beg, bnd_off, ell_w, lds, slot, ldr;   // slot = its backward segment partials
    long long goff, uoff, ell_off;
    int xo, pad;   // backward copy, kSubX: LDS offset of its x rows (-1: no boundary names them)
};
struct SubLevel { int n0, fa0, nfa, fr0, nfr, bv0, nbv, bc0, nbc, bs0, nbs, pad; };   // item ranges
// nodes [node0, node0 + nnode) staged in LDS. flags: kSubU = the children's update vectors
// stay in LDS (the forward records' slot = the LDS offset of their own, -1 = global U; the
// ELL pull lists of the subtree's supernodes hold LDS offsets); kSubX = the x rows a boundary
// inside the subtree can name stay in LDS -- the columns of its inner supernodes (backward
// record's xo) and the root's boundary (entry a at xst + 3a, staged from x[xg[xg_off + a]]);
// the subtree's boundary lists hold those LDS offsets.
// Offsets are in doubles of a 3-column solve (scaled by NR / 3 on the device, like U's).
constexpr int kSubU = 1, kSubX = 2;
struct SubTree { int lvl0, nlvl, node0, nnode, flags, xst, nxg, xg_off; };
#ifndef AA_SUB_SEG
#define AA_SUB_SEG 64
#endif
constexpr int kSubSegRows = AA_SUB_SEG;   // rows per segment of the fused backward column products
// split-K backward of large supernodes: a tile (64 columns from c0, nr rows from r0) and the
// per-column-block reduction of its nt tile partials (64 x 3 doubles each, from poff)
// toff: the tile's block in the packed tile stream Gt (every tile's factor entries stored
// contiguously in the order its waves consume them)
// streamed levels (see Stream): dep = the counter a tile waits on (its parent's, -1 = none)
// until it reaches need; a reduction adds 1 to counter sig (its own supernode's) when done;
// xso = the supernode's first row in the padded in-launch copy Xs of x
struct BTile { int beg, p, nb, bnd_off, c0, r0, nr, rid, ldr, dep; long long goff, poff, toff; int need, pad; };
struct BRed { int beg, c0, nc, nt; long long poff; int sig, xso; };
// split-K forward of large supernodes: tile (64 rows from r0, nc columns from c0) and the
// per-row-block reduction of its nt partials
// streamed levels: dep / need as for BTile (dep = the tile's own supernode: its children's
// update vectors), sig = the parent's counter a reduction writing update rows adds to
struct FTile { int beg, p, R, c0, r0, nc, rid, ell_w; long long goff, ell_off, poff, toff; int dep, need, pad0, pad1; };
struct FRed { int beg, p, r0, nr, nt, ell_w; long long uoff, ell_off, poff; int sig, pad; };

// Branches (AA_SOLVE_BRANCHES=B; single GPU, not with AA_SOLVE_STREAM): the tree below its top
// supernodes split into B disjoint groups of subtrees, each swept on its own stream. Per level
// and branch (and the top, slot B): the sub-ranges of the level's four launches.
constexpr int kMaxBranches = 8;
struct BrRange { int fwd_first = 0, fwd_count = 0, ft_first = 0, ft_count = 0, bwd_first = 0, bwd_count = 0,
                 bt_first = 0, bt_count = 0; };
struct Level {
    int fwd_first = 0, fwd_count = 0, bwd_first = 0, bwd_count = 0;
    int bt_first = 0, bt_count = 0, br_first = 0, br_count = 0;   // split-K backward tiles
    int ft_first = 0, ft_count = 0, fr_first = 0, frd_count = 0;  // split-K forward tiles
    int fblock = 256, bblock = 256, lds_fwd = 0, lds_bwd = 0;
    int ftw = 256, btw = 256;   // split-K tile widths (forward columns / backward rows)
};
// Streamed tile levels (AA_SOLVE_STREAM=1; measured slower than one launch per level on C4): a run
// of consecutive levels that have split-K tiles only is ONE launch. Its workgroups take tiles in
// level order from a queue (ticket = atomic add), issue their factor loads, and only then wait for
// the tile's inputs: the children's update vectors (forward) or the parent's x rows (backward),
// published in-launch by the reductions (write-through stores, drained, then a counter add; the
// waiting workgroup polls, takes one agent acquire, then reads -- MI355X_MICROARCH.md "Valid
// forms"). A level's factor stream thus overlaps the previous level's tail and reductions
// instead of waiting for its kernel boundary. Same tiles, partials and sums: bit-identical.
struct Stream { int l0, l1, first, count, head; };   // levels [l0, l1), queue order[first, +count)

// What was planned, for tests that must know which kernels a solve runs (capi.cpp
// aa_test_direct_solve). Row-task / tiled supernodes: the level-scheduled (not fused) ones
// whose forward or backward sweep runs as row tasks / split-K tiles (a supernode can be both).
struct PlanSummary {
    int supernodes, levels;                       // all supernodes; level-scheduled heights
    int fused_subtrees, fused_supernodes, sub_u, sub_x;   // subtrees with kSubU / kSubX
    int fwd_tasks, bwd_tasks, fwd_tiles, bwd_tiles;
    int fwd_tile_w, bwd_tile_w;                   // widths in use, or'ed (64 | 128 | 256); 0: no tiles
    int fwd_streams, bwd_streams, stream_all, stream_gated;   // streamed runs; which solves take them
    int branches;
    int packed, nt, nt_rows;
    int row_p_min, row_p_max, row_R_min, row_R_max;       // over row-task supernodes (0 when none)
    int tile_p_min, tile_p_max, tile_R_min, tile_R_max;   // over tiled supernodes
    int fwd_row_nodes, fwd_tile_nodes, bwd_row_nodes, bwd_tile_nodes;
    int fwd_row_bwd_tile_nodes, fwd_tile_bwd_row_nodes;   // the two mixed classes
    int multi_block_fwd_nodes, odd_p_nodes;       // row-task supernodes over several forward blocks; odd p
    int sub_block, wave_p, wave_r, max_sets;
};

// ---- the knobs: every environment variable the solver reads, read once (DirectSolver::build) ----
struct SolveKnobs {
    // tri-state switches: -1 = not set (the planner decides), else 0 / 1
    bool stats = false;            // AA_SOLVE_STATS: print the [solve] lines
    int min_subtrees = -1;         // AA_SOLVE_MIN_SUBTREES (-1: 256, fewer when partitioned)
    int sub_block = 1024;          // AA_SUB_BLOCK: workgroup size of the fused subtrees
    int tile = 0;                  // AA_SOLVE_TILE: one split-K tile width (64 / 128 / 256) everywhere; 0: per level
    int min_tiles = 0;             // AA_SOLVE_MIN_TILES: 0 = 256 everywhere (narrower measured slower on C4)
    int wave_p = -1, wave_r = -1;  // AA_SOLVE_WAVEP / _WAVER (-1: the caller's)
    bool has_wave_p = false, has_wave_r = false;
    int sub_timing = 0;            // AA_SUB_TIMING: solves to time phase by phase
    bool packed = true;            // AA_SOLVE_PACKED=0 keeps the tiles on the strided copies (A/B)
    bool stream = false;           // AA_SOLVE_STREAM=1: every solve streams its tile runs
    int stream_gated = -1;         // AA_SOLVE_STREAM_GATED (-1: on, one GPU)
    bool sub_lds_u = true, sub_lds_x = true;   // AA_SUB_LDS_U / _X = 0: keep those vectors in HBM
    bool has_branches = false;     // AA_SOLVE_BRANCHES (not set: the caller's default)
    int branches = 1;
    bool branches_reject = false;  // AA_SOLVE_BRANCHES_REJECT=1: the gated reject solve branched too
    int factor_nt = -1, factor_nt_rows = -1;   // AA_FACTOR_NT / AA_FACTOR_NT_ROWS (-1: by factor bytes)
    static SolveKnobs from_env();
};

// What the caller of DirectSolver::build decides (the communicator as two ints)
struct SolvePlanIn {
    const SupernodalFactor* F = nullptr;
    const std::vector<int>* node_part = nullptr;   // partitioned: part of every supernode (-1 = shared top)
    int my_part = -1, top_beg = -1;
    int comm_size = 1, comm_rank = 0;
    int max_sets = 1;
    bool wide = false;
    int wave_p = 192, wave_r = 384;
    int default_branches = 1;
};

constexpr int kTopBlk = 64;   // row granularity of the dense top's split (the forward tiles' rows)
// Rows [first, second) of a dense top of p_top rows that `rank` of P takes: blocks of blk rows,
// equal areas of the lower triangle per rank (over the ranks they tile [0, p_top))
inline std::pair<int, int> top_row_split(int p_top, int P, int rank, int blk = kTopBlk) {
    const int nblk = (p_top + blk - 1) / blk;
    const double total = 0.5 * p_top * (p_top + 1.0);
    std::vector<int> cut(P + 1, nblk);
    cut[0] = 0;
    double acc = 0;
    int r = 1;
    for (int b = 0; b < nblk && r < P; ++b) {
        const double r0 = (double)b * blk, r1 = std::min<double>(p_top, r0 + blk);
        acc += 0.5 * (r1 * (r1 + 1) - r0 * (r0 + 1));
        while (r < P && acc >= total * r / P) cut[r++] = b + 1;
    }
    return {std::min(p_top, cut[rank] * blk), std::min(p_top, cut[rank + 1] * blk)};
}

// Everything build() computes that is neither a device buffer nor a factor value
struct SolvePlan {
    int n = 0, nn = 0, max_sets = 1;
    int KS = 1;                 // sets the layout is planned for (2 when `wide` or max_sets = 2)
    bool partitioned = false;   // node_part given and more than one rank
    int top_beg = 0;            // first row of the shared top (n when not partitioned)
    // per supernode: the factor layout (goff / uoff into G / U, ldr = row stride of the row-major G)
    std::vector<char> inc;      // supernodes this solver holds
    std::vector<int> beg, p, nb, bnd_off, ldr, ell_w;
    std::vector<long long> goff, uoff, ell_off;
    std::vector<int> bnd;          // boundary rows (LDS offsets inside kSubX subtrees)
    std::vector<long long> ell;    // per front row, ell_w pull offsets into U (-1 = none)
    long long g_doubles = 0, u_doubles = 0, part_doubles = 0, gt_doubles = 0, xs_rows = 0;   // buffer sizes (one set)
    size_t nnz_L = 0;
    // fused bottom subtrees
    int cut_height = -1, sub_block = 1024, sub_nodes_max = 0;
    int sub_lds_f = 0, sub_lds_b = 0, sub_lds_u = 0, sub_lds_x = 0;   // bytes per 3 columns
    std::vector<char> fused;
    std::vector<SubNode> snodes;
    std::vector<SubLevel> slevels;
    std::vector<SubTree> strees;
    std::vector<int> items, xg;    // (local node << 16 | row) per item; kSubX roots' boundaries (global x rows)
    std::vector<long long> items2; // backward segment items (local node << 40 | segment << 20 | column)
    // branches
    int nbr = 1;
    bool branch_reject = false;
    std::vector<int> brn;                        // branch of every supernode (nbr = top)
    std::vector<BrRange> lbr;                    // [level][nbr + 1]
    std::vector<std::pair<int, int>> sub_rng;    // fused subtrees per branch: (first, count)
    // levels, row tasks, split-K tiles (ft_sn ... = the supernode of every tile / reduction)
    int wave_p = 192, wave_r = 384, max_lds = 0;
    std::vector<Level> levels;
    std::vector<int> lev_of;                     // level of every level-scheduled supernode (-1: none)
    std::vector<Task> tasks;
    std::vector<FTile> ftiles;
    std::vector<FRed> freds;
    std::vector<BTile> btiles;
    std::vector<BRed> breds;
    std::vector<int> fwid, bwid, ft_sn, fr_sn, bt_sn, br_sn;
    // partitioned with a dense shared top (nested_dissection merge_top): the top root supernode
    // top_sn is solved outside the levels, each GPU its rows [top_r0, top_r1)
    int top_sn = -1, top_p = 0, top_r0 = 0, top_r1 = 0;
    int top_ft_first = 0, top_ft_count = 0, top_bt_first = 0, top_bt_count = 0, top_ftw = 256, top_btw = 256;
    Task top_task{};
    // streamed runs
    std::vector<Stream> fstreams, bstreams;
    std::vector<int> forder, border, bndx;   // tile queues; per boundary entry its Xs row (-1: read x)
    int n_heads = 0;
    bool stream = false;        // every solve streams its tile runs
    bool stream_gated = false;  // the reject path's gated solves do
    bool stream_plan = false;   // the runs are planned (either of the above)
    bool packed = true, nt = true, nt_rows = true;
    int kernels = 0, sub_timing = 0;
    double bytes = 0, bytes2 = 0;
    PlanSummary summary{};

    // dynamic LDS of a fused-subtree launch: the level vectors (K sets), the LDS-resident update
    // vectors (forward) or x rows (backward), then the staged node records
    size_t sub_lds_bytes(int K, bool fwd) const {
        const size_t v = (size_t)K * (fwd ? sub_lds_f + sub_lds_u : sub_lds_b + sub_lds_x);
        return (v + 15) / 16 * 16 + (size_t)sub_nodes_max * sizeof(SubNode);
    }
};

// non-temporal factor loads: on when both sweeps' factor bytes exceed kNtBytes, i.e. the factor
// streams past the 256 MB Infinity Cache every solve
constexpr double kNtBytes = 192e6, kNtRowsMaxBytes = 512e6;

// Throws aa::Error (ERR_NUMERIC: inconsistent supernode structure; ERR_STATE: internal checks)
SolvePlan plan_solve(const SolvePlanIn& in, const SolveKnobs& knobs);

struct CutPlanIn {
    const std::vector<int>* parent;   // supernode -> parent (-1 = root)
    const std::vector<int>* height;   // 0 at the leaves
    const std::vector<char>* inc;     // supernodes this solver holds
    const std::vector<int>* p;        // pivots per supernode
    const std::vector<int>* nb;       // boundary rows per supernode
    int max_height = 0;
    int ks = 1;                       // right-hand-side sets (the LDS figures scale with it)
    int min_sub = 256;                // fused subtrees wanted (workgroups)
    int seg_rows = 64;                // backward segment rows (kSubSegRows)
    long long node_bytes = 56;        // sizeof(SubNode)
    long long lds_fwd_level = 64 * 1024, lds_bwd_level = 144 * 1024, lds_max = 160 * 1024;
    int max_item_row = 0xffff;
    const std::vector<std::vector<int>>* kids = nullptr;   // held children per supernode (built here when null)
};

inline bool sub_lds_fits(long long vec_bytes, long long rec_bytes, long long lds_max) {
    return (vec_bytes + 15) / 16 * 16 + rec_bytes <= lds_max;
}

// the largest cut height H (< max_height) such that at least min_sub subtrees root at height
// <= H and the fused launch's aggregate LDS fits; -1 if none
inline int choose_cut_height(const CutPlanIn& a) {
    const auto& parent = *a.parent;
    const auto& height = *a.height;
    const auto& inc = *a.inc;
    const auto& p = *a.p;
    const auto& nb = *a.nb;
    const int nn = (int)parent.size();
    std::vector<std::vector<int>> own;
    if (!a.kids) {
        own.resize(nn);
        for (int sn = 0; sn < nn; ++sn) if (parent[sn] >= 0 && inc[sn]) own[parent[sn]].push_back(sn);
    }
    const std::vector<std::vector<int>>& kids = a.kids ? *a.kids : own;
    for (int H = a.max_height - 1; H >= 1; --H) {
        std::vector<int> roots;
        for (int sn = 0; sn < nn; ++sn)
            if (inc[sn] && height[sn] <= H && (parent[sn] < 0 || height[parent[sn]] > H)) roots.push_back(sn);
        if ((int)roots.size() < a.min_sub) continue;
        bool ok = true;
        long long max_f = 0, max_b = 0, max_rec = 0;
        for (int rt : roots) {
            std::vector<long long> lf(H + 1, 0), lb(H + 1, 0), nodes_at(H + 1, 0);
            std::vector<int> all, st{rt};
            while (!st.empty()) { int v = st.back(); st.pop_back(); all.push_back(v); for (int c : kids[v]) st.push_back(c); }
            // two records per supernode (forward and backward LDS offsets)
            max_rec = std::max(max_rec, 2LL * (long long)all.size() * a.node_bytes);
            for (int v : all) {
                lf[height[v]] += 24LL * a.ks * p[v];
                long long slots = 0;
                for (int sg = 0; sg < (p[v] + nb[v] + a.seg_rows - 1) / a.seg_rows; ++sg)
                    slots += std::min(p[v], (sg + 1) * a.seg_rows);
                lb[height[v]] += 24LL * a.ks * (p[v] + nb[v] + slots);
                nodes_at[height[v]] += 1;
                if (p[v] + nb[v] > a.max_item_row) ok = false;
            }
            for (int h = 0; h <= H; ++h) {
                if (lf[h] > a.lds_fwd_level || lb[h] > a.lds_bwd_level || nodes_at[h] > a.max_item_row) ok = false;
                max_f = std::max(max_f, lf[h]);
                max_b = std::max(max_b, lb[h]);
            }
            if (!ok) break;
        }
        if (ok && sub_lds_fits(max_f, max_rec, a.lds_max) && sub_lds_fits(max_b, max_rec, a.lds_max)) return H;
    }
    return -1;
}

// LDS slots (in rows) for the update vectors a fused subtree keeps on chip (kSubU). `all` is the
// subtree's supernodes, root first; the root's update vector leaves the subtree (slot -1). The
// forward kernel runs a level in two phases -- (1) the front gathers of the level's supernodes,
// (2) their rows, whose boundary rows gather their own front values again and then write the
// supernode's update vector -- so a child's slot is live from its own level until its parent's
// level has finished both phases: slots of level h are taken first-fit, and the children of
// level h are released after them. Returns the peak row count (the LDS region's size).
inline int plan_update_slots(const std::vector<int>& all, const std::vector<std::vector<int>>& kids,
                             const std::vector<int>& height, const std::vector<int>& nb, std::vector<int>& slot) {
    if (all.empty()) return 0;
    const int root = all[0];
    int H = 0;
    for (int v : all) H = std::max(H, height[v]);
    std::vector<std::vector<int>> at(H + 1);
    for (int v : all) at[height[v]].push_back(v);
    std::vector<std::pair<int, int>> used;   // (first row, rows), sorted by first row
    int peak = 0;
    for (int h = 0; h <= H; ++h) {
        std::sort(at[h].begin(), at[h].end());
        for (int v : at[h]) {
            slot[v] = -1;
            if (v == root || nb[v] == 0) continue;
            int pos = 0;
            size_t i = 0;
            for (; i < used.size(); ++i) {
                if (used[i].first - pos >= nb[v]) break;
                pos = used[i].first + used[i].second;
            }
            used.insert(used.begin() + (long)i, {pos, nb[v]});
            slot[v] = pos;
            peak = std::max(peak, pos + nb[v]);
        }
        for (int v : at[h])
            for (int c : kids[v]) {
                if (slot[c] < 0) continue;
                for (size_t i = 0; i < used.size(); ++i)
                    if (used[i].first == slot[c]) { used.erase(used.begin() + (long)i); break; }
            }
    }
    return peak;
}

}  // namespace aa
