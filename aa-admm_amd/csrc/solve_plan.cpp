// The stages of plan_solve() (solve_plan.hpp): host-only, no HIP, no environment reads outside
// SolveKnobs::from_env().
#include "solve_plan.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>

#include "error.hpp"

namespace aa {

SolveKnobs SolveKnobs::from_env() {
    SolveKnobs k;
    auto get = [](const char* name) { return std::getenv(name); };
    auto tri = [&](const char* name) { const char* e = get(name); return e ? (int)(e[0] == '1') : -1; };
    auto not0 = [&](const char* name) { const char* e = get(name); return !(e && e[0] == '0'); };
    auto is1 = [&](const char* name) { const char* e = get(name); return e && e[0] == '1'; };
    k.stats = get("AA_SOLVE_STATS") != nullptr;
    if (const char* e = get("AA_SOLVE_MIN_SUBTREES")) k.min_subtrees = std::atoi(e);
    if (const char* e = get("AA_SUB_BLOCK")) k.sub_block = std::atoi(e);
    if (const char* e = get("AA_SOLVE_TILE")) k.tile = std::atoi(e) >= 256 ? 256 : (std::atoi(e) >= 128 ? 128 : 64);
    if (const char* e = get("AA_SOLVE_MIN_TILES")) k.min_tiles = std::atoi(e);
    if (const char* e = get("AA_SOLVE_WAVEP")) { k.has_wave_p = true; k.wave_p = std::atoi(e); }
    if (const char* e = get("AA_SOLVE_WAVER")) { k.has_wave_r = true; k.wave_r = std::atoi(e); }
    if (const char* e = get("AA_SUB_TIMING")) k.sub_timing = std::atoi(e);
    k.packed = not0("AA_SOLVE_PACKED");
    k.stream = is1("AA_SOLVE_STREAM");
    k.stream_gated = tri("AA_SOLVE_STREAM_GATED");
    k.sub_lds_u = not0("AA_SUB_LDS_U");
    k.sub_lds_x = not0("AA_SUB_LDS_X");
    if (const char* e = get("AA_SOLVE_BRANCHES")) { k.has_branches = true; k.branches = std::atoi(e); }
    k.branches_reject = is1("AA_SOLVE_BRANCHES_REJECT");
    k.factor_nt = tri("AA_FACTOR_NT");
    k.factor_nt_rows = tri("AA_FACTOR_NT_ROWS");
    return k;
}

namespace {

// factor entries of a supernode (dense triangle + boundary block)
inline double entries(int p, int nb) { return 0.5 * p * (p + 1.0) + (double)p * nb; }

// The stages share one view of the tree: the factor's structure, the held children of every
// supernode (built once) and the plan so far.
struct Planner {
    const SolvePlanIn& in;
    const SolveKnobs& K;
    const SupernodalFactor& F;
    SolvePlan& P;
    const int nn;
    std::vector<std::vector<int>> kids;       // held children of every supernode
    std::vector<std::vector<int>> sub_all;    // supernodes of every fused subtree (root first)
    std::vector<int> fidx, bidx;              // forward / backward record of every fused supernode
    double dense = 0, offd = 0, bsum = 0, piv = 0;   // factor entries / rows (the byte counts)

    Planner(const SolvePlanIn& i, const SolveKnobs& k, SolvePlan& pl)
        : in(i), K(k), F(*i.F), P(pl), nn(i.F->n_nodes) {}

    int R(int sn) const { return P.p[sn] + P.nb[sn]; }
    void layout();
    void pull_lists();
    void fused_subtrees();
    void fuse_one(int rt);
    void sub_lds();
    void sub_lds_u(size_t t, long long cap, std::vector<int>& slot);
    bool sub_lds_x(size_t t, long long cap);
    void branches();
    void group_subtrees();
    void sub_stats() const;
    void levels();
    void level_blocks(const std::vector<int>& l, Level& L) const;
    int pick_width(bool fwd, const std::vector<int>& l) const;
    void branch_ranges(const Level& L);
    Task task(int sn, int r0, int nr) const;
    void emit_ftiles(int sn, int r_lo, int r_hi, int w, bool pulls);
    void emit_btiles(int sn, int r_lo, int r_hi, int w);
    void dense_top();
    void packed_offsets();
    void streams();
    std::vector<std::pair<int, int>> runs(bool fwd) const;
    void fwd_run(int l0, int l1, int head, const std::vector<int>& nfr_b);
    void bwd_run(int l0, int l1, int head, const std::vector<int>& nbr, const std::vector<int>& node_sn,
                 std::vector<int>& xso);
    void bytes_and_nt();
    void summary();
};

// ---- layout: which supernodes are held, and where their factor blocks and update vectors lie
void Planner::layout() {
    P.n = F.n;
    P.nn = nn;
    P.max_sets = in.max_sets >= 2 ? 2 : 1;
    // LDS scale the layout (fused-subtree cut, tile width) is planned for: the two-set budget
    // whenever `wide`, so a one-set solver built wide sums every column in the same order as a
    // two-set one (bit-identical AA_Z_PIPELINE=0 / 1)
    P.KS = (in.wide || P.max_sets >= 2) ? 2 : 1;
    P.partitioned = in.node_part && in.comm_size > 1;
    P.top_beg = P.partitioned ? in.top_beg : P.n;
    P.wave_p = K.has_wave_p ? K.wave_p : in.wave_p;
    P.wave_r = K.has_wave_r ? K.wave_r : in.wave_r;
    P.sub_block = K.sub_block;
    P.sub_timing = K.sub_timing;
    // partitioned: this GPU holds the supernodes of its own part and the shared top only
    P.inc.assign(nn, 1);
    if (P.partitioned)
        for (int sn = 0; sn < nn; ++sn) P.inc[sn] = (*in.node_part)[sn] == in.my_part || (*in.node_part)[sn] == -1;
    P.beg.resize(nn); P.p.resize(nn); P.nb.resize(nn); P.bnd_off.resize(nn);
    P.goff.resize(nn); P.uoff.resize(nn);
    P.ldr.assign(nn, 0);
    long long go = 0, uo = 0;
    for (int sn = 0; sn < nn; ++sn) {
        const int ps = F.end[sn] - F.beg[sn], nbs = (int)F.bnd[sn].size();
        P.beg[sn] = F.beg[sn]; P.p[sn] = ps; P.nb[sn] = nbs;
        P.goff[sn] = go; P.uoff[sn] = uo;
        P.ldr[sn] = ps + (ps & 1);   // row-major rows padded to even length (16-B loads in k_bwd_tile)
        P.bnd_off[sn] = (int)P.bnd.size();
        if (!P.inc[sn]) continue;
        P.bnd.insert(P.bnd.end(), F.bnd[sn].begin(), F.bnd[sn].end());
        P.nnz_L += (size_t)ps * (ps + 1) / 2 + (size_t)ps * nbs;
        go += (long long)(ps + nbs) * (ps + (ps & 1));
        uo += 3LL * nbs;
        uo = (uo + 15) / 16 * 16;   // every update vector on 128-B lines of its own (streamed levels)
        dense += 0.5 * ps * (ps + 1.0);
        offd += (double)ps * nbs;
        piv += ps;
        bsum += nbs;
    }
    P.g_doubles = go;
    P.u_doubles = uo;
    // (partitioned: the children of the top that belong to other GPUs' parts contribute nothing
    // here -- their update vectors arrive through the all-reduce of the top rows)
    kids.assign(nn, {});
    for (int sn = 0; sn < nn; ++sn) if (F.parent[sn] >= 0 && P.inc[sn]) kids[F.parent[sn]].push_back(sn);
}

// ---- ELL pull lists (front row q of a parent <- child update entries, fixed order)
void Planner::pull_lists() {
    std::vector<int> pull_off(nn);
    int rows_total = 0;
    for (int sn = 0; sn < nn; ++sn) { pull_off[sn] = rows_total; if (P.inc[sn]) rows_total += R(sn); }
    std::vector<std::vector<long long>> pull(rows_total);
    for (int par = 0; par < nn; ++par) {
        const std::vector<int>& pb = F.bnd[par];
        for (int c : kids[par]) {
            for (int a = 0; a < P.nb[c]; ++a) {
                const int i = F.bnd[c][a];
                int q;
                if (i >= F.beg[par] && i < F.end[par]) q = i - F.beg[par];
                else {
                    auto it = std::lower_bound(pb.begin(), pb.end(), i);
                    if (it == pb.end() || *it != i) throw Error(ERR_NUMERIC, "DirectSolver: inconsistent supernode structure");
                    q = P.p[par] + (int)(it - pb.begin());
                }
                pull[pull_off[par] + q].push_back(P.uoff[c] + 3LL * a);
            }
        }
    }
    P.ell_w.assign(nn, 0);
    P.ell_off.assign(nn, 0);
    for (int sn = 0; sn < nn; ++sn) {
        const int rows = P.inc[sn] ? R(sn) : 0;
        int w = 0;
        for (int q = 0; q < rows; ++q) w = std::max(w, (int)pull[pull_off[sn] + q].size());
        P.ell_w[sn] = w;
        P.ell_off[sn] = (long long)P.ell.size();
        for (int q = 0; q < rows; ++q) {
            const auto& l = pull[pull_off[sn] + q];
            for (int k = 0; k < w; ++k) P.ell.push_back(k < (int)l.size() ? l[k] : -1);
        }
    }
}

// ---- fused bottom subtrees: the largest cut height H such that at least `min_sub` subtrees root
// at height <= H (enough workgroups to fill the chip) and every subtree level fits the LDS
// budget; supernodes above H are solved level by level.
void Planner::fused_subtrees() {
    // fused subtrees wanted: enough workgroups to fill the chip on one GPU; a partitioned GPU's
    // share of the tree is P times smaller, and its fused subtrees cost a latency chain per level
    // whatever their count, so it takes fewer, taller ones (measured)
    const int min_sub = K.min_subtrees != -1 ? K.min_subtrees
                                             : (P.partitioned ? std::max(32, 256 / in.comm_size) : 256);
    // the cut height against the launch's aggregate LDS (the fused kernels' LDS attribute is 160 KiB)
    CutPlanIn pl;
    pl.parent = &F.parent; pl.height = &F.height; pl.inc = &P.inc; pl.p = &P.p; pl.nb = &P.nb;
    pl.max_height = F.max_height; pl.ks = P.KS; pl.min_sub = min_sub; pl.seg_rows = kSubSegRows;
    pl.node_bytes = (long long)sizeof(SubNode);
    pl.kids = &kids;
    P.cut_height = choose_cut_height(pl);
    P.fused.assign(nn, 0);
    fidx.assign(nn, -1);
    bidx.assign(nn, -1);
    if (P.cut_height < 0) return;
    const int H = P.cut_height;
    for (int sn = 0; sn < nn; ++sn)
        if (P.inc[sn] && F.height[sn] <= H && (F.parent[sn] < 0 || F.height[F.parent[sn]] > H)) fuse_one(sn);
}

// the records, level ranges and items of the subtree rooted at rt
void Planner::fuse_one(int rt) {
    const std::vector<int>& p = P.p;
    const std::vector<int>& nb = P.nb;
    std::vector<SubNode>& snodes = P.snodes;
    std::vector<int>& items = P.items;
    std::vector<int> all, st{rt};
    while (!st.empty()) { int v = st.back(); st.pop_back(); all.push_back(v); for (int c : kids[v]) st.push_back(c); }
    const int H = F.height[rt];
    SubTree T{(int)P.slevels.size(), H + 1, (int)snodes.size(), 0};
    for (int h = 0; h <= H; ++h) {
        SubLevel L{};
        L.n0 = (int)snodes.size();
        int lf = 0, lb = 0;
        std::vector<int> lv;
        for (int v : all) if (F.height[v] == h) lv.push_back(v);
        std::sort(lv.begin(), lv.end());
        for (int v : lv) {
            P.fused[v] = 1;
            SubNode nd{};
            nd.p = p[v]; nd.nb = nb[v]; nd.beg = P.beg[v]; nd.bnd_off = P.bnd_off[v]; nd.ell_w = P.ell_w[v];
            nd.lds = 0; nd.goff = P.goff[v]; nd.uoff = P.uoff[v]; nd.ell_off = P.ell_off[v]; nd.ldr = P.ldr[v];
            nd.slot = -1;   // forward copy: LDS update-vector slot (kSubU, set by sub_lds)
            nd.xo = -1;
            fidx[v] = (int)snodes.size();
            snodes.push_back(nd);
        }
        // forward: f_P offsets, assembly items, row items
        L.fa0 = (int)items.size();
        for (size_t k = 0; k < lv.size(); ++k) {
            snodes[L.n0 + k].lds = lf / 8;
            for (int c = 0; c < p[lv[k]]; ++c) items.push_back(((int)k << 16) | c);
            lf += 24 * p[lv[k]];
        }
        L.nfa = (int)items.size() - L.fa0;
        L.fr0 = (int)items.size();
        for (size_t k = 0; k < lv.size(); ++k)
            for (int r = 0; r < R(lv[k]); ++r) items.push_back(((int)k << 16) | r);
        L.nfr = (int)items.size() - L.fr0;
        // backward: the same supernodes with their [y_P ; -x_B] vectors; the LDS
        // offsets differ, so the backward items address a second copy of the nodes
        const int n1 = (int)snodes.size();
        for (size_t k = 0; k < lv.size(); ++k) {
            SubNode nd = snodes[L.n0 + k];
            bidx[lv[k]] = (int)snodes.size();
            nd.lds = lb / 8;
            lb += 24 * R(lv[k]);
            snodes.push_back(nd);
        }
        L.bv0 = (int)items.size();
        for (size_t k = 0; k < lv.size(); ++k)
            for (int r = 0; r < R(lv[k]); ++r) items.push_back(((int)(k + (n1 - L.n0)) << 16) | r);
        L.nbv = (int)items.size() - L.bv0;
        // segment partial slots after the level's vectors; items (node, segment, column)
        L.bs0 = (int)P.items2.size();
        for (size_t k = 0; k < lv.size(); ++k) {
            SubNode& nd = snodes[n1 + k];
            nd.slot = lb / 8;
            const int pp = p[lv[k]], RR = R(lv[k]);
            for (int sg = 0; sg * kSubSegRows < RR; ++sg) {
                const int nc = std::min(pp, (sg + 1) * kSubSegRows);
                for (int j = 0; j < nc; ++j)
                    P.items2.push_back(((long long)(k + (n1 - L.n0)) << 40) | ((long long)sg << 20) | j);
                lb += 24 * nc;
            }
        }
        L.nbs = (int)P.items2.size() - L.bs0;
        L.bc0 = (int)items.size();
        for (size_t k = 0; k < lv.size(); ++k)
            for (int j = 0; j < p[lv[k]]; ++j) items.push_back(((int)(k + (n1 - L.n0)) << 16) | j);
        L.nbc = (int)items.size() - L.bc0;
        P.sub_lds_f = std::max(P.sub_lds_f, lf);
        P.sub_lds_b = std::max(P.sub_lds_b, lb);
        P.slevels.push_back(L);
    }
    T.nnode = (int)snodes.size() - T.node0;
    P.sub_nodes_max = std::max(P.sub_nodes_max, T.nnode);
    P.strees.push_back(T);
    sub_all.push_back(std::move(all));
}

// ---- subtree LDS residency: kSubU / kSubX per subtree where the extra LDS fits beside the level
// vectors and records; rewrites those subtrees' ELL pull lists and boundary lists to LDS offsets
void Planner::sub_lds() {
    // vector bytes (KS sets) a launch may hold: 160 KiB less the staged records
    const long long cap = (160LL * 1024 - (long long)P.sub_nodes_max * (long long)sizeof(SubNode)) / 16 * 16;
    std::vector<int> slot(nn, -1);
    int nu = 0, nx = 0;
    for (size_t t = 0; t < sub_all.size(); ++t) {
        if (K.sub_lds_u) sub_lds_u(t, cap, slot);
        if (K.sub_lds_x) sub_lds_x(t, cap);
        nu += (P.strees[t].flags & kSubU) != 0;
        nx += (P.strees[t].flags & kSubX) != 0;
    }
    if (P.xg.empty()) P.xg.push_back(0);
    if (K.stats)
        std::fprintf(stderr, "[solve] fused subtrees in LDS: update vectors %d / %zu (%d B), x rows %d / %zu (%d B), per 3 columns\n",
                     nu, sub_all.size(), P.sub_lds_u, nx, sub_all.size(), P.sub_lds_x);
}

// kSubU: the update vectors consumed inside subtree t in LDS slots (the regions follow the level vectors)
void Planner::sub_lds_u(size_t t, long long cap, std::vector<int>& slot) {
    const std::vector<int>& all = sub_all[t];
    const int ubase = P.sub_lds_f / 8;
    const int peak = plan_update_slots(all, kids, F.height, P.nb, slot);
    if ((long long)P.KS * (P.sub_lds_f + 24LL * peak) > cap) return;
    P.strees[t].flags |= kSubU;
    P.sub_lds_u = std::max(P.sub_lds_u, 24 * peak);
    for (int v : all) {
        P.snodes[fidx[v]].slot = slot[v] >= 0 ? ubase + 3 * slot[v] : -1;
        // v's pull lists name its children's update entries (all inside the subtree)
        const long long e1 = P.ell_off[v] + (long long)R(v) * P.ell_w[v];
        for (long long i = P.ell_off[v]; i < e1; ++i) {
            const long long e = P.ell[i];
            if (e < 0) continue;
            long long to = -1;
            for (int c : kids[v])
                if (e >= P.uoff[c] && e < P.uoff[c] + 3LL * P.nb[c]) { to = ubase + 3LL * slot[c] + (e - P.uoff[c]); break; }
            if (to < 0) throw Error(ERR_STATE, "DirectSolver: internal error: a pull outside its fused subtree");
            P.ell[i] = to;
        }
    }
}

// kSubX: the x rows a boundary inside subtree t can name: the columns of its inner supernodes
// (a boundary names ancestors only, so leaves' columns never) and the root's boundary (every
// entry leaving the subtree is one of them: fill-path property of the elimination tree;
// checked, else the subtree keeps HBM)
bool Planner::sub_lds_x(size_t t, long long cap) {
    const std::vector<int>& all = sub_all[t];
    const std::vector<int>& beg = P.beg;
    const std::vector<int>& p = P.p;
    SubTree& T = P.strees[t];
    const int xbase = P.sub_lds_b / 8;
    std::vector<std::pair<int, int>> inner;   // (first column, supernode), sorted
    int rows = 0;
    for (int v : all)
        if (!kids[v].empty()) { inner.emplace_back(beg[v], v); rows += p[v]; }
    std::sort(inner.begin(), inner.end());
    const std::vector<int>& rb = F.bnd[all[0]];
    const int nxg = (int)rb.size();
    if ((long long)P.KS * (P.sub_lds_b + 24LL * (rows + nxg)) > cap) return false;
    std::vector<int> xo(inner.size());
    for (size_t k = 0, r = 0; k < inner.size(); r += p[inner[k].second], ++k) xo[k] = xbase + 3 * (int)r;
    std::vector<std::pair<int, int>> rw;
    for (int v : all)
        for (int a = 0; a < P.nb[v]; ++a) {
            const int i = P.bnd[P.bnd_off[v] + a];
            auto in_ = std::upper_bound(inner.begin(), inner.end(), std::make_pair(i, INT_MAX));
            int o = -1;
            if (in_ != inner.begin()) {
                --in_;
                const int w = in_->second;
                if (i < beg[w] + p[w]) o = xo[in_ - inner.begin()] + 3 * (i - beg[w]);
            }
            if (o < 0) {
                auto it = std::lower_bound(rb.begin(), rb.end(), i);
                if (it == rb.end() || *it != i) return false;
                o = xbase + 3 * (rows + (int)(it - rb.begin()));
            }
            rw.emplace_back(P.bnd_off[v] + a, o);
        }
    for (const auto& q : rw) P.bnd[q.first] = q.second;
    for (size_t k = 0; k < inner.size(); ++k) P.snodes[bidx[inner[k].second]].xo = xo[k];
    T.flags |= kSubX;
    T.xst = xbase + 3 * rows;
    T.nxg = nxg;
    T.xg_off = (int)P.xg.size();
    P.xg.insert(P.xg.end(), rb.begin(), rb.end());
    P.sub_lds_x = std::max(P.sub_lds_x, 24 * (rows + nxg));
    return true;
}

// ---- branches: the supernodes that head the B heaviest disjoint subtrees (found by expanding the
// heaviest non-fused node of the frontier, from the roots down, until there are B of them;
// expanded nodes form the top), dealt to B streams by decreasing factor bytes (each to the
// lightest stream so far). Every launch of a sweep below the top then runs once per branch on its
// own stream: a branch's next level starts while another branch's level still drains, so the
// levels' ramp and tail overlap instead of adding up. Same tasks, tiles and sums: bit-identical.
void Planner::branches() {
    const std::vector<int>& p = P.p;
    const std::vector<int>& nb = P.nb;
    P.nbr = 1;
    P.brn.assign(nn, 0);
    P.branch_reject = K.branches_reject;
    const int want = std::max(1, std::min(kMaxBranches, K.has_branches ? K.branches : in.default_branches));
    if (want < 2 || K.stream) return;
    // subtree weights (factor entries), children before parents by height
    std::vector<int> order;
    for (int sn = 0; sn < nn; ++sn) if (P.inc[sn]) order.push_back(sn);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return F.height[a] < F.height[b]; });
    std::vector<double> wt(nn, 0.0);
    for (int sn : order) {
        wt[sn] += entries(p[sn], nb[sn]);
        if (F.parent[sn] >= 0 && P.inc[F.parent[sn]]) wt[F.parent[sn]] += wt[sn];
    }
    std::vector<int> front, top;
    for (int sn : order) if (F.parent[sn] < 0 || !P.inc[F.parent[sn]]) front.push_back(sn);
    while ((int)front.size() < want) {
        int best = -1;
        for (size_t k = 0; k < front.size(); ++k) {
            const int v = front[k];
            if (P.fused[v] || kids[v].empty()) continue;
            if (best < 0 || wt[v] > wt[front[best]]) best = (int)k;
        }
        if (best < 0) break;
        const int v = front[best];
        front.erase(front.begin() + best);
        top.push_back(v);
        for (int c : kids[v]) front.push_back(c);
    }
    if (front.size() < 2) return;
    const int B = std::min<int>(want, (int)front.size());
    std::sort(front.begin(), front.end(), [&](int a, int b) { return wt[a] > wt[b]; });
    std::vector<double> load(B, 0.0);
    for (int v : front) {
        const int b = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[b] += wt[v];
        std::vector<int> st2{v};
        while (!st2.empty()) {
            const int u = st2.back();
            st2.pop_back();
            P.brn[u] = b;
            for (int c : kids[u]) st2.push_back(c);
        }
    }
    for (int v : top) P.brn[v] = B;
    P.nbr = B;
    if (K.stats) {
        double tw = 0;
        for (int v : top) tw += entries(p[v], nb[v]);
        std::fprintf(stderr, "[solve] branches: %d streams, %zu top supernodes (%.1f MB/sweep), branch MB/sweep:", B, top.size(),
                     8e-6 * tw);
        for (double l : load) std::fprintf(stderr, " %.1f", 8e-6 * l);
        std::fprintf(stderr, "\n");
    }
}

// fused subtrees grouped by branch (a SubTree is self-contained: reorder freely)
void Planner::group_subtrees() {
    const int n_sub = (int)P.strees.size();
    P.sub_rng.assign(P.nbr + 1, {0, 0});
    if (P.nbr == 1) { P.sub_rng[0] = {0, n_sub}; return; }
    std::vector<int> ord(n_sub);
    for (int t = 0; t < n_sub; ++t) ord[t] = t;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return P.brn[sub_all[a][0]] < P.brn[sub_all[b][0]]; });
    std::vector<SubTree> st2;
    for (int t : ord) st2.push_back(P.strees[t]);
    P.strees.swap(st2);
    for (int k = 0; k < n_sub; ++k) {
        const int b = P.brn[sub_all[ord[k]][0]];
        if (b < 0 || b >= P.nbr) throw Error(ERR_STATE, "DirectSolver: fused subtree outside the branches");
        if (P.sub_rng[b].second == 0) P.sub_rng[b].first = k;
        ++P.sub_rng[b].second;
    }
}

void Planner::sub_stats() const {
    const int n_sub = (int)P.strees.size();
    double by = 0;
    int nsn = 0;
    for (int sn = 0; sn < nn; ++sn)
        if (P.fused[sn]) { by += 8.0 * entries(P.p[sn], P.nb[sn]); ++nsn; }
    std::fprintf(stderr, "[solve] fused subtrees: %d (cut height %d), %d supernodes, %.2f MB/sweep, lds f %d b %d\n",
                 n_sub, P.cut_height, nsn, by / 1e6, P.sub_lds_f, P.sub_lds_b);
    // per height inside the subtrees: supernodes, rows, the longest forward row loop (p)
    // and bytes -- a level's time is bounded below by its longest serial loop
    for (int h = 0; h <= P.cut_height; ++h) {
        long long cnt = 0, rows = 0, maxp = 0, maxR = 0;
        double bh = 0;
        for (int sn = 0; sn < nn; ++sn) {
            if (!P.fused[sn] || F.height[sn] != h) continue;
            ++cnt; rows += R(sn);
            maxp = std::max<long long>(maxp, P.p[sn]); maxR = std::max<long long>(maxR, R(sn));
            bh += 8.0 * entries(P.p[sn], P.nb[sn]);
        }
        std::fprintf(stderr, "[solve]   sub height %d: %lld supernodes, %.1f rows/subtree, max p %lld, max R %lld, %.2f MB\n",
                     h, cnt, n_sub ? (double)rows / n_sub : 0.0, maxp, maxR, bh / 1e6);
    }
}

Task Planner::task(int sn, int r0, int nr) const {
    Task t{};
    t.node = sn; t.r0 = r0; t.nr = nr;
    t.p = P.p[sn]; t.nb = P.nb[sn]; t.beg = P.beg[sn]; t.bnd_off = P.bnd_off[sn];
    t.ell_w = P.ell_w[sn];
    t.goff = P.goff[sn]; t.uoff = P.uoff[sn]; t.ell_off = P.ell_off[sn]; t.ldr = P.ldr[sn];
    return t;
}

// Split-K forward tiles of rows [r_lo, r_hi) of supernode sn (64 rows x w columns; tiles entirely
// above the diagonal of L_PP^-1 are zero and skipped), one reduction task per row block.
// pulls = false: the front is read assembled (the dense top's), no pull list.
void Planner::emit_ftiles(int sn, int r_lo, int r_hi, int w, bool pulls) {
    const int p = P.p[sn];
    const long long ell_off = pulls ? P.ell_off[sn] : 0;
    const int ell_w = pulls ? P.ell_w[sn] : 0;
    for (int r0 = r_lo; r0 < r_hi; r0 += 64) {
        FRed rd{};
        rd.beg = P.beg[sn]; rd.p = p; rd.r0 = r0; rd.nr = std::min(64, r_hi - r0);
        rd.uoff = P.uoff[sn]; rd.ell_off = ell_off; rd.ell_w = ell_w; rd.poff = P.part_doubles;
        for (int c0 = 0; c0 < p; c0 += w) {
            if (r0 + 63 < c0) break;
            FTile ft{};
            ft.beg = P.beg[sn]; ft.p = p; ft.R = R(sn); ft.c0 = c0; ft.r0 = r0;
            ft.nc = std::min(w, p - c0);
            ft.goff = P.goff[sn]; ft.ell_off = ell_off; ft.ell_w = ell_w; ft.poff = P.part_doubles;
            ft.rid = (int)P.freds.size();
            P.part_doubles += 3 * 64;
            P.ftiles.push_back(ft);
            P.fwid.push_back(w);
            P.ft_sn.push_back(sn);
            ++rd.nt;
        }
        P.freds.push_back(rd);
        P.fr_sn.push_back(sn);
    }
}

// Split-K backward tiles of rows [r_lo, r_hi) of supernode sn (128 columns x w rows; the tiles
// above the diagonal of L_PP^-1 are all zero and skipped) and one reduction task per column block
// that those rows reach
void Planner::emit_btiles(int sn, int r_lo, int r_hi, int w) {
    const int p = P.p[sn];
    for (int c0 = 0; c0 < std::min(p, r_hi); c0 += 128) {
        const int rs = std::max(c0, r_lo);
        if (rs >= r_hi) continue;
        BRed rd{};
        rd.beg = P.beg[sn]; rd.c0 = c0; rd.nc = std::min(128, p - c0); rd.poff = P.part_doubles;
        for (int r0 = rs; r0 < r_hi; r0 += w) {
            BTile bt{};
            bt.beg = P.beg[sn]; bt.p = p; bt.nb = P.nb[sn]; bt.bnd_off = P.bnd_off[sn];
            bt.c0 = c0; bt.r0 = r0; bt.nr = std::min(w, r_hi - r0);
            bt.goff = P.goff[sn]; bt.poff = P.part_doubles; bt.ldr = P.ldr[sn];
            bt.rid = (int)P.breds.size();
            P.part_doubles += 6 * 64;
            P.btiles.push_back(bt);
            P.bwid.push_back(w);
            P.bt_sn.push_back(sn);
            ++rd.nt;
        }
        P.breds.push_back(rd);
        P.br_sn.push_back(sn);
    }
}

// workgroup sizes of a level's row tasks: by its longest forward row count / backward column count
void Planner::level_blocks(const std::vector<int>& l, Level& L) const {
    int fr = 0, br = 0;
    for (int sn : l) {
        if (P.p[sn] <= P.wave_p) fr = std::max(fr, R(sn));
        if (R(sn) <= P.wave_r) br = std::max(br, P.p[sn]);
    }
    L.fblock = fr > 128 ? 256 : (fr > 64 ? 128 : 64);
    L.bblock = br > 128 ? 256 : (br > 64 ? 128 : 64);
}

// split-K tile width (forward columns / backward rows) of a level: the widest of 256 / 128 / 64
// that still gives the level >= min_tiles workgroups (a level of few big supernodes gets narrow
// tiles and enough workgroups to keep loads in flight on every CU; wide tiles keep the partial
// traffic low where there is parallelism anyway). Structure only: the same for one- and two-set
// solves. AA_SOLVE_TILE forces one width, AA_SOLVE_MIN_TILES the target.
int Planner::pick_width(bool fwd, const std::vector<int>& l) const {
    if (K.tile) return K.tile;
    if (K.min_tiles <= 0) return 256;
    for (int w : {256, 128}) {
        long long n = 0;
        for (int sn : l) {
            const int p = P.p[sn], rows = R(sn);
            if (fwd && p > P.wave_p)
                for (int r0 = 0; r0 < rows; r0 += 64) n += std::min((r0 + 63) / w + 1, (p + w - 1) / w);
            if (!fwd && rows > P.wave_r)
                for (int c0 = 0; c0 < p; c0 += 128) n += (rows - c0 + w - 1) / w;
        }
        if (n >= K.min_tiles) return w;
    }
    return 64;
}

// per branch (and the top, slot nbr): the sub-ranges of a level's four launches
void Planner::branch_ranges(const Level& L) {
    const size_t base = P.lbr.size();
    P.lbr.resize(base + P.nbr + 1);
    auto ranges = [&](int first, int count, auto node_of, int BrRange::*f, int BrRange::*c) {
        for (int k = first; k < first + count; ++k) {
            const int b = P.nbr > 1 ? P.brn[node_of(k)] : 0;
            BrRange& r = P.lbr[base + b];
            if (r.*c == 0) r.*f = k;
            else if (r.*f + r.*c != k) throw Error(ERR_STATE, "DirectSolver: branch ranges not contiguous");
            ++(r.*c);
        }
    };
    ranges(L.fwd_first, L.fwd_count, [&](int k) { return P.tasks[k].node; }, &BrRange::fwd_first, &BrRange::fwd_count);
    ranges(L.ft_first, L.ft_count, [&](int k) { return P.ft_sn[k]; }, &BrRange::ft_first, &BrRange::ft_count);
    ranges(L.bwd_first, L.bwd_count, [&](int k) { return P.tasks[k].node; }, &BrRange::bwd_first, &BrRange::bwd_count);
    ranges(L.bt_first, L.bt_count, [&](int k) { return P.bt_sn[k]; }, &BrRange::bt_first, &BrRange::bt_count);
}

// ---- levels by height: row tasks for the small supernodes, split-K tiles for the large ones
void Planner::levels() {
    const std::vector<int>& p = P.p;
    // partitioned: the shared top as ONE dense root supernode (nested_dissection merge_top) is
    // split over the GPUs by rows instead of being solved whole on each
    if (P.partitioned) {
        int ntop = 0, cand = -1;
        for (int sn = 0; sn < nn; ++sn)
            if ((*in.node_part)[sn] == -1 && p[sn] > 0) { ++ntop; cand = sn; }
        if (ntop == 1 && F.parent[cand] < 0 && P.nb[cand] == 0 && P.beg[cand] == P.top_beg && p[cand] == P.n - P.top_beg &&
            !P.fused[cand])
            P.top_sn = cand;
    }
    std::vector<std::vector<int>> hl(F.max_height + 1);
    for (int sn = 0; sn < nn; ++sn) if (!P.fused[sn] && P.inc[sn] && sn != P.top_sn) hl[F.height[sn]].push_back(sn);
    P.lev_of.assign(nn, -1);
    for (auto& l : hl) {
        if (l.empty()) continue;
        if (P.nbr > 1)   // contiguous per branch (then the top): every launch below takes a range
            std::stable_sort(l.begin(), l.end(), [&](int a, int b) { return P.brn[a] < P.brn[b]; });
        Level L;
        level_blocks(l, L);
        L.fwd_first = (int)P.tasks.size();
        for (int sn : l) {
            if (p[sn] > P.wave_p) continue;
            for (int r0 = 0; r0 < R(sn); r0 += L.fblock) P.tasks.push_back(task(sn, r0, std::min(L.fblock, R(sn) - r0)));
            L.lds_fwd = std::max(L.lds_fwd, 24 * p[sn]);
        }
        L.fwd_count = (int)P.tasks.size() - L.fwd_first;
        L.ftw = pick_width(true, l);
        L.btw = pick_width(false, l);
        L.ft_first = (int)P.ftiles.size();
        L.fr_first = (int)P.freds.size();
        for (int sn : l) if (p[sn] > P.wave_p) emit_ftiles(sn, 0, R(sn), L.ftw, true);
        L.ft_count = (int)P.ftiles.size() - L.ft_first;
        L.frd_count = (int)P.freds.size() - L.fr_first;
        L.bwd_first = (int)P.tasks.size();
        for (int sn : l) {
            if (R(sn) > P.wave_r) continue;
            for (int j0 = 0; j0 < p[sn]; j0 += L.bblock) P.tasks.push_back(task(sn, j0, std::min(L.bblock, p[sn] - j0)));
            L.lds_bwd = std::max(L.lds_bwd, 24 * R(sn));
        }
        L.bwd_count = (int)P.tasks.size() - L.bwd_first;
        L.bt_first = (int)P.btiles.size();
        L.br_first = (int)P.breds.size();
        for (int sn : l) if (R(sn) > P.wave_r) emit_btiles(sn, 0, R(sn), L.btw);
        L.bt_count = (int)P.btiles.size() - L.bt_first;
        L.br_count = (int)P.breds.size() - L.br_first;
        P.max_lds = std::max(P.max_lds, std::max(L.lds_fwd, L.lds_bwd));
        P.kernels += (L.fwd_count ? 1 : 0) + (L.bwd_count ? 1 : 0) + (L.bt_count ? 1 : 0) + (L.ft_count ? 1 : 0);
        branch_ranges(L);
        P.levels.push_back(L);
        for (int sn : l) P.lev_of[sn] = (int)P.levels.size() - 1;
        if (K.stats) {
            double by = 0;
            int maxp = 0, maxnb = 0, nw = 0;
            for (int sn : l) {
                by += 8.0 * entries(p[sn], P.nb[sn]);
                maxp = std::max(maxp, p[sn]); maxnb = std::max(maxnb, P.nb[sn]);
                nw += p[sn] > P.wave_p;
            }
            std::fprintf(stderr, "[solve] level %zu: %zu supernodes (%d tiled), max p %d, max nb %d, %.2f MB/sweep, "
                         "fwd tasks %d (blk %d) fwd tiles %d (w %d) bwd tasks %d (blk %d) bwd tiles %d (w %d)\n",
                         P.levels.size() - 1, l.size(), nw, maxp, maxnb, by / 1e6, L.fwd_count, L.fblock, L.ft_count, L.ftw,
                         L.bwd_count, L.bblock, L.bt_count, L.btw);
        }
    }
}

// ---- dense top: this GPU's rows [top_r0, top_r1) of the top triangle (top_row_split). Forward
// tiles of the own rows, the front read summed; backward the products of the own rows only (a
// partial x_top, summed over the GPUs)
void Planner::dense_top() {
    if (P.top_sn < 0) return;
    const int sn = P.top_sn, pt = P.p[sn];
    const std::pair<int, int> rows = top_row_split(pt, in.comm_size, in.comm_rank);
    P.top_p = pt;
    P.top_r0 = rows.first;
    P.top_r1 = rows.second;
    P.top_task = task(sn, 0, pt);
    P.top_ftw = P.top_btw = K.tile ? K.tile : 256;
    P.top_ft_first = (int)P.ftiles.size();
    emit_ftiles(sn, P.top_r0, P.top_r1, P.top_ftw, false);
    P.top_ft_count = (int)P.ftiles.size() - P.top_ft_first;
    P.top_bt_first = (int)P.btiles.size();
    emit_btiles(sn, P.top_r0, P.top_r1, P.top_btw);
    P.top_bt_count = (int)P.btiles.size() - P.top_bt_first;
    P.kernels += 4;
    // bytes: this GPU streams its row slice of the triangle (twice), not the whole top
    const double whole = 0.5 * pt * (pt + 1.0), a0 = P.top_r0, a1 = P.top_r1;
    dense -= whole;
    dense += 0.5 * (a1 * (a1 + 1) - a0 * (a0 + 1));
    if (K.stats)
        std::fprintf(stderr, "[solve] dense top: %d rows, this GPU rows [%d, %d), fwd tiles %d, bwd tiles %d\n", pt,
                     P.top_r0, P.top_r1, P.top_ft_count, P.top_bt_count);
}

// ---- packed tiles: every tile's block of Gt, in consumption order (see k_fwd_ptile)
void Planner::packed_offsets() {
    P.packed = K.packed && (!P.ftiles.empty() || !P.btiles.empty());
    if (!P.packed) return;
    long long to = 0;
    for (size_t i = 0; i < P.ftiles.size(); ++i) { P.ftiles[i].toff = to; to += 64LL * P.fwid[i]; }
    for (size_t i = 0; i < P.btiles.size(); ++i) {   // narrow blocks (<= 64 columns): half (k_pack_btiles)
        P.btiles[i].toff = to;
        to += (P.btiles[i].p - P.btiles[i].c0 <= 64 ? 64LL : 128LL) * P.bwid[i];
    }
    P.gt_doubles = to;
    if (K.stats) std::fprintf(stderr, "[solve] packed tiles: %zu forward, %zu backward, %.1f MB\n", P.ftiles.size(),
                              P.btiles.size(), 8e-6 * (double)to);
}

// maximal runs of >= 2 consecutive levels with split-K tiles only and one tile width
std::vector<std::pair<int, int>> Planner::runs(bool fwd) const {
    const int nL = (int)P.levels.size();
    auto ok = [&](int l) {
        const Level& L = P.levels[l];
        return fwd ? (L.fwd_count == 0 && L.ft_count > 0) : (L.bwd_count == 0 && L.bt_count > 0);
    };
    auto wid = [&](int l) { return fwd ? P.levels[l].ftw : P.levels[l].btw; };
    std::vector<std::pair<int, int>> r;
    for (int i = 0; i < nL;) {
        if (!ok(i)) { ++i; continue; }
        int j = i + 1;
        while (j < nL && ok(j) && wid(j) == wid(i)) ++j;
        if (j - i >= 2) r.push_back({i, j});
        i = j;
    }
    return r;
}

// ---- streamed tile levels (see Stream in solve_plan.hpp). Forward: a tile of supernode s waits
// for every update-row reduction of its children in the same run; backward: for every reduction
// of its parent in the same run (the parent's rows and, through the parent's own wait, all its
// ancestors' rows in the run).
void Planner::streams() {
    P.stream = P.packed && K.stream;   // measured slower on C4: opt-in
    // a gated solve that is skipped (the Anderson reject path's, most iterations) costs one
    // dependent launch (~4.6 us in a graph) per level: its tile runs as one launch each cut
    // that; taken, a streamed run is slower than its levels
    P.stream_gated = P.packed && !in.node_part && K.stream_gated != 0;   // (one GPU)
    P.stream_plan = P.stream || P.stream_gated;
    P.bndx.assign(P.bnd.size(), -1);
    if (!P.stream_plan) return;
    const auto fr = runs(true), br = runs(false);
    P.n_heads = (int)(fr.size() + br.size());
    std::vector<int> nfr_b(nn, 0), nbr(nn, 0);     // per supernode: update-row / all reductions
    for (size_t i = 0; i < P.freds.size(); ++i)
        if (P.freds[i].r0 + P.freds[i].nr > P.freds[i].p) ++nfr_b[P.fr_sn[i]];
    for (size_t i = 0; i < P.breds.size(); ++i) ++nbr[P.br_sn[i]];
    int head = 0;
    for (const auto& run : fr) fwd_run(run.first, run.second, head++, nfr_b);
    std::vector<int> node_sn(P.n, -1), xso(nn, -1);
    for (int sn = 0; sn < nn; ++sn)
        for (int i = F.beg[sn]; i < F.end[sn] && i < P.n; ++i) node_sn[i] = sn;
    for (auto it = br.rbegin(); it != br.rend(); ++it)   // processing order: top runs first
        bwd_run(it->first, it->second, head++, nbr, node_sn, xso);
    if (K.stats)
        for (auto& S : P.fstreams)
            std::fprintf(stderr, "[solve] streamed forward levels [%d, %d): %d tiles, one launch\n", S.l0, S.l1, S.count);
    if (K.stats)
        for (auto& S : P.bstreams)
            std::fprintf(stderr, "[solve] streamed backward levels [%d, %d): %d tiles, one launch\n", S.l0, S.l1, S.count);
    if (P.fstreams.empty() && P.bstreams.empty()) P.stream = P.stream_gated = P.stream_plan = false;
}

// counters in the sync buffer: [queue heads | forward counters (nn) | backward counters (nn)]
void Planner::fwd_run(int l0, int l1, int head, const std::vector<int>& nfr_b) {
    const int CF = P.n_heads;
    auto in_run = [&](int sn) { return sn >= 0 && P.lev_of[sn] >= l0 && P.lev_of[sn] < l1; };
    Stream S{l0, l1, (int)P.forder.size(), 0, head};
    for (int l = l0; l < l1; ++l)
        for (int k = 0; k < P.levels[l].ft_count; ++k) P.forder.push_back(P.levels[l].ft_first + k);
    S.count = (int)P.forder.size() - S.first;
    for (int k = S.first; k < S.first + S.count; ++k) {
        FTile& ft = P.ftiles[P.forder[k]];
        const int sn = P.ft_sn[P.forder[k]];
        int need = 0;
        for (int c : kids[sn]) if (in_run(c)) need += nfr_b[c];
        ft.dep = CF + sn;
        ft.need = need;
    }
    for (size_t i = 0; i < P.freds.size(); ++i) {
        const int sn = P.fr_sn[i];
        if (!in_run(sn)) continue;
        const int par = F.parent[sn];
        P.freds[i].sig = (in_run(par) && P.freds[i].r0 + P.freds[i].nr > P.freds[i].p) ? CF + par : -1;
    }
    P.fstreams.push_back(S);
}

void Planner::bwd_run(int l0, int l1, int head, const std::vector<int>& nbr, const std::vector<int>& node_sn,
                      std::vector<int>& xso) {
    const int CB = P.n_heads + nn;
    auto in_run = [&](int sn) { return sn >= 0 && P.lev_of[sn] >= l0 && P.lev_of[sn] < l1; };
    Stream S{l0, l1, (int)P.border.size(), 0, head};
    for (int l = l1 - 1; l >= l0; --l)
        for (int k = 0; k < P.levels[l].bt_count; ++k) P.border.push_back(P.levels[l].bt_first + k);
    S.count = (int)P.border.size() - S.first;
    std::vector<char> has_kid(nn, 0);
    for (int l = l0; l < l1; ++l)
        for (int k = 0; k < P.levels[l].bt_count; ++k) {
            const int sn = P.bt_sn[P.levels[l].bt_first + k];
            if (in_run(F.parent[sn])) has_kid[F.parent[sn]] = 1;
        }
    for (int k = S.first; k < S.first + S.count; ++k) {
        BTile& bt = P.btiles[P.border[k]];
        const int sn = P.bt_sn[P.border[k]], par = F.parent[sn];
        bt.dep = in_run(par) ? CB + par : -1;
        bt.need = in_run(par) ? nbr[par] : 0;
        if (has_kid[sn] && xso[sn] < 0) { xso[sn] = (int)P.xs_rows; P.xs_rows += (P.p[sn] + 15) / 16 * 16; }
    }
    for (size_t i = 0; i < P.breds.size(); ++i) {
        const int sn = P.br_sn[i];
        if (!in_run(sn)) continue;
        P.breds[i].sig = has_kid[sn] ? CB + sn : -1;
        P.breds[i].xso = xso[sn];
    }
    // boundary rows of this run's supernodes owned by supernodes of the run: read from Xs
    for (int l = l0; l < l1; ++l)
        for (int k = 0; k < P.levels[l].bt_count; ++k) {
            const int sn = P.bt_sn[P.levels[l].bt_first + k];
            for (int a = 0; a < P.nb[sn]; ++a) {
                const int node = F.bnd[sn][a], ow = node < P.n ? node_sn[node] : -1;
                if (ow >= 0 && in_run(ow) && xso[ow] >= 0) P.bndx[P.bnd_off[sn] + a] = xso[ow] + (node - P.beg[ow]);
            }
        }
    P.bstreams.push_back(S);
}

// ---- algorithmic bytes of one solve: the factor once per sweep (dense triangles + boundary
// blocks, fp64), b/y/x (24 B per node each way) and the update vectors (write + read); and
// non-temporal factor loads when a solve's factor stream cannot stay in the Infinity Cache
void Planner::bytes_and_nt() {
    if (!P.strees.empty()) P.kernels += 2;
    const double factor = 2.0 * 8.0 * (dense + offd);
    P.bytes = factor + 4.0 * 24.0 * piv + 3.0 * 24.0 * bsum;
    P.bytes2 = factor + 2.0 * (4.0 * 24.0 * piv + 3.0 * 24.0 * bsum);
    P.nt = K.factor_nt >= 0 ? K.factor_nt == 1 : factor > kNtBytes;
    // the thread-per-row kernels (fused subtrees, row tasks) separately (AA_FACTOR_NT_ROWS):
    // their 8-B-per-lane loads cover partial lines that a neighbouring wave re-reads, which nt
    // drops from L2 (PMC, C4: fused backward 1.41 -> 1.81x its factor bytes read). Measured
    // (same-box A/B): nt on the rows costs C4 (2 GB both sweeps) 33 us and C5 (0.69 GB) 44 us
    // per solve, and saves C3 (0.28 GB) 12 us -- on only where the factor is within ~2x the
    // Infinity Cache
    P.nt_rows = K.factor_nt_rows >= 0 ? K.factor_nt_rows == 1 : (P.nt && factor < kNtRowsMaxBytes);
}

// ---- the plan in numbers
void Planner::summary() {
    PlanSummary& S = P.summary;
    S = PlanSummary{};
    for (const SubTree& T : P.strees) { S.sub_u += (T.flags & kSubU) != 0; S.sub_x += (T.flags & kSubX) != 0; }
    S.supernodes = nn; S.levels = (int)P.levels.size();
    S.fused_subtrees = (int)P.strees.size();
    for (int sn = 0; sn < nn; ++sn) S.fused_supernodes += P.fused[sn] != 0;
    for (const Level& L : P.levels) {
        S.fwd_tasks += L.fwd_count; S.bwd_tasks += L.bwd_count;
        S.fwd_tiles += L.ft_count; S.bwd_tiles += L.bt_count;
        if (L.ft_count) S.fwd_tile_w |= L.ftw;
        if (L.bt_count) S.bwd_tile_w |= L.btw;
    }
    S.fwd_streams = (int)P.fstreams.size(); S.bwd_streams = (int)P.bstreams.size();
    S.stream_all = P.stream; S.stream_gated = P.stream_gated;
    S.branches = P.nbr;
    S.packed = P.packed; S.nt = P.nt; S.nt_rows = P.nt_rows;
    auto span = [](int& lo, int& hi, int v, bool first) { lo = first ? v : std::min(lo, v); hi = first ? v : std::max(hi, v); };
    int nrow = 0, ntile = 0;
    for (int sn = 0; sn < nn; ++sn) {
        if (P.lev_of[sn] < 0) continue;
        const int p = P.p[sn], rows = R(sn);
        const bool frow = p <= P.wave_p, brow = rows <= P.wave_r;
        S.fwd_row_nodes += frow; S.fwd_tile_nodes += !frow; S.bwd_row_nodes += brow; S.bwd_tile_nodes += !brow;
        S.fwd_row_bwd_tile_nodes += frow && !brow; S.fwd_tile_bwd_row_nodes += !frow && brow;
        S.odd_p_nodes += p & 1;
        if (frow && rows > P.levels[P.lev_of[sn]].fblock) ++S.multi_block_fwd_nodes;
        if (frow || brow) { span(S.row_p_min, S.row_p_max, p, nrow == 0); span(S.row_R_min, S.row_R_max, rows, nrow == 0); ++nrow; }
        if (!frow || !brow) { span(S.tile_p_min, S.tile_p_max, p, ntile == 0); span(S.tile_R_min, S.tile_R_max, rows, ntile == 0); ++ntile; }
    }
    S.sub_block = P.sub_block; S.wave_p = P.wave_p; S.wave_r = P.wave_r; S.max_sets = P.max_sets;
}

}  // namespace

SolvePlan plan_solve(const SolvePlanIn& in, const SolveKnobs& knobs) {
    SolvePlan plan;
    Planner pl(in, knobs, plan);
    pl.layout();
    pl.pull_lists();
    pl.fused_subtrees();
    pl.sub_lds();
    pl.branches();
    pl.group_subtrees();
    if (knobs.stats) pl.sub_stats();
    pl.levels();
    pl.dense_top();
    pl.packed_offsets();
    pl.streams();
    pl.bytes_and_nt();
    pl.summary();
    // internal assert: choose_cut_height budgets exactly this aggregate
    // (the LDS figures are per 3 columns; a 6-column solve needs twice as much; + the staged nodes)
    if (std::max(plan.sub_lds_bytes(plan.KS, true), plan.sub_lds_bytes(plan.KS, false)) > 160 * 1024)
        throw Error(ERR_STATE, "DirectSolver: internal error: fused subtrees exceed 160 KiB of LDS");
    return plan;
}

}  // namespace aa
