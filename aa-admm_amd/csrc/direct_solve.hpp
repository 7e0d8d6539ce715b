// GPU supernodal triangular solves against the host multifrontal factor (spd_direct.hpp).
//
// Replaces the reference's per-iteration LDLTSolver::solve (LinearSolver.hpp:87-90) and
// SPDSolver::solve (Geometry/SPDSolver.h:60-63) with a level-scheduled solve over the
// nested-dissection supernode tree. Per supernode s (pivots P, boundary rows B, |P| = p,
// |B| = nb) the host pre-multiplies the factor into one dense (p + nb) x p matrix
//        G_s = [ Linv_PP ; M ],   M = L_BP Linv_PP,
// so that both sweeps of a supernode are single matrix-vector products with no dependency
// inside the supernode:
//   forward   f = [b_P ; 0] + extend_add(children's update vectors)
//             y_P = Linv_PP f_P ,   u = f_B - M f_P        (rows of G_s . f_P)
//   backward  x_P = Linv_PP^T y_P - M^T x_B                (columns of G_s . [y_P ; -x_B])
// All supernodes of one tree height are independent, so a level is one launch whose work is
// cut into row tasks: small supernodes get a workgroup (thread per row, front vector in LDS),
// large ones are spread over many workgroups (wave per row, lanes across the row). Every
// product reads a coalesced copy of G_s (row-major for lane-across-row, column-major for
// thread-per-row); sums are in a fixed order (no atomics): deterministic. Three right-hand
// sides (x, y, z coordinates) are processed together -- or six: solve2() runs two independent
// solves in one pass over the factor (bit-identical to two solve() calls).
//
// What a solve launches is decided on the host by plan_solve() (solve_plan.hpp / .cpp: no HIP,
// tested on the CPU). build() reads the knobs once, plans, forms the factor values G_s, uploads
// the plan's arrays and packs the tiles; solve() replays the plan.
#pragma once
#include <cstdlib>
#include <vector>

#include "comm.hpp"
#include "common.hpp"
#include "elastic_kernels.hpp"
#include "solve_plan.hpp"
#include "spd_direct.hpp"

namespace aa {

class DirectSolver {
public:
    static constexpr int kTopRows = 2048;    // upper tree levels amalgamated into one dense root
    // the amalgamation budget in pivots for an n-unknown system (AA_TOP_ROWS overrides): 4096 below
    // 300 k unknowns, kTopRows above. Measured (same-box sweeps 2048 / 4096 / 6500 / 10000): C2
    // (25 k) 6 740 -> 8 173 it/s at 4096 (solve 91 -> 66 us: the top levels of a small tree are
    // latency, not bytes), C3 (101 k) 1 238 -> 1 300, C4 (211 k) flat, C5 (501 k) 167.9 -> 164.9
    // (the larger dense top costs more bytes than its levels cost latency)
    static int top_rows(int n) {
        const char* e = std::getenv("AA_TOP_ROWS");
        return e ? std::atoi(e) : (n < 300000 ? 4096 : kTopRows);
    }
    static constexpr int kPartTopRows = 4096;   // partitioned: a part's upper levels amalgamated (rows)
    static constexpr int kWaveP = 192;       // forward rows longer than this: wave per row
    static constexpr int kWaveR = 384;       // backward columns longer than this: wave per column

    // Partitioned (comm with size > 1): node_part[s] is the part of supernode s
    // (-1 = shared top separator, rows [top_beg, n)); only the supernodes of `my_part` and of
    // the top are stored and solved here, and the top rows of the forward result are summed
    // over the GPUs between the two sweeps.
    // max_sets = 2 sizes the workspaces and the fused subtrees' LDS budget for solve2().
    // wide: plan the layout (subtree cut, 256-wide split-K tiles) for two sets even when
    // max_sets = 1, so both solvers sum in the same order.
    // wave_p / wave_r: supernodes with p above wave_p (forward) / R above wave_r (backward) are
    // split-K tiled, the rest run as row tasks (defaults kWaveP / kWaveR; AA_SOLVE_WAVEP / _WAVER)
    void build(const SupernodalFactor& F, hipStream_t s, const std::vector<int>* node_part = nullptr, int my_part = -1,
               int top_beg = -1, Comm* comm = nullptr, int max_sets = 1, bool wide = false, int wave_p = kWaveP,
               int wave_r = kWaveR);
    // x (n x 3, stride 3 doubles) = A^-1 b ; b is read only. gate: skip when ctrl->done (or !reject).
    void solve(const double* b, double* x, const Ctrl* ctrl, int gate_reject, hipStream_t s);
    // x0 = A^-1 b0 and x1 = A^-1 b1 in one pass (needs build(..., max_sets = 2))
    void solve2(const double* b0, double* x0, const double* b1, double* x1, const Ctrl* ctrl, int gate_reject,
                hipStream_t s);
    int n() const { return pl_.n; }
    size_t nnz_L() const { return pl_.nnz_L; }
    double bytes_per_solve() const { return pl_.bytes; }
    double bytes_per_solve2() const { return pl_.bytes2; }
    int kernels_per_solve() const { return pl_.kernels; }

    // The device-facing records (Task, SubNode, FTile, ...) and the plan live in solve_plan.hpp
    using PlanSummary = aa::PlanSummary;
    static constexpr int kSubU = aa::kSubU, kSubX = aa::kSubX;
    const PlanSummary& plan_summary() const { return pl_.summary; }
    int default_branches = 1;   // set by the caller before build(); AA_SOLVE_BRANCHES overrides

private:
    struct SideStream {   // branch b's stream (b >= 1; branch 0 runs on the caller's) and its events
        hipStream_t st = nullptr;
        hipEvent_t fork_f = nullptr, join_f = nullptr, fork_b = nullptr, join_b = nullptr;
        void create(int dev) {
            if (st) return;
            AA_HIP(hipSetDevice(dev));
            AA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            for (hipEvent_t* e : {&fork_f, &join_f, &fork_b, &join_b}) AA_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        }
        ~SideStream() {
            for (hipEvent_t e : {fork_f, join_f, fork_b, join_b}) if (e) (void)hipEventDestroy(e);
            if (st) (void)hipStreamDestroy(st);
        }
    };
    SideStream side_[kMaxBranches];
    // what plan_solve() decided; solve_nr reads its scalars, levels, ranges and runs (the arrays
    // that only the device reads are dropped after the upload)
    SolvePlan pl_;
    Comm* comm_ = nullptr;
    void upload_factor(const SupernodalFactor& F, hipStream_t s);   // Gr, Gc and the packed tiles Gt
    template <int NR>
    void launch_ftiles(int w, int count, int first, const double* b0, const double* b1, int ext_off, const Ctrl* ctrl,
                       int gate_reject, hipStream_t s);
    template <int NR>
    void launch_btiles(int w, int count, int first, double* x0, double* x1, int ext_off, const Ctrl* ctrl,
                       int gate_reject, hipStream_t s);
    template <int NR>
    void launch_fstream(const Stream& S, const double* b0, const double* b1, const Ctrl* ctrl, int gate_reject,
                        hipStream_t s);
    template <int NR>
    void launch_bstream(const Stream& S, double* x0, double* x1, const Ctrl* ctrl, int gate_reject, hipStream_t s);
    template <int NR>
    void solve_nr(const double* b0, double* x0, const double* b1, double* x1, const Ctrl* ctrl, int gate_reject,
                  hipStream_t s);
    DevBuf<int> bnd_;
    DevBuf<long long> ell_;   // per front row, ell_w pull offsets into U (-1 = none)
    DevBuf<double> Gr_, Gc_, Y_, U_;
    // packed split-K tiles (AA_SOLVE_PACKED, default on): per tile one contiguous block, per wave
    // a sequential stream of 1-KB rows (64 lanes x 16 B): forward [wave][column pair][row][2],
    // backward [wave][row][column pair][2]; zero-padded to whole tiles
    DevBuf<double> Gt_;
    DevBuf<Task> tasks_;
    DevBuf<BTile> btiles_;
    DevBuf<BRed> breds_;
    DevBuf<FTile> ftiles_;
    DevBuf<FRed> freds_;
    DevBuf<int> fcnt_, bcnt_;   // tiles finished per reduction task (reset by the last tile)
    DevBuf<double> bpart_;
    // streamed runs (Stream in solve_plan.hpp)
    DevBuf<int> forder_, border_, bndx_;   // tile queues; per boundary entry its Xs_ row (-1: read x)
    DevBuf<int> sync_;   // [queue heads | forward counters (nn) | backward counters (nn)], zeroed per solve
    DevBuf<double> Xs_;   // backward: x rows of streamed supernodes, each supernode 128-B aligned
    // partitioned with a dense shared top: its front assembled locally and summed over the GPUs,
    // then each GPU runs the forward rows [top_r0, top_r1) and the backward products of those
    // rows (a partial x_top), and one more sum gives every GPU the whole x_top.
    DevBuf<Task> top_task_d_;
    DevBuf<double> top_f_, top_x_;   // [set][3 * top_p]: summed front, partial then summed x_top
    // fused bottom subtrees
    DevBuf<int> sub_xg_;                  // per kSubX subtree: its root's boundary (global x rows)
    DevBuf<SubNode> sub_nodes_;
    DevBuf<SubLevel> sub_levels_;
    DevBuf<SubTree> sub_trees_;
    DevBuf<int> sub_items_;   // (local node << 16 | row) per item
    DevBuf<long long> sub_items2_;   // backward segment items (local node << 40 | segment << 20 | column)
    int sub_timing_ = 0;              // AA_SUB_TIMING: solves left to time phase by phase
    DevBuf<long long> sub_clk_;       // [2][n_sub][64] s_memrealtime stamps
};

}  // namespace aa
