// Refit of a mesh obstacle to new vertex positions on the device (gfx950): the restatement of
// refit_mesh_obstacle_host (mesh_obstacle.hpp) the deforming-obstacle setter runs. Three passes:
//   k_refit_tris    one lane per leaf triangle: corners gathered from V', BvhTri written, unit
//                   normal and corner angles to scratch;
//   k_refit_pn      one lane per leaf triangle: the 21 pseudonormal doubles, every sum in the
//                   host's order (the vertex lists are sorted by caller triangle index);
//   k_refit_nodes   one wave per node over its contiguous triangle range, 12 running min / max
//                   reduced across the lanes; nodes of more than kRefitChunk triangles are cut into
//                   chunks (k_refit_chunks, one block each, partials to scratch) and finished by
//                   k_refit_big (one wave per such node). No atomics: min and max are exact, so the
//                   reduction shape does not show in the bits.
// Bound obstacles (vertices that follow solver nodes) run four kernels before those, all device-side:
//   k_bound_gather  one lane per vertex: the node's position from the step's start state, and per
//                   block whether a coordinate is not finite;
//   k_bound_check   one block per chunk of kBoundChunk caller triangles, one lane per triangle: the
//                   zero-area test, the chunk's vol6 partial (the pairwise tree of
//                   check_bound_refit) and the chunk's coordinate range;
//   k_bound_decide  one block: the causes in order, vol6 = the partials added in chunk order, the
//                   status word and the counts;
//   k_bound_commit  gated: the gathered vertices become the ones in force, the row's fp64 root box
//                   is the min / max of the chunk ranges (no atomics).
// The refit kernels take the status word as a trailing parameter pack and exit at once when it says
// skip; with the empty pack they are the kernels the vertex setter always launched.
// The arithmetic is the host's operation by operation, so nothing may be contracted into an FMA:
#pragma clang fp contract(off)
#include "mesh_refit.hpp"

#include <cfloat>
#include <cmath>

namespace aa {
namespace {

constexpr int kWave = 64;

// BvhBuilder::down / up: the cast, then one step where the cast went the wrong way
__device__ inline float round_down(double v) {
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, -INFINITY);
    return f;
}
__device__ inline float round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

// the gate of a bound refit: empty pack = never gated (no code)
__device__ __forceinline__ bool refit_gated() { return false; }
__device__ __forceinline__ bool refit_gated(const MeshBoundStatus* st) { return st->skip != 0; }

template <class... G>
__global__ __launch_bounds__(kBlock) void k_refit_tris(MeshRefitView m, G... gate) {
    if (refit_gated(gate...)) return;
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= m.nf) return;
    BvhTri tr;
    for (int a = 0; a < 3; ++a) {
        const double* P = m.V + 3 * (size_t)m.leaf_vid[3 * (size_t)k + a];
        for (int d = 0; d < 3; ++d) tr.v[3 * a + d] = P[d];
    }
    m.tris[k] = tr;
    double fa[6];
    mesh_detail::tri_normal_angles(tr.v, fa, fa + 3);
    for (int c = 0; c < 6; ++c) m.fa[6 * (size_t)k + c] = fa[c];
}

template <class... G>
__global__ __launch_bounds__(kBlock) void k_refit_pn(MeshRefitView m, G... gate) {
    if (refit_gated(gate...)) return;
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= m.nf) return;
    double* P = m.pn + (size_t)kPnStride * k;
    const int corner_slot[3] = {0, 1, 3}, edge_slot[3] = {2, 5, 4};   // a b c; ab bc ca
    for (int a = 0; a < 3; ++a) {
        const int p = m.leaf_vid[3 * (size_t)k + a];
        double s[3] = {0.0, 0.0, 0.0};
        for (int j = m.vt_ptr[p]; j < m.vt_ptr[p + 1]; ++j) {
            const int e = m.vt[j];
            const double* f = m.fa + 6 * (size_t)(e >> 2);
            const double ang = f[3 + (e & 3)];
            for (int d = 0; d < 3; ++d) s[d] += ang * f[d];
        }
        const double* f0 = m.fa + 6 * (size_t)m.edge_tris[6 * (size_t)k + 2 * a];
        const double* f1 = m.fa + 6 * (size_t)m.edge_tris[6 * (size_t)k + 2 * a + 1];
        for (int d = 0; d < 3; ++d) {
            P[3 * corner_slot[a] + d] = s[d];
            P[3 * edge_slot[a] + d] = (0.0 + f0[d]) + f1[d];
        }
    }
    for (int d = 0; d < 3; ++d) P[18 + d] = m.fa[6 * (size_t)k + d];
}

// running min (r[0..5]) and max (r[6..11]) of x, y, z and of the three axis projections
struct Range12 {
    double r[12];
    __device__ void init() {
        for (int c = 0; c < 6; ++c) { r[c] = DBL_MAX; r[6 + c] = -DBL_MAX; }
    }
    __device__ void take(int c, double lo, double hi) {
        r[c] = lo < r[c] ? lo : r[c];
        r[6 + c] = hi > r[6 + c] ? hi : r[6 + c];
    }
    __device__ void add_triangle(const BvhTri& t, const float (*ax)[3]) {
        for (int a = 0; a < 3; ++a) {
            const double* P = t.v + 3 * a;
            for (int d = 0; d < 3; ++d) take(d, P[d], P[d]);
            for (int x = 0; x < 3; ++x) {
                const double s = ((double)ax[x][0] * P[0] + (double)ax[x][1] * P[1]) + (double)ax[x][2] * P[2];
                take(3 + x, s, s);
            }
        }
    }
    __device__ void wave_reduce() {   // every lane of the wave calls it; every lane ends with the result
        for (int off = kWave / 2; off > 0; off >>= 1)
            for (int c = 0; c < 6; ++c) take(c, __shfl_xor(r[c], off, kWave), __shfl_xor(r[6 + c], off, kWave));
    }
};

__device__ inline void load_axes(const BvhNode& nd, float (*ax)[3]) {
    for (int d = 0; d < 3; ++d) { ax[0][d] = nd.nrm[d]; ax[1][d] = nd.t1[d]; ax[2][d] = nd.t2[d]; }
}

// one lane writes the node's bounds; a range stored as (-FLT_MAX, FLT_MAX) stays so
__device__ inline void store_bounds(BvhNode& nd, const Range12& g) {
    for (int d = 0; d < 3; ++d) { nd.lo[d] = round_down(g.r[d]); nd.hi[d] = round_up(g.r[6 + d]); }
    if (!(nd.dlo == -FLT_MAX && nd.dhi == FLT_MAX)) { nd.dlo = round_down(g.r[3]); nd.dhi = round_up(g.r[9]); }
    if (!(nd.t1lo == -FLT_MAX && nd.t1hi == FLT_MAX)) { nd.t1lo = round_down(g.r[4]); nd.t1hi = round_up(g.r[10]); }
    if (!(nd.t2lo == -FLT_MAX && nd.t2hi == FLT_MAX)) { nd.t2lo = round_down(g.r[5]); nd.t2hi = round_up(g.r[11]); }
}

template <class... G>
__global__ __launch_bounds__(kBlock) void k_refit_nodes(MeshRefitView m, G... gate) {
    if (refit_gated(gate...)) return;
    const int i = (blockIdx.x * kBlock + threadIdx.x) / kWave;   // wave-uniform
    const int lane = threadIdx.x % kWave;
    if (i >= m.n_nodes) return;
    const int cnt = m.node_cnt[i];
    if (cnt > kRefitChunk) return;   // k_refit_chunks + k_refit_big
    const int beg = m.node_beg[i];
    float ax[3][3];
    load_axes(m.nodes[i], ax);
    Range12 g;
    g.init();
    for (int k = lane; k < cnt; k += kWave) g.add_triangle(m.tris[beg + k], ax);
    g.wave_reduce();
    if (lane == 0) store_bounds(m.nodes[i], g);
}

template <class... G>
__global__ __launch_bounds__(kBlock) void k_refit_chunks(MeshRefitView m, G... gate) {
    if (refit_gated(gate...)) return;
    __shared__ double part[kBlock / kWave][12];
    const int c = blockIdx.x;   // grid = n_chunks
    const int beg = m.chunk_beg[c], cnt = m.chunk_cnt[c];
    float ax[3][3];
    load_axes(m.nodes[m.big_node[m.chunk_big[c]]], ax);
    Range12 g;
    g.init();
    for (int k = threadIdx.x; k < cnt; k += kBlock) g.add_triangle(m.tris[beg + k], ax);
    g.wave_reduce();
    if (threadIdx.x % kWave == 0)
        for (int q = 0; q < 12; ++q) part[threadIdx.x / kWave][q] = g.r[q];
    __syncthreads();
    if (threadIdx.x < 12) {
        const int q = threadIdx.x;
        double v = part[0][q];
        for (int w = 1; w < kBlock / kWave; ++w) v = q < 6 ? (part[w][q] < v ? part[w][q] : v) : (part[w][q] > v ? part[w][q] : v);
        m.partial[12 * (size_t)c + q] = v;
    }
}

template <class... G>
__global__ __launch_bounds__(kBlock) void k_refit_big(MeshRefitView m, G... gate) {
    if (refit_gated(gate...)) return;
    const int b = (blockIdx.x * kBlock + threadIdx.x) / kWave;   // wave-uniform
    const int lane = threadIdx.x % kWave;
    if (b >= m.n_big) return;
    Range12 g;
    g.init();
    for (int c = m.big_chunk_ptr[b] + lane; c < m.big_chunk_ptr[b + 1]; c += kWave)
        for (int q = 0; q < 6; ++q) g.take(q, m.partial[12 * (size_t)c + q], m.partial[12 * (size_t)c + 6 + q]);
    g.wave_reduce();
    if (lane == 0) store_bounds(m.nodes[m.big_node[b]], g);
}

// ---------------------------------------------------------------------------------------------
// bound obstacles
static_assert(kBoundChunk == kBlock, "k_bound_check: one lane per triangle of a chunk");

__global__ __launch_bounds__(kBlock) void k_bound_gather(MeshBoundView b) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int bad = 0;
    if (i < b.nv) {
        const double* P = b.xs + 3 * (size_t)b.bind[i];
        for (int d = 0; d < 3; ++d) {
            const double v = P[d];
            b.cand[3 * (size_t)i + d] = v;
            if (!isfinite(v)) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) b.bad[blockIdx.x] = bad;
}

__global__ __launch_bounds__(kBlock) void k_bound_check(MeshBoundView b) {
    __shared__ double p[kBoundChunk];
    __shared__ double rng[kBlock / kWave][6];
    const int c = blockIdx.x, j = threadIdx.x;
    const int t = c * kBoundChunk + j;
    double term = 0.0, r[6] = {DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX};
    int zero = 0;
    if (t < b.nf) {
        const double *A = b.cand + 3 * (size_t)b.F[3 * (size_t)t], *B = b.cand + 3 * (size_t)b.F[3 * (size_t)t + 1],
                     *C = b.cand + 3 * (size_t)b.F[3 * (size_t)t + 2];
        zero = mesh_detail::bound_tri_term(A, B, C, term) ? 1 : 0;
        const double* corner[3] = {A, B, C};
        for (int a = 0; a < 3; ++a)
            for (int d = 0; d < 3; ++d) {
                const double v = corner[a][d];
                r[d] = v < r[d] ? v : r[d];
                r[3 + d] = v > r[3 + d] ? v : r[3 + d];
            }
    }
    p[j] = term;
    for (int off = kWave / 2; off > 0; off >>= 1)
        for (int d = 0; d < 3; ++d) {
            const double lo = __shfl_xor(r[d], off, kWave), hi = __shfl_xor(r[3 + d], off, kWave);
            r[d] = lo < r[d] ? lo : r[d];
            r[3 + d] = hi > r[3 + d] ? hi : r[3 + d];
        }
    if (j % kWave == 0)
        for (int q = 0; q < 6; ++q) rng[j / kWave][q] = r[q];
    zero = __syncthreads_or(zero);   // also the barrier after the writes of p and rng
    for (int w = kBoundChunk / 2; w > 0; w >>= 1) {   // check_bound_refit's tree
        if (j < w) p[j] = p[j] + p[j + w];
        __syncthreads();
    }
    if (j == 0) { b.vol[c] = p[0]; b.zero[c] = zero; }
    if (j < 6) {
        double v = rng[0][j];
        for (int w = 1; w < kBlock / kWave; ++w) v = j < 3 ? (rng[w][j] < v ? rng[w][j] : v) : (rng[w][j] > v ? rng[w][j] : v);
        b.box[6 * (size_t)c + j] = v;
    }
}

__global__ __launch_bounds__(kBlock) void k_bound_decide(MeshBoundView b) {   // one block
    __shared__ double sh[kBlock];
    const int j = threadIdx.x;
    int bad = 0, zero = 0;
    for (int i = j; i < b.n_vblocks; i += kBlock) bad |= b.bad[i];
    for (int i = j; i < b.n_chunks; i += kBlock) zero |= b.zero[i];
    bad = __syncthreads_or(bad);
    zero = __syncthreads_or(zero);
    double vol6 = 0.0;   // lane 0's: the partials in chunk order, staged through LDS a block at a time
    for (int base = 0; base < b.n_chunks; base += kBlock) {
        sh[j] = base + j < b.n_chunks ? b.vol[base + j] : 0.0;
        __syncthreads();
        if (j == 0) {
            const int m = b.n_chunks - base < kBlock ? b.n_chunks - base : kBlock;
            for (int q = 0; q < m; ++q) vol6 = vol6 + sh[q];
        }
        __syncthreads();
    }
    if (j == 0) {
        const int cause = bad ? BOUND_NONFINITE : (zero ? BOUND_ZERO_AREA : (!(vol6 > 0.0) ? BOUND_VOLUME : BOUND_OK));
        MeshBoundStatus& st = *b.st;
        st.cause = cause;
        st.skip = cause != BOUND_OK;
        st.vol6 = vol6;
        if (cause != BOUND_OK) { st.skipped += 1; st.last_cause = cause; }
        else st.refits += 1;
    }
}

__global__ __launch_bounds__(kBlock) void k_bound_commit(MeshBoundView b) {
    if (b.st->skip) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < b.nv)
        for (int d = 0; d < 3; ++d) b.verts[3 * (size_t)i + d] = b.cand[3 * (size_t)i + d];
    if (blockIdx.x == 0 && threadIdx.x < 6) {   // the row's root box: the exact range of the referenced vertices
        const int q = threadIdx.x;
        double v = b.box[q];
        for (int c = 1; c < b.n_chunks; ++c) {
            const double w = b.box[6 * (size_t)c + q];
            v = q < 3 ? (w < v ? w : v) : (w > v ? w : v);
        }
        if (q < 3) b.row->lo[q] = v;
        else b.row->hi[q - 3] = v;
    }
}

}  // namespace

namespace {
template <class... G>
void launch_mesh_refit_g(const MeshRefitView& v, hipStream_t s, G... gate) {
    hipLaunchKernelGGL((k_refit_tris<G...>), dim3(blocks_for(v.nf)), dim3(kBlock), 0, s, v, gate...);
    AA_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_refit_pn<G...>), dim3(blocks_for(v.nf)), dim3(kBlock), 0, s, v, gate...);
    AA_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_refit_nodes<G...>), dim3(blocks_for((long long)v.n_nodes * kWave)), dim3(kBlock), 0, s, v, gate...);
    AA_CHECK_LAUNCH();
    if (v.n_big > 0) {
        hipLaunchKernelGGL((k_refit_chunks<G...>), dim3(v.n_chunks), dim3(kBlock), 0, s, v, gate...);
        AA_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_refit_big<G...>), dim3(blocks_for((long long)v.n_big * kWave)), dim3(kBlock), 0, s, v, gate...);
        AA_CHECK_LAUNCH();
    }
}
}  // namespace

void launch_mesh_refit(const MeshRefitView& v, hipStream_t s, const MeshBoundStatus* gate) {
    if (v.nf <= 0 || v.n_nodes <= 0) return;
    if (gate) launch_mesh_refit_g(v, s, gate);
    else launch_mesh_refit_g(v, s);
}

void launch_mesh_bound(const MeshBoundView& b, hipStream_t s) {
    if (b.nv <= 0 || b.nf <= 0) return;
    hipLaunchKernelGGL(k_bound_gather, dim3(b.n_vblocks), dim3(kBlock), 0, s, b);
    AA_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bound_check, dim3(b.n_chunks), dim3(kBlock), 0, s, b);
    AA_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bound_decide, dim3(1), dim3(kBlock), 0, s, b);
    AA_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bound_commit, dim3(b.n_vblocks), dim3(kBlock), 0, s, b);
    AA_CHECK_LAUNCH();
}

}  // namespace aa
