// Device refit of a mesh obstacle to new vertex positions (deforming obstacles): the kernels of
// mesh_refit.hip reproduce refit_mesh_obstacle_host (mesh_obstacle.hpp, where the semantics are
// stated) on the uploaded tables, in place -- every buffer keeps its address, so a captured step
// graph stays valid.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "mesh_obstacle.hpp"

namespace aa {

// What the kernels read and write (device pointers)
struct MeshRefitView {
    const double* V;    // [nv][3] the new vertices
    int nf, n_nodes;
    BvhNode* nodes;
    BvhTri* tris;
    double* pn;
    const int *leaf_vid, *node_beg, *node_cnt, *vt_ptr, *vt, *edge_tris;
    double* fa;         // scratch [nf][6]: unit normal and corner angles of every leaf triangle
    int n_big, n_chunks;
    const int *big_node, *big_chunk_ptr, *chunk_big, *chunk_beg, *chunk_cnt;
    double* partial;    // scratch [n_chunks][12]: min then max of x, y, z, n, t1, t2 over a chunk
};

// Bound obstacles (a mesh whose vertices follow solver nodes): the device-side outcome of the check
// a bound refit runs on the gathered vertices (check_bound_refit, mesh_obstacle.hpp). `skip` is the
// word every later kernel of that refit is gated on; the counts run since binding.
struct MeshBoundStatus {
    int skip;         // this step's refit is not taken
    int cause;        // BOUND_* of this step's check
    int refits, skipped, last_cause;   // taken / skipped refits, the cause of the last skipped one
    int pad_;
    double vol6;      // the chunked sum of this step's check
};

// What the gather, check and root-box kernels read and write (device pointers)
struct MeshBoundView {
    const double* xs;     // [n][3] the step's start state, internal numbering
    const int* bind;      // [nv] internal node of vertex i
    int nv, nf;
    const int* F;         // [nf][3] the caller's triangles
    double* cand;         // [nv][3] the gathered vertices
    double* verts;        // [nv][3] the vertices in force (what the refit kernels read)
    int n_vblocks, n_chunks;
    int* bad;             // [n_vblocks] a non-finite coordinate among the block's vertices
    int* zero;            // [n_chunks]  a triangle of the chunk with !(n . n > 0)
    double* vol;          // [n_chunks]  the chunk's vol6 partial
    double* box;          // [n_chunks][6] min then max of x, y, z over the chunk's corners
    MeshBoundStatus* st;
    MeshObsDev* row;      // the mesh's row of the table: lo / hi rewritten after a passed check
};

// Enqueues the refit on s: triangles (+ normals and angles), pseudonormal table, node bounds.
// gate given: every kernel exits at once when gate->skip is set (the forms without it are the
// ones the vertex setter launches).
void launch_mesh_refit(const MeshRefitView& v, hipStream_t s, const MeshBoundStatus* gate = nullptr);
// Enqueues gather + check + decision + (gated) commit of the vertices in force and the root box.
void launch_mesh_bound(const MeshBoundView& b, hipStream_t s);

// Device copies of a mesh's MeshRefitTables, the vertex staging buffer and the scratch arrays
struct MeshRefitBuffers {
    DevBuf<int> leaf_vid, node_beg, node_cnt, vt_ptr, vt, edge_tris, big_node, big_chunk_ptr, chunk_big, chunk_beg, chunk_cnt;
    DevBuf<double> verts, fa, partial;
    // a carrying mesh (aa_elastic_set_mesh_obstacle_carry): the vertices in force during the last
    // step in which the friction pass ran, refreshed from verts on the device after the pass
    DevBuf<double> verts_prev;
    PinnedBuf<double> stage;
    int nv = 0, nf = 0;
    // bound obstacles: the caller's triangles, the binding and the check's partials (bind())
    DevBuf<int> F, bind_nodes, bad, zero;
    DevBuf<double> cand, vol, box;
    void upload(const MeshRefitTables& T, hipStream_t s) {
        nv = T.nv; nf = (int)T.F.size() / 3;
        leaf_vid.upload(T.leaf_vid, s); node_beg.upload(T.node_beg, s); node_cnt.upload(T.node_cnt, s);
        vt_ptr.upload(T.vt_ptr, s); vt.upload(T.vt, s); edge_tris.upload(T.edge_tris, s);
        big_node.upload(T.big_node, s); big_chunk_ptr.upload(T.big_chunk_ptr, s); chunk_big.upload(T.chunk_big, s);
        chunk_beg.upload(T.chunk_beg, s); chunk_cnt.upload(T.chunk_cnt, s);
        verts.alloc(3 * (size_t)nv);
        fa.alloc(6 * (size_t)nf);
        partial.alloc(12 * std::max<size_t>(T.chunk_big.size(), 1));
        AA_HIP(hipStreamSynchronize(s));   // T may be a temporary of the caller's
    }
    MeshRefitView view(BvhNode* nodes, int n_nodes, BvhTri* tris, double* pn) const {
        MeshRefitView v{};
        v.V = verts.p; v.nf = nf; v.n_nodes = n_nodes; v.nodes = nodes; v.tris = tris; v.pn = pn;
        v.leaf_vid = leaf_vid.p; v.node_beg = node_beg.p; v.node_cnt = node_cnt.p; v.vt_ptr = vt_ptr.p; v.vt = vt.p;
        v.edge_tris = edge_tris.p; v.fa = fa.p;
        v.n_big = (int)big_node.n; v.n_chunks = (int)chunk_big.n;
        v.big_node = big_node.p; v.big_chunk_ptr = big_chunk_ptr.p; v.chunk_big = chunk_big.p; v.chunk_beg = chunk_beg.p;
        v.chunk_cnt = chunk_cnt.p; v.partial = partial.p;
        return v;
    }
    // V staged with one copy, then the kernels; nothing is waited for
    void refit(const double* V, BvhNode* nodes, int n_nodes, BvhTri* tris, double* pn, hipStream_t s) {
        double* h = stage.get(3 * (size_t)nv);
        std::copy(V, V + 3 * (size_t)nv, h);
        AA_HIP(hipMemcpyAsync(verts.p, h, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice, s));
        launch_mesh_refit(view(nodes, n_nodes, tris, pn), s);
    }
    // Bound obstacles. bind(): vertex i follows internal node nodes_int[i]; verts_now = the vertices
    // in force (the device copy the refit kernels read is made current).
    void bind(const MeshRefitTables& T, const int* nodes_int, const double* verts_now, hipStream_t s) {
        F.upload(T.F, s);
        bind_nodes.upload(nodes_int, (size_t)nv, s);
        cand.alloc(3 * (size_t)nv);
        bad.alloc((size_t)blocks_for(nv));
        const size_t nc = (size_t)blocks_for(nf, kBoundChunk);
        zero.alloc(nc); vol.alloc(nc); box.alloc(6 * nc);
        AA_HIP(hipMemcpyAsync(verts.p, verts_now, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice, s));
        AA_HIP(hipStreamSynchronize(s));   // both sources may be temporaries of the caller's
    }
    // gather from xs, check, and -- gated on st->skip -- the vertices in force, the row's root box and
    // the refit; all on s, nothing copied from or to the host, nothing waited for
    void bound_refit(const double* xs, MeshObsDev* row, MeshBoundStatus* st, BvhNode* nodes, int n_nodes, BvhTri* tris,
                     double* pn, hipStream_t s) {
        MeshBoundView b{};
        b.xs = xs; b.bind = bind_nodes.p; b.nv = nv; b.nf = nf; b.F = F.p; b.cand = cand.p; b.verts = verts.p;
        b.n_vblocks = (int)bad.n; b.n_chunks = (int)zero.n;
        b.bad = bad.p; b.zero = zero.p; b.vol = vol.p; b.box = box.p; b.st = st; b.row = row;
        launch_mesh_bound(b, s);
        launch_mesh_refit(view(nodes, n_nodes, tris, pn), s, st);
    }
};

}  // namespace aa
