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

// Enqueues the refit on s: triangles (+ normals and angles), pseudonormal table, node bounds.
void launch_mesh_refit(const MeshRefitView& v, hipStream_t s);

// Device copies of a mesh's MeshRefitTables, the vertex staging buffer and the scratch arrays
struct MeshRefitBuffers {
    DevBuf<int> leaf_vid, node_beg, node_cnt, vt_ptr, vt, edge_tris, big_node, big_chunk_ptr, chunk_big, chunk_beg, chunk_cnt;
    DevBuf<double> verts, fa, partial;
    PinnedBuf<double> stage;
    int nv = 0, nf = 0;
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
    // V staged with one copy, then the kernels; nothing is waited for
    void refit(const double* V, BvhNode* nodes, int n_nodes, BvhTri* tris, double* pn, hipStream_t s) {
        double* h = stage.get(3 * (size_t)nv);
        std::copy(V, V + 3 * (size_t)nv, h);
        AA_HIP(hipMemcpyAsync(verts.p, h, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice, s));
        MeshRefitView v{};
        v.V = verts.p; v.nf = nf; v.n_nodes = n_nodes; v.nodes = nodes; v.tris = tris; v.pn = pn;
        v.leaf_vid = leaf_vid.p; v.node_beg = node_beg.p; v.node_cnt = node_cnt.p; v.vt_ptr = vt_ptr.p; v.vt = vt.p;
        v.edge_tris = edge_tris.p; v.fa = fa.p;
        v.n_big = (int)big_node.n; v.n_chunks = (int)chunk_big.n;
        v.big_node = big_node.p; v.big_chunk_ptr = big_chunk_ptr.p; v.chunk_big = chunk_big.p; v.chunk_beg = chunk_beg.p;
        v.chunk_cnt = chunk_cnt.p; v.partial = partial.p;
        launch_mesh_refit(v, s);
    }
};

}  // namespace aa
