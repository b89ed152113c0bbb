// ptrt_accel.hip.h -- the acceleration-structure half of the C ABI: the caller's reference-shaped meshes and TLAS re-laid-out
// and uploaded (ptrt_upload_geometry, ptrt_update_instances), instances moved (ptrt_set_instance_transforms*, ptrt_set_instance_poses_device, ptrt_refit_tlas,
// ptrt_reorder_tlas), meshes moved (ptrt_update_vertices, ptrt_update_triangles, ptrt_refit, ptrt_build_bvh) and the read-backs.
// Included by ptrt_capi.hip behind struct ptrt_ctx and the helpers every entry point shares (fail, HIP_TRY, upload, ctx_live,
// set_device); the state only this file touches is in ptrt_accel_state.hip.h.  Nothing here is on the frame path.
#pragma once

namespace {

// ---- mesh records (pt::MESH_REC_F4 float4 each): {bmin, root}, {bmax, flags}, inverse 3 rows, world 3 rows, normal 3 rows ----
constexpr int REC_INSTANCE = 1;    // flags bit 0: the mesh is an instance with its own transform
constexpr int REC_SHADOW_SKIP = 2; // flags bit 1: skipped by shadow rays (from the materials: transmission > 0.5)

int rec_flags(const float4 *rec) {
    int flags;
    std::memcpy(&flags, &rec[1].w, 4);
    return flags;
}
void set_rec_flag(float4 *rec, int bit, bool on) {
    const int flags = rec_flags(rec);
    rec[1].w = as_f(on ? flags | bit : flags & ~bit);
}
// the nine matrix rows, from a ptrt_mesh_desc or a ptrt_instance_xform (row-major 4x4 each; the normal matrix's fourth column is not kept)
void set_rec_xform(float4 *rec, const float *inverse, const float *world, const float *normal) {
    for (int r = 0; r < 3; ++r) {
        rec[2 + r] = f4(inverse[r * 4], inverse[r * 4 + 1], inverse[r * 4 + 2], inverse[r * 4 + 3]);
        rec[5 + r] = f4(world[r * 4], world[r * 4 + 1], world[r * 4 + 2], world[r * 4 + 3]);
        rec[8 + r] = f4(normal[r * 4], normal[r * 4 + 1], normal[r * 4 + 2], 0.0f);
    }
}

// Inverse of a 3x3 matrix by cofactors in double precision, with the Frobenius norms of both: what the instances' first-pass
// boxes are made of (upload_instance_pretests, host_inst_c2; DESIGN.md 3.16 rests on the two agreeing with
// pt::instance_pretest).  !ok (singular or non-finite): I and the norms are zero.
struct Inv3 {
    bool ok;
    double I[3][3], nA, nI;
};
Inv3 inverse3(const double A[3][3]) {
    Inv3 v{};
    const double co[3][3] = {{A[1][1] * A[2][2] - A[1][2] * A[2][1], A[0][2] * A[2][1] - A[0][1] * A[2][2], A[0][1] * A[1][2] - A[0][2] * A[1][1]},
                             {A[1][2] * A[2][0] - A[1][0] * A[2][2], A[0][0] * A[2][2] - A[0][2] * A[2][0], A[0][2] * A[1][0] - A[0][0] * A[1][2]},
                             {A[1][0] * A[2][1] - A[1][1] * A[2][0], A[0][1] * A[2][0] - A[0][0] * A[2][1], A[0][0] * A[1][1] - A[0][1] * A[1][0]}};
    const double det = A[0][0] * co[0][0] - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + A[0][2] * co[2][0];
    v.ok = std::isfinite(det) && std::fabs(det) > 1e-30;
    if (!v.ok)
        return v;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            v.I[r][k] = co[r][k] / det;
            v.nA += A[r][k] * A[r][k];
            v.nI += v.I[r][k] * v.I[r][k];
        }
    v.nA = std::sqrt(v.nA);
    v.nI = std::sqrt(v.nI);
    return v;
}

// ---- scene re-layout ---------------------------------------------------------------
struct Relayout {
    std::vector<float4> nodes; // child-pair inner nodes
    std::vector<int2> leaves;
    std::vector<float4> tris;
    int max_depth = 0;
};

// Converts one reference-shaped tree (pre-order 40-byte nodes) into child-pair nodes.
// `emit_leaf(start,count)` returns the leaf id for a leaf node.  Returns the root
// reference, or INT32_MIN on malformed input.
// `dst` codes say where a subtree's box is stored, for the GPU refit: >= 0 -> inner node
// (code >> 1), side (code & 1); < 0 -> root box of tree `root_dst`.  `emit_leaf(start,count,dst)`.
// `node_dst`/`node_depth` (optional) receive that code and the depth of every inner node created.
template <class EmitLeaf>
int convert_tree(const ptrt_bvh_node *in, int n_in, std::vector<float4> &out_nodes, EmitLeaf emit_leaf, int &max_depth,
                 std::string &why, int root_dst = -1, std::vector<int> *node_dst = nullptr,
                 std::vector<int> *node_depth = nullptr, std::vector<int> *old_dst = nullptr) {
    struct Item {
        int old_idx, new_idx, depth;
    };
    if (n_in <= 0) {
        why = "empty node array";
        return INT32_MIN;
    }
    std::vector<char> seen((size_t)n_in, 0);
    auto ref_of = [&](int old_idx, int depth, int dst, std::vector<Item> &work) -> int {
        if (old_idx < 0)
            return ~emit_leaf(0, 0, dst); // absent child: an empty leaf behind an unhittable box
        if (old_idx >= n_in) {
            why = "child index out of range";
            return INT32_MIN;
        }
        if (seen[old_idx]) {
            why = "node referenced twice (not a tree)";
            return INT32_MIN;
        }
        seen[old_idx] = 1;
        if (old_dst)
            (*old_dst)[old_idx] = dst; // (`old_dst`, optional, sized n_in: the code of every input node that was reached)
        const ptrt_bvh_node &N = in[old_idx];
        if (N.count > 0)
            return ~emit_leaf(N.start, N.count, dst);
        const int ni = (int)(out_nodes.size() / 4);
        out_nodes.resize(out_nodes.size() + 4);
        if (node_dst) {
            node_dst->resize((size_t)ni + 1, 0);
            node_depth->resize((size_t)ni + 1, 0);
            (*node_dst)[ni] = dst;
            (*node_depth)[ni] = depth + 1;
        }
        work.push_back({old_idx, ni, depth + 1});
        return ni;
    };
    std::vector<Item> work;
    const int root = ref_of(0, 0, root_dst, work);
    if (root == INT32_MIN)
        return root;
    // Numbering: the top TOP_LEVELS levels in level order (a tree's first 2^TOP_LEVELS - 1 inner nodes are then its top
    // levels, which the LDS-staged variant of the trace kernel copies per workgroup), everything below depth first.
    size_t head = 0;
    while (head < work.size()) {
        Item it;
        if (work[head].depth <= pt::TOP_LEVELS) { // (a node of the top levels: first in, first out)
            it = work[head];
            ++head;
        } else {
            it = work.back();
            work.pop_back();
        }
        if (it.depth > max_depth)
            max_depth = it.depth;
        const ptrt_bvh_node &N = in[it.old_idx];
        const int L = ref_of(N.left, it.depth, it.new_idx * 2, work);
        if (L == INT32_MIN)
            return L;
        const int R = ref_of(N.right, it.depth, it.new_idx * 2 + 1, work);
        if (R == INT32_MIN)
            return R;
        const float BIG = 1e30f;
        ptrt_vec3 lmin{BIG, BIG, BIG}, lmax{-BIG, -BIG, -BIG}, rmin = lmin, rmax = lmax;
        if (N.left >= 0) {
            lmin = in[N.left].bmin;
            lmax = in[N.left].bmax;
        }
        if (N.right >= 0) {
            rmin = in[N.right].bmin;
            rmax = in[N.right].bmax;
        }
        float4 *o = &out_nodes[(size_t)it.new_idx * 4];
        o[0] = f4(lmin.x, lmin.y, lmin.z, lmax.x);
        o[1] = f4(lmax.y, lmax.z, rmin.x, rmin.y);
        o[2] = f4(rmin.z, rmax.x, rmax.y, rmax.z);
        o[3] = f4(as_f(L), as_f(R), 0.0f, 0.0f);
    }
    return root;
}

// words of ptrt_ctx::d_tlas_sort for n meshes (layout there)
size_t tlas_sort_words(int n) {
    const size_t n_waves = ((size_t)n + pt::RS_WAVE_KEYS - 1) / pt::RS_WAVE_KEYS;
    return 8 + (size_t)n * 3 + (n > pt::TLAS_WIDE ? (size_t)n * 4 + n_waves * 256 * 2 : 0);
}

// TLAS part of an upload: converts the reference-shaped TLAS, uploads it and derives what the launch needs of it
int upload_tlas(ptrt_ctx *c, int mesh_count, const ptrt_bvh_node *tlas_nodes, int tlas_node_count,
                const int32_t *tlas_mesh_indices, int tlas_index_count, bool dry_run) {
    std::vector<float4> tnodes;
    std::vector<int2> tleaves;
    bool bad = false;
    std::string why;
    std::vector<int> leaf_dst, node_dst, node_depth, in_dst((size_t)tlas_node_count, INT32_MIN);
    auto emit_tleaf = [&](int start, int count, int dst) -> int {
        if (count > 0 && (start < 0 || start + count > tlas_index_count)) {
            bad = true;
            count = 0;
        }
        tleaves.push_back(make_int2(start < 0 ? 0 : start, count));
        leaf_dst.push_back(dst);
        return (int)tleaves.size() - 1;
    };
    int tdepth = 0;
    const int troot = convert_tree(tlas_nodes, tlas_node_count, tnodes, emit_tleaf, tdepth, why, -1, &node_dst, &node_depth, &in_dst);
    if (troot == INT32_MIN || bad)
        return fail(c, PTRT_E_INVALID, "malformed TLAS (%s)", bad ? "leaf range out of bounds" : why.c_str());
    if (tdepth > 23)
        return fail(c, PTRT_E_INVALID, "TLAS is %d levels deep; needs <= 23", tdepth);
    std::vector<int> tids(tlas_mesh_indices, tlas_mesh_indices + tlas_index_count);
    for (int id : tids)
        if (id < 0 || id >= mesh_count)
            return fail(c, PTRT_E_INVALID, "TLAS references mesh %d of %d", id, mesh_count);
    if (dry_run)
        return PTRT_OK;
    std::vector<float4> rootbox = {f4(tlas_nodes[0].bmin.x, tlas_nodes[0].bmin.y, tlas_nodes[0].bmin.z, 0.0f),
                                   f4(tlas_nodes[0].bmax.x, tlas_nodes[0].bmax.y, tlas_nodes[0].bmax.z, 0.0f)};
    if (int rc = upload(c, c->d_tlas_root_box, rootbox))
        return rc;
    if (int rc = upload(c, c->d_tlas_nodes, tnodes))
        return rc;
    if (int rc = upload(c, c->d_tlas_leaves, tleaves))
        return rc;
    if (int rc = upload(c, c->d_tlas_mesh_ids, tids))
        return rc;
    dfree(c->d_tlas_heads);
    HIP_TRY(c, hipMalloc((void **)&c->d_tlas_heads, (size_t)tlas_index_count * pt::TLAS_HEAD_F4 * sizeof(float4)));
    // what a refit over this topology needs (pt_tlas.hip.h): the dst codes and the inner nodes level by level, deepest first
    const int n_inner = (int)node_dst.size();
    std::vector<int> refit(leaf_dst);
    refit.insert(refit.end(), node_dst.begin(), node_dst.end());
    c->tlas_levels = pt::TopLevels{};
    for (int d = tdepth; d >= 1; --d) {
        const int begin = (int)refit.size() - (int)leaf_dst.size() - n_inner;
        for (int n = 0; n < n_inner; ++n)
            if (node_depth[n] == d)
                refit.push_back(n);
        const int count = (int)refit.size() - (int)leaf_dst.size() - n_inner - begin;
        if (count > 0) { // (tdepth <= 23 was checked above: at most 23 entries of 24)
            c->tlas_levels.begin[c->tlas_levels.n] = begin;
            c->tlas_levels.count[c->tlas_levels.n] = count;
            ++c->tlas_levels.n;
        }
    }
    if (int rc = upload(c, c->d_tlas_refit, refit))
        return rc;
    if (tlas_index_count > c->tlas_world_cap) {
        dfree(c->d_tlas_world);
        c->tlas_world_cap = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_tlas_world, (size_t)tlas_index_count * 2 * sizeof(float4)));
        c->tlas_world_cap = tlas_index_count;
    }
    // a re-order (ptrt_reorder_tlas) deals MESHES to the indices: it needs every mesh exactly once
    std::vector<char> seen((size_t)mesh_count, 0);
    bool perm = tlas_index_count == mesh_count;
    for (int id : tids) {
        perm = perm && !seen[(size_t)id];
        seen[(size_t)id] = 1;
    }
    c->tlas_is_perm = perm;
    if (perm && troot >= 0 && mesh_count > c->tlas_sort_cap) {
        dfree(c->d_tlas_sort);
        c->tlas_sort_cap = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_tlas_sort, tlas_sort_words(mesh_count) * sizeof(uint32_t)));
        c->tlas_sort_cap = mesh_count;
        const uint32_t cb[8] = {~0u, ~0u, ~0u, 0u, 0u, 0u, 0u, 0u}; // min words all-ones, max words zero; every re-order leaves them so
        HIP_TRY(c, hipMemcpy(c->d_tlas_sort, cb, sizeof cb, hipMemcpyHostToDevice));
    }
    c->n_tlas_leaves = (int)leaf_dst.size();
    c->n_tlas_inner = n_inner;
    c->h_tlas_in.assign(tlas_nodes, tlas_nodes + tlas_node_count);
    c->h_tlas_in_dst = in_dst;
    c->n_tlas_index = tlas_index_count;
    c->tlas_root_ref = troot;
    c->tlas_single_leaf = troot < 0;
    c->pair_meshes = troot < 0 ? tleaves[~troot].y : 0;
    c->tlas_depth = tdepth;
    c->tlas_max_leaf = 0;
    for (const int2 &lf : tleaves)
        if (lf.y > c->tlas_max_leaf)
            c->tlas_max_leaf = lf.y;
    return PTRT_OK;
}

// ---- dynamic geometry: launch sequences, replayed as hipGraphs ------------------------------
// A refit is ~16 and a rebuild ~35 microsecond-sized launches; issued one by one they cost more in
// launch gaps than in work.  The sequences are fixed for a given upload (same kernels, grids and
// arena pointers), so each is captured once on a private stream and replayed with one
// hipGraphLaunch on the context's stream, under one key of ptrt_ctx::graphs per sequence.
enum GraphKey {
    GK_REFIT = -1,        // ptrt_refit
    GK_REFIT_TLAS = -2,   // ptrt_refit_tlas
    GK_REORDER_TLAS = -3, // ptrt_reorder_tlas: the re-order with its refit
    // m >= 0: ptrt_build_bvh of mesh m, with its refit
};
void drop_graph(ptrt_ctx *c, int key) {
    auto it = c->graphs.find(key);
    if (it != c->graphs.end()) {
        (void)hipGraphExecDestroy(it->second);
        c->graphs.erase(it);
    }
}
void drop_graphs(ptrt_ctx *c) {
    for (auto &kv : c->graphs)
        (void)hipGraphExecDestroy(kv.second);
    c->graphs.clear();
}

// the two-level records follow the canonical nodes (after an upload, a refit, a rebuild)
void enqueue_expand_nodes(ptrt_ctx *c, hipStream_t st) {
    if (PT_TWO_LEVEL && c->n_nodes > 0 && c->d_nodes2)
        hipLaunchKernelGGL(pt::expand_nodes_kernel, dim3((c->n_nodes * 3 + 255) / 256), dim3(256), 0, st, c->d_nodes, c->d_nodes2,
                           c->n_nodes);
}

int enqueue_refit(ptrt_ctx *c, hipStream_t st) {
    const int B = 256;
    if (c->n_slots > 0)
        hipLaunchKernelGGL(pt::repack_tris_kernel, dim3((c->n_slots + B - 1) / B), dim3(B), 0, st, c->d_verts,
                           c->d_slot_face, c->d_tris, c->n_slots);
    if (c->n_leaves > 0)
        hipLaunchKernelGGL(pt::refit_leaves_kernel, dim3((c->n_leaves + B - 1) / B), dim3(B), 0, st, c->d_verts,
                           c->d_slot_face, c->d_leaves, c->d_leaf_dst, c->d_nodes, c->d_mesh_recs, c->n_leaves);
    // wide levels: one launch each, deepest first; the narrow levels near the root (<= 2048 nodes) and the
    // TLAS root box: one workgroup, barriers between levels (a tiny launch costs ~4.6 us whatever it does)
    pt::TopLevels T{};
    bool top = false;
    for (int d = (int)c->level_offset.size() - 1; d >= 1; --d) { // depth d nodes: [offset[d-1], offset[d])
        const int begin = c->level_offset[d - 1], count = c->level_offset[d] - begin;
        if (count <= 0)
            continue;
        top = top || count <= 2048; // counts shrink towards the root; once narrow, the rest goes to the fused kernel
        if (top) {
            T.begin[T.n] = begin;
            T.count[T.n] = count;
            ++T.n;
        } else {
            hipLaunchKernelGGL(pt::refit_level_kernel, dim3((count + B - 1) / B), dim3(B), 0, st, c->d_level_nodes + begin,
                               count, c->d_node_dst, c->d_nodes, c->d_mesh_recs);
        }
    }
    hipLaunchKernelGGL(pt::refit_top_levels_kernel, dim3(1), dim3(1024), 0, st, c->d_level_nodes, T, c->d_node_dst,
                       c->d_nodes, c->d_mesh_recs, c->d_tlas_leaves, c->d_tlas_mesh_ids, c->tlas_root_ref,
                       c->d_tlas_root_box);
    enqueue_expand_nodes(c, st);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// stable sort of n (30-bit Morton code, value) pairs in keys[0] / vals[0]; `hist`: n_waves * 256 counts, then as many
// positions.  Returns which of the two buffers holds the result.
int enqueue_radix_sort(hipStream_t st, uint32_t *const keys[2], uint32_t *const vals[2], uint32_t *hist, int n) {
    const int n_waves = (n + pt::RS_WAVE_KEYS - 1) / pt::RS_WAVE_KEYS;
    const int wg = (n_waves + pt::RS_BLOCK / 64 - 1) / (pt::RS_BLOCK / 64);
    int cur = 0;
    for (int shift = 0; shift < 32; shift += 8) { // the top pass only sees bits 24..29 of the 30-bit code
        hipLaunchKernelGGL(pt::rs_hist_kernel, dim3(wg), dim3(pt::RS_BLOCK), 0, st, keys[cur], n, shift, hist, n_waves);
        uint32_t *positions = hist + (size_t)n_waves * 256;
        hipLaunchKernelGGL(pt::rs_scan_kernel, dim3(1), dim3(1024), 0, st, hist, positions, n_waves);
        hipLaunchKernelGGL(pt::rs_scatter_kernel, dim3(wg), dim3(pt::RS_BLOCK), 0, st, keys[cur], vals[cur], n, shift, positions,
                           n_waves, keys[cur ^ 1], vals[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}

int enqueue_build(ptrt_ctx *c, int mesh, hipStream_t st) {
    const int n = c->mesh_face_count[mesh];
    const int B = 256, G = (n + B - 1) / B;
    const int4 *faces = c->d_face_src + c->mesh_face_base[mesh];
    hipLaunchKernelGGL(pt::centroid_bounds_kernel, dim3(G < 128 ? G : 128), dim3(B), 0, st, c->d_verts, faces, n,
                       c->build.d_centroids, c->build.d_cbounds);
    hipLaunchKernelGGL(pt::morton_kernel, dim3(G), dim3(B), 0, st, c->build.d_centroids, c->build.d_cbounds, n, c->build.d_sort_keys[0],
                       c->build.d_sort_vals[0]);
    const int cur = enqueue_radix_sort(st, c->build.d_sort_keys, c->build.d_sort_vals, c->build.d_sort_hist, n);
    hipLaunchKernelGGL(pt::apply_order_kernel, dim3(G), dim3(B), 0, st, c->build.d_sort_vals[cur], c->d_slot_pos, faces,
                       c->d_slot_face, c->mesh_slot_base[mesh], n, c->build.d_cbounds);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

template <class F> int run_graphed(ptrt_ctx *c, int key, F enqueue) {
    if (!c->use_graphs)
        return enqueue(c->stream);
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
        if (!c->capture_stream)
            HIP_TRY(c, hipStreamCreateWithFlags(&c->capture_stream, hipStreamNonBlocking));
        HIP_TRY(c, hipStreamBeginCapture(c->capture_stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue(c->capture_stream);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(c->capture_stream, &g);
        if (rc != PTRT_OK || e != hipSuccess || !g) {
            if (g)
                (void)hipGraphDestroy(g);
            return rc != PTRT_OK ? rc : fail(c, PTRT_E_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ei != hipSuccess)
            return fail(c, PTRT_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
        it = c->graphs.emplace(key, exec).first;
    }
    HIP_TRY(c, hipGraphLaunch(it->second, c->stream));
    return PTRT_OK;
}

void free_scene(ptrt_ctx *c) {
    drop_graphs(c); // captured launch sequences hold arena pointers
    dfree(c->d_mesh_recs);
    dfree(c->d_nodes);
    dfree(c->d_nodes2);
    dfree(c->d_tris);
    dfree(c->d_tri_frames);
    c->tri_frames_ok = false;
    dfree(c->d_tlas_nodes);
    dfree(c->d_leaves);
    dfree(c->d_tlas_leaves);
    dfree(c->d_tlas_mesh_ids);
    dfree(c->d_tlas_heads);
    dfree(c->d_inst_pre);
    dfree(c->d_tlas_root_box);
    dfree(c->d_tlas_refit);
    dfree(c->d_tlas_world);
    c->tlas_world_cap = 0;
    dfree(c->d_tlas_sort);
    c->tlas_sort_cap = 0;
    dfree(c->d_verts);
    dfree(c->d_slot_face);
    dfree(c->d_leaf_dst);
    dfree(c->d_node_dst);
    dfree(c->d_level_nodes);
    dfree(c->d_face_src);
    dfree(c->d_slot_pos);
    c->build.release();
}

// ... and what outlives a re-upload: the staging areas of the moving parts and the capture stream.  ptrt_destroy calls both.
void free_staging(ptrt_ctx *c) {
    c->verts.release();
    c->xf.release();
    if (c->capture_stream)
        (void)hipStreamDestroy(c->capture_stream);
    c->capture_stream = nullptr;
}

// After ptrt_set_instance_transforms_device the has_transform bits and matrices of h_mesh_recs lag the device's.  The paths
// that write host flag words back (push_mesh_recs) fetch them first; they synchronise anyway.  Until then the host copy is
// only used conservatively: any_transform is held true, and host_inst_c2 over old matrices gives a cap under which
// pt::instance_pretest hands an instance it does not cover the infinite box.
int sync_host_xforms(ptrt_ctx *c) {
    if (!c->xf_host_stale)
        return PTRT_OK;
    std::vector<float4> dev((size_t)c->n_meshes * pt::MESH_REC_F4);
    HIP_TRY(c, hipMemcpyAsync(dev.data(), c->d_mesh_recs, dev.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->any_transform = false;
    for (int m = 0; m < c->n_meshes; ++m) {
        float4 *rec = &c->h_mesh_recs[(size_t)m * pt::MESH_REC_F4];
        const float4 *d = &dev[(size_t)m * pt::MESH_REC_F4];
        const bool inst = (rec_flags(d) & REC_INSTANCE) != 0;
        set_rec_flag(rec, REC_INSTANCE, inst);
        std::memcpy(&rec[2], &d[2], 9 * sizeof(float4));
        c->any_transform = c->any_transform || inst;
    }
    c->xf_host_stale = false;
    return PTRT_OK;
}

// flags bit1 (skipped by shadow rays) comes from the materials; re-applied on either upload.
// `full` re-sends the whole records (geometry upload); otherwise only the flag words are patched
// so that boxes moved by ptrt_refit on the device are not overwritten with stale host copies.
int push_mesh_recs(ptrt_ctx *c, bool full) {
    if (!full)
        if (int rc = sync_host_xforms(c))
            return rc;
    for (int m = 0; m < c->n_meshes; ++m)
        set_rec_flag(&c->h_mesh_recs[(size_t)m * pt::MESH_REC_F4], REC_SHADOW_SKIP,
                     m < (int)c->h_shadow_skip.size() && c->h_shadow_skip[m]);
    if (full)
        return upload(c, c->d_mesh_recs, c->h_mesh_recs);
    for (int m = 0; m < c->n_meshes; ++m)
        HIP_TRY(c, hipMemcpyAsync(&c->d_mesh_recs[(size_t)m * pt::MESH_REC_F4 + 1].w,
                                  &c->h_mesh_recs[(size_t)m * pt::MESH_REC_F4 + 1].w, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

// What the entry points that need an uploaded scene open with, in this order: a live context and (where the caller passes it)
// well-formed arguments, else PTRT_E_INVALID; geometry, else PTRT_E_NOT_READY.  ctx_live marks the context as touched, so it
// runs even when `args_ok` is false.  set_device and the checks against the scene (a mesh index, a count) follow at the call site.
int enter_geometry(ptrt_ctx *c, const char *who, bool args_ok = true) {
    if (!ctx_live(c) || !args_ok)
        return fail(c, PTRT_E_INVALID, "%s: bad %s", who, args_ok ? "context" : "argument");
    if (!c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "%s: geometry not uploaded", who);
    return PTRT_OK;
}

// World-space first-pass boxes of the instances (PMODE 3, pt_render.hip.h build_pairs_general).  The reference tests an
// instance's root box in ITS space with the ray transformed by the instance's inverse matrix A|t (intersection.cuh:
// 284-297, 454-463).  Here a ray is first tested against a world-space box W that contains every ray that test can
// accept: W = the bounding box of A^-1 (corner - t) over the eight corners of the local box, in double precision (A is
// whatever matrix the caller supplies -- the reference's own mat4::inverse is not always the true inverse, which is
// why W comes from A and not from the world matrix), grown by C1 + C2 |o|_1 with
//     C1 = Kc (|A^-1|_F (|t| + |box|) + |W|_inf) + 1e-6,   C2 = Kc (|A^-1|_F |A|_F + 1),   Kc = 1e-4.
// The fp32 local test can accept a ray only if the exact ray passes within eta <= ~32 * 2^-24 (|A o + t| + |box|) of
// the local box (five roundings per slab term on quantities of that size, plus the rounded direction over a path of
// that length); mapped back to world space that is at most |A^-1|_2 eta <= 2e-6 |A^-1|_F (|A|_F |o| + |t| + |box|), and
// the world test's own rounding is below 1e-6 (|W| + |o|): Kc leaves a factor of 50.  A singular or non-finite A gets
// an infinite box (every ray is a candidate: the local test decides, as before).
// `device_recs`: the mesh records as the DEVICE holds them now (root boxes moved by ptrt_refit / ptrt_build_bvh included); when
// given, the local boxes come from there and the descriptors' BVH arrays are not read.
int upload_instance_pretests(ptrt_ctx *c, const ptrt_mesh_desc *meshes, int mesh_count, const float4 *device_recs = nullptr) {
    std::vector<float4> pre((size_t)mesh_count * 2, f4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f));
    double c2max = 0.0;
    const double Kc = 1e-4, BIG = 3.0e38;
    for (int m = 0; m < mesh_count; ++m) {
        const ptrt_mesh_desc &M = meshes[m];
        pre[(size_t)m * 2 + 1] = f4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f);
        if (!M.has_transform || (!device_recs && (!M.nodes || M.node_count <= 0)))
            continue;
        double A[3][3], t[3];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k)
                A[r][k] = M.inverse[r * 4 + k];
            t[r] = M.inverse[r * 4 + 3];
        }
        const Inv3 inv = inverse3(A);
        bool ok = inv.ok;
        double lo[3], hi[3];
        if (device_recs) {
            const float4 a = device_recs[(size_t)m * pt::MESH_REC_F4], b = device_recs[(size_t)m * pt::MESH_REC_F4 + 1];
            lo[0] = a.x, lo[1] = a.y, lo[2] = a.z, hi[0] = b.x, hi[1] = b.y, hi[2] = b.z;
        } else {
            const ptrt_bvh_node &rn = M.nodes[0];
            lo[0] = rn.bmin.x, lo[1] = rn.bmin.y, lo[2] = rn.bmin.z, hi[0] = rn.bmax.x, hi[1] = rn.bmax.y, hi[2] = rn.bmax.z;
        }
        double wmin[3] = {BIG, BIG, BIG}, wmax[3] = {-BIG, -BIG, -BIG}, boxn = 0.0, tn = 0.0, wn = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double a = std::fmax(std::fabs(lo[k]), std::fabs(hi[k]));
            boxn += a * a;
            tn += t[k] * t[k];
        }
        boxn = std::sqrt(boxn);
        tn = std::sqrt(tn);
        for (int corner = 0; ok && corner < 8; ++corner) {
            const double p[3] = {((corner & 1) ? hi[0] : lo[0]) - t[0], ((corner & 2) ? hi[1] : lo[1]) - t[1],
                                 ((corner & 4) ? hi[2] : lo[2]) - t[2]};
            for (int r = 0; r < 3; ++r) {
                const double x = inv.I[r][0] * p[0] + inv.I[r][1] * p[1] + inv.I[r][2] * p[2];
                ok = ok && std::isfinite(x);
                wmin[r] = std::fmin(wmin[r], x);
                wmax[r] = std::fmax(wmax[r], x);
                wn = std::fmax(wn, std::fabs(x));
            }
        }
        const double C1 = Kc * (inv.nI * (tn + boxn) + wn) + 1e-6, C2 = Kc * (inv.nI * inv.nA + 1.0);
        ok = ok && std::isfinite(C1) && std::isfinite(C2) && C1 < 1e30 && C2 < 1e3 && wn < 1e30;
        if (!ok)
            continue; // infinite box: every ray is a candidate
        c2max = std::fmax(c2max, C2);
        // (outward rounding of the double results to float: one more ulp-sized step than the margin needs)
        pre[(size_t)m * 2] = f4(std::nextafterf((float)(wmin[0] - C1), -INFINITY), std::nextafterf((float)(wmin[1] - C1), -INFINITY),
                                 std::nextafterf((float)(wmin[2] - C1), -INFINITY), 0.0f);
        pre[(size_t)m * 2 + 1] = f4(std::nextafterf((float)(wmax[0] + C1), INFINITY), std::nextafterf((float)(wmax[1] + C1), INFINITY),
                                     std::nextafterf((float)(wmax[2] + C1), INFINITY), 0.0f);
    }
    c->inst_c2 = std::nextafterf((float)c2max, INFINITY);
    c->inst_c2_all = false;
    if (int rc = upload(c, c->d_inst_pre, pre))
        return rc;
    c->inst_pre_ok = true;
    return PTRT_OK;
}

// The growth factor C2 of the instances' first-pass boxes (see upload_instance_pretests) from the matrices alone, over
// EVERY mesh of h_mesh_recs that is an instance: an upper bound of what the device derives per instance in
// pt::instance_pretest, which gives an instance whose own factor exceeds the value handed to it the infinite box.
float host_inst_c2(const ptrt_ctx *c) {
    double c2max = 0.0;
    for (int m = 0; m < c->n_meshes; ++m) {
        const float4 *rec = &c->h_mesh_recs[(size_t)m * pt::MESH_REC_F4];
        if (!(rec_flags(rec) & REC_INSTANCE))
            continue;
        const double A[3][3] = {{rec[2].x, rec[2].y, rec[2].z}, {rec[3].x, rec[3].y, rec[3].z}, {rec[4].x, rec[4].y, rec[4].z}};
        const Inv3 inv = inverse3(A);
        if (!inv.ok)
            continue; // (infinite box on the device too)
        const double C2 = 1e-4 * (inv.nI * inv.nA + 1.0) * (1.0 + 1e-9); // (a hair above the device's own rounding)
        if (std::isfinite(C2) && C2 < 1e3)
            c2max = std::fmax(c2max, C2);
    }
    return std::nextafterf((float)c2max, INFINITY);
}

// inst_c2 is an argument of the TLAS refit: a captured launch sequence holds the old value
void set_inst_c2(ptrt_ctx *c, float v) {
    if (v != c->inst_c2 || !c->inst_c2_all) {
        drop_graph(c, GK_REFIT_TLAS);
        drop_graph(c, GK_REORDER_TLAS);
    }
    c->inst_c2 = v;
    c->inst_c2_all = true;
}

int enqueue_refit_tlas(ptrt_ctx *c, hipStream_t st) {
    const int *leaf_dst = c->d_tlas_refit, *node_dst = leaf_dst + c->n_tlas_leaves, *level_nodes = node_dst + c->n_tlas_inner;
    const bool wide = c->n_tlas_index > pt::TLAS_WIDE;
    if (wide)
        hipLaunchKernelGGL(pt::tlas_world_boxes_kernel, dim3((c->n_tlas_index + pt::TLAS_BLOCK - 1) / pt::TLAS_BLOCK),
                           dim3(pt::TLAS_BLOCK), 0, st, c->d_mesh_recs, c->d_tlas_mesh_ids, c->n_tlas_index, c->inst_c2,
                           c->d_tlas_world, c->d_inst_pre);
    hipLaunchKernelGGL(pt::refit_tlas_kernel, dim3(1), dim3(pt::TLAS_BLOCK), 0, st, c->d_mesh_recs, c->d_tlas_mesh_ids,
                       c->n_tlas_index, c->d_tlas_leaves, leaf_dst, c->n_tlas_leaves, level_nodes, c->tlas_levels, node_dst,
                       c->inst_c2, wide ? 0 : 1, c->d_tlas_world, c->d_inst_pre, c->d_tlas_nodes, c->d_tlas_root_box);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// the meshes re-dealt to the TLAS indices in Morton order of their world boxes' centres (pt_tlas.hip.h), then the refit.
// Invariant of the wide path: cbounds hold {all-ones x 3, zero x 3} between calls -- upload_tlas seeds them with the
// allocation and tlas_take_order_kernel, the last launch of every sequence, restores them (as apply_order_kernel does for a
// BLAS build).  The launches are enqueued or captured as one sequence, so a sequence that starts also ends.
int enqueue_reorder_tlas(ptrt_ctx *c, hipStream_t st) {
    const int n = c->n_meshes;
    uint32_t *cbounds = c->d_tlas_sort, *rest = cbounds + 8;
    float *centres = reinterpret_cast<float *>(rest);
    if (n <= pt::TLAS_WIDE) {
        hipLaunchKernelGGL(pt::reorder_tlas_kernel, dim3(1), dim3(pt::TLAS_BLOCK), 0, st, c->d_mesh_recs, n, centres,
                           c->d_tlas_mesh_ids);
    } else {
        uint32_t *keys[2] = {rest + (size_t)n * 3, rest + (size_t)n * 4}, *vals[2] = {rest + (size_t)n * 5, rest + (size_t)n * 6};
        uint32_t *hist = rest + (size_t)n * 7;
        const int B = 256, G = (n + B - 1) / B;
        hipLaunchKernelGGL(pt::tlas_centres_kernel, dim3(G < 128 ? G : 128), dim3(B), 0, st, c->d_mesh_recs, n, centres, cbounds);
        hipLaunchKernelGGL(pt::morton_kernel, dim3(G), dim3(B), 0, st, centres, cbounds, n, keys[0], vals[0]);
        const int cur = enqueue_radix_sort(st, keys, vals, hist, n);
        hipLaunchKernelGGL(pt::tlas_take_order_kernel, dim3(G), dim3(B), 0, st, vals[cur], n, c->d_tlas_mesh_ids, cbounds);
    }
    return enqueue_refit_tlas(c, st);
}

// What ptrt_refit_tlas and ptrt_reorder_tlas share: ctx_live orders the next frame (pipelined or split) behind the stream and
// has the TLAS-leaf-order heads gathered again; the launches go out on the stream, replayed as a hipGraph under use_graphs;
// the instances' first-pass boxes are fresh behind them.  A single-leaf TLAS has nothing to re-deal (and its kernels' mesh
// order must stay): the re-order is the refit there.
int refit_tlas_entry(ptrt_ctx *c, const char *who, bool reorder) {
    if (int rc = enter_geometry(c, who))
        return rc;
    const bool deal = reorder && !c->tlas_single_leaf;
    if (deal && !c->tlas_is_perm)
        return fail(c, PTRT_E_INVALID, "%s: the uploaded TLAS indices are not a permutation of the %d meshes", who, c->n_meshes);
    if (int rc = set_device(c))
        return rc;
    if (!c->inst_c2_all)
        set_inst_c2(c, host_inst_c2(c));
    c->plain_leaf_ok = c->tri_frames_ok = false; // (the device rewrites the TLAS root box)
    if (int rc = deal ? run_graphed(c, GK_REORDER_TLAS, [c](hipStream_t st) { return enqueue_reorder_tlas(c, st); })
                      : run_graphed(c, GK_REFIT_TLAS, [c](hipStream_t st) { return enqueue_refit_tlas(c, st); }))
        return rc;
    c->inst_pre_ok = true;
    ++(reorder ? c->tlas_reorders : c->tlas_refits);
    return PTRT_OK;
}

// What ptrt_upload_geometry gathers over the meshes before anything of the old scene is freed.
struct FlatScene {
    Relayout R;
    std::vector<float4> recs; // the mesh records
    bool all_leaf = true;
    // refit bookkeeping
    std::vector<float> verts;
    std::vector<int4> slot_face;
    std::vector<int> leaf_dst, node_dst, node_depth, vert_base, vert_count;
    // rebuild bookkeeping
    std::vector<int4> face_src;
    std::vector<int> slot_pos, face_base, face_count, slot_base, slot_count;
    std::vector<unsigned char> rebuildable, is_soup;
    // read-back bookkeeping (ptrt_read_bvh): per mesh, where the device keeps the box of each input node
    std::vector<std::vector<int>> in_dst;
};

// Validates mesh `m` and appends it to `S`: vertices, faces, the BVH as child-pair nodes with its leaves' triangle packets,
// the bookkeeping of the GPU refit and rebuild, the mesh record.
int flatten_mesh(ptrt_ctx *c, int m, const ptrt_mesh_desc &M, FlatScene &S) {
    if (!M.verts || !M.faces || !M.nodes || !M.prim_indices || M.node_count <= 0 || M.face_count <= 0 ||
        M.vert_count <= 0 || M.prim_count <= 0)
        return fail(c, PTRT_E_INVALID, "mesh %d: missing arrays (a mesh needs vertices, faces and a built BVH)", m);
    for (int f = 0; f < M.face_count; ++f) {
        const ptrt_tri &t = M.faces[f];
        if (t.v0 < 0 || t.v1 < 0 || t.v2 < 0 || t.v0 >= M.vert_count || t.v1 >= M.vert_count ||
            t.v2 >= M.vert_count)
            return fail(c, PTRT_E_INVALID, "mesh %d: face %d references a vertex out of range", m, f);
    }
    const int vb = (int)(S.verts.size() / 3), slot_base = (int)S.slot_face.size();
    S.vert_base.push_back(vb);
    S.vert_count.push_back(M.vert_count);
    S.verts.insert(S.verts.end(), &M.verts[0].x, &M.verts[0].x + (size_t)M.vert_count * 3);
    S.face_base.push_back((int)S.face_src.size());
    S.face_count.push_back(M.face_count);
    S.slot_base.push_back(slot_base);
    bool soup = M.vert_count == 3 * M.face_count;
    for (int f = 0; f < M.face_count; ++f) {
        const ptrt_tri &t = M.faces[f];
        S.face_src.push_back(make_int4(vb + t.v0, vb + t.v1, vb + t.v2, f));
        soup = soup && t.v0 == 3 * f && t.v1 == 3 * f + 1 && t.v2 == 3 * f + 2;
    }
    S.is_soup.push_back(soup ? 1 : 0);
    bool bad = false;
    auto emit_leaf = [&](int start, int count, int dst) -> int {
        const int id = (int)S.R.leaves.size();
        if (count > 0 && (start < 0 || start + count > M.prim_count)) {
            bad = true;
            count = 0;
        }
        S.R.leaves.push_back(make_int2((int)(S.R.tris.size() / 3), count));
        S.leaf_dst.push_back(dst);
        for (int i = 0; i < count; ++i) {
            const int fidx = M.prim_indices[start + i];
            S.slot_pos.push_back(start + i);
            if (fidx < 0 || fidx >= M.face_count) {
                bad = true;
                S.R.tris.insert(S.R.tris.end(), 3, f4(0, 0, 0, 0));
                S.slot_face.push_back(make_int4(vb, vb, vb, 0));
                continue;
            }
            const ptrt_tri &t = M.faces[fidx];
            S.slot_face.push_back(make_int4(vb + t.v0, vb + t.v1, vb + t.v2, fidx));
            const ptrt_vec3 &a = M.verts[t.v0], &b = M.verts[t.v1], &d = M.verts[t.v2];
            // e1 = v1 - v0, e2 = v2 - v0: the same fp32 subtractions the reference performs per
            // test (intersection.cuh:224-225), done once here
            S.R.tris.push_back(f4(a.x, a.y, a.z, 0.0f)); // (the w words: tri_normals_kernel, in ptrt_upload_geometry)
            S.R.tris.push_back(f4(b.x - a.x, b.y - a.y, b.z - a.z, 0.0f));
            S.R.tris.push_back(f4(d.x - a.x, d.y - a.y, d.z - a.z, 0.0f));
        }
        return id;
    };
    int depth = 0;
    std::string why;
    S.in_dst.emplace_back((size_t)M.node_count, INT32_MIN);
    const int root = convert_tree(M.nodes, M.node_count, S.R.nodes, emit_leaf, depth, why, -(m + 1), &S.node_dst, &S.node_depth,
                                  &S.in_dst.back());
    if (root == INT32_MIN || bad)
        return fail(c, PTRT_E_INVALID, "mesh %d: malformed BVH (%s)", m, bad ? "leaf range out of bounds" : why.c_str());
    if (depth > 23)
        return fail(c, PTRT_E_INVALID,
                    "mesh %d: BVH is %d levels deep; the traversal stack (24 entries, as in the reference) needs <= 23",
                    m, depth);
    if (depth > S.R.max_depth)
        S.R.max_depth = depth;
    if (root >= 0)
        S.all_leaf = false;
    // a GPU rebuild permutes faces over prim positions: every position 0..face_count-1 must be a leaf slot once
    const int slot_count = (int)S.slot_face.size() - slot_base;
    S.slot_count.push_back(slot_count);
    bool once = slot_count == M.face_count && M.prim_count == M.face_count;
    if (once) {
        std::vector<unsigned char> used((size_t)M.face_count, 0);
        for (int s = slot_base; s < slot_base + slot_count; ++s) {
            once = once && !used[(size_t)S.slot_pos[s]];
            used[(size_t)S.slot_pos[s]] = 1;
        }
    }
    S.rebuildable.push_back(once ? 1 : 0);
    S.recs.resize(S.recs.size() + pt::MESH_REC_F4, f4(0, 0, 0, 0));
    float4 *rec = &S.recs[S.recs.size() - pt::MESH_REC_F4];
    const ptrt_bvh_node &rn = M.nodes[0];
    rec[0] = f4(rn.bmin.x, rn.bmin.y, rn.bmin.z, as_f(root));
    rec[1] = f4(rn.bmax.x, rn.bmax.y, rn.bmax.z, as_f(M.has_transform ? REC_INSTANCE : 0));
    set_rec_xform(rec, M.inverse, M.world, M.normal);
    return PTRT_OK;
}

// Inner nodes grouped by depth for the level-by-level refit: level_nodes[level_offset[d - 1] .. level_offset[d]) are the
// nodes at depth d (node_depth: 1 = a root; 0 = not an inner node).
struct LevelOrder {
    std::vector<int> level_offset, level_nodes;
};
LevelOrder level_order(const std::vector<int> &node_depth) {
    LevelOrder o;
    int maxd = 0;
    for (int d : node_depth)
        if (d > maxd)
            maxd = d;
    o.level_offset.assign((size_t)maxd + 1, 0);
    for (int d : node_depth)
        if (d >= 1)
            o.level_offset[d]++;
    // level_offset[d] currently holds the count of depth d (index 0 unused); prefix-sum it
    int run = 0;
    for (int d = 1; d <= maxd; ++d) {
        const int n = o.level_offset[d];
        o.level_offset[d - 1] = run;
        run += n;
    }
    o.level_offset[maxd] = run;
    std::vector<int> fill(o.level_offset);
    o.level_nodes.resize((size_t)run);
    for (int i = 0; i < (int)node_depth.size(); ++i)
        if (node_depth[i] >= 1)
            o.level_nodes[(size_t)fill[node_depth[i] - 1]++] = i;
    return o;
}

} // namespace

extern "C" {

int ptrt_upload_geometry(ptrt_ctx *c, const ptrt_mesh_desc *meshes, int mesh_count, const ptrt_bvh_node *tlas_nodes,
                         int tlas_node_count, const int32_t *tlas_mesh_indices, int tlas_index_count) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_upload_geometry: bad context");
    if (!meshes || mesh_count <= 0 || !tlas_nodes || tlas_node_count <= 0 || !tlas_mesh_indices ||
        tlas_index_count <= 0)
        return fail(c, PTRT_E_INVALID, "ptrt_upload_geometry: empty scene");
    if (int rc = set_device(c))
        return rc;

    FlatScene S;
    for (int m = 0; m < mesh_count; ++m)
        if (int rc = flatten_mesh(c, m, meshes[m], S))
            return rc;
    // TLAS: validated before anything of the old scene is freed, uploaded below
    if (int rc = upload_tlas(c, mesh_count, tlas_nodes, tlas_node_count, tlas_mesh_indices, tlas_index_count, true))
        return rc;

    free_scene(c);
    // nothing of the old scene is left: until the last upload below has succeeded the context has no geometry,
    // so a failure in between (hipMalloc) leaves it answering PTRT_E_NOT_READY instead of launching on NULL arenas
    c->have_geometry = false;
    c->n_slots = c->n_leaves = 0;
    c->n_meshes = mesh_count;
    c->h_mesh_recs = S.recs;
    c->xf_host_stale = false;
    if (int rc = push_mesh_recs(c, true))
        return rc;
    const Relayout &R = S.R;
    S.node_dst.resize(R.nodes.size() / 4, 0);
    S.node_depth.resize(R.nodes.size() / 4, 0);
    const LevelOrder levels = level_order(S.node_depth);
    int failed = PTRT_OK; // the first failing upload's code; the uploads behind it are skipped
    auto put = [&](auto *&dst, const auto &src) { failed = failed ? failed : upload(c, dst, src); };
    put(c->d_verts, S.verts);
    put(c->d_slot_face, S.slot_face);
    put(c->d_leaf_dst, S.leaf_dst);
    put(c->d_node_dst, S.node_dst);
    put(c->d_level_nodes, levels.level_nodes);
    put(c->d_face_src, S.face_src);
    put(c->d_slot_pos, S.slot_pos);
    put(c->d_nodes, R.nodes);
    if (failed)
        return failed;
    c->level_offset = levels.level_offset;
    c->mesh_face_base = S.face_base;
    c->mesh_face_count = S.face_count;
    c->mesh_slot_base = S.slot_base;
    c->mesh_slot_count = S.slot_count;
    c->mesh_rebuildable = S.rebuildable;
    c->mesh_is_soup = S.is_soup;
    c->mesh_vert_base = S.vert_base;
    c->mesh_vert_count = S.vert_count;
    c->h_mesh_in.resize((size_t)mesh_count);
    for (int m = 0; m < mesh_count; ++m)
        c->h_mesh_in[(size_t)m].assign(meshes[m].nodes, meshes[m].nodes + meshes[m].node_count);
    c->h_mesh_in_dst = std::move(S.in_dst);
    c->n_slots = (int)S.slot_face.size();
    c->n_leaves = (int)R.leaves.size();
    c->n_nodes = (int)(R.nodes.size() / 4);
    dfree(c->d_nodes2);
    if (PT_TWO_LEVEL) { // (a build whose queue modes read two-level records: measured, no gain -- DESIGN.md 3.11)
        HIP_TRY(c, hipMalloc((void **)&c->d_nodes2, (size_t)(c->n_nodes > 0 ? c->n_nodes : 1) * pt::NODE2_F4 * sizeof(float4)));
        enqueue_expand_nodes(c, c->stream);
    }
    put(c->d_leaves, R.leaves);
    put(c->d_tris, R.tris);
    if (failed)
        return failed;
    if (!R.tris.empty()) { // the packets' geometric normals, by the same device code a repack uses (pt::packet_normal), and with
                           // them the tangent frames of both shading normals of every triangle (option "tri_frames")
        const int n = (int)(R.tris.size() / 3);
        HIP_TRY(c, hipMalloc((void **)&c->d_tri_frames, (size_t)n * pt::TRI_FRAME_F4 * sizeof(float4)));
        hipLaunchKernelGGL(pt::tri_normals_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_tris, c->d_tri_frames, n);
        HIP_TRY(c, hipGetLastError());
    }
    if (int rc = upload_tlas(c, mesh_count, tlas_nodes, tlas_node_count, tlas_mesh_indices, tlas_index_count, false))
        return rc;
    // the derived scalars
    c->n_geometry_uploads++;
    c->tlas_refits = 0;
    c->tlas_reorders = 0;
    c->all_single_leaf = S.all_leaf;
    c->any_transform = false;
    for (int m = 0; m < mesh_count; ++m)
        c->any_transform = c->any_transform || meshes[m].has_transform != 0;
    c->stack_entries = R.max_depth < 1 ? 1 : R.max_depth;
    c->pair_tri_slots = (int)(R.tris.size() / 3);
    c->pair_max_leaf = 0;
    for (const int2 &lf : R.leaves)
        if (lf.y > c->pair_max_leaf)
            c->pair_max_leaf = lf.y;
    c->pair_leaf_uniform = c->pair_max_leaf > 0;
    for (const int2 &lf : R.leaves)
        c->pair_leaf_uniform = c->pair_leaf_uniform && lf.y == c->pair_max_leaf;
    c->pm1_plan_ok = c->pair_leaf_uniform && pt::pm1_build_plan(c->pair_max_leaf, &c->pm1_plan);
    // (from the descriptors' fp32 values, which are the ones that went up: rec[0..1] of a mesh, node 0 of the TLAS)
    c->plain_leaf_ok = pt::plain_leaf_scene(meshes, mesh_count, tlas_nodes, tlas_node_count, tlas_mesh_indices, tlas_index_count);
    // the frames stand while the packets' normals do and a shading normal is one of them: no mesh with a transform.  A refit or
    // rebuild writes new normals and no frames (a scene that refits every frame would pay for a table it reads once); whatever
    // clears plain_leaf_ok clears this too, until the next full upload.
    c->tri_frames_ok = c->d_tri_frames != nullptr && !c->any_transform;
    if (int rc = upload_instance_pretests(c, meshes, mesh_count))
        return rc;
    c->have_geometry = true;
    return PTRT_OK;
}

// Instances moved, nothing else changed (Scene::updateAccelerationStructures for a mesh whose transform is dirty,
// scene.cuh:656-743): new matrices and has_transform flags into the mesh records, new TLAS; vertices, BLASes and
// triangle packets stay where they are.
int ptrt_update_instances(ptrt_ctx *c, const ptrt_mesh_desc *meshes, int mesh_count, const ptrt_bvh_node *tlas_nodes,
                          int tlas_node_count, const int32_t *tlas_mesh_indices, int tlas_index_count) {
    if (int rc = enter_geometry(c, "ptrt_update_instances",
                                meshes && tlas_nodes && tlas_mesh_indices && tlas_node_count > 0 && tlas_index_count > 0))
        return rc;
    if (mesh_count != c->n_meshes)
        return fail(c, PTRT_E_INVALID, "ptrt_update_instances: %d meshes, %d uploaded (use ptrt_upload_geometry)", mesh_count,
                    c->n_meshes);
    if (int rc = set_device(c))
        return rc;
    if (int rc = upload_tlas(c, mesh_count, tlas_nodes, tlas_node_count, tlas_mesh_indices, tlas_index_count, true))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // frames in flight still read the old records
    c->plain_leaf_ok = c->tri_frames_ok = false; // (a new root box over mesh boxes only the device may know: derived again by the next full upload)
    c->any_transform = false;
    c->xf_host_stale = false; // (every mesh's flag bit and matrices are rewritten below, on both sides)
    for (int m = 0; m < mesh_count; ++m) {
        const ptrt_mesh_desc &M = meshes[m];
        float4 *rec = &c->h_mesh_recs[(size_t)m * pt::MESH_REC_F4];
        set_rec_flag(rec, REC_INSTANCE, M.has_transform != 0);
        set_rec_xform(rec, M.inverse, M.world, M.normal);
        c->any_transform = c->any_transform || M.has_transform != 0;
        // flags word and the nine matrix rows only: the root box (rec[0].xyz, rec[1].xyz) on the device may have
        // been moved by ptrt_refit / ptrt_build_bvh since the upload and stays as it is
        HIP_TRY(c, hipMemcpyAsync(&c->d_mesh_recs[(size_t)m * pt::MESH_REC_F4 + 1].w, &rec[1].w, 4, hipMemcpyHostToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(&c->d_mesh_recs[(size_t)m * pt::MESH_REC_F4 + 2], &rec[2], 9 * sizeof(float4),
                                  hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = upload_tlas(c, mesh_count, tlas_nodes, tlas_node_count, tlas_mesh_indices, tlas_index_count, false))
        return rc;
    drop_graphs(c);
    c->n_instance_updates++;
    // First-pass boxes of the instances (PMODE 3) from the root boxes the DEVICE holds: after a ptrt_refit / ptrt_build_bvh
    // the caller's descriptors may describe the tree as it was uploaded (or BVH arrays that no longer exist), and a box
    // built from a stale root would cull instances the reference's local test hits.  The descriptors' BVH arrays are not read.
    std::vector<float4> dev_recs((size_t)mesh_count * pt::MESH_REC_F4);
    HIP_TRY(c, hipMemcpyAsync(dev_recs.data(), c->d_mesh_recs, dev_recs.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = upload_instance_pretests(c, meshes, mesh_count, dev_recs.data()))
        return rc;
    return PTRT_OK;
}

int ptrt_set_instance_transforms(ptrt_ctx *c, int first_mesh, int count, const ptrt_instance_xform *xf) {
    if (int rc = enter_geometry(c, "ptrt_set_instance_transforms"))
        return rc;
    if (!xf || count < 0 || first_mesh < 0 || first_mesh > c->n_meshes || count > c->n_meshes - first_mesh)
        return fail(c, PTRT_E_INVALID, "ptrt_set_instance_transforms: meshes [%d, %d + %d) of %d%s", first_mesh, first_mesh, count,
                    c->n_meshes, xf ? "" : ", NULL transforms");
    if (count == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    // Staging (as ptrt_update_vertices stages host positions): two halves of pinned memory and a device mirror.  Calls fill the
    // current half; when it is full the other one is taken, after the event behind the last copy out of it -- enqueued at
    // least a half's worth of records (two frames of every mesh moving) ago.  No allocation unless the mesh count grew.
    const size_t need = std::max<size_t>((size_t)c->n_meshes * 2, 256);
    if (c->xf.cap < need) {
        for (int k = 0; k < 2; ++k)
            if (c->xf.pending[k])
                HIP_TRY(c, hipEventSynchronize(c->xf.ev[k]));
        if (c->xf.h_xf)
            HIP_TRY(c, hipHostFree(c->xf.h_xf));
        c->xf.h_xf = nullptr;
        dfree(c->xf.d_xf);
        c->xf.cap = 0;
        HIP_TRY(c, hipHostMalloc((void **)&c->xf.h_xf, need * 2 * pt::XFORM_F * sizeof(float), hipHostMallocDefault));
        HIP_TRY(c, hipMalloc((void **)&c->xf.d_xf, need * 2 * pt::XFORM_F * sizeof(float)));
        for (int k = 0; k < 2; ++k) {
            if (!c->xf.ev[k])
                HIP_TRY(c, hipEventCreateWithFlags(&c->xf.ev[k], hipEventDisableTiming));
            c->xf.used[k] = 0;
            c->xf.pending[k] = false;
        }
        c->xf.cap = need;
        c->xf.cur = 0;
    }
    if (c->xf.used[c->xf.cur] + (size_t)count > c->xf.cap) {
        c->xf.cur ^= 1;
        if (c->xf.pending[c->xf.cur])
            HIP_TRY(c, hipEventSynchronize(c->xf.ev[c->xf.cur]));
        c->xf.pending[c->xf.cur] = false;
        c->xf.used[c->xf.cur] = 0;
    }
    const int half = c->xf.cur;
    const size_t at = ((size_t)half * c->xf.cap + c->xf.used[half]) * pt::XFORM_F;
    float *hs = c->xf.h_xf + at;
    for (int i = 0; i < count; ++i) {
        const ptrt_instance_xform &X = xf[i];
        float4 *rec = &c->h_mesh_recs[(size_t)(first_mesh + i) * pt::MESH_REC_F4];
        set_rec_flag(rec, REC_INSTANCE, X.has_transform != 0);
        set_rec_xform(rec, X.inverse, X.world, X.normal);
        float *o = hs + (size_t)i * pt::XFORM_F;
        o[0] = as_f(X.has_transform ? 1 : 0);
        o[1] = o[2] = o[3] = 0.0f;
        std::memcpy(o + 4, &rec[2], 9 * sizeof(float4));
    }
    c->any_transform = c->xf_host_stale; // (flags only the device knows: held true, see sync_host_xforms)
    for (int m = 0; m < c->n_meshes && !c->any_transform; ++m)
        c->any_transform = (rec_flags(&c->h_mesh_recs[(size_t)m * pt::MESH_REC_F4]) & REC_INSTANCE) != 0;
    set_inst_c2(c, host_inst_c2(c));
    c->inst_pre_ok = false; // the first-pass boxes follow with the next ptrt_refit_tlas
    HIP_TRY(c, hipMemcpyAsync(c->xf.d_xf + at, hs, (size_t)count * pt::XFORM_F * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pt::scatter_xforms_kernel, dim3((count * 37 + 255) / 256), dim3(256), 0, c->stream, c->xf.d_xf + at,
                       pt::XFORM_STAGED, c->d_mesh_recs, first_mesh, count);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->xf.ev[half], c->stream)); // (this half's records are free again behind this)
    c->xf.pending[half] = true;
    c->xf.used[half] += (size_t)count;
    return PTRT_OK;
}

// The same records from DEVICE memory ordered on the context's stream: one scatter launch that reads them in place.  The host
// copy of the flag bits and matrices lags from here on (sync_host_xforms).
int ptrt_set_instance_transforms_device(ptrt_ctx *c, int first_mesh, int count, const ptrt_instance_xform *d_xf) {
    static_assert(sizeof(ptrt_instance_xform) == 49 * sizeof(float), "ptrt_instance_xform is read as 49 words");
    constexpr int W = (int)sizeof(float);
    constexpr pt::XformLayout abi{49, (int)offsetof(ptrt_instance_xform, has_transform) / W, (int)offsetof(ptrt_instance_xform, inverse) / W,
                                  (int)offsetof(ptrt_instance_xform, world) / W, (int)offsetof(ptrt_instance_xform, normal) / W};
    if (int rc = enter_geometry(c, "ptrt_set_instance_transforms_device"))
        return rc;
    if (!d_xf || count < 0 || first_mesh < 0 || first_mesh > c->n_meshes || count > c->n_meshes - first_mesh)
        return fail(c, PTRT_E_INVALID, "ptrt_set_instance_transforms_device: meshes [%d, %d + %d) of %d%s", first_mesh, first_mesh,
                    count, c->n_meshes, d_xf ? "" : ", NULL transforms");
    if (count == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    c->xf_host_stale = true;
    c->any_transform = true;
    c->plain_leaf_ok = c->tri_frames_ok = false;
    c->inst_pre_ok = false; // the first-pass boxes follow with the next ptrt_refit_tlas / ptrt_reorder_tlas
    hipLaunchKernelGGL(pt::scatter_xforms_kernel, dim3((count * 37 + 255) / 256), dim3(256), 0, c->stream,
                       reinterpret_cast<const float *>(d_xf), abi, c->d_mesh_recs, first_mesh, count);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// Poses (Transform3D's nine floats) from DEVICE memory: one launch derives the has_transform bit and the nine matrix rows as the
// reference's host code would (pt::compose_poses_kernel) and writes them into the mesh records.  Host bookkeeping as above.
// The kernel follows d_pose for count * 36 bytes, so memory that is not the device's is refused here, before the launch.
int ptrt_set_instance_poses_device(ptrt_ctx *c, int first_mesh, int count, const ptrt_instance_pose *d_pose) {
    static_assert(sizeof(ptrt_instance_pose) == pt::POSE_F * sizeof(float) && offsetof(ptrt_instance_pose, rotation) == 12 &&
                      offsetof(ptrt_instance_pose, scale) == 24,
                  "ptrt_instance_pose is read as nine floats: position, rotation, scale");
    if (int rc = enter_geometry(c, "ptrt_set_instance_poses_device"))
        return rc;
    if (!d_pose || count < 0 || first_mesh < 0 || first_mesh > c->n_meshes || count > c->n_meshes - first_mesh)
        return fail(c, PTRT_E_INVALID, "ptrt_set_instance_poses_device: meshes [%d, %d + %d) of %d%s", first_mesh, first_mesh, count,
                    c->n_meshes, d_pose ? "" : ", NULL poses");
    if (count == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    const size_t bytes = (size_t)count * sizeof(ptrt_instance_pose);
    if (!device_span(c, d_pose, bytes))
        return fail(c, PTRT_E_INVALID, "ptrt_set_instance_poses_device: poses are not %zu bytes of device memory on device %d", bytes,
                    c->device);
    c->xf_host_stale = true;
    c->any_transform = true;
    c->plain_leaf_ok = c->tri_frames_ok = false;
    c->inst_pre_ok = false; // the first-pass boxes follow with the next ptrt_refit_tlas / ptrt_reorder_tlas
    hipLaunchKernelGGL(pt::compose_poses_kernel, dim3((count + pt::POSE_BLOCK - 1) / pt::POSE_BLOCK), dim3(pt::POSE_BLOCK), 0, c->stream,
                       reinterpret_cast<const float *>(d_pose), c->d_mesh_recs, first_mesh, count);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// What the device's mesh records hold now, as records ptrt_set_instance_transforms takes: rows 0-2 of each matrix (a normal
// row's fourth word is 0: the records do not keep it), row 3 = 0 0 0 1.
int ptrt_read_instance_transforms(ptrt_ctx *c, int first_mesh, int count, ptrt_instance_xform *out) {
    if (int rc = enter_geometry(c, "ptrt_read_instance_transforms"))
        return rc;
    if (!out || count < 0 || first_mesh < 0 || first_mesh > c->n_meshes || count > c->n_meshes - first_mesh)
        return fail(c, PTRT_E_INVALID, "ptrt_read_instance_transforms: meshes [%d, %d + %d) of %d%s", first_mesh, first_mesh, count,
                    c->n_meshes, out ? "" : ", NULL output");
    if (count == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    std::vector<float4> dev((size_t)count * pt::MESH_REC_F4);
    HIP_TRY(c, hipMemcpyAsync(dev.data(), c->d_mesh_recs + (size_t)first_mesh * pt::MESH_REC_F4, dev.size() * sizeof(float4),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < count; ++i) {
        const float4 *rec = &dev[(size_t)i * pt::MESH_REC_F4];
        ptrt_instance_xform &X = out[i];
        std::memcpy(X.inverse, &rec[2], 3 * sizeof(float4));
        std::memcpy(X.world, &rec[5], 3 * sizeof(float4));
        std::memcpy(X.normal, &rec[8], 3 * sizeof(float4));
        X.normal[3] = X.normal[7] = X.normal[11] = 0.0f;
        for (float *m : {X.world, X.inverse, X.normal}) {
            m[12] = m[13] = m[14] = 0.0f;
            m[15] = 1.0f;
        }
        X.has_transform = (rec_flags(rec) & REC_INSTANCE) ? 1 : 0;
    }
    return PTRT_OK;
}

int ptrt_refit_tlas(ptrt_ctx *c) { return refit_tlas_entry(c, "ptrt_refit_tlas", false); }

int ptrt_reorder_tlas(ptrt_ctx *c) { return refit_tlas_entry(c, "ptrt_reorder_tlas", true); }

int ptrt_read_tlas_order(ptrt_ctx *c, int32_t *mesh_indices_out, int count) {
    if (int rc = enter_geometry(c, "ptrt_read_tlas_order", mesh_indices_out != nullptr))
        return rc;
    if (count != c->n_tlas_index)
        return fail(c, PTRT_E_INVALID, "ptrt_read_tlas_order: the uploaded TLAS has %d indices, asked for %d", c->n_tlas_index, count);
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(mesh_indices_out, c->d_tlas_mesh_ids, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

int ptrt_read_tlas(ptrt_ctx *c, ptrt_bvh_node *nodes_out, int node_count) {
    if (int rc = enter_geometry(c, "ptrt_read_tlas", nodes_out != nullptr))
        return rc;
    if (node_count != (int)c->h_tlas_in.size())
        return fail(c, PTRT_E_INVALID, "ptrt_read_tlas: the uploaded TLAS has %d nodes, asked for %d", (int)c->h_tlas_in.size(),
                    node_count);
    if (int rc = set_device(c))
        return rc;
    std::vector<float4> nodes((size_t)c->n_tlas_inner * 4), root(2);
    if (!nodes.empty())
        HIP_TRY(c, hipMemcpyAsync(nodes.data(), c->d_tlas_nodes, nodes.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(root.data(), c->d_tlas_root_box, 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < node_count; ++i) {
        ptrt_bvh_node N = c->h_tlas_in[i];
        const int dst = c->h_tlas_in_dst[i];
        if (dst >= 0) {
            const float *n = reinterpret_cast<const float *>(&nodes[(size_t)(dst >> 1) * 4]) + ((dst & 1) ? 6 : 0);
            N.bmin = ptrt_vec3{n[0], n[1], n[2]};
            N.bmax = ptrt_vec3{n[3], n[4], n[5]};
        } else if (dst != INT32_MIN) {
            N.bmin = ptrt_vec3{root[0].x, root[0].y, root[0].z};
            N.bmax = ptrt_vec3{root[1].x, root[1].y, root[1].z};
        }
        nodes_out[i] = N;
    }
    return PTRT_OK;
}

// test hook: how often each kind of acceleration-structure upload ran
int ptrt_debug_upload_counts(ptrt_ctx *c, int *out2) {
    if (!ctx_live(c) || !out2)
        return PTRT_E_INVALID;
    out2[0] = c->n_geometry_uploads;
    out2[1] = c->n_instance_updates;
    return PTRT_OK;
}

int ptrt_update_vertices(ptrt_ctx *c, int mesh, const float *verts, int vert_count, int on_device) {
    if (int rc = enter_geometry(c, "ptrt_update_vertices", verts != nullptr))
        return rc;
    if (mesh < 0 || mesh >= c->n_meshes || vert_count != c->mesh_vert_count[mesh])
        return fail(c, PTRT_E_INVALID, "ptrt_update_vertices: mesh %d has %d vertices, got %d (topology must not change)",
                    mesh, (mesh >= 0 && mesh < c->n_meshes) ? c->mesh_vert_count[mesh] : -1, vert_count);
    if (int rc = set_device(c))
        return rc;
    const size_t bytes = (size_t)vert_count * 12;
    float *dst = c->d_verts + (size_t)c->mesh_vert_base[mesh] * 3;
    auto device_copy = [&](const float *src) -> int { // (a kernel of our own: the runtime's blit ran this copy at 50 GB/s)
        const size_t nf = bytes / 4;
        const int vec4 = (((size_t)src | (size_t)dst) & 15u) == 0u ? 1 : 0;
        const unsigned blocks = (unsigned)std::min<size_t>((nf / (vec4 ? 4 : 1) + 255) / 256, (size_t)c->n_cus * 8);
        hipLaunchKernelGGL(pt::copy_words_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, c->stream, src, dst, nf, vec4);
        HIP_TRY(c, hipGetLastError());
        return PTRT_OK;
    };
    if (on_device)
        return device_copy(verts);
    // Host positions: the caller may reuse its buffer the moment this returns.  Waiting for the copy would mean waiting for
    // everything in front of it on the stream -- the previous frame's trace -- so the host could not prepare frame N + 1 while the
    // GPU renders frame N (the reference's updatePTScene -> commitObjectChanges() loop: 2.04 ms per fluid frame, host and GPU
    // in turn).  The positions go through one of four pinned staging buffers of the context instead and cross PCIe behind the
    // stream's work; a buffer is waited for only when it comes round again, four updates later.
    constexpr size_t STAGE_MAX = (size_t)256 << 20;
    if (bytes > STAGE_MAX) {
        HIP_TRY(c, hipMemcpyAsync(dst, verts, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return PTRT_OK;
    }
    const int k = (int)(c->verts.stage_n++ % VertexStage::STAGES);
    if (c->verts.stage_ev[k])
        HIP_TRY(c, hipEventSynchronize(c->verts.stage_ev[k]));
    else
        HIP_TRY(c, hipEventCreateWithFlags(&c->verts.stage_ev[k], hipEventDisableTiming));
    // (Positions already in PINNED memory need no host copy: they cross PCIe on a stream of their own into a device staging
    // buffer -- the call waits for that transfer alone, ~0.1 ms for 4.7 MB -- and move into the arena on the context's stream.)
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, verts) == hipSuccess && pa.type == hipMemoryTypeHost) {
        if (!c->verts.copy_stream) {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->verts.copy_stream, hipStreamNonBlocking));
            HIP_TRY(c, hipEventCreateWithFlags(&c->verts.copy_ev, hipEventDisableTiming));
        }
        if (c->verts.d_stage_bytes[k] < bytes) {
            dfree(c->verts.d_stage[k]);
            c->verts.d_stage_bytes[k] = 0;
            HIP_TRY(c, hipMalloc((void **)&c->verts.d_stage[k], bytes));
            c->verts.d_stage_bytes[k] = bytes;
        }
        HIP_TRY(c, hipMemcpyAsync(c->verts.d_stage[k], verts, bytes, hipMemcpyHostToDevice, c->verts.copy_stream));
        HIP_TRY(c, hipEventRecord(c->verts.copy_ev, c->verts.copy_stream));
        HIP_TRY(c, hipStreamSynchronize(c->verts.copy_stream)); // the caller's buffer is its own again
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->verts.copy_ev, 0));
        if (int rc = device_copy(c->verts.d_stage[k]))
            return rc;
        HIP_TRY(c, hipEventRecord(c->verts.stage_ev[k], c->stream)); // (the staging buffer is free again behind this)
        return PTRT_OK;
    }
    (void)hipGetLastError(); // (an address HIP does not know is ordinary host memory)
    if (c->verts.stage_bytes[k] < bytes) {
        if (c->verts.h_stage[k])
            HIP_TRY(c, hipHostFree(c->verts.h_stage[k]));
        c->verts.h_stage[k] = nullptr;
        c->verts.stage_bytes[k] = 0;
        HIP_TRY(c, hipHostMalloc(&c->verts.h_stage[k], bytes, hipHostMallocDefault));
        c->verts.stage_bytes[k] = bytes;
    }
    std::memcpy(c->verts.h_stage[k], verts, bytes);
    HIP_TRY(c, hipMemcpyAsync(dst, c->verts.h_stage[k], bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->verts.stage_ev[k], c->stream));
    return PTRT_OK;
}

int ptrt_refit(ptrt_ctx *c) {
    if (int rc = enter_geometry(c, "ptrt_refit"))
        return rc;
    if (int rc = set_device(c))
        return rc;
    c->inst_pre_ok = false; // root boxes move on the device: the instances' first-pass boxes are stale until the next upload
    c->plain_leaf_ok = c->tri_frames_ok = false; // ... and nobody has compared them with the root box (plain_leaf.h)
    return run_graphed(c, GK_REFIT, [c](hipStream_t st) { return enqueue_refit(c, st); });
}

int ptrt_build_bvh(ptrt_ctx *c, int mesh) {
    if (int rc = enter_geometry(c, "ptrt_build_bvh"))
        return rc;
    // (as in ptrt_refit -- but ahead of the mesh check: a call refused for its mesh index still marks the boxes stale)
    c->inst_pre_ok = false;
    c->plain_leaf_ok = c->tri_frames_ok = false;
    if (mesh < 0 || mesh >= c->n_meshes)
        return fail(c, PTRT_E_INVALID, "ptrt_build_bvh: no mesh %d", mesh);
    if (!c->mesh_rebuildable[mesh])
        return fail(c, PTRT_E_INVALID, "ptrt_build_bvh: mesh %d's uploaded BVH does not place every face in exactly one "
                                       "leaf position; rebuild on the host and re-upload", mesh);
    if (int rc = set_device(c))
        return rc;
    const int n = c->mesh_face_count[mesh];
    const int n_waves = (n + pt::RS_WAVE_KEYS - 1) / pt::RS_WAVE_KEYS;
    if (n > c->build.sort_capacity) {
        for (int k = 0; k < 2; ++k) {
            dfree(c->build.d_sort_keys[k]);
            dfree(c->build.d_sort_vals[k]);
        }
        dfree(c->build.d_sort_hist);
        dfree(c->build.d_centroids);
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(c, hipMalloc((void **)&c->build.d_sort_keys[k], (size_t)n * 4));
            HIP_TRY(c, hipMalloc((void **)&c->build.d_sort_vals[k], (size_t)n * 4));
        }
        HIP_TRY(c, hipMalloc((void **)&c->build.d_sort_hist, (size_t)n_waves * 256 * 4 * 2)); // counts | positions
        HIP_TRY(c, hipMalloc((void **)&c->build.d_centroids, (size_t)n * 12));
        if (!c->build.d_cbounds) { // min words all-ones, max words zero; every build leaves them so again
            HIP_TRY(c, hipMalloc((void **)&c->build.d_cbounds, 6 * 4));
            HIP_TRY(c, hipMemsetAsync(c->build.d_cbounds, 0xff, 12, c->stream));
            HIP_TRY(c, hipMemsetAsync(c->build.d_cbounds + 3, 0, 12, c->stream));
        }
        c->build.sort_capacity = n;
        drop_graphs(c); // captured launches hold the old scratch pointers
    }
    return run_graphed(c, mesh, [c, mesh](hipStream_t st) {
        if (int rc = enqueue_build(c, mesh, st))
            return rc;
        return enqueue_refit(c, st);
    });
}

int ptrt_update_triangles(ptrt_ctx *c, int mesh, const float *verts9, int tri_count, int on_device) {
    if (int rc = enter_geometry(c, "ptrt_update_triangles", (verts9 || tri_count <= 0) && tri_count >= 0))
        return rc;
    if (mesh < 0 || mesh >= c->n_meshes)
        return fail(c, PTRT_E_INVALID, "ptrt_update_triangles: no mesh %d", mesh);
    if (!c->mesh_is_soup[mesh])
        return fail(c, PTRT_E_INVALID, "ptrt_update_triangles: mesh %d is not a triangle soup (face i = vertices 3i..3i+2)", mesh);
    if (tri_count > c->mesh_face_count[mesh])
        return fail(c, PTRT_E_INVALID, "ptrt_update_triangles: mesh %d was uploaded with room for %d triangles, got %d", mesh,
                    c->mesh_face_count[mesh], tri_count);
    if (int rc = set_device(c))
        return rc;
    float *dst = c->d_verts + (size_t)c->mesh_vert_base[mesh] * 3;
    if (tri_count > 0)
        HIP_TRY(c, hipMemcpyAsync(dst, verts9, (size_t)tri_count * 36, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                  c->stream));
    const int total = c->mesh_vert_count[mesh], real = tri_count * 3;
    if (total > real)
        hipLaunchKernelGGL(pt::pad_soup_kernel, dim3((total - real + 255) / 256), dim3(256), 0, c->stream, dst, real, total);
    HIP_TRY(c, hipGetLastError());
    if (!on_device)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

int ptrt_read_prim_order(ptrt_ctx *c, int mesh, int32_t *out, int count) {
    if (int rc = enter_geometry(c, "ptrt_read_prim_order", out != nullptr))
        return rc;
    if (mesh < 0 || mesh >= c->n_meshes || !c->mesh_rebuildable[mesh] || count != c->mesh_face_count[mesh])
        return fail(c, PTRT_E_INVALID, "ptrt_read_prim_order: mesh %d has %d rebuildable prim positions, asked for %d", mesh,
                    (mesh >= 0 && mesh < c->n_meshes && c->mesh_rebuildable[mesh]) ? c->mesh_face_count[mesh] : 0, count);
    if (int rc = set_device(c))
        return rc;
    std::vector<int4> sf((size_t)count);
    std::vector<int> pos((size_t)count);
    HIP_TRY(c, hipMemcpyAsync(sf.data(), c->d_slot_face + c->mesh_slot_base[mesh], (size_t)count * 16, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(pos.data(), c->d_slot_pos + c->mesh_slot_base[mesh], (size_t)count * 4, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < count; ++i)
        out[pos[(size_t)i]] = sf[(size_t)i].w;
    return PTRT_OK;
}

// The counterpart of ptrt_read_tlas for one mesh's BVH: the uploaded nodes with the boxes the device holds now.  A node's box
// is the child-pair slot of its parent in d_nodes (dst >= 0), the root's the mesh's root box in d_mesh_recs (dst < 0); a node
// convert_tree did not reach (INT32_MIN) keeps its uploaded box.  The canonical nodes only: d_nodes2 is derived from them.
int ptrt_read_bvh(ptrt_ctx *c, int mesh, ptrt_bvh_node *nodes_out, int node_count) {
    if (int rc = enter_geometry(c, "ptrt_read_bvh", nodes_out != nullptr))
        return rc;
    if (mesh < 0 || mesh >= c->n_meshes || node_count != (int)c->h_mesh_in[(size_t)mesh].size())
        return fail(c, PTRT_E_INVALID, "ptrt_read_bvh: mesh %d was uploaded with %d nodes, asked for %d", mesh,
                    (mesh >= 0 && mesh < c->n_meshes) ? (int)c->h_mesh_in[(size_t)mesh].size() : 0, node_count);
    if (int rc = set_device(c))
        return rc;
    std::vector<float4> nodes((size_t)c->n_nodes * 4), rec(2);
    if (!nodes.empty())
        HIP_TRY(c, hipMemcpyAsync(nodes.data(), c->d_nodes, nodes.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rec.data(), c->d_mesh_recs + (size_t)mesh * pt::MESH_REC_F4, 2 * sizeof(float4), hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < node_count; ++i) {
        ptrt_bvh_node N = c->h_mesh_in[(size_t)mesh][(size_t)i];
        const int dst = c->h_mesh_in_dst[(size_t)mesh][(size_t)i];
        if (dst >= 0) {
            const float *n = reinterpret_cast<const float *>(&nodes[(size_t)(dst >> 1) * 4]) + ((dst & 1) ? 6 : 0);
            N.bmin = ptrt_vec3{n[0], n[1], n[2]};
            N.bmax = ptrt_vec3{n[3], n[4], n[5]};
        } else if (dst != INT32_MIN) {
            N.bmin = ptrt_vec3{rec[0].x, rec[0].y, rec[0].z};
            N.bmax = ptrt_vec3{rec[1].x, rec[1].y, rec[1].z};
        }
        nodes_out[i] = N;
    }
    return PTRT_OK;
}

} // extern "C"
