// ptrt_render.hip.h -- the frame path of the C ABI: what one ptrt_render call decides about its trace (FramePlan: which loop
// shape, how much LDS, whether it may be dealt to several launches), whether the frame may overlap its predecessor
// (plan_overlap), the launches (launch_frame, launch_trace, the wavefront and asynchronous-lane runners), the post chain
// (denoiser, bloom, up-scale) and the kernel timings.  Included by ptrt_capi.hip behind struct ptrt_ctx, the helpers every
// entry point shares (fail, HIP_TRY, ctx_live, set_device, make_params) and ptrt_present.hip.h (ring_mark_rendered).
#pragma once

namespace {

// ---- geometry and traversal mode of a scene ------------------------------------------------------------------------
int pick_geom(ptrt_ctx *c) {
    int g = c->tlas_single_leaf ? (c->all_single_leaf ? 0 : 1) : 2;
    if (c->force_geom > g)
        g = c->force_geom; // a more general variant is always valid
    return g;
}

// PMODE 4 keeps extension and shadow pairs in one list; the shadow pairs get what is left of a 10-KB LDS budget (16 waves
// per CU), within the clamps of lds::merged_pair_cap
constexpr size_t MERGED_LDS_BUDGET = 10240;
int merged_pair_cap(const ptrt_ctx *c) { return pt::lds::merged_pair_cap(c->pair_meshes, c->stack_entries, MERGED_LDS_BUDGET); }

// in-wave (ray, mesh) pair compaction needs every BLAS to be one leaf and the staged
// triangle packets to fit a modest LDS budget
size_t pair_lds_bytes(const ptrt_ctx *c, int pmode) {
    return pt::lds::pair_layout(pmode, c->pair_meshes, c->pair_tri_slots, c->stack_entries, c->tlas_max_leaf, c->tlas_depth,
                                pmode == 4 ? merged_pair_cap(c) : 0).total;
}
// 0 lock-step, 1 pairs over single-leaf BLASes, 2 pairs over general BLASes (single-leaf TLAS)
int pair_mode(const ptrt_ctx *c, int geom, bool merged) {
    if (!c->pair_trace)
        return 0;
    if (geom == 2) // a real TLAS: rounds of one leaf per ray (pt_render.hip.h)
        return (c->tlas_max_leaf > 0 && c->tlas_max_leaf <= 32 && c->pair_tri_slots < (1 << 24) && pair_lds_bytes(c, 3) <= 40 * 1024)
                   ? 3 : 0;
    if (c->pair_meshes <= 0)
        return 0;
    if (geom == 0 && c->pair_meshes < 1024 && c->pair_max_leaf < 65536 && pair_lds_bytes(c, 1) <= 40 * 1024)
        return 1;
    // (PMODE 4's compacted leaf phase is not optional: scenes with leaves beyond its list keep PMODE 2)
    if (geom <= 1 && merged && c->leaf_pairs && c->pair_meshes < 256 && c->pair_tri_slots < (1 << 24) &&
        pt::leaf_pairs_fit(c->pair_max_leaf) && pair_lds_bytes(c, 4) <= 40 * 1024)
        return 4;
    if (geom <= 1 && c->pair_meshes < 256 && c->pair_tri_slots < (1 << 24) && pair_lds_bytes(c, 2) <= 40 * 1024)
        return 2;
    return 0;
}

// Dynamic LDS of a launch in bytes: the total of its shape's layout in lds_layout.h (PMODE 1: pm1_layout, below).
// A launch_trace workgroup or a ray query
size_t trace_lds_bytes(const ptrt_ctx *c, int geom, int pmode) {
    return pmode ? pair_lds_bytes(c, pmode) : pt::lds::lockstep_layout(geom == 0 ? 0 : c->stack_entries).total;
}
// PMODE 2 with option lds_nodes: four tiles per workgroup, one LDS copy of the mesh heads and of the BLAS top levels (north
// star: "BVH nodes ... staged in LDS")
size_t lds_nodes_bytes(const ptrt_ctx *c) { return pt::lds::nodes_layout(c->pair_meshes, c->stack_entries, pt::TOP_NODES).total; }
size_t wavefront_lds_bytes(const ptrt_ctx *c) { return pt::lds::wavefront_layout(c->stack_entries).total; }
size_t async_lds_bytes(const ptrt_ctx *c) { return pt::lds::async_layout(c->stack_entries).total; }

// The 3 * EV_RING events of option "time_launches" for auxiliary stream i, all of them or none: a failure part-way destroys
// what it made and turns the option off for this context, so that no later frame records on a null event.
int create_launch_events(ptrt_ctx *c, int i) {
    std::vector<hipEvent_t> ev(3 * EV_RING, nullptr);
    for (auto &e : ev) {
        const hipError_t err = hipEventCreate(&e);
        if (err != hipSuccess) {
            for (hipEvent_t made : ev)
                if (made)
                    (void)hipEventDestroy(made);
            c->time_launches = 0;
            return fail(c, PTRT_E_HIP, "hipEventCreate failed: %s (time_launches is off now)", hipGetErrorString(err));
        }
    }
    c->launch_ev[i].swap(ev);
    return PTRT_OK;
}

// One 8x8 tile per 64-thread workgroup.  The frame's tile rows may be dealt to `c->split_eff` launches that run concurrently
// on the context's stream and its auxiliary streams (forked and joined by events around them: render_split_begin / _end).
template <int GEOM, int PMODE> int launch_trace(ptrt_ctx *c, const pt::KParams &K0, bool full, int grid, size_t lds) {
    const int n = c->split_eff > 1 ? c->split_eff : 1;
    const int tiles_y = grid / K0.tiles_x;
    const int slot = (int)(c->launches % EV_RING);
    const bool timed = c->time_launches && n > 1; // (one launch on the context's stream is what the frame's own events bracket)
    c->launch_timed[slot] = 0;
    for (int i = 0; i < n; ++i) {
        pt::KParams K = K0;
        K.split_n = n;
        K.split_i = i;
        const int g = n > 1 ? K0.tiles_x * ((tiles_y - i + n - 1) / n) : grid;
        if (g <= 0)
            continue;
        hipStream_t st = n > 1 ? c->aux_stream[i] : c->stream;
        hipEvent_t *ev = nullptr;
        if (timed) {
            if (c->launch_ev[i].empty())
                if (int rc = create_launch_events(c, i))
                    return rc;
            ev = &c->launch_ev[i][3 * slot];
            HIP_TRY(c, hipEventRecord(ev[0], st));
            c->launch_timed[slot] = (unsigned char)(c->launch_timed[slot] | (1u << i));
        }
        if constexpr (PMODE == 1) {
            if (c->refill_eff) {
                // Lane refill: persistent waves -- as many as the chip holds at this variant's occupancy (option "persist":
                // waves per CU) -- that draw the launch's tiles from a queue; the image is tonemapped by a pass behind them.
                K.n_tiles = g;
                K.ticket_tiles = c->ticket_tiles;
                K.queue = c->d_queue + 2 * (n > 1 ? 1 + i : 0); // (launches that share a queue are ordered: one stream each)
                if (K.counters) // (slots of its own: a launch of the one-tile kernel on another stream may still be adding to the tile slots)
                    K.counters += c->refill_counter_base * pt::COUNTER_WORDS;
                const int per_cu = c->persist > 0 ? c->persist : 4 * pt::waves_per_simd(PMODE, full, 1);
                const int waves = std::min((g + c->ticket_tiles - 1) / c->ticket_tiles, c->n_cus * per_cu);
                if (full)
                    hipLaunchKernelGGL((pt::path_trace_kernel<GEOM, true, PMODE, 1, true>), dim3(waves), dim3(64), lds, st, K);
                else
                    hipLaunchKernelGGL((pt::path_trace_kernel<GEOM, false, PMODE, 1, true>), dim3(waves), dim3(64), lds, st, K);
                if (ev)
                    HIP_TRY(c, hipEventRecord(ev[1], st));
                if (K.rgb8) {
                    hipStream_t ts = st;
                    if ((c->tm_prio & 1) && n > 1) { // the pass on a stream of the highest priority, between two events of the launch's stream
                        if (!c->tm_stream[i]) {
                            int lo = 0, hi = 0;
                            HIP_TRY(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
                            HIP_TRY(c, hipStreamCreateWithPriority(&c->tm_stream[i], hipStreamNonBlocking, hi));
                            HIP_TRY(c, hipEventCreateWithFlags(&c->tm_fork[i], hipEventDisableTiming));
                            HIP_TRY(c, hipEventCreateWithFlags(&c->tm_join[i], hipEventDisableTiming));
                        }
                        ts = c->tm_stream[i];
                        HIP_TRY(c, hipEventRecord(c->tm_fork[i], st));
                        HIP_TRY(c, hipStreamWaitEvent(ts, c->tm_fork[i], 0));
                    }
                    if (c->tm_prio & 2)
                        hipLaunchKernelGGL(pt::tonemap_tiles_kernel<true>, dim3(g), dim3(64), 0, ts, K);
                    else
                        hipLaunchKernelGGL(pt::tonemap_tiles_kernel<false>, dim3(g), dim3(64), 0, ts, K);
                    if (ts != st) {
                        HIP_TRY(c, hipEventRecord(c->tm_join[i], ts));
                        HIP_TRY(c, hipStreamWaitEvent(st, c->tm_join[i], 0));
                    }
                }
                if (ev)
                    HIP_TRY(c, hipEventRecord(ev[2], st));
                continue;
            }
        }
        if (full)
            hipLaunchKernelGGL((pt::path_trace_kernel<GEOM, true, PMODE>), dim3(g), dim3(64), lds, st, K);
        else
            hipLaunchKernelGGL((pt::path_trace_kernel<GEOM, false, PMODE>), dim3(g), dim3(64), lds, st, K);
        if (ev) {
            HIP_TRY(c, hipEventRecord(ev[1], st));
            HIP_TRY(c, hipEventRecord(ev[2], st));
        }
    }
    return PTRT_OK;
}

// ---- wavefront stages ------------------------------------------------------------------------
constexpr int WF_MAX_ITERS = 16 * 17 + 2; // spp and max_depth are clamped to 16 by the Scene mirror; larger frames fall back

bool wavefront_applicable(const ptrt_ctx *c, int spp, int max_depth) {
    if (!c->wavefront || !c->tlas_single_leaf || c->pair_meshes <= 0 || c->pair_meshes > 64)
        return false;
    if (spp > 255 || max_depth > 255 || spp * (max_depth + 1) + 2 > WF_MAX_ITERS)
        return false;
    return wavefront_lds_bytes(c) <= 64 * 1024;
}

int run_wavefront(ptrt_ctx *c, const pt::KParams &K, bool full, size_t lds, int spp, int max_depth) {
    const int tiles_y = (K.rows + 7) / 8;
    const size_t items = (size_t)K.tiles_x * tiles_y * 64;
    if (items > c->wf_items) {
        dfree(c->wf_st);
        dfree(c->wf_occ);
        dfree(c->wf_planes);
        dfree(c->wf_hit);
        c->wf_items = 0;
        HIP_TRY(c, hipMalloc((void **)&c->wf_st, items * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc((void **)&c->wf_occ, items * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc((void **)&c->wf_planes, items * 25 * sizeof(float)));
        HIP_TRY(c, hipMalloc((void **)&c->wf_hit, items * sizeof(float4)));
        c->wf_items = items;
    }
    if (!c->wf_live)
        HIP_TRY(c, hipMalloc((void **)&c->wf_live, WF_MAX_ITERS * sizeof(uint32_t)));
    if (!c->wf_trace_blocks || c->wf_trace_lds != lds) {
        int per_cu = 0, cus = 0;
        HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pt::wf_trace_kernel, 256, lds));
        HIP_TRY(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        if (per_cu < 1 || cus < 1)
            return fail(c, PTRT_E_HIP, "wavefront trace kernel does not fit (LDS %zu bytes)", lds);
        c->wf_trace_blocks = per_cu * cus;
        c->wf_trace_lds = lds;
    }
    pt::WfParams W{};
    W.st = c->wf_st;
    W.occ = c->wf_occ;
    W.live = c->wf_live;
    W.hit = c->wf_hit;
    float *p = c->wf_planes;
    W.ray = p;
    W.thr = p + 6 * items;
    W.acc = p + 9 * items;
    W.avg = p + 12 * items;
    W.pend = p + 15 * items;
    W.sh = p + 18 * items;
    W.n_items = (int)items;
    W.fetch_min = c->fetch_min > 0 ? c->fetch_min : 16;
    const int iters = spp * (max_depth + 1);
    HIP_TRY(c, hipMemsetAsync(c->wf_live, 0, (size_t)(iters + 2) * sizeof(uint32_t), c->stream));
    const int shade_blocks = (int)((items + 255) / 256);
    const int chunks = (int)(items / 64);
    const int trace_blocks = std::min(c->wf_trace_blocks, (chunks + 3) / 4);
    for (int it = 0; it <= iters; ++it) {
        W.iter = it;
        if (it > 0)
            hipLaunchKernelGGL(pt::wf_trace_kernel, dim3(trace_blocks), dim3(256), lds, c->stream, K, W);
        if (c->wf_sort && it > 0) { // (the first shade only regenerates: one class)
            const int G = c->wf_sort;
            const int sb = (int)((items + 256 * (size_t)G - 1) / (256 * (size_t)G));
            auto kern = full ? (G == 1 ? pt::wf_shade_kernel<true, 1> : G == 2 ? pt::wf_shade_kernel<true, 2> : pt::wf_shade_kernel<true, 4>)
                             : (G == 1 ? pt::wf_shade_kernel<false, 1> : G == 2 ? pt::wf_shade_kernel<false, 2> : pt::wf_shade_kernel<false, 4>);
            hipLaunchKernelGGL(kern, dim3(sb), dim3(256), 0, c->stream, K, W);
        } else if (full)
            hipLaunchKernelGGL(pt::wf_shade_kernel<true>, dim3(shade_blocks), dim3(256), 0, c->stream, K, W);
        else
            hipLaunchKernelGGL(pt::wf_shade_kernel<false>, dim3(shade_blocks), dim3(256), 0, c->stream, K, W);
    }
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// ---- asynchronous-lane megakernel -------------------------------------------------------------
bool async_applicable(const ptrt_ctx *c) {
    if (!c->async_lanes || !c->tlas_single_leaf || c->pair_meshes <= 0 || c->pair_meshes > 64)
        return false;
    if (!pt::leaf_pairs_fit(c->pair_max_leaf)) // its leaf phase is always the compacted one
        return false;
    return async_lds_bytes(c) <= 40 * 1024;
}

int run_async(ptrt_ctx *c, const pt::KParams &K, bool full, size_t lds) {
    if (!c->as_cursor)
        HIP_TRY(c, hipMalloc((void **)&c->as_cursor, sizeof(uint32_t)));
    if (c->as_lds != lds || !c->as_blocks[full ? 1 : 0]) {
        if (c->as_lds != lds)
            c->as_blocks[0] = c->as_blocks[1] = 0;
        int per_cu = 0, cus = 0;
        if (full)
            HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pt::path_trace_async_kernel<true>, 64, lds));
        else
            HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pt::path_trace_async_kernel<false>, 64, lds));
        HIP_TRY(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        if (per_cu < 1 || cus < 1)
            return fail(c, PTRT_E_HIP, "asynchronous trace kernel does not fit (LDS %zu bytes)", lds);
        c->as_blocks[full ? 1 : 0] = per_cu * cus;
        c->as_lds = lds;
    }
    pt::AsyncParams A{};
    A.cursor = c->as_cursor;
    A.n_tiles = K.tiles_x * ((K.rows + 7) / 8);
    A.shade_min = c->shade_min;
    A.leaf_min = c->as_leaf_min;
    const int grid = std::min(c->as_blocks[full ? 1 : 0], A.n_tiles);
    HIP_TRY(c, hipMemsetAsync(c->as_cursor, 0, sizeof(uint32_t), c->stream));
    if (full)
        hipLaunchKernelGGL(pt::path_trace_async_kernel<true>, dim3(grid), dim3(64), lds, c->stream, K, A);
    else
        hipLaunchKernelGGL(pt::path_trace_async_kernel<false>, dim3(grid), dim3(64), lds, c->stream, K, A);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// ---- post chain ---------------------------------------------------------------------------------------------------------
// motion vectors -> Denoiser::denoise (non-split) -> tonemap of the denoised image, all on the
// context's stream (Scene::render_to_device, scene.cuh:1103-1127,1204).  History hand-over is a
// swap of the double-buffered sets (history moments AND the packed G-buffer); no device copies.
// 3 + atrous_iterations launches per frame: prep, temporal, variance, a-trous x N (the last one
// also writes the API's vec3 image and the RGB8 frame).
int run_denoiser(ptrt_ctx *c, const pt::KParams &K, unsigned char *rgb8) {
    const int W = c->rw, H = c->rh; // the render size (the denoiser was allocated for it)
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(256);
    const pt::DenoiseSettings &S = c->dn;
    const int prev = c->dn_cur, next = c->dn_cur ^ 1;
    // perfSettings.enableMotionVectors (scene.cuh:1103); when off the last vectors are reused
    if (c->mv_active)
        HIP_TRY(c, hipMemcpyAsync(c->dn_pvp, c->prev_view_proj, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pt::prep_kernel, grid, block, 0, c->stream, c->dn_g4[next], c->dn_motion, c->dn_cur4, K.accum,
                       K.normal, K.depth, W, H, c->cam.origin, c->cam.llc, c->cam.horizontal, c->cam.vertical, c->cam.u,
                       c->cam.v, c->cam.lens_radius, c->dn_pvp, c->mv_active, S.sky_depth_threshold, S.enable_firefly_suppression);
    hipLaunchKernelGGL(pt::temporal_kernel, grid, block, 0, c->stream, c->dn_h1[next], c->dn_h2[next], c->dn_cur4,
                       c->dn_h1[prev], c->dn_h2[prev], c->dn_motion, c->dn_g4[next], c->dn_g4[prev], K.object_id,
                       c->dn_hobj, S, c->dn_first ? 1 : 0, W, H);
    c->dn_cur = next;
    hipLaunchKernelGGL(pt::variance_kernel, grid, block, 0, c->stream, c->dn_c4[0], c->dn_h1[next], c->dn_h2[next],
                       c->dn_g4[next], K.object_id, c->dn_hobj, S.sky_depth_threshold, S.use_object_ids, W, H);
    const int steps[5] = {1, 2, 4, 8, 16};
    const int iters = S.atrous_iterations < 5 ? (S.atrous_iterations < 0 ? 0 : S.atrous_iterations) : 5;
    for (int i = 0; i < iters; ++i) {
        const float4 *in = c->dn_c4[i & 1];
        float4 *out = c->dn_c4[(i + 1) & 1];
        // a workgroup = 64 consecutive pixels x 4 rows of ONE row class (y mod step); the class is the fast block index
        const int s = steps[i];
        const dim3 agrid((W + pt::AT_W - 1) / pt::AT_W, (((H + s - 1) / s + pt::AT_ROWS - 1) / pt::AT_ROWS) * s);
        const size_t alds = pt::atrous_lds_bytes(s);
        const bool last = i == iters - 1;
        auto kern = last ? (c->atrous_exp ? pt::atrous_kernel<true, true> : pt::atrous_kernel<true, false>)
                         : (c->atrous_exp ? pt::atrous_kernel<false, true> : pt::atrous_kernel<false, false>);
        hipLaunchKernelGGL(kern, agrid, block, alds, c->stream, out, in, c->dn_g4[next], K.object_id, steps[i], S.sigma_luminance,
                           S.sky_depth_threshold, S.edge_depth_threshold, S.edge_normal_threshold, S.use_object_ids, W, H,
                           last ? c->dn_out : (float *)nullptr, last ? rgb8 : (unsigned char *)nullptr);
    }
    if (iters == 0)
        hipLaunchKernelGGL(pt::c4_to_output_kernel, grid, block, 0, c->stream, c->dn_c4[0], W, H, c->dn_out, rgb8);
    HIP_TRY(c, hipGetLastError());
    c->dn_first = false;
    return PTRT_OK;
}

// Step 5 of Scene::render_to_device (scene.cuh:1137-1183) on `image` (w x h, in place), with the
// reference's own pass list and sizes (see pt_post.hip.h); `rgb8` non-NULL: also tonemap the result.
int run_bloom(ptrt_ctx *c, float *image, int w, int h, unsigned char *rgb8) {
    std::vector<pt::BloomPass> passes;
    int mip_w = w, mip_h = h;
    const float *last = image;
    for (int i = 0; i < 6; ++i) {
        const int next_w = mip_w / 2, next_h = mip_h / 2;
        passes.push_back(pt::BloomPass{i == 0 ? 0 : 1, c->bl_mip[i], last, mip_w, mip_h, next_w, next_h});
        last = c->bl_mip[i];
        mip_w = next_w;
        mip_h = next_h;
    }
    for (int i = 4; i >= 0; --i) {
        mip_w *= 2;
        mip_h *= 2;
        passes.push_back(pt::BloomPass{2, c->bl_mip[i], c->bl_mip[i + 1], mip_w / 2, mip_h / 2, (mip_w / 2) * 2, (mip_h / 2) * 2});
    }
    const bool fuse_final = (w % 2) == 0; // else the reference's row stride 2*(w/2) is not the frame's
    if (!fuse_final)
        passes.push_back(pt::BloomPass{2, image, c->bl_mip[0], w / 2, h / 2, (w / 2) * 2, (h / 2) * 2});
    for (size_t k = 0; k < passes.size();) {
        // one workgroup beats a launch (~6 us) only for the smallest levels: measured 46 us for five passes of
        // up to 8 K pixels vs ~30 us as separate launches
        auto small = [&](size_t i) { return (size_t)passes[i].out_w * passes[i].out_h <= 4096; };
        if (small(k)) {
            pt::BloomSmallPasses S{};
            while (k < passes.size() && small(k) && S.n < 8)
                S.p[S.n++] = passes[k++];
            hipLaunchKernelGGL(pt::bloom_small_passes_kernel, dim3(1), dim3(1024), 0, c->stream, S);
        } else {
            const pt::BloomPass &P = passes[k++];
            hipLaunchKernelGGL(pt::bloom_pass_kernel, dim3((P.out_w + 63) / 64, (P.out_h + 3) / 4), dim3(256), 0, c->stream, P);
        }
    }
    const dim3 grid((w + 63) / 64, (h + 3) / 4), block(256);
    if (fuse_final)
        hipLaunchKernelGGL(pt::bloom_final_kernel, grid, block, 0, c->stream, image, c->bl_mip[0], w, h, w / 2, h / 2, rgb8);
    else if (rgb8)
        hipLaunchKernelGGL(pt::tonemap_only_kernel, grid, block, 0, c->stream, rgb8, image, w, h);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// ---- ptrt_render, step by step ----------------------------------------------------------------------------------------
// The caller is recording the context's stream into a hipGraph.
bool stream_capturing(ptrt_ctx *c) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess)
        (void)hipGetLastError();
    return cs != hipStreamCaptureStatusNone;
}

// Which of the two exact shapes of the queue modes' loop this frame runs (option "merged"); true while the choice is being
// sampled (the frame's launch is then timed and ordered behind the stream).
bool choose_loop_shape(ptrt_ctx *c, int spp, int max_depth, int geom) {
    // merged = -1: the two exact shapes of the queue modes' loop (shadow rays in their own traversal, or riding with the next
    // extension rays) take turns over a scene's frames 4-7 (the first four warm the clocks up); their kernel times (the event
    // ring) decide the rest at frame 8, which waits for frame 7 once
    bool tuning = false;
    const bool merged_possible = pair_mode(c, geom, true) == 4; // (only the queue mode over BLASes has the merged shape)
    c->last_merged_possible = merged_possible;
    c->merged_eff = c->merged > 0 ? 1 : 0;
    // (a caller recording this stream into a hipGraph: no host wait, no choice -- the default shape; asked only while the choice
    // is open: a driver call per frame otherwise)
    const bool capturing = c->merged < 0 && merged_possible && c->tune_choice < 0 && stream_capturing(c);
    if (c->merged < 0 && merged_possible && !capturing) {
        const unsigned long long key = ((((unsigned long long)c->n_geometry_uploads * 131 + (unsigned)spp) * 131 + (unsigned)max_depth) * 131 +
                                        (unsigned)(c->steal * 64 + c->fetch_min + c->csteal * 4096 + c->csteal_leaf_min * 65536)) * 131 + (unsigned)(c->leaf_min * 8 + c->leaf_pairs * 4 + c->lds_nodes * 2 + c->pair_trace);
        if (key != c->tune_key) {
            c->tune_key = key;
            c->tune_n = 0;
            c->tune_choice = -1;
        }
        if (c->tune_choice < 0 && c->tune_n < TUNE_WARM + 2 * TUNE_SAMPLES) { // warm-up frames, then merged / separate in turns
            c->merged_eff = c->tune_n >= TUNE_WARM && !((c->tune_n - TUNE_WARM) & 1);
            tuning = true;
        } else if (c->tune_choice < 0) { // the frame after the last sample: ONE host wait for that sample, once per scene and setting
            float t[2 * TUNE_SAMPLES] = {};
            bool ok = c->launches - c->tune_launch[0] < (unsigned long long)EV_RING - 8 &&
                      hipEventSynchronize(c->ev_ring[2 * (c->tune_launch[2 * TUNE_SAMPLES - 1] % EV_RING) + 1]) == hipSuccess;
            for (int i = 0; i < 2 * TUNE_SAMPLES && ok; ++i)
                ok = hipEventElapsedTime(&t[i], c->ev_ring[2 * (c->tune_launch[i] % EV_RING)], c->ev_ring[2 * (c->tune_launch[i] % EV_RING) + 1]) == hipSuccess;
            (void)hipGetLastError();
            float tm[TUNE_SAMPLES], ts[TUNE_SAMPLES];
            for (int i = 0; i < TUNE_SAMPLES; ++i) {
                tm[i] = t[2 * i];
                ts[i] = t[2 * i + 1];
            }
            std::sort(tm, tm + TUNE_SAMPLES);
            std::sort(ts, ts + TUNE_SAMPLES);
            // the separate-phase loop is the default; the merged one must be faster by TUNE_MIN_GAIN in the medians to replace it
            c->tune_choice = (ok && tm[TUNE_SAMPLES / 2] < ts[TUNE_SAMPLES / 2] * (1.0f - TUNE_MIN_GAIN)) ? 1 : 0;
            c->merged_eff = c->tune_choice;
            if (getenv("PTRT_DEBUG_LDS"))
                fprintf(stderr, "ptrt: merged loop median %.3f ms, separate %.3f ms -> %s\n", tm[TUNE_SAMPLES / 2], ts[TUNE_SAMPLES / 2],
                        c->tune_choice ? "merged" : "separate");
        } else {
            c->merged_eff = c->tune_choice;
        }
    }
    return tuning;
}

// PMODE 1: what a workgroup stages and how many tiles it takes (lds::pm1_choose, from the budgets of the occupancy the kernels
// are built for) -> its size in bytes; fills K.lds_* for pt::carve_pm1.  With the simple materials the kernel exists for one
// tile per workgroup at five waves per SIMD and for TWO tiles at six (option pm1_wg: 0 = the larger one if the scene fits its
// LDS budget, 1 / 2 force).
pt::lds::Pm1Choice pm1_choice(int meshes, int tri_slots, int n_lights, bool full, int stage, int sample_sync, int lds_pad, int pm1_wg) {
    // (the lanes' blue-noise slots, 512 bytes per wave, are only worth their LDS while [A] runs in every iteration: with the
    // samples in step it runs once per sample for the whole wave and reads the table itself -- room for the materials)
    const bool stage_bn = sample_sync == 0;
    return pt::lds::pm1_choose(meshes, tri_slots, n_lights, full, stage, stage_bn, lds_pad, pm1_wg, (size_t)pt::lds_per_workgroup(1, false, 2),
                               (size_t)pt::lds_per_wave(1, full), 64 * 1024);
}
size_t pm1_layout(ptrt_ctx *c, pt::KParams &K, bool full, int grid, int &pm1_wg) {
    const pt::lds::Pm1Choice P = pm1_choice(c->pair_meshes, c->pair_tri_slots, c->n_lights, full, c->stage, K.sample_sync, c->lds_pad, c->pm1_wg);
    K.lds_extra = P.s.lds_extra;
    K.lds_flags = P.s.lds_flags;
    K.lds_wave = P.s.lds_wave;
    K.lds_wave_bytes = P.s.lds_wave_bytes;
    pm1_wg = P.wg;
    K.n_tiles = grid;
    return P.total;
}

// What one ptrt_render call has decided about its trace: the loop shape that renders the frame and the facts its launch
// needs.  plan_frame makes the decision, once; plan_overlap and launch_frame read it.
struct FramePlan {
    enum Shape {
        TILES,     // one 8x8 tile per 64-thread workgroup (launch_trace), by PMODE and GEOM: the only shape that can be split
        PM1_WG2,   // path_trace_kernel<0, false, 1, 2>: PMODE 1, two tiles per workgroup
        LDS_NODES, // path_trace_kernel<1, *, 2, 4>: PMODE 2, four tiles per workgroup (option lds_nodes)
        WAVEFRONT, // trace / shade stages (run_wavefront)
        ASYNC,     // asynchronous-lane megakernel (run_async)
    } shape = TILES;
    int geom = 0, pmode = 0, pm1_wg = 1; // pm1_wg: tiles per workgroup of PMODE 1's layout (also when another shape renders the frame)
    bool full = false, tuning = false;   // full materials; the loop-shape choice is being sampled (choose_loop_shape)
    int tiles_y = 0, grid = 0;           // rows of tiles, tiles
    size_t lds = 0;                      // dynamic LDS bytes of the launch that runs, whichever shape it is
    bool one_launch_only() const { return shape != TILES; }
};

// Decides the frame's loop shape and fills K's per-frame choices.  The read-only options (pmode, merged_eff, *_eff) report the
// pair mode and the options even when the asynchronous lanes or the stages render the frame.  It fails (lds_nodes over 64 KiB)
// before ptrt_render records an event or updates touched / prev_*: a refused frame leaves fewer traces than it used to.
int plan_frame(ptrt_ctx *c, pt::KParams &K, int spp, int max_depth, FramePlan &P) {
    // Samples in step (path_trace_kernel [A], K.sample_sync): the lanes of a wave start a sample together, so a wave's lanes sit at the
    // same bounce -- a first hit samples no light and the whole wave skips [C2] / [D] in that iteration, [A] runs once per sample
    // for 64 lanes instead of every iteration for a quarter of them -- at the price of lanes that wait for the longest path of
    // the sample.  Pays while most paths run to the depth limit: Cornell 4 bounces 1.764 -> 1.638 ms (3 bounces 1.42 -> 1.26),
    // `many` 15.9 -> 14.8; loses once Russian roulette thins the wave (5 bounces 1.966 -> 1.980, 6: 2.10 -> 2.31, 8: 2.26 ->
    // 2.80); scenes of short paths are indifferent once a path's last vertex costs nothing (showcase 3.90 -> 3.90; the fluid frame
    // gains 3 %), so the depth limit alone decides.  Releasing the waiting lanes early (when few are still under way, or when many
    // wait) was measured at every threshold and is worse than both extremes.
    K.sample_sync = c->sample_sync >= 0 ? c->sample_sync : (max_depth <= 4 ? 1 : 0);
    c->sample_sync_eff = K.sample_sync;
    P.tiles_y = (K.rows + 7) / 8;
    P.grid = K.tiles_x * P.tiles_y;
    P.geom = pick_geom(c);
    P.full = c->mats_full || c->force_full;
    P.tuning = choose_loop_shape(c, spp, max_depth, P.geom);
    const int pmode = P.pmode = pair_mode(c, P.geom, c->merged_eff != 0);
    c->last_pmode = pmode;
    // Dense root tests (build_pairs_dense): a call with R <= 32 live rays runs ceil(M / G) slab rounds instead of M, G = 2 or 4,
    // for one ballot, a 32-byte LDS table and seven or eight ds_bpermute -- about what half a slab round issues.  With fewer
    // than four meshes in the leaf G = 2 saves at most one round: not worth the branch.  Decided here, once per frame, from the
    // scene alone.
    K.pm1_dense = (pmode == 1 && (c->pm1_dense_roots >= 0 ? c->pm1_dense_roots : (c->pair_meshes >= 4 ? 1 : 0))) ? 1 : 0;
    c->pm1_dense_roots_eff = K.pm1_dense;
    c->pm1_full_leaf_eff = pmode == 1 ? K.pm1_full_leaf : 0;
    c->pm1_lane_groups_eff = pmode == 1 ? K.pm1_groups : 0;
    // (PMODE 4's trace_merged runs its own root tests ahead of build_pairs_merged and does not read the flag)
    c->plain_leaf_eff = (pmode == 1 || pmode == 2) ? K.plain_leaf : 0;
    // (round 2: the merged loop was at its best WITHOUT shadow-ray subtree stealing, 3.98 vs 4.17 ms on the showcase frame -- its
    // yields served ten shadow pairs at the price of sixty closest-hit walks; with the closest-hit walks stolen from as well the
    // yields pay for both kinds: 3.19 ms with, 3.49 without)
    if (c->merged < 0 && pmode == 4 && c->csteal == 0)
        K.steal = 0;
    const size_t lds = trace_lds_bytes(c, P.geom, pmode);
    const size_t lds_main = pmode == 1 ? pm1_layout(c, K, P.full, P.grid, P.pm1_wg) : lds + (size_t)c->lds_pad;
    if (c->launches == 0 && getenv("PTRT_DEBUG_LDS"))
        fprintf(stderr, "ptrt: pmode %d, %d meshes in the leaf, %d triangle slots, stack %d, LDS %zu + %zu bytes per workgroup\n", pmode,
                c->pair_meshes, c->pair_tri_slots, c->stack_entries, lds, lds_main - lds);
    // (the precedence is the order of the lines; a new loop shape is one more)
    P.shape = async_applicable(c)                                 ? FramePlan::ASYNC
              : wavefront_applicable(c, spp, max_depth)           ? FramePlan::WAVEFRONT
              : pmode == 1 && P.pm1_wg == 2                       ? FramePlan::PM1_WG2
              : pmode == 2 && c->lds_nodes && c->stack_entries > 0 ? FramePlan::LDS_NODES
                                                                  : FramePlan::TILES;
    // to_world's frame from the per-triangle table: PMODE 1's megakernel alone (K.tri_frames is null out of make_params)
    if (pmode == 1 && (P.shape == FramePlan::TILES || P.shape == FramePlan::PM1_WG2) && c->tri_frames != 0 && c->tri_frames_ok && !c->any_transform)
        K.tri_frames = c->d_tri_frames;
    c->tri_frames_eff = K.tri_frames ? 1 : 0;
    switch (P.shape) {
    case FramePlan::ASYNC: P.lds = async_lds_bytes(c); break;
    case FramePlan::WAVEFRONT: P.lds = wavefront_lds_bytes(c); break;
    case FramePlan::PM1_WG2: P.lds = lds_main; break;
    case FramePlan::LDS_NODES: P.lds = lds_nodes_bytes(c); break;
    case FramePlan::TILES: P.lds = pmode ? lds_main : lds; break; // (PMODE 0 takes no lds_pad)
    }
    if (P.shape == FramePlan::LDS_NODES && P.lds > 64 * 1024)
        return fail(c, PTRT_E_INVALID, "lds_nodes: %zu bytes of LDS per workgroup", P.lds);
    return PTRT_OK;
}

// PMODE 3: the mesh-record heads in TLAS-leaf order (a 136-thread copy, outside the timed kernel).  They only change with the
// mesh records: heads_fresh.  `also_if_touched`: ptrt_render, which regathers as well after any touching entry point -- a frame
// recorded into a caller's graph sets `touched` and leaves heads_fresh; a ray query sets `touched` itself and goes by heads_fresh.
int refresh_tlas_heads(ptrt_ctx *c, bool also_if_touched) {
    if (c->heads_fresh && !(also_if_touched && c->touched))
        return PTRT_OK;
    c->heads_fresh = true;
    hipLaunchKernelGGL(pt::gather_tlas_heads_kernel, dim3((c->n_tlas_index + 63) / 64), dim3(64), 0, c->stream,
                       c->d_mesh_recs, c->d_inst_pre, c->d_tlas_mesh_ids, c->n_tlas_index, c->d_tlas_heads,
                       c->inst_pre_ok ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// Whether this frame may overlap its predecessor on the device, and the waits that make it safe.  Sets c->split_eff /
// c->pipelined_last, swaps in the second HDR / G-buffer set for a frame with a post chain, records the stream's head for the
// next frame.  `splittable`: the frame's kernel can be dealt to several launches at all; `recording`: the caller is capturing
// the stream into a hipGraph.
struct OverlapPlan {
    bool splittable = false, recording = false;
};
int plan_overlap(ptrt_ctx *c, pt::KParams &K, const FramePlan &P, bool post, bool scaled, void *out_rgb8, int out_is_device,
                 OverlapPlan &plan) {
    // Options "split" / "pipeline": frame pipelining.  A frame ends with a tail -- its last waves drain while most of the chip
    // idles, then the next launch ramps up: ~8 % of a 1080p Cornell frame.  With the frame's rows of tiles dealt to `split`
    // launches on auxiliary streams, launch i of frame N + 1 touches the same pixels (generator states, accumulators, image
    // rows) as launch i of frame N and nothing else of that frame, so it only has to follow THAT launch, which it does on
    // its stream; it need not wait for the stream the caller sees, onto which every frame is joined by events.  That is safe
    // only while nothing else has a claim on what it reads or overwrites: no entry point that could have enqueued device work
    // or changed device data since the last frame (`touched`, set by ctx_live), no reduced render size (a post chain at full
    // size gets a second set of HDR image and G-buffers: below), no pointers into the context's buffers in the caller's hands,
    // no loop-shape sampling (it times launches), not while the caller records the stream into a graph, and a DEVICE target
    // other than the previous frame's (whatever consumes that one on the stream is still entitled to it).
    // A frame that cannot overlap is ONE launch on the context's stream, as ever (concurrent launches of one frame buy
    // nothing: Cornell 1.85 vs 1.82 ms) -- followed by an event the next frame's launches wait for if that one can.
    // What an overlapping frame DOES wait for, besides its predecessor's launches: everything that was on the stream when the
    // PREVIOUS ptrt_render was called -- the consumers of the frame before that one, whose target a double-buffering caller
    // hands in again now.  (head_ev alternates: [head_n & 1] is recorded now, the other one is the previous call's.)
    c->split_eff = 1;
    c->pipelined_last = false;
    const int n_split = c->split < ptrt_ctx::MAX_SPLIT ? c->split : ptrt_ctx::MAX_SPLIT;
    const bool splittable = c->pipeline && n_split > 1 && P.tiles_y >= 2 * n_split && !P.one_launch_only();
    // (a caller recording the stream into a hipGraph: the bookkeeping events below would become nodes of its graph, and a replay
    // never passes through here -- such a frame is one ordered launch, and so is the first frame after it)
    const bool recording = splittable && stream_capturing(c);
    // (the previous frame's post chain reads the HDR image and G-buffers this frame's trace would overwrite: a frame WITH a chain
    // writes the other set, below; one without -- the chain was switched off in between -- waits for the stream instead.  A
    // changed number of launches moves the rows between the auxiliary streams: only a one-launch frame may precede it.)
    const bool may_overlap = splittable && !recording && !c->touched && !c->escaped && !P.tuning && !scaled && out_rgb8 &&
                             out_is_device && out_rgb8 != c->prev_out && c->prev_stream == c->stream &&
                             (c->prev_split == n_split || c->prev_split == 1) && !(c->prev_post && !post);
    // (the second set of HDR image and G-buffers: all four or none -- a failed allocation leaves the frame unpipelined)
    bool alt_ok = true;
    if (may_overlap && post && !c->alt_accum) {
        float *a = nullptr, *nrm = nullptr, *d = nullptr;
        int *o = nullptr;
        alt_ok = hipMalloc((void **)&a, c->npix * 3 * sizeof(float)) == hipSuccess &&
                 hipMalloc((void **)&nrm, c->npix * 3 * sizeof(float)) == hipSuccess &&
                 hipMalloc((void **)&d, c->npix * sizeof(float)) == hipSuccess &&
                 hipMalloc((void **)&o, c->npix * sizeof(int)) == hipSuccess;
        if (alt_ok) {
            c->alt_accum = a;
            c->alt_normal = nrm;
            c->alt_depth = d;
            c->alt_object_id = o;
        } else {
            (void)hipGetLastError();
            dfree(a);
            dfree(nrm);
            dfree(d);
            dfree(o);
        }
    }
    if (may_overlap && alt_ok) {
        for (int i = 0; i < n_split; ++i)
            if (!c->aux_stream[i]) {
                HIP_TRY(c, hipStreamCreateWithFlags(&c->aux_stream[i], hipStreamNonBlocking));
                HIP_TRY(c, hipEventCreateWithFlags(&c->split_join[i], hipEventDisableTiming));
            }
        for (int i = 0; i < n_split; ++i) {
            if (c->prev_split != n_split) // the previous frame was one launch on the stream: follow it (and only it)
                HIP_TRY(c, hipStreamWaitEvent(c->aux_stream[i], c->split_fork, 0));
            if (c->head_ev[(c->head_n + 1) & 1])
                HIP_TRY(c, hipStreamWaitEvent(c->aux_stream[i], c->head_ev[(c->head_n + 1) & 1], 0));
        }
        if (post) {
            // the post chain of the previous frame may still be reading the HDR image and the G-buffers on the stream:
            // this frame's trace writes the OTHER set (its own post chain, enqueued behind the join, reads that one)
            std::swap(c->d_accum, c->alt_accum);
            std::swap(c->d_normal, c->alt_normal);
            std::swap(c->d_depth, c->alt_depth);
            std::swap(c->d_object_id, c->alt_object_id);
            K.accum = c->d_accum;
            K.normal = c->d_normal;
            K.depth = c->d_depth;
            K.object_id = c->d_object_id;
        }
        c->split_eff = n_split;
        c->pipelined_last = true;
    }
    if (splittable && !recording) { // the stream's head at this call, for the NEXT frame
        hipEvent_t &he = c->head_ev[c->head_n & 1];
        if (!he)
            HIP_TRY(c, hipEventCreateWithFlags(&he, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(he, c->stream));
        ++c->head_n;
    }
    plan = {splittable, recording};
    return PTRT_OK;
}

// The frame's trace launch(es) in the loop shape plan_frame chose.
int launch_frame(ptrt_ctx *c, pt::KParams &K, const FramePlan &P, int spp, int max_depth) {
    int rc = PTRT_OK;
    switch (P.shape) {
    case FramePlan::ASYNC:
        if ((rc = run_async(c, K, P.full, P.lds)))
            return rc;
        c->last_mode = 2;
        break;
    case FramePlan::WAVEFRONT:
        if ((rc = run_wavefront(c, K, P.full, P.lds, spp, max_depth)))
            return rc;
        c->last_mode = 1;
        break;
    case FramePlan::PM1_WG2:
        c->split_eff = 1;
        hipLaunchKernelGGL((pt::path_trace_kernel<0, false, 1, 2>), dim3((P.grid + 1) / 2), dim3(128), P.lds, c->stream, K);
        break;
    case FramePlan::LDS_NODES:
        K.n_tiles = P.grid;
        K.top_off = c->lds_nodes == 2 ? 1 : 0;
        if (P.full)
            hipLaunchKernelGGL((pt::path_trace_kernel<1, true, 2, 4>), dim3((P.grid + 3) / 4), dim3(256), P.lds, c->stream, K);
        else
            hipLaunchKernelGGL((pt::path_trace_kernel<1, false, 2, 4>), dim3((P.grid + 3) / 4), dim3(256), P.lds, c->stream, K);
        break;
    case FramePlan::TILES:
        switch (P.pmode ? P.pmode : -P.geom) { // PMODE 1..4 (the pair walks do not depend on GEOM: one instantiation each), else PMODE 0 by GEOM
        case 1: rc = launch_trace<0, 1>(c, K, P.full, P.grid, P.lds); break;
        case 2: rc = launch_trace<1, 2>(c, K, P.full, P.grid, P.lds); break;
        case 3: rc = launch_trace<2, 3>(c, K, P.full, P.grid, P.lds); break;
        case 4: rc = launch_trace<1, 4>(c, K, P.full, P.grid, P.lds); break;
        case 0: rc = launch_trace<0, 0>(c, K, P.full, P.grid, P.lds); break;
        case -1: rc = launch_trace<1, 0>(c, K, P.full, P.grid, P.lds); break;
        default: rc = launch_trace<2, 0>(c, K, P.full, P.grid, P.lds); break;
        }
        if (rc)
            return rc;
        break;
    }
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// Joins a split frame onto the context's stream and notes what the NEXT frame may follow.
int join_frame(ptrt_ctx *c, const OverlapPlan &plan, bool post) {
    for (int i = 0; c->split_eff > 1 && i < c->split_eff; ++i) { // join: what follows on the context's stream follows every launch
        HIP_TRY(c, hipEventRecord(c->split_join[i], c->aux_stream[i]));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->split_join[i], 0));
    }
    c->prev_split = 0;
    c->prev_post = post;
    if (plan.recording) {
        c->touched = true; // (what a replayed graph does to the buffers is not this call's to know: the next frame waits for the stream)
    } else if (c->split_eff > 1) {
        c->prev_split = c->split_eff;
    } else if (plan.splittable && c->last_mode == 0) { // one launch on the stream: the point the next frame's launches may follow
        if (!c->split_fork)
            HIP_TRY(c, hipEventCreateWithFlags(&c->split_fork, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->split_fork, c->stream));
        c->prev_split = 1;
    }
    return PTRT_OK;
}

// The tail ptrt_render and ptrt_post_frame share behind the HDR image K.accum (`current_image` of Scene::render_to_device,
// scene.cuh:1086): denoiser, bloom, up-scale, the presentation ring's mark, the copy to host memory with its wait.  The stage
// that produces the final HDR image also tonemaps it into `frame_rgb8`; earlier stages skip theirs.
int finish_frame(ptrt_ctx *c, const pt::KParams &K, unsigned char *frame_rgb8, bool scaled, bool mark_ring, void *out_rgb8,
                 int out_is_device) {
    const bool denoise = c->dn_on && c->dn_active, bloom = c->bloom_on != 0;
    float *current = K.accum;
    if (denoise) {
        if (int rc = run_denoiser(c, K, (bloom || scaled) ? nullptr : frame_rgb8))
            return rc;
        current = c->dn_out;
    }
    if (bloom) {
        if (int rc = run_bloom(c, current, c->rw, c->rh, scaled ? nullptr : frame_rgb8))
            return rc;
    }
    if (scaled) { // up-scale into the full-size colour buffer (scene.cuh:1192-1201) + tonemap
        hipLaunchKernelGGL(pt::upscale_tonemap_kernel, dim3((c->W + 63) / 64, (c->H + 3) / 4), dim3(256), 0, c->stream,
                           c->d_accum, current, c->W, c->H, c->rw, c->rh, frame_rgb8);
        HIP_TRY(c, hipGetLastError());
    }
    if (mark_ring)
        ring_mark_rendered(out_rgb8, c->stream);
    if (out_rgb8 && !out_is_device) {
        HIP_TRY(c, hipMemcpyAsync(out_rgb8, c->d_rgb8, c->npix * 3, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return PTRT_OK;
}

} // namespace

extern "C" {

int ptrt_render(ptrt_ctx *c, int frame_index, int spp, int max_depth, void *out_rgb8, int out_is_device) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_render: bad context");
    if (!c->have_geometry || !c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "ptrt_render: %s not uploaded", c->have_geometry ? "materials" : "geometry");
    if (c->n_materials < c->n_meshes)
        return fail(c, PTRT_E_NOT_READY, "ptrt_render: %d materials for %d meshes", c->n_materials, c->n_meshes);
    if (!c->rng_ready)
        return fail(c, PTRT_E_NOT_READY, "ptrt_render: generator states not initialised (ptrt_reset_rng)");
    if (spp < 1 || max_depth < 1 || spp > 32767 || max_depth > 32767) // (a lane keeps its sample index and bounce in one register's halves)
        return fail(c, PTRT_E_INVALID, "ptrt_render: spp=%d max_depth=%d (1..32767)", spp, max_depth);
    if (frame_index < 0 || frame_index > INT_MAX - spp) // (sample s of the frame indexes the jitter table with (frame_index + s) % 16)
        return fail(c, PTRT_E_INVALID, "ptrt_render: frame_index=%d", frame_index);
    if (int rc = set_device(c))
        return rc;
    pt::KParams K = make_params(c);
    K.spp = spp;
    K.max_depth = max_depth;
    K.tile_run = c->tile_run;
    K.frame_count = frame_index;
    unsigned char *frame_rgb8 = (out_rgb8 && out_is_device) ? (unsigned char *)out_rgb8 : c->d_rgb8;
    const bool scaled = c->scaled(), denoise = c->dn_on && c->dn_active, bloom = c->bloom_on != 0;
    // PTRT_OUT_DEVICE_FRAME: out_rgb8 is the whole W x H frame on this device; a band / strip context writes its rows where
    // they belong in it -- no image of its own, nothing for a tile farm to copy (ptrt_farm_*)
    const bool into_frame = out_rgb8 && out_is_device == PTRT_OUT_DEVICE_FRAME;
    if (into_frame && (denoise || bloom || scaled))
        return fail(c, PTRT_E_INVALID, "ptrt_render: PTRT_OUT_DEVICE_FRAME with the denoiser, bloom or a reduced render size");
    c->last_rgb8 = into_frame ? nullptr : frame_rgb8; // (a frame target is the caller's: ptrt_read_buffer(RGB8) has nothing to read)
    c->last_frame_target = into_frame ? out_rgb8 : nullptr;
    K.rgb8_frame = into_frame ? 1 : 0;
    K.rgb8 = (denoise || bloom || scaled) ? nullptr : frame_rgb8;
    if (c->count_rays)
        K.counters = c->d_counters;
    FramePlan P;
    if (int rc = plan_frame(c, K, spp, max_depth, P))
        return rc;
    if (P.pmode == 3)
        if (int rc = refresh_tlas_heads(c, true))
            return rc;
    const int slot = (int)(c->launches % EV_RING);
    const bool timing = c->time_kernels || P.tuning;
    c->ev_ms_known[slot] = false; // (the slot's events are recorded anew: the intervals kept of them are another frame's)
    for (int i = 0; i < ptrt_ctx::MAX_SPLIT; ++i)
        c->launch_ms_known[i][slot] = false;
    if (timing)
        HIP_TRY(c, hipEventRecord(c->ev_ring[2 * slot], c->stream));
    // frame pipelining (options "split" / "pipeline"): may this frame's launches follow the previous frame's instead of the stream?
    const bool post = denoise || bloom;
    OverlapPlan plan;
    if (int rc = plan_overlap(c, K, P, post, scaled, out_rgb8, out_is_device, plan))
        return rc;
    // Lane refill (launch_trace): where it was measured to pay.  Overlapping 1080p Cornell frames 1.67 -> 1.62 ms, 8 bounces 2.12
    // -> 1.88, 4K 6.65 -> 6.27; a frame alone on the chip ends in a long drain of half-empty persistent waves (1.81 -> 1.97),
    // short pixels finish before the refill pays for itself (1 spp: 0.43 -> 0.61), and beside a post chain the persistent waves
    // keep the chain's kernels waiting for a place on the chip (balanced preset 2.41 -> 2.50).
    // (And a launch must hold at least two tiles per persistent wave -- 1280 x 720 measured even, smaller frames lose.)
    const long per_launch = (long)P.grid / (c->split_eff > 1 ? c->split_eff : 1);
    const long resident = (long)c->n_cus * (c->persist > 0 ? c->persist : 4 * pt::waves_per_simd(1, P.full, 1));
    c->refill_eff = P.pmode == 1 && P.pm1_wg == 1 &&
                    (c->refill == 2 || (c->refill == 1 && c->pipelined_last && !P.full && !post &&
                                        (long)spp * max_depth >= 16 && per_launch >= 2 * resident));
    c->prev_out = (out_rgb8 && out_is_device) ? out_rgb8 : nullptr;
    c->prev_stream = c->stream;
    c->touched = false;
    c->last_mode = 0;
    c->launch_timed[slot] = 0; // (launch_trace sets it for the launches it puts events around; the other loop shapes leave none)
    if (int rc = launch_frame(c, K, P, spp, max_depth))
        return rc;
    if (int rc = join_frame(c, plan, post))
        return rc;
    if (timing)
        HIP_TRY(c, hipEventRecord(c->ev_ring[2 * slot + 1], c->stream));
    if (P.tuning) {
        if (c->tune_n >= TUNE_WARM)
            c->tune_launch[c->tune_n - TUNE_WARM] = c->launches;
        ++c->tune_n;
    }
    c->launches++;
    c->timed = timing;
    // (a frame shared by several contexts is marked by whoever joins them)
    return finish_frame(c, K, frame_rgb8, scaled, out_rgb8 && out_is_device && !into_frame, out_rgb8, out_is_device);
}

// Presenting rank of the tile farm: steps 3-7 of Scene::render_to_device (motion vectors,
// denoiser, bloom, tonemap; scene.cuh:1103-1208) of a FULL-FRAME context over a frame whose HDR image and
// G-buffers were rendered elsewhere -- the band contexts -- and gathered into device memory.
int ptrt_post_frame(ptrt_ctx *c, const float *accum, const float *normal, const float *depth, const int32_t *object_id,
                    void *out_rgb8, int out_is_device) {
    if (!ctx_live(c) || !accum || !normal || !depth || !object_id)
        return fail(c, PTRT_E_INVALID, "ptrt_post_frame: bad argument");
    if (c->rows != c->H || c->y0 != 0)
        return fail(c, PTRT_E_INVALID, "ptrt_post_frame: needs a full-frame context (this one holds rows %d..%d of %d)", c->y0,
                    c->y0 + c->rows, c->H);
    if (c->scaled())
        return fail(c, PTRT_E_INVALID, "ptrt_post_frame: the frame must have the context's size (render size %dx%d != %dx%d)",
                    c->rw, c->rh, c->W, c->H);
    const bool denoise = c->dn_on && c->dn_active, bloom = c->bloom_on != 0;
    if (!denoise && !bloom)
        return fail(c, PTRT_E_INVALID, "ptrt_post_frame: neither denoiser nor bloom is enabled (gather the RGB8 bands instead)");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_accum, accum, c->npix * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_normal, normal, c->npix * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_depth, depth, c->npix * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_object_id, object_id, c->npix * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    pt::KParams K = make_params(c);
    unsigned char *frame_rgb8 = (out_rgb8 && out_is_device) ? (unsigned char *)out_rgb8 : c->d_rgb8;
    c->last_rgb8 = frame_rgb8;
    return finish_frame(c, K, frame_rgb8, false, out_rgb8 && out_is_device, out_rgb8, out_is_device);
}

} // extern "C"

// The duration of the frame whose events slot `slot` of ev_ring holds (both complete): asked of the runtime once, then kept.
static int slot_ms(ptrt_ctx *c, int slot, float *ms) {
    if (!c->ev_ms_known[slot]) {
        HIP_TRY(c, hipEventElapsedTime(&c->ev_ms[slot], c->ev_ring[2 * slot], c->ev_ring[2 * slot + 1]));
        c->ev_ms_known[slot] = true;
    }
    *ms = c->ev_ms[slot];
    return PTRT_OK;
}

extern "C" {

int ptrt_last_kernel_ms(ptrt_ctx *c, float *trace_ms, float *tonemap_ms) {
    if (!ctx_live(c) || !c->timed)
        return fail(c, PTRT_E_NOT_READY, "ptrt_last_kernel_ms: nothing rendered yet");
    if (int rc = set_device(c))
        return rc;
    const int slot = (int)((c->launches - 1) % EV_RING);
    HIP_TRY(c, hipEventSynchronize(c->ev_ring[2 * slot + 1]));
    float ms = 0.0f;
    if (int rc = slot_ms(c, slot, &ms))
        return rc;
    if (trace_ms)
        *trace_ms = ms;
    if (tonemap_ms)
        *tonemap_ms = 0.0f; // the tonemap is fused into the path-trace kernel
    return PTRT_OK;
}

int ptrt_kernel_ms_history(ptrt_ctx *c, float *out_ms, int max_n) {
    if (!ctx_live(c) || !out_ms || max_n < 0)
        return fail(c, PTRT_E_INVALID, "ptrt_kernel_ms_history: bad argument");
    if (int rc = set_device(c))
        return rc;
    if (!c->time_kernels)
        return 0; // (option time_kernels = 0: no events were recorded)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long n = c->launches < (unsigned long long)EV_RING ? c->launches : EV_RING;
    if (n > (unsigned long long)max_n)
        n = max_n;
    for (unsigned long long i = 0; i < n; ++i) {
        const int slot = (int)((c->launches - n + i) % EV_RING);
        if (int rc = slot_ms(c, slot, &out_ms[i]))
            return rc;
    }
    return (int)n;
}

// Durations of the LAUNCHES of the last frames that were dealt to the auxiliary streams with option "time_launches" on, oldest
// first: trace_ms[k] = the path-trace kernel of launch k, tail_ms[k] = from its end to the end of the tonemap pass behind it
// (lane refill; 0 otherwise).  A frame of `split` launches contributes `split` entries.  Waits for the stream.
int ptrt_launch_ms_history(ptrt_ctx *c, float *trace_ms, float *tail_ms, int max_n) {
    if (!ctx_live(c) || !trace_ms || max_n < 0)
        return fail(c, PTRT_E_INVALID, "ptrt_launch_ms_history: bad argument");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long frames = c->launches < (unsigned long long)EV_RING ? c->launches : EV_RING;
    // newest first, then reversed into the caller's arrays
    std::vector<float> a, b;
    for (unsigned long long f = 0; f < frames && (int)a.size() < max_n; ++f) {
        const int slot = (int)((c->launches - 1 - f) % EV_RING);
        if (!c->launch_timed[slot])
            break; // (the run of timed frames ends here)
        for (int i = ptrt_ctx::MAX_SPLIT - 1; i >= 0 && (int)a.size() < max_n; --i)
            if ((c->launch_timed[slot] >> i) & 1) {
                float t = 0.0f, u = 0.0f;
                hipEvent_t *ev = &c->launch_ev[i][3 * slot];
                HIP_TRY(c, hipEventSynchronize(ev[2]));
                if (!c->launch_ms_known[i][slot]) {
                    HIP_TRY(c, hipEventElapsedTime(&c->launch_ms[i][slot][0], ev[0], ev[1]));
                    HIP_TRY(c, hipEventElapsedTime(&c->launch_ms[i][slot][1], ev[1], ev[2]));
                    c->launch_ms_known[i][slot] = true;
                }
                t = c->launch_ms[i][slot][0];
                u = c->launch_ms[i][slot][1];
                a.push_back(t);
                b.push_back(u);
            }
    }
    const int n = (int)a.size();
    for (int k = 0; k < n; ++k) {
        trace_ms[k] = a[n - 1 - k];
        if (tail_ms)
            tail_ms[k] = b[n - 1 - k];
    }
    return n;
}

} // extern "C"
