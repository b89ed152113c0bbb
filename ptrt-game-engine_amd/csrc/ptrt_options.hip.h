// ptrt_options.hip.h -- the tuning / diagnostics knobs by name (ptrt_set_option, ptrt_get_option) and the test and
// profiling hooks (ptrt_debug_*).  Included by ptrt_capi.hip.
#pragma once

namespace {

// The exhaustive *_check hooks: nine zeroed words on the device, the check kernel that `launch` enqueues on the context's
// stream over them, and the words back.
template <class Launch> int run_check(ptrt_ctx *c, unsigned int *out9, Launch launch) {
    if (int rc = set_device(c))
        return rc;
    DeviceTemp<unsigned int> d;
    HIP_TRY(c, d.alloc(9));
    HIP_TRY(c, hipMemset(d.p, 0, 9 * sizeof(unsigned int)));
    launch(d.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out9, d.p, 9 * sizeof(unsigned int), hipMemcpyDeviceToHost));
    return PTRT_OK;
}

// How ptrt_set_option turns a caller's value into the stored one.
enum OptPolicy {
    OPT_READ_ONLY, // a fact about the last launch: ptrt_set_option refuses the name
    OPT_BOOL,      // value ? 1 : 0
    OPT_REJECT,    // PTRT_E_INVALID outside [lo, hi]
    OPT_CLAMP,     // to [lo, hi]
    OPT_MASK,      // value & hi
    OPT_TRISTATE,  // negative -> -1 (choose), else 0 / 1
    OPT_SNAP_124,  // <= 0 -> 0, else the largest of 1, 2, 4 not above it
    OPT_LANES,     // -1 (choose) or a power of four up to 64 -- 1, 4, 16, 64; PTRT_E_INVALID otherwise
};

// One row per name: both entry points walk this table.  `field` is where the value lives; the few entries that are computed
// or touch more than one field have `get` / `set` instead (or beside it).
struct Option {
    const char *name;
    int ptrt_ctx::*field;
    OptPolicy policy;
    long long lo, hi; // OPT_REJECT, OPT_CLAMP: the range; OPT_MASK: hi is the mask (lo unused)
    long long (*get)(const ptrt_ctx *);
    void (*set)(ptrt_ctx *, int);
};

const Option OPTIONS[] = {
    {"count_rays", &ptrt_ctx::count_rays, OPT_BOOL},
    {"force_geom", &ptrt_ctx::force_geom, OPT_REJECT, -1, 2}, // -1 auto; 1 / 2 force a more general traversal variant (tests)
    {"force_full", &ptrt_ctx::force_full, OPT_BOOL},
    {"pair_trace", &ptrt_ctx::pair_trace, OPT_BOOL}, // 0: lock-step mesh loop instead of (ray, mesh) pair compaction (A/B, tests)
    {"steal", &ptrt_ctx::steal, OPT_REJECT, 0, 64}, // PMODE 2 shadow rays: 0 = no subtree stealing; n = node steps between steal rounds
    {"csteal", &ptrt_ctx::csteal, OPT_REJECT, 0, 64}, // PMODE 2 closest hit: 0 = no subtree stealing; n = node steps between steal rounds (verified: same bits)
    {"atrous_exp", &ptrt_ctx::atrous_exp, OPT_BOOL},
    {"csteal_follow", &ptrt_ctx::csteal_follow, OPT_BOOL},
    {"csteal_leaf_min", &ptrt_ctx::csteal_leaf_min, OPT_REJECT, 1, 64},
    {"csteal_min", &ptrt_ctx::csteal_min, OPT_REJECT, 0, 1024},
    // PMODE 2 in 4-wave workgroups with the BLAS top levels staged in LDS (A/B, tests) (2: the larger workgroups without reading the staged nodes)
    {"lds_nodes", &ptrt_ctx::lds_nodes, OPT_CLAMP, 0, 2},
    {"merged", &ptrt_ctx::merged, OPT_TRISTATE}, // PMODE 4 instead of 2: shadow rays ride with the next extension rays (A/B, tests)
    {"leaf_pairs", &ptrt_ctx::leaf_pairs, OPT_BOOL}, // PMODE 2: 0 = every lane walks its own leaf (A/B, tests)
    {"lds_pad", &ptrt_ctx::lds_pad, OPT_REJECT, 0, 32768}, // extra bytes of LDS per workgroup: fewer waves per CU (A/B of the occupancy, tests)
    {"time_kernels", &ptrt_ctx::time_kernels, OPT_BOOL}, // 0: no start / stop events around the trace kernel (two driver calls per frame; ptrt_kernel_ms_history then has nothing)
    {"time_launches", &ptrt_ctx::time_launches, OPT_BOOL}, // 1: events around every launch of a frame dealt to the auxiliary streams (ptrt_launch_ms_history)
    {"tm_prio", &ptrt_ctx::tm_prio, OPT_MASK, 0, 3}, // lane refill's tonemap pass: | 1 on a stream of the highest priority, | 2 its waves at s_setprio 3
    {"pipeline", &ptrt_ctx::pipeline, OPT_BOOL}, // 1 (default): consecutive frames may overlap on the device when that is safe (ptrt_render); 0: never
    {"persist", &ptrt_ctx::persist, OPT_CLAMP, 0, INT_MAX},
    {"sample_sync", &ptrt_ctx::sample_sync, OPT_TRISTATE},
    {"pm1_dense_roots", &ptrt_ctx::pm1_dense_roots, OPT_TRISTATE}, // PMODE 1: root-box tests of a half-empty wave dealt over all lanes
    {"pm1_full_leaf", &ptrt_ctx::pm1_full_leaf, OPT_TRISTATE}, // PMODE 1: triangle loops without partial-leaf handling when every leaf is full (0: never)
    {"pm1_lane_groups", &ptrt_ctx::pm1_lane_groups, OPT_TRISTATE}, // PMODE 1: a pair-list tail's lanes per pair from the leaf's divisors, by the upload's plan (0: the 2^sh rule)
    {"plain_leaf", &ptrt_ctx::plain_leaf, OPT_TRISTATE}, // PMODE 1, 2: no TLAS root test, no instance arithmetic per pair batch, where the upload found the leaf plain (0: never; 1 does not force it)
    {"tri_frames", &ptrt_ctx::tri_frames, OPT_TRISTATE}, // PMODE 1 megakernel: to_world's tangent frame from the per-triangle table where the upload's normals stand and no mesh has a transform (0: never; 1 does not force it)
    {"tile_run", &ptrt_ctx::tile_run, OPT_REJECT, 0, 64}, // 0 (tile k on workgroup k) or the tiles per XCD and run, 1..64
    {"ticket_tiles", &ptrt_ctx::ticket_tiles, OPT_CLAMP, 1, 16},
    {"refill", &ptrt_ctx::refill, OPT_CLAMP, 0, 2},
    {"split", &ptrt_ctx::split, OPT_REJECT, 1, ptrt_ctx::MAX_SPLIT}, // tile rows of the frame dealt to that many concurrent launches of the megakernel (1 = one launch)
    {"tlas_rounds", &ptrt_ctx::tlas_rounds, OPT_BOOL}, // PMODE 3 shadow rays: one TLAS leaf per ray and fill instead of all of them (A/B, tests)
    {"pm1_wg", &ptrt_ctx::pm1_wg, OPT_REJECT, 0, 2}, // PMODE 1: one or two tiles per workgroup (0 = choose by the LDS budget; A/B, tests)
    {"stage", &ptrt_ctx::stage, OPT_MASK, 0, 7}, // PMODE 1: shading inputs staged in LDS (0 none; else jitter inputs, | 1 lights, | 2 materials; A/B, tests)
    {"pair_split", &ptrt_ctx::pair_split, OPT_BOOL}, // PMODE 1: 0 = one lane per pair also in batches that do not fill the wave (A/B, tests)
    {"async_lanes", &ptrt_ctx::async_lanes, OPT_BOOL}, // 1: persistent megakernel with asynchronous lanes for single-leaf-TLAS scenes
    {"shade_min", &ptrt_ctx::shade_min, OPT_REJECT, 1, 64}, // async_lanes: lanes that wait for the shading block before it runs
    // PMODE 2 and async_lanes: lanes waiting at a leaf that end the node loop
    {"leaf_min", &ptrt_ctx::leaf_min, OPT_REJECT, 1, 64, nullptr, [](ptrt_ctx *c, int v) { c->leaf_min = c->as_leaf_min = v; }},
    {"wavefront", &ptrt_ctx::wavefront, OPT_BOOL}, // 1: trace/shade stages over the whole frame's rays instead of the megakernel
    {"wf_sort", &ptrt_ctx::wf_sort, OPT_SNAP_124}, // wavefront stages: the shade stage sorts its paths by class (material, bounce) in LDS first, 1 / 2 / 4 groups of 256 together
    {"fetch_min", &ptrt_ctx::fetch_min, OPT_REJECT, 0, 64}, // PMODE 2: refill threshold in idle lanes; 0 = static batches of 64 pairs (A/B, tests)
    {"denoiser_active", &ptrt_ctx::dn_active, OPT_BOOL}, // perfSettings.enableDenoiser: use the (already allocated) denoiser or not
    {"motion_vectors", &ptrt_ctx::mv_active, OPT_BOOL}, // perfSettings.enableMotionVectors
    {"use_graphs", &ptrt_ctx::use_graphs, OPT_BOOL}, // 0: issue the refit / rebuild launches one by one instead of replaying a hipGraph
    {"atlas_lanes", &ptrt_ctx::atlas_lanes, OPT_LANES}, // ptrt_atlas_texels: lanes that share one triangle's texel range (-1: from atlas texels per face)
    {"atlas_filter_tile", &ptrt_ctx::atlas_filter_tile, OPT_TRISTATE}, // ptrt_atlas_filter: stage a tile's guides and colours in LDS at steps 1, 2 and 4 (-1: the measured rule)
    // read-only facts about the last ptrt_render (so that a measurement can say what ran)
    {"sample_sync_eff", &ptrt_ctx::sample_sync_eff, OPT_READ_ONLY},
    {"pm1_dense_roots_eff", &ptrt_ctx::pm1_dense_roots_eff, OPT_READ_ONLY},
    {"pm1_full_leaf_eff", &ptrt_ctx::pm1_full_leaf_eff, OPT_READ_ONLY},
    {"pm1_lane_groups_eff", &ptrt_ctx::pm1_lane_groups_eff, OPT_READ_ONLY}, // ... of the last frame or ray query, whichever came last
    {"plain_leaf_eff", &ptrt_ctx::plain_leaf_eff, OPT_READ_ONLY}, // ... of the last frame or query, whichever came last
    {"tri_frames_eff", &ptrt_ctx::tri_frames_eff, OPT_READ_ONLY}, // ... of the last frame
    {"atlas_lanes_eff", &ptrt_ctx::atlas_lanes_eff, OPT_READ_ONLY}, // ... of the last ptrt_atlas_texels: 1, 4, 16 or 64 (0: none yet)
    {"atlas_filter_tile_eff", &ptrt_ctx::atlas_filter_tile_eff, OPT_READ_ONLY}, // passes of the last ptrt_atlas_filter that ran the LDS tile (-1: none yet)
    {"refilled", nullptr, OPT_READ_ONLY, 0, 0, [](const ptrt_ctx *c) -> long long { return c->refill_eff ? 1 : 0; }},
    {"split_eff", &ptrt_ctx::split_eff, OPT_READ_ONLY},
    {"pipelined", nullptr, OPT_READ_ONLY, 0, 0, [](const ptrt_ctx *c) -> long long { return c->pipelined_last ? 1 : 0; }},
    {"render_mode", &ptrt_ctx::last_mode, OPT_READ_ONLY}, // 0 megakernel, 1 wavefront stages, 2 asynchronous lanes
    {"pmode", &ptrt_ctx::last_pmode, OPT_READ_ONLY}, // PMODE of the megakernel: 0 lock-step, 1 pairs/LDS triangles, 2 queue, 3 TLAS rounds, 4 merged queue
    {"merged_eff", &ptrt_ctx::merged_eff, OPT_READ_ONLY}, // loop shape of the last launch (1 = shadow rays ride with the next extension rays)
    // 0 while "merged" = -1 is still sampling
    {"merged_decided", nullptr, OPT_READ_ONLY, 0, 0,
     [](const ptrt_ctx *c) -> long long { return (c->merged >= 0 || c->tune_choice >= 0 || !c->last_merged_possible) ? 1 : 0; }},
    {"launches", nullptr, OPT_READ_ONLY, 0, 0, [](const ptrt_ctx *c) { return (long long)c->launches; }},
    {"query_pmode", &ptrt_ctx::query_pmode, OPT_READ_ONLY}, // traversal of the last ptrt_query_rays / ptrt_trace_rays / ptrt_query_radiance / ptrt_query_probes / ptrt_query_irradiance / ptrt_query_direct / ptrt_query_bounce: 0 one ray per lane, 1..3 pairs
    // the instances' first-pass boxes (PMODE 3) match the device's root boxes and matrices
    {"inst_pre_ok", nullptr, OPT_READ_ONLY, 0, 0, [](const ptrt_ctx *c) -> long long { return c->inst_pre_ok ? 1 : 0; }},
    {"tlas_refits", &ptrt_ctx::tlas_refits, OPT_READ_ONLY}, // ptrt_refit_tlas calls since the last geometry upload
    {"tlas_reorders", &ptrt_ctx::tlas_reorders, OPT_READ_ONLY}, // ptrt_reorder_tlas calls since the last geometry upload
    // the hipStream_t the context enqueues on (stream-ordering its device results)
    {"stream", nullptr, OPT_READ_ONLY, 0, 0, [](const ptrt_ctx *c) { return (long long)(intptr_t)c->stream; }},
};

const Option *find_option(const char *name) {
    for (const Option &o : OPTIONS)
        if (std::strcmp(o.name, name) == 0)
            return &o;
    return nullptr;
}

} // namespace

extern "C" {

int ptrt_set_option(ptrt_ctx *c, const char *name, long long value) {
    if (!ctx_live(c, false) || !name)
        return fail(c, PTRT_E_INVALID, "ptrt_set_option: bad argument");
    const Option *o = find_option(name);
    if (!o || o->policy == OPT_READ_ONLY)
        return fail(c, PTRT_E_INVALID, "unknown option '%s'", name);
    long long v = value;
    switch (o->policy) {
    case OPT_BOOL: v = value ? 1 : 0; break;
    case OPT_REJECT:
        if (value < o->lo || value > o->hi)
            return fail(c, PTRT_E_INVALID, "%s must be %lld..%lld", name, o->lo, o->hi);
        break;
    case OPT_CLAMP: v = value < o->lo ? o->lo : (value > o->hi ? o->hi : value); break;
    case OPT_MASK: v = value & o->hi; break;
    case OPT_TRISTATE: v = value < 0 ? -1 : (value ? 1 : 0); break;
    case OPT_SNAP_124: v = value <= 0 ? 0 : (value >= 4 ? 4 : (value >= 2 ? 2 : 1)); break;
    case OPT_LANES:
        if (value != -1 && value != 1 && value != 4 && value != 16 && value != 64)
            return fail(c, PTRT_E_INVALID, "%s must be -1, 1, 4, 16 or 64", name);
        break;
    case OPT_READ_ONLY: break;
    }
    if (o->set)
        o->set(c, (int)v);
    else
        c->*(o->field) = (int)v;
    return PTRT_OK;
}

// what ptrt_set_option set, plus the read-only facts
int ptrt_get_option(ptrt_ctx *c, const char *name, long long *value) {
    if (!ctx_live(c, false) || !name || !value)
        return fail(c, PTRT_E_INVALID, "ptrt_get_option: bad argument");
    const Option *o = find_option(name);
    if (!o)
        return fail(c, PTRT_E_INVALID, "unknown option '%s'", name);
    *value = o->get ? o->get(c) : c->*(o->field);
    return PTRT_OK;
}

// test hook: which kernels rendered the last frame (0 megakernel, 1 wavefront stages)
int ptrt_debug_last_render_mode(ptrt_ctx *c) { return ctx_live(c) ? c->last_mode : -1; }

// profiling hook (not part of the drop-in surface): reads and clears pt::g_trav_stats (32 words); all zero unless
// the library was built with -DPT_TRAV_STATS
int ptrt_debug_trav_stats(ptrt_ctx *c, unsigned long long *out32) {
    if (!ctx_live(c) || !out32)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_trav_stats: bad argument");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyFromSymbol(out32, HIP_SYMBOL(pt::g_trav_stats), 32 * sizeof(unsigned long long)));
    unsigned long long zero[32] = {};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(pt::g_trav_stats), zero, sizeof(zero)));
    return PTRT_OK;
}

// ... and pt::g_trav_bounce (64 words: the sixteen traversal counters split by the rays' bounce 0, 1, 2, >= 3)
int ptrt_debug_trav_bounce(ptrt_ctx *c, unsigned long long *out64) {
    if (!ctx_live(c) || !out64)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_trav_bounce: bad argument");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyFromSymbol(out64, HIP_SYMBOL(pt::g_trav_bounce), 64 * sizeof(unsigned long long)));
    unsigned long long zero[64] = {};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(pt::g_trav_bounce), zero, sizeof(zero)));
    return PTRT_OK;
}

#ifdef PT_TRAV_STATS
// ... and pt::g_trav_rhist (8 words: build_pairs calls by their live rays, TS_RHIST)
int ptrt_debug_trav_rhist(ptrt_ctx *c, unsigned long long *out8) {
    if (!ctx_live(c) || !out8)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_trav_rhist: bad argument");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyFromSymbol(out8, HIP_SYMBOL(pt::g_trav_rhist), 8 * sizeof(unsigned long long)));
    unsigned long long zero[8] = {};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(pt::g_trav_rhist), zero, sizeof(zero)));
    return PTRT_OK;
}

// ... and pt::g_trav_pm1 (136 words: the PMODE 1 triangle loops' iterations, batches and tail histogram, TS_PM1_*)
int ptrt_debug_trav_pm1(ptrt_ctx *c, unsigned long long *out136) {
    if (!ctx_live(c) || !out136)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_trav_pm1: bad argument");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyFromSymbol(out136, HIP_SYMBOL(pt::g_trav_pm1), 136 * sizeof(unsigned long long)));
    unsigned long long zero[136] = {};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(pt::g_trav_pm1), zero, sizeof(zero)));
    return PTRT_OK;
}

int ptrt_debug_trav_dbg(ptrt_ctx *c, unsigned long long *out1033) {
    if (!ctx_live(c) || !out1033)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_trav_dbg: bad argument");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyFromSymbol(out1033, HIP_SYMBOL(pt::g_trav_dbg), 1033 * sizeof(unsigned long long)));
    static unsigned long long zero[1033] = {};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(pt::g_trav_dbg), zero, sizeof(zero)));
    return PTRT_OK;
}
#endif

// test hook: exhaustive rcp_ieee check; out9[0] = mismatches, out9[1..8] = first offending inputs
int ptrt_debug_rcp_check(ptrt_ctx *c, unsigned int *out9) {
    if (!ctx_live(c) || !out9)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_rcp_check: bad argument");
    return run_check(c, out9, [c](unsigned int *d) { hipLaunchKernelGGL(pt::rcp_check_kernel, dim3(4096), dim3(256), 0, c->stream, d); });
}

// test hook: exhaustive rcp_ieee_above check over the inputs of its contract (|y| >= 2^-60, infinities and NaN included);
// out9 as above
int ptrt_debug_rcp_above_check(ptrt_ctx *c, unsigned int *out9) {
    if (!ctx_live(c) || !out9)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_rcp_above_check: bad argument");
    return run_check(c, out9, [c](unsigned int *d) { hipLaunchKernelGGL(pt::rcp_above_check_kernel, dim3(4096), dim3(256), 0, c->stream, d); });
}

// test hook: exhaustive sqrt_ieee check; out9[0] = mismatches, out9[1] = mismatches of the bare core in its range, out9[2..8] = inputs
int ptrt_debug_sqrt_check(ptrt_ctx *c, unsigned int *out9) {
    if (!ctx_live(c) || !out9)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_sqrt_check: bad argument");
    return run_check(c, out9, [c](unsigned int *d) { hipLaunchKernelGGL(pt::sqrt_check_kernel, dim3(4096), dim3(256), 0, c->stream, d); });
}

// test hook: div3's core for the divisors 1.m, m in [first, first + count), against every numerator significand (mode 0), or
// div3 with out-of-range exponents (modes 1, 2); out9[0] = mismatches, out9[1..8] = first offending {a, t} bit patterns.
// Two more checks of reciprocals ride on this entry point (the exported names are pinned): mode 4, neg_rcp_ieee against
// `-1.0f / y` for all 2^32 inputs (first, count unused; out9 as ptrt_debug_rcp_check); mode 5, orthoBasis against its text
// with the compiler's divisions over `count` normals from the seed `first` (out9: pt::orthoBasis_check_kernel)
int ptrt_debug_div3_check(ptrt_ctx *c, unsigned int first, unsigned int count, int mode, unsigned int *out9) {
    if (!ctx_live(c) || !out9 || count == 0 || count > (1u << 23) || mode < 0 || mode > 5)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_div3_check: bad argument");
    if (mode == 4)
        return run_check(c, out9, [c](unsigned int *d) { hipLaunchKernelGGL(pt::neg_rcp_check_kernel, dim3(4096), dim3(256), 0, c->stream, d); });
    if (mode == 5)
        return run_check(c, out9, [=](unsigned int *d) {
            hipLaunchKernelGGL(pt::orthoBasis_check_kernel, dim3((count + 255) / 256), dim3(256), 0, c->stream, first, count, d);
        });
    return run_check(c, out9, [=](unsigned int *d) {
        hipLaunchKernelGGL(pt::div3_check_kernel, dim3((count + 63) / 64), dim3(64), 0, c->stream, first, count, mode, d);
    });
}

// test hook (not part of the drop-in surface): the kernels' deterministic math on the GPU
int ptrt_debug_detmath(ptrt_ctx *c, int op, const float *x, const float *y, int n, float *out) {
    if (!ctx_live(c) || !x || !out || n <= 0)
        return fail(c, PTRT_E_INVALID, "ptrt_debug_detmath: bad argument");
    if (int rc = set_device(c))
        return rc;
    DeviceTemp<float> dx, dy, dout;
    HIP_TRY(c, dx.alloc((size_t)n));
    HIP_TRY(c, dy.alloc((size_t)n));
    HIP_TRY(c, dout.alloc((size_t)n));
    HIP_TRY(c, hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dy.p, y ? y : x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pt::detmath_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, op, dx.p, dy.p, n, dout.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PTRT_OK;
}

// test hook: the shading functions one by one on the device (pt::shade_probe_kernel) over the context's uploaded materials;
// op 0: n items of 11 floats -> 4 floats each; op 1: n items of 14 -> 13 (see the kernel).  full = 0: the simple-material variant
int ptrt_debug_shade(ptrt_ctx *c, int op, int full, const float *in, int n, float *out) {
    if (!ctx_live(c) || !in || !out || n <= 0 || (op != 0 && op != 1))
        return fail(c, PTRT_E_INVALID, "ptrt_debug_shade: bad argument");
    if (!c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "ptrt_debug_shade: materials not uploaded");
    if (int rc = set_device(c))
        return rc;
    const size_t ni = (size_t)n * (op == 0 ? 11 : 14) * 4, no = (size_t)n * (op == 0 ? 4 : 13) * 4;
    DeviceTemp<float> din, dout;
    HIP_TRY(c, din.alloc(ni / 4));
    HIP_TRY(c, dout.alloc(no / 4));
    HIP_TRY(c, hipMemcpy(din.p, in, ni, hipMemcpyHostToDevice));
    if (full)
        hipLaunchKernelGGL(pt::shade_probe_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->d_materials, op, din.p, n, dout.p);
    else
        hipLaunchKernelGGL(pt::shade_probe_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->d_materials, op, din.p, n, dout.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dout.p, no, hipMemcpyDeviceToHost));
    return PTRT_OK;
}

} // extern "C"
