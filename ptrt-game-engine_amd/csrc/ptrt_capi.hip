// ptrt_capi.hip -- implementation of the C ABI in include/ptrt.h over HIP (gfx950).
//
// Host responsibilities here: own every device allocation of a context, re-lay-out
// the caller's reference-shaped scene arrays (40-byte nodes, index triples,
// per-mesh pointers; mesh.cuh:37-47, intersection.cuh:90-106) into the arena the
// kernels read (pt_kernels.hip.h), pick the kernel instantiation that matches the
// scene, launch on the context's stream, time kernels with HIP events.
// There is no CPU rendering path in this library.
#include "../../include/ptrt.h"
#include "plain_leaf.h"
#include "pt_build.hip.h"
#include "pt_denoise.hip.h"
#include "pt_post.hip.h"
#include "pt_refit.hip.h"
#include "pt_tlas.hip.h"
#include "pt_render.hip.h"
#include "pt_wavefront.hip.h"
#include "pt_async.hip.h"
#include "pt_wireframe.hip.h"
#include "pt_query.hip.h"
#include "pt_radiance.hip.h"
#include "pt_probe.hip.h"
#include "pt_irradiance.hip.h"
#include "pt_direct.hip.h"
#include "pt_bounce.hip.h"
#include "pt_atlas.hip.h"
#include "pt_atlas_filter.hip.h"
#include "pt_lightmap.hip.h"
#include "pt_probe_sample.hip.h"
#include "pt_baked.hip.h"
#include "rt_render.hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <climits>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <algorithm>
#include <vector>

#include "ptrt_accel_state.hip.h"
#include "ptrt_frame_ring.hip.h"

namespace {

constexpr int EV_RING = 256;
// loop-shape choice of the queue modes (ptrt_set_option "merged" = -1): frames that only warm the clocks up, samples per
// shape (odd: their median decides), and the gain the merged loop must show to replace the separate-phase default
constexpr int TUNE_WARM = 4, TUNE_SAMPLES = 3;
constexpr float TUNE_MIN_GAIN = 0.005f;
thread_local std::string g_last_error = "";
std::mutex g_live_mutex;
std::set<ptrt_ctx *> g_live;

} // namespace

struct ptrt_ctx {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    std::vector<hipEvent_t> ev_ring; // 2 * EV_RING events: start/stop per launch
    unsigned long long launches = 0;
    int W = 0, H = 0, y0 = 0, rows = 0;
    int il_period = 1, il_phase = 0; // > 1: rows = the 8-row strips il_phase, il_phase + il_period, ... of the frame
    size_t npix = 0;
    std::string err;

    // frame buffers (tile)
    uint32_t *d_rng = nullptr;
    float *d_accum = nullptr, *d_normal = nullptr, *d_depth = nullptr;
    int *d_object_id = nullptr;
    // second set of the four, allocated when frames with a post chain overlap (ptrt_render "pipeline"): the trace of frame
    // N + 1 writes one set while the denoiser / bloom of frame N still reads the other; d_* is always the latest frame's
    float *alt_accum = nullptr, *alt_normal = nullptr, *alt_depth = nullptr;
    int *alt_object_id = nullptr;
    unsigned char *d_rgb8 = nullptr;
    unsigned char *wire_rgb8 = nullptr; // ptrt_render_wireframe to host memory: its own image (PTRT_BUF_RGB8 stays the path tracer's)
    unsigned char *last_rgb8 = nullptr; // where the last frame's RGB8 went
    void *last_frame_target = nullptr;  // ... or the caller's frame it was written into (PTRT_OUT_DEVICE_FRAME)
    int time_kernels = 1;               // option: record the two events per launch that ptrt_kernel_ms_history reads
    unsigned long long *d_counters = nullptr; // n_counter_slots x pt::COUNTER_WORDS {extension rays, shadow rays, paths, zero-valued light samples}
    size_t n_counter_slots = 0;
    float2 *d_blue = nullptr;
    uint32_t *d_jump = nullptr;
    int n_jump = 0;
    bool rng_ready = false;

    // scene arena
    float4 *d_nodes2 = nullptr; // two-level records derived from d_nodes (pt::expand_nodes_kernel), NODE2_F4 float4 per node
    float4 *d_mesh_recs = nullptr, *d_nodes = nullptr, *d_tris = nullptr, *d_tlas_nodes = nullptr,
           *d_materials = nullptr, *d_lights = nullptr;
    int2 *d_leaves = nullptr, *d_tlas_leaves = nullptr;
    int *d_tlas_mesh_ids = nullptr;
    float4 *d_tlas_heads = nullptr; // mesh-record heads in TLAS-leaf order (PMODE 3), gathered before each frame
    float4 *d_inst_pre = nullptr;   // per mesh: world-space first-pass box of an instance (PMODE 3), host-computed
    float inst_c2 = 0.0f;           // ... and the per-ray growth factor that goes with it
    bool inst_pre_ok = false;       // false once device-side boxes have moved (GPU refit / rebuild) since it was computed
    int n_tlas_index = 0;
    std::vector<float4> h_mesh_recs;
    std::vector<unsigned char> h_shadow_skip; // per material: transmission > 0.5
    int n_meshes = 0, n_materials = 0, n_lights = 0;
    float4 *d_tlas_root_box = nullptr; // {bmin, bmax}
    int tlas_root_ref = 0;
    // TLAS refit support (ptrt_set_instance_transforms / ptrt_refit_tlas / ptrt_read_tlas, pt_tlas.hip.h)
    int *d_tlas_refit = nullptr;        // {per leaf: where its box is stored | per inner node: the same | inner nodes by depth}
    float4 *d_tlas_world = nullptr;     // scratch: per TLAS index the mesh's world box
    int n_tlas_leaves = 0, n_tlas_inner = 0, tlas_world_cap = 0;
    pt::TopLevels tlas_levels{};        // the inner levels, deepest first, as offsets into the third part of d_tlas_refit
    std::vector<ptrt_bvh_node> h_tlas_in; // the TLAS as it was uploaded ...
    std::vector<int> h_tlas_in_dst;       // ... and where the device keeps each of its nodes' boxes (INT32_MIN: nowhere)
    int tlas_refits = 0;                // ptrt_refit_tlas calls since the last geometry upload
    // TLAS re-order support (ptrt_reorder_tlas, pt_tlas.hip.h)
    uint32_t *d_tlas_sort = nullptr;    // scratch: {cbounds 8 | centres 3n | keys n, n | meshes n, n | radix counts, positions}
    int tlas_sort_cap = 0;              // (the cbounds, key and radix parts are used only beyond pt::TLAS_WIDE meshes)
    bool tlas_is_perm = false;          // the uploaded TLAS index array is a permutation of 0 .. mesh count - 1
    int tlas_reorders = 0;              // ptrt_reorder_tlas calls since the last geometry upload
    bool xf_host_stale = false;         // ptrt_set_instance_transforms_device wrote flag bits and matrices h_mesh_recs has not seen
    bool inst_c2_all = false;           // inst_c2 covers every instance's matrices (host_inst_c2), not only the upload's finite boxes
    XformStage xf;                      // staged instance transforms (ptrt_set_instance_transforms)
    // refit support (ptrt_update_vertices / ptrt_refit)
    float *d_verts = nullptr;       // all meshes' vertices, xyz packed
    int4 *d_slot_face = nullptr;    // per leaf slot: global vertex indices + face index
    int *d_leaf_dst = nullptr;      // per leaf: where its box is stored (see convert_tree)
    int *d_node_dst = nullptr;      // per inner node: where its own box is stored
    int *d_level_nodes = nullptr;   // inner nodes ordered by depth
    std::vector<int> level_offset;  // level_offset[d] .. level_offset[d+1]: nodes at depth d+1
    std::vector<int> mesh_vert_base, mesh_vert_count;
    std::vector<std::vector<ptrt_bvh_node>> h_mesh_in; // per mesh the BVH as it was uploaded ... (ptrt_read_bvh; no render path reads these)
    std::vector<std::vector<int>> h_mesh_in_dst;       // ... and where the device keeps each of its nodes' boxes (INT32_MIN: nowhere)
    int n_slots = 0, n_leaves = 0;
    // GPU rebuild support (ptrt_build_bvh, pt_build.hip.h)
    int4 *d_face_src = nullptr;   // per face, mesh-major, original order: global vertex indices + face index
    int *d_slot_pos = nullptr;    // per leaf slot: its position in the mesh's prim order
    std::vector<int> mesh_face_base, mesh_face_count, mesh_slot_base, mesh_slot_count;
    std::vector<unsigned char> mesh_rebuildable, mesh_is_soup;
    BuildScratch build;
    std::map<int, hipGraphExec_t> graphs; // captured launch sequences by GraphKey (ptrt_accel.hip.h)
    hipStream_t capture_stream = nullptr;
    int use_graphs = 0; // measured: replaying the sequence as a hipGraph gains nothing on ROCm 7.2
    bool tlas_single_leaf = false, all_single_leaf = false, mats_full = false;
    int stack_entries = 1;
    int pair_meshes = 0, pair_tri_slots = 0, pair_max_leaf = 0;
    bool pair_leaf_uniform = false; // every leaf has exactly pair_max_leaf triangles
    pt::Pm1Plan pm1_plan{};         // ... then: the sub-batches of a pair-list tail (pm1_plan.h), built at upload
    bool pm1_plan_ok = false;
    // single-leaf TLAS, no instanced mesh, every mesh box inside the root box (plain_leaf.h): derived by a full upload, cleared by
    // whatever moves a box or sets a transform without the host seeing the result
    bool plain_leaf_ok = false;
    // per leaf slot the tangent frames of orthoBasis(gn) and orthoBasis(-gn) (pt::tri_normals_kernel), written by a full upload;
    // tri_frames_ok: they match the packets' normals and no mesh has a transform -- set there, cleared with plain_leaf_ok
    float4 *d_tri_frames = nullptr;
    bool tri_frames_ok = false;
    int tlas_max_leaf = 0, tlas_depth = 0;
    bool have_geometry = false, have_materials = false;

    pt::Camera cam{};
    pt::f3 sky_top{0.6f, 0.7f, 1.0f}, sky_bottom{1.0f, 1.0f, 1.0f};
    int use_sky = 1;
    float4 *d_env = nullptr; // equirectangular environment map (ptrt_set_env_map)
    int env_w = 0, env_h = 0;

    // denoiser (class Denoiser, denoiser.cuh:781-1070): scratch + double-buffered history
    bool dn_on = false, dn_first = true;
    pt::DenoiseSettings dn{};
    // float4 images (pt_denoise.hip.h): cur4 {rgb,0}; c4 {rgb,variance} ping-pong; g4 {normal,depth},
    // h1 {mean,len}, h2 {m2,-} double-buffered across frames
    float4 *dn_cur4 = nullptr, *dn_c4[2] = {nullptr, nullptr}, *dn_g4[2] = {nullptr, nullptr};
    float4 *dn_h1[2] = {nullptr, nullptr}, *dn_h2[2] = {nullptr, nullptr};
    int *dn_hobj = nullptr;
    float *dn_motion = nullptr, *dn_out = nullptr, *dn_pvp = nullptr;
    int dn_cur = 0; // which history set holds the latest result
    int dn_active = 1, mv_active = 1;
    float prev_view_proj[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

    // post chain (pt_post.hip.h): render size (perfSettings.resolutionScale) and bloom
    int rw = 0, rh = 0; // render size; == W,H unless ptrt_set_render_size asked for less
    float *s_accum = nullptr, *s_normal = nullptr, *s_depth = nullptr; // the d_scaled_* set (scene.cuh:181-186)
    int *s_object_id = nullptr;
    int bloom_on = 0;
    float *bl_mip[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // d_bloom_mip_chain (scene.cuh:161, 809-822)
    bool scaled() const { return rw != W || rh != H; }
    size_t rpix() const { return scaled() ? (size_t)rw * rh : npix; } // pixels the path tracer renders

    // presentation ring (ptrt_present_*): device RGB8 frames mirrored into pinned host memory
    FrameRing present;

    // wavefront stages (pt_wavefront.hip.h): per-path state, planar, tile-ordered
    int wavefront = 0; // option: 1 = render scenes with a single-leaf TLAS through the trace/shade stages
    int wf_sort = 0;   // option: the shade stage bins its paths by class first (active-path sorting, pt_wavefront.hip.h)
    uint32_t *wf_st = nullptr, *wf_occ = nullptr, *wf_live = nullptr;
    float *wf_planes = nullptr; // 25 planes: ray 6, thr 3, acc 3, avg 3, pend 3, shadow ray 7
    float4 *wf_hit = nullptr;
    size_t wf_items = 0;
    int wf_trace_blocks = 0;
    size_t wf_trace_lds = 0;
    int n_geometry_uploads = 0, n_instance_updates = 0;
    bool any_transform = false; // some mesh is an instance with its own transform
    int pair_split = 1;         // option (A/B, tests)
    int last_mode = 0; // how the last frame was rendered: 0 megakernel, 1 wavefront stages, 2 asynchronous lanes
    // asynchronous-lane megakernel (pt_async.hip.h)
    int async_lanes = 0, shade_min = 32, as_leaf_min = 24; // options
    uint32_t *as_cursor = nullptr;
    // Lane refill (PMODE 1, path_trace_kernel<.., STREAM = true>): option "refill" 0 never, 1 (default) where it was measured to
    // pay -- frames that overlap their predecessor, simple materials, no post chain, spp * bounces >= 16 --, 2 wherever PMODE 1 runs (tests)
    int refill = 1;
    bool refill_eff = false;         // ... the last frame
    VertexStage verts;               // staged vertex positions (ptrt_update_vertices)
    unsigned int *d_queue = nullptr; // {ticket, waves out} per launch lane: [0] the stream, [1 + i] auxiliary stream i
    int sample_sync = -1;            // option "sample_sync": -1 (default) where it was measured to pay, 0 never, 1 always (ptrt_render)
    int sample_sync_eff = 0;         // ... the last frame
    int pm1_dense_roots = -1;        // option "pm1_dense_roots": -1 (default) where it pays, 0 never, 1 always (ptrt_render)
    int pm1_dense_roots_eff = 0;     // ... the last frame (0 as well when another traversal mode rendered it)
    int pm1_full_leaf = -1;          // option "pm1_full_leaf": -1 (default) and 1: on when the leaves are uniform, 0 never (make_params)
    int pm1_full_leaf_eff = 0;       // ... the last frame (0 as well when another traversal mode rendered it)
    int pm1_lane_groups = -1;        // option "pm1_lane_groups": -1 (default) and 1: on where pm1_full_leaf is in effect, 0 the 2^sh rule (make_params)
    int pm1_lane_groups_eff = 0;     // ... the last frame or ray query (0 as well when another traversal mode ran it)
    int plain_leaf = -1;             // option "plain_leaf": -1 (default) and 1: on where the upload derived it (plain_leaf_ok), 0 never (make_params)
    int plain_leaf_eff = 0;          // ... the last frame or query (0 as well when a traversal mode without the pair builder ran it)
    int tri_frames = -1;             // option "tri_frames": -1 (default) and 1: PMODE 1 reads to_world's frame from d_tri_frames where tri_frames_ok, 0 never (plan_frame)
    int tri_frames_eff = 0;          // ... the last frame
    int tile_run = 8;                // option "tile_run": of every 8 * run consecutive tiles XCD x renders a run of neighbours (path_trace_kernel); 0: tile k on workgroup k
    int ticket_tiles = 1;            // option "ticket_tiles": consecutive tiles per ticket of the queue
    int persist = 0, n_cus = 0;      // option "persist": persistent waves per CU (0 = the variant's occupancy): lane refill and the radiance query
    int as_blocks[2] = {0, 0}; // resident workgroups of the <false>/<true> kernel at as_lds bytes of LDS
    size_t as_lds = 0;

    // options
    int count_rays = 0, force_geom = -1, force_full = 0, pair_trace = 1, fetch_min = 16, leaf_pairs = 1, steal = 1, leaf_min = 8;
    int atrous_exp = 0; // option: 1 = the a-trous luminance weight through v_exp_f32 (the reference's __expf) instead of det_exp: tolerance mode
    int csteal_follow = 1, csteal_leaf_min = 32;
    int csteal = 2, csteal_min = 0; // options: PMODE 2 closest-hit subtree stealing with verification (pt_render.hip.h run_closest_queue)
    int lds_pad = 0; // extra bytes of LDS per workgroup (A/B of the occupancy)
    // PMODE 1, simple materials: tiles per workgroup.  1 (default): five waves per SIMD.  2: two tiles share the LDS copies, six
    // waves per SIMD on 80 VGPRs -- measured on Cornell 1080p: 1.875 vs 1.877 ms, the 112 B per lane it spills eat what 24
    // instead of 20 waves per CU bring.  0: two when the scene fits that budget.
    int pm1_wg = 1;
    // option "split": the frame's tile rows dealt to that many launches on auxiliary streams of the context (forked from and
    // joined to its stream by events, so the caller still sees one stream).  Concurrent launches of ONE frame buy nothing
    // (Cornell 1080p 1.85 vs 1.82 ms); what they make possible is option "pipeline": frame N + 1's launches follow frame N's
    // on their own streams and do not wait for the rest of frame N to drain -- 1.81 -> 1.66 ms (see ptrt_render).
    static constexpr int MAX_SPLIT = 4;
    int split = 2, split_eff = 1, pipeline = 1;
    hipStream_t aux_stream[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t split_fork = nullptr, split_join[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr};
    bool heads_fresh = false;     // PMODE 3: the TLAS-leaf-order heads were gathered since the last touching entry point
    bool touched = true;          // an entry point that may enqueue device work ran since the last ptrt_render (ctx_live)
    bool escaped = false;         // ptrt_device_buffer handed out pointers into the context's buffers
    void *prev_out = nullptr;     // the previous frame's device target
    hipStream_t prev_stream = nullptr;
    int prev_split = 0;
    bool pipelined_last = false;  // the last frame's launches did not wait for the stream (ptrt_get_option "pipelined")
    hipEvent_t head_ev[2] = {nullptr, nullptr}; // the stream's head at the start of the last two ptrt_render calls
    unsigned head_n = 0;
    int tlas_rounds = 0; // option (A/B, tests): PMODE 3 shadow rays take one TLAS leaf per fill, as scenes with > 1024 meshes do
    int stage = 7; // PMODE 1, shading inputs staged in LDS: 0 none, else jitter table + blue noise, | 1 lights, | 2 materials
    int lds_nodes = 0; // option: PMODE 2 in 256-thread workgroups sharing an LDS copy of the BLAS top levels (measured slower: DESIGN.md 3.1)
    int n_nodes = 0;
    // option: PMODE 4 (one traversal per loop iteration) where PMODE 2 applies: 0 / 1, or -1 = try both on a scene's first
    // frames and keep the faster (showcase: PMODE 4 by 1.5 %; fluid, 1 M triangles: PMODE 2 by 2-5 %; the bits are the same)
    int merged = -1;
    int merged_eff = 0;                  // what this launch uses
    int tune_n = 0, tune_choice = -1;    // auto: frames measured so far (variants alternate), the decision (-1: none yet)
    unsigned long long tune_key = ~0ull, tune_launch[2 * TUNE_SAMPLES] = {};
    int last_pmode = 0;                  // PMODE of the last megakernel launch (ptrt_get_option "pmode")
    int query_pmode = -1;                // traversal of the last ray query (ptrt_get_option "query_pmode"; -1 none yet)
    int atlas_lanes = -1;                // option "atlas_lanes": lanes per triangle of ptrt_atlas_texels, 1 / 4 / 16 / 64, or -1: by the texels per face
    int atlas_lanes_eff = 0;             // ... of the last ptrt_atlas_texels (0 none yet)
    int atlas_filter_tile = -1;          // option "atlas_filter_tile": ptrt_atlas_filter's LDS tile, 0 never / 1 wherever it fits / -1: by the measured rule
    int atlas_filter_tile_eff = -1;      // passes of the last ptrt_atlas_filter that ran the LDS tile (-1 none yet)
    bool last_merged_possible = false;   // ... and whether that scene has the two loop shapes to choose from
    bool timed = false;
    bool prev_post = false;              // the previous frame had a denoiser / bloom chain behind its trace (ptrt_render "pipeline")
    size_t refill_counter_base = 0;      // first counter slot of the lane-refill kernel's launches (disjoint from the tile slots)
    // option "time_launches": three events per launch of a frame dealt to the auxiliary streams -- before the trace kernel,
    // behind it, behind the tonemap pass that follows it with lane refill -- on the stream the launch runs on, so that a
    // measurement can state the duration of the very launches it timed (ptrt_launch_ms_history); the events around a frame on
    // the context's stream (time_kernels) measure the frame INTERVAL once frames overlap
    int time_launches = 0;
    std::vector<hipEvent_t> launch_ev[MAX_SPLIT]; // 3 * EV_RING per auxiliary stream
    unsigned char launch_timed[EV_RING] = {};     // launches of frame (launches % EV_RING) that carry events (0: none)
    // An interval between two recorded events is asked of the runtime ONCE and kept until the slot's events are recorded again:
    // hipEventElapsedTime may read the same pair a nanosecond differently the next time (the runtime re-fits its tick-to-time
    // conversion now and then), and a history must not move because something else ran in between
    float ev_ms[EV_RING] = {};                    // ... of ev_ring's pair of a slot
    bool ev_ms_known[EV_RING] = {};
    float launch_ms[MAX_SPLIT][EV_RING][2] = {};  // ... of launch_ev's two intervals
    bool launch_ms_known[MAX_SPLIT][EV_RING] = {};
    // option "tm_prio" (lane refill's tonemap pass): bit 0 = the pass runs on a stream of the highest priority, forked from
    // and joined to the launch's stream by events; bit 1 = its waves raise their issue priority (s_setprio 3)
    int tm_prio = 0;
    hipStream_t tm_stream[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t tm_fork[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr}, tm_join[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr};
};

namespace {

// Records the message for ptrt_last_error.  `c` may be a stale (already destroyed) handle -- every entry point
// reports "bad context" through here -- so it is only written to while it is in the live set.
int fail(ptrt_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (c) {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        if (g_live.count(c))
            c->err = buf;
    }
    return code;
}

#define HIP_TRY(c, call)                                                                                       \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return fail((c), PTRT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_));                       \
    } while (0)

template <class T> void dfree(T *&p) {
    if (p) {
        (void)hipFree(p);
        p = nullptr;
    }
}
// A function-local device allocation of n elements: freed when it goes out of scope, so that no early return (HIP_TRY) leaks
// it.  Move-only.  The context's long-lived buffers stay raw pointers: they feed the kernel-parameter structs directly.
template <class T> struct DeviceTemp {
    T *p = nullptr;
    DeviceTemp() = default;
    DeviceTemp(DeviceTemp &&o) noexcept : p(o.p) { o.p = nullptr; }
    DeviceTemp &operator=(DeviceTemp &&o) noexcept {
        std::swap(p, o.p);
        return *this;
    }
    ~DeviceTemp() { dfree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, n * sizeof(T)); }
};
template <class T> int upload(ptrt_ctx *c, T *&dst, const std::vector<T> &src) {
    dfree(dst);
    const size_t n = src.empty() ? 1 : src.size();
    HIP_TRY(c, hipMalloc((void **)&dst, n * sizeof(T)));
    if (!src.empty())
        HIP_TRY(c, hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // src may be a temporary
    return PTRT_OK;
}

float4 f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
float as_f(int i) {
    float f;
    std::memcpy(&f, &i, 4);
    return f;
}

// ---- GF(2) algebra for the XORWOW subsequence jump (cuRAND: subsequence = 2^67 draws) ----
struct GF2 {
    uint32_t col[160][5];
};
void gf2_apply(const GF2 &m, const uint32_t in[5], uint32_t out[5]) {
    uint32_t a[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < 5; ++w)
        for (uint32_t bits = in[w]; bits; bits &= bits - 1) {
            const uint32_t *c = m.col[w * 32 + __builtin_ctz(bits)];
            for (int k = 0; k < 5; ++k)
                a[k] ^= c[k];
        }
    std::memcpy(out, a, sizeof a);
}
void gf2_square(GF2 &m) {
    GF2 t;
    for (int j = 0; j < 160; ++j)
        gf2_apply(m, m.col[j], t.col[j]);
    m = t;
}
// jump[k] = (one generator step)^(2^(67+k)), k = 0..JUMP_MAX-1, as 800 words each.  Computed once for the largest
// pixel index a context can have (2^40 pixels), so the vector never reallocates under a concurrent reader.
constexpr int JUMP_MAX = 40;
const std::vector<uint32_t> &jump_matrices() {
    static std::vector<uint32_t> out;
    static std::once_flag once;
    std::call_once(once, [] {
    const int n = JUMP_MAX;
    GF2 m;
    for (int j = 0; j < 160; ++j) { // image of basis vector j under one step of the recurrence
        uint32_t v[5] = {0, 0, 0, 0, 0};
        v[j / 32] = 1u << (j % 32);
        const uint32_t t = v[0] ^ (v[0] >> 2);
        uint32_t nv[5] = {v[1], v[2], v[3], v[4], (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))};
        std::memcpy(m.col[j], nv, sizeof nv);
    }
    for (int i = 0; i < 67; ++i)
        gf2_square(m);
    out.resize((size_t)n * 800);
    for (int k = 0; k < n; ++k) {
        std::memcpy(&out[(size_t)k * 800], m.col, 800 * sizeof(uint32_t));
        gf2_square(m);
    }
    });
    return out;
}

// The jump matrices on the device, enough of them for subsequence numbers up to `last` (one per bit).
int ensure_jump(ptrt_ctx *c, unsigned long long last, const char *who) {
    int bits = 1;
    while (bits < 64 && (last >> bits) != 0)
        ++bits;
    if (bits > c->n_jump) {
        if (bits > JUMP_MAX)
            return fail(c, PTRT_E_INVALID, "%s: subsequence numbers of %d bits (at most %d: 2^%d pixels or states)", who, bits, JUMP_MAX, JUMP_MAX);
        const std::vector<uint32_t> &J = jump_matrices();
        dfree(c->d_jump);
        c->n_jump = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_jump, (size_t)bits * 800 * sizeof(uint32_t)));
        HIP_TRY(c, hipMemcpy(c->d_jump, J.data(), (size_t)bits * 800 * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->n_jump = bits;
    }
    return PTRT_OK;
}
// curand_init's state scrambling (published cuRAND XORWOW; constants unverified)
struct XorwowSeed {
    uint32_t d, v[5];
};
XorwowSeed xorwow_seed(unsigned long long seed) {
    const uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
    const uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * s0;
    const uint32_t t1 = 2591861531u * s1;
    return XorwowSeed{6615241u + t1 + t0, {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0}};
}

int set_device(ptrt_ctx *c) {
    HIP_TRY(c, hipSetDevice(c->device));
    return PTRT_OK;
}

int merged_pair_cap(const ptrt_ctx *c); // (ptrt_render.hip.h, with the other LDS sizes)
pt::KParams make_params(ptrt_ctx *c) {
    pt::KParams K{};
    K.mesh_recs = c->d_mesh_recs;
    K.nodes = c->d_nodes;
    K.nodes2 = c->d_nodes2;
    K.leaves = c->d_leaves;
    K.tris = c->d_tris;
    K.slot_face = c->d_slot_face;
    K.tlas_nodes = c->d_tlas_nodes;
    K.tlas_leaves = c->d_tlas_leaves;
    K.tlas_mesh_ids = c->d_tlas_mesh_ids;
    K.tlas_heads = c->d_tlas_heads;
    K.inst_c2 = c->inst_c2;
    K.materials = c->d_materials;
    K.lights = c->d_lights;
    K.blue_noise = c->d_blue;
    K.tlas_root_box = c->d_tlas_root_box;
    K.tlas_root_ref = c->tlas_root_ref;
    K.n_meshes = c->n_meshes;
    K.n_lights = c->n_lights;
    K.inv_n_lights = c->n_lights > 0 ? 1.0f / (float)c->n_lights : 0.0f;
    K.stack_entries = c->stack_entries;
    K.pair_meshes = c->pair_meshes;
    K.pair_tri_slots = c->pair_tri_slots;
    K.pair_max_leaf = c->pair_max_leaf;
    K.tlas_max_leaf = c->tlas_max_leaf;
    K.tlas_depth = c->tlas_depth < 1 ? 1 : c->tlas_depth;
    K.tlas_any_rounds = (c->n_meshes > 1024 || c->tlas_rounds) ? 1 : 0; // (TLAS indices beyond 10 bits do not fit a 16-bit pair entry)
    K.pair_split = (c->pair_split && !c->any_transform) ? 1 : 0;
    K.pm1_full_leaf = (c->pm1_full_leaf != 0 && c->pair_leaf_uniform) ? 1 : 0;
    K.pm1_groups = (c->pm1_lane_groups != 0 && K.pm1_full_leaf && c->pm1_plan_ok) ? 1 : 0;
    if (K.pm1_groups)
        K.pm1_plan = c->pm1_plan;
    K.plain_leaf = (c->plain_leaf != 0 && c->plain_leaf_ok && c->tlas_single_leaf && !c->any_transform) ? 1 : 0;
    K.fetch_min = c->fetch_min > 0 ? c->fetch_min : 64; // 0 = refill only when the whole wave is idle: batches of 64
    K.pair_cap = merged_pair_cap(c);
    K.n_nodes = c->n_nodes;
    // the compacted leaf phase lists up to 64 x (largest leaf) tests in its owner list (lds_layout.h): the reference
    // builder's leaves (<= 17 triangles) fit; a scene built with a larger leaf target walks its leaves lane by lane
    K.leaf_pairs = (c->leaf_pairs && pt::leaf_pairs_fit(c->pair_max_leaf)) ? 1 : 0;
    K.leaf_min = c->leaf_min;
    K.steal = c->steal;
    K.csteal = c->csteal;
    K.csteal_min = c->csteal_min;
    K.csteal_follow = c->csteal_follow;
    K.csteal_leaf_min = c->csteal_leaf_min;
    K.cam = c->cam;
    K.sky_top = c->sky_top;
    K.sky_bottom = c->sky_bottom;
    K.use_sky = c->use_sky;
    K.env = c->d_env;
    K.env_w = c->env_w;
    K.env_h = c->env_h;
    // at a reduced render size (full-frame contexts only) the frame is rw x rh in the d_scaled_* set; the
    // generator states stay where they are: pixel p of the small frame uses state p (scene.cuh:1091-1098)
    const bool scaled = c->scaled();
    K.width = c->rw;
    K.height = c->rh;
    K.y0 = c->y0;
    K.il_period = c->il_period;
    K.il_phase = c->il_phase;
    K.rows = scaled ? c->rh : c->rows;
    K.tiles_x = (c->rw + 7) / 8;
    K.rng = c->d_rng;
    K.rng_plane = c->npix;
    K.accum = scaled ? c->s_accum : c->d_accum;
    K.normal = scaled ? c->s_normal : c->d_normal;
    K.depth = scaled ? c->s_depth : c->d_depth;
    K.object_id = scaled ? c->s_object_id : c->d_object_id;
    K.rgb8 = c->d_rgb8;
    K.counters = nullptr;
    K.tile_run = 0;
    return K;
}

// `device_work`: the caller may enqueue work on the context's stream or change what its kernels read from memory -- every
// entry point except the few host-only ones below.  The next ptrt_render then orders its launches behind the stream (see
// "pipeline" there) instead of overlapping them with the previous frame's.
bool ctx_live(ptrt_ctx *c, bool device_work = true) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    const bool live = c && g_live.count(c);
    if (live && device_work) {
        c->touched = true;
        c->heads_fresh = false;
    }
    return live;
}

void free_denoiser(ptrt_ctx *c) {
    dfree(c->dn_cur4);
    for (int k = 0; k < 2; ++k) {
        dfree(c->dn_c4[k]);
        dfree(c->dn_g4[k]);
        dfree(c->dn_h1[k]);
        dfree(c->dn_h2[k]);
    }
    dfree(c->dn_hobj);
    dfree(c->dn_motion);
    dfree(c->dn_out);
    dfree(c->dn_pvp);
    c->dn_on = false;
}

void free_post(ptrt_ctx *c) {
    dfree(c->s_accum);
    dfree(c->s_normal);
    dfree(c->s_depth);
    dfree(c->s_object_id);
    for (int i = 0; i < 6; ++i)
        dfree(c->bl_mip[i]);
    c->bloom_on = 0;
}

// `bytes` of device memory at p, all inside one allocation on the context's device
bool device_span(ptrt_ctx *c, const void *p, size_t bytes) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // (memory HIP has never seen: an error it would report again later)
        return false;
    }
    if (a.type != hipMemoryTypeDevice || a.device != c->device)
        return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const size_t off = (size_t)((const char *)p - (const char *)base);
    return off <= size && bytes <= size - off;
}

} // namespace

#include "ptrt_present.hip.h"
#include "ptrt_accel.hip.h"
#include "ptrt_render.hip.h"

// =====================================================================================
extern "C" {

int ptrt_abi_version(void) { return PTRT_ABI_VERSION; }

// include/ptrt.h: the LDS layout of a launch shape (lds_layout.h) with the budgets plan_frame uses, without a device
int ptrt_lds_layout(int shape, const ptrt_lds_params *p, ptrt_lds_region *regions, int max_regions, ptrt_lds_info *info) {
    namespace lds = pt::lds;
    if (!p || !info || max_regions < 0 || (max_regions > 0 && !regions) || p->meshes < 0 || p->tri_slots < 0 || p->stack_entries < 0 ||
        p->tlas_leaf < 0 || p->tlas_depth < 0 || p->lights < 0 || p->lds_pad < 0)
        return -1;
    *info = ptrt_lds_info{};
    lds::Layout Y;
    switch (shape) {
    case PTRT_LDS_LOCKSTEP: Y = lds::lockstep_layout(p->stack_entries); break;
    case PTRT_LDS_PAIR4:
        info->pair_cap = lds::merged_pair_cap(p->meshes, p->stack_entries, MERGED_LDS_BUDGET);
        info->pair_cap_lo = lds::merged_cap_lo(p->meshes);
        info->pair_cap_hi = lds::merged_cap_hi(p->meshes);
        [[fallthrough]];
    case PTRT_LDS_PAIR1:
    case PTRT_LDS_PAIR2:
    case PTRT_LDS_PAIR3:
        if (shape != PTRT_LDS_PAIR3 && p->meshes < 1)
            return -1;
        Y = lds::pair_layout(shape, p->meshes, p->tri_slots, p->stack_entries, p->tlas_leaf, p->tlas_depth, info->pair_cap);
        break;
    case PTRT_LDS_PM1_WG: {
        if (p->meshes < 1)
            return -1;
        const bool full = p->full != 0;
        const lds::Pm1Choice P = pm1_choice(p->meshes, p->tri_slots, p->lights, full, p->stage, p->sample_sync, p->lds_pad, p->pm1_wg);
        info->lds_extra = P.s.lds_extra;
        info->lds_flags = P.s.lds_flags;
        info->lds_wave = P.s.lds_wave;
        info->lds_wave_bytes = P.s.lds_wave_bytes;
        info->wg = P.wg;
        if (P.total)
            Y = lds::pm1_layout(p->meshes, p->tri_slots, p->lights, full, P.wg, P.s, p->lds_pad);
        break;
    }
    case PTRT_LDS_NODES: Y = lds::nodes_layout(p->meshes, p->stack_entries, pt::TOP_NODES); break;
    case PTRT_LDS_ASYNC: Y = lds::async_layout(p->stack_entries); break;
    case PTRT_LDS_WAVEFRONT: Y = lds::wavefront_layout(p->stack_entries); break;
    default: return -1;
    }
    info->total = (int64_t)Y.total;
    info->waves = Y.waves;
    info->max_leaf = pt::LEAF_PAIR_TESTS;
    int n = 0;
    for (int id = 0; id < lds::N_REGIONS; ++id)
        for (int w = 0; w < (id >= lds::FIRST_WAVE ? Y.waves : 1); ++w) {
            const lds::Region &r = Y.r[id];
            if (!r.bytes)
                continue;
            if (n < max_regions)
                regions[n] = ptrt_lds_region{id, id >= lds::FIRST_WAVE ? w : -1, (int64_t)Y.at(id, w), (int64_t)r.bytes, r.align, r.in_first, r.in_last};
            ++n;
        }
    return n;
}
const char *ptrt_lds_region_name(int id) {
    static const char *const names[pt::lds::N_REGIONS] = {"tris", "meshtab", "meshbox", "topnodes", "jit", "lights", "mats", "best",
                                                           "pairs", "occ", "stack", "tstack", "leafx", "lkey", "owner", "bn",
                                                           "count", "dirty", "ring", "tail", "limits", "dense_owner", "park"};
    return id >= 0 && id < pt::lds::N_REGIONS ? names[id] : nullptr;
}

const char *ptrt_last_error(const ptrt_ctx *ctx) {
    if (ctx && ctx_live(const_cast<ptrt_ctx *>(ctx), false))
        return ctx->err.c_str();
    return g_last_error.c_str();
}

namespace {
int create_ctx(int full_w, int full_h, int tile_y0, int tile_rows, int il_period, int il_phase, int device, ptrt_ctx **out) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PTRT_E_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return fail(nullptr, PTRT_E_NO_DEVICE, "device %d out of range (have %d)", device, ndev);
    ptrt_ctx *c = new ptrt_ctx();
    c->device = device;
    c->W = full_w;
    c->H = full_h;
    c->y0 = tile_y0;
    c->rows = tile_rows;
    c->il_period = il_period;
    c->il_phase = il_phase;
    c->npix = (size_t)full_w * tile_rows;
    c->rw = full_w;
    c->rh = full_h;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live.insert(c);
    }
    *out = c;
    int rc = set_device(c);
    if (rc)
        return rc;
    HIP_TRY(c, hipStreamCreate(&c->own_stream));
    c->stream = c->own_stream;
    c->ev_ring.assign(2 * EV_RING, nullptr);
    for (auto &ev : c->ev_ring)
        HIP_TRY(c, hipEventCreate(&ev));
    HIP_TRY(c, hipMalloc((void **)&c->d_rng, c->npix * 6 * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc((void **)&c->d_accum, c->npix * 3 * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_normal, c->npix * 3 * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_depth, c->npix * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_object_id, c->npix * sizeof(int)));
    HIP_TRY(c, hipMalloc((void **)&c->d_rgb8, c->npix * 3));
    c->n_counter_slots = (size_t)((c->W + 7) / 8) * ((c->rows + 7) / 8); // one slot of pt::COUNTER_WORDS per 8x8-pixel workgroup
    c->n_counter_slots += 4; // the shade stage uses one slot per wave of a 256-thread grid (rounded up)
    c->n_counter_slots += (size_t)ptrt_ctx::MAX_SPLIT * ((c->W + 7) / 8);
    // (lane refill: a slot per persistent wave and launch of a split frame -- never more waves than tiles -- in a range of their own:
    // consecutive overlapping frames may run the one-tile kernel and the refill kernel on different streams at the same time)
    c->refill_counter_base = c->n_counter_slots;
    c->n_counter_slots += (size_t)((c->W + 7) / 8) * ((c->rows + 7) / 8) + (size_t)ptrt_ctx::MAX_SPLIT * ((c->W + 7) / 8);
    HIP_TRY(c, hipMalloc((void **)&c->d_queue, 2 * (1 + ptrt_ctx::MAX_SPLIT) * sizeof(unsigned int)));
    HIP_TRY(c, hipMemsetAsync(c->d_queue, 0, 2 * (1 + ptrt_ctx::MAX_SPLIT) * sizeof(unsigned int), c->stream));
    HIP_TRY(c, hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    HIP_TRY(c, hipMalloc((void **)&c->d_counters, c->n_counter_slots * pt::COUNTER_WORDS * sizeof(unsigned long long)));
    HIP_TRY(c, hipMalloc((void **)&c->d_blue, PTRT_BLUE_NOISE_FLOATS * sizeof(float)));
    HIP_TRY(c, hipMemsetAsync(c->d_rng, 0, c->npix * 6 * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_accum, 0, c->npix * 3 * sizeof(float), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_rgb8, 0, c->npix * 3, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, c->n_counter_slots * pt::COUNTER_WORDS * sizeof(unsigned long long), c->stream));
    // the blue-noise table is all zeros until the application installs one (bluenoise.cuh:46,189)
    HIP_TRY(c, hipMemsetAsync(c->d_blue, 0, PTRT_BLUE_NOISE_FLOATS * sizeof(float), c->stream));
    c->last_rgb8 = c->d_rgb8;
    // default camera: Camera(aspect, 2, 1) of the Scene constructor (scene.cuh:748, camera.cuh:127-148)
    const float aspect = (float)full_w / (float)full_h;
    const float vw = 2.0f * aspect;
    c->cam.origin = pt::f3{0, 0, 0};
    c->cam.horizontal = pt::f3{vw, 0, 0};
    c->cam.vertical = pt::f3{0, 2.0f, 0};
    c->cam.llc = pt::f3{0.0f - vw * 0.5f, 0.0f - 2.0f * 0.5f, -1.0f};
    c->cam.u = pt::f3{1, 0, 0};
    c->cam.v = pt::f3{0, 1, 0};
    c->cam.w = pt::f3{0, 0, 1};
    c->cam.lens_radius = 0.0f;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}
} // namespace

int ptrt_create(int full_w, int full_h, int tile_y0, int tile_rows, int device, ptrt_ctx **out) {
    if (!out)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_create: out is NULL");
    *out = nullptr;
    if (full_w <= 0 || full_h <= 0)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_create: bad frame size %dx%d", full_w, full_h);
    if (tile_rows <= 0) {
        tile_y0 = 0;
        tile_rows = full_h;
    }
    if (tile_y0 < 0 || tile_y0 + tile_rows > full_h)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_create: tile rows [%d,%d) outside 0..%d", tile_y0,
                    tile_y0 + tile_rows, full_h);
    return create_ctx(full_w, full_h, tile_y0, tile_rows, 1, 0, device, out);
}

int ptrt_create_interleaved(int full_w, int full_h, int phase, int period, int device, ptrt_ctx **out) {
    if (!out)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_create_interleaved: out is NULL");
    *out = nullptr;
    if (full_w <= 0 || full_h <= 0)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_create_interleaved: bad frame size %dx%d", full_w, full_h);
    const int strips = (full_h + 7) / 8;
    if (period < 1 || phase < 0 || phase >= period || phase >= strips)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_create_interleaved: strip %d of every %d (the frame has %d strips of 8 rows)",
                    phase, period, strips);
    if (period == 1)
        return create_ctx(full_w, full_h, 0, full_h, 1, 0, device, out);
    // rows of the strips phase, phase + period, ...; only the frame's last strip can be short, and it is the owner's last
    int rows = 0;
    for (int t = phase; t < strips; t += period)
        rows += (t * 8 + 8 <= full_h) ? 8 : full_h - t * 8;
    return create_ctx(full_w, full_h, phase * 8, rows, period, phase, device, out);
}

void ptrt_destroy(ptrt_ctx *c) {
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        if (!c || !g_live.count(c))
            return; // NULL or already destroyed: ignored, like a repeated cudaFree in the reference
        g_live.erase(c);
    }
    (void)hipSetDevice(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < ptrt_ctx::MAX_SPLIT; ++i) { // the auxiliary streams of split launches
        if (c->aux_stream[i]) {
            (void)hipStreamSynchronize(c->aux_stream[i]);
            (void)hipStreamDestroy(c->aux_stream[i]);
        }
        if (c->split_join[i])
            (void)hipEventDestroy(c->split_join[i]);
    }
    for (int i = 0; i < ptrt_ctx::MAX_SPLIT; ++i) {
        if (c->tm_stream[i]) {
            (void)hipStreamSynchronize(c->tm_stream[i]);
            (void)hipStreamDestroy(c->tm_stream[i]);
        }
        if (c->tm_fork[i])
            (void)hipEventDestroy(c->tm_fork[i]);
        if (c->tm_join[i])
            (void)hipEventDestroy(c->tm_join[i]);
        for (hipEvent_t e : c->launch_ev[i])
            if (e)
                (void)hipEventDestroy(e);
    }
    if (c->split_fork)
        (void)hipEventDestroy(c->split_fork);
    for (hipEvent_t e : c->head_ev)
        if (e)
            (void)hipEventDestroy(e);
    free_scene(c);
    free_staging(c);
    dfree(c->d_materials);
    dfree(c->d_lights);
    dfree(c->d_rng);
    dfree(c->d_accum);
    dfree(c->d_normal);
    dfree(c->d_depth);
    dfree(c->d_object_id);
    dfree(c->alt_accum);
    dfree(c->alt_normal);
    dfree(c->alt_depth);
    dfree(c->alt_object_id);
    dfree(c->d_rgb8);
    dfree(c->wire_rgb8);
    dfree(c->d_counters);
    dfree(c->d_queue);
    dfree(c->wf_st);
    dfree(c->wf_occ);
    dfree(c->wf_live);
    dfree(c->wf_planes);
    dfree(c->wf_hit);
    dfree(c->as_cursor);
    dfree(c->d_blue);
    dfree(c->d_jump);
    dfree(c->d_env);
    free_denoiser(c);
    free_post(c);
    c->present.free();
    for (auto &ev : c->ev_ring)
        if (ev)
            (void)hipEventDestroy(ev);
    if (c->own_stream)
        (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int ptrt_set_blue_noise(ptrt_ctx *c, const float *table) {
    if (!ctx_live(c) || !table)
        return fail(c, PTRT_E_INVALID, "ptrt_set_blue_noise: bad argument");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_blue, table, PTRT_BLUE_NOISE_FLOATS * sizeof(float), hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

int ptrt_reset_rng(ptrt_ctx *c, unsigned long long seed) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_reset_rng: bad context");
    if (int rc = set_device(c))
        return rc;
    // bits needed for the largest global pixel index of this tile
    const unsigned long long last = (unsigned long long)(c->il_period > 1 ? c->H : c->y0 + c->rows) * (unsigned long long)c->W;
    if (int rc = ensure_jump(c, last, "ptrt_reset_rng"))
        return rc;
    const XorwowSeed s = xorwow_seed(seed);
    const int grid = (int)((c->npix + 255) / 256);
    hipLaunchKernelGGL(pt::xorwow_init_kernel, dim3(grid), dim3(256), 0, c->stream, c->d_rng, c->W, c->rows, c->y0,
                       c->il_period, c->il_phase, s.d, s.v[0], s.v[1], s.v[2], s.v[3], s.v[4], c->d_jump, c->n_jump);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the reference synchronises here too (scene.cuh:455)
    c->rng_ready = true;
    return PTRT_OK;
}

int ptrt_upload_materials(ptrt_ctx *c, const ptrt_materials *m) {
    if (!ctx_live(c) || !m || m->count <= 0)
        return fail(c, PTRT_E_INVALID, "ptrt_upload_materials: bad argument");
    if (!m->albedo || !m->specular || !m->metallic || !m->roughness || !m->emission || !m->ior || !m->transmission ||
        !m->transmission_roughness || !m->clearcoat || !m->clearcoat_roughness || !m->sheen || !m->sheen_tint ||
        !m->iridescence || !m->iridescence_thickness)
        return fail(c, PTRT_E_INVALID, "ptrt_upload_materials: a required array is NULL");
    if (int rc = set_device(c))
        return rc;
    std::vector<float4> recs((size_t)m->count * 6);
    c->h_shadow_skip.assign(m->count, 0);
    bool full = false;
    for (int i = 0; i < m->count; ++i) {
        float4 *r = &recs[(size_t)i * 6];
        r[0] = f4(m->albedo[i].x, m->albedo[i].y, m->albedo[i].z, m->metallic[i]);
        r[1] = f4(m->specular[i].x, m->specular[i].y, m->specular[i].z, m->roughness[i]);
        r[2] = f4(m->emission[i].x, m->emission[i].y, m->emission[i].z, m->transmission[i]);
        r[3] = f4(m->sheen_tint[i].x, m->sheen_tint[i].y, m->sheen_tint[i].z, m->ior[i]);
        r[4] = f4(m->transmission_roughness[i], m->clearcoat[i], m->clearcoat_roughness[i], m->iridescence[i]);
        r[5] = f4(m->iridescence_thickness[i], m->sheen[i], 0.0f, 0.0f);
        c->h_shadow_skip[i] = (m->transmission[i] > 0.5f) ? 1 : 0;
        // the lean shading variant drops branches that are provably dead when all of these are <= 0
        if (!(m->transmission[i] <= 0.0f) || !(m->clearcoat[i] <= 0.0f) || !(m->iridescence[i] <= 0.0f) ||
            !(m->sheen[i] <= 0.0f))
            full = true;
    }
    if (int rc = upload(c, c->d_materials, recs))
        return rc;
    c->n_materials = m->count;
    c->mats_full = full;
    c->have_materials = true;
    if (c->have_geometry)
        return push_mesh_recs(c, false);
    return PTRT_OK;
}

int ptrt_upload_lights(ptrt_ctx *c, const ptrt_light *lights, int n) {
    if (!ctx_live(c) || n < 0 || (n > 0 && !lights))
        return fail(c, PTRT_E_INVALID, "ptrt_upload_lights: bad argument");
    if (int rc = set_device(c))
        return rc;
    std::vector<float4> recs((size_t)n * 4);
    for (int i = 0; i < n; ++i) {
        const ptrt_light &l = lights[i];
        if (l.type < 0 || l.type > 2)
            return fail(c, PTRT_E_INVALID, "light %d: unknown type %d", i, l.type);
        recs[(size_t)i * 4 + 0] = f4(l.position.x, l.position.y, l.position.z, as_f(l.type));
        recs[(size_t)i * 4 + 1] = f4(l.direction.x, l.direction.y, l.direction.z, l.intensity);
        recs[(size_t)i * 4 + 2] = f4(l.color.x, l.color.y, l.color.z, l.range);
        recs[(size_t)i * 4 + 3] = f4(l.inner_cone, l.outer_cone, l.radius, 0.0f);
    }
    if (int rc = upload(c, c->d_lights, recs))
        return rc;
    c->n_lights = n;
    return PTRT_OK;
}

int ptrt_set_camera(ptrt_ctx *c, const ptrt_camera *cam) {
    if (!ctx_live(c, false) || !cam)
        return fail(c, PTRT_E_INVALID, "ptrt_set_camera: bad argument");
    auto v = [](const ptrt_vec3 &a) { return pt::f3{a.x, a.y, a.z}; };
    c->cam.origin = v(cam->origin);
    c->cam.llc = v(cam->lower_left_corner);
    c->cam.horizontal = v(cam->horizontal);
    c->cam.vertical = v(cam->vertical);
    c->cam.u = v(cam->u);
    c->cam.v = v(cam->v);
    c->cam.w = v(cam->w);
    c->cam.lens_radius = cam->lens_radius;
    return PTRT_OK;
}

int ptrt_set_sky(ptrt_ctx *c, const ptrt_vec3 *top, const ptrt_vec3 *bottom, int use_sky) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_set_sky: bad context");
    if (top)
        c->sky_top = pt::f3{top->x, top->y, top->z};
    if (bottom)
        c->sky_bottom = pt::f3{bottom->x, bottom->y, bottom->z};
    c->use_sky = use_sky ? 1 : 0;
    return PTRT_OK;
}

int ptrt_upload_scene(ptrt_ctx *c, const ptrt_scene_desc *s) {
    if (!ctx_live(c) || !s)
        return fail(c, PTRT_E_INVALID, "ptrt_upload_scene: bad argument");
    if (int rc = ptrt_upload_geometry(c, s->meshes, s->mesh_count, s->tlas_nodes, s->tlas_node_count,
                                      s->tlas_mesh_indices, s->tlas_index_count))
        return rc;
    if (int rc = ptrt_upload_materials(c, &s->materials))
        return rc;
    if (int rc = ptrt_upload_lights(c, s->lights, s->light_count))
        return rc;
    if (int rc = ptrt_set_camera(c, &s->camera))
        return rc;
    if (int rc = ptrt_set_env_map(c, s->env_rgba, s->env_width, s->env_height))
        return rc;
    return ptrt_set_sky(c, &s->sky_top, &s->sky_bottom, s->use_sky);
}

int ptrt_set_env_map(ptrt_ctx *c, const float *rgba, int width, int height) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_set_env_map: bad context");
    if (rgba && (width < 1 || height < 1))
        return fail(c, PTRT_E_INVALID, "ptrt_set_env_map: %dx%d is not a map size", width, height);
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // frames in flight may still read the old map
    dfree(c->d_env);
    c->env_w = c->env_h = 0;
    if (!rgba)
        return PTRT_OK;
    const size_t bytes = (size_t)width * height * 16;
    HIP_TRY(c, hipMalloc((void **)&c->d_env, bytes));
    HIP_TRY(c, hipMemcpyAsync(c->d_env, rgba, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->env_w = width;
    c->env_h = height;
    return PTRT_OK;
}

void ptrt_denoiser_default_settings(ptrt_denoiser_settings *s) {
    if (!s)
        return;
    // DenoiserSettings defaults, diffuse_* channel (denoiser.cuh:40-72)
    *s = ptrt_denoiser_settings{0.06f, 0.05f, 32.0f, 4.0f, 64.0f, 0.5f, 5,    1.2f, 3.0f,
                                0.1f,  0.005f, 0.95f, 1e9f, 0.01f, 0.95f, 1,  1};
}

int ptrt_denoiser_enable(ptrt_ctx *c, const ptrt_denoiser_settings *s) {
    static_assert(sizeof(ptrt_denoiser_settings) == sizeof(pt::DenoiseSettings), "settings mirror");
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_denoiser_enable: bad context");
    if (c->rows != c->H || c->y0 != 0)
        return fail(c, PTRT_E_INVALID, "ptrt_denoiser_enable: the denoiser needs a full-frame context (its filters "
                                       "read across band borders); denoise on the presenting rank instead");
    if (int rc = set_device(c))
        return rc;
    ptrt_denoiser_settings d;
    ptrt_denoiser_default_settings(&d);
    if (s)
        d = *s;
    free_denoiser(c);
    std::memcpy(&c->dn, &d, sizeof d);
    const size_t n = c->rpix(); // "(re)create at current render resolution" (scene.cuh:1984-1996)
    HIP_TRY(c, hipMalloc((void **)&c->dn_cur4, n * 16));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c, hipMalloc((void **)&c->dn_c4[k], n * 16));
        HIP_TRY(c, hipMalloc((void **)&c->dn_g4[k], n * 16));
        HIP_TRY(c, hipMalloc((void **)&c->dn_h1[k], n * 16));
        HIP_TRY(c, hipMalloc((void **)&c->dn_h2[k], n * 16));
    }
    HIP_TRY(c, hipMalloc((void **)&c->dn_hobj, n * 4));
    HIP_TRY(c, hipMalloc((void **)&c->dn_motion, n * 8));
    HIP_TRY(c, hipMalloc((void **)&c->dn_out, n * 12));
    HIP_TRY(c, hipMalloc((void **)&c->dn_pvp, 16 * sizeof(float)));
    HIP_TRY(c, hipMemsetAsync(c->dn_out, 0, n * 12, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dn_motion, 0, n * 8, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->dn_cur = 0;
    c->dn_first = true;
    c->dn_on = true;
    return PTRT_OK;
}

int ptrt_denoiser_disable(ptrt_ctx *c) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_denoiser_disable: bad context");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_denoiser(c);
    return PTRT_OK;
}

int ptrt_set_prev_view_proj(ptrt_ctx *c, const float *m16) {
    if (!ctx_live(c, false) || !m16)
        return fail(c, PTRT_E_INVALID, "ptrt_set_prev_view_proj: bad argument");
    std::memcpy(c->prev_view_proj, m16, sizeof c->prev_view_proj);
    return PTRT_OK;
}

int ptrt_set_render_size(ptrt_ctx *c, int render_w, int render_h) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_set_render_size: bad context");
    if (render_w == c->rw && render_h == c->rh)
        return PTRT_OK;
    if (c->rows != c->H || c->y0 != 0)
        return fail(c, PTRT_E_INVALID, "ptrt_set_render_size: only full-frame contexts can render at a reduced size");
    if (render_w < 1 || render_h < 1 || render_w > c->W || render_h > c->H)
        return fail(c, PTRT_E_INVALID, "ptrt_set_render_size: %dx%d is not within 1x1 .. %dx%d", render_w, render_h, c->W, c->H);
    if (c->bloom_on && (render_w < 64 || render_h < 64))
        return fail(c, PTRT_E_INVALID, "ptrt_set_render_size: bloom needs at least 64x64 (six mip levels)");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dfree(c->s_accum);
    dfree(c->s_normal);
    dfree(c->s_depth);
    dfree(c->s_object_id);
    free_denoiser(c); // its images have the old size; the caller re-enables it (Scene::updateScaledBuffers does)
    c->rw = render_w;
    c->rh = render_h;
    if (c->scaled()) {
        const size_t n = c->rpix();
        HIP_TRY(c, hipMalloc((void **)&c->s_accum, n * 12));
        HIP_TRY(c, hipMalloc((void **)&c->s_normal, n * 12));
        HIP_TRY(c, hipMalloc((void **)&c->s_depth, n * 4));
        HIP_TRY(c, hipMalloc((void **)&c->s_object_id, n * 4));
        HIP_TRY(c, hipMemsetAsync(c->s_accum, 0, n * 12, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return PTRT_OK;
}

int ptrt_set_bloom(ptrt_ctx *c, int enabled) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_set_bloom: bad context");
    if (!enabled) {
        c->bloom_on = 0; // the mips stay allocated, as in the reference
        return PTRT_OK;
    }
    if (c->rows != c->H || c->y0 != 0)
        return fail(c, PTRT_E_INVALID, "ptrt_set_bloom: bloom needs a full-frame context (its blur reads across band "
                                       "borders); apply it on the presenting rank instead");
    if (c->rw < 64 || c->rh < 64)
        return fail(c, PTRT_E_INVALID, "ptrt_set_bloom: bloom needs at least 64x64 pixels: below that one of the six mip "
                                       "levels is empty (the reference would read a NULL mip, scene.cuh:812-816,1175)");
    if (int rc = set_device(c))
        return rc;
    int mw = c->W, mh = c->H;
    for (int i = 0; i < 6; ++i) { // scene.cuh:809-822: sized from the FULL frame
        mw /= 2;
        mh /= 2;
        if (!c->bl_mip[i]) {
            c->touched = true; // (the first time only: a caller that sets the flag every frame keeps its frames overlapping)
            HIP_TRY(c, hipMalloc((void **)&c->bl_mip[i], (size_t)mw * mh * 12));
        }
    }
    c->bloom_on = 1;
    return PTRT_OK;
}

int ptrt_sync(ptrt_ctx *c) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_sync: bad context");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

int ptrt_set_stream(ptrt_ctx *c, void *hip_stream) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_set_stream: bad context");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // finish what was queued on the old stream
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    c->launches = 0;
    c->timed = false;
    memset(c->launch_timed, 0, sizeof c->launch_timed);
    memset(c->ev_ms_known, 0, sizeof c->ev_ms_known);
    memset(c->launch_ms_known, 0, sizeof c->launch_ms_known);
    return PTRT_OK;
}

void *ptrt_device_buffer(ptrt_ctx *c, int kind) {
    if (!ctx_live(c))
        return nullptr;
    c->escaped = true; // (the caller may read the context's buffers on streams of its own: frames no longer overlap)
    switch (kind) {
    case PTRT_BUF_ACCUM: return c->d_accum;
    case PTRT_BUF_NORMAL: return c->scaled() ? c->s_normal : c->d_normal;
    case PTRT_BUF_DEPTH: return c->scaled() ? c->s_depth : c->d_depth;
    case PTRT_BUF_OBJECT_ID: return c->scaled() ? c->s_object_id : c->d_object_id;
    case PTRT_BUF_RENDER_ACCUM: return c->scaled() ? c->s_accum : c->d_accum;
    case PTRT_BUF_RGB8: return c->last_rgb8;
    case PTRT_BUF_DENOISED: return c->dn_on ? c->dn_out : nullptr;
    case PTRT_BUF_MOTION: return c->dn_on ? c->dn_motion : nullptr;
    default: return nullptr;
    }
}

int ptrt_read_buffer(ptrt_ctx *c, int kind, void *dst, size_t bytes) {
    if (!ctx_live(c) || !dst)
        return fail(c, PTRT_E_INVALID, "ptrt_read_buffer: bad argument");
    if (int rc = set_device(c))
        return rc;
    size_t need = 0;
    const void *src = nullptr;
    switch (kind) {
    // G-buffers, denoiser images and RENDER_ACCUM hold render-size frames (== the frame size unless
    // ptrt_set_render_size reduced it); ACCUM is the full-size HDR image that was tonemapped
    case PTRT_BUF_ACCUM: need = c->npix * 12; src = c->d_accum; break;
    case PTRT_BUF_RENDER_ACCUM: need = c->rpix() * 12; src = c->scaled() ? c->s_accum : c->d_accum; break;
    case PTRT_BUF_NORMAL: need = c->rpix() * 12; src = c->scaled() ? c->s_normal : c->d_normal; break;
    case PTRT_BUF_DEPTH: need = c->rpix() * 4; src = c->scaled() ? c->s_depth : c->d_depth; break;
    case PTRT_BUF_OBJECT_ID: need = c->rpix() * 4; src = c->scaled() ? c->s_object_id : c->d_object_id; break;
    case PTRT_BUF_RGB8: need = c->npix * 3; src = c->last_rgb8; break;
    case PTRT_BUF_RNG: need = c->npix * 24; break;
    case PTRT_BUF_DENOISED:
    case PTRT_BUF_MOTION:
        if (!c->dn_on)
            return fail(c, PTRT_E_NOT_READY, "ptrt_read_buffer: the denoiser is not enabled");
        need = c->rpix() * (kind == PTRT_BUF_DENOISED ? 12 : 8);
        src = kind == PTRT_BUF_DENOISED ? c->dn_out : c->dn_motion;
        break;
    default: return fail(c, PTRT_E_INVALID, "ptrt_read_buffer: unknown kind %d", kind);
    }
    if (bytes < need)
        return fail(c, PTRT_E_INVALID, "ptrt_read_buffer: destination holds %zu bytes, need %zu", bytes, need);
    if (kind == PTRT_BUF_RGB8 && !src) // (the last frame went straight into a caller's frame: PTRT_OUT_DEVICE_FRAME)
        return fail(c, PTRT_E_NOT_READY, "ptrt_read_buffer: the last frame was written into the caller's frame, the context holds no RGB8 image of it");
    if (kind == PTRT_BUF_RNG) {
        DeviceTemp<uint32_t> tmp;
        HIP_TRY(c, tmp.alloc(c->npix * 6));
        hipLaunchKernelGGL(pt::rng_planar_to_aos, dim3((unsigned)((c->npix + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_rng, tmp.p, c->npix);
        HIP_TRY(c, hipMemcpyAsync(dst, tmp.p, need, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return PTRT_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

int ptrt_write_rng(ptrt_ctx *c, const uint32_t *states, size_t bytes) {
    if (!ctx_live(c) || !states || bytes < c->npix * 24)
        return fail(c, PTRT_E_INVALID, "ptrt_write_rng: bad argument");
    if (int rc = set_device(c))
        return rc;
    DeviceTemp<uint32_t> tmp;
    HIP_TRY(c, tmp.alloc(c->npix * 6));
    HIP_TRY(c, hipMemcpyAsync(tmp.p, states, c->npix * 24, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pt::rng_aos_to_planar, dim3((unsigned)((c->npix + 255) / 256)), dim3(256), 0, c->stream, tmp.p,
                       c->d_rng, c->npix);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->rng_ready = true;
    return PTRT_OK;
}

} // extern "C"

#include "ptrt_query.hip.h"

extern "C" {

int ptrt_render_wireframe(ptrt_ctx *c, float thickness, void *out_rgb8, int out_is_device) {
    if (!ctx_live(c)) // (marks the context touched: a pipelined path frame that follows waits for the stream, and so for this)
        return fail(c, PTRT_E_INVALID, "ptrt_render_wireframe: bad context");
    if (c->il_period > 1)
        return fail(c, PTRT_E_INVALID, "ptrt_render_wireframe: an interleaved context (its strips are assembled by the tile farm, "
                                       "which has no wireframe view); use a full-frame or band context");
    if (!out_rgb8 || out_is_device < PTRT_OUT_HOST || out_is_device > PTRT_OUT_DEVICE_FRAME)
        return fail(c, PTRT_E_INVALID, "ptrt_render_wireframe: needs a target (out_rgb8 %p, out_is_device %d)", out_rgb8,
                    out_is_device);
    if (!c->have_geometry || !c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "ptrt_render_wireframe: %s not uploaded", c->have_geometry ? "materials" : "geometry");
    if (c->n_materials < c->n_meshes)
        return fail(c, PTRT_E_NOT_READY, "ptrt_render_wireframe: %d materials for %d meshes", c->n_materials, c->n_meshes);
    if (int rc = set_device(c))
        return rc;
    if (!out_is_device && !c->wire_rgb8)
        HIP_TRY(c, hipMalloc((void **)&c->wire_rgb8, c->npix * 3));
    pt::KParams K = make_params(c);
    // the full frame, whatever the render size of the path tracer (the reference launches width x height)
    K.width = c->W;
    K.height = c->H;
    K.y0 = c->y0;
    K.rows = c->rows;
    K.tiles_x = (c->W + 7) / 8;
    K.rng = nullptr;
    K.accum = K.normal = K.depth = nullptr;
    K.object_id = nullptr;
    K.counters = nullptr;
    K.rgb8 = out_is_device ? (unsigned char *)out_rgb8 : c->wire_rgb8;
    K.rgb8_frame = out_is_device == PTRT_OUT_DEVICE_FRAME ? 1 : 0;
    const int geom = pick_geom(c);
    const size_t lds = trace_lds_bytes(c, geom, 0);
    const dim3 grid(K.tiles_x, (c->rows + 7) / 8);
    if (geom == 0)
        hipLaunchKernelGGL(pt::wireframe_kernel<0>, grid, dim3(64), lds, c->stream, K, thickness);
    else if (geom == 1)
        hipLaunchKernelGGL(pt::wireframe_kernel<1>, grid, dim3(64), lds, c->stream, K, thickness);
    else
        hipLaunchKernelGGL(pt::wireframe_kernel<2>, grid, dim3(64), lds, c->stream, K, thickness);
    HIP_TRY(c, hipGetLastError());
    if (out_is_device == PTRT_OUT_DEVICE)
        ring_mark_rendered(out_rgb8, c->stream);
    if (!out_is_device) {
        HIP_TRY(c, hipMemcpyAsync(out_rgb8, c->wire_rgb8, c->npix * 3, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return PTRT_OK;
}

// The baked-light view: baked_view_kernel (pt_baked.hip.h) through the queries' plan, variant and persistent grid, into the
// wireframe view's targets.  Every refusal comes before anything is enqueued.
int ptrt_render_baked(ptrt_ctx *c, int frame_index, const ptrt_baked_view *view, void *out_rgb8, int out_is_device) {
    const char *fn = "ptrt_render_baked";
    if (!ctx_live(c)) // (marks the context touched: a pipelined path frame that follows waits for the stream, and so for this)
        return fail(c, PTRT_E_INVALID, "%s: bad context", fn);
    if (c->il_period > 1)
        return fail(c, PTRT_E_INVALID, "%s: an interleaved context (its strips are assembled by the tile farm, which has no baked "
                                       "view); use a full-frame or band context", fn);
    if (!view)
        return fail(c, PTRT_E_INVALID, "%s: view is NULL", fn);
    if (frame_index < 0)
        return fail(c, PTRT_E_INVALID, "%s: frame_index=%d", fn, frame_index);
    if (c->cam.lens_radius > 0.0f)
        return fail(c, PTRT_E_INVALID, "%s: a thin lens (lens_radius %g): the lens sample of a primary ray is drawn from the pixel's "
                                       "generator stream", fn, (double)c->cam.lens_radius);
    if (out_is_device < PTRT_OUT_HOST || out_is_device > PTRT_OUT_DEVICE_FRAME || (!out_rgb8 && !view->d_hdr))
        return fail(c, PTRT_E_INVALID, "%s: needs a target (out_rgb8 %p, out_is_device %d, d_hdr %p)", fn, out_rgb8, out_is_device,
                    (const void *)view->d_hdr);
    const bool lightmap = view->d_image != nullptr, probes = view->d_probes != nullptr;
    // the lightmap half: what ptrt_query_lightmap refuses
    if (lightmap) {
        if (view->n_chart_faces < 1 || !view->d_charts || !view->d_chart_first || !atlas_size_ok(view->atlas_w, view->atlas_h) ||
            (view->lightmap_mode != PTRT_LIGHTMAP_NEAREST && view->lightmap_mode != PTRT_LIGHTMAP_BILINEAR))
            return fail(c, PTRT_E_INVALID, "%s: lightmap: bad argument (charts %p, n_chart_faces %d: >= 1, chart_first %p, atlas %d x %d: "
                                           "1 x 1 .. 2^28 texels, mode %d: 0 or 1)", fn, (const void *)view->d_charts, view->n_chart_faces,
                        (const void *)view->d_chart_first, view->atlas_w, view->atlas_h, view->lightmap_mode);
        if (!aligned16(view->d_image) || ((uintptr_t)view->d_charts & 3u) || ((uintptr_t)view->d_chart_first & 3u))
            return fail(c, PTRT_E_INVALID, "%s: lightmap: image %p must be 16-byte aligned, charts %p and chart_first %p 4-byte", fn,
                        (const void *)view->d_image, (const void *)view->d_charts, (const void *)view->d_chart_first);
    }
    // the probe half: what ptrt_query_probe_light refuses
    long long probe_rows = 1;
    if (probes) {
        if ((view->probe_mode != PTRT_PROBES_TRILINEAR && view->probe_mode != PTRT_PROBES_VISIBILITY) || !(view->normal_bias >= 0.0f) ||
            !std::isfinite(view->normal_bias))
            return fail(c, PTRT_E_INVALID, "%s: probes: bad argument (mode %d: 0 or 1, normal_bias %g: >= 0 and finite)", fn,
                        view->probe_mode, (double)view->normal_bias);
        for (int a = 0; a < 3; ++a) {
            const ptrt_probe_volume &vol = view->volume;
            if (vol.counts[a] < 1 || !(vol.spacing[a] > 0.0f) || !std::isfinite(vol.spacing[a]) || !std::isfinite(vol.origin[a]))
                return fail(c, PTRT_E_INVALID, "%s: volume axis %d: count %d (>= 1), spacing %g (positive and finite), origin %g (finite)",
                            fn, a, vol.counts[a], (double)vol.spacing[a], (double)vol.origin[a]);
            probe_rows *= vol.counts[a]; // each factor < 2^31 and the product so far <= 2^24: no overflow
            if (probe_rows > (1ll << 24))
                return fail(c, PTRT_E_INVALID, "%s: a volume of %d x %d x %d probes (at most 2^24)", fn, vol.counts[0], vol.counts[1],
                            vol.counts[2]);
        }
        if (!aligned16(view->d_probes))
            return fail(c, PTRT_E_INVALID, "%s: probes %p must be 16-byte aligned", fn, (const void *)view->d_probes);
    }
    if (((uintptr_t)view->d_hdr & 3u) || ((uintptr_t)view->d_normal & 3u) || ((uintptr_t)view->d_depth & 3u) || ((uintptr_t)view->d_object_id & 3u))
        return fail(c, PTRT_E_INVALID, "%s: hdr %p, normal %p, depth %p and object_id %p must be 4-byte aligned", fn, (const void *)view->d_hdr,
                    (const void *)view->d_normal, (const void *)view->d_depth, (const void *)view->d_object_id);
    if (!c->have_geometry || !c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "%s: %s not uploaded", fn, c->have_geometry ? "materials" : "geometry");
    if (c->n_materials < c->n_meshes)
        return fail(c, PTRT_E_NOT_READY, "%s: %d materials for %d meshes", fn, c->n_materials, c->n_meshes);
    // the spans: every output apart from every input and from every other output, all of them the context's device memory
    const size_t pix = (size_t)c->rows * (size_t)c->W;
    const Span ins[4] = {{"charts", view->d_charts, lightmap ? (size_t)view->n_chart_faces * 24 : 0},
                         {"chart_first", view->d_chart_first, lightmap ? (size_t)c->n_meshes * sizeof(int32_t) : 0},
                         {"image", view->d_image, lightmap ? (size_t)view->atlas_w * (size_t)view->atlas_h * 16 : 0},
                         {"probes", view->d_probes, probes ? (size_t)probe_rows * sizeof(ptrt_probe) : 0}};
    const Span outs[5] = {{"hdr", view->d_hdr, pix * 12},
                          {"normal", view->d_normal, pix * 12},
                          {"depth", view->d_depth, pix * 4},
                          {"object_id", view->d_object_id, pix * 4},
                          {"out_rgb8", out_is_device ? out_rgb8 : nullptr,
                           (out_is_device == PTRT_OUT_DEVICE_FRAME ? (size_t)c->H : (size_t)c->rows) * (size_t)c->W * 3}};
    for (int i = 0; i < 5; ++i) {
        if (!outs[i].p)
            continue;
        for (const Span &s : ins)
            if (s.bytes && !spans_apart(outs[i], s))
                return fail(c, PTRT_E_INVALID, "%s: %s %p (%zu bytes) overlaps %s %p (%zu bytes)", fn, outs[i].name, outs[i].p, outs[i].bytes,
                            s.name, s.p, s.bytes);
        for (int j = 0; j < i; ++j)
            if (outs[j].p && !spans_apart(outs[i], outs[j]))
                return fail(c, PTRT_E_INVALID, "%s: %s %p (%zu bytes) overlaps %s %p (%zu bytes)", fn, outs[i].name, outs[i].p, outs[i].bytes,
                            outs[j].name, outs[j].p, outs[j].bytes);
    }
    if (int rc = set_device(c))
        return rc;
    for (const Span &s : ins)
        if (s.bytes && !device_span(c, s.p, s.bytes))
            return fail(c, PTRT_E_INVALID, "%s: %s is not %zu bytes of device memory on device %d", fn, s.name, s.bytes, c->device);
    for (const Span &s : outs)
        if (s.p && !device_span(c, s.p, s.bytes))
            return fail(c, PTRT_E_INVALID, "%s: %s is not %zu bytes of device memory on device %d", fn, s.name, s.bytes, c->device);
    if (!out_is_device && out_rgb8 && !c->wire_rgb8)
        HIP_TRY(c, hipMalloc((void **)&c->wire_rgb8, c->npix * 3));

    pt::BakedViewParams B{};
    if (lightmap) {
        B.L.charts = view->d_charts;
        B.L.chart_first = view->d_chart_first;
        B.L.image = reinterpret_cast<const float4 *>(view->d_image);
        B.L.n_chart_faces = view->n_chart_faces;
        B.L.n_meshes = c->n_meshes;
        B.L.aw = view->atlas_w;
        B.L.ah = view->atlas_h;
        B.L.mode = view->lightmap_mode;
    }
    if (probes) {
        B.V.probes = reinterpret_cast<const float4 *>(view->d_probes);
        for (int a = 0; a < 3; ++a) {
            B.V.origin[a] = view->volume.origin[a];
            B.V.spacing[a] = view->volume.spacing[a];
            B.V.counts[a] = view->volume.counts[a];
        }
        B.V.mode = view->probe_mode;
        B.V.bias = view->normal_bias;
    }
    B.hdr = view->d_hdr;
    B.normal = view->d_normal;
    B.depth = view->d_depth;
    B.object_id = view->d_object_id;
    QueryPlan P;
    if (int rc = plan_query(c, false, 0, 0, P))
        return rc;
    // the full frame, whatever the render size of the path tracer; the context's own per-pixel buffers are no business of the view's
    P.K.width = c->W;
    P.K.height = c->H;
    P.K.y0 = c->y0;
    P.K.rows = c->rows;
    P.K.tiles_x = (c->W + 7) / 8;
    P.K.frame_count = frame_index;
    P.K.rng = nullptr;
    P.K.accum = P.K.normal = P.K.depth = nullptr;
    P.K.object_id = nullptr;
    P.K.counters = nullptr;
    P.K.rgb8 = !out_rgb8 ? nullptr : out_is_device ? (unsigned char *)out_rgb8 : c->wire_rgb8;
    P.K.rgb8_frame = out_is_device == PTRT_OUT_DEVICE_FRAME ? 1 : 0;
    const size_t tiles = (size_t)P.K.tiles_x * (size_t)((c->rows + 7) / 8);
    if (int rc = with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
            return launch_persistent(c, pt::baked_view_kernel<G, PM>, P.lds, tiles, true, P.K, B);
        }))
        return rc;
    if (out_rgb8 && out_is_device == PTRT_OUT_DEVICE)
        ring_mark_rendered(out_rgb8, c->stream);
    if (out_rgb8 && !out_is_device) {
        HIP_TRY(c, hipMemcpyAsync(out_rgb8, c->wire_rgb8, c->npix * 3, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return PTRT_OK;
}

int ptrt_get_stats(ptrt_ctx *c, ptrt_stats *out) {
    if (!ctx_live(c) || !out)
        return fail(c, PTRT_E_INVALID, "ptrt_get_stats: bad argument");
    if (int rc = set_device(c))
        return rc;
    // per-workgroup slots (no atomics in the kernel, see pt_render.hip.h): summed here
    std::vector<unsigned long long> slots(c->n_counter_slots * pt::COUNTER_WORDS);
    HIP_TRY(c, hipMemcpyAsync(slots.data(), c->d_counters, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, slots.size() * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long h[pt::COUNTER_WORDS] = {0, 0, 0, 0};
    for (size_t i = 0; i < slots.size(); ++i)
        h[i % pt::COUNTER_WORDS] += slots[i];
    out->extension_rays = h[0];
    out->shadow_rays = h[1];
    out->paths = h[2];
    out->shadow_rays_walked = h[1] - h[3];
    return PTRT_OK;
}

} // extern "C"

#include "ptrt_options.hip.h"

#include "ptrt_farm.hip.h"

// =====================================================================================
// The one-bounce ray tracer (include/ptrt.h "ptrt_rt_*"; kernel rt_render.hip.h)
static_assert(sizeof(ptrt_rt_material) == sizeof(rt::Mat), "ptrt_rt_material and rt::Mat differ");
static_assert(sizeof(ptrt_rt_light) == sizeof(rt::LightDev), "ptrt_rt_light and rt::LightDev differ");

struct ptrt_rt_ctx {
    int device = 0, W = 0, H = 0;
    hipStream_t stream = nullptr;
    std::string err;
    struct Slot {
        float4 *tris = nullptr; // 3 per face: v0, v1 - v0, v2 - v0
        int faces = 0;
        float4 *nodes = nullptr; // 2 per node
        int node_count = 0;
        int *prims = nullptr;
        int max_prim = -1; // the largest face index the tree names
    };
    std::vector<Slot> slots;
    std::vector<ptrt_rt_mesh> meshes; // the last ptrt_rt_set_scene
    std::vector<ptrt_rt_light> lights;
    bool have_scene = false;
    rt::MeshDev *d_desc = nullptr;
    int desc_cap = 0;
    rt::LightDev *d_lights = nullptr;
    int light_cap = 0;
    unsigned char *d_out = nullptr; // staging of PTRT_OUT_HOST renders
};

namespace {
std::set<ptrt_rt_ctx *> g_rt_live;

bool rt_live(const ptrt_rt_ctx *c) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    return c && g_rt_live.count(const_cast<ptrt_rt_ctx *>(c));
}

// as fail(): a stale handle is never written to
int rt_fail(ptrt_rt_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (c) {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        if (g_rt_live.count(c))
            c->err = buf;
    }
    return code;
}

#define RT_TRY(c, call)                                                                                        \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return rt_fail((c), PTRT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_));                    \
    } while (0)

float rt_bits(int i) {
    float f;
    std::memcpy(&f, &i, sizeof f);
    return f;
}

void rt_free_slot(ptrt_rt_ctx::Slot &s) {
    dfree(s.tris);
    dfree(s.nodes);
    dfree(s.prims);
    s = ptrt_rt_ctx::Slot{};
}
} // namespace

extern "C" {

int ptrt_rt_create(int width, int height, int device, ptrt_rt_ctx **out) {
    if (!out)
        return rt_fail(nullptr, PTRT_E_INVALID, "ptrt_rt_create: out is NULL");
    *out = nullptr;
    if (width <= 0 || height <= 0)
        return rt_fail(nullptr, PTRT_E_INVALID, "ptrt_rt_create: bad frame size %dx%d", width, height);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return rt_fail(nullptr, PTRT_E_NO_DEVICE, "ptrt_rt_create: no HIP device available (%s); this library has no CPU path",
                       e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return rt_fail(nullptr, PTRT_E_NO_DEVICE, "ptrt_rt_create: device %d out of range (have %d)", device, ndev);
    RT_TRY(nullptr, hipSetDevice(device));
    ptrt_rt_ctx *c = new ptrt_rt_ctx();
    c->device = device;
    c->W = width;
    c->H = height;
    if (hipStreamCreate(&c->stream) != hipSuccess) {
        delete c;
        return rt_fail(nullptr, PTRT_E_HIP, "ptrt_rt_create: hipStreamCreate failed");
    }
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_rt_live.insert(c);
    }
    *out = c;
    return PTRT_OK;
}

void ptrt_rt_destroy(ptrt_rt_ctx *c) {
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        if (!c || !g_rt_live.count(c))
            return;
        g_rt_live.erase(c);
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &s : c->slots)
        rt_free_slot(s);
    dfree(c->d_desc);
    dfree(c->d_lights);
    dfree(c->d_out);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *ptrt_rt_last_error(const ptrt_rt_ctx *c) {
    if (rt_live(c))
        return c->err.c_str();
    return g_last_error.c_str();
}

int ptrt_rt_upload_mesh(ptrt_rt_ctx *c, int index, const ptrt_vec3 *verts, int vert_count, const ptrt_tri *faces,
                        int face_count) {
    if (!rt_live(c))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_mesh: bad context");
    if (index < 0 || index > (int)c->slots.size())
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_mesh: slot %d of %d", index, (int)c->slots.size());
    if (vert_count < 0 || face_count < 0 || (face_count > 0 && (!verts || !faces)))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_mesh: bad arrays (%d vertices, %d faces)", vert_count, face_count);
    std::vector<float4> rec((size_t)face_count * 3);
    for (int f = 0; f < face_count; ++f) {
        const ptrt_tri t = faces[f];
        if (t.v0 < 0 || t.v1 < 0 || t.v2 < 0 || t.v0 >= vert_count || t.v1 >= vert_count || t.v2 >= vert_count)
            return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_mesh: face %d references a vertex out of range", f);
        const ptrt_vec3 a = verts[t.v0], b = verts[t.v1], d = verts[t.v2];
        rec[3 * f + 0] = make_float4(a.x, a.y, a.z, 0.0f);
        rec[3 * f + 1] = make_float4(b.x - a.x, b.y - a.y, b.z - a.z, 0.0f);
        rec[3 * f + 2] = make_float4(d.x - a.x, d.y - a.y, d.z - a.z, 0.0f);
    }
    RT_TRY(c, hipSetDevice(c->device));
    RT_TRY(c, hipStreamSynchronize(c->stream)); // a render in flight may still read the old buffer
    if (index == (int)c->slots.size())
        c->slots.emplace_back();
    ptrt_rt_ctx::Slot &s = c->slots[index];
    dfree(s.tris);
    s.faces = 0;
    if (face_count > 0) {
        RT_TRY(c, hipMalloc((void **)&s.tris, rec.size() * sizeof(float4)));
        RT_TRY(c, hipMemcpy(s.tris, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    s.faces = face_count;
    return PTRT_OK;
}

int ptrt_rt_upload_bvh(ptrt_rt_ctx *c, int index, const ptrt_bvh_node *nodes, int node_count, const int32_t *prims,
                       int prim_count) {
    if (!rt_live(c))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_bvh: bad context");
    if (index < 0 || index >= (int)c->slots.size())
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_bvh: slot %d of %d (upload the mesh first)", index, (int)c->slots.size());
    if (node_count < 0 || prim_count < 0 || (node_count > 0 && !nodes) || (prim_count > 0 && !prims))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_bvh: bad arrays (%d nodes, %d primitives)", node_count, prim_count);
    std::vector<float4> rec((size_t)node_count * 2);
    for (int i = 0; i < node_count; ++i) {
        const ptrt_bvh_node &n = nodes[i];
        int a, b;
        if (n.count > 0) {
            if (n.start < 0 || n.start > prim_count - n.count)
                return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_bvh: leaf %d's range [%d, +%d) outside %d primitives", i, n.start,
                               n.count, prim_count);
            a = n.start;
            b = ~n.count;
        } else {
            // children after their parent: the walk from node 0 ends
            if ((n.left != -1 && (n.left <= i || n.left >= node_count)) || (n.right != -1 && (n.right <= i || n.right >= node_count)))
                return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_bvh: node %d's children %d, %d (need -1 or %d..%d)", i, n.left,
                               n.right, i + 1, node_count - 1);
            a = n.left;
            b = n.right;
        }
        rec[2 * i + 0] = make_float4(n.bmin.x, n.bmin.y, n.bmin.z, rt_bits(a));
        rec[2 * i + 1] = make_float4(n.bmax.x, n.bmax.y, n.bmax.z, rt_bits(b));
    }
    int max_prim = -1;
    for (int i = 0; i < prim_count; ++i) {
        if (prims[i] < 0)
            return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_upload_bvh: primitive %d is face %d", i, prims[i]);
        max_prim = std::max(max_prim, (int)prims[i]);
    }
    RT_TRY(c, hipSetDevice(c->device));
    RT_TRY(c, hipStreamSynchronize(c->stream));
    ptrt_rt_ctx::Slot &s = c->slots[index];
    dfree(s.nodes);
    dfree(s.prims);
    s.node_count = 0;
    s.max_prim = -1;
    if (node_count > 0) {
        RT_TRY(c, hipMalloc((void **)&s.nodes, rec.size() * sizeof(float4)));
        RT_TRY(c, hipMemcpy(s.nodes, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    if (prim_count > 0) {
        RT_TRY(c, hipMalloc((void **)&s.prims, (size_t)prim_count * sizeof(int)));
        RT_TRY(c, hipMemcpy(s.prims, prims, (size_t)prim_count * sizeof(int), hipMemcpyHostToDevice));
    }
    s.node_count = node_count;
    s.max_prim = max_prim;
    return PTRT_OK;
}

int ptrt_rt_set_scene(ptrt_rt_ctx *c, const ptrt_rt_mesh *meshes, int mesh_count, const ptrt_rt_light *lights, int light_count) {
    if (!rt_live(c))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_set_scene: bad context");
    if (mesh_count < 0 || mesh_count > (int)c->slots.size() || (mesh_count > 0 && !meshes) || light_count < 0 ||
        (light_count > 0 && !lights))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_set_scene: %d meshes (%d uploaded), %d lights", mesh_count,
                       (int)c->slots.size(), light_count);
    c->meshes.assign(meshes, meshes + mesh_count);
    c->lights.assign(lights, lights + light_count);
    c->have_scene = true;
    return PTRT_OK;
}

int ptrt_rt_render(ptrt_rt_ctx *c, const ptrt_rt_view *view, void *out_rgb8, int out_is_device) {
    if (!rt_live(c))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_render: bad context");
    if (!view || !out_rgb8 || (out_is_device != PTRT_OUT_HOST && out_is_device != PTRT_OUT_DEVICE))
        return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_render: needs a view and a target (out_rgb8 %p, out_is_device %d)", out_rgb8,
                       out_is_device);
    if (!c->have_scene)
        return rt_fail(c, PTRT_E_NOT_READY, "ptrt_rt_render: no scene (ptrt_rt_set_scene)");
    const int n = (int)c->meshes.size(), nl = (int)c->lights.size();
    std::vector<rt::MeshDev> desc(n);
    for (int i = 0; i < n; ++i) {
        const ptrt_rt_ctx::Slot &s = c->slots[i];
        const ptrt_rt_mesh &m = c->meshes[i];
        const bool has_tree = s.node_count > 0 && s.faces > 0;
        if (has_tree && s.max_prim >= s.faces)
            return rt_fail(c, PTRT_E_INVALID, "ptrt_rt_render: mesh %d's tree names face %d of %d (upload a tree built for these faces)",
                           i, s.max_prim, s.faces);
        rt::MeshDev &d = desc[i];
        d.tris = s.tris;
        d.nodes = s.nodes;
        d.prims = s.prims;
        d.face_count = has_tree ? s.faces : 0;
        d.node_count = has_tree ? s.node_count : 0;
        d.translation[0] = m.translation.x;
        d.translation[1] = m.translation.y;
        d.translation[2] = m.translation.z;
        std::memcpy(d.rot, m.rotation, sizeof d.rot);
        std::memcpy(d.inv, m.inv_rotation, sizeof d.inv);
        std::memcpy(&d.mat, &m.material, sizeof d.mat);
    }
    RT_TRY(c, hipSetDevice(c->device));
    RT_TRY(c, hipStreamSynchronize(c->stream));
    if (n > c->desc_cap) {
        dfree(c->d_desc);
        RT_TRY(c, hipMalloc((void **)&c->d_desc, (size_t)n * sizeof(rt::MeshDev)));
        c->desc_cap = n;
    }
    if (nl > c->light_cap) {
        dfree(c->d_lights);
        RT_TRY(c, hipMalloc((void **)&c->d_lights, (size_t)nl * sizeof(rt::LightDev)));
        c->light_cap = nl;
    }
    if (n)
        RT_TRY(c, hipMemcpy(c->d_desc, desc.data(), (size_t)n * sizeof(rt::MeshDev), hipMemcpyHostToDevice));
    if (nl)
        RT_TRY(c, hipMemcpy(c->d_lights, c->lights.data(), (size_t)nl * sizeof(rt::LightDev), hipMemcpyHostToDevice));
    const size_t bytes = (size_t)c->W * c->H * 3;
    if (out_is_device == PTRT_OUT_HOST && !c->d_out)
        RT_TRY(c, hipMalloc((void **)&c->d_out, bytes));
    auto v3 = [](ptrt_vec3 v) { return pt::f3{v.x, v.y, v.z}; };
    rt::Params P{};
    P.meshes = c->d_desc;
    P.lights = c->d_lights;
    P.n_meshes = n;
    P.n_lights = nl;
    P.cam_origin = v3(view->origin);
    P.cam_cmo = v3(view->corner_minus_origin);
    P.cam_horizontal = v3(view->horizontal);
    P.cam_vertical = v3(view->vertical);
    P.ambient = v3(view->ambient);
    P.sky_top = v3(view->sky_top);
    P.sky_bottom = v3(view->sky_bottom);
    P.use_sky = view->use_sky ? 1 : 0;
    P.out = out_is_device ? (unsigned char *)out_rgb8 : c->d_out;
    P.width = c->W;
    P.height = c->H;
    const dim3 grid((c->W + 7) / 8, (c->H + 7) / 8);
    hipLaunchKernelGGL(rt::rt_render_kernel, grid, dim3(64), 0, c->stream, P);
    RT_TRY(c, hipGetLastError());
    if (!out_is_device)
        RT_TRY(c, hipMemcpyAsync(out_rgb8, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    RT_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

} // extern "C"
