// ptrt_accel_state.hip.h -- the state that only the acceleration-structure entry points (ptrt_accel.hip.h) touch: the two
// staging areas and the BVH builder's scratch.  Included by ptrt_capi.hip ahead of struct ptrt_ctx, which embeds one of each
// (as it embeds a FrameRing); the code that uses them needs the complete context and follows in ptrt_accel.hip.h.
// release() is for a context that is going away: a geometry re-upload keeps the staging areas.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

// Staged instance transforms (ptrt_set_instance_transforms): two halves of pinned host / device memory, each waited for when
// it comes round again.
struct XformStage {
    float *h_xf = nullptr, *d_xf = nullptr;
    size_t cap = 0, used[2] = {0, 0}; // records per half / handed out of each
    int cur = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};

    void release() {
        if (h_xf)
            (void)hipHostFree(h_xf);
        if (d_xf)
            (void)hipFree(d_xf);
        for (hipEvent_t e : ev)
            if (e)
                (void)hipEventDestroy(e);
        *this = XformStage{};
    }
};

// Staged vertex positions (ptrt_update_vertices), STAGES buffers in rotation.
struct VertexStage {
    static constexpr int STAGES = 4;
    void *h_stage[STAGES] = {nullptr, nullptr, nullptr, nullptr}; // from host memory: pinned staging
    size_t stage_bytes[STAGES] = {0, 0, 0, 0};
    hipEvent_t stage_ev[STAGES] = {nullptr, nullptr, nullptr, nullptr};
    unsigned long long stage_n = 0;
    float *d_stage[STAGES] = {nullptr, nullptr, nullptr, nullptr}; // from PINNED host memory: device staging behind a copy stream
    size_t d_stage_bytes[STAGES] = {0, 0, 0, 0};
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_ev = nullptr;

    void release() {
        for (int k = 0; k < STAGES; ++k) {
            if (h_stage[k])
                (void)hipHostFree(h_stage[k]);
            if (stage_ev[k])
                (void)hipEventDestroy(stage_ev[k]);
            if (d_stage[k])
                (void)hipFree(d_stage[k]);
        }
        if (copy_stream)
            (void)hipStreamDestroy(copy_stream);
        if (copy_ev)
            (void)hipEventDestroy(copy_ev);
        *this = VertexStage{};
    }
};

// Scratch of the GPU rebuild (ptrt_build_bvh, pt_build.hip.h), sized for the largest mesh rebuilt so far.
struct BuildScratch {
    uint32_t *d_sort_keys[2] = {nullptr, nullptr}, *d_sort_vals[2] = {nullptr, nullptr}, *d_sort_hist = nullptr,
             *d_cbounds = nullptr;
    float *d_centroids = nullptr;
    int sort_capacity = 0;

    void release() {
        for (void *p : {(void *)d_sort_keys[0], (void *)d_sort_keys[1], (void *)d_sort_vals[0], (void *)d_sort_vals[1],
                        (void *)d_sort_hist, (void *)d_cbounds, (void *)d_centroids})
            if (p)
                (void)hipFree(p);
        *this = BuildScratch{};
    }
};

} // namespace
