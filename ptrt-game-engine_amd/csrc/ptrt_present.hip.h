// ptrt_present.hip.h -- presentation: RGB8 frames on the device mirrored into pinned host memory (FrameRing,
// ptrt_frame_ring.hip.h), as the context's own ring (ptrt_present_*) and as a ring without a context (ptrt_ring_*).  The two
// differ in who records a slot's `rendered` event: the context always does, on its stream; the free-standing ring only when
// no render call marked the slot.  Included by ptrt_capi.hip.
#pragma once

// Presentation ring without a context (ptrt_ring_*): the CUDA-registered GL pixel-buffer object of
// rtgl::init_interop_viewer as `slots` device frames mirrored into pinned host memory.
struct ptrt_ring {
    int device = 0;
    FrameRing ring;
    std::vector<char> marked; // per slot: `rendered` was recorded by the render call that wrote the slot
};

namespace {

std::mutex g_ring_mutex;
std::set<ptrt_ring *> g_rings;

// ptrt_render / ptrt_post_frame wrote their RGB8 frame to `out` on `stream`: if that is a ring slot, the slot's
// download must wait for exactly this point of the stream.
void ring_mark_rendered(const void *out, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    for (ptrt_ring *r : g_rings)
        for (size_t i = 0; i < r->ring.slots.size(); ++i)
            if (r->ring.slots[i].dev == out) {
                r->marked[i] = hipEventRecord(r->ring.slots[i].rendered, stream) == hipSuccess;
                return;
            }
}

bool ring_live(ptrt_ring *r) {
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    return r && g_rings.count(r);
}
void ring_free(ptrt_ring *r) {
    (void)hipSetDevice(r->device);
    r->ring.free();
    delete r;
}

} // namespace

extern "C" {

int ptrt_present_destroy(ptrt_ctx *c) {
    if (!ctx_live(c))
        return fail(c, PTRT_E_INVALID, "ptrt_present_destroy: bad context");
    if (c->present.slots.empty())
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    (void)hipStreamSynchronize(c->stream);
    c->present.free();
    return PTRT_OK;
}

int ptrt_present_create(ptrt_ctx *c, int slots) {
    if (!ctx_live(c) || slots < 1 || slots > 8)
        return fail(c, PTRT_E_INVALID, "ptrt_present_create: 1..8 slots");
    if (int rc = ptrt_present_destroy(c))
        return rc;
    HIP_TRY(c, c->present.create(c->npix * 3, slots));
    return PTRT_OK;
}

int ptrt_present_map(ptrt_ctx *c, int slot, void **device_pixels) {
    if (!ctx_live(c) || !device_pixels || !c->present.has(slot))
        return fail(c, PTRT_E_INVALID, "ptrt_present_map: no such slot (ptrt_present_create first)");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, c->present.map(slot, device_pixels));
    return PTRT_OK;
}

int ptrt_present_unmap(ptrt_ctx *c, int slot) {
    if (!ctx_live(c) || !c->present.has(slot))
        return fail(c, PTRT_E_INVALID, "ptrt_present_unmap: no such slot");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, c->present.unmap(slot, true, c->stream));
    return PTRT_OK;
}

int ptrt_present_acquire(ptrt_ctx *c, int slot, const unsigned char **host_pixels) {
    if (!ctx_live(c) || !host_pixels || !c->present.has(slot))
        return fail(c, PTRT_E_INVALID, "ptrt_present_acquire: no such slot");
    if (int rc = set_device(c))
        return rc;
    HIP_TRY(c, c->present.acquire(slot, host_pixels));
    return PTRT_OK;
}

int ptrt_ring_create(int device, size_t frame_bytes, int slots, ptrt_ring **out) {
    if (!out)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_ring_create: out is NULL");
    *out = nullptr;
    if (frame_bytes == 0 || slots < 1 || slots > 8)
        return fail(nullptr, PTRT_E_INVALID, "ptrt_ring_create: %zu bytes, %d slots (1..8)", frame_bytes, slots);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, PTRT_E_NO_DEVICE, "no HIP device available; this library has no CPU path");
    if (device < 0 || device >= ndev)
        return fail(nullptr, PTRT_E_NO_DEVICE, "device %d out of range (have %d)", device, ndev);
    ptrt_ring *r = new ptrt_ring;
    r->device = device;
    r->marked.assign((size_t)slots, 0);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
        e = r->ring.create(frame_bytes, slots);
    if (e != hipSuccess) {
        ring_free(r);
        return fail(nullptr, PTRT_E_HIP, "ptrt_ring_create: %s", hipGetErrorString(e));
    }
    {
        std::lock_guard<std::mutex> lock(g_ring_mutex);
        g_rings.insert(r);
    }
    *out = r;
    return PTRT_OK;
}

int ptrt_ring_map(ptrt_ring *r, int slot, void **device_pixels) {
    if (!ring_live(r) || !device_pixels || !r->ring.has(slot))
        return fail(nullptr, PTRT_E_INVALID, "ptrt_ring_map: bad ring or slot");
    HIP_TRY(nullptr, hipSetDevice(r->device));
    HIP_TRY(nullptr, r->ring.map(slot, device_pixels));
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    r->marked[(size_t)slot] = 0;
    return PTRT_OK;
}

int ptrt_ring_unmap(ptrt_ring *r, int slot) {
    if (!ring_live(r) || !r->ring.has(slot))
        return fail(nullptr, PTRT_E_INVALID, "ptrt_ring_unmap: bad ring or slot");
    HIP_TRY(nullptr, hipSetDevice(r->device));
    bool marked;
    {
        std::lock_guard<std::mutex> lock(g_ring_mutex);
        marked = r->marked[(size_t)slot] != 0;
    }
    // a slot not written through ptrt_render: behind everything already submitted to the device's blocking
    // streams, which is what cudaGraphicsUnmapResources guarantees the GL side
    HIP_TRY(nullptr, r->ring.unmap(slot, !marked, nullptr));
    return PTRT_OK;
}

int ptrt_ring_acquire(ptrt_ring *r, int slot, const unsigned char **host_pixels) {
    if (!ring_live(r) || !host_pixels || !r->ring.has(slot))
        return fail(nullptr, PTRT_E_INVALID, "ptrt_ring_acquire: bad ring or slot");
    HIP_TRY(nullptr, hipSetDevice(r->device));
    HIP_TRY(nullptr, r->ring.acquire(slot, host_pixels));
    return PTRT_OK;
}

void ptrt_ring_destroy(ptrt_ring *r) {
    {
        std::lock_guard<std::mutex> lock(g_ring_mutex);
        if (!r || !g_rings.count(r))
            return;
        g_rings.erase(r);
    }
    ring_free(r);
}

} // extern "C"
