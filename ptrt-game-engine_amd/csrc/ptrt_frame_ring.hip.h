// ptrt_frame_ring.hip.h -- FrameRing: frames in device memory mirrored into pinned host memory, the one mechanism behind
// the context's presentation ring (ptrt_present_*) and the ring without a context (ptrt_ring_*); ptrt_present.hip.h holds
// both surfaces.  Included by ptrt_capi.hip ahead of struct ptrt_ctx: a context embeds one.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace {

// A slot is written on the device (map), then downloaded on the ring's own copy stream behind the point where its frame was
// rendered (unmap) -- so the download overlaps the NEXT frame's kernels; a copy enqueued on the render stream would only be
// asynchronous to the host -- and read on the host once the download has arrived (acquire).  The calls return the HIP
// error of their first failing step; the caller selects the device.
struct FrameRing {
    struct Slot {
        unsigned char *dev = nullptr, *host = nullptr;
        hipEvent_t rendered = nullptr, done = nullptr;
        bool in_flight = false; // a download of this slot has been enqueued and not yet waited for
    };
    std::vector<Slot> slots;
    hipStream_t copy_stream = nullptr;
    size_t bytes = 0; // of one frame

    bool has(int slot) const { return slot >= 0 && slot < (int)slots.size(); }

    // all `n` slots or none: a failure part-way frees what was made
    hipError_t create(size_t frame_bytes, int n) {
        bytes = frame_bytes;
        slots.resize((size_t)n);
        hipError_t e = hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking);
        for (auto &s : slots) {
            if (e == hipSuccess)
                e = hipMalloc((void **)&s.dev, bytes);
            if (e == hipSuccess)
                e = hipHostMalloc((void **)&s.host, bytes, hipHostMallocDefault);
            if (e == hipSuccess)
                e = hipEventCreateWithFlags(&s.rendered, hipEventDisableTiming);
            if (e == hipSuccess)
                e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        }
        if (e != hipSuccess)
            free();
        return e;
    }

    hipError_t wait(Slot &s) {
        if (s.in_flight) {
            if (hipError_t e = hipEventSynchronize(s.done))
                return e;
            s.in_flight = false;
        }
        return hipSuccess;
    }

    // the frame about to be overwritten must have reached the host
    hipError_t map(int slot, void **device_pixels) {
        Slot &s = slots[(size_t)slot];
        if (hipError_t e = wait(s))
            return e;
        *device_pixels = s.dev;
        return hipSuccess;
    }

    // `record`: the end of the slot's frame is the present head of `stream`; false when `rendered` has been recorded already
    hipError_t unmap(int slot, bool record, hipStream_t stream) {
        Slot &s = slots[(size_t)slot];
        hipError_t e = record ? hipEventRecord(s.rendered, stream) : hipSuccess;
        if (e == hipSuccess)
            e = hipStreamWaitEvent(copy_stream, s.rendered, 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync(s.host, s.dev, bytes, hipMemcpyDeviceToHost, copy_stream);
        if (e == hipSuccess)
            e = hipEventRecord(s.done, copy_stream);
        if (e == hipSuccess)
            s.in_flight = true;
        return e;
    }

    hipError_t acquire(int slot, const unsigned char **host_pixels) {
        Slot &s = slots[(size_t)slot];
        if (hipError_t e = wait(s))
            return e;
        *host_pixels = s.host;
        return hipSuccess;
    }

    void free() {
        if (copy_stream) {
            (void)hipStreamSynchronize(copy_stream);
            (void)hipStreamDestroy(copy_stream);
            copy_stream = nullptr;
        }
        for (auto &s : slots) {
            if (s.dev)
                (void)hipFree(s.dev);
            if (s.host)
                (void)hipHostFree(s.host);
            if (s.rendered)
                (void)hipEventDestroy(s.rendered);
            if (s.done)
                (void)hipEventDestroy(s.done);
        }
        slots.clear();
    }
};

} // namespace
