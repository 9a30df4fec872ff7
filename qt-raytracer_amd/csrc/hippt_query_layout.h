// hippt_query_layout.h — the caller's buffers of a ray or path query as one table, and the layout of the
// staging buffer a host-memory query copies them through.  No HIP, no global state: the product
// (hippt_api.cpp) and a host-compiled driver (tests/native/query_layout_check.cpp) call the same code.
//
// A query call names up to kMaxBuffers per-ray buffers (include/hippt.h hipptTraceRays, hipptOccluded,
// hipptTraceCamera, hipptTraceHits, hipptTraceCameraHits, hipptTraceRadiance, hipptCameraRays).  What is
// done per buffer — the device-pointer check, the advance to a launch's first ray, the place in the
// staging buffer, the copy in before a launch or out after it — walks the table.
#pragma once

#include <cstddef>

namespace hippt {
namespace qlayout {

// Where a buffer's device pointer goes in a launch's parameters (hippt_query.h QueryParams, hippt_path.h
// PathParams, CameraRaysParams).  The order is that of the device-pointer check.
enum class Slot { Rays, T, Prim, Occluded, Hits, Seeds, Radiance, Segments, OutRays, OutSeeds };

struct Buffer {
    const void *ptr;      // the caller's pointer (null: the buffer is not part of this call)
    size_t bytesPerRay;
    size_t align;         // what a device pointer of the caller's must be a multiple of
    bool out;             // a result (copied back after a launch), else an input (copied in before it)
    Slot slot;
};

constexpr int kMaxBuffers = 4;

struct Table {
    Buffer b[kMaxBuffers];
    int n = 0;

    // Adds the caller's buffer for `slot` (ptr may be null).  At most kMaxBuffers per call.
    void add(Slot slot, const void *ptr) {
        // bytes per ray, alignment, direction, by Slot
        static constexpr struct {
            size_t bytes, align;
            bool out;
        } kInfo[] = {{32, 16, false}, {4, 4, true},  {4, 4, true},  {1, 1, true},   {32, 32, true},
                     {4, 4, false},   {16, 16, true}, {4, 4, true}, {32, 16, true}, {4, 4, true}};
        if (n == kMaxBuffers) return;
        b[n++] = Buffer{ptr, kInfo[int(slot)].bytes, kInfo[int(slot)].align, kInfo[int(slot)].out, slot};
    }
    const void *ptr(Slot slot) const {
        for (int k = 0; k < n; ++k)
            if (b[k].slot == slot) return b[k].ptr;
        return nullptr;
    }
    bool any_out() const {
        for (int k = 0; k < n; ++k)
            if (b[k].out && b[k].ptr) return true;
        return false;
    }
};

// The staging buffer of slices of up to `cap` rays: buffer k of the table (if the call has it) at
// [off[k], off[k] + cap * bytesPerRay), in the table's order, every offset a multiple of 16 (the
// kernels load rays and store records 16 bytes at a time); `total` bytes in all.
struct Staging {
    size_t off[kMaxBuffers] = {};
    size_t total = 0;
};

inline Staging staging(const Table &t, size_t cap) {
    Staging s;
    for (int k = 0; k < t.n; ++k) {
        if (!t.b[k].ptr) continue;
        s.off[k] = (s.total + 15) & ~size_t(15);
        s.total = s.off[k] + cap * t.b[k].bytesPerRay;
    }
    return s;
}

}  // namespace qlayout
}  // namespace hippt
