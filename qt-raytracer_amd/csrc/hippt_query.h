// hippt_query.h — launch interface of the batched ray queries (hippt_query.hip): closest hit,
// occlusion and camera first-hit buffers over the uploaded scene (include/hippt.h hipptTraceRays,
// hipptOccluded, hipptTraceCamera).
#pragma once

#include <type_traits>

#include "hippt_device.h"

namespace hippt {

// The camera sample's arguments (trace::camera_sample's PP): the whole image as one band, item =
// pixel index y * width + x, one frame.
struct QueryCam {
    CameraF cam;
    float invW, invH;  // 1/max(1,W-1), 1/max(1,H-1), as MeshParams
    int width, y0, rowStride, firstFrame;
    unsigned bandPixels;  // width * height
    float rcpBandPixels, rcpWidth;
};

// The rays of a launch are split into kQueryShards contiguous shards of whole waves' worth, each with
// its own claim counter on its own 128-byte line (counter[k * kQueryCtrStride]): claims on one word
// serialise (~11 ns each, MI355X_MICROARCH.md "dequeue"), which alone bound a 2^24-ray launch over one
// counter at 19 G rays/s whatever the rays (DESIGN_LOG.md §A.Q).  A block starts on shard blockIdx % 8
// (its XCD's) and moves on to the others once it is drained.
constexpr unsigned kQueryShards = 8, kQueryCtrStride = 32;
constexpr size_t kQueryCtrBytes = size_t(kQueryShards) * kQueryCtrStride * sizeof(unsigned);

// One launch traces rays [0, numRays) of `rays` (or, camera: pixels firstItem .. firstItem + numRays
// - 1 of the image) and writes result i to t[i], prim[i], occluded[i] (each may be null), or, a
// hit-record launch, to hits[2 i], hits[2 i + 1] alone.  Every pointer is device memory of the launch's device.
struct QueryParams {
    const float4 *nodes;  // float nodes: the 2-wide tree or the 4-wide one (Bvh4 layout)
    const float4 *tris;   // MeshParams::tris
    const float4 *rays;   // 2 float4 per ray: (origin, tmin) (direction, tmax); camera: unused
    float *t;
    int *prim;
    unsigned char *occluded;
    unsigned *counter;  // the launch's kQueryShards claim counters (zeroed before it)
    int *spill;         // 4-wide traversal: per-lane stack spill area (MeshParams::spill)
    unsigned numRays, firstItem, chunk;  // chunk: rays per claim (a multiple of 64)
    int stackDepth, numNodes, numTris;
    int ldsScene, full, wide;  // wide: 0 the 2-wide tree, 1 the 4-wide float nodes
    int stackCap, spillCap;
    unsigned topBytes, leafExit, nodeExit;
    int waveThreshold;
    QueryCam cam;
    // hit records (last, so that the other modes' kernel arguments stay where they were)
    const float4 *shade;  // MeshParams::shade
    float4 *hits;         // 2 float4 per ray (hipptHit)
    const float *pad;     // the pad word of the scene's boxes (the upload's, rewritten by a refit): M * 2^-16
};

// What a launch of the query kernel computes per ray.
enum class QueryMode {
    Closest,     // t[i], prim[i] of the closest hit
    Any,         // occluded[i]: the traversal of a ray ends at its first accepted hit
    Camera,      // Closest over rays generated in the kernel
    Hits,        // hits[2 i], hits[2 i + 1]: the closest hit's record
    CameraHits,  // Hits over rays generated in the kernel
};
constexpr bool query_camera(QueryMode m) { return m == QueryMode::Camera || m == QueryMode::CameraHits; }
constexpr bool query_hits(QueryMode m) { return m == QueryMode::Hits || m == QueryMode::CameraHits; }

// The launch's contract with a ray-per-lane kernel (query_kernel, path_kernel), as far as every such
// kernel shares it: what it dereferences is there, the LDS top is whole nodes of the array, claims are
// whole waves.
inline bool query_params_ok(const QueryParams &q, int blocks) {
    if (!q.nodes || !q.tris || !q.counter || !q.pad || blocks <= 0 || q.numRays == 0 || q.chunk < 64 || q.chunk % 64 ||
        q.numRays > (1u << 31) || (q.wide != 0 && q.wide != 1))
        return false;
    if (q.wide && (q.stackCap < 1 || !q.spill)) return false;
    return !q.topBytes ||
           (!q.ldsScene && q.wide && q.topBytes % 128u == 0 && q.topBytes <= (unsigned(q.numNodes) << 7));
}

// The kernel variant of q's scene layout: f(ldsScene, full, wide), each a std::bool_constant.
template <class F>
auto for_scene_layout(const QueryParams &q, F f) {
    using Y = std::true_type;
    using N = std::false_type;
    switch ((q.ldsScene ? 4 : 0) | (q.full ? 2 : 0) | (q.wide ? 1 : 0)) {
    case 0: return f(N{}, N{}, N{});
    case 1: return f(N{}, N{}, Y{});
    case 2: return f(N{}, Y{}, N{});
    case 3: return f(N{}, Y{}, Y{});
    case 4: return f(Y{}, N{}, N{});
    case 5: return f(Y{}, N{}, Y{});
    case 6: return f(Y{}, Y{}, N{});
    default: return f(Y{}, Y{}, Y{});
    }
}

hipError_t launch_query(const QueryParams &q, int blocks, QueryMode mode, hipStream_t s);
size_t query_lds_bytes(const QueryParams &q);
int query_blocks_per_cu(const QueryParams &q, QueryMode mode);

}  // namespace hippt
