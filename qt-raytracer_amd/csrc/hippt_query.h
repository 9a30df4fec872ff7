// hippt_query.h — launch interface of the batched ray queries (hippt_query.hip): closest hit,
// occlusion and camera first-hit buffers over the uploaded scene (include/hippt.h hipptTraceRays,
// hipptOccluded, hipptTraceCamera).
#pragma once

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
};

// any: occlusion (the traversal of a ray ends at its first accepted hit); camera: rays generated in
// the kernel; hits: hit records (not with any).
hipError_t launch_query(const QueryParams &q, int blocks, bool any, bool camera, bool hits, hipStream_t s);
size_t query_lds_bytes(const QueryParams &q);
int query_blocks_per_cu(const QueryParams &q, bool any, bool camera, bool hits);

}  // namespace hippt
