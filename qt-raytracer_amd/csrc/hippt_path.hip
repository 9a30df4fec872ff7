// hippt_path.hip — path queries over the uploaded scene: the renderer's path from a
// caller-supplied ray and RNG state (include/hippt.h hipptTraceRadiance), and the rays and RNG states
// the renderer's own camera starts a sample with (hipptCameraRays).  DESIGN.md §14.
//
// path_kernel has the query kernel's outer shape (hippt_query.hip): a persistent grid of 256-thread
// blocks, a ray per lane, runs of consecutive ray indices claimed from the shard counters
// (hippt_query.h kQueryShards) and handed to the requesting lanes by ballot, the LDS scene copy or the
// LDS top of a global tree, the per-lane LDS stack with its spill area.  A lane keeps its path until
// the path ends: a traversal that finishes on a hit within the depth limit scatters (the renderer's
// scatter, hippt_trace.h) and the lane goes on traversing the scattered ray with the renderer's tmin
// 0.001 and no tmax; only a finished path (sky, a light, depth limit, absorbed, invalid ray) stores its result
// and asks for a new ray.  Segment 0 alone uses the ray's own tmin and exclusive tmax, started as the
// query kernel starts a ray.
//
// Shading is batched by the wave threshold, as in the render megakernel: a wave leaves the traversal
// loop once at most Q.waveThreshold lanes are still traversing, and all lanes whose traversal has
// finished shade together.  scatter's unit-sphere draw is the plain per-lane loop (TAIL = -1, as the
// wavefront shade kernel): it is called under per-lane control flow (hit, depth, material).
#include "hippt_path.h"

#include "hippt_ray_loop.h"

namespace hippt {
namespace {
using namespace rayloop;

// LDS_SCENE: the scene copy in LDS (else the tree in global memory, the top of a 4-wide one in LDS);
// FULL: spheres or materials other than Lambertian present; WIDE: the 4-wide tree.
template <bool LDS_SCENE, bool FULL, bool WIDE>
__global__ __launch_bounds__(kMeshBlock) void path_kernel(PathParams P) {
    const QueryParams &Q = P.q;
    const Staged sc = stage_scene<LDS_SCENE, WIDE>(Q.nodes, Q.tris, Q.numNodes, Q.numTris, Q.stackDepth, Q.topBytes);
    const SpillArea S = lane_spill(Q.spill, Q.spillCap, Q.stackCap);
    // shard k: rays [k * per, (k + 1) * per) below numRays, `per` a multiple of 64 (whole lines)
    const unsigned per = ((Q.numRays + kQueryShards * 64u - 1u) / (kQueryShards * 64u)) * 64u;
    unsigned fs = blockIdx.x % kQueryShards, left = kQueryShards;  // the wave's shard; shards not yet found drained
    unsigned fsBase = min(fs * per, Q.numRays), fsCount = min((fs + 1u) * per, Q.numRays) - fsBase;
    unsigned poolNext = 0, poolEnd = 0;
    unsigned idx = kNone;  // this lane's ray
    bool need = true;
    QueryRay r{};
    float tmin = 0.0f;
    const float M = scene_M(Q.pad);
    // the path's state: RNG, throughput, segments traced so far that hit (-1: an invalid ray), and
    // whether segment 0 hit
    uint32_t rng = 0;
    float tr = 1.0f, tg = 1.0f, tb = 1.0f;
    int depth = 0;
    bool hit0 = false;
    Trav T;
    begin(T);
    T.cur = kDone;
    unsigned long long nvis = 0, ntest = 0;
    unsigned pc[kProfSlots] = {};  // phase profile slots (not reported by the queries)
    for (;;) {
        while (left && __ballot(need)) {
            const unsigned qi =
                wave_fetch(need, poolNext, poolEnd, &Q.counter[fs * kQueryCtrStride], Q.chunk, fsCount);
            if (need && qi != kNone) {  // a new path: segment 0 starts as a ray query's ray
                need = false;
                idx = fsBase + qi;
                float tmax;
                rng = P.seeds[idx];  // (before the ray: the three loads are in flight together)
                const bool valid = load_query_ray(Q.rays, idx, r, tmin, tmax);
                tr = tg = tb = 1.0f;
                depth = 0;
                hit0 = false;
                // begin_query_ray, with the mark of hipptTraceRays' invalid rays (no segment, (0, 0, 0, 0))
                // in its branch: set after it, the mark costs path_kernel<false, false, false> 2 VGPRs
                begin(T);
                T.bestO = -1;  // a hit at exactly t == tmax loses the tie on the id: tmax is exclusive
                if (valid) {
                    prepare_query<FULL, WIDE>(r, M);  // segment 0 may start anywhere
                    T.bestT = tmax;
                } else {
                    T.cur = kDone;
                    depth = -1;
                }
            }
            if (__ballot(need)) {  // a requesting lane got none: this shard is drained
                fs = fs + 1 == kQueryShards ? 0u : fs + 1;
                fsBase = min(fs * per, Q.numRays);
                fsCount = min((fs + 1u) * per, Q.numRays) - fsBase;
                poolNext = poolEnd = 0;
                --left;
            }
        }
        need = false;
        if (!__any(idx != kNone)) break;
        if (__any(busy(T))) {
            do {
                traverse_step<LDS_SCENE, FULL, WIDE>(T, r, tmin, sc, Q, S, nvis, ntest, pc);
            } while (__popcll(__ballot(busy(T))) > unsigned(Q.waveThreshold));
        }
        if (idx != kNone && !busy(T)) {  // the segment's traversal is finished: po_mesh_sample's loop body
            float L0 = 0.0f, L1 = 0.0f, L2 = 0.0f;
            int segs = 0;
            bool finished = true;
            if (depth < 0) {
                // invalid ray
            } else if (T.bestI < 0) {  // miss: the sky of the segment's direction
                sky(r, tr, tg, tb, L0, L1, L2);
                segs = depth + 1;
            } else {
                hit0 = true;
                segs = ++depth;
                if (FULL && emitted(T.bestI, Q.shade, P.mats, tr, tg, tb, L0, L1, L2)) {
                    // ends at a light with throughput x emission, whatever the depth
                } else if (depth < P.maxDepth &&  // depth exhausted or absorbed: contributes 0
                    scatter<FULL, false, -1>(r, T.bestT, T.bestI, Q.shade, sc.tris, P.mats, rng, tr, tg, tb, pc)) {
                    finished = false;
                    prepare_segment(r);  // on a surface of the scene: the renderer's test
                    begin(T);
                    tmin = 0.001f;
                }
            }
            if (finished) {
                P.radiance[idx] = float4{L0, L1, L2, hit0 ? 1.0f : 0.0f};
                if (P.segments) P.segments[idx] = segs;
                idx = kNone;
                need = true;
            }
        }
    }
}

using PathFn = void (*)(PathParams);
PathFn path_fn(const QueryParams &q) {
    return for_scene_layout(q, [](auto lds, auto full, auto wide) -> PathFn { return path_kernel<lds(), full(), wide()>; });
}

constexpr int kCameraRaysBlock = 256;
__global__ __launch_bounds__(kCameraRaysBlock) void camera_rays_kernel(CameraRaysParams P) {
    const unsigned i = blockIdx.x * unsigned(kCameraRaysBlock) + threadIdx.x;
    if (i >= P.numRays) return;
    Ray r{};
    uint32_t rng;
    camera_sample(P.cam, P.firstItem + i, r, rng);
    if (P.rays) {
        P.rays[2 * size_t(i)] = float4{r.ox, r.oy, r.oz, 0.001f};
        P.rays[2 * size_t(i) + 1] = float4{r.dx, r.dy, r.dz, INFINITY};
    }
    if (P.seeds) P.seeds[i] = rng;
}

}  // namespace

hipError_t launch_path(const PathParams &p, int blocks, hipStream_t s) {
    const QueryParams &q = p.q;
    if (!query_params_ok(q, blocks)) return hipErrorInvalidValue;
    // the path's own pointers; rays and records are read and stored whole
    if (!q.shade || !q.rays || !p.mats || !p.seeds || !p.radiance || p.maxDepth < 1 ||
        reinterpret_cast<uintptr_t>(q.rays) % 16 || reinterpret_cast<uintptr_t>(p.radiance) % 16)
        return hipErrorInvalidValue;
    return launch_ray_kernel(path_fn(q), q, p, blocks, s);
}

int path_blocks_per_cu(const PathParams &p) { return ray_kernel_blocks_per_cu(path_fn(p.q), p.q); }

hipError_t launch_camera_rays(const CameraRaysParams &p, hipStream_t s) {
    if ((!p.rays && !p.seeds) || p.numRays == 0 || p.numRays > (1u << 31) || reinterpret_cast<uintptr_t>(p.rays) % 16)
        return hipErrorInvalidValue;
    const unsigned blocks = (p.numRays + unsigned(kCameraRaysBlock) - 1u) / unsigned(kCameraRaysBlock);
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(kCameraRaysBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace hippt
