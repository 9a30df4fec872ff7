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
// 0.001 and no tmax; only a finished path (sky, depth limit, absorbed, invalid ray) stores its result
// and asks for a new ray.  Segment 0 alone uses the ray's own tmin and exclusive tmax, started as the
// query kernel starts a ray.
//
// Shading is batched by the wave threshold, as in the render megakernel: a wave leaves the traversal
// loop once at most Q.waveThreshold lanes are still traversing, and all lanes whose traversal has
// finished shade together.  scatter's unit-sphere draw is the plain per-lane loop (TAIL = -1, as the
// wavefront shade kernel): it is called under per-lane control flow (hit, depth, material).
#include "hippt_path.h"

#include <algorithm>

#include "hippt_trace.h"

namespace hippt {
namespace {
using namespace trace;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// LDS_SCENE: the scene copy in LDS (else the tree in global memory, the top of a 4-wide one in LDS);
// FULL: spheres or materials other than Lambertian present; WIDE: the 4-wide tree.
template <bool LDS_SCENE, bool FULL, bool WIDE>
__global__ __launch_bounds__(kMeshBlock) void path_kernel(PathParams P) {
    const QueryParams &Q = P.q;
    extern __shared__ int lds[];  // LDS scene: nodes at address 0, then stack, primitives
    constexpr int ldsNodeF4 = WIDE ? kLdsNode4F4 : kLdsNodeF4;  // mesh_lds_bytes layout
    constexpr bool TOP = WIDE && !LDS_SCENE;
    int *const stk = LDS_SCENE ? lds + Q.numNodes * ldsNodeF4 * 4 : lds + (TOP ? (Q.topBytes >> 2) : 0u);
    int *const my = stk + threadIdx.x;
    const float4 *nodes = Q.nodes, *tris = Q.tris;
    if (LDS_SCENE) {
        float4 *sNodes = reinterpret_cast<float4 *>(lds);
        float4 *sTris = reinterpret_cast<float4 *>(stk + (Q.stackDepth + 1) * kMeshBlock);
        if (WIDE) {
            for (int i = threadIdx.x; i < Q.numNodes * kLdsNode4F4; i += kMeshBlock) sNodes[i] = Q.nodes[i];
        } else {
            for (int i = threadIdx.x; i < Q.numNodes * 4; i += kMeshBlock)
                sNodes[(i >> 2) * kLdsNodeF4 + (i & 3)] = Q.nodes[i];
        }
        for (int i = threadIdx.x; i < Q.numTris * 3; i += kMeshBlock) sTris[i] = Q.tris[i];
        __syncthreads();
        nodes = sNodes;
        tris = sTris;
    }
    if (TOP && Q.topBytes) {
        float4 *sTop = reinterpret_cast<float4 *>(lds);
        for (unsigned i = threadIdx.x; i < (Q.topBytes >> 4); i += kMeshBlock) sTop[i] = Q.nodes[i];
        __syncthreads();
    }
    constexpr int nodeF4 = WIDE ? (LDS_SCENE ? kLdsNode4F4 : 8) : (LDS_SCENE ? kLdsNodeF4 : 4);
    const SpillArea S{Q.spill, (blockIdx.x * unsigned(kMeshBlock) + threadIdx.x) * unsigned(Q.spillCap), Q.stackCap};
    // shard k: rays [k * per, (k + 1) * per) below numRays, `per` a multiple of 64 (whole lines)
    const unsigned per = ((Q.numRays + kQueryShards * 64u - 1u) / (kQueryShards * 64u)) * 64u;
    unsigned fs = blockIdx.x % kQueryShards, left = kQueryShards;  // the wave's shard; shards not yet found drained
    unsigned fsBase = min(fs * per, Q.numRays), fsCount = min((fs + 1u) * per, Q.numRays) - fsBase;
    unsigned poolNext = 0, poolEnd = 0;
    unsigned idx = kNone;  // this lane's ray
    bool need = true;
    Ray r{};
    float tmin = 0.0f;
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
            if (need && qi != kNone) {
                need = false;
                idx = fsBase + qi;
                const float4 a = Q.rays[2 * size_t(idx)], b = Q.rays[2 * size_t(idx) + 1];
                rng = P.seeds[idx];
                r.ox = a.x;
                r.oy = a.y;
                r.oz = a.z;
                r.dx = b.x;
                r.dy = b.y;
                r.dz = b.z;
                tmin = a.w + 0.0f;  // -0 -> +0: the box test's near bound orders as unsigned
                const float tmax = b.w;
                tr = tg = tb = 1.0f;
                depth = 0;
                hit0 = false;
                begin(T);
                T.bestO = -1;  // a hit at exactly t == tmax loses the tie on the id: tmax is exclusive
                // hipptTraceRays' invalid rays: no segment, (0, 0, 0, 0)
                const bool valid = finite3(r.ox, r.oy, r.oz) && finite3(r.dx, r.dy, r.dz) && fabsf(tmin) < INFINITY &&
                                   (r.dx != 0.0f || r.dy != 0.0f || r.dz != 0.0f) && tmin >= 0.0f && tmax > tmin;
                if (valid) {
                    prepare(r);
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
                if (WIDE)
                    traverse_round_wide<nodeF4, false, FULL, false, true, LDS_SCENE, TOP>(
                        T, r, my, nodes, tris, nvis, ntest, pc, Q.leafExit, Q.nodeExit, S, Q.topBytes, 0u, tmin);
                else
                    traverse_round<nodeF4, false, FULL>(T, r, my, nodes, tris, nvis, ntest, pc, Q.leafExit, Q.nodeExit,
                                                        tmin);
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
                // depth exhausted or absorbed: contributes 0
                if (depth < P.maxDepth &&
                    scatter<FULL, false, -1>(r, T.bestT, T.bestI, Q.shade, tris, P.mats, rng, tr, tg, tb, pc)) {
                    finished = false;
                    prepare(r);
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
template <bool LDS_SCENE, bool FULL>
PathFn path_fn_wide(bool wide) {
    return wide ? path_kernel<LDS_SCENE, FULL, true> : path_kernel<LDS_SCENE, FULL, false>;
}
PathFn path_fn(const QueryParams &q) {
    const bool wide = q.wide != 0;
    if (q.ldsScene) return q.full ? path_fn_wide<true, true>(wide) : path_fn_wide<true, false>(wide);
    return q.full ? path_fn_wide<false, true>(wide) : path_fn_wide<false, false>(wide);
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
    const bool lds = q.ldsScene != 0;
    // the launch's contract with the kernel: what it dereferences is there, the LDS top is whole
    // nodes of the array, claims are whole waves, records are stored whole
    if (!q.nodes || !q.tris || !q.shade || !q.counter || !q.rays || !p.mats || !p.seeds || !p.radiance || blocks <= 0 ||
        q.numRays == 0 || q.chunk < 64 || q.chunk % 64 || q.numRays > (1u << 31) || (q.wide != 0 && q.wide != 1) ||
        p.maxDepth < 1)
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(q.rays) % 16 || reinterpret_cast<uintptr_t>(p.radiance) % 16) return hipErrorInvalidValue;
    if (q.wide && q.stackCap < 1) return hipErrorInvalidValue;
    if (q.wide && !q.spill) return hipErrorInvalidValue;
    if (q.topBytes && (lds || !q.wide || q.topBytes % 128u || q.topBytes > (unsigned(q.numNodes) << 7)))
        return hipErrorInvalidValue;
    const PathFn fn = path_fn(q);
    if (q.wide && (lds || q.topBytes)) {  // the 4-wide traversal reads the LDS nodes at address 0
        const hipError_t e = check_lds_at_zero(reinterpret_cast<const void *>(fn));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kMeshBlock), query_lds_bytes(q), s, p);
    return hipGetLastError();
}

int path_blocks_per_cu(const PathParams &p) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, path_fn(p.q), kMeshBlock, query_lds_bytes(p.q)) != hipSuccess ||
        n <= 0)
        n = 1;
    return std::min(n, 8);
}

hipError_t launch_camera_rays(const CameraRaysParams &p, hipStream_t s) {
    if ((!p.rays && !p.seeds) || p.numRays == 0 || p.numRays > (1u << 31) || reinterpret_cast<uintptr_t>(p.rays) % 16)
        return hipErrorInvalidValue;
    const unsigned blocks = (p.numRays + unsigned(kCameraRaysBlock) - 1u) / unsigned(kCameraRaysBlock);
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(kCameraRaysBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace hippt
