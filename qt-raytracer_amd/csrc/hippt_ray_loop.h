// hippt_ray_loop.h — what the ray-per-lane query kernels share (hippt_query.hip query_kernel,
// hippt_path.hip path_kernel; the scene staging also hippt_wavefront.hip wf_extend): the scene copy in
// LDS, the ray load with its validity rule, the traversal round and the launch.  A kernel joins them in
// its own persistent loop: stage; then claim ray indices from the shard counters, start the claimed
// rays, traverse until at most waveThreshold lanes are busy, finish the lanes whose traversal has ended.
//
// The loop is written out twice: once in query_kernel, once in path_kernel.  path_kernel's copy serves
// plain paths, light-sampled path queries and the light-sampling render route: what those add sits
// behind the compile-time flags NEE and CAMERA of the one template, and every instantiation has the
// VGPRs, SGPRs and scratch of the separately written kernels it replaced
// (profiles/path_merge/regs.txt).  Sharing between query_kernel and path_kernel is another matter: the
// walk over the shards and the loop moved here (the walk as a small struct, the loop as an inlined
// function over two hooks) compile to other register counts than the code they replace: the walk +1
// or +2 VGPRs in seven 2-wide query kernels, the loop up to +11 in the 2-wide path kernels.  So those
// two stay written out in both kernels.  Device code only.
#pragma once

#include <algorithm>

#include "hippt_query.h"
#include "hippt_trace.h"

namespace hippt {
namespace rayloop {
using namespace trace;

// ---- scene staging ----
// A block's view of the scene after staging: the nodes and primitives to traverse (the LDS copies where
// the scene is there) and the lane's slot of the LDS stack.
struct Staged {
    const float4 *nodes, *tris;
    int *my;
};

// LDS_SCENE: copies the tree and the primitives into LDS (nodes at address 0, then the stack, then the
// primitives: the mesh_lds_bytes layout); else, a 4-wide tree: copies its first topBytes into LDS at
// address 0, below the stack.  Every thread of the block calls it (it synchronises).
template <bool LDS_SCENE, bool WIDE>
__device__ __forceinline__ Staged stage_scene(const float4 *gNodes, const float4 *gTris, int numNodes, int numTris,
                                              int stackDepth, unsigned topBytes) {
    extern __shared__ int lds[];  // LDS scene: nodes at address 0, then stack, primitives
    constexpr int ldsNodeF4 = WIDE ? kLdsNode4F4 : kLdsNodeF4;  // mesh_lds_bytes layout
    constexpr bool TOP = WIDE && !LDS_SCENE;
    int *const stk = LDS_SCENE ? lds + numNodes * ldsNodeF4 * 4 : lds + (TOP ? (topBytes >> 2) : 0u);
    Staged s{gNodes, gTris, stk + threadIdx.x};
    if (LDS_SCENE) {
        float4 *sNodes = reinterpret_cast<float4 *>(lds);
        float4 *sTris = reinterpret_cast<float4 *>(stk + (stackDepth + 1) * kMeshBlock);
        if (WIDE) {
            for (int i = threadIdx.x; i < numNodes * kLdsNode4F4; i += kMeshBlock) sNodes[i] = gNodes[i];
        } else {
            for (int i = threadIdx.x; i < numNodes * 4; i += kMeshBlock)
                sNodes[(i >> 2) * kLdsNodeF4 + (i & 3)] = gNodes[i];
        }
        for (int i = threadIdx.x; i < numTris * 3; i += kMeshBlock) sTris[i] = gTris[i];
        __syncthreads();
        s.nodes = sNodes;
        s.tris = sTris;
    }
    if (TOP && topBytes) {
        float4 *sTop = reinterpret_cast<float4 *>(lds);
        for (unsigned i = threadIdx.x; i < (topBytes >> 4); i += kMeshBlock) sTop[i] = gNodes[i];
        __syncthreads();
    }
    return s;
}

// This lane's part of the launch's stack spill area (MeshParams::spill).
__device__ __forceinline__ SpillArea lane_spill(int *spill, int spillCap, int stackCap) {
    return SpillArea{spill, (blockIdx.x * unsigned(kMeshBlock) + threadIdx.x) * unsigned(spillCap), stackCap};
}

// ---- ray load ----
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// Rays that are a miss without being traversed (the oracle's arithmetic agrees): non-finite origin,
// direction or tmin, NaN tmax, zero direction, tmin < 0, tmax <= tmin.
__device__ __forceinline__ bool query_ray_valid(const Ray &r, float tmin, float tmax) {
    return finite3(r.ox, r.oy, r.oz) && finite3(r.dx, r.dy, r.dz) && fabsf(tmin) < INFINITY &&
           (r.dx != 0.0f || r.dy != 0.0f || r.dz != 0.0f) && tmin >= 0.0f && tmax > tmin;
}

// Ray idx of a query's ray buffer (2 float4 per ray: (origin, tmin) (direction, tmax)); returns whether
// it is to be traversed (query_ray_valid).
__device__ __forceinline__ bool load_query_ray(const float4 *rays, unsigned idx, Ray &r, float &tmin, float &tmax) {
    const float4 a = rays[2 * size_t(idx)], b = rays[2 * size_t(idx) + 1];
    r.ox = a.x;
    r.oy = a.y;
    r.oz = a.z;
    r.dx = b.x;
    r.dy = b.y;
    r.dz = b.z;
    tmin = a.w + 0.0f;  // -0 -> +0: the box test's near bound orders as unsigned
    tmax = b.w;
    return query_ray_valid(r, tmin, tmax);
}

// ---- the queries' ray ----
// A ray with two origin terms per axis for the box test (hippt_slab.h "the ray queries' box test"):
// Ray's oix, oiy, oiz are the near planes' terms in the 4-wide test and the lo planes' in the 2-wide
// one, fox, foy, foz the far / hi planes'.  The traversal (hippt_trace.h) is the renderer's code over
// this type: child_key and hi_oi* below replace the ones it calls for a Ray.
struct QueryRay : Ray {
    float fox, foy, foz;
};

__device__ __forceinline__ float hi_oix(const QueryRay &r) { return r.fox; }
__device__ __forceinline__ float hi_oiy(const QueryRay &r) { return r.foy; }
__device__ __forceinline__ float hi_oiz(const QueryRay &r) { return r.foz; }

__device__ __forceinline__ unsigned child_key(float nx, float fx, float ny, float fy, float nz, float fz,
                                              const QueryRay &r, float tmin, float bestT) {
    float n;
    return slab::box_hit_query(nx, fx, ny, fy, nz, fz, r.ix, r.iy, r.iz, r.oix, r.oiy, r.oiz, r.fox, r.foy, r.foz, tmin,
                               bestT, n)
               ? __float_as_uint(n)
               : 0xffffffffu;
}

// The scene's M (the largest |coordinate| the builder or the last refit saw) from the pad word.
__device__ __forceinline__ float scene_M(const float *pad) { return pad[0] * float(1 << slab::kPadExponent); }

// prepare() for a caller's ray, which may start anywhere and have any length (hippt_slab.h query_*).
// FULL: the scene may hold spheres, whose arithmetic overflows for long directions (query_all_boxes).
template <bool FULL, bool WIDE>
__device__ __forceinline__ void prepare_query(QueryRay &r, float M) {
    const float dmax = fmaxf(fabsf(r.dx), fmaxf(fabsf(r.dy), fabsf(r.dz)));
    const float omax = fmaxf(fabsf(r.ox), fmaxf(fabsf(r.oy), fabsf(r.oz)));
    const float reach = omax + M, away = slab::query_away(omax, M);
    const float floor = slab::query_dir_floor(dmax, reach);
    r.ix = __builtin_amdgcn_rcpf(slab::query_clamp_dir(r.dx, floor));
    r.iy = __builtin_amdgcn_rcpf(slab::query_clamp_dir(r.dy, floor));
    r.iz = __builtin_amdgcn_rcpf(slab::query_clamp_dir(r.dz, floor));
    const float tb = slab::query_far_bound(reach, fminf(fabsf(r.ix), fminf(fabsf(r.iy), fabsf(r.iz))));
    float nx, ny, nz, fx, fy, fz;
    slab::query_origin_terms(r.ox, r.dx, r.ix, floor, tb, away, slab::kQuerySlack, nx, fx);
    slab::query_origin_terms(r.oy, r.dy, r.iy, floor, tb, away, slab::kQuerySlack, ny, fy);
    slab::query_origin_terms(r.oz, r.dz, r.iz, floor, tb, away, slab::kQuerySlack, nz, fz);
    if (FULL && slab::query_all_boxes(dmax, reach)) {
        nx = ny = nz = slab::kAllBoxesNear;
        fx = fy = fz = -slab::kAllBoxesNear;
    }
    // 2-wide: the lo planes are the near ones where the direction is positive
    const bool sx = !WIDE && (__float_as_uint(r.ix) >> 31), sy = !WIDE && (__float_as_uint(r.iy) >> 31),
               sz = !WIDE && (__float_as_uint(r.iz) >> 31);
    r.oix = sx ? fx : nx, r.fox = sx ? nx : fx;
    r.oiy = sy ? fy : ny, r.foy = sy ? ny : fy;
    r.oiz = sz ? fz : nz, r.foz = sz ? nz : fz;
}

// prepare() for a ray that starts on a surface of the scene (a path's later segments): the renderer's
// box test, one origin term per axis.
__device__ __forceinline__ void prepare_segment(QueryRay &r) {
    prepare(r);
    r.fox = r.oix, r.foy = r.oiy, r.foz = r.oiz;
}

// Starts the traversal of a query's ray over [tmin, tmax), or, an invalid ray, leaves it finished
// without a hit.
template <bool FULL, bool WIDE>
__device__ __forceinline__ void begin_query_ray(Trav &T, QueryRay &r, float tmax, bool valid, float M) {
    begin(T);
    T.bestO = -1;  // a hit at exactly t == tmax loses the tie on the id: tmax is exclusive
    if (valid) {
        prepare_query<FULL, WIDE>(r, M);
        T.bestT = tmax;
    } else {
        T.cur = kDone;
    }
}

// ---- traversal step ----
// One speculative while-while round of the queries' traversal (hippt_trace.h), over float nodes of
// either width, with the ray's own tmin.
template <bool LDS_SCENE, bool FULL, bool WIDE>
__device__ __forceinline__ void traverse_step(Trav &T, const QueryRay &r, float tmin, const Staged &sc, const QueryParams &Q,
                                              const SpillArea &S, unsigned long long &nvis, unsigned long long &ntest,
                                              unsigned *pc) {
    constexpr int nodeF4 = WIDE ? (LDS_SCENE ? kLdsNode4F4 : 8) : (LDS_SCENE ? kLdsNodeF4 : 4);
    constexpr bool TOP = WIDE && !LDS_SCENE;
    if (WIDE)
        traverse_round_wide<nodeF4, false, FULL, false, true, LDS_SCENE, TOP>(
            T, r, sc.my, sc.nodes, sc.tris, nvis, ntest, pc, Q.leafExit, Q.nodeExit, S, Q.topBytes, 0u, tmin);
    else
        traverse_round<nodeF4, false, FULL>(T, r, sc.my, sc.nodes, sc.tris, nvis, ntest, pc, Q.leafExit, Q.nodeExit, tmin);
}

// ---- launch (host) ----
// Launches a ray-per-lane kernel over q's scene layout, after the check its 4-wide LDS reads need.
template <class Params>
hipError_t launch_ray_kernel(void (*fn)(Params), const QueryParams &q, const Params &p, int blocks, hipStream_t s) {
    if (q.wide && (q.ldsScene || q.topBytes)) {  // the 4-wide traversal reads the LDS nodes at address 0
        const hipError_t e = check_lds_at_zero(reinterpret_cast<const void *>(fn));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kMeshBlock), query_lds_bytes(q), s, p);
    return hipGetLastError();
}

// Resident blocks per CU of such a kernel (at most 8).
template <class Params>
int ray_kernel_blocks_per_cu(void (*fn)(Params), const QueryParams &q) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, kMeshBlock, query_lds_bytes(q)) != hipSuccess || n <= 0) n = 1;
    return std::min(n, 8);
}

}  // namespace rayloop
}  // namespace hippt
