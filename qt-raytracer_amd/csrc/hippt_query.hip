// hippt_query.hip — batched ray queries over the uploaded scene: closest hit (t, original primitive
// id), occlusion, and the camera's first-hit buffers (include/hippt.h hipptTraceRays, hipptOccluded,
// hipptTraceCamera).
//
// hipptTraceHits / hipptTraceCameraHits are the closest-hit query with a longer epilogue (HITS): the
// 32-byte hit record in place of (t, id).
//
// One persistent kernel shaped like wf_extend (hippt_wavefront.hip): 256-thread blocks, each lane a
// ray; a wave claims runs of consecutive ray indices from its shard's counter (hippt_query.h
// kQueryShards) and its finished lanes refill by ballot, consecutive requesting lanes taking consecutive indices, so that the 32-byte ray reads
// and the 4-byte / 1-byte result writes cover whole lines.  The traversal is the renderer's
// speculative while-while round (hippt_trace.h traverse_round / traverse_round_wide over float
// nodes, per-lane LDS stack with spill), with the ray's own tmin in place of the renderer's 0.001
// and the ray's tmax as the starting bestT.
//
// The contract is the renderer's (DESIGN.md "Semantic contract"): the closest hit is the
// lexicographic minimum of (t, original primitive id) over the hits with tmin <= t < tmax, every t
// computed with the oracle's arithmetic; the box test only culls.
#include "hippt_query.h"

#include <algorithm>

#include "hippt_trace.h"

namespace hippt {
namespace {
using namespace trace;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// The hit record (include/hippt.h hipptHit) of the finished traversal T of ray r, as two float4: the
// winner's shade record and primitive (leaf-order index T.bestI; `tris` is the LDS copy where the scene
// is there) give the normal as scatter() forms and faces it, the barycentrics as test_prim_data's
// un / det and vn / det, and the material word.
template <bool FULL>
__device__ __forceinline__ void hit_record(const Trav &T, const Ray &r, const float4 *shade, const float4 *tris,
                                           float4 &h0, float4 &h1) {
    const float4 sh = shade[T.bestI];
    const float4 *tp = tris + 3 * T.bestI;
    const float4 A = tp[0], B = tp[1], Cc = tp[2];
    int mw = __float_as_int(sh.w);
    float nx = sh.x, ny = sh.y, nz = sh.z, u = 0.0f, v = 0.0f;
    if (FULL && (mw & kShadeSphere)) {  // (p - center) / radius, p = Ray::at(t)
        const float px = fmaf(T.bestT, r.dx, r.ox), py = fmaf(T.bestT, r.dy, r.oy), pz = fmaf(T.bestT, r.dz, r.oz);
        nx = (px - sh.x) / A.w;
        ny = (py - sh.y) / A.w;
        nz = (pz - sh.z) / A.w;
    } else {  // test_prim_data's det, un, vn
        const float e1x = A.w, e1y = B.x, e1z = B.y;
        const float e2x = B.z, e2y = B.w, e2z = Cc.x;
        const float pvx = fmaf(r.dy, e2z, -(r.dz * e2y));
        const float pvy = fmaf(r.dz, e2x, -(r.dx * e2z));
        const float pvz = fmaf(r.dx, e2y, -(r.dy * e2x));
        const float det = fdot(e1x, e1y, e1z, pvx, pvy, pvz);
        const float tvx = r.ox - A.x, tvy = r.oy - A.y, tvz = r.oz - A.z;
        const float qvx = fmaf(tvy, e1z, -(tvz * e1y));
        const float qvy = fmaf(tvz, e1x, -(tvx * e1z));
        const float qvz = fmaf(tvx, e1y, -(tvy * e1x));
        u = fdot(tvx, tvy, tvz, pvx, pvy, pvz) / det;
        v = fdot(r.dx, r.dy, r.dz, qvx, qvy, qvz) / det;
    }
    if (!(fdot(r.dx, r.dy, r.dz, nx, ny, nz) < 0.0f)) {  // set_face_normal
        nx = -nx;
        ny = -ny;
        nz = -nz;
        mw |= int(0x80000000u);  // HIPPT_HIT_BACKFACE
    }
    h0 = float4{T.bestT, __int_as_float(T.bestO), nx, ny};
    h1 = float4{nz, u, v, __int_as_float(mw)};
}

// LDS_SCENE: the scene copy in LDS (else the tree in global memory, the top of a 4-wide one in LDS);
// FULL: spheres present; WIDE: the 4-wide tree; ANY: occlusion; CAMERA: rays from camera_sample;
// HITS: hit records (hit_record below) in place of (t, prim), not with ANY.
template <bool LDS_SCENE, bool FULL, bool WIDE, bool ANY, bool CAMERA, bool HITS>
__global__ __launch_bounds__(kMeshBlock) void query_kernel(QueryParams Q) {
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
    unsigned idx = kNone;   // this lane's ray
    bool need = true;
    Ray r{};
    float tmin = 0.0f;
    Trav T;
    begin(T);
    T.cur = kDone;
    T.bestO = -1;
    unsigned long long nvis = 0, ntest = 0;
    unsigned pc[kProfSlots] = {};  // phase profile slots (not reported by the queries)
    for (;;) {
        while (left && __ballot(need)) {
            const unsigned qi =
                wave_fetch(need, poolNext, poolEnd, &Q.counter[fs * kQueryCtrStride], Q.chunk, fsCount);
            if (need && qi != kNone) {
                need = false;
                idx = fsBase + qi;
                float tmax;
                if (CAMERA) {
                    uint32_t rng;
                    camera_sample(Q.cam, Q.firstItem + idx, r, rng);
                    tmin = 0.001f;
                    tmax = INFINITY;
                } else {
                    const float4 a = Q.rays[2 * size_t(idx)], b = Q.rays[2 * size_t(idx) + 1];
                    r.ox = a.x;
                    r.oy = a.y;
                    r.oz = a.z;
                    r.dx = b.x;
                    r.dy = b.y;
                    r.dz = b.z;
                    tmin = a.w + 0.0f;  // -0 -> +0: the box test's near bound orders as unsigned
                    tmax = b.w;
                }
                begin(T);
                T.bestO = -1;  // a hit at exactly t == tmax loses the tie on the id: tmax is exclusive
                // rays that are a miss without being traversed (the oracle's arithmetic agrees):
                // non-finite origin, direction or tmin, NaN tmax, zero direction, tmin < 0, tmax <= tmin
                const bool valid = finite3(r.ox, r.oy, r.oz) && finite3(r.dx, r.dy, r.dz) && fabsf(tmin) < INFINITY &&
                                   (r.dx != 0.0f || r.dy != 0.0f || r.dz != 0.0f) && tmin >= 0.0f && tmax > tmin;
                if (valid) {
                    prepare(r);
                    T.bestT = tmax;
                } else {
                    T.cur = kDone;
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
                if (ANY && T.bestO >= 0) {  // occlusion: any accepted hit answers the ray
                    T.cur = kDone;
                    T.leaf = 0;
                    T.sp = 0;
                    T.ovf = 0;
                }
            } while (__popcll(__ballot(busy(T))) > unsigned(Q.waveThreshold));
        }
        if (idx != kNone && !busy(T)) {
            const bool hit = T.bestO >= 0;  // T.bestO: the original id (T.bestI is the leaf-order index)
            if (HITS) {
                float4 h0{INFINITY, __int_as_float(-1), 0.0f, 0.0f}, h1{0.0f, 0.0f, 0.0f, __int_as_float(-1)};
                if (hit) hit_record<FULL>(T, r, Q.shade, tris, h0, h1);
                float4 *const out = Q.hits + 2 * size_t(idx);
                out[0] = h0;
                out[1] = h1;
            } else if (ANY) {
                Q.occluded[idx] = hit ? 1 : 0;
            } else {
                if (Q.t) Q.t[idx] = hit ? T.bestT : INFINITY;
                if (Q.prim) Q.prim[idx] = hit ? T.bestO : -1;
            }
            idx = kNone;
            need = true;
        }
    }
}

using QueryFn = void (*)(QueryParams);
template <bool LDS_SCENE, bool FULL, bool WIDE>
QueryFn query_fn_mode(bool any, bool camera, bool hits) {
    if (hits)
        return camera ? query_kernel<LDS_SCENE, FULL, WIDE, false, true, true>
                      : query_kernel<LDS_SCENE, FULL, WIDE, false, false, true>;
    if (camera) return query_kernel<LDS_SCENE, FULL, WIDE, false, true, false>;
    return any ? query_kernel<LDS_SCENE, FULL, WIDE, true, false, false>
               : query_kernel<LDS_SCENE, FULL, WIDE, false, false, false>;
}
template <bool LDS_SCENE, bool FULL>
QueryFn query_fn_wide(bool wide, bool any, bool camera, bool hits) {
    return wide ? query_fn_mode<LDS_SCENE, FULL, true>(any, camera, hits)
                : query_fn_mode<LDS_SCENE, FULL, false>(any, camera, hits);
}
QueryFn query_fn(const QueryParams &q, bool any, bool camera, bool hits) {
    const bool wide = q.wide != 0;
    if (q.ldsScene)
        return q.full ? query_fn_wide<true, true>(wide, any, camera, hits)
                      : query_fn_wide<true, false>(wide, any, camera, hits);
    return q.full ? query_fn_wide<false, true>(wide, any, camera, hits)
                  : query_fn_wide<false, false>(wide, any, camera, hits);
}

}  // namespace

size_t query_lds_bytes(const QueryParams &q) {
    const bool lds = q.ldsScene != 0;
    return mesh_lds_bytes(q.stackDepth, lds ? q.numNodes : 0, lds ? q.numTris : 0, q.wide != 0, q.topBytes);
}

hipError_t launch_query(const QueryParams &q, int blocks, bool any, bool camera, bool hits, hipStream_t s) {
    const bool lds = q.ldsScene != 0;
    // the launch's contract with the kernel: what it dereferences is there, the LDS top is whole
    // nodes of the array, claims are whole waves
    if (!q.nodes || !q.tris || !q.counter || blocks <= 0 || q.numRays == 0 || q.chunk < 64 || q.chunk % 64 ||
        q.numRays > (1u << 31) || (q.wide != 0 && q.wide != 1) || (any && camera))
        return hipErrorInvalidValue;
    if (hits) {  // hit records: not with occlusion, the shade records there, two 16-byte stores per record
        if (any || !q.shade || !q.hits || reinterpret_cast<uintptr_t>(q.hits) % 16) return hipErrorInvalidValue;
    } else if (any ? !q.occluded : (!q.t && !q.prim)) {
        return hipErrorInvalidValue;
    }
    if (!camera && !q.rays) return hipErrorInvalidValue;
    if (q.wide && q.stackCap < 1) return hipErrorInvalidValue;
    if (q.wide && !q.spill) return hipErrorInvalidValue;
    if (q.topBytes && (lds || !q.wide || q.topBytes % 128u || q.topBytes > (unsigned(q.numNodes) << 7)))
        return hipErrorInvalidValue;
    const QueryFn fn = query_fn(q, any, camera, hits);
    if (q.wide && (lds || q.topBytes)) {  // the 4-wide traversal reads the LDS nodes at address 0
        const hipError_t e = check_lds_at_zero(reinterpret_cast<const void *>(fn));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kMeshBlock), query_lds_bytes(q), s, q);
    return hipGetLastError();
}

int query_blocks_per_cu(const QueryParams &q, bool any, bool camera, bool hits) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, query_fn(q, any, camera, hits), kMeshBlock, query_lds_bytes(q)) !=
            hipSuccess ||
        n <= 0)
        n = 1;
    return std::min(n, 8);
}

}  // namespace hippt
