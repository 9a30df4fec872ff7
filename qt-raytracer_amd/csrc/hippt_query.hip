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

#include "hippt_ray_loop.h"

namespace hippt {
namespace {
using namespace rayloop;

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
// FULL: spheres present; WIDE: the 4-wide tree; MODE: hippt_query.h QueryMode.
template <bool LDS_SCENE, bool FULL, bool WIDE, QueryMode MODE>
__global__ __launch_bounds__(kMeshBlock) void query_kernel(QueryParams Q) {
    constexpr bool ANY = MODE == QueryMode::Any, CAMERA = query_camera(MODE), HITS = query_hits(MODE);
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
                bool valid;
                if (CAMERA) {
                    uint32_t rng;
                    camera_sample(Q.cam, Q.firstItem + idx, r, rng);
                    tmin = 0.001f;
                    tmax = INFINITY;
                    valid = query_ray_valid(r, tmin, tmax);
                } else {
                    valid = load_query_ray(Q.rays, idx, r, tmin, tmax);
                }
                begin_query_ray<FULL, WIDE>(T, r, tmax, valid, M);
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
                if (hit) hit_record<FULL>(T, r, Q.shade, sc.tris, h0, h1);
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
QueryFn query_fn_mode(QueryMode mode) {
    switch (mode) {
    case QueryMode::Any: return query_kernel<LDS_SCENE, FULL, WIDE, QueryMode::Any>;
    case QueryMode::Camera: return query_kernel<LDS_SCENE, FULL, WIDE, QueryMode::Camera>;
    case QueryMode::Hits: return query_kernel<LDS_SCENE, FULL, WIDE, QueryMode::Hits>;
    case QueryMode::CameraHits: return query_kernel<LDS_SCENE, FULL, WIDE, QueryMode::CameraHits>;
    default: return query_kernel<LDS_SCENE, FULL, WIDE, QueryMode::Closest>;
    }
}
QueryFn query_fn(const QueryParams &q, QueryMode mode) {
    return for_scene_layout(q, [&](auto lds, auto full, auto wide) { return query_fn_mode<lds(), full(), wide()>(mode); });
}

}  // namespace

size_t query_lds_bytes(const QueryParams &q) {
    const bool lds = q.ldsScene != 0;
    return mesh_lds_bytes(q.stackDepth, lds ? q.numNodes : 0, lds ? q.numTris : 0, q.wide != 0, q.topBytes);
}

hipError_t launch_query(const QueryParams &q, int blocks, QueryMode mode, hipStream_t s) {
    if (!query_params_ok(q, blocks)) return hipErrorInvalidValue;
    // the mode's own pointers: two 16-byte stores per hit record, from the shade records
    if (query_hits(mode) ? (!q.shade || !q.hits || reinterpret_cast<uintptr_t>(q.hits) % 16)
        : mode == QueryMode::Any ? !q.occluded
                                 : (!q.t && !q.prim))
        return hipErrorInvalidValue;
    if (!query_camera(mode) && !q.rays) return hipErrorInvalidValue;
    return launch_ray_kernel(query_fn(q, mode), q, q, blocks, s);
}

int query_blocks_per_cu(const QueryParams &q, QueryMode mode) { return ray_kernel_blocks_per_cu(query_fn(q, mode), q); }

}  // namespace hippt
