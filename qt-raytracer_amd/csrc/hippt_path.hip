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
//
// Light sampling (HIPPT_OPT_LIGHT_SAMPLING, HIPPT_OPT_LIGHT_SAMPLING_MODE), its weighting against the scatter sample
// (HIPPT_LIGHT_SAMPLING_MIS) and the renderer's own camera start are compile-time flags of the same kernel
// (NEE, MIS, CAMERA): one persistent loop serves plain paths, light-sampled path queries and the
// light-sampling render route.
#include "hippt_path.h"

#include "hippt_env.h"
#include "hippt_ray_loop.h"

namespace hippt {
namespace {
using namespace rayloop;

// ---- light sampling (DESIGN.md §2 "Light sampling", §16; tests/nee_ref.py is the statement of record) ----
// The faced normal scatter() forms at the hit of primitive `prim` at t, and the material's kind: asked
// before scatter() replaces the ray.
__device__ __forceinline__ int hit_normal_kind(const Ray &r, float t, int prim, const float4 *shade, const float4 *prims,
                                               const float4 *mats, float &nx, float &ny, float &nz) {
    const float4 sh = shade[prim];
    const int mw = __float_as_int(sh.w);
    nx = sh.x, ny = sh.y, nz = sh.z;
    if (mw & kShadeSphere) {
        const float px = fmaf(t, r.dx, r.ox), py = fmaf(t, r.dy, r.oy), pz = fmaf(t, r.dz, r.oz);
        const float rad = prims[3 * prim].w;
        nx = (px - sh.x) / rad;
        ny = (py - sh.y) / rad;
        nz = (pz - sh.z) / rad;
    }
    if (!(fdot(r.dx, r.dy, r.dz, nx, ny, nz) < 0.0f)) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    return __float_as_int(mats[2 * (mw & ~kShadeSphere)].w);
}

// The area of light `k` (leaf order) as both techniques form it: a triangle's from its edges (v0, e1, e2), a
// sphere's from its radius.
__device__ __forceinline__ float light_area(const float4 *prims, int k, bool sphere) {
    const float4 A = prims[3 * k];
    if (sphere) return (12.566371f * A.w) * A.w;
    const float4 B = prims[3 * k + 1];
    const float e1x = A.w, e1y = B.x, e1z = B.y;
    const float e2x = B.z, e2y = B.w, e2z = prims[3 * k + 2].x;
    const float cx = fmaf(e1y, e2z, -(e1z * e2y)), cy = fmaf(e1z, e2x, -(e1x * e2z)), cz = fmaf(e1x, e2y, -(e1y * e2x));
    return 0.5f * sqrtf(fdot(cx, cy, cz, cx, cy, cz));
}

// One connection from the Lambertian vertex p (faced normal n, throughput t* after the scatter): picks a
// light (uniformly over the list, or under SELECT, HIPPT_LIGHT_SELECT_POWER, by the selection table `cdf`: one
// draw either way) and a point on it from `rng`, and returns whether a shadow ray is to be traced; then (wx, wy, wz)
// is its unit direction, (l0, l1, l2) what the light adds if the ray's closest hit is primitive `lk`
// (leaf order).  The draws are consumed either way.  MIS: the power heuristic's weight against the scatter
// sample, 1 / (1 + g^2), is in (l0, l1, l2), and a g that is not below +inf makes no shadow ray.
// ENVS (HIPPT_OPT_ENV_SAMPLING): the coin sent this connection to the lights with probability 1/2, so twice the inverse
// selection probability stands where it stood (exact: a power of two).
template <bool MIS, bool SELECT, bool ENVS>
__device__ __forceinline__ bool light_connect(const int *lights, int numLights, const unsigned *cdf, const float *ipPrim,
                                              const float4 *shade, const float4 *prims, const float4 *mats, float px,
                                              float py, float pz, float nx, float ny,
                                              float nz, float tr, float tg, float tb, uint32_t &rng, unsigned *pc,
                                              float &wx, float &wy, float &wz, float &l0, float &l1, float &l2, int &lk) {
    float nl = float(numLights);
    if (SELECT) {  // by the selection table: the smallest j with c_j > x, x uniform below T
        rng = hash32(rng);
        const unsigned total = cdf[numLights - 1];
        if (total == 0u) return false;  // no light can add anything: no further draw
        const unsigned x = __umulhi(rng, total);
        int lo = 0, hi = numLights - 1;  // c_hi = T > x
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] > x)
                hi = mid;
            else
                lo = mid + 1;
        }
        lk = lights[lo];
        nl = ipPrim[lk];
    } else {
        lk = lights[min(int(rand01(rng) * nl), numLights - 1)];
    }
    const float4 sh = shade[lk];
    const float4 A = prims[3 * lk], B = prims[3 * lk + 1];
    const int mw = __float_as_int(sh.w);
    const float4 le = mats[2 * (mw & ~kShadeSphere)];
    float qx, qy, qz, lx, ly, lz, area;
    bool flip = false, sphere = (mw & kShadeSphere) != 0;
    if (sphere) {  // (centre, r): c + r * unit(random_in_unit_sphere), the Lambertian scatter's draw
        float ux, uy, uz;
        const float inv = rsqrt_unit_draw(rius<false, -1>(rng, ux, uy, uz, pc));
        lx = ux * inv, ly = uy * inv, lz = uz * inv;
        const float rad = A.w;
        qx = fmaf(rad, lx, sh.x), qy = fmaf(rad, ly, sh.y), qz = fmaf(rad, lz, sh.z);
        area = light_area(prims, lk, true);
        const float ox = px - sh.x, oy = py - sh.y, oz = pz - sh.z;
        flip = fdot(ox, oy, oz, ox, oy, oz) >= rad * rad;  // seen from outside: the near side emits
    } else {  // (v0, e1, e2): uniform by folding the unit square
        float a = rand01(rng), b = rand01(rng);
        if (a + b > 1.0f) {
            a = 1.0f - a;
            b = 1.0f - b;
        }
        const float e1x = A.w, e1y = B.x, e1z = B.y;
        const float e2x = B.z, e2y = B.w, e2z = prims[3 * lk + 2].x;
        qx = fmaf(b, e2x, fmaf(a, e1x, A.x)), qy = fmaf(b, e2y, fmaf(a, e1y, A.y)), qz = fmaf(b, e2z, fmaf(a, e1z, A.z));
        area = light_area(prims, lk, false);
        lx = sh.x, ly = sh.y, lz = sh.z;
    }
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    const float d2 = fdot(dx, dy, dz, dx, dy, dz);
    const float il = rsqrt_rn(d2);
    wx = dx * il, wy = dy * il, wz = dz * il;
    const float cosS = fdot(nx, ny, nz, wx, wy, wz);
    const float sL = fdot(lx, ly, lz, wx, wy, wz);
    const float cosL = sphere ? (flip ? -sL : sL) : fabsf(sL);
    if (ENVS) nl = nl * 2.0f;
    if (!(cosS > 0.0f) || !(cosL > 0.0f) || !(d2 > 0.0f) || !(area > 0.0f)) return false;
    float g = (((cosS * cosL) * area) * nl) / (3.14159274f * d2);
    if (MIS) {
        if (!(g < INFINITY)) return false;
        g = g / fmaf(g, g, 1.0f);
    }
    l0 = (tr * le.x) * g;
    l1 = (tg * le.y) * g;
    l2 = (tb * le.z) * g;
    return true;
}

// MIS: the weight wb of the emission of light `prim`, met at t on the segment r that a Lambertian scatter
// with cosine cb to its normal started: the scatter's density against light sampling's at that point,
// squared (the power heuristic); 1 where light sampling could not have produced the point.
template <bool SELECT, bool ENVS>
__device__ __forceinline__ float light_hit_weight(const Ray &r, float t, int prim, const float4 *shade, const float4 *prims,
                                                  float cb, int numLights, const float *ipPrim) {
    const float4 sh = shade[prim];
    const bool sphere = (__float_as_int(sh.w) & kShadeSphere) != 0;
    const float dd = fdot(r.dx, r.dy, r.dz, r.dx, r.dy, r.dz);
    const float d2 = (t * t) * dd;
    const float inv = rsqrt_rn(dd);
    float nx = sh.x, ny = sh.y, nz = sh.z;
    if (sphere) {
        const float px = fmaf(t, r.dx, r.ox), py = fmaf(t, r.dy, r.oy), pz = fmaf(t, r.dz, r.oz);
        const float rad = prims[3 * prim].w;
        nx = (px - sh.x) / rad;
        ny = (py - sh.y) / rad;
        nz = (pz - sh.z) / rad;
    }
    const float cosL = fabsf(fdot(nx, ny, nz, r.dx * inv, r.dy * inv, r.dz * inv));
    const float area = light_area(prims, prim, sphere);
    // the inverse of the light's selection probability: the count, or the table's ip (0: never selected)
    float nl = SELECT ? ipPrim[prim] : float(numLights);
    if (ENVS) nl = nl * 2.0f;  // (the coin's 1/2)
    float wb = 1.0f;
    if (cb > 0.0f && cosL > 0.0f && d2 > 0.0f && area > 0.0f && (!SELECT || nl > 0.0f)) {
        const float gh = (((cb * cosL) * area) * nl) / (3.14159274f * d2);
        const float s = gh * gh;
        if (s < INFINITY) wb = s / fmaf(gh, gh, 1.0f);
    }
    return wb;
}

// ---- environment sampling (HIPPT_OPT_ENV_SAMPLING; tests/envs_ref.py is the statement of record) ----
// One connection from a Lambertian vertex (faced normal n, throughput t* after the scatter) to the map: a
// direction from the selection table (hippt_env.h draw: four draws from `rng`, consumed either way), and whether
// a shadow ray is to be traced; then (wx, wy, wz) is its unit direction and (l0, l1, l2) what the map adds if the
// ray has no hit at all.  `sel`: the coin's probability of the map (1 without lights).  MIS as in light_connect.
template <bool MIS>
__device__ __forceinline__ bool env_connect(const PathParams &P, float sel, float nx, float ny, float nz, float tr,
                                            float tg, float tb, uint32_t &rng, float &wx, float &wy, float &wz,
                                            float &l0, float &l1, float &l2) {
    const env::Draw d = env::draw(P.envRowC, P.envTexels, P.envSize, rng);
    wx = d.ox, wy = d.oy, wz = d.oz;
    float g;
    if (!env::connect_factor(d, fdot(nx, ny, nz, d.ox, d.oy, d.oz), sel, MIS, g)) return false;
    float e0, e1, e2;
    env::lookup(P.env, P.envSize, d.ox, d.oy, d.oz, e0, e1, e2);
    l0 = (tr * e0) * g;
    l1 = (tg * e1) * g;
    l2 = (tb * e2) * g;
    return true;
}

// The connection of a Lambertian vertex under ENVS: to the map, or in a scene with lights (LIT; the coin is drawn
// whenever the scene holds one) by a fair coin to the map or to a light.  lk = -1 marks the map.
template <bool MIS, bool SELECT, bool LIT>
__device__ __forceinline__ bool envs_connect(const PathParams &P, const float4 *shade, const float4 *prims, float px,
                                             float py, float pz, float nx, float ny, float nz, float tr, float tg, float tb,
                                             uint32_t &rng, unsigned *pc, float &wx, float &wy, float &wz, float &l0,
                                             float &l1, float &l2, int &lk) {
    float sel = 1.0f;
    if (LIT) {
        sel = 0.5f;
        if (!(rand01(rng) < 0.5f))
            return light_connect<MIS, SELECT, true>(P.lights, P.numLights, P.lightCdf, P.lightIp, shade, prims, P.mats, px,
                                                    py, pz, nx, ny, nz, tr, tg, tb, rng, pc, wx, wy, wz, l0, l1, l2, lk);
    }
    lk = -1;
    return env_connect<MIS>(P, sel, nx, ny, nz, tr, tg, tb, rng, wx, wy, wz, l0, l1, l2);
}

// LDS_SCENE: the scene copy in LDS (else the tree in global memory, the top of a 4-wide one in LDS);
// FULL: spheres or materials other than Lambertian present; WIDE: the 4-wide tree.
// NEE: light sampling, for scenes that hold a light (general kernels only: FULL).  A lane's path gains a
// shadow phase: after a Lambertian scatter that connects, the lane first traverses the shadow ray (p, w)
// from the scattered ray's origin, keeping the scattered direction, the connection's radiance and the
// light's index; when that traversal ends it adds the radiance if the closest hit is the light and goes on
// along the scattered ray.  Shadow and path segments share the traversal rounds.  Everything it adds is
// under the flag: without it the kernel holds none of the state below "light sampling".
// CAMERA (with NEE): the renderer's samples in place of the caller's rays (PathParams::scratch).
// MIS (with NEE): HIPPT_LIGHT_SAMPLING_MIS (tests/mis_ref.py is the statement of record).  In
// place of `spec` the path carries cb, the cosine of the last scatter if it was Lambertian, else -1; the
// connection and a light met after a Lambertian scatter are each weighted against the other technique.
// SELECT (with NEE): HIPPT_LIGHT_SELECT_POWER (tests/select_ref.py is the statement of record): the
// connection's light comes from the selection table (PathParams::lightCdf) and the table's ip stands where
// float(numLights) stood.  A flag and not a branch on the pointer: the branch cost every NEE kernel 1 to 4 VGPRs,
// and three of the 2-wide query kernels an occupancy step, with the option off.
// ENV (general kernels only: FULL): hipptSetEnvironment (tests/env_ref.py is the statement of
// record).  A miss takes throughput x env(d) of the map (PathParams::env, hippt_env.h) in place of the sky
// gradient, d the missed segment's direction as the path holds it; nothing else changes.  A flag for the
// reason SELECT is one.  With ENV the camera start serves plain paths too: an environment sends every mesh
// render down the ray-per-lane route.
// ENVS (with NEE and ENV): HIPPT_OPT_ENV_SAMPLING.  A Lambertian vertex connects to the map (env_connect) or, in
// a scene with lights (LIT, with ENVS: P.numLights > 0), by a fair coin to the map or to a light; lk = -1 marks a
// connection to the map, visible iff the shadow ray has no hit.  A miss after a Lambertian scatter adds nothing
// (the connection counted it) or, with MIS, env(d) by the scatter sample's weight.  NEE is then on whether or not
// the scene holds a light.  LIT is a flag and not a branch on P.numLights: without the light connection the
// sixteen kernels of a scene without lights, the common case under a sky, take 3 to 6 VGPRs fewer, and six of them
// stand an occupancy step higher (profiles/env_sampling/regs.txt).
template <bool LDS_SCENE, bool FULL, bool WIDE, bool NEE, bool CAMERA, bool MIS, bool SELECT, bool ENV, bool ENVS, bool LIT>
__global__ __launch_bounds__(kMeshBlock) void path_kernel(PathParams P) {
    static_assert(FULL || !NEE, "light sampling has general kernels only");
    static_assert(FULL || !ENV, "the environment has general kernels only");
    static_assert(NEE || ENV || !CAMERA, "the camera start belongs to the ray-per-lane render route");
    static_assert(NEE || !MIS, "the weights belong to light sampling");
    static_assert(NEE || !SELECT, "the light choice belongs to light sampling");
    static_assert((NEE && ENV) || !ENVS, "environment sampling belongs to light sampling under an environment");
    static_assert(ENVS || !LIT, "the coin belongs to environment sampling");
    static_assert(LIT || !ENVS || !SELECT, "the light choice needs lights");
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
    // light sampling: the segments traced so far (shadow segments too), the radiance gathered so far,
    // whether a light met next emits (the last scatter was not Lambertian), and the shadow phase's kept
    // values
    int nseg = 0;
    float la0 = 0.0f, la1 = 0.0f, la2 = 0.0f;
    bool spec = true, shadow = false;
    float cb = -1.0f;  // (MIS: in place of spec)
    float sdx = 0.0f, sdy = 0.0f, sdz = 0.0f, ld0 = 0.0f, ld1 = 0.0f, ld2 = 0.0f;
    int lk = -1;
    unsigned long long segsAll = 0, samplesAll = 0;  // CAMERA: the launch counters' share of this lane
    unsigned shadowAll = 0;                          // (the shadow segments among segsAll)
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
                bool valid;
                if (CAMERA) {
                    camera_sample(Q.cam, Q.firstItem + idx, r, rng);
                    tmin = 0.001f;
                    tmax = INFINITY;
                    valid = query_ray_valid(r, tmin, tmax);
                } else {
                    rng = P.seeds[idx];  // (before the ray: the three loads are in flight together)
                    valid = load_query_ray(Q.rays, idx, r, tmin, tmax);
                }
                tr = tg = tb = 1.0f;
                depth = 0;
                hit0 = false;
                if (NEE) {
                    la0 = la1 = la2 = 0.0f;
                    nseg = 0;
                    spec = true;
                    cb = -1.0f;
                    shadow = false;
                }
                // begin_query_ray, with the mark of hipptTraceRays' invalid rays (no segment, (0, 0, 0, 0))
                // in its branch: set after it, the mark costs path_kernel<false, false, false, false, false, false, false, false, false, false>
                // 2 VGPRs
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
            if (NEE && shadow) {  // the shadow segment: visible iff its closest hit is the light itself
                ++nseg;
                if (CAMERA) ++shadowAll;
                if (ENVS && lk < 0 ? T.bestI < 0 : T.bestI == lk) {
                    la0 += ld0;
                    la1 += ld1;
                    la2 += ld2;
                }
                shadow = false;
                finished = false;
                r.dx = sdx, r.dy = sdy, r.dz = sdz;  // on along the scattered ray
                prepare_segment(r);
                begin(T);
            } else if (depth < 0) {
                // invalid ray
            } else if (T.bestI < 0) {  // miss: the sky, or the environment, of the segment's direction
                if (ENV) {
                    float e0, e1, e2;
                    env::lookup(P.env, P.envSize, r.dx, r.dy, r.dz, e0, e1, e2);
                    L0 = tr * e0;
                    L1 = tg * e1;
                    L2 = tb * e2;
                    if (ENVS) {  // after a Lambertian scatter: counted by the connection, or weighted against it
                        if (MIS) {
                            if (!(cb < 0.0f)) {
                                const float wb = env::miss_weight(P.envTexels, P.envSize, r.dx, r.dy, r.dz, cb,
                                                                  LIT ? 0.5f : 1.0f);
                                L0 *= wb;
                                L1 *= wb;
                                L2 *= wb;
                            }
                        } else if (!spec) {
                            L0 = L1 = L2 = 0.0f;
                        }
                    }
                } else {
                    sky(r, tr, tg, tb, L0, L1, L2);
                }
                segs = depth + 1;
                if (NEE) ++nseg;
            } else {
                hit0 = true;
                segs = ++depth;
                if (NEE) ++nseg;
                if (FULL && emitted(T.bestI, Q.shade, P.mats, tr, tg, tb, L0, L1, L2)) {
                    // ends at a light with throughput x emission, whatever the depth; light
                    // sampling: unless the vertex before it sampled the lights itself; with MIS: then with the
                    // scatter sample's weight
                    if (MIS) {
                        if (!(cb < 0.0f)) {
                            const float wb = light_hit_weight<SELECT, ENVS>(r, T.bestT, T.bestI, Q.shade, sc.tris, cb,
                                                                      P.numLights, P.lightIp);
                            L0 *= wb;
                            L1 *= wb;
                            L2 *= wb;
                        }
                    } else if (NEE && !spec) {
                        L0 = L1 = L2 = 0.0f;
                    }
                } else if (depth < P.maxDepth) {  // depth exhausted or absorbed: contributes 0
                    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
                    int kind = kLambertian;
                    if (NEE) kind = hit_normal_kind(r, T.bestT, T.bestI, Q.shade, sc.tris, P.mats, nx, ny, nz);
                    if (scatter<FULL, false, -1>(r, T.bestT, T.bestI, Q.shade, sc.tris, P.mats, rng, tr, tg, tb, pc)) {
                        finished = false;
                        if (NEE) {
                            spec = kind != kLambertian;
                            if (MIS)
                                cb = spec ? -1.0f
                                          : fdot(nx, ny, nz, r.dx, r.dy, r.dz) *
                                                rsqrt_rn(fdot(r.dx, r.dy, r.dz, r.dx, r.dy, r.dz));
                            float wx, wy, wz;
                            if (!spec &&
                                (ENVS ? envs_connect<MIS, SELECT, LIT>(P, Q.shade, sc.tris, r.ox, r.oy, r.oz, nx, ny, nz, tr, tg,
                                                                  tb, rng, pc, wx, wy, wz, ld0, ld1, ld2, lk)
                                      : light_connect<MIS, SELECT, false>(P.lights, P.numLights, P.lightCdf, P.lightIp,
                                                                          Q.shade, sc.tris, P.mats, r.ox, r.oy, r.oz, nx, ny,
                                                                          nz, tr, tg, tb, rng, pc, wx, wy, wz, ld0, ld1, ld2,
                                                                          lk))) {
                                shadow = true;
                                sdx = r.dx, sdy = r.dy, sdz = r.dz;
                                r.dx = wx, r.dy = wy, r.dz = wz;
                            }
                        }
                        prepare_segment(r);  // on a surface of the scene: the renderer's test
                        begin(T);
                        tmin = 0.001f;
                    }
                }
            }
            if (finished) {
                if (NEE) {  // (not for plain paths: 0 + L is not L for L = -0)
                    L0 = la0 + L0;
                    L1 = la1 + L1;
                    L2 = la2 + L2;
                    segs = nseg;
                }
                if (CAMERA) {
                    store_radiance(P.scratch, idx, L0, L1, L2);
                    segsAll += unsigned(segs);
                    ++samplesAll;
                } else {
                    P.radiance[idx] = float4{L0, L1, L2, hit0 ? 1.0f : 0.0f};
                    if (P.segments) P.segments[idx] = segs;
                }
                idx = kNone;
                need = true;
            }
        }
    }
    if (CAMERA) {
        segsAll = wave_sum(segsAll);
        samplesAll = wave_sum(samplesAll);
        const unsigned long long shadows = wave_sum((unsigned long long)shadowAll);
        if (__lane_id() == 0) {
            unsigned long long *const st = stat_slot(P.stats);
            atomicAdd(&st[0], segsAll);
            atomicAdd(&st[1], samplesAll);
            atomicAdd(&st[kStatShadowRays], shadows);
        }
    }
}

// The kernel of p's scene layout and route: plain paths in all eight layouts, light sampling (plain or with
// MIS: p.lightMode) and the environment in the four general ones (whatever p.q.full says), for a query or a
// render batch.
using PathFn = void (*)(PathParams);
template <bool L, bool W, bool E>
PathFn general_path_fn(const PathParams &p) {
    const bool cam = p.scratch != nullptr;
    if constexpr (E) {
        if (p.envRowC) {  // environment sampling: the light-sampling kernels, with or without lights
            if (p.numLights > 0 && p.lightCdf) {
                if (p.lightMode == 2)
                    return cam ? path_kernel<L, true, W, true, true, true, true, true, true, true>
                               : path_kernel<L, true, W, true, false, true, true, true, true, true>;
                return cam ? path_kernel<L, true, W, true, true, false, true, true, true, true>
                           : path_kernel<L, true, W, true, false, false, true, true, true, true>;
            }
            if (p.numLights > 0) {
                if (p.lightMode == 2)
                    return cam ? path_kernel<L, true, W, true, true, true, false, true, true, true>
                               : path_kernel<L, true, W, true, false, true, false, true, true, true>;
                return cam ? path_kernel<L, true, W, true, true, false, false, true, true, true>
                           : path_kernel<L, true, W, true, false, false, false, true, true, true>;
            }
            if (p.lightMode == 2)
                return cam ? path_kernel<L, true, W, true, true, true, false, true, true, false>
                           : path_kernel<L, true, W, true, false, true, false, true, true, false>;
            return cam ? path_kernel<L, true, W, true, true, false, false, true, true, false>
                       : path_kernel<L, true, W, true, false, false, false, true, true, false>;
        }
    }
    if (p.lights && p.lightCdf) {
        if (p.lightMode == 2)
            return cam ? path_kernel<L, true, W, true, true, true, true, E, false, false> : path_kernel<L, true, W, true, false, true, true, E, false, false>;
        return cam ? path_kernel<L, true, W, true, true, false, true, E, false, false> : path_kernel<L, true, W, true, false, false, true, E, false, false>;
    }
    if (p.lights && p.lightMode == 2)
        return cam ? path_kernel<L, true, W, true, true, true, false, E, false, false> : path_kernel<L, true, W, true, false, true, false, E, false, false>;
    if (p.lights)
        return cam ? path_kernel<L, true, W, true, true, false, false, E, false, false> : path_kernel<L, true, W, true, false, false, false, E, false, false>;
    if constexpr (E) {
        if (cam) return path_kernel<L, true, W, false, true, false, false, true, false, false>;
    }
    return path_kernel<L, true, W, false, false, false, false, E, false, false>;
}

PathFn path_fn(const PathParams &p) {
    QueryParams q = p.q;
    if (p.lights || p.env) q.full = 1;
    return for_scene_layout(q, [&p](auto lds, auto full, auto wide) -> PathFn {
        constexpr bool L = decltype(lds)::value, F = decltype(full)::value, W = decltype(wide)::value;
        if constexpr (F) return p.env ? general_path_fn<L, W, true>(p) : general_path_fn<L, W, false>(p);
        return path_kernel<L, F, W, false, false, false, false, false, false, false>;
    });
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
    if (!q.shade || !p.mats || p.maxDepth < 1) return hipErrorInvalidValue;
    if (p.lights ? (!q.full || p.numLights < 1 || p.lightMode < 1 || p.lightMode > 2) : (p.scratch != nullptr && !p.env))
        return hipErrorInvalidValue;
    if (p.env ? (p.envSize < 1 || p.envSize > env::kMaxSize || reinterpret_cast<uintptr_t>(p.env) % 16) : p.envSize != 0)
        return hipErrorInvalidValue;
    if (p.lightCdf ? (!p.lights || !p.lightIp) : p.lightIp != nullptr) return hipErrorInvalidValue;
    // environment sampling: the map, a light-sampling mode, and an empty light list where the scene has none
    if (p.envRowC ? (!p.env || !p.envTexels || p.lightMode < 1 || p.lightMode > 2 || (p.lights ? p.numLights < 1 : p.numLights != 0))
                  : p.envTexels != nullptr)
        return hipErrorInvalidValue;
    // a render batch's counters; a query's own pointers: rays and records are read and stored whole
    if (p.scratch ? !p.stats
                  : (!q.rays || !p.seeds || !p.radiance || reinterpret_cast<uintptr_t>(q.rays) % 16 ||
                     reinterpret_cast<uintptr_t>(p.radiance) % 16))
        return hipErrorInvalidValue;
    return launch_ray_kernel(path_fn(p), q, p, blocks, s);
}

int path_blocks_per_cu(const PathParams &p) { return ray_kernel_blocks_per_cu(path_fn(p), p.q); }

hipError_t launch_camera_rays(const CameraRaysParams &p, hipStream_t s) {
    if ((!p.rays && !p.seeds) || p.numRays == 0 || p.numRays > (1u << 31) || reinterpret_cast<uintptr_t>(p.rays) % 16)
        return hipErrorInvalidValue;
    const unsigned blocks = (p.numRays + unsigned(kCameraRaysBlock) - 1u) / unsigned(kCameraRaysBlock);
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(kCameraRaysBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace hippt
