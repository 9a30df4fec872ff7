// hippt_api.cpp — C ABI of libhippt.so (include/hippt.h).
//
// Owns all device state, like the reference's single global CudaState
// (CudaPathTracerKernel.cu:12-21), but:
//   * one context per device, each rendering a contiguous row band of the image
//     (multi-GPU; no collective — bands are gathered on the host);
//   * every entry point is serialised by a mutex (the reference is called from the GUI
//     thread and the QSG render thread without a lock, RayTracerFboItem.cpp:261,521,529);
//   * triangle-mesh scenes with a host-built SAH BVH in addition to the reference's
//     built-in 4-sphere scene.
// What a render batch or a ray query launches with (tree width, LDS residency, stack, node format,
// camera pool, top of the tree, loop exits, claim size) is decided in hippt_plan.h, a pure header;
// this file gathers its inputs, allocates what the plan needs and enqueues the launches.
#include "../../include/hippt.h"
#include "item_order.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "bvh_builder.h"
#include "env_io.h"
#include "mesh_io.h"
#include "hippt_chain_logic.h"
#include "hippt_denoise.h"
#include "hippt_device.h"
#include "hippt_path.h"
#include "hippt_plan.h"
#include "hippt_query.h"
#include "hippt_query_layout.h"
#include "hippt_refit.h"
#include "hippt_sky_rect.h"
#include "hippt_slab.h"
#include "hippt_wavefront.h"

struct hipptBvh {
    hippt::Bvh bvh;
    hippt::Bvh4 bvh4;
    std::vector<uint32_t> bvh4q;
};

namespace {

using hippt::CameraF;
namespace plan = hippt::plan;

using hippt::kStatSlots;
using hippt::kStatWords;
constexpr size_t kStatBytes = size_t(kStatSlots) * kStatWords * sizeof(unsigned long long);

// hippt_trace.h kQueues x kQueueStride work counters, then (its own line) the fused combine's
// chunk counter (MeshParams::combCtr)
constexpr size_t kCombCtrWord = 8 * 32;
constexpr size_t kQueueBytes = (kCombCtrWord + 32) * sizeof(unsigned);

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
};

#ifndef HIPPT_LEGACY_ZERO_COPY
#define HIPPT_LEGACY_ZERO_COPY 1
#endif
constexpr bool kLegacyZeroCopy = HIPPT_LEGACY_ZERO_COPY != 0;

// The key of a context's run-cost estimates (item order): what the estimate depends on.
struct OrderKey {
    int version = -1, width = 0, height = 0, y0 = 0, rows = 0, stride = 0, maxDepth = 0;
    unsigned tileShift = 6;  // the runs' shape (item_order.h RunLayout)
    CameraF cam{};
};

bool same_key(const OrderKey &a, const OrderKey &b) {
    if (a.version != b.version || a.width != b.width || a.height != b.height || a.y0 != b.y0 || a.rows != b.rows ||
        a.stride != b.stride || a.maxDepth != b.maxDepth || a.tileShift != b.tileShift ||
        a.cam.lens_radius != b.cam.lens_radius)
        return false;
    for (int k = 0; k < 3; ++k)
        if (a.cam.origin[k] != b.cam.origin[k] || a.cam.llc[k] != b.cam.llc[k] ||
            a.cam.horizontal[k] != b.cam.horizontal[k] || a.cam.vertical[k] != b.cam.vertical[k] ||
            a.cam.u[k] != b.cam.u[k] || a.cam.v[k] != b.cam.v[k])
            return false;
    return true;
}

// The key of a context's cached occupancy queries (resident blocks per CU of the megakernel, the
// wavefront extend kernel or the query kernel): the scene and what selects the kernel variant and
// sizes its LDS.
struct OccKey {
    int version = -1, stackDepth = 0, fmt = 0, poolWords = 0;
    unsigned topBytes = 0;
    bool ldsScene = false, full = false, spills = false;
    int variant = 0;  // ray-per-lane launches: the QueryMode, or a path kernel's route (kVariantPath ...)
    bool select = false;  // a light-sampling route's kernel with the selection table (HIPPT_OPT_LIGHT_SELECT)
    bool env = false;     // a path kernel's ENV variant (hipptSetEnvironment)
    bool envs = false;    // its ENVS variant (HIPPT_OPT_ENV_SAMPLING)
};
// The path kernel's routes as OccKey variants, after the QueryModes: plain paths, light-sampled path
// queries, the light-sampling render route.
constexpr int kVariantPath = 8, kVariantLitPath = 9, kVariantLitRender = 10, kVariantMisPath = 11, kVariantMisRender = 12;
constexpr int kVariantEnvRender = 13;  // plain paths from the camera start: the render route under an environment

bool same_key(const OccKey &a, const OccKey &b) {
    return a.version == b.version && a.stackDepth == b.stackDepth && a.fmt == b.fmt && a.poolWords == b.poolWords &&
           a.topBytes == b.topBytes && a.ldsScene == b.ldsScene && a.full == b.full && a.spills == b.spills &&
           a.variant == b.variant && a.select == b.select && a.env == b.env && a.envs == b.envs;
}

// Run costs computed on a detached host thread (HIPPT_OPT_ITEM_ORDER automatic).  The thread owns a
// reference to its job and reads only the job's copies of the tree and primitives, so scene uploads,
// renders and process exit never wait for it: a context that no longer wants the result drops its
// reference (abandon_cost_job), and no joinable std::thread is ever destroyed (a
// function-local static State destroyed at exit with a joinable thread called std::terminate).
struct CostJob {
    OrderKey key;
    hippt::Bvh4 bvh;
    std::vector<float4> tris;
    std::vector<float> cost;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    bool finished() {
        std::lock_guard<std::mutex> g(mu);
        return done;
    }
    void wait() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [this] { return done; });
    }
};

// What the ray-per-lane launches of one route (hippt_ray_loop.h) keep on a context: the resident blocks
// per CU of the route's kernel, the launch's claim counters and the 4-wide traversal's spill area.
// Allocated on first use (ensure_ray_launch), freed with the context.
struct RayLaunch {
    OccKey occKey;  // of blocksPerCu
    int blocksPerCu = 0;
    unsigned *ctr = nullptr;
    int *spill = nullptr;
    size_t spillBytes = 0;
};

struct Ctx {
    int device = 0;
    int y0 = 0, rows = 0, stride = 1;  // image rows y0, y0+stride, ... (rows of them)
    hipStream_t stream = nullptr;
    float4 *accum = nullptr;
    uint32_t *out = nullptr;
    float *scratch = nullptr;
    size_t scratchBytes = 0;
    // Megakernel batches defer their combine (running average + tonemap) into the next batch's
    // launch on this context, which does it between its paths (MeshParams::comb); the two batches'
    // per-sample radiances then live in two buffers.  Flushed (a combine launch of its own) before
    // anything reads or resets the image: sync, present, copies, reset, a non-megakernel batch.
    float *scratchAlt = nullptr;
    size_t scratchAltBytes = 0;
    hippt::CombineParams deferred{};
    hippt::HostFrame deferredHost{};  // a blocking frame's flush: the words into the host frame too
    bool hasDeferred = false;
    unsigned *queue = nullptr;
    unsigned long long *stats = nullptr;
    int sceneVersion = -1;
    float4 *nodes = nullptr, *tris = nullptr, *shade = nullptr, *mats = nullptr;
    float4 *nodes4 = nullptr;  // 4-wide BVH (same primitive order as nodes)
    float4 *nodes4q = nullptr; // the 4-wide BVH with 8-bit child boxes
    float4 *nodes4h = nullptr; // hybrid layout (float top + 8-bit nodes) for hybridTop top nodes
    float4 *nodes4f = nullptr; // the 4-wide BVH with half-precision planes (half_bvh4; on use)
    int halfVersion = -1;      // scene version of nodes4f
    int hybridTop = -1;
    // the pad the float nodes were built or last refitted with (MeshParams::padWord): written by the
    // scene upload and by every vertex update, in stream order
    float *padDev = nullptr;
    // Vertex updates (hipptUpdateVertices, hippt_refit.h): the refit's own buffers for the uploaded
    // scene, allocated at the context's first update and freed with the scene buffers
    float *rfVerts = nullptr;   // the update's vertices (host memory, or memory of another device)
    float *rfBoxes = nullptr;   // pbox, ubox2, ubox4
    int *rfLists = nullptr;     // RefitPlan list2, list4
    unsigned *rfWords = nullptr;
    bool rfUpdated = false;     // rfWords hold an update's counts
    // the queues' pixel-run order of this context's rows (HIPPT_OPT_ITEM_ORDER): run costs per key,
    // device item tables per batch size for those costs
    OrderKey orderKey;            // of runCosts
    std::vector<float> runCosts;  // per run of 64 band pixels (item_order.h run_costs)
    bool runCostsValid = false;
    struct OrderTable {
        int frames;
        unsigned *dev;
        // HIPPT_OPT_SKY_COMBINE: the table leaves out the skyRuns runs wholly outside skyRect (0: none left out)
        unsigned skyRuns = 0;
        hippt::SkyRect skyRect{};
    };
    std::vector<OrderTable> orderTables;  // most recently used first, at most kOrderTables
    struct SkyFlags {  // item_order.h sky_runs of the last rectangle asked for (ensure_order)
        bool valid = false;
        int width = 0, rows = 0, y0 = 0, stride = 0;
        unsigned tileShift = 6, count = 0;
        hippt::SkyRect rect{};
        std::vector<uint8_t> flags;
    } skyFlags;
    struct RetiredTable {
        unsigned *dev;
        hipEvent_t done;  // recorded on the stream after the last launch that may read it
    };
    std::vector<RetiredTable> retiredTables;
    std::shared_ptr<CostJob> costJob;  // automatic mode: the costs of a new key, off the render path
    int *spill = nullptr;      // 4-wide traversal: per-lane stack spill area
    size_t spillBytes = 0;
    // wavefront path-state pool (allocated on first use)
    void *wfPool = nullptr;
    unsigned wfSlots = 0;  // slots allocated
    unsigned wfWant = 0;   // slots asked for when the pool was allocated (>= wfSlots)
    unsigned *wfCtr = nullptr;
    unsigned *wfHost = nullptr;  // pinned: two snapshots of the ray-queue shard counters
    hipEvent_t wfPoll[2] = {nullptr, nullptr};
    OccKey wfOccKey;  // of wfBlocksPerCu
    int wfBlocksPerCu[2] = {0, 0};
    int cus = 0;
    OccKey occKey;  // of meshBlocksPerCu, meshBlocksPerCuChain
    int meshBlocksPerCu[2] = {0, 0};
    int meshBlocksPerCuChain = 0;  // the chained-batch kernel's
    // Chained batches (HIPPT_OPT_CHAIN; MeshParams::chain*, hippt_trace.h): the open run.  Its launches
    // share a ring of `slots` scratch slots and work-counter blocks (chainCtl, zeroed when a run
    // starts); the host posts each batch in the mailbox (chain::box_word: run, consecutive frames, batch) before
    // its launch is enqueued, and the run's last combines are a flush before anything reads or
    // resets the image (flush_deferred).  The run's integers and every decision over them (continue,
    // hold, group, post, close) are hippt_chain_logic.h's HostRun and host_* rules, which the protocol
    // model drives too; here is what is the library's own.
    struct Chain {
        hippt::chain::HostRun host;  // live, run, seq, epoch, firstFrame, step, cap, slots, the held group
        unsigned shift = 0;
        hippt::MeshParams key{};  // what every batch of the run shares (chain_same)
        long long blocks = 0;
        unsigned geomRev = 0;     // SceneHost::geomRev of the run's batches (MeshParams' pointers do not
                                  // change across hipptUpdateVertices)
        // the first held batch's parameters (host.pendN of them wait for one group launch)
        hippt::MeshParams pendP{};
        unsigned *audit = nullptr;  // the run's audit records (HIPPT_OPT_CHAIN_AUDIT), or null
    } chain;
    // HIPPT_OPT_CHAIN_AUDIT: kAuditRuns runs' records on the device (run k in slab k % kAuditRuns) and
    // the headers of the runs not yet copied to the host (State::auditWords), oldest first
    unsigned *auditDev = nullptr;
    unsigned auditNext = 0;
    struct AuditRun {
        unsigned hdr[hippt::kAuditWords];
        unsigned slab;
        bool closed;
    };
    std::vector<AuditRun> auditRuns;
    hipEvent_t chainStartEv = nullptr;  // recorded before each chained launch (chain_batch's hold test)
    hipEvent_t chainEndEv = nullptr;    // recorded after each chained launch (chain_batch's hold test)
    unsigned *chainCtl = nullptr;
    float *chainScratch = nullptr;
    size_t chainScratchBytes = 0;
    unsigned long long *chainBox = nullptr;     // pinned, coherent mailbox word
    unsigned long long *chainBoxDev = nullptr;  // its device address
    // pixel samples of chained batches (their kernels do not count them: every item is one sample)
    unsigned long long hostSamples = 0;
    long long skyCombinePixels = 0;  // HIPPT_INFO_SKY_COMBINE: this context's share of the last batch
    unsigned long long hostSegments = 0;  // segments of the samples a combine finishes (HIPPT_OPT_SKY_COMBINE)
    std::vector<EventPair> pool;                         // every timing event pair created
    std::vector<EventPair> freeEv;                       // pairs not in flight
    std::vector<std::pair<int, EventPair>> pending;      // (0 trace / 1 combine, events)
    hipEvent_t presentEv[2] = {nullptr, nullptr};        // band copy into State::present[b] done
    // Ray queries (hipptTraceRays, hipptOccluded, hipptTraceCamera): the claim counters, a spill area of
    // their own (a render's may be in use by launches queued before the query, and growing it would
    // wait for them), the staging buffers of one slice of a host-memory batch (rays in, results out),
    // and the event a call waits on.  Allocated on first use, freed with the context.
    RayLaunch qLaunch;
    void *qStage = nullptr;
    size_t qStageBytes = 0;
    hipEvent_t qDone = nullptr;
    // Light sampling (HIPPT_OPT_LIGHT_SAMPLING): the scene's light list (SceneHost::lights; a scene buffer),
    // and what the render route's launches take in place of the queries' (an asynchronous render may still
    // be in flight when a query grows qLaunch.spill): claim counters, spill area, resident blocks per CU.
    int *lights = nullptr;
    RayLaunch litLaunch;
    // Light selection (HIPPT_OPT_LIGHT_SELECT): the selection table of the scene's lights (hippt_refit.h
    // light_table_buffers; a scene buffer), built on the device when the context gets its scene and again
    // behind every vertex update's refit, so it is current in stream order whatever the option says.
    // Null for a scene without lights or with more than the table's limit (light_table_fits).
    unsigned *lightTable = nullptr;
    // Environment (hipptSetEnvironment): the context's copy of State::env, envSize x envSize texels, written
    // on the stream (upload_env); envRev: the State::envRev it holds or has queued.  Not a scene buffer: it
    // outlives the scene, and goes with the context.
    hippt::env::Texel *env = nullptr;
    int envSize = 0;
    unsigned envRev = 0;
    // Its selection table (HIPPT_OPT_ENV_SAMPLING; hippt_refit.h env_table_buffers), allocated and freed with
    // `env` and built on the stream behind every copy into it, whatever the option says.
    unsigned *envTable = nullptr;
    // Denoiser (hipptDenoise, hippt_denoise.h): one buffer of 80 bytes per pixel (the guide sample's hit
    // records, two colour buffers, the guide), allocated at first use, reused while large enough and
    // freed with the context; the stages' timing events (HIPPT_OPT_DENOISE_TIMING), created on use.
    void *dnBuf = nullptr;
    size_t dnBytes = 0;
    std::vector<hipEvent_t> dnEv;
};

struct SceneHost {
    int kind = HIPPT_SCENE_SPHERE4;
    int version = 0;
    std::vector<float4> nodes, tris, shade, mats;  // device layouts (hippt_device.h MeshParams)
    int numTris = 0, numNodes = 0, levels = 0;  // numTris: primitive records (triangles + spheres)
    std::vector<float4> nodes4;                 // 4-wide BVH (bvh_builder.h Bvh4)
    std::vector<float4> nodes4q;                // quantize_bvh4 of it
    std::vector<float4> nodes4f;                // half_bvh4 of it (device codes; built on use)
    int halfState = 0;                          // nodes4f: 0 not built, 1 built, -1 out of half range
    hippt::Bvh4 bvh4;                           // the 4-wide tree with node-index codes ...
    std::vector<uint32_t> q4;                   // ... and its 8-bit nodes (hybrid_bvh4 inputs)
    std::vector<float4> hybrid;                 // hybrid_bvh4 for hybridTop top nodes (built on use)
    int hybridTop = -1;
    int numNodes4 = 0, levels4 = 0, stackBound4 = 0;
    bool full = false;                          // spheres or non-Lambertian materials
    bool emissive = false;                      // an emissive material among them (MeshParams::full = 2)
    std::vector<int> lights;                    // leaf-order indices of the emissive primitives, ascending id
    double lookfrom[3] = {0, 0, 0}, lookat[3] = {0, 0, -1}, vup[3] = {0, 1, 0};
    double vfov = 90, aperture = 0, focus = 1;
    bool rawCamera = false;
    CameraF cam{};
    // hipptUpdateVertices: the 2-wide tree with its primitive order, both trees' level lists, what the
    // pad's maxabs starts from (the upload's extent hint and the spheres' boxes, which no update
    // changes), and the number of updates (a chained run's key)
    hippt::Bvh bvh2;
    hippt::RefitPlan plan;
    int numTriangles = 0;
    float extent = 0.0f, padSeed = 0.0f;
    float pad = 0.0f;  // the pad the host copy's node boxes carry (Bvh::pad; Ctx::padDev on upload)
    // smallest sine of the angle between a triangle's edges (min_edge_sine); 0: not known (a vertex
    // update from device memory that the host copy has not caught up with)
    float minEdgeSine = 0.0f;
    unsigned geomRev = 0;
};

struct State {
    std::mutex mu;
    bool ready = false;
    int width = 0, height = 0;
    int rowY0 = 0, rowY1 = 0;              // process rows: range [rowY0, rowY1) ...
    int rowPhase = 0, rowStride = 1;       // ... or every rowStride-th row from rowPhase
    bool deviceInterleave = true;          // devices of this process: interleaved rows (else bands)
    std::vector<int> devices;
    std::vector<Ctx> ctxs;
    unsigned *host = nullptr;  // pinned W*H ARGB frame (library-owned, as gState.hostOutput)
    size_t hostCount = 0;
    // asynchronous hand-off (hipptRenderFramesPresent / hipptLatestFrame): two pinned frames
    unsigned *present[2] = {nullptr, nullptr};
    int presentNext = 0;                 // buffer the next present call writes
    bool presentPending[2] = {false, false};
    long long presentSeq[2] = {-1, -1};  // present call number of the buffer's contents
    int presentFrames[2] = {0, 0};       // frames accumulated in that image
    long long presentCalls = 0;
    int latest = -1;                     // newest completed buffer
    SceneHost scene;
    char error[256] = {0};
    // options: those the traversal plan reads (hippt_plan.h), then the others
    plan::Knobs knobs = [] {
        plan::Knobs k;
        k.renderPad = hippt::slab::kRenderPadDefault;
        return k;
    }();
    // one batch (and one end-of-batch tail) per call up to 4K/256 spp: 2.12G samples x 12 B
    long long scratchMB = 32768;
    bool rngTable = false;  // memoized random_in_unit_sphere (HIPPT_OPT_RNG_TABLE)
    int pixelFormat = HIPPT_PIXEL_ARGB;  // output frame words (HIPPT_OPT_PIXEL_FORMAT)
    int itemOrder = -1;    // scene-hitting pixel runs first (HIPPT_OPT_ITEM_ORDER; -1: automatic)
    int pixelTile = -1;    // the item order's runs: tile columns (HIPPT_OPT_PIXEL_TILE; 0 rows, -1 automatic)
    bool chainAudit = false;            // HIPPT_OPT_CHAIN_AUDIT
    long long querySlice = 0;           // rays per staged slice of a host-memory query (HIPPT_OPT_QUERY_SLICE; 0 automatic)
    bool denoiseTiming = false;         // HIPPT_OPT_DENOISE_TIMING
    int lightSampling = 0;              // HIPPT_OPT_LIGHT_SAMPLING_MODE: 0, 1 or HIPPT_LIGHT_SAMPLING_MIS
    int activeLightSampling = 0;        // the mode of the light-sampling route if the last render took it (HIPPT_INFO_LIGHT_SAMPLING)
    int lightSelect = 0;                // HIPPT_OPT_LIGHT_SELECT: 0 uniform, HIPPT_LIGHT_SELECT_POWER
    int activeLightSelect = 0;          // as the last light-sampling render applied it (HIPPT_INFO_LIGHT_SELECT)
    int envSampling = 0;                // HIPPT_OPT_ENV_SAMPLING
    int activeEnvSampling = 0;          // whether the last render applied it (HIPPT_INFO_ENV_SAMPLING)
    // hipptSetEnvironment: the host copy (envSize x envSize texels in the device layout; empty: the sky
    // gradient), its revision (a context whose envRev differs has yet to receive it), the size the last
    // render applied (HIPPT_INFO_ENVIRONMENT), and the pinned staging buffers of uploads that may still be
    // queued on a stream: a call fills a free one (every event passed) and leaves it to its copies.
    std::vector<hippt::env::Texel> env;
    int envSize = 0;
    unsigned envRev = 0;
    int activeEnv = 0;
    struct EnvStage {
        hippt::env::Texel *ptr = nullptr;
        size_t bytes = 0;
        unsigned rev = 0;                              // the State::envRev it holds
        std::vector<std::pair<int, hipEvent_t>> busy;  // (device, event)
    };
    std::vector<EnvStage> envStages;
    long long denoiseNs[hippt::kDenoiseStages] = {};  // HIPPT_INFO_DENOISE_NS + k of the last timed hipptDenoise
    std::vector<unsigned> auditWords;   // closed runs' audit words not yet read (hipptChainAudit)
    std::vector<std::pair<int, uint32_t *>> rngTables;  // per device, built on first use
    // The big work buffers (sample scratch, chain ring, spill area) of the contexts a re-initialization
    // destroyed, kept for the new contexts of the same device: a fresh hipMalloc of a 13 GB ring took
    // up to 5.9 s and its hipFree ~0.29 s (r6ae/r6af), a stall on the first render after every resize.
    // Held for one initialization; cudaPathTracerShutdown frees them.
    struct SpareBuf {
        int device;
        void *ptr;
        size_t bytes;
    };
    std::vector<SpareBuf> spare;
    // hipptUpdateVertices: two pinned staging arrays of the scene's triangle vertices, used in turn, so
    // that an update does not wait for the copies of the one before it (only for those of the one
    // before that), and the events of the copies still reading or writing each.  hostStale: the newest
    // update's vertices (stage[staleBuf], complete once staleEv has passed; null: already) are not
    // yet in SceneHost; settle_scene brings them in before anything on the host reads it.
    struct Update {
        float *stage[2] = {nullptr, nullptr};
        size_t floats = 0;
        int next = 0;
        std::vector<std::pair<int, hipEvent_t>> busy[2];  // (device, event)
        bool hostStale = false;
        int staleBuf = 0;
        hipEvent_t staleEv = nullptr;  // one of busy[staleBuf]
    } upd;
    unsigned activeTopBytes = 0;  // of the last mesh render (hipptGetOption HIPPT_INFO_*)
    int activeBlocksPerCu = 0;
    int activeChunk = 0;     // the last megakernel batch's claim size
    int activeChainCap = 0;  // its run's chain cap (0: not chained)
    long long activeSkyPixels = 0;  // its image pixels outside the sky rectangle (HIPPT_OPT_SKY_RECT as applied; 0: off)
    int activeRenderPad = 0; // its LDS scene copy's pad exponent (HIPPT_OPT_RENDER_PAD as applied; 0: no trim)
    int activeWidth = 0;  // BVH width of the last mesh render (hipptActiveBvhWidth)
    int blocksPerCu = 0;
    // wavefront path-state slots per device: 2^27 holds a whole 1080p/64-spp step in flight (one
    // generation, no regenerate rounds; 8.6 GB of 64-byte records): blob70k 6.8 -> 7.4+ G vs 2^24
    unsigned wfSlots = 1u << 27;
    int wfSort = -1;  // wavefront coherence sort key bits (HIPPT_OPT_WAVEFRONT_SORT: 0, 3, 6; -1 automatic)
    hippt::BvhParams bvh;         // applied at the next scene upload
    // host-side timing accumulators
    double traceMs = 0, combineMs = 0;
    int traceLaunches = 0, combineLaunches = 0;
};

State &S() {
    static State s;
    return s;
}

// A kept buffer of `device` of at least `need` bytes (the smallest such), or null.
void *spare_take(int device, size_t need, size_t *bytes) {
    auto &v = S().spare;
    size_t best = v.size();
    for (size_t k = 0; k < v.size(); ++k)
        if (v[k].device == device && v[k].bytes >= need && (best == v.size() || v[k].bytes < v[best].bytes)) best = k;
    if (best == v.size()) return nullptr;
    void *p = v[best].ptr;
    *bytes = v[best].bytes;
    v.erase(v.begin() + long(best));
    return p;
}

void spare_free_all() {
    for (auto &b : S().spare) {
        (void)hipSetDevice(b.device);
        (void)hipFree(b.ptr);
    }
    S().spare.clear();
}

// hipMalloc of a big work buffer, or a kept one of the same device (spare_take); *bytes = its size,
// set only on success (a failed allocation leaves the caller's buffer empty, size 0).
hipError_t work_malloc(int device, void **p, size_t need, size_t *bytes) {
    if ((*p = spare_take(device, need, bytes)) != nullptr) return hipSuccess;
    const hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) {
        *p = nullptr;
        return e;
    }
    *bytes = need;
    return hipSuccess;
}

bool fail(const char **errorMessage, const std::string &msg) {
    State &s = S();
    std::strncpy(s.error, msg.c_str(), sizeof(s.error) - 1);
    s.error[sizeof(s.error) - 1] = '\0';
    if (errorMessage) *errorMessage = s.error;
    return false;
}

// fail() for the C ABI's exception handlers (abi_guard below; no lock held there: the guard's lock is
// gone by the time its handler runs).  An exception (std::bad_alloc from a scene
// buffer sized by caller input, ...) becomes the reference's false + message
// (CudaPathTracerKernel.cu:181-184) instead of crossing extern "C" into std::terminate.
bool fail_free(const char **errorMessage, const char *what) {
    std::lock_guard<std::mutex> g(S().mu);
    return fail(errorMessage, std::string("HIP path tracer: ") + (what ? what : "exception"));
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail(err, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// ---- the C ABI's guard ---------------------------------------------------------------------------
// Every extern "C" entry point is its argument packing plus one of these calls.  They run `body`, under
// the state's lock where `lock` says so, and turn an exception into the entry point's failure value: an
// exception must not cross the C ABI (the caller is C or Qt code).  The lock is released before the
// failure value is made (fail_free takes it again).  The failure value is one of three: false with the
// exception's message (abi_bool), a fixed value (abi_value), nothing (abi_void); the two entry points
// that leave the message and return a value of their own call abi_guard itself.
enum AbiLock { kUnlocked, kLocked };

template <class Body, class OnThrow>
auto abi_guard(AbiLock lock, Body body, OnThrow onThrow) -> decltype(body()) {
    try {
        std::unique_lock<std::mutex> g(S().mu, std::defer_lock);
        if (lock == kLocked) g.lock();
        return body();
    } catch (const std::exception &e) {
        return onThrow(e.what());
    } catch (...) {
        return onThrow("unknown exception");
    }
}
// false and the exception's message in *err (and hipptLastError)
template <class Body>
bool abi_bool(AbiLock lock, const char **err, Body body) {
    return abi_guard(lock, body, [err](const char *what) { return fail_free(err, what); });
}
// a fixed value
template <class R, class Body>
R abi_value(AbiLock lock, R fallback, Body body) {
    return abi_guard(lock, body, [fallback](const char *) { return fallback; });
}
// nothing
template <class Body>
void abi_void(AbiLock lock, Body body) {
    abi_guard(lock, body, [](const char *) {});
}

// ---- fp32 helpers with the oracle's contract (explicit fma only) ---------------------------
inline float fdot(const float *a, const float *b) { return std::fmaf(a[0], b[0], std::fmaf(a[1], b[1], a[2] * b[2])); }
inline void fcross(const float *a, const float *b, float *o) {
    o[0] = std::fmaf(a[1], b[2], -(a[2] * b[1]));
    o[1] = std::fmaf(a[2], b[0], -(a[0] * b[2]));
    o[2] = std::fmaf(a[0], b[1], -(a[1] * b[0]));
}
inline float as_float(int v) {
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}

// RayTracer.h Camera::Camera (:545-561), FP64, stored FP32.
void build_camera(const double lookfrom[3], const double lookat[3], const double vup[3], double vfov,
                  double aspect, double aperture, double focus, CameraF &out) {
    const double pi = 3.1415926535897932385;
    const double theta = vfov * pi / 180.0;
    const double h = std::tan(theta / 2);
    const double vh = 2.0 * h, vw = aspect * vh;
    auto unit = [](const double a[3], double o[3]) {
        const double len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double inv = 1.0 / len;
        o[0] = inv * a[0];
        o[1] = inv * a[1];
        o[2] = inv * a[2];
    };
    auto cross = [](const double a[3], const double b[3], double o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double wv[3] = {lookfrom[0] - lookat[0], lookfrom[1] - lookat[1], lookfrom[2] - lookat[2]};
    double w[3], u[3], v[3], c[3];
    unit(wv, w);
    cross(vup, w, c);
    unit(c, u);
    cross(w, u, v);
    for (int i = 0; i < 3; ++i) {
        const double hor = (focus * vw) * u[i];
        const double ver = (focus * vh) * v[i];
        const double llc = ((lookfrom[i] - 0.5 * hor) - 0.5 * ver) - focus * w[i];
        out.origin[i] = float(lookfrom[i]);
        out.llc[i] = float(llc);
        out.horizontal[i] = float(hor);
        out.vertical[i] = float(ver);
        out.u[i] = float(u[i]);
        out.v[i] = float(v[i]);
    }
    out.lens_radius = float(aperture / 2);
    out.reserved = 0.0f;
}

// The held batches of the open chain run (Ctx::chain.host.pendN) launched now as one group: before
// anything frees or replaces a buffer their parameters (Ctx::chain.pendP) point at — scene buffers,
// node layouts, item tables, the spill area (a held group launched after the free read
// freed memory).  The run stays open (chain::host_launch_held).
bool launch_held(Ctx &c, const char **err);

// Item tables no launch reads any more are freed; with `all`, after waiting for the stream.
void free_retired_tables(Ctx &c, bool all) {
    size_t k = 0;
    for (auto &t : c.retiredTables) {
        if (all || hipEventQuery(t.done) == hipSuccess) {
            if (all) (void)hipEventSynchronize(t.done);
            (void)hipFree(t.dev);
            (void)hipEventDestroy(t.done);
        } else {
            c.retiredTables[k++] = t;
        }
    }
    c.retiredTables.resize(k);
}

// A table the queued launches may still read: freed once the stream has passed this point.
void retire_table(Ctx &c, unsigned *dev) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess ||
        hipEventRecord(e, c.stream) != hipSuccess) {
        if (e) (void)hipEventDestroy(e);
        (void)hipStreamSynchronize(c.stream);
        (void)hipFree(dev);
        return;
    }
    c.retiredTables.push_back({dev, e});
}

// The context stops waiting for its cost job; the detached thread finishes on its own reference.
void abandon_cost_job(Ctx &c) { c.costJob.reset(); }

// Forgets the run costs and every item table (scene buffers freed, context destroyed).
void drop_order(Ctx &c) {
    abandon_cost_job(c);
    for (auto &t : c.orderTables) retire_table(c, t.dev);
    c.orderTables.clear();
    c.orderKey = OrderKey{};
    c.runCostsValid = false;
}

void free_scene_buffers(Ctx &c) {
    (void)hipFree(c.nodes);
    (void)hipFree(c.tris);
    (void)hipFree(c.shade);
    (void)hipFree(c.mats);
    (void)hipFree(c.nodes4);
    (void)hipFree(c.nodes4q);
    (void)hipFree(c.nodes4h);
    (void)hipFree(c.nodes4f);
    (void)hipFree(c.padDev);
    (void)hipFree(c.lights);
    (void)hipFree(c.lightTable);
    c.padDev = nullptr;
    c.lights = nullptr;
    c.lightTable = nullptr;
    c.nodes = c.tris = c.shade = c.mats = c.nodes4 = c.nodes4q = c.nodes4h = c.nodes4f = nullptr;
    (void)hipFree(c.rfVerts);
    (void)hipFree(c.rfBoxes);
    (void)hipFree(c.rfLists);
    (void)hipFree(c.rfWords);
    c.rfVerts = c.rfBoxes = nullptr;
    c.rfLists = nullptr;
    c.rfWords = nullptr;
    c.rfUpdated = false;
    c.halfVersion = -1;
    c.hybridTop = -1;
    drop_order(c);
    c.sceneVersion = -1;
}

void harvest_audit(Ctx &c);
void env_stages_release();

// Waits for the copies that still read or write staging array b (State::Update) and forgets them.
void stage_wait(int b) {
    State::Update &u = S().upd;
    for (auto &de : u.busy[b]) {
        (void)hipSetDevice(de.first);
        (void)hipEventSynchronize(de.second);
        (void)hipEventDestroy(de.second);
        if (u.staleEv == de.second) u.staleEv = nullptr;
    }
    u.busy[b].clear();
}

// A triangle's primitive record (3 words of SceneHost::tris) and shading normal, as the oracle's
// po_tri_setup: e1 = v1-v0, e2 = v2-v0, n = cross/len; the zero record when !(len > 0).  The material
// word (shade.w) is the caller's.  hippt_refit.hip's primitive pass restates this operation by operation.
void tri_record(const float *v, int id, float4 *rec, float4 &shade) {
    float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
    float e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
    float cr[3], n[3];
    fcross(e1, e2, cr);
    const float len = std::sqrt(fdot(cr, cr));
    if (!(len > 0.0f)) {
        e1[0] = e1[1] = e1[2] = 0.0f;
        e2[0] = e2[1] = e2[2] = 0.0f;
        n[0] = n[1] = n[2] = 0.0f;
    } else {
        const float inv = 1.0f / len;
        for (int a = 0; a < 3; ++a) n[a] = cr[a] * inv;
    }
    rec[0] = float4{v[0], v[1], v[2], e1[0]};
    rec[1] = float4{e1[1], e1[2], e2[0], e2[1]};
    rec[2] = float4{e2[2], as_float(id), 0.0f, 0.0f};
    shade = float4{n[0], n[1], n[2], shade.w};
}

// Primitive boxes as build_bvh_boxes takes them: triangles from verts, then the spheres.
void triangle_boxes(const float *verts, int numTris, float *boxes) {
    for (int i = 0; i < numTris; ++i) {
        const float *v = verts + 9 * size_t(i);
        float *bx = boxes + 6 * size_t(i);
        for (int a = 0; a < 3; ++a) {
            bx[a] = std::min(v[a], std::min(v[3 + a], v[6 + a]));
            bx[3 + a] = std::max(v[a], std::max(v[3 + a], v[6 + a]));
        }
    }
}
void sphere_box(const float *q, float *bx) {
    // slack for the FP32 root's error near the box faces (pt_oracle.c po_scene_create2)
    const float r = std::fabs(q[3]) * (1.0f + 1.0f / 4096.0f);
    for (int a = 0; a < 3; ++a) {
        bx[a] = q[a] - r;
        bx[3 + a] = q[a] + r;
    }
}

// Smallest sine of the angle between the two edges e1, e2 of any non-degenerate triangle of `verts`
// (numTris * 9 floats): what the render pad's bound depends on (the error of an
// accepted Möller–Trumbore hit's t grows with 1 / sin).  1 for no triangles.
float min_edge_sine(const float *verts, int numTris) {
    double m = 1.0;
    for (int i = 0; i < numTris; ++i) {
        const float *v = verts + 9 * size_t(i);
        const double a[3] = {double(v[3]) - v[0], double(v[4]) - v[1], double(v[5]) - v[2]};
        const double b[3] = {double(v[6]) - v[0], double(v[7]) - v[1], double(v[8]) - v[2]};
        const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
        const double ab = (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
        if (!(cc > 0.0) || !std::isfinite(ab)) continue;  // degenerate or dropped: no ray hits it
        m = std::min(m, std::sqrt(cc / ab));
    }
    return float(m);
}

// SceneHost refitted to `verts` (numTriangles * 9 floats) as the device refit does it: a triangle with
// a non-finite coordinate becomes the zero record without a box (the host-memory path of
// hipptUpdateVertices has rejected those before).
void refit_scene_host(SceneHost &sc, const float *verts) {
    const int numPrims = sc.numTris, nt = sc.numTriangles;
    std::vector<float> boxes(size_t(numPrims) * 6);
    triangle_boxes(verts, nt, boxes.data());
    std::vector<char> dropped(size_t(nt), 0);
    for (int i = 0; i < nt; ++i) {
        bool finite = true;
        for (int j = 0; j < 9; ++j) finite = finite && std::isfinite(verts[9 * size_t(i) + j]);
        if (finite) continue;
        dropped[size_t(i)] = 1;
        for (int a = 0; a < 3; ++a) {
            boxes[6 * size_t(i) + a] = INFINITY;
            boxes[6 * size_t(i) + 3 + a] = -INFINITY;
        }
    }
    for (int k = 0; k < numPrims; ++k) {
        const int id = sc.bvh2.order[size_t(k)];
        float4 *rec = &sc.tris[3 * size_t(k)];
        if (id >= nt) {
            const float q[4] = {rec[0].x, rec[0].y, rec[0].z, rec[0].w};
            sphere_box(q, &boxes[6 * size_t(id)]);
        } else if (dropped[size_t(id)]) {
            rec[0] = rec[1] = float4{};
            rec[2] = float4{0.0f, as_float(id), 0.0f, 0.0f};
            sc.shade[size_t(k)] = float4{0.0f, 0.0f, 0.0f, sc.shade[size_t(k)].w};
        } else {
            tri_record(verts + 9 * size_t(id), id, rec, sc.shade[size_t(k)]);
        }
    }
    std::string msg;
    if (!hippt::refit_bvh(sc.bvh2, sc.bvh4, boxes.data(), numPrims, sc.extent, msg, &sc.plan))
        throw std::runtime_error("vertex update: " + msg);  // (sizes and values were checked: not reached)
    sc.pad = sc.bvh2.pad;
    sc.minEdgeSine = min_edge_sine(verts, nt);
    std::memcpy(sc.nodes.data(), sc.bvh2.nodes.data(), sc.bvh2.nodes.size() * sizeof(uint32_t));
    auto *w4 = reinterpret_cast<uint32_t *>(sc.nodes4.data());
    for (size_t k = 0; k < size_t(sc.numNodes4); ++k)  // the boxes; the device layout keeps its byte codes
        std::memcpy(w4 + k * hippt::kNode4Words, &sc.bvh4.nodes[k * hippt::kNode4Words], 24 * sizeof(uint32_t));
}

// After an update the 8-bit, half and hybrid trees are stale: dropped, so that every path reads the
// refitted float nodes (the kernels' own fallback for a scene without an 8-bit tree; same results).
// A fresh hipptUploadScene builds them again.
void drop_derived_trees(SceneHost &sc) {
    sc.nodes4q.clear();
    sc.q4.clear();
    sc.nodes4f.clear();
    sc.halfState = -1;
    sc.hybrid.clear();
    sc.hybridTop = -1;
}

// Brings the newest update's vertices into SceneHost before the host reads it (a new context's
// upload, the run-cost estimate, the wavefront sort's scene box).
void settle_scene() {
    State &s = S();
    State::Update &u = s.upd;
    if (!u.hostStale) return;
    if (u.staleEv) {
        for (auto &de : u.busy[u.staleBuf])
            if (de.second == u.staleEv) (void)hipSetDevice(de.first);
        (void)hipEventSynchronize(u.staleEv);  // the device-to-host copy of a HIPPT_VERTS_DEVICE update
        u.staleEv = nullptr;
    }
    u.hostStale = false;
    refit_scene_host(s.scene, u.stage[u.staleBuf]);
}

// keep: the big work buffers go to State::spare (a re-initialization) instead of hipFree.
void destroy_ctx(Ctx &c, bool keep) {
    (void)hipSetDevice(c.device);
    if (c.stream) (void)hipStreamSynchronize(c.stream);  // (so no queued launch reads a kept buffer)
    auto drop = [&](void *p, size_t bytes) {
        if (!p) return;
        if (keep && bytes) S().spare.push_back({c.device, p, bytes});
        else (void)hipFree(p);
    };
    harvest_audit(c);  // closed runs' records; an open run's (its image discarded) are dropped
    (void)hipFree(c.auditDev);
    (void)hipFree(c.accum);
    (void)hipFree(c.out);
    drop(c.scratch, c.scratchBytes);
    drop(c.scratchAlt, c.scratchAltBytes);
    c.scratchAlt = nullptr;
    c.scratchAltBytes = 0;
    c.hasDeferred = false;
    (void)hipFree(c.queue);
    (void)hipFree(c.chainCtl);
    drop(c.chainScratch, c.chainScratchBytes);
    if (c.chainBox) (void)hipHostFree(c.chainBox);
    if (c.chainStartEv) (void)hipEventDestroy(c.chainStartEv);
    if (c.chainEndEv) (void)hipEventDestroy(c.chainEndEv);
    (void)hipFree(c.stats);
    (void)hipFree(c.wfPool);
    (void)hipFree(c.wfCtr);
    drop(c.spill, c.spillBytes);
    c.spill = nullptr;
    c.spillBytes = 0;
    for (RayLaunch *r : {&c.qLaunch, &c.litLaunch}) {
        (void)hipFree(r->ctr);
        (void)hipFree(r->spill);
    }
    (void)hipFree(c.qStage);
    if (c.qDone) (void)hipEventDestroy(c.qDone);
    (void)hipFree(c.dnBuf);
    (void)hipFree(c.env);
    (void)hipFree(c.envTable);
    for (hipEvent_t e : c.dnEv) (void)hipEventDestroy(e);
    (void)hipHostFree(c.wfHost);
    for (hipEvent_t e : c.wfPoll)
        if (e) (void)hipEventDestroy(e);
    free_scene_buffers(c);
    free_retired_tables(c, true);
    for (auto &e : c.pool) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    for (hipEvent_t e : c.presentEv)
        if (e) (void)hipEventDestroy(e);
    if (c.stream) (void)hipStreamDestroy(c.stream);
    c = Ctx();
}

// keep: a re-initialization (init_inner) keeps the contexts' big work buffers for the new ones.
void destroy_all(bool keep = false) {
    State &s = S();
    if (!keep) spare_free_all();
    for (auto &c : s.ctxs) destroy_ctx(c, keep);
    s.ctxs.clear();
    for (auto &t : s.rngTables) {
        (void)hipSetDevice(t.first);
        (void)hipFree(t.second);
    }
    s.rngTables.clear();
    stage_wait(0);  // (the contexts' streams are finished: these return at once)
    stage_wait(1);
    env_stages_release();
    if (!keep) {
        settle_scene();
        for (float *&p : s.upd.stage) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
        }
        s.upd.floats = 0;
    }
    if (s.host) (void)hipHostFree(s.host);
    s.host = nullptr;
    s.hostCount = 0;
    for (int b = 0; b < 2; ++b) {
        if (s.present[b]) (void)hipHostFree(s.present[b]);
        s.present[b] = nullptr;
        s.presentPending[b] = false;
        s.presentSeq[b] = -1;
    }
    s.presentNext = 0;
    s.latest = -1;
    s.ready = false;
}

bool next_events(Ctx &c, EventPair &ev, const char **err) {
    if (c.freeEv.empty()) {
        EventPair e;
        HIP_TRY(hipEventCreate(&e.a));
        HIP_TRY(hipEventCreate(&e.b));
        c.pool.push_back(e);
        c.freeEv.push_back(e);
    }
    ev = c.freeEv.back();
    c.freeEv.pop_back();
    return true;
}

// One launch on c.stream between a pair of timing events, to be accounted as `kind` (0 trace / 1 combine)
// once it has finished.  `what`: the launch's expression, for the failure text (as HIP_TRY's).
template <class F>
bool timed_launch(Ctx &c, int kind, const char *what, const char **err, F launch) {
    EventPair ev;
    if (!next_events(c, ev, err)) return false;
    HIP_TRY(hipEventRecord(ev.a, c.stream));
    const hipError_t e = launch();
    if (e != hipSuccess) return fail(err, std::string(what) + ": " + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(ev.b, c.stream));
    c.pending.push_back({kind, ev});
    return true;
}
#define TIMED_LAUNCH(c, kind, expr) timed_launch(c, kind, #expr, err, [&] { return (expr); })

// Blocks of a persistent launch of kMeshBlock threads over `items` items: what is resident at
// blocksPerCu blocks per CU, no more than the items fill, at least one.
long long ray_blocks(const Ctx &c, int blocksPerCu, long long items) {
    return std::max(1LL, std::min<long long>((long long)c.cus * blocksPerCu, (items + hippt::kMeshBlock - 1) / hippt::kMeshBlock));
}

// Adds a finished launch's event time to the stats and recycles its events.
bool account(const std::pair<int, EventPair> &pe, Ctx &c, const char **err) {
    State &s = S();
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, pe.second.a, pe.second.b));
    if (pe.first == 0) {
        s.traceMs += ms;
        ++s.traceLaunches;
    } else {
        s.combineMs += ms;
        ++s.combineLaunches;
    }
    c.freeEv.push_back(pe.second);
    return true;
}

// Non-blocking: accounts the launches (in stream order) that have already finished.
bool harvest_locked(Ctx &c, const char **err) {
    size_t done = 0;
    while (done < c.pending.size() && hipEventQuery(c.pending[done].second.b) == hipSuccess) {
        if (!account(c.pending[done], c, err)) return false;
        ++done;
    }
    c.pending.erase(c.pending.begin(), c.pending.begin() + long(done));
    return true;
}

// Enqueues a build of c's light selection table from its scene buffers as they are at that point of the stream.
bool enqueue_light_table(Ctx &c, const char **err) {
    const SceneHost &sc = S().scene;
    if (!c.lightTable) return true;
    hippt::LightTableBuffers t = hippt::light_table_buffers(c.lightTable, int(sc.lights.size()), sc.numTris);
    t.tris = c.tris;
    t.shade = c.shade;
    t.mats = c.mats;
    t.lights = c.lights;
    HIP_TRY(hippt::launch_light_table(t, c.stream));
    return true;
}

bool ensure_scene(Ctx &c, const char **err) {
    State &s = S();
    if (s.scene.kind != HIPPT_SCENE_MESH || c.sceneVersion == s.scene.version) return true;
    settle_scene();  // (a vertex update not yet in the host copy)
    if (!launch_held(c, err)) return false;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamSynchronize(c.stream));  // queued launches read the old buffers
    free_scene_buffers(c);
    auto up = [&](float4 *&dst, const std::vector<float4> &src) -> bool {
        HIP_TRY(hipMalloc(&dst, std::max<size_t>(16, src.size() * sizeof(float4))));
        if (!src.empty()) HIP_TRY(hipMemcpy(dst, src.data(), src.size() * sizeof(float4), hipMemcpyHostToDevice));
        return true;
    };
    if (!up(c.nodes, s.scene.nodes) || !up(c.tris, s.scene.tris) || !up(c.shade, s.scene.shade) ||
        !up(c.mats, s.scene.mats) || !up(c.nodes4, s.scene.nodes4) || !up(c.nodes4q, s.scene.nodes4q))
        return false;
    HIP_TRY(hipMalloc(&c.padDev, 16));
    HIP_TRY(hipMemcpy(c.padDev, &s.scene.pad, sizeof(float), hipMemcpyHostToDevice));
    if (!s.scene.lights.empty()) {
        HIP_TRY(hipMalloc(&c.lights, s.scene.lights.size() * sizeof(int)));
        HIP_TRY(hipMemcpy(c.lights, s.scene.lights.data(), s.scene.lights.size() * sizeof(int), hipMemcpyHostToDevice));
        if (hippt::light_table_fits(s.scene.lights.size())) {
            const size_t bytes = hippt::light_table_words(s.scene.lights.size(), size_t(s.scene.numTris)) * sizeof(unsigned);
            HIP_TRY(hipMalloc(&c.lightTable, bytes));
            // (ip of the primitives that are no lights: 0 for good; on the stream, ahead of the build)
            HIP_TRY(hipMemsetAsync(c.lightTable, 0, bytes, c.stream));
            if (!enqueue_light_table(c, err)) return false;
        }
    }
    c.sceneVersion = s.scene.version;
    return true;
}

// The preconditions of the render pad's bound, without which the LDS scene copy keeps
// the builder's pad: every ray origin within the M the pad was sized from (the camera's origin, lens
// included; hipptSetCamera may have moved it since the upload), and no triangle whose edges meet at
// a sine below kRenderPadMinSine.  M: the host copy's pad * 2^16, or, while a vertex update is not in
// the host copy yet, its lower bound padSeed (no update lowers it; the device's M is at least that).
constexpr float kRenderPadMinSine = 0.3f;
bool render_pad_holds(const SceneHost &sc, bool hostStale, const CameraF &cam) {
    const float M = hostStale ? sc.padSeed : std::max(sc.padSeed, sc.pad * 65536.0f);
    float o = 0.0f;
    for (int k = 0; k < 3; ++k) o = std::max(o, std::fabs(cam.origin[k]));
    const float reach = o + 1.5f * std::fabs(cam.lens_radius);  // (a lens offset's component: at most sqrt(2) radii)
    return std::isfinite(reach) && reach <= M && sc.minEdgeSine >= kRenderPadMinSine;
}

// The sky rectangle of a batch (HIPPT_OPT_SKY_RECT; hippt_sky_rect.h): from the camera
// the kernel gets and the host tree's root box (the 2-wide root's child boxes, as the builder or the
// last host refit padded them; every 4-wide box lies inside).  The whole image when the bound does not
// apply.  The caller leaves it off while a vertex update is not in the host copy yet.
hippt::skyrect::Rect sky_rect_of(const SceneHost &sc, const CameraF &cam, int width, int height) {
    const hippt::skyrect::Rect all = hippt::skyrect::whole(width, height);
    if (sc.bvh2.nodes.size() < size_t(hippt::kNodeWords)) return all;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool any = false;
    for (int slot = 0; slot < 2; ++slot) {
        if (int32_t(sc.bvh2.nodes[size_t(hippt::node_code_word(2, slot))]) == hippt::leaf_code(0, 0)) continue;
        any = true;
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], as_float(int(sc.bvh2.nodes[size_t(hippt::node_lo_word(2, slot, a))])));
            hi[a] = std::max(hi[a], as_float(int(sc.bvh2.nodes[size_t(hippt::node_hi_word(2, slot, a))])));
        }
    }
    if (!any) return all;
    return hippt::skyrect::sky_rect(cam, width, height, lo, hi, sc.pad, sc.numTris);
}

// The queues' item table of a context's rows (item_order.h) for a batch of `frames` frames: run cost
// estimates per key (scene, camera, image, rows, depth), tables per batch size (kOrderTables of
// them, so a call's full batches and its remainder batch both stay cached).  With `forced`
// (HIPPT_OPT_ITEM_ORDER 1) new costs are computed here, on all host threads.  In automatic mode they
// are computed on a host thread of their own, and the batches queued meanwhile run in image order
// (*table = nullptr: the same results), so moving the camera never stalls a frame on
// the estimate (0.34 s single-threaded at 1080p).  A replaced table is freed once the launches
// that read it are done (an event, not a stream synchronisation).
constexpr size_t kOrderTables = 4;

int cost_threads() { return int(std::max(1u, std::min(16u, std::thread::hardware_concurrency()))); }

// skyOmit (HIPPT_OPT_SKY_COMBINE): the batch's sky rectangle when its table is to leave out the runs
// wholly outside it; *skyRuns: how many runs per frame the table left out (0: none, the mode is off).
bool ensure_order(Ctx &c, const CameraF &cam, int frames, int maxDepth, bool forced, unsigned tileShift,
                  const unsigned **table, const char **err, const hippt::SkyRect *skyOmit = nullptr,
                  unsigned *skyRuns = nullptr) {
    if (skyRuns) *skyRuns = 0;
    State &s = S();
    *table = nullptr;
    OrderKey key;
    key.tileShift = hippt::tile_shift_for(unsigned(s.width), tileShift);
    key.version = s.scene.version;
    key.width = s.width;
    key.height = s.height;
    key.y0 = c.y0;
    key.rows = c.rows;
    key.stride = c.stride;
    key.maxDepth = maxDepth;
    key.cam = cam;
    HIP_TRY(hipSetDevice(c.device));
    free_retired_tables(c, false);
    if (!c.runCostsValid || !same_key(key, c.orderKey)) {
        std::vector<float> cost;
        const bool jobForKey = c.costJob && same_key(c.costJob->key, key);
        if (jobForKey && (forced || c.costJob->finished())) {
            // forced mode takes the in-flight job's estimate for this key rather than computing it
            // again
            c.costJob->wait();
            cost = std::move(c.costJob->cost);
            c.costJob.reset();
        } else if (forced) {
            abandon_cost_job(c);  // a stale key's job: not joined on the render path
            settle_scene();
            hippt::run_costs(s.scene.bvh4, reinterpret_cast<const float *>(s.scene.tris.data()), cam,
                             hippt::RunLayout{unsigned(s.width), unsigned(c.rows), key.tileShift}, s.height, c.y0,
                             c.stride, maxDepth, cost, cost_threads());
        } else {
            if (c.costJob && !jobForKey) abandon_cost_job(c);
            if (!c.costJob) {
                auto job = std::make_shared<CostJob>();
                settle_scene();
                job->key = key;
                job->bvh = s.scene.bvh4;
                job->tris = s.scene.tris;
                const int nt = std::max(1, cost_threads() / 2);
                try {
                    std::thread([job, nt] {
                        // an exception must not leave the thread (std::terminate): no estimate then,
                        // and this key's batches stay in image order
                        try {
                            hippt::run_costs(job->bvh, reinterpret_cast<const float *>(job->tris.data()),
                                             job->key.cam,
                                             hippt::RunLayout{unsigned(job->key.width), unsigned(job->key.rows),
                                                              job->key.tileShift},
                                             job->key.height, job->key.y0, job->key.stride, job->key.maxDepth,
                                             job->cost, nt);
                        } catch (...) {
                            job->cost.clear();
                        }
                        {
                            std::lock_guard<std::mutex> g(job->mu);
                            job->done = true;
                        }
                        job->cv.notify_all();
                    }).detach();
                    c.costJob = std::move(job);
                } catch (const std::system_error &) {
                    // no thread to be had: this batch in image order, the next one tries again
                }
            }
            return true;  // this batch in image order
        }
        if (!launch_held(c, err)) return false;
        for (auto &t : c.orderTables) retire_table(c, t.dev);
        c.orderTables.clear();
        c.runCosts = std::move(cost);
        c.orderKey = key;
        c.runCostsValid = true;
    }
    if (c.runCosts.empty()) return true;  // no estimate for this key (its job failed): image order
    const hippt::RunLayout layout{unsigned(s.width), unsigned(c.rows), c.orderKey.tileShift};
    // the runs' flags for this rectangle: kept with their key (the cost key's layout and rows, and the rectangle),
    // so that a batch whose table is cached pays a comparison, not a pass over the runs
    if (skyOmit) {
        Ctx::SkyFlags &f = c.skyFlags;
        const bool same = f.valid && f.width == s.width && f.rows == c.rows && f.y0 == c.y0 && f.stride == c.stride &&
                          f.tileShift == layout.tileShift && f.rect.x0 == skyOmit->x0 && f.rect.y0 == skyOmit->y0 &&
                          f.rect.x1 == skyOmit->x1 && f.rect.y1 == skyOmit->y1;
        if (!same) {
            f.count = unsigned(hippt::sky_runs(layout, c.y0, c.stride,
                                               hippt::skyrect::Rect{skyOmit->x0, skyOmit->y0, skyOmit->x1, skyOmit->y1},
                                               f.flags));
            f.width = s.width, f.rows = c.rows, f.y0 = c.y0, f.stride = c.stride, f.tileShift = layout.tileShift;
            f.rect = *skyOmit;
            f.valid = true;
        }
    }
    const std::vector<uint8_t> &sky = c.skyFlags.flags;
    unsigned omitted = skyOmit ? c.skyFlags.count : 0u;
    if (omitted >= c.runCosts.size()) omitted = 0;  // (nothing left to trace: the table keeps every run)
    auto same_omit = [&](const Ctx::OrderTable &t) {
        return t.skyRuns == omitted &&
               (!omitted || (t.skyRect.x0 == skyOmit->x0 && t.skyRect.y0 == skyOmit->y0 && t.skyRect.x1 == skyOmit->x1 &&
                             t.skyRect.y1 == skyOmit->y1));
    };
    if (skyRuns) *skyRuns = omitted;
    for (size_t k = 0; k < c.orderTables.size(); ++k)
        if (c.orderTables[k].frames == frames && same_omit(c.orderTables[k])) {
            std::rotate(c.orderTables.begin(), c.orderTables.begin() + k, c.orderTables.begin() + k + 1);
            *table = c.orderTables.front().dev;
            return true;
        }
    std::vector<uint32_t> order;
    hippt::build_item_table(c.runCosts, layout, unsigned(frames), hippt::kMeshQueues, order, omitted ? &sky : nullptr);
    unsigned *dev = nullptr;
    HIP_TRY(hipMalloc(&dev, std::max<size_t>(1, order.size()) * sizeof(unsigned)));
    // a fresh buffer: the copy need not wait for the launches queued on the context's stream
    if (!order.empty() && hipMemcpy(dev, order.data(), order.size() * sizeof(unsigned), hipMemcpyHostToDevice) !=
                              hipSuccess) {
        (void)hipFree(dev);
        return fail(err, "HIP path tracer: item table upload failed");
    }
    if (c.orderTables.size() >= kOrderTables) {
        if (!launch_held(c, err)) return false;
        retire_table(c, c.orderTables.back().dev);
        c.orderTables.pop_back();
    }
    c.orderTables.insert(c.orderTables.begin(),
                         Ctx::OrderTable{frames, dev, omitted, omitted ? *skyOmit : hippt::SkyRect{}});
    *table = dev;
    return true;
}

// The half-precision node layout (bvh_builder.h half_bvh4, HIPPT_OPT_BVH_QUANT 3): built on the host
// once per scene (half_tree_ok) and uploaded to a context's device the first time a render there
// uses it.
bool half_tree_ok(SceneHost &sc) {
    if (sc.halfState == 0) {
        std::vector<uint32_t> h;
        if (hippt::half_bvh4(reinterpret_cast<const uint32_t *>(sc.nodes4.data()), size_t(sc.numNodes4), h)) {
            sc.nodes4f.assign(h.size() / 4, float4{});
            std::memcpy(sc.nodes4f.data(), h.data(), h.size() * sizeof(uint32_t));
            sc.halfState = 1;
        } else {
            sc.halfState = -1;  // planes beyond the half range: float nodes
        }
    }
    return sc.halfState > 0;
}

bool ensure_half(Ctx &c, const char **err) {
    SceneHost &sc = S().scene;
    if (!half_tree_ok(sc)) return fail(err, "HIP path tracer: no half-precision tree for this scene");
    if (c.halfVersion == sc.version && c.nodes4f) return true;
    if (!launch_held(c, err)) return false;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamSynchronize(c.stream));
    (void)hipFree(c.nodes4f);
    c.nodes4f = nullptr;
    HIP_TRY(hipMalloc(&c.nodes4f, sc.nodes4f.size() * sizeof(float4)));
    HIP_TRY(hipMemcpy(c.nodes4f, sc.nodes4f.data(), sc.nodes4f.size() * sizeof(float4), hipMemcpyHostToDevice));
    c.halfVersion = sc.version;
    return true;
}

// The hybrid node layout (bvh_builder.h hybrid_bvh4) for `top` top-of-tree nodes: built on the
// host once per (scene, top) and uploaded to the context's device.
bool ensure_hybrid(Ctx &c, int top, const char **err) {
    State &s = S();
    SceneHost &sc = s.scene;
    if (sc.hybridTop != top) {
        std::vector<uint32_t> w;
        if (!hippt::hybrid_bvh4(sc.bvh4, sc.q4, top, w)) return fail(err, "hybrid BVH layout failed");
        sc.hybrid.assign(w.size() / 4, float4{});
        std::memcpy(sc.hybrid.data(), w.data(), w.size() * sizeof(uint32_t));
        sc.hybridTop = top;
    }
    if (c.hybridTop == top && c.nodes4h) return true;
    if (!launch_held(c, err)) return false;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamSynchronize(c.stream));
    (void)hipFree(c.nodes4h);
    c.nodes4h = nullptr;
    c.hybridTop = -1;
    HIP_TRY(hipMalloc(&c.nodes4h, sc.hybrid.size() * sizeof(float4)));
    HIP_TRY(hipMemcpy(c.nodes4h, sc.hybrid.data(), sc.hybrid.size() * sizeof(float4), hipMemcpyHostToDevice));
    c.hybridTop = top;
    return true;
}

bool init_inner(int width, int height, const char **err) {
    State &s = S();
    spare_free_all();   // the previous initialization's, none of which its contexts took again
    destroy_all(true);  // this one's, for the new contexts
    if (width <= 0 || height <= 0) return fail(err, "invalid image size");
    s.width = width;
    s.height = height;
    std::vector<int> devs = s.devices;
    if (devs.empty()) {
        int d = 0;
        HIP_TRY(hipGetDevice(&d));
        devs.push_back(d);
    }
    // this process's rows: first p0, count pn, stride ps
    int p0, pn, ps;
    if (s.rowStride > 1) {
        p0 = std::min(s.rowPhase, height);
        ps = s.rowStride;
        pn = p0 < height ? (height - p0 + ps - 1) / ps : 0;
    } else {
        p0 = std::clamp(s.rowY0, 0, height);
        pn = (s.rowY1 <= 0 ? height : std::clamp(s.rowY1, p0, height)) - p0;
        ps = 1;
    }
    const int n = int(devs.size());
    s.ctxs.resize(size_t(n));
    for (int k = 0; k < n; ++k) {
        Ctx &c = s.ctxs[size_t(k)];
        c.device = devs[size_t(k)];
        if (s.deviceInterleave && n > 1) {  // device k: every n-th of the process's rows
            c.y0 = p0 + ps * k;
            c.rows = pn > k ? (pn - k + n - 1) / n : 0;
            c.stride = ps * n;
        } else {  // device k: a contiguous run of the process's rows
            const int a = int((long long)pn * k / n), b = int((long long)pn * (k + 1) / n);
            c.y0 = p0 + ps * a;
            c.rows = b - a;
            c.stride = ps;
        }
        HIP_TRY(hipSetDevice(c.device));
        HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        const size_t px = size_t(c.rows) * size_t(width);
        HIP_TRY(hipMalloc(&c.accum, std::max<size_t>(16, px * sizeof(float4))));
        HIP_TRY(hipMalloc(&c.out, std::max<size_t>(16, px * sizeof(uint32_t))));
        HIP_TRY(hipMalloc(&c.queue, kQueueBytes));
        HIP_TRY(hipMalloc(&c.stats, kStatBytes));
        HIP_TRY(hipMemsetAsync(c.accum, 0, px * sizeof(float4), c.stream));
        HIP_TRY(hipMemsetAsync(c.out, 0, px * sizeof(uint32_t), c.stream));
        HIP_TRY(hipMemsetAsync(c.stats, 0, kStatBytes, c.stream));
        HIP_TRY(hipDeviceGetAttribute(&c.cus, hipDeviceAttributeMultiprocessorCount, c.device));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    s.hostCount = size_t(width) * size_t(height);
    // portable, mapped, coherent (fine-grained: the GPU writes go straight to host memory): every
    // context's device may write it (legacy zero-copy frames)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.host), s.hostCount * sizeof(unsigned),
                          hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(s.host, 0, s.hostCount * sizeof(unsigned));
    s.ready = true;
    return true;
}

// Cleans up on failure, as cudaPathTracerInit does (CudaPathTracerKernel.cu:202-234).
bool init_locked(int width, int height, const char **err) {
    if (init_inner(width, height, err)) return true;
    destroy_all();
    return false;
}

// 4-wide traversal of a tree whose stack bound exceeds the LDS capacity: a per-lane spill
// area of spillCap entries for every lane of a `blocks`-block persistent grid.
bool ensure_spill(Ctx &c, hippt::MeshParams &p, long long blocks, bool spills, int spillCap, const char **err) {
    if (!spills) return true;
    p.spillCap = spillCap;
    const size_t bytes = size_t(blocks) * hippt::kMeshBlock * size_t(spillCap) * sizeof(int);
    if (c.spillBytes < bytes) {
        if (!launch_held(c, err)) return false;
        HIP_TRY(hipStreamSynchronize(c.stream));
        (void)hipFree(c.spill);
        c.spill = nullptr;
        c.spillBytes = 0;
        void *p = nullptr;
        HIP_TRY(work_malloc(c.device, &p, bytes, &c.spillBytes));
        c.spill = static_cast<int *>(p);
    }
    p.spill = c.spill;
    return true;
}

// The memoized random_in_unit_sphere table of c's device (hippt_device.h launch_rng_table),
// built once per device on first use (16 GiB, a few ms) and shared by the device's contexts.
bool rng_table(Ctx &c, const uint32_t **out, const char **err) {
    State &s = S();
    for (auto &t : s.rngTables)
        if (t.first == c.device) {
            *out = t.second;
            return true;
        }
    uint32_t *t = nullptr;
    HIP_TRY(hipMalloc(&t, hippt::kRngTableBytes));
    const hipError_t e = hippt::launch_rng_table(t, c.stream);
    if (e != hipSuccess || hipStreamSynchronize(c.stream) != hipSuccess) {
        (void)hipFree(t);
        return fail(err, std::string("rng table: ") + hipGetErrorString(e));
    }
    s.rngTables.emplace_back(c.device, t);
    *out = t;
    return true;
}

// Wavefront variant (hippt_wavefront.hip): init + generate, then extend/shade/generate
// iterations until the ray queue stays empty.  The host reads the queue size with one batch of
// lag (pinned snapshot + event), so the call returns within ~16 iterations of the end.
bool run_wavefront(Ctx &c, hippt::MeshParams p, bool cnt, bool spills, int spillCap, const char **err) {
    State &s = S();
    unsigned slots = std::max(64u, std::min(s.wfSlots, std::max(64u, p.totalItems)));
    unsigned shardCap = 0;
    if (c.wfWant != slots || !c.wfPool) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        (void)hipFree(c.wfPool);
        c.wfPool = nullptr;
        c.wfSlots = c.wfWant = 0;
        const unsigned want = slots;
        // Every context owns a pool, and several contexts may share a device (hipptSetDevices
        // with a repeated id): each takes at most half the device's free memory divided by the
        // contexts on it, and a failed allocation retries with half the slots.  A smaller pool
        // only adds regenerate rounds; the image is the same.
        size_t freeB = 0, totalB = 0;
        HIP_TRY(hipMemGetInfo(&freeB, &totalB));
        int sharing = 0;
        for (const Ctx &o : s.ctxs) sharing += o.device == c.device && !o.wfPool ? 1 : 0;
        const size_t budget = freeB / 2 / size_t(std::max(1, sharing));
        while (slots > 64u && hippt::wf_pool_words(slots, &shardCap) * sizeof(uint32_t) > budget) slots >>= 1;
        for (;;) {
            const hipError_t e = hipMalloc(&c.wfPool, hippt::wf_pool_words(slots, &shardCap) * sizeof(uint32_t));
            if (e == hipSuccess) break;
            (void)hipGetLastError();  // clear the sticky allocation error
            c.wfPool = nullptr;
            if (slots <= (1u << 16)) return fail(err, std::string("wavefront pool: ") + hipGetErrorString(e));
            slots >>= 1;
        }
        c.wfSlots = slots;
        c.wfWant = want;
    }
    slots = c.wfSlots;
    (void)hippt::wf_pool_words(slots, &shardCap);
    if (!c.wfCtr) HIP_TRY(hipMalloc(&c.wfCtr, hippt::kCtrWords * sizeof(unsigned)));
    hippt::WfParams W{};
    W.mp = p;
    W.slots = slots;
    W.shardCap = shardCap;
    W.ctr = c.wfCtr;
    // the two ray queues' payload arrays (float4 each), then the hit array
    auto *base = static_cast<float4 *>(c.wfPool);
    const size_t entries = size_t(hippt::kWfShards) * shardCap;
    for (int q = 0; q < 2; ++q) {
        W.ra[q] = base + (3 * q + 0) * entries;
        W.rb[q] = base + (3 * q + 1) * entries;
        W.rc[q] = base + (3 * q + 2) * entries;
    }
    W.hit = reinterpret_cast<float2 *>(base + 6 * entries);
    // coherence sort of the scattered paths (HIPPT_OPT_WAVEFRONT_SORT; automatic: off)
    W.sortBits = unsigned(s.wfSort > 0 ? s.wfSort : 0);
    if (W.sortBits > 3) {
        // the scene box: the union of the 4-wide root's child boxes (Bvh4 words lo.x[4] hi.x[4] ...)
        settle_scene();
        const std::vector<uint32_t> &n = s.scene.bvh4.nodes;
        for (int a = 0; a < 3; ++a) {
            float lo = INFINITY, hi = -INFINITY;
            for (int i = 0; i < 4 && n.size() >= size_t(hippt::kNode4Words); ++i) {
                float l, h;
                std::memcpy(&l, &n[size_t(8 * a + i)], 4);
                std::memcpy(&h, &n[size_t(8 * a + 4 + i)], 4);
                if (l <= h) {
                    lo = std::min(lo, l);
                    hi = std::max(hi, h);
                }
            }
            const bool ok = std::isfinite(lo) && std::isfinite(hi) && hi > lo;
            W.sortLo[a] = ok ? lo : 0.0f;
            W.sortScale[a] = ok ? 2.0f / (hi - lo) : 0.0f;
        }
    }
    const bool wide = p.wide != 0, quant = p.wide == 2;
    OccKey occKey;
    occKey.version = s.scene.version, occKey.stackDepth = p.stackDepth, occKey.fmt = p.wide, occKey.topBytes = p.topBytes;
    occKey.ldsScene = p.ldsScene != 0, occKey.full = p.full != 0;
    if (!same_key(c.wfOccKey, occKey)) {
        const int ln = p.ldsScene ? p.numNodes : 0, lt = p.ldsScene ? p.numTris : 0;
        c.wfBlocksPerCu[0] =
            hippt::wf_extend_blocks_per_cu(false, p.full != 0, wide, quant, p.stackDepth, ln, lt, p.topBytes);
        c.wfBlocksPerCu[1] =
            hippt::wf_extend_blocks_per_cu(true, p.full != 0, wide, quant, p.stackDepth, ln, lt, p.topBytes);
        c.wfOccKey = occKey;
    }
    s.activeBlocksPerCu = c.wfBlocksPerCu[cnt ? 1 : 0];
    const int bpc = s.blocksPerCu > 0 ? s.blocksPerCu : c.wfBlocksPerCu[cnt ? 1 : 0];
    const int blocks = int(std::max(1LL, std::min<long long>((long long)c.cus * bpc, (slots + 255) / 256)));
    if (!ensure_spill(c, p, blocks, spills, spillCap, err)) return false;
    W.mp = p;
    EventPair ev;
    if (!next_events(c, ev, err)) return false;
    HIP_TRY(hipEventRecord(ev.a, c.stream));
    HIP_TRY(hippt::wf_launch_init(W, c.stream));
    HIP_TRY(hippt::wf_launch_generate(W, 0, c.stream));
    // every path needs <= maxDepth extend rounds; slots regenerate as paths end
    const long long maxIter = (long long)p.maxDepth * ((p.totalItems + slots - 1) / slots + 1) + 64;
    // Every kPollEvery iterations the ray-queue sizes (appended + generated entries) are copied to
    // pinned memory; the host reads the snapshot one batch later, so the stream always holds a
    // batch of queued work.  Iterations after the queue drained are no-ops (empty queues).
    constexpr int kPollEvery = 8, kSnap = 2 * hippt::kWfShards * hippt::kCtrStride;
    if (!c.wfHost) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c.wfHost), 2 * kSnap * sizeof(unsigned)));
    for (hipEvent_t &e : c.wfPoll)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int cur = 0;
    // A pool that holds every work item of the batch generates them all up front and never
    // regenerates, and every path ends within maxDepth extend rounds: at most maxDepth iterations
    // (a polled loop alone runs up to 2*kPollEvery - 1 empty iterations past the end; the poll
    // still ends a deep maxDepth early once every path has ended).
    const bool allInFlight = slots >= p.totalItems;
    for (long long it = 0;; ++it) {
        if (allInFlight && it == p.maxDepth) break;
        if (it > maxIter) return fail(err, "wavefront path tracer did not drain its ray queue");
        HIP_TRY(hippt::wf_launch_extend(W, cur, blocks, cnt, c.stream));
        HIP_TRY(hippt::wf_launch_shade(W, cur, c.stream));
        if (!allInFlight) HIP_TRY(hippt::wf_launch_generate(W, cur ^ 1, c.stream));
        cur ^= 1;
        if (it % kPollEvery != kPollEvery - 1) continue;
        const int b = int(it / kPollEvery) & 1;
        HIP_TRY(hipMemcpyAsync(c.wfHost + b * kSnap, c.wfCtr + hippt::ctr_word(hippt::ctr_queue(cur)),
                               kSnap * sizeof(unsigned), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipEventRecord(c.wfPoll[b], c.stream));
        if (it < 2 * kPollEvery - 1) continue;
        HIP_TRY(hipEventSynchronize(c.wfPoll[b ^ 1]));
        unsigned left = 0;
        for (int k = 0; k < 2 * hippt::kWfShards; ++k) left += c.wfHost[(b ^ 1) * kSnap + k * hippt::kCtrStride];
        if (left == 0) break;
    }
    HIP_TRY(hipEventRecord(ev.b, c.stream));
    c.pending.push_back({0, ev});
    return true;
}

CameraF current_camera() {
    State &s = S();
    if (s.scene.rawCamera) return s.scene.cam;
    CameraF cam;
    build_camera(s.scene.lookfrom, s.scene.lookat, s.scene.vup, s.scene.vfov, double(s.width) / double(s.height),
                 s.scene.aperture, s.scene.focus, cam);
    return cam;
}

// Copies a context's compact rows (c.rows rows of W pixels of `bytes` each) to their image rows
// c.y0, c.y0 + c.stride, ... of a full-frame host buffer, on the context's stream.
bool copy_rows_async(Ctx &c, void *dstFrame, const void *src, size_t bytes, const char **err) {
    State &s = S();
    if (c.rows <= 0) return true;
    const size_t row = size_t(s.width) * bytes;
    char *dst = static_cast<char *>(dstFrame) + size_t(c.y0) * row;
    HIP_TRY(hipMemcpy2DAsync(dst, row * size_t(c.stride), src, row, row, size_t(c.rows), hipMemcpyDeviceToHost, c.stream));
    return true;
}

// The open chain run's last combines (Ctx::chain): every batch no launch combined, in order; the run
// ends (the next chained batch starts a new one).
bool launch_chained(Ctx &c, hippt::MeshParams &p, const hippt::chain::HostLaunch &l, const char **err);

bool flush_chain(Ctx &c, const char **err) {
    Ctx::Chain &ch = c.chain;
    if (!ch.host.live) return true;
    HIP_TRY(hipSetDevice(c.device));
    hippt::chain::HostClose cl;
    hippt::chain::host_close(ch.host, cl);
    // The held batches' group launch, before the flush.  (The run counts as closed from here on even if
    // this launch fails: a HIP error of a launch is fatal to the context, and no batch joins the run.)
    if (cl.held && !launch_chained(c, ch.pendP, cl.launch, err)) return false;
    hippt::ChainFlushParams f{};
    f.comb = ch.key.comb;
    f.scratch = c.chainScratch;
    f.ctl = c.chainCtl;
    f.epoch = cl.epoch;
    f.lastSeq = cl.lastSeq;
    f.slots = ch.host.slots;
    f.shift = ch.shift;
    f.step = cl.step;
    f.audit = ch.audit;
    if (ch.audit && !c.auditRuns.empty()) {  // the run's header: what it asked for
        Ctx::AuditRun &a = c.auditRuns.back();
        a.hdr[4] = unsigned(ch.host.step);
        a.hdr[8] = cl.lastSeq + 1u;
        a.hdr[9] = cl.epoch;
        a.hdr[11] = a.hdr[8] > hippt::kAuditBatches ? a.hdr[8] - hippt::kAuditBatches : 0u;
        a.closed = true;
    }
    return TIMED_LAUNCH(c, 1, hippt::launch_chain_flush(f, c.stream));
}

// The deferred combine of a context as a launch of its own (see Ctx::deferred), or the open chain
// run's flush.
bool flush_deferred(Ctx &c, const char **err) {
    if (!flush_chain(c, err)) return false;
    if (!c.hasDeferred) return true;
    c.hasDeferred = false;
    HIP_TRY(hipSetDevice(c.device));
    if (!TIMED_LAUNCH(c, 1, hippt::launch_combine(c.deferred, c.stream, c.deferredHost))) return false;
    c.deferredHost = hippt::HostFrame{};
    return true;
}

// A per-sample radiance buffer of at least `need` bytes that the deferred combine does not read.
bool batch_scratch(Ctx &c, size_t need, float **out, const char **err) {
    const bool alt = c.hasDeferred && c.deferred.scratch == c.scratch;
    float *&buf = alt ? c.scratchAlt : c.scratch;
    size_t &bytes = alt ? c.scratchAltBytes : c.scratchBytes;
    if (bytes < need) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        (void)hipFree(buf);
        buf = nullptr;
        bytes = 0;
        void *p = nullptr;
        HIP_TRY(work_malloc(c.device, &p, need, &bytes));
        buf = static_cast<float *>(p);
    }
    *out = buf;
    return true;
}

// Chained batches (Ctx::chain).  Automatic (HIPPT_OPT_CHAIN -1): every batch (whose items fit the ring's
// slot bits) is chained; a launch traces up to cap batches (chain_cap) and the ring holds twice that, so
// that a launch traces one group of batches while it combines the previous one.  Measured (r5s/r5x, 20
// steps, cap by chain_cap): 1/8 shares Cornell 1.112 -> 1.047 ms, blob70k 3.003 -> 2.518, cornell_mixed
// 1.831 -> 1.573; 1/2 shares blob70k 9.79 -> 9.49, cornell_mixed 6.20 -> 5.92, Cornell 3.757 -> 3.765;
// whole images blob70k 18.94 -> 18.69, cornell_mixed 12.06 -> 11.70, but Cornell 7.255 -> 7.321, so
// round 5 ran a whole image of an LDS-resident Lambertian scene one launch per batch.  Round 6 (r6aw/r6ax,
// alternating passes, with the held groups and the clock warm-up): a whole Cornell image chained at cap 8
// 55,875 -> 56,111 M/s, so it is chained too.
// chain_batch's held groups (an A/B build knob)
#ifndef HIPPT_CHAIN_GROUPS
#define HIPPT_CHAIN_GROUPS 1
#endif
constexpr bool kChainGroups = HIPPT_CHAIN_GROUPS != 0;
// chain_batch holds the batches that arrive while the run's first launch runs (an A/B build knob)
#ifndef HIPPT_CHAIN_HOLD_RUNNING
#define HIPPT_CHAIN_HOLD_RUNNING 1
#endif
constexpr bool kChainHoldRunning = HIPPT_CHAIN_HOLD_RUNNING != 0;

// (the cap and the ring of a run: hippt_plan.h chain_cap, ring_slots, ring_plan)

// The ring's buffers for plan `r` (allocated, or grown after the open run's last combines); *ok =
// false when the device has no memory for them (the batch then runs unchained).
bool ensure_ring(Ctx &c, const plan::RingPlan &r, bool *ok, const char **err) {
    *ok = true;
    if (!c.chainCtl) HIP_TRY(hipMalloc(&c.chainCtl, hippt::kChainCtlWords * sizeof(unsigned)));
    if (!c.chainBox) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c.chainBox), sizeof(unsigned long long),
                              hipHostMallocMapped | hipHostMallocCoherent));
        *c.chainBox = 0;
        void *d = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&d, c.chainBox, 0));
        c.chainBoxDev = static_cast<unsigned long long *>(d);
    }
    if (c.chainScratchBytes >= r.bytes) return true;
    if (!flush_deferred(c, err)) return false;  // the open run's last combines read the old ring
    HIP_TRY(hipStreamSynchronize(c.stream));
    (void)hipFree(c.chainScratch);
    c.chainScratch = nullptr;
    c.chainScratchBytes = 0;
    void *p = nullptr;
    size_t got = 0;
    if (work_malloc(c.device, &p, r.bytes, &got) != hipSuccess) {
        (void)hipGetLastError();
        c.chainScratch = nullptr;
        *ok = false;
        return true;
    }
    c.chainScratch = static_cast<float *>(p);
    c.chainScratchBytes = got;
    return true;
}

bool same_cam(const CameraF &a, const CameraF &b) {
    if (a.lens_radius != b.lens_radius) return false;
    for (int k = 0; k < 3; ++k)
        if (a.origin[k] != b.origin[k] || a.llc[k] != b.llc[k] || a.horizontal[k] != b.horizontal[k] ||
            a.vertical[k] != b.vertical[k] || a.u[k] != b.u[k] || a.v[k] != b.v[k])
            return false;
    return true;
}

// Two batches' launch parameters agree on everything the run's launches take from their own
// parameters for every batch of the run (all but the frames, scratch, counters and chain fields).
bool chain_same(const hippt::MeshParams &a, const hippt::MeshParams &b) {
    return a.nodes == b.nodes && a.tris == b.tris && a.shade == b.shade && a.mats == b.mats && a.stats == b.stats &&
           same_cam(a.cam, b.cam) && a.invW == b.invW && a.invH == b.invH && a.width == b.width &&
           a.height == b.height && a.y0 == b.y0 && a.bandRows == b.bandRows && a.rowStride == b.rowStride &&
           a.frames == b.frames && a.maxDepth == b.maxDepth && a.bandPixels == b.bandPixels &&
           a.totalItems == b.totalItems && a.stackDepth == b.stackDepth && a.numNodes == b.numNodes &&
           a.numTris == b.numTris && a.numMats == b.numMats && a.ldsScene == b.ldsScene && a.full == b.full &&
           a.waveThreshold == b.waveThreshold && a.chunk == b.chunk && a.leafExit == b.leafExit &&
           a.nodeExit == b.nodeExit && a.wide == b.wide && a.stackCap == b.stackCap && a.spillCap == b.spillCap &&
           a.spill == b.spill && a.topBytes == b.topBytes && a.refBits == b.refBits && a.runOrder == b.runOrder &&
           a.runCount == b.runCount && a.runTileShift == b.runTileShift && a.rngTable == b.rngTable && a.poolOffset == b.poolOffset &&
           a.poolWords == b.poolWords && a.comb.format == b.comb.format && a.padWord == b.padWord &&
           a.trimScale == b.trimScale && a.skyRect.x0 == b.skyRect.x0 && a.skyRect.y0 == b.skyRect.y0 &&
           a.skyRect.x1 == b.skyRect.x1 && a.skyRect.y1 == b.skyRect.y1 && a.orderRow == b.orderRow;
}

// Enqueues launch `l` of the run (chain::host_add, host_launch_held, host_close) with batch p's
// parameters, between the start and end events chain_batch's hold test queries.
bool launch_chained(Ctx &c, hippt::MeshParams &p, const hippt::chain::HostLaunch &l, const char **err) {
    p.chainSeq = l.own;
    p.chainGroup = l.group;
    p.chainPosted = l.posted;
    p.chainEpoch = l.epoch;
    if (!c.chainStartEv) HIP_TRY(hipEventCreateWithFlags(&c.chainStartEv, hipEventDisableTiming));
    if (!c.chainEndEv) HIP_TRY(hipEventCreateWithFlags(&c.chainEndEv, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c.chainStartEv, c.stream));
    if (!TIMED_LAUNCH(c, 0, hippt::launch_mesh(p, int(c.chain.blocks), false, c.stream))) return false;
    HIP_TRY(hipEventRecord(c.chainEndEv, c.stream));
    return true;
}

bool launch_held(Ctx &c, const char **err) {
    Ctx::Chain &ch = c.chain;
    if (!hippt::chain::host_has_held(ch.host)) return true;
    HIP_TRY(hipSetDevice(c.device));
    hippt::chain::HostLaunch l;
    hippt::chain::host_launch_held(ch.host, l);
#ifdef HIPPT_CHAIN_TRACE
    std::fprintf(stderr, "chain run %u group launched early: own %u batches %u epoch %u\n", ch.host.run, l.own, l.group,
                 l.epoch);
#endif
    return launch_chained(c, ch.pendP, l, err);
}

// The closed runs' audit records to State::auditWords (the context's stream finished past their
// final flush: after a synchronisation).  A run still open stays.
void harvest_audit(Ctx &c) {
    if (!c.auditDev) return;
    State &s = S();
    size_t k = 0;
    for (auto &a : c.auditRuns) {
        if (!a.closed) {
            c.auditRuns[k++] = a;
            continue;
        }
        const unsigned recs = std::min(a.hdr[8], hippt::kAuditBatches) + 1u;
        std::vector<unsigned> w(size_t(recs) * hippt::kAuditWords);
        if (hipMemcpy(w.data(), c.auditDev + size_t(a.slab) * hippt::kAuditRunWords, w.size() * sizeof(unsigned),
                      hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        s.auditWords.insert(s.auditWords.end(), a.hdr, a.hdr + hippt::kAuditWords);
        s.auditWords.insert(s.auditWords.end(), w.begin(), w.end());
    }
    c.auditRuns.resize(k);
}

// Makes batch `p` (its parameters otherwise complete, `blocks` its grid) the next batch of the open
// run, or of a new run (the old one flushed first): the chain fields, the ring slot's scratch, and
// the launch.  While the run's last enqueued launch has not started, batches are held (not posted)
// and then launched together as one group (MeshParams::chainGroup, up to chainCap): the group is one
// job whose queues walk the item order once for all its batches, as one batch of that many frames
// would (a chain of small batches walks it once per batch: -3.6% for a 1/8 share, r5ad), and a burst
// of async batches gets one launch per group instead of one per batch (each a ~21 us launch that
// finds its batch taken, plus the gap between launches; r5j).  A batch launched on its own is posted
// in the mailbox, so that a running launch may go on with it (chained batches); held batches are
// not, so no launch but their group's takes them.  Every decision here is hippt_chain_logic.h's
// (host_continues, host_open, host_add); this function does the HIP work around them.
bool chain_batch(Ctx &c, hippt::MeshParams &p, long long blocks, const plan::RingPlan &ring, const char **err) {
    namespace chain = hippt::chain;
    Ctx::Chain &ch = c.chain;
    chain::HostRun &run = ch.host;
    p.comb = hippt::CombineParams{c.accum, c.out, nullptr, p.bandPixels, p.totalItems, 0, p.frames, p.comb.format,
                                  p.comb.sky};
    const bool same = run.live && blocks == ch.blocks && ch.geomRev == S().scene.geomRev && chain_same(p, ch.key);
    if (!chain::host_continues(run, same, p.firstFrame, p.frames)) {
        if (!flush_deferred(c, err)) return false;  // the old run's (or an unchained batch's) combines
        // (the ring's buffers: ensure_ring, before the batch was chained)
        HIP_TRY(hipMemsetAsync(c.chainCtl, 0, hippt::kChainCtlWords * sizeof(unsigned), c.stream));
        chain::host_open(run, p.firstFrame, ring.cap, ring.slots);
        ch.shift = ring.shift;
        ch.blocks = blocks;
        ch.geomRev = S().scene.geomRev;
        p.comb.scratch = c.chainScratch;
        p.comb.firstFrame = p.firstFrame;
        ch.key = p;
        ch.audit = nullptr;
        if (S().chainAudit) {
            if (!c.auditDev) {
                HIP_TRY(hipMalloc(&c.auditDev, size_t(hippt::kAuditRuns) * hippt::kAuditRunWords * sizeof(unsigned)));
            }
            if (c.auditRuns.size() >= hippt::kAuditRuns) {  // every slab holds a closed run: to the host first
                HIP_TRY(hipStreamSynchronize(c.stream));
                harvest_audit(c);
            }
            const unsigned slab = c.auditNext++ % hippt::kAuditRuns;
            ch.audit = c.auditDev + size_t(slab) * hippt::kAuditRunWords;
            HIP_TRY(hipMemsetAsync(ch.audit, 0, hippt::kAuditRunWords * sizeof(unsigned), c.stream));
            Ctx::AuditRun a{};
            a.hdr[0] = 0xC4A1D17u;
            a.hdr[1] = run.run;
            a.hdr[2] = unsigned(c.device);
            a.hdr[3] = unsigned(p.firstFrame);
            a.hdr[4] = ~0u;
            a.hdr[5] = unsigned(p.frames);
            a.hdr[6] = p.bandPixels;
            a.hdr[7] = p.totalItems;
            a.hdr[10] = run.slots;
            a.slab = slab;
            a.closed = false;
            c.auditRuns.push_back(a);
        }
    }
    p.chainAudit = ch.audit;
    p.scratch = c.chainScratch;
    p.queue = c.chainCtl;
    p.combCtr = nullptr;
    p.comb.scratch = c.chainScratch;
    p.comb.firstFrame = run.firstFrame;
    p.chainCtl = c.chainCtl;
    p.chainBox = c.chainBoxDev;
    p.chainRun = run.run;
    p.chainSlots = run.slots;
    p.chainShift = ch.shift;
    p.chainCap = run.cap;
    p.chainStep = run.step;
    c.hostSamples += (unsigned long long)p.bandPixels * unsigned(p.frames);  // (the combine's samples too)
    // What host_add reads of the run's last launch, and no more (chain::host_add_reads).  Groups are for
    // 64-item runs only: a group interleaves its batches' runs.
    const bool groupable = kChainGroups && p.totalItems % 64u == 0;
    const unsigned reads = chain::host_add_reads(run, groupable, kChainHoldRunning);
    const bool started = !(reads & chain::kReadsStarted) || hipEventQuery(c.chainStartEv) != hipErrorNotReady;
    const bool ended = !(reads & chain::kReadsEnded) || !started || hipEventQuery(c.chainEndEv) != hipErrorNotReady;
    const chain::HostAdd a = chain::host_add(run, groupable, started, ended, kChainHoldRunning);
#ifdef HIPPT_CHAIN_TRACE
    std::fprintf(stderr, "chain run %u seq %u %s (held %u epoch %u cap %u slots %u)\n", run.run, a.seq,
                 a.kind == chain::kAddHeld ? "held" : a.kind == chain::kAddGroup ? "launched with the held ones" : "launched",
                 a.held, a.launch.epoch, run.cap, run.slots);
#endif
    switch (a.kind) {
    case chain::kAddHeld:
        // the group's own batch (chainSeq, chainGroup, chainPosted and chainEpoch: set at its launch)
        if (!a.held) ch.pendP = p;
        return true;
    case chain::kAddGroup:  // the held batches and this one: one group launch
        return launch_chained(c, ch.pendP, a.launch, err);
    case chain::kAddAlone:
        // post: one word, so that a launch reads the run, its frame pattern and the last batch together
        __atomic_store_n(c.chainBox, a.word, __ATOMIC_RELEASE);
        return launch_chained(c, p, a.launch, err);
    }
    return true;
}

// The device address of a mapped pinned host frame on the current device, or null where the
// runtime cannot map it (the caller then copies after the kernel).
uint32_t *host_frame_on_device(unsigned *frame) {
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, frame, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint32_t *>(d);
}

// The planner's inputs (hippt_plan.h): the LDS limits of the kernels as built, and the uploaded scene's
// facts (halfTree: render_layout, which builds that tree on use).
plan::Limits lds_limits() { return plan::Limits{hippt::mesh_lds_scene_limit(), hippt::mesh_lds_block_budget()}; }

plan::Facts scene_facts(const SceneHost &sc) {
    plan::Facts f;
    f.numNodes = sc.numNodes;
    f.numNodes4 = sc.numNodes4;
    f.numTris = sc.numTris;
    f.numMats = int(sc.mats.size() / 2);
    f.levels = sc.levels;
    f.stackBound4 = sc.stackBound4;
    f.full = sc.full;
    f.quantTree = !sc.nodes4q.empty();
    return f;
}

// A render's layout plan under the options as set.  The half-precision tree is built here, the first
// time a plan reads it (and never for a plan that does not).
plan::Layout render_layout(plan::Facts &f, const CameraF &cam) {
    State &s = S();
    const plan::Limits lim = lds_limits();
    f.halfTree = plan::wants_half(f, s.knobs, lim) && half_tree_ok(s.scene);
    const bool pinhole = cam.lens_radius == 0.0f && cam.origin[0] != 0.0f && cam.origin[1] != 0.0f &&
                         cam.origin[2] != 0.0f;
    return plan::layout(f, s.knobs, lim, pinhole);
}

// The legacy 4-sphere scene's frames on context c: one launch.  *copied: the kernel wrote the frame's
// rows into the pinned host frame `dst` itself (legacy zero copy).
bool enqueue_sphere4(Ctx &c, int firstFrame, int count, int maxDepth, bool copy, unsigned *dst, bool *copied,
                     const char **err) {
    State &s = S();
    // the legacy kernel writes accum/out itself: a mesh batch's pending combine goes first
    if (!flush_deferred(c, err)) return false;
    c.skyCombinePixels = 0;
    s.activeEnv = 0;  // (the built-in scene keeps its gradient)
    hippt::Sphere4Params p{c.accum, c.out, c.stats, s.width, s.height, c.y0, c.rows, c.stride, firstFrame, count,
                           maxDepth, s.pixelFormat, nullptr};
    // A blocking frame (the app's cudaPathTracerRender): the kernel writes the words into
    // the pinned host frame itself, overlapping the PCIe transfer with the trace, instead
    // of a D2H copy after it (1080p: 0.17 ms of copy behind 0.13 ms of kernel)
    if (copy && kLegacyZeroCopy) {
        p.hostOut = host_frame_on_device(dst);
        *copied = p.hostOut != nullptr;  // else the copy after the kernel
    }
    return TIMED_LAUNCH(c, 0, hippt::launch_sphere4(p, c.stream));
}

// HIPPT_OPT_ENV_SAMPLING as applied: 1 for an uploaded scene under an environment with a light-sampling mode set,
// whether or not the scene holds a light; else 0 (the option-off code runs).
int env_sampling_applies() {
    const State &s = S();
    return s.scene.kind == HIPPT_SCENE_MESH && s.envSize && s.lightSampling ? s.envSampling : 0;
}

// HIPPT_OPT_LIGHT_SAMPLING_MODE as applied: its value (1, or 2 with MIS) if the scene holds an emissive primitive
// or the environment is sampled (the light-sampling route with an empty light list), else 0 (the option-off
// code runs).
int light_sampling_applies() {
    const State &s = S();
    return s.scene.kind == HIPPT_SCENE_MESH && (!s.scene.lights.empty() || env_sampling_applies()) ? s.lightSampling : 0;
}

// HIPPT_OPT_LIGHT_SELECT as applied: its value where light sampling applies and the scene's lights have a
// selection table (hippt_refit.h light_table_fits), else 0 (uniform).
int light_select_applies() {
    const State &s = S();
    return light_sampling_applies() && hippt::light_table_fits(s.scene.lights.size()) ? s.lightSelect : 0;
}

// The table's pointers for a launch of c under the option as applied (nulls: the uniform choice).
void set_light_select(const Ctx &c, hippt::PathParams &p) {
    if (!light_select_applies() || !c.lightTable) return;
    const hippt::LightTableBuffers t =
        hippt::light_table_buffers(c.lightTable, int(S().scene.lights.size()), S().scene.numTris);
    p.lightCdf = t.cdf;
    p.lightIp = t.ipPrim;
}

// ---- environment (hipptSetEnvironment; hippt_env.h) ----
// The environment as applied: its size for an uploaded scene, else 0 (the built-in scene keeps its gradient).
int env_applies() {
    const State &s = S();
    return s.scene.kind == HIPPT_SCENE_MESH ? s.envSize : 0;
}

// Forgets the copies of a staging buffer that have finished; true if none is left.
bool env_stage_free(State::EnvStage &st) {
    size_t kept = 0;
    for (auto &de : st.busy) {
        (void)hipSetDevice(de.first);
        if (hipEventQuery(de.second) == hipSuccess) (void)hipEventDestroy(de.second);
        else st.busy[kept++] = de;
    }
    (void)hipGetLastError();  // (hipErrorNotReady is no error of ours)
    st.busy.resize(kept);
    return st.busy.empty();
}

// Waits for every queued upload and frees the staging buffers (the contexts go away).
void env_stages_release() {
    for (auto &st : S().envStages) {
        for (auto &de : st.busy) {
            (void)hipSetDevice(de.first);
            (void)hipEventSynchronize(de.second);
            (void)hipEventDestroy(de.second);
        }
        if (st.ptr) (void)hipHostFree(st.ptr);
    }
    S().envStages.clear();
}

// Brings context c's copy of the environment up to the host copy's revision, in stream order: launches
// queued before see the old texels, later ones the new.  A copy of the same size is one hipMemcpyAsync from
// a pinned staging buffer that no earlier upload still reads; another size waits for the stream (queued
// launches read the buffer that is freed).
bool upload_env(Ctx &c, const char **err) {
    State &s = S();
    if (c.envRev == s.envRev) return true;
    if (s.envSize == 0) {  // removed: the buffer stays for the launches that may still read it
        c.envRev = s.envRev;
        return true;
    }
    HIP_TRY(hipSetDevice(c.device));
    const size_t bytes = s.env.size() * sizeof(hippt::env::Texel);
    if (c.envSize != s.envSize) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        (void)hipFree(c.env);
        (void)hipFree(c.envTable);
        c.env = nullptr;
        c.envTable = nullptr;
        c.envSize = 0;
        HIP_TRY(hipMalloc(&c.env, bytes));
        if (hipMalloc(&c.envTable, hippt::env_table_words(size_t(s.envSize)) * sizeof(unsigned)) != hipSuccess) {
            (void)hipFree(c.env);
            c.env = nullptr;
            c.envTable = nullptr;
            return fail(err, "hipMalloc(&c.envTable, ...) failed");
        }
        c.envSize = s.envSize;
    }
    // the staging buffer of this revision, or a free one filled now; other free ones beyond one go
    State::EnvStage *st = nullptr;
    for (auto &e : s.envStages)
        if (e.rev == s.envRev) st = &e;
    if (!st) {
        std::vector<State::EnvStage> keep;
        bool taken = false, spare = false;
        for (auto &e : s.envStages) {
            const bool free = env_stage_free(e);
            if (free && !taken && e.bytes >= bytes) {
                taken = true;
                keep.insert(keep.begin(), e);  // (first: found again below)
            } else if (!free || !spare) {
                spare = spare || free;
                keep.push_back(e);
            } else {
                (void)hipHostFree(e.ptr);
            }
        }
        s.envStages.swap(keep);
        if (taken) st = &s.envStages.front();
        if (!st) {
            State::EnvStage e;
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e.ptr), bytes, hipHostMallocDefault));
            e.bytes = bytes;
            s.envStages.push_back(e);
            st = &s.envStages.back();
        }
        std::memcpy(st->ptr, s.env.data(), bytes);
        st->rev = s.envRev;
    }
    HIP_TRY(hipMemcpyAsync(c.env, st->ptr, bytes, hipMemcpyHostToDevice, c.stream));
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    st->busy.push_back({c.device, ev});
    HIP_TRY(hipEventRecord(ev, c.stream));
    // the selection table follows the new texels, behind the copy on the same stream
    HIP_TRY(hippt::launch_env_table(hippt::env_table_buffers(c.env, c.envTable, c.envSize), c.stream));
    c.envRev = s.envRev;
    return true;
}

// The environment's pointers for a launch of c (upload_env has run), or nulls without one.
void set_env(const Ctx &c, hippt::PathParams &p) {
    if (!env_applies()) return;
    p.env = c.env;
    p.envSize = c.envSize;
    if (!env_sampling_applies() || !p.lightMode) return;
    const hippt::EnvTableBuffers t = hippt::env_table_buffers(c.env, c.envTable, c.envSize);
    p.envRowC = t.rowC;
    p.envTexels = t.texels;
}

// A mesh call's batches on a context: as many frames per batch as the sample scratch budget
// (HIPPT_OPT_SCRATCH_MB) and the 2^31 work items of a launch hold.
struct BatchSize {
    int frames;
    size_t need;    // scratch bytes of a full batch
    size_t budget;  // the scratch budget (also the chain ring's, ring_plan)
};
BatchSize frames_per_batch(unsigned bandPixels, int count) {
    const size_t perFrame = size_t(bandPixels) * 3 * sizeof(float);
    const size_t cap = size_t(std::max<long long>(1, S().scratchMB)) << 20;
    int fpb = int(std::max<size_t>(1, cap / perFrame));
    fpb = std::min(fpb, count);
    fpb = int(std::min<long long>(fpb, (1LL << 31) / std::max<unsigned>(1, bandPixels)));
    fpb = std::max(fpb, 1);
    return BatchSize{fpb, perFrame * size_t(fpb), cap};
}

// Resident blocks per CU of the plan's megakernel variants on context c (cached per OccKey).
void mesh_occupancy(Ctx &c, const plan::Facts &f, const plan::Layout &L) {
    State &s = S();
    OccKey key;
    key.version = s.scene.version, key.stackDepth = L.stackDepth, key.fmt = L.fmt, key.poolWords = L.poolWords;
    key.topBytes = L.topBytes, key.ldsScene = L.ldsScene, key.full = f.full, key.spills = L.spills;
    if (same_key(c.occKey, key)) return;
    const int ln = L.ldsScene ? L.numNodes : 0, lt = L.ldsScene ? f.numTris : 0, lm = L.ldsScene ? f.numMats : 0;
    const int full = f.full ? (s.scene.emissive ? 2 : 1) : 0;  // (the key's scene version covers `emissive`)
    c.meshBlocksPerCu[0] =
        hippt::mesh_blocks_per_cu(false, full, L.fmt, L.stackDepth, ln, lt, L.spills, L.topBytes, lm, L.poolWords);
    c.meshBlocksPerCu[1] =
        hippt::mesh_blocks_per_cu(true, full, L.fmt, L.stackDepth, ln, lt, L.spills, L.topBytes, lm, L.poolWords);
    c.meshBlocksPerCuChain = L.poolWords && L.fmt == hippt::kWideFloat
                                 ? hippt::mesh_blocks_per_cu(false, full, L.fmt, L.stackDepth, ln, lt, L.spills,
                                                             L.topBytes, lm, L.poolWords, true)
                                 : 0;
    c.occKey = key;
}

// One batch's launch parameters from (context, plan, batch): frames [firstFrame, firstFrame + frames)
// of the context's rows.  The chain fields, the spill area and the combine are the launch's (chain_batch,
// ensure_spill, enqueue_mesh).
bool fill_mesh_params(Ctx &c, const plan::Facts &f, const plan::Layout &L, const plan::Batch &B, bool chained,
                      const CameraF &cam, int firstFrame, int frames, int maxDepth, float *scratch, hippt::MeshParams &p,
                      hippt::SkyComb &sky, const char **err) {
    State &s = S();
    const unsigned bandPixels = unsigned(c.rows) * unsigned(s.width);
    unsigned long long skyPixels = 0;  // band pixels whose samples the combine finishes (HIPPT_OPT_SKY_COMBINE)
    switch (L.fmt) {
    case hippt::kWideHybrid: p.nodes = c.nodes4h; break;
    case hippt::kWideQuant: p.nodes = c.nodes4q; break;
    case hippt::kWideHalf: p.nodes = c.nodes4f; break;
    case hippt::kWideFloat: p.nodes = c.nodes4; break;
    default: p.nodes = c.nodes; break;
    }
    p.tris = c.tris;
    p.shade = c.shade;
    p.mats = c.mats;
    p.scratch = scratch;
    p.queue = c.queue;
    p.stats = c.stats;
    p.cam = cam;
    p.invW = 1.0f / float(std::max(1, s.width - 1));
    p.invH = 1.0f / float(std::max(1, s.height - 1));
    p.width = s.width;
    p.height = s.height;
    p.y0 = c.y0;
    p.bandRows = c.rows;
    p.rowStride = c.stride;
    p.firstFrame = firstFrame;
    p.frames = frames;
    p.maxDepth = maxDepth;
    p.bandPixels = bandPixels;
    p.totalItems = bandPixels * unsigned(frames);
    p.rcpBandPixels = 1.0f / float(bandPixels);
    p.rcpWidth = 1.0f / float(s.width);
    p.stackDepth = L.stackDepth;
    p.numNodes = L.numNodes;
    p.numTris = f.numTris;
    p.numMats = f.numMats;
    p.ldsScene = L.ldsScene ? 1 : 0;
    p.full = f.full ? (s.scene.emissive ? 2 : 1) : 0;
    p.waveThreshold = L.waveThreshold;
    p.chunk = B.chunk[chained ? 1 : 0];
    p.leafExit = L.leafExit;
    p.nodeExit = L.nodeExit;
    p.wide = L.fmt;
    p.stackCap = L.stackCap;
    p.topBytes = L.topBytes;
    p.refBits = L.refBits;
    // The sky rectangle (below) needs the host copy's root box.  A host-memory vertex
    // update's vertices are on the host already: for a scene that fits the LDS copy the
    // host copy takes them here, a refit of a few hundred primitives, before anything of
    // this batch looks at it; a larger scene's waits for whatever next needs the host
    // copy (blob70k's host refit takes 10 ms).
    const bool skyWanted = B.skyWanted[chained ? 1 : 0];
    if (skyWanted && L.ldsScene && s.upd.hostStale && !s.upd.staleEv) settle_scene();
    const bool trims = B.trimWanted && render_pad_holds(s.scene, s.upd.hostStale, cam);
    p.padWord = c.padDev;
    p.trimScale = trims ? hippt::slab::trim_scale(s.knobs.renderPad) : 0.0f;
    s.activeRenderPad = trims ? s.knobs.renderPad : 0;
    // the sky rectangle (HIPPT_OPT_SKY_RECT): not while a device-memory vertex update is ahead of the
    // host copy (the scene may have grown past the host's root box)
    const bool skyOn = skyWanted && !s.upd.hostStale;
    const hippt::skyrect::Rect sr = skyOn ? sky_rect_of(s.scene, cam, s.width, s.height)
                                          : hippt::skyrect::whole(s.width, s.height);
    p.skyRect = hippt::SkyRect{sr.x0, sr.y0, sr.x1, sr.y1};
    s.activeSkyPixels = hippt::skyrect::pixels_outside(sr, s.width, s.height);
    p.rngTable = nullptr;
    p.poolWords = L.poolWords;
    // Pixel runs by estimated sample length, longest first, per XCD queue
    // (megakernel; item_order.h): Cornell +2.4%, cornell_mixed +3%, blob70k
    // +0.8% at full size; the slowest 1/8 Cornell share -2% (r5w)
    if (s.knobs.pathMode == 0 && s.itemOrder != 0) {
        const unsigned *table = nullptr;
        // the runs' shape: HIPPT_OPT_PIXEL_TILE columns.  Automatic: 8x8 tiles for
        // a band of consecutive rows (blob70k 1080p +0.45%, Cornell +0.6%, two
        // alternating passes, r6d), row runs for an interleaved share (the tile's
        // rows are `stride` image rows apart: the 1/8 shares neutral to -0.9%, r6f)
        const int tile = s.pixelTile >= 0 ? s.pixelTile : c.stride == 1 ? 8 : 0;
        const unsigned tileShift = tile == 8 ? 3u : tile == 16 ? 4u : tile == 32 ? 5u : 6u;
        // HIPPT_OPT_SKY_COMBINE: the runs wholly outside the rectangle are left out of the table and
        // finished by the batch's combine.  Not for a counted or an audited batch (their
        // counts are per traced item), and only with the built-in gradient sky (this function's callers).
        const bool skyComb = B.skyCombine[chained ? 1 : 0] && skyOn && !s.chainAudit &&
                             !hippt::skyrect::is_whole(sr, s.width, s.height);
        unsigned skyRuns = 0;
        if (!ensure_order(c, cam, frames, maxDepth, s.itemOrder == 1, tileShift, &table, err, skyComb ? &p.skyRect : nullptr,
                          &skyRuns))
            return false;
        if (table) {
            p.runOrder = table;
            p.runCount = unsigned(c.runCosts.size()) - skyRuns;
            p.runTileShift = c.orderKey.tileShift;
            if (skyRuns) {
                p.orderRow = hippt::skyrect::order_row_len(bandPixels, p.runCount);
                p.rcpOrderRow = 1.0f / float(p.orderRow);
                p.totalItems = p.orderRow * unsigned(frames);
                skyPixels = 64ull * skyRuns;
            }
        }
    }
    // the batch's snapshot for its combine (enqueue_mesh, chain_batch)
    sky = hippt::SkyComb{};
    if (skyPixels) {
        sky.on = 1;
        sky.width = unsigned(s.width);
        sky.rows = unsigned(c.rows);
        sky.tileShift = p.runTileShift;
        sky.y0 = c.y0;
        sky.rowStride = c.stride;
        sky.rect = p.skyRect;
        sky.invW = p.invW;
        sky.invH = p.invH;
        for (int k = 0; k < 3; ++k) {
            sky.origin[k] = cam.origin[k];
            sky.llc[k] = cam.llc[k];
            sky.horizontal[k] = cam.horizontal[k];
            sky.vertical[k] = cam.vertical[k];
        }
    }
    c.skyCombinePixels = (long long)skyPixels;
    p.poolOffset = L.poolOffset;
    if (s.rngTable && !rng_table(c, &p.rngTable, err)) return false;
    return true;
}

// A mesh scene's frames on context c, in batches: each a megakernel launch (on its own, or a batch of
// the context's chained run), or the wavefront's launches; its combine deferred into the next batch's
// launch, or flushed.
bool enqueue_mesh_lights(Ctx &c, const CameraF &cam, int firstFrame, int count, int maxDepth, int mode, const char **err);

bool enqueue_mesh(Ctx &c, const CameraF &cam, int firstFrame, int count, int maxDepth, bool copy, const char **err) {
    State &s = S();
    c.skyCombinePixels = 0;
    if (!ensure_scene(c, err)) return false;
    s.activeLightSampling = 0;
    s.activeLightSelect = 0;
    s.activeEnv = 0;
    s.activeEnvSampling = 0;
    if (const int mode = light_sampling_applies(); maxDepth > 0 && (mode || env_applies()))
        return enqueue_mesh_lights(c, cam, firstFrame, count, maxDepth, mode, err);
    const unsigned bandPixels = unsigned(c.rows) * unsigned(s.width);
    const BatchSize size = frames_per_batch(bandPixels, count);
    const bool cnt = s.knobs.countTraversal;
    plan::Facts facts = scene_facts(s.scene);
    const plan::Layout L = render_layout(facts, cam);
    s.activeWidth = L.wide ? 4 : 2;
    if (L.fmt == hippt::kWideHybrid && !ensure_hybrid(c, int(L.topBytes / 128), err)) return false;
    if (L.fmt == hippt::kWideHalf && !ensure_half(c, err)) return false;
    mesh_occupancy(c, facts, L);
    s.activeTopBytes = L.topBytes;
    s.activeBlocksPerCu = c.meshBlocksPerCu[cnt ? 1 : 0];
    const int bpc = s.blocksPerCu > 0 ? s.blocksPerCu : c.meshBlocksPerCu[cnt ? 1 : 0];
    for (int b = 0; b < count; b += size.frames) {
        const int nf = std::min(size.frames, count - b);
        const unsigned total = bandPixels * unsigned(nf);
        const plan::Batch B = plan::batch(facts, s.knobs, L, copy, maxDepth, total);
        const bool fuse = B.fuse;
        bool chained = B.mayChain && c.meshBlocksPerCuChain > 0;
        plan::RingPlan ring;
        if (chained) {
            ring = plan::ring_plan(total, s.knobs.chainBatches, L.ldsScene, size.budget);
            bool ok = ring.bytes != 0;
            if (ok && !ensure_ring(c, ring, &ok, err)) return false;
            chained = ok;
        }
        if ((!fuse || !chained) && !flush_chain(c, err)) return false;
        if (!fuse && !flush_deferred(c, err)) return false;
        float *scratch = nullptr;
        if (!chained && !batch_scratch(c, size.need, &scratch, err)) return false;
        hippt::SkyComb sky{};  // the batch's snapshot for its combine (HIPPT_OPT_SKY_COMBINE)
        if (maxDepth <= 0) {
            // ray_color with depth <= 0 returns black without tracing (RayTracer.h:582-583)
            HIP_TRY(hipMemsetAsync(scratch, 0, size_t(total) * 3 * sizeof(float), c.stream));
        } else {
            hippt::MeshParams p{};
            if (!fill_mesh_params(c, facts, L, B, chained, cam, firstFrame + b, nf, maxDepth, scratch, p, sky, err)) return false;
            if (sky.on) {
                // the left-out samples: one segment each, counted once per batch (the chained batches' pixel
                // samples are the host's already, chain_batch)
                const unsigned long long left = (unsigned long long)c.skyCombinePixels * unsigned(nf);
                c.hostSegments += left;
                if (!chained) c.hostSamples += left;
            }
            if (s.knobs.pathMode == 1) {
                if (!run_wavefront(c, p, cnt, L.spills, L.spillCap, err)) return false;
            } else {
                const long long blocks = ray_blocks(c, chained && s.blocksPerCu <= 0 ? c.meshBlocksPerCuChain : bpc, total);
                if (!ensure_spill(c, p, blocks, L.spills, L.spillCap, err)) return false;
                s.activeChunk = int(p.chunk);
                s.activeChainCap = 0;
                if (chained) {
                    p.comb.format = s.pixelFormat;
                    p.comb.sky = sky;  // (one camera per run, chain_same: the run's snapshot)
                    if (!chain_batch(c, p, blocks, ring, err)) return false;
                    s.activeChainCap = int(c.chain.host.cap);
                    continue;  // launched or taken by the run's last launch; its combine
                               // belongs to the run (Ctx::chain)
                } else {
                    HIP_TRY(hipMemsetAsync(c.queue, 0, kQueueBytes, c.stream));
                    // (a pending sky-mode combine goes to combine_kernel when this launch's variant has no sky
                    // branch, plan::sky_combine_kernel)
                    if (c.hasDeferred && c.deferred.sky.on &&
                        !plan::sky_combine_kernel(cnt, L.ldsScene, facts.full, L.spills, L.poolWords != 0, false) &&
                        !flush_deferred(c, err))
                        return false;
                    if (c.hasDeferred) {
                        p.comb = c.deferred;
                        c.hasDeferred = false;
                    }
                    p.combCtr = c.queue + kCombCtrWord;
                }
                if (!TIMED_LAUNCH(c, 0, hippt::launch_mesh(p, int(blocks), cnt, c.stream))) return false;
            }
        }
        if (chained && maxDepth > 0) continue;  // its combine belongs to the run (Ctx::chain)
        c.deferred = hippt::CombineParams{c.accum, c.out, scratch, bandPixels, total, firstFrame + b, nf, s.pixelFormat, sky};
        c.hasDeferred = true;
        if (!fuse && !flush_deferred(c, err)) return false;
    }
    return true;
}

// The end of a blocking call on context c: the frame's words into the pinned host frame `dst`, by the
// deferred combine itself where the frame can be mapped, else by a copy after the flush.  copied: the
// legacy kernel wrote them already.
bool finish_blocking_frame(Ctx &c, unsigned *dst, bool copied, const char **err) {
    State &s = S();
    if (c.rows > 0 && c.hasDeferred && kLegacyZeroCopy) {
        // a blocking mesh frame: its combine writes the words into the pinned host frame too
        if (uint32_t *d = host_frame_on_device(dst)) {
            c.deferredHost = hippt::HostFrame{d, s.width, c.y0, c.stride};
            copied = true;
        }
    }
    if (!flush_deferred(c, err)) return false;
    if (c.rows > 0 && !copied) {
        if (!copy_rows_async(c, dst, c.out, sizeof(uint32_t), err)) return false;
    }
    return true;
}

// Enqueues `count` frames on every context (no host wait).
// copy: the frame's words end in the full-frame pinned host buffer `dst` (State::host when null),
// written by the kernel that makes them (legacy kernel or combine) or copied after it.
bool enqueue_locked(int firstFrame, int count, int maxDepth, bool copy, const char **err, unsigned *dst = nullptr) {
    State &s = S();
    if (!dst) dst = s.host;
    if (!s.ready) return fail(err, "HIP path tracer not initialized");
    if (count < 0) return fail(err, "negative frame count");
    const bool mesh = s.scene.kind == HIPPT_SCENE_MESH;
    const CameraF cam = mesh ? current_camera() : CameraF{};
    for (Ctx &c : s.ctxs) {
        HIP_TRY(hipSetDevice(c.device));
        bool copied = false;  // the kernel wrote the frame's rows into the host frame (legacy zero copy)
        if (c.rows > 0 && count > 0) {
            if (!(mesh ? enqueue_mesh(c, cam, firstFrame, count, maxDepth, copy, err)
                       : enqueue_sphere4(c, firstFrame, count, maxDepth, copy, dst, &copied, err)))
                return false;
        }
        if (copy && !finish_blocking_frame(c, dst, copied, err)) return false;
    }
    return true;
}

bool sync_locked(const char **err) {
    State &s = S();
    for (Ctx &c : s.ctxs) {
        if (!flush_deferred(c, err)) return false;
        HIP_TRY(hipSetDevice(c.device));
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (auto &pe : c.pending)
            if (!account(pe, c, err)) return false;
        c.pending.clear();
        harvest_audit(c);
    }
    return true;
}

bool render_locked(int frameIndex, int count, int maxDepth, const unsigned int **hostPixels, const char **err) {
    if (!enqueue_locked(frameIndex, count, maxDepth, true, err)) return false;
    if (!sync_locked(err)) return false;
    if (hostPixels) *hostPixels = S().host;
    return true;
}

// ---- ray queries (hippt_query.hip; include/hippt.h hipptTraceRays, hipptOccluded, hipptTraceCamera,
// hipptTraceHits, hipptTraceCameraHits) and path queries (hippt_path.hip; hipptTraceRadiance,
// hipptCameraRays) ----
// A query is one or more launches of the query kernel on a context's stream, after whatever the stream
// already holds, followed by a wait for the query's own event.  It reads the scene buffers only: it
// does not flush the deferred combine or the chain, launches no held batch, and leaves the stats and
// the timing events alone, so pending asynchronous frames come out as if it had not been made.
using hippt::QueryMode;
using hippt::qlayout::Slot;

struct QueryCall {
    QueryMode mode = QueryMode::Closest;
    bool path = false;     // hipptTraceRadiance: the renderer's path per ray, in place of the mode's result
    bool camRays = false;  // hipptCameraRays: no traversal, the camera's rays and RNG states alone
    long long n = 0;       // rays (a camera call: the image's pixels instead)
    int flags = 0;
    int frame = 0;     // camera calls
    int maxDepth = 0;  // path
    hippt::qlayout::Table bufs;  // the caller's buffers (hippt_query_layout.h)
    bool camera() const { return camRays || hippt::query_camera(mode); }
};

QueryCall query_call(QueryMode mode, long long n, int frame, int flags,
                     std::initializer_list<std::pair<Slot, const void *>> bufs) {
    QueryCall q;
    q.mode = mode;
    q.n = n;
    q.frame = frame;
    q.flags = flags;
    for (const auto &b : bufs) q.bufs.add(b.first, b.second);
    return q;
}

// The device pointers of one launch of a path query or of the camera's rays (those QueryParams lacks).
struct PathPtrs {
    const unsigned *seeds = nullptr;
    float4 *radiance = nullptr;
    int *segments = nullptr;
    float4 *outRays = nullptr;
    unsigned *outSeeds = nullptr;
};

// Puts a buffer's device pointer where its slot says.
void set_slot(hippt::QueryParams &q, PathPtrs &pp, Slot slot, void *p) {
    switch (slot) {
    case Slot::Rays: q.rays = static_cast<const float4 *>(p); break;
    case Slot::T: q.t = static_cast<float *>(p); break;
    case Slot::Prim: q.prim = static_cast<int *>(p); break;
    case Slot::Occluded: q.occluded = static_cast<unsigned char *>(p); break;
    case Slot::Hits: q.hits = static_cast<float4 *>(p); break;
    case Slot::Seeds: pp.seeds = static_cast<const unsigned *>(p); break;
    case Slot::Radiance: pp.radiance = static_cast<float4 *>(p); break;
    case Slot::Segments: pp.segments = static_cast<int *>(p); break;
    case Slot::OutRays: pp.outRays = static_cast<float4 *>(p); break;
    case Slot::OutSeeds: pp.outSeeds = static_cast<unsigned *>(p); break;
    }
}

// Ray `at` of a caller's buffer.
char *ray_at(const hippt::qlayout::Buffer &b, long long at) {
    return static_cast<char *>(const_cast<void *>(b.ptr)) + size_t(at) * b.bytesPerRay;
}

// Makes *buf a device buffer of at least `need` bytes (*bytes: its size).  A buffer that is too small
// is freed first: if the allocation fails, *buf is null and *bytes 0.  `what` names the allocation in
// the error message.
bool grow(void **buf, size_t *bytes, size_t need, const char *what, const char **err) {
    if (*bytes >= need) return true;
    (void)hipFree(*buf);
    *buf = nullptr;
    *bytes = 0;
    const hipError_t e = hipMalloc(buf, need);
    if (e != hipSuccess) return fail(err, std::string(what) + ": " + hipGetErrorString(e));
    *bytes = need;
    return true;
}

// The check of a call's device pointers (the null ones skipped), in order; per pointer: device memory,
// on `requiredDevice` (-1: on the device of the pointers before it), aligned.  *device: where they are.
bool device_pointers_ok(const std::string &who, const char *flagName, int requiredDevice, const void *const *ptrs,
                        const size_t *aligns, int count, int *device, const char **err) {
    int dev = requiredDevice;
    for (int k = 0; k < count; ++k) {
        if (!ptrs[k]) continue;
        hipPointerAttribute_t a{};
        if (hipPointerGetAttributes(&a, ptrs[k]) != hipSuccess || a.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return fail(err, who + ": " + flagName + " needs device memory pointers");
        }
        if (dev >= 0 && a.device != dev)
            return fail(err, who + (requiredDevice >= 0 ? ": the pointers are not on the context's device"
                                                        : ": pointers on different devices"));
        dev = a.device;
        if (reinterpret_cast<uintptr_t>(ptrs[k]) % aligns[k]) return fail(err, who + ": misaligned device pointer");
    }
    if (device) *device = dev;
    return true;
}

// The traversal's layout and parameters for the current scene on context c: the render's plan under
// the queries' profile (hippt_plan.h query_knobs: the wavefront extend kernel's loop parameters, float
// nodes, no camera pool).  Unlike a render, whose launches take a spill area only when the stack bound
// exceeds the LDS capacity, the query kernel takes one for every 4-wide tree.
plan::Layout query_scene_params(Ctx &c, hippt::QueryParams &q) {
    State &s = S();
    const plan::Facts f = scene_facts(s.scene);
    const plan::Layout L = plan::layout(f, plan::query_knobs(s.knobs), lds_limits(), false);
    q = hippt::QueryParams{};
    q.nodes = L.wide ? c.nodes4 : c.nodes;
    q.tris = c.tris;
    q.shade = c.shade;
    q.pad = c.padDev;
    q.stackDepth = L.stackDepth;
    q.numNodes = L.numNodes;
    q.numTris = f.numTris;
    q.ldsScene = L.ldsScene ? 1 : 0;
    q.full = f.full ? 1 : 0;
    q.wide = L.wide ? 1 : 0;
    q.stackCap = L.stackCap;
    q.spillCap = L.spillCap;
    q.topBytes = L.topBytes;
    q.waveThreshold = L.waveThreshold;
    q.leafExit = L.leafExit;
    q.nodeExit = L.nodeExit;
    return L;
}

// The camera sample's arguments for `cam` over the image rows y0, y0 + rowStride, ... (bandPixels pixels
// of them), items frame-major from firstFrame.
hippt::QueryCam query_cam(const CameraF &cam, int y0, int rowStride, unsigned bandPixels, int firstFrame) {
    State &s = S();
    hippt::QueryCam k{};
    k.cam = cam;
    k.invW = 1.0f / float(std::max(1, s.width - 1));
    k.invH = 1.0f / float(std::max(1, s.height - 1));
    k.width = s.width;
    k.y0 = y0;
    k.rowStride = rowStride;
    k.firstFrame = firstFrame;
    k.bandPixels = bandPixels;
    k.rcpBandPixels = 1.0f / float(bandPixels);
    k.rcpWidth = 1.0f / float(s.width);
    return k;
}

// Makes `r` ready for launches of kernel `variant` (a QueryMode or kVariantPath ...) over q, the current
// scene's parameters under layout L (query_scene_params): the kernel's resident blocks per CU, the claim
// counters and, a 4-wide tree, a spill area for every resident lane, set in q.
bool ensure_ray_launch(Ctx &c, RayLaunch &r, const plan::Layout &L, int variant, hippt::QueryParams &q, const char **err) {
    const bool lit = variant >= kVariantLitPath && variant <= kVariantMisRender;
    const bool select = lit && light_select_applies() && c.lightTable;
    // the environment (a path kernel's launches only): the context's copy first, in stream order; the general kernels
    const bool envOn = variant >= kVariantPath && env_applies();
    if (envOn) {
        if (!upload_env(c, err)) return false;
        q.full = 1;
    }
    OccKey occKey;
    occKey.version = S().scene.version, occKey.stackDepth = L.stackDepth, occKey.fmt = L.fmt, occKey.topBytes = L.topBytes;
    occKey.ldsScene = L.ldsScene, occKey.full = q.full != 0;
    occKey.variant = variant;
    occKey.select = select;
    occKey.env = envOn;
    occKey.envs = envOn && lit && env_sampling_applies();
    if (!same_key(r.occKey, occKey)) {
        // (the pointers select the kernel: any non-null scratch the render route's)
        const bool render = variant == kVariantLitRender || variant == kVariantMisRender || variant == kVariantEnvRender;
        hippt::PathParams pp{q, c.mats, nullptr, nullptr, nullptr, 1, lit ? c.lights : nullptr, lit && c.lights ? 1 : 0,
                             variant == kVariantMisPath || variant == kVariantMisRender ? 2 : 1,
                             render ? reinterpret_cast<float *>(c.stats) : nullptr, nullptr};
        if (select) set_light_select(c, pp);
        if (envOn) set_env(c, pp);
        r.blocksPerCu = variant >= kVariantPath ? hippt::path_blocks_per_cu(pp)
                                                : hippt::query_blocks_per_cu(q, hippt::QueryMode(variant));
        r.occKey = occKey;
    }
    if (!r.ctr) HIP_TRY(hipMalloc(&r.ctr, hippt::kQueryCtrBytes));
    if (L.wide) {
        const size_t bytes = size_t(c.cus) * size_t(r.blocksPerCu) * hippt::kMeshBlock * size_t(q.spillCap) * sizeof(int);
        // a render route's earlier batches use the old area (no query is in flight: every call waits for its own)
        if (&r == &c.litLaunch && r.spillBytes < bytes) HIP_TRY(hipStreamSynchronize(c.stream));
        if (!grow(reinterpret_cast<void **>(&r.spill), &r.spillBytes, bytes, "hipMalloc(&r.spill, bytes)", err)) return false;
        q.spill = r.spill;
    }
    q.counter = r.ctr;
    return true;
}

bool query_setup(Ctx &c, const QueryCall &call, hippt::QueryParams &q, const char **err) {
    State &s = S();
    const plan::Layout L = query_scene_params(c, q);
    if (call.camera()) q.cam = query_cam(current_camera(), 0, 1, unsigned(s.width) * unsigned(s.height), call.frame);
    HIP_TRY(hipSetDevice(c.device));
    if (!c.qDone) HIP_TRY(hipEventCreateWithFlags(&c.qDone, hipEventDisableTiming));
    if (call.camRays) return true;  // no traversal: the camera alone
    const int lit = light_sampling_applies();
    const int variant = !call.path ? int(call.mode) : lit == 2 ? kVariantMisPath : lit ? kVariantLitPath : kVariantPath;
    return ensure_ray_launch(c, c.qLaunch, L, variant, q, err);
}

// The ray-per-lane render route: light sampling (HIPPT_OPT_LIGHT_SAMPLING on a scene with a light; DESIGN.md §16;
// mode 1 or 2) and, with or without it (mode 0: plain paths), an environment (hipptSetEnvironment; §19).  Each
// batch is one launch of the path queries' kernel of that mode over the renderer's own camera samples
// (QueryCam: the context's rows of the image, frame-major items as the combine reads them), into the batch
// scratch, combined by the deferred combine.  No chaining, sky rectangle, render pad or item order.  Its
// counters and spill area are the route's own: a batch may still be in flight when a query is made.
bool enqueue_mesh_lights(Ctx &c, const CameraF &cam, int firstFrame, int count, int maxDepth, int mode, const char **err) {
    State &s = S();
    const unsigned bandPixels = unsigned(c.rows) * unsigned(s.width);
    const BatchSize size = frames_per_batch(bandPixels, count);
    hippt::QueryParams q;
    const plan::Layout L = query_scene_params(c, q);
    q.cam = query_cam(cam, c.y0, c.stride, bandPixels, firstFrame);
    RayLaunch &R = c.litLaunch;
    const int variant = mode == 2 ? kVariantMisRender : mode ? kVariantLitRender : kVariantEnvRender;
    if (!ensure_ray_launch(c, R, L, variant, q, err)) return false;
    hippt::PathParams np{q,    c.mats,  nullptr, nullptr, nullptr, maxDepth, mode ? c.lights : nullptr,
                         mode ? int(s.scene.lights.size()) : 0, mode, nullptr, c.stats};
    set_light_select(c, np);
    set_env(c, np);
    s.activeEnv = np.envSize;
    s.activeEnvSampling = np.envRowC ? 1 : 0;
    s.activeLightSelect = np.lightCdf ? light_select_applies() : 0;
    s.activeWidth = L.wide ? 4 : 2;
    s.activeTopBytes = L.topBytes;
    s.activeBlocksPerCu = R.blocksPerCu;
    s.activeChainCap = 0;
    s.activeRenderPad = 0;
    s.activeSkyPixels = 0;
    s.activeLightSampling = mode;
    for (int b = 0; b < count; b += size.frames) {
        const int nf = std::min(size.frames, count - b);
        const unsigned total = bandPixels * unsigned(nf);
        if (!flush_deferred(c, err)) return false;  // (the chain's flush too)
        float *scratch = nullptr;
        if (!batch_scratch(c, size.need, &scratch, err)) return false;
        np.scratch = scratch;
        hippt::QueryParams &bq = np.q;
        bq.cam.firstFrame = firstFrame + b;
        bq.numRays = total;
        bq.firstItem = 0;
        bq.chunk = plan::query_chunk(total);
        s.activeChunk = int(bq.chunk);
        const long long blocks = ray_blocks(c, R.blocksPerCu, total);
        HIP_TRY(hipMemsetAsync(R.ctr, 0, hippt::kQueryCtrBytes, c.stream));
        if (!TIMED_LAUNCH(c, 0, hippt::launch_path(np, int(blocks), c.stream))) return false;
        c.deferred = hippt::CombineParams{c.accum, c.out, scratch, bandPixels, total, firstFrame + b, nf, s.pixelFormat};
        c.hasDeferred = true;
    }
    return true;
}

// Enqueues rays [first, first + m) of a query whose pointers (q.rays, q.t, ...) are already those of
// ray `first`.
bool query_enqueue(Ctx &c, hippt::QueryParams q, unsigned first, unsigned m, const QueryCall &call, const char **err,
                   const PathPtrs &pp = PathPtrs{}) {
    if (call.camRays) {
        HIP_TRY(hippt::launch_camera_rays(hippt::CameraRaysParams{q.cam, pp.outRays, pp.outSeeds, m, first}, c.stream));
        return true;
    }
    q.numRays = m;
    q.firstItem = first;
    q.chunk = plan::query_chunk(m);
    const long long blocks = ray_blocks(c, c.qLaunch.blocksPerCu, m);
    HIP_TRY(hipMemsetAsync(c.qLaunch.ctr, 0, hippt::kQueryCtrBytes, c.stream));
    if (call.path) {
        const int lit = light_sampling_applies();
        hippt::PathParams np{q, c.mats, pp.seeds, pp.radiance, pp.segments, call.maxDepth,
                             lit ? c.lights : nullptr, lit ? int(S().scene.lights.size()) : 0, lit,
                             nullptr, nullptr};
        set_light_select(c, np);
        set_env(c, np);
        HIP_TRY(hippt::launch_path(np, int(blocks), c.stream));
    } else {
        HIP_TRY(hippt::launch_query(q, int(blocks), call.mode, c.stream));
    }
    return true;
}

// Enqueues rays [0, n) of a query whose buffers are device memory, at most kLaunchRays per launch.
bool query_enqueue_device(Ctx &c, const hippt::QueryParams &q0, const QueryCall &call, long long n, const char **err) {
    constexpr long long kLaunchRays = 1LL << 30;
    for (long long at = 0; at < n; at += kLaunchRays) {
        hippt::QueryParams q = q0;
        PathPtrs pp;
        for (int k = 0; k < call.bufs.n; ++k)
            if (call.bufs.b[k].ptr) set_slot(q, pp, call.bufs.b[k].slot, ray_at(call.bufs.b[k], at));
        if (!query_enqueue(c, q, unsigned(at), unsigned(std::min(kLaunchRays, n - at)), call, err, pp)) return false;
    }
    return true;
}

bool query_locked(const QueryCall &call, const char **err) {
    State &s = S();
    const hippt::qlayout::Table &bufs = call.bufs;
    // argument and state checks first: none of them touches the GPU
    const bool pathApi = call.path || call.camRays;  // (their messages name them)
    const std::string who = pathApi ? "path query" : "ray query";
    if (call.path && call.maxDepth < 1) return fail(err, who + ": maxDepth must be at least 1");
    if (call.n < 0) return fail(err, who + ": negative ray count");
    if (!call.camera() && !bufs.ptr(Slot::Rays) && call.n > 0) return fail(err, who + ": null ray buffer");
    if (call.path && !bufs.ptr(Slot::Seeds) && call.n > 0) return fail(err, who + ": null seed buffer");
    if (call.path ? (!bufs.ptr(Slot::Radiance) && call.n > 0) : !bufs.any_out())
        return fail(err, who + ": no output buffer");
    if (call.camera() && call.frame < 0) return fail(err, who + ": negative frame");
    if (pathApi && (call.flags & ~HIPPT_RAYS_DEVICE)) return fail(err, who + ": unknown flags");
    if (s.scene.kind != HIPPT_SCENE_MESH)
        return fail(err, who + ": needs a scene from hipptUploadMesh or hipptUploadScene (the built-in scene has none)");
    if (!s.ready || s.ctxs.empty()) return fail(err, who + ": HIP path tracer not initialized");
    long long n = call.n;
    if (call.camera()) {
        n = (long long)s.width * (long long)s.height;
        if (n > (1LL << 31) - 1) return fail(err, who + ": image too large");
    }
    if (n == 0) return true;
    const bool device = (call.flags & HIPPT_RAYS_DEVICE) != 0;
    if (call.flags & ~HIPPT_RAYS_DEVICE) return fail(err, who + ": unknown flags");
    if (device) {
        // every pointer on the device of one context: the whole batch runs there, unstaged
        const void *ptrs[hippt::qlayout::kMaxBuffers];
        size_t aligns[hippt::qlayout::kMaxBuffers];
        for (int k = 0; k < bufs.n; ++k) ptrs[k] = bufs.b[k].ptr, aligns[k] = bufs.b[k].align;
        int dev = -1;
        if (!device_pointers_ok(who, "HIPPT_RAYS_DEVICE", -1, ptrs, aligns, bufs.n, &dev, err)) return false;
        Ctx *cp = nullptr;
        for (Ctx &c : s.ctxs)
            if (c.device == dev && !cp) cp = &c;
        if (!cp) return fail(err, who + ": the pointers are on a device that is none of hipptSetDevices'");
        Ctx &c = *cp;
        HIP_TRY(hipSetDevice(c.device));
        if (!ensure_scene(c, err)) return false;
        hippt::QueryParams q;
        if (!query_setup(c, call, q, err)) return false;
        if (!query_enqueue_device(c, q, call, n, err)) return false;
        HIP_TRY(hipEventRecord(c.qDone, c.stream));
        HIP_TRY(hipEventSynchronize(c.qDone));
        return true;
    }
    // host memory: contiguous shares over the contexts, each cut into slices staged through the
    // context's buffers (inputs in, results out); slice j of every context is enqueued before slice j + 1
    const long long slice = s.querySlice > 0 ? std::max(64LL, s.querySlice) : (1LL << 22);
    const size_t K = s.ctxs.size();
    std::vector<hippt::QueryParams> qs(K);
    std::vector<char *> stage(K, nullptr);
    const hippt::qlayout::Staging lay = hippt::qlayout::staging(bufs, size_t(std::min(slice, n)));
    for (size_t k = 0; k < K; ++k) {
        Ctx &c = s.ctxs[k];
        if (n * (long long)(k + 1) / (long long)K == n * (long long)k / (long long)K) continue;  // an empty share
        HIP_TRY(hipSetDevice(c.device));
        if (!ensure_scene(c, err)) return false;
        if (!query_setup(c, call, qs[k], err)) return false;
        if (!grow(&c.qStage, &c.qStageBytes, lay.total, "hipMalloc(&c.qStage, stageBytes)", err)) return false;
        stage[k] = static_cast<char *>(c.qStage);
    }
    bool left = true;
    for (long long j = 0; left; ++j) {
        left = false;
        for (size_t k = 0; k < K; ++k) {
            const long long a = n * (long long)k / (long long)K, b = n * (long long)(k + 1) / (long long)K;
            const long long at = a + j * slice;
            if (at >= b) continue;
            left = true;
            Ctx &c = s.ctxs[k];
            const unsigned m = unsigned(std::min(slice, b - at));
            HIP_TRY(hipSetDevice(c.device));
            hippt::QueryParams q = qs[k];
            PathPtrs pp;
            for (int i = 0; i < bufs.n; ++i) {
                const hippt::qlayout::Buffer &bf = bufs.b[i];
                if (!bf.ptr) continue;
                char *const dev = stage[k] + lay.off[i];
                if (!bf.out) HIP_TRY(hipMemcpyAsync(dev, ray_at(bf, at), m * bf.bytesPerRay, hipMemcpyHostToDevice, c.stream));
                set_slot(q, pp, bf.slot, dev);
            }
            if (!query_enqueue(c, q, unsigned(at), m, call, err, pp)) return false;
            for (int i = 0; i < bufs.n; ++i) {
                const hippt::qlayout::Buffer &bf = bufs.b[i];
                if (bf.ptr && bf.out)
                    HIP_TRY(hipMemcpyAsync(ray_at(bf, at), stage[k] + lay.off[i], m * bf.bytesPerRay, hipMemcpyDeviceToHost,
                                           c.stream));
            }
        }
    }
    for (size_t k = 0; k < K; ++k) {
        if (!stage[k]) continue;
        Ctx &c = s.ctxs[k];
        HIP_TRY(hipSetDevice(c.device));
        HIP_TRY(hipEventRecord(c.qDone, c.stream));
    }
    for (size_t k = 0; k < K; ++k)
        if (stage[k]) HIP_TRY(hipEventSynchronize(s.ctxs[k].qDone));
    return true;
}

// ---- denoiser (hippt_denoise.hip; include/hippt.h hipptDenoise) ----
// Input side as hipptReadback: the image's readers' flush, then the accumulation.  Everything after
// that goes on the context's stream and writes the context's denoiser buffer and the caller's outputs
// only: the guide sample's camera hit records (the ray queries' own launch, into the buffer), prepare,
// the passes between two colour buffers, finish; the call waits for its own event, as queries do.
bool denoise_locked(const hipptDenoiseParams *params, unsigned int *pixels, float *rgba, const char **err) {
    State &s = S();
    hipptDenoiseParams P;
    hipptDenoiseDefaults(&P);
    if (params) P = *params;
    // argument and state checks first: none of them touches the GPU
    if (P.passes < 0 || P.passes > hippt::kDenoiseMaxPasses) return fail(err, "denoise: passes out of range (0..8)");
    if (P.guideFrame < 0) return fail(err, "denoise: negative guide frame");
    if (P.normalPower < 0 || P.normalPower > hippt::kDenoiseMaxNormalPower)
        return fail(err, "denoise: normal power out of range (0..10)");
    if (!(P.sigmaColor > 0.0f) || !std::isfinite(P.sigmaColor)) return fail(err, "denoise: sigmaColor must be positive and finite");
    if (!(P.sigmaDepth > 0.0f) || !std::isfinite(P.sigmaDepth)) return fail(err, "denoise: sigmaDepth must be positive and finite");
    if (P.flags & ~(HIPPT_DENOISE_NO_DEMODULATE | HIPPT_DENOISE_DEVICE)) return fail(err, "denoise: unknown flags");
    if (P.reserved[0] != 0.0f || P.reserved[1] != 0.0f) return fail(err, "denoise: reserved fields must be 0");
    if (!pixels && !rgba) return fail(err, "denoise: no output buffer");
    if (s.scene.kind != HIPPT_SCENE_MESH)
        return fail(err, "denoise: needs a scene from hipptUploadMesh or hipptUploadScene (the built-in scene has no hit records)");
    if (!s.ready || s.ctxs.empty()) return fail(err, "denoise: HIP path tracer not initialized");
    if (s.ctxs.size() != 1) return fail(err, "denoise: needs the whole image on one device (more than one device is set)");
    Ctx &c = s.ctxs[0];
    if (c.y0 != 0 || c.stride != 1 || c.rows != s.height)
        return fail(err, "denoise: needs every row of the image (a row range or a row interleave is set)");
    const long long n = (long long)s.width * (long long)s.height;
    if (n > (1LL << 31) - 1) return fail(err, "denoise: image too large");
    const bool device = (P.flags & HIPPT_DENOISE_DEVICE) != 0;
    if (device) {
        const void *ptrs[2] = {pixels, rgba};
        const size_t aligns[2] = {4, 16};
        if (!device_pointers_ok("denoise", "HIPPT_DENOISE_DEVICE", c.device, ptrs, aligns, 2, nullptr, err)) return false;
    }
    if (!sync_locked(err)) return false;
    HIP_TRY(hipSetDevice(c.device));
    if (!ensure_scene(c, err)) return false;
    const size_t px = size_t(n);
    const size_t bytes = px * 80;
    // (no denoise is in flight: every call waits for its own)
    if (!grow(&c.dnBuf, &c.dnBytes, bytes, "hipMalloc(&c.dnBuf, bytes)", err)) return false;
    float4 *const hits = static_cast<float4 *>(c.dnBuf);  // 2 per pixel
    float4 *col[2] = {hits + 2 * px, hits + 3 * px};
    float4 *const guide = hits + 4 * px;
    const bool timing = s.denoiseTiming;
    if (timing)
        while (c.dnEv.size() < size_t(hippt::kDenoiseStages) + 1) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            c.dnEv.push_back(e);
        }
    int marks = 0;  // events recorded so far: stageOf[m] ran between events m and m + 1
    int stageOf[hippt::kDenoiseStages] = {};
    auto mark = [&](int stage) -> bool {  // closes `stage` (-1: opens the first)
        if (!timing) return true;
        HIP_TRY(hipEventRecord(c.dnEv[size_t(marks)], c.stream));
        if (stage >= 0) stageOf[marks - 1] = stage;
        ++marks;
        return true;
    };
    if (!mark(-1)) return false;
    // the guides: sample guideFrame's camera hit records
    const QueryCall call = query_call(QueryMode::CameraHits, 0, P.guideFrame, 0, {{Slot::Hits, hits}});
    hippt::QueryParams q;
    if (!query_setup(c, call, q, err)) return false;
    if (!query_enqueue_device(c, q, call, n, err)) return false;
    if (!mark(0)) return false;
    const int demodulate = (P.flags & HIPPT_DENOISE_NO_DEMODULATE) ? 0 : 1;
    HIP_TRY(hippt::launch_denoise_prepare(
        hippt::DenoisePrepareParams{c.accum, hits, c.mats, col[0], guide, unsigned(n), demodulate}, c.stream));
    if (!mark(1)) return false;
    int cur = 0;
    for (int k = 0; k < P.passes; ++k) {
        const float fs = float(1 << k);
        const float sigma = P.sigmaColor * (1.0f / fs);
        hippt::DenoisePassParams pp{col[cur], guide, col[cur ^ 1], s.width, s.height, k, P.normalPower,
                                    sigma * sigma, fs, P.sigmaDepth};
        HIP_TRY(hippt::launch_denoise_pass(pp, c.stream));
        cur ^= 1;
        if (!mark(2 + k)) return false;
    }
    // host outputs are staged in what the passes no longer need: rgba in the other colour buffer, the
    // words in the guide
    float4 *const drgba = rgba ? (device ? reinterpret_cast<float4 *>(rgba) : col[cur ^ 1]) : nullptr;
    uint32_t *const dwords = pixels ? (device ? pixels : reinterpret_cast<uint32_t *>(guide)) : nullptr;
    HIP_TRY(hippt::launch_denoise_finish(
        hippt::DenoiseFinishParams{col[cur], hits, c.mats, drgba, dwords, unsigned(n), demodulate, s.pixelFormat}, c.stream));
    if (!mark(2 + hippt::kDenoiseMaxPasses)) return false;
    if (!device) {
        if (rgba) HIP_TRY(hipMemcpyAsync(rgba, drgba, px * sizeof(float4), hipMemcpyDeviceToHost, c.stream));
        if (pixels) HIP_TRY(hipMemcpyAsync(pixels, dwords, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    }
    if (!c.qDone) HIP_TRY(hipEventCreateWithFlags(&c.qDone, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c.qDone, c.stream));
    HIP_TRY(hipEventSynchronize(c.qDone));
    if (timing) {
        for (long long &v : s.denoiseNs) v = 0;
        for (int m = 0; m + 1 < marks; ++m) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, c.dnEv[size_t(m)], c.dnEv[size_t(m) + 1]));
            s.denoiseNs[stageOf[m]] = (long long)std::llround(double(ms) * 1e6);
        }
    }
    return true;
}

}  // namespace

// ---- reference ABI ----------------------------------------------------------------------------
extern "C" bool cudaPathTracerInit(int width, int height, const char **errorMessage) {
    return abi_bool(kLocked, errorMessage, [&]() -> bool {
        return init_locked(width, height, errorMessage);
    });
}

extern "C" bool cudaPathTracerRender(int frameIndex, int maxDepth, const unsigned int **hostPixels,
                                     const char **errorMessage) {
    return abi_bool(kLocked, errorMessage, [&]() -> bool {
        // the CUDA backend's ABI always hands out its ARGB words (HIPPT_OPT_PIXEL_FORMAT applies to
        // the hippt* render calls)
        // (restored on every way out, an exception caught below included: ADVICE r4)
        struct FormatScope {
            int &fmt;
            const int saved;
            ~FormatScope() { fmt = saved; }
        } scope{S().pixelFormat, S().pixelFormat};
        scope.fmt = HIPPT_PIXEL_ARGB;
        return render_locked(frameIndex, 1, maxDepth, hostPixels, errorMessage);
    });
}

extern "C" void cudaPathTracerShutdown(void) {
    abi_void(kLocked, [&] {
        destroy_all();
    });
}

extern "C" bool hipPathTracerInit(int width, int height, const char **errorMessage) {
    return abi_bool(kUnlocked, errorMessage, [&]() -> bool {
        return cudaPathTracerInit(width, height, errorMessage);
    });
}
extern "C" bool hipPathTracerRender(int frameIndex, int maxDepth, const unsigned int **hostPixels,
                                    const char **errorMessage) {
    return abi_bool(kUnlocked, errorMessage, [&]() -> bool {
        return cudaPathTracerRender(frameIndex, maxDepth, hostPixels, errorMessage);
    });
}
extern "C" void hipPathTracerShutdown(void) { cudaPathTracerShutdown(); }

// ---- scene --------------------------------------------------------------------------------------
extern "C" void hipptBuildCamera(const double lookfrom[3], const double lookat[3], const double vup[3],
                                 double vfovDeg, double aspect, double aperture, double focusDist, hipptCamera *out) {
    abi_void(kUnlocked, [&] {
        static_assert(sizeof(hipptCamera) == sizeof(CameraF), "camera layout");
        CameraF c;
        build_camera(lookfrom, lookat, vup, vfovDeg, aspect, aperture, focusDist, c);
        std::memcpy(out, &c, sizeof(c));
    });
}

extern "C" bool hipptUseBuiltinScene(int sceneId, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        if (sceneId != HIPPT_SCENE_SPHERE4) return fail(err, "unknown built-in scene id");
        // a pending mesh combine belongs to the image rendered so far: enqueue it before the switch
        for (Ctx &c : S().ctxs)
            if (!flush_deferred(c, err)) return false;
        S().scene.kind = HIPPT_SCENE_SPHERE4;
        return true;
    });
}

namespace {
bool upload_scene_locked(const float *verts, const int *triMaterial, int numTris, const float *spheres,
                                 const int *sphereMaterial, int numSpheres, const hipptMaterial *materials,
                                 int numMaterials, const double lookfrom[3], const double lookat[3],
                                 const double vup[3], double vfovDeg, double aperture, double focusDist,
                                 const char **err) {
    State &s = S();
    if (numTris < 0 || numSpheres < 0) return fail(err, "negative primitive count");
    if ((numTris > 0 && (!verts || !triMaterial)) || (numSpheres > 0 && (!spheres || !sphereMaterial)) ||
        !materials || !lookfrom || !lookat || !vup)
        return fail(err, "null scene pointer");
    if (numMaterials <= 0) return fail(err, "scene needs at least one material");
    if (numTris + (long long)numSpheres >= (1LL << 27)) return fail(err, "too many primitives");
    for (int i = 0; i < numTris; ++i)
        if (triMaterial[i] < 0 || triMaterial[i] >= numMaterials) return fail(err, "triangle material out of range");
    for (int j = 0; j < numSpheres; ++j) {
        if (sphereMaterial[j] < 0 || sphereMaterial[j] >= numMaterials) return fail(err, "sphere material out of range");
        for (int a = 0; a < 4; ++a)
            if (!std::isfinite(spheres[4 * j + a])) return fail(err, "non-finite sphere");
    }
    bool full = numSpheres > 0, emissive = false;
    for (int m = 0; m < numMaterials; ++m) {
        const hipptMaterial &mt = materials[m];
        if (mt.kind < HIPPT_MAT_LAMBERTIAN || mt.kind > HIPPT_MAT_EMISSIVE) return fail(err, "unknown material kind");
        if (!std::isfinite(mt.albedo[0]) || !std::isfinite(mt.albedo[1]) || !std::isfinite(mt.albedo[2]) ||
            !std::isfinite(mt.fuzz) || !std::isfinite(mt.ir))
            return fail(err, "non-finite material parameter");
        // an emissive material's albedo words are its radiance: >= 0, may exceed 1
        if (mt.kind == HIPPT_MAT_EMISSIVE && (mt.albedo[0] < 0.0f || mt.albedo[1] < 0.0f || mt.albedo[2] < 0.0f))
            return fail(err, "negative emission component");
        full = full || mt.kind != HIPPT_MAT_LAMBERTIAN;
        emissive = emissive || mt.kind == HIPPT_MAT_EMISSIVE;
    }
    // primitive id p: triangles 0..numTris-1, then spheres (the closest-hit tie order)
    const int numPrims = numTris + numSpheres;
    std::vector<float> boxes(size_t(numPrims) * 6);
    triangle_boxes(verts, numTris, boxes.data());
    for (int j = 0; j < numSpheres; ++j) sphere_box(spheres + 4 * size_t(j), &boxes[6 * size_t(numTris + j)]);
    float extent = 0.0f;
    for (int i = 0; i < 3; ++i) extent = std::max(extent, float(std::fabs(lookfrom[i])));
    hippt::Bvh bvh;
    std::string msg;
    if (!hippt::build_bvh_boxes(boxes.data(), numPrims, extent, bvh, msg, s.bvh)) return fail(err, msg);
    SceneHost sc;  // the new scene, swapped in at the end (a failure keeps the old one)
    sc.version = s.scene.version;
    sc.nodes.assign(bvh.nodes.size() / 4, float4{});
    std::memcpy(sc.nodes.data(), bvh.nodes.data(), bvh.nodes.size() * sizeof(uint32_t));
    hippt::Bvh4 bvh4;
    hippt::collapse_bvh4(bvh, bvh4, s.bvh);
    if (s.bvh.collapse == -1) {
        // Automatic collapse: the SAH-optimal 4-wide tree for scenes that fit the LDS scene copy
        // (leaves of <= 2 primitives: Cornell +1.6-1.9%, cornell_mixed +1.0%, r3ap/r3aq), the
        // greedy one for trees read from global memory (SAH-optimal: blob70k -9%, random_scene -4%)
        auto fits = [&](const hippt::Bvh4 &b) {
            return plan::fits_lds_scene(int(b.nodes.size() / hippt::kNode4Words), numPrims, true, numMaterials,
                                        lds_limits().scene);
        };
        if (fits(bvh4)) {
            hippt::BvhParams p = s.bvh;
            p.collapse = 1;
            hippt::Bvh4 sah;
            hippt::collapse_bvh4(bvh, sah, p);
            if (fits(sah)) bvh4 = std::move(sah);
        }
    }
    hippt::order_bvh4_top(bvh4, plan::kTopOrderNodes);
    sc.nodes4.assign(bvh4.nodes.size() / 4, float4{});
    std::memcpy(sc.nodes4.data(), bvh4.nodes.data(), bvh4.nodes.size() * sizeof(uint32_t));
    sc.numNodes4 = int(bvh4.nodes.size() / hippt::kNode4Words);
    std::vector<uint32_t> q;
    (void)hippt::quantize_bvh4(bvh4, q);  // empty on failure: the float nodes serve every path
    sc.nodes4q.assign(q.size() / 4, float4{});
    std::memcpy(sc.nodes4q.data(), q.data(), q.size() * sizeof(uint32_t));
    sc.bvh4 = bvh4;
    sc.q4 = q;
    sc.hybrid.clear();
    sc.hybridTop = -1;
    if (bvh4.nodes.size() / hippt::kNode4Words >= (1u << 24)) return fail(err, "4-wide BVH too large (2^24 nodes)");
    // device layouts of the 4-wide trees: an interior child's code is its node's BYTE offset (the
    // kernels address a node without a multiply; leaf codes and the root, 0, are unchanged)
    auto byte_codes = [](std::vector<float4> &v, int nodeWords, int codeWord, int stride) {
        auto *w = reinterpret_cast<int32_t *>(v.data());
        const size_t n = v.size() * 4 / size_t(nodeWords);
        for (size_t k = 0; k < n; ++k)
            for (int i = 0; i < 4; ++i) {
                int32_t &c = w[k * size_t(nodeWords) + size_t(codeWord + i)];
                if (c >= 0) c *= stride;
            }
    };
    byte_codes(sc.nodes4, hippt::kNode4Words, 24, hippt::kNode4Words * 4);
    byte_codes(sc.nodes4q, hippt::kNode4QWords, 12, hippt::kNode4QWords * 4);
    sc.nodes4f.clear();
    sc.halfState = 0;
    sc.levels4 = bvh4.levels;
    sc.stackBound4 = bvh4.stackBound;
    sc.tris.assign(size_t(numPrims) * 3, float4{});
    sc.shade.assign(size_t(numPrims), float4{});
    for (int k = 0; k < numPrims; ++k) {
        const int id = bvh.order[size_t(k)];
        if (id >= numTris) {  // sphere: (center, r) (r^2) (-, id, tag 1); shade (center, mat | flag)
            const float *q = spheres + 4 * size_t(id - numTris);
            sc.tris[3 * size_t(k)] = float4{q[0], q[1], q[2], q[3]};
            sc.tris[3 * size_t(k) + 1] = float4{q[3] * q[3], 0.0f, 0.0f, 0.0f};
            sc.tris[3 * size_t(k) + 2] = float4{0.0f, as_float(id), as_float(1), 0.0f};
            sc.shade[size_t(k)] =
                float4{q[0], q[1], q[2], as_float(sphereMaterial[id - numTris] | hippt::kShadeSphere)};
            continue;
        }
        sc.shade[size_t(k)].w = as_float(triMaterial[id]);
        tri_record(verts + 9 * size_t(id), id, &sc.tris[3 * size_t(k)], sc.shade[size_t(k)]);
    }
    // what hipptUpdateVertices needs: the level lists and the pad's seed (extent hint and sphere boxes)
    hippt::refit_plan(bvh, bvh4, sc.plan);
    sc.numTriangles = numTris;
    sc.extent = extent;
    sc.pad = bvh.pad;
    sc.minEdgeSine = min_edge_sine(verts, numTris);
    sc.padSeed = std::fabs(extent);
    for (size_t k = size_t(numTris) * 6; k < boxes.size(); ++k) sc.padSeed = std::max(sc.padSeed, std::fabs(boxes[k]));
    sc.geomRev = s.scene.geomRev + 1;
    sc.bvh2 = std::move(bvh);
    sc.mats.assign(size_t(numMaterials) * 2, float4{});
    for (int m = 0; m < numMaterials; ++m) {
        const hipptMaterial &mt = materials[m];
        // Metal(a, f): fuzz(f < 1 ? f : 1), RayTracer.h:494
        const float fuzz = mt.kind == HIPPT_MAT_METAL && !(mt.fuzz < 1.0f) ? 1.0f : mt.fuzz;
        sc.mats[2 * size_t(m)] = float4{mt.albedo[0], mt.albedo[1], mt.albedo[2], as_float(mt.kind)};
        sc.mats[2 * size_t(m) + 1] = float4{fuzz, mt.ir, 0.0f, 0.0f};
    }
    sc.numTris = numPrims;
    sc.numNodes = int(sc.bvh2.nodes.size() / hippt::kNodeWords);
    sc.levels = sc.bvh2.levels;
    sc.full = full;
    sc.emissive = emissive;
    // the light list (HIPPT_OPT_LIGHT_SAMPLING): leaf-order indices of the emissive primitives by ascending id
    {
        std::vector<std::pair<int, int>> byId;
        for (int k = 0; k < numPrims; ++k) {
            const int id = sc.bvh2.order[size_t(k)];
            const int m = id >= numTris ? sphereMaterial[id - numTris] : triMaterial[id];
            if (materials[m].kind == HIPPT_MAT_EMISSIVE) byId.emplace_back(id, k);
        }
        std::sort(byId.begin(), byId.end());
        for (const auto &e : byId) sc.lights.push_back(e.second);
    }
    for (int i = 0; i < 3; ++i) {
        sc.lookfrom[i] = lookfrom[i];
        sc.lookat[i] = lookat[i];
        sc.vup[i] = vup[i];
    }
    sc.vfov = vfovDeg;
    sc.aperture = aperture;
    sc.focus = focusDist;
    sc.rawCamera = false;
    sc.kind = HIPPT_SCENE_MESH;
    ++sc.version;
    s.scene = std::move(sc);
    s.upd.hostStale = false;  // (an update of the replaced scene)
    return true;
}
}  // namespace

extern "C" bool hipptUploadScene(const float *verts, const int *triMaterial, int numTris, const float *spheres,
                                 const int *sphereMaterial, int numSpheres, const hipptMaterial *materials,
                                 int numMaterials, const double lookfrom[3], const double lookat[3],
                                 const double vup[3], double vfovDeg, double aperture, double focusDist,
                                 const char **err) {
    return abi_bool(kLocked, err, [&] {
        return upload_scene_locked(verts, triMaterial, numTris, spheres, sphereMaterial, numSpheres, materials, numMaterials,
                                   lookfrom, lookat, vup, vfovDeg, aperture, focusDist, err);
    });
}

extern "C" bool hipptUploadMesh(const float *verts, const int *triMaterial, int numTris, const float *albedo,
                                int numMaterials, const double lookfrom[3], const double lookat[3],
                                const double vup[3], double vfovDeg, double aperture, double focusDist,
                                const char **err) {
    return abi_bool(kUnlocked, err, [&]() -> bool {
        if (!albedo) return fail(err, "null scene pointer");
        if (numTris <= 0) return fail(err, "BVH requires at least one triangle");
        std::vector<hipptMaterial> mats(size_t(std::max(0, numMaterials)));
        for (int m = 0; m < numMaterials; ++m)
            mats[size_t(m)] = hipptMaterial{HIPPT_MAT_LAMBERTIAN, {albedo[3 * m], albedo[3 * m + 1], albedo[3 * m + 2]}, 0.0f,
                                            1.0f};
        return hipptUploadScene(verts, triMaterial, numTris, nullptr, nullptr, 0, mats.data(), numMaterials, lookfrom,
                                lookat, vup, vfovDeg, aperture, focusDist, err);
    });
}

// ---- vertex updates --------------------------------------------------------------------------------
namespace {

// The refit's buffers of context c for the uploaded scene (first update of the scene there).
bool ensure_refit_buffers(Ctx &c, const char **err) {
    const SceneHost &sc = S().scene;
    if (c.rfWords) return true;
    const size_t n2 = size_t(sc.numNodes), n4 = size_t(sc.numNodes4), np = size_t(sc.numTris);
    HIP_TRY(hipMalloc(&c.rfVerts, std::max<size_t>(1, size_t(sc.numTriangles) * 9) * sizeof(float)));
    HIP_TRY(hipMalloc(&c.rfBoxes, (np * 6 + n2 * 12 + n4 * 24) * sizeof(float)));
    HIP_TRY(hipMalloc(&c.rfLists, std::max<size_t>(1, n2 + n4) * sizeof(int)));
    HIP_TRY(hipMalloc(&c.rfWords, 2 * sizeof(unsigned)));
    // fresh buffers: the copies need not wait for the launches queued on the context's stream
    HIP_TRY(hipMemcpy(c.rfLists, sc.plan.list2.data(), sc.plan.list2.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c.rfLists + n2, sc.plan.list4.data(), sc.plan.list4.size() * sizeof(int), hipMemcpyHostToDevice));
    return true;
}

bool update_vertices_locked(const float *verts, int numTris, int flags, const char **err) {
    State &s = S();
    SceneHost &sc = s.scene;
    State::Update &u = s.upd;
    // argument and state checks first: none of them touches the GPU
    if (s.scene.kind != HIPPT_SCENE_MESH)
        return fail(err, s.scene.version == 0 ? "vertex update: no mesh scene (hipptUploadMesh or hipptUploadScene first)"
                                              : "vertex update: the built-in scene is active");
    if (flags & ~HIPPT_VERTS_DEVICE) return fail(err, "vertex update: unknown flags");
    if (numTris != sc.numTriangles) return fail(err, "vertex update: numTris differs from the uploaded scene's");
    if (numTris <= 0) return fail(err, "vertex update: the uploaded scene has no triangles");
    if (!verts) return fail(err, "vertex update: null vertex pointer");
    const bool device = (flags & HIPPT_VERTS_DEVICE) != 0;
    const size_t floats = size_t(numTris) * 9;
    if (device && (!s.ready || s.ctxs.empty()))
        return fail(err, "vertex update: HIPPT_VERTS_DEVICE needs an initialized path tracer");
    if (!device)
        for (size_t k = 0; k < floats; ++k)
            if (!std::isfinite(verts[k])) return fail(err, "vertex update: non-finite vertex coordinate");
    if (!s.ready || s.ctxs.empty()) {  // no device yet: the host copy only, which the next Init uploads
        settle_scene();
        refit_scene_host(sc, verts);
        drop_derived_trees(sc);
        ++sc.geomRev;
        return true;
    }
    Ctx *owner = nullptr;  // device vertices: the first context of the memory's device
    if (device) {
        hipPointerAttribute_t a{};
        if (hipPointerGetAttributes(&a, verts) != hipSuccess || a.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return fail(err, "vertex update: HIPPT_VERTS_DEVICE needs a device memory pointer");
        }
        for (Ctx &c : s.ctxs)
            if (c.device == a.device && !owner) owner = &c;
        if (!owner) return fail(err, "vertex update: the vertices are on a device that is none of hipptSetDevices'");
    }
    // the staging array of this update: pinned, shared by every device; the one before the last
    // update's, whose copies are long done in a pipeline one update deep
    if (u.floats != floats) {
        stage_wait(0);
        stage_wait(1);
        settle_scene();
        for (float *&p : u.stage) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
        }
        u.floats = 0;
        for (float *&p : u.stage)
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p), floats * sizeof(float), hipHostMallocPortable));
        u.floats = floats;
    }
    const int b = u.next;
    u.next ^= 1;
    stage_wait(b);
    auto record = [&](Ctx &c, hipEvent_t *out) -> bool {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        u.busy[b].push_back({c.device, e});
        HIP_TRY(hipEventRecord(e, c.stream));
        if (out) *out = e;
        return true;
    };
    hipEvent_t staged = nullptr;  // device vertices: their copy into the staging array
    if (device) {
        HIP_TRY(hipSetDevice(owner->device));
        HIP_TRY(hipMemcpyAsync(u.stage[b], verts, floats * sizeof(float), hipMemcpyDeviceToHost, owner->stream));
        if (!record(*owner, &staged)) return false;
    } else {
        std::memcpy(u.stage[b], verts, floats * sizeof(float));  // the caller may reuse its array at once
    }
    // the host copy follows when something on the host reads it (settle_scene); every path reads the
    // float nodes from here on
    // (the render pad's precondition: known at once for host vertices, with the host copy for others)
    sc.minEdgeSine = device ? 0.0f : min_edge_sine(verts, numTris);
    u.hostStale = true;
    u.staleBuf = b;
    u.staleEv = staged;
    drop_derived_trees(sc);
    ++sc.geomRev;
    unsigned seedBits;
    std::memcpy(&seedBits, &sc.padSeed, 4);
    for (Ctx &c : s.ctxs) {
        // a context that has not uploaded this scene yet uploads the settled host copy when it renders
        if (c.sceneVersion != sc.version) continue;
        HIP_TRY(hipSetDevice(c.device));
        // Pending work is closed first: the held batches launched and the open chained run ended (its
        // flush enqueued), so that no persistent launch of the run goes on with a batch posted behind
        // the update; the next batch opens a new run (Ctx::Chain::geomRev).  The deferred combine
        // stays deferred: it reads no geometry.
        if (!flush_chain(c, err)) return false;
        if (!ensure_refit_buffers(c, err)) return false;
        const float *dv = verts;
        if (!device || c.device != owner->device) {
            if (staged && &c != owner) HIP_TRY(hipStreamWaitEvent(c.stream, staged, 0));
            HIP_TRY(hipMemcpyAsync(c.rfVerts, u.stage[b], floats * sizeof(float), hipMemcpyHostToDevice, c.stream));
            if (!record(c, nullptr)) return false;
            dv = c.rfVerts;
        }
        hippt::RefitBuffers r{};
        r.verts = dv;
        r.tris = c.tris;
        r.shade = c.shade;
        r.nodes2 = reinterpret_cast<uint32_t *>(c.nodes);
        r.nodes4 = reinterpret_cast<uint32_t *>(c.nodes4);
        r.pbox = c.rfBoxes;
        r.ubox2 = r.pbox + size_t(sc.numTris) * 6;
        r.ubox4 = r.ubox2 + size_t(sc.numNodes) * 12;
        r.words = c.rfWords;
        r.padOut = c.padDev;
        r.list2 = c.rfLists;
        r.list4 = c.rfLists + sc.numNodes;
        r.numPrims = sc.numTris;
        r.numTris = sc.numTriangles;
        r.numNodes2 = sc.numNodes;
        r.numNodes4 = sc.numNodes4;
        HIP_TRY(hippt::launch_refit(r, sc.plan.level2, sc.plan.level4, seedBits, c.stream));
        // the light selection table follows the new areas, behind the refit on the same stream
        if (!enqueue_light_table(c, err)) return false;
        c.rfUpdated = true;
    }
    return true;
}

}  // namespace

extern "C" bool hipptUpdateVertices(const float *verts, int numTris, int flags, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        return update_vertices_locked(verts, numTris, flags, err);
    });
}

extern "C" long long hipptSceneDownload(int what, void *dst, long long bytes, const char **err) {
    return abi_guard(
        kLocked,
        [&]() -> long long {
            State &s = S();
            auto bad = [&](const char *m) -> long long { return (fail(err, m), -1); };
            if (what == HIPPT_SCENE_ENVIRONMENT) {  // (not the scene's: whatever scene is current)
                const size_t envBytes = s.env.size() * sizeof(hippt::env::Texel);
                if (!envBytes || !dst) return (long long)envBytes;
                if (bytes < (long long)envBytes) return bad("scene download: destination too small");
                if (!s.ready || s.ctxs.empty()) return bad("scene download: HIP path tracer not initialized");
                Ctx &c = s.ctxs[0];
                if (!upload_env(c, err)) return -1;
                if (hipSetDevice(c.device) != hipSuccess ||
                    hipMemcpyAsync(dst, c.env, envBytes, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
                    hipStreamSynchronize(c.stream) != hipSuccess) {
                    (void)hipGetLastError();
                    return bad("scene download: copy failed");
                }
                return (long long)envBytes;
            }
            if (what == HIPPT_SCENE_ENV_TABLE) {  // rows (m, C), then texels (q, c, bits of k): include/hippt.h
                const size_t n = size_t(s.envSize);
                const size_t tabBytes = (2 * n + 3 * n * n) * sizeof(unsigned);
                if (!tabBytes || !dst) return (long long)tabBytes;
                if (bytes < (long long)tabBytes) return bad("scene download: destination too small");
                if (!s.ready || s.ctxs.empty()) return bad("scene download: HIP path tracer not initialized");
                Ctx &c = s.ctxs[0];
                if (!upload_env(c, err)) return -1;
                std::vector<unsigned> dev(hippt::env_table_words(n));
                if (hipSetDevice(c.device) != hipSuccess ||
                    hipMemcpyAsync(dev.data(), c.envTable, dev.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c.stream) !=
                        hipSuccess ||
                    hipStreamSynchronize(c.stream) != hipSuccess) {
                    (void)hipGetLastError();
                    return bad("scene download: copy failed");
                }
                unsigned *out = static_cast<unsigned *>(dst);
                const unsigned *tex = dev.data(), *rowC = tex + 2 * n * n, *rowM = rowC + n;
                for (size_t y = 0; y < n; ++y) {
                    out[2 * y] = rowM[y];
                    out[2 * y + 1] = rowC[y];
                }
                out += 2 * n;
                for (size_t y = 0; y < n; ++y)
                    for (size_t x = 0; x < n; ++x) {
                        const size_t i = y * n + x;
                        out[3 * i] = tex[2 * i] - (x ? tex[2 * (i - 1)] : 0u);
                        out[3 * i + 1] = tex[2 * i];
                        out[3 * i + 2] = tex[2 * i + 1];
                    }
                return (long long)tabBytes;
            }
            if (s.scene.kind != HIPPT_SCENE_MESH) return bad("scene download: no mesh scene");
            const SceneHost &sc = s.scene;
            size_t need = 0;
            switch (what) {
            case HIPPT_SCENE_NODES2: need = sc.nodes.size(); break;
            case HIPPT_SCENE_NODES4: need = sc.nodes4.size(); break;
            case HIPPT_SCENE_PRIMS: need = sc.tris.size(); break;
            case HIPPT_SCENE_SHADE: need = sc.shade.size(); break;
            case HIPPT_SCENE_LIGHTS:  // one record of 4 words per light; none without a table
                need = hippt::light_table_fits(sc.lights.size()) ? sc.lights.size() : 0;
                if (!need) return 0;
                break;
            default: return bad("scene download: unknown buffer");
            }
            need *= sizeof(float4);
            if (!dst) return (long long)need;
            if (bytes < (long long)need) return bad("scene download: destination too small");
            if (!s.ready || s.ctxs.empty()) return bad("scene download: HIP path tracer not initialized");
            Ctx &c = s.ctxs[0];
            if (!ensure_scene(c, err)) return -1;
            if (!launch_held(c, err)) return -1;
            const float4 *src = what == HIPPT_SCENE_NODES2   ? c.nodes
                                : what == HIPPT_SCENE_NODES4 ? c.nodes4
                                : what == HIPPT_SCENE_PRIMS  ? c.tris
                                : what == HIPPT_SCENE_SHADE  ? c.shade
                                                             : nullptr;
            if (what == HIPPT_SCENE_LIGHTS) {  // (built with the scene and behind every update: current here)
                if (!c.lightTable) return bad("scene download: no light table");
                src = reinterpret_cast<const float4 *>(
                    hippt::light_table_buffers(c.lightTable, int(sc.lights.size()), sc.numTris).records);
            }
            if (hipSetDevice(c.device) != hipSuccess ||
                hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
                hipStreamSynchronize(c.stream) != hipSuccess) {
                (void)hipGetLastError();
                return bad("scene download: copy failed");
            }
            return (long long)need;
        },
        [err](const char *what) { return (fail_free(err, what), -1LL); });
}

// ---- environment ---------------------------------------------------------------------------------
namespace {
bool set_environment_locked(const float *texels, int size, int flags, const char **err) {
    State &s = S();
    const std::string who = "environment";
    // argument checks first: none of them touches the GPU, and a rejected call changes nothing
    if (flags & ~HIPPT_ENV_DEVICE) return fail(err, who + ": unknown flags");
    if (!texels && size == 0) {  // remove: the sky gradient again
        s.env.clear();
        s.env.shrink_to_fit();
        s.envSize = 0;
        ++s.envRev;
        return true;
    }
    if (size < 1 || size > hippt::env::kMaxSize)
        return fail(err, who + ": size must be in 1.." + std::to_string(hippt::env::kMaxSize));
    if (!texels) return fail(err, who + ": null texels");
    const size_t count = size_t(size) * size_t(size);
    std::vector<float> fetched;
    if (flags & HIPPT_ENV_DEVICE) {
        if (!s.ready || s.ctxs.empty()) return fail(err, who + ": HIPPT_ENV_DEVICE needs an initialized path tracer");
        const void *ptr = texels;
        const size_t align = sizeof(float);
        int dev = -1;
        if (!device_pointers_ok(who, "HIPPT_ENV_DEVICE", -1, &ptr, &align, 1, &dev, err)) return false;
        bool ours = false;
        for (const Ctx &c : s.ctxs) ours = ours || c.device == dev;
        if (!ours) return fail(err, who + ": the pointer is on a device that is none of hipptSetDevices'");
        // the host copy fetches it (not inspected: what the device holds is what the paths see)
        fetched.resize(count * 3);
        HIP_TRY(hipSetDevice(dev));
        HIP_TRY(hipMemcpy(fetched.data(), texels, fetched.size() * sizeof(float), hipMemcpyDeviceToHost));
        texels = fetched.data();
    } else {
        for (size_t k = 0; k < count * 3; ++k)
            if (!(texels[k] >= 0.0f) || !std::isfinite(texels[k]))
                return fail(err, who + ": texel " + std::to_string(k / 3) + " is negative or not finite");
    }
    std::vector<hippt::env::Texel> next(count);
    for (size_t k = 0; k < count; ++k) next[k] = hippt::env::Texel{texels[3 * k], texels[3 * k + 1], texels[3 * k + 2], 0.0f};
    s.env.swap(next);
    s.envSize = size;
    ++s.envRev;
    // every context takes it now, in its stream's order (one that does not exist yet: at its first use)
    if (s.ready)
        for (Ctx &c : s.ctxs)
            if (!upload_env(c, err)) return false;
    return true;
}
}  // namespace

extern "C" bool hipptSetEnvironment(const float *texels, int size, int flags, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool { return set_environment_locked(texels, size, flags, err); });
}

extern "C" bool hipptEnvLookup(const float *dirs, long long n, float *rgb, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        const State &s = S();
        if (n < 0) return fail(err, "environment lookup: negative count");
        if (n > 0 && (!dirs || !rgb)) return fail(err, "environment lookup: null pointer");
        if (!s.envSize) return fail(err, "environment lookup: no environment set");
        for (long long i = 0; i < n; ++i)
            hippt::env::lookup(s.env.data(), s.envSize, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], rgb[3 * i],
                               rgb[3 * i + 1], rgb[3 * i + 2]);
        return true;
    });
}

extern "C" void hipptEnvDirections(int size, float *dirs) {
    abi_void(kUnlocked, [&] { hippt::envio::directions(size, dirs); });
}

extern "C" bool hipptEnvFromEquirect(const float *rgb, int width, int height, int size, float *texels, const char **err) {
    return abi_bool(kUnlocked, err, [&]() -> bool {
        std::string msg;
        if (hippt::envio::from_equirect(rgb, width, height, size, texels, &msg)) return true;
        std::lock_guard<std::mutex> g(S().mu);
        return fail(err, msg);
    });
}

// ---- ray queries ---------------------------------------------------------------------------------
// (each call's buffers in the order of the device-pointer check)
extern "C" bool hipptTraceRays(const float *rays, long long numRays, int flags, float *t, int *prim,
                               const char **err) {
    return abi_bool(kLocked, err, [&] {
        return query_locked(
            query_call(QueryMode::Closest, numRays, 0, flags, {{Slot::Rays, rays}, {Slot::T, t}, {Slot::Prim, prim}}), err);
    });
}

extern "C" bool hipptOccluded(const float *rays, long long numRays, int flags, unsigned char *occluded,
                              const char **err) {
    return abi_bool(kLocked, err, [&] {
        return query_locked(query_call(QueryMode::Any, numRays, 0, flags, {{Slot::Rays, rays}, {Slot::Occluded, occluded}}),
                            err);
    });
}

extern "C" bool hipptTraceCamera(int frame, int flags, float *t, int *prim, const char **err) {
    return abi_bool(kLocked, err, [&] {
        return query_locked(query_call(QueryMode::Camera, 0, frame, flags, {{Slot::T, t}, {Slot::Prim, prim}}), err);
    });
}

extern "C" bool hipptTraceHits(const float *rays, long long numRays, int flags, hipptHit *hits, const char **err) {
    return abi_bool(kLocked, err, [&] {
        return query_locked(query_call(QueryMode::Hits, numRays, 0, flags, {{Slot::Rays, rays}, {Slot::Hits, hits}}), err);
    });
}

extern "C" bool hipptTraceCameraHits(int frame, int flags, hipptHit *hits, const char **err) {
    return abi_bool(kLocked, err, [&] {
        return query_locked(query_call(QueryMode::CameraHits, 0, frame, flags, {{Slot::Hits, hits}}), err);
    });
}

// ---- path queries --------------------------------------------------------------------------------
extern "C" bool hipptTraceRadiance(const float *rays, const unsigned int *seeds, long long numRays, int maxDepth, int flags,
                                   float *radiance, int *segments, const char **err) {
    return abi_bool(kLocked, err, [&] {
        QueryCall q = query_call(
            QueryMode::Closest, numRays, 0, flags,
            {{Slot::Rays, rays}, {Slot::Seeds, seeds}, {Slot::Radiance, radiance}, {Slot::Segments, segments}});
        q.path = true;
        q.maxDepth = maxDepth;
        return query_locked(q, err);
    });
}

extern "C" bool hipptCameraRays(int frame, int flags, float *rays, unsigned int *seeds, const char **err) {
    return abi_bool(kLocked, err, [&] {
        QueryCall q = query_call(QueryMode::Closest, 0, frame, flags, {{Slot::OutRays, rays}, {Slot::OutSeeds, seeds}});
        q.camRays = true;
        return query_locked(q, err);
    });
}

extern "C" void hipptDenoiseDefaults(hipptDenoiseParams *out) {
    abi_void(kUnlocked, [&] {
        if (!out) return;
        std::memset(out, 0, sizeof(*out));
        out->passes = 5;
        out->guideFrame = 0;
        out->normalPower = 6;
        out->sigmaColor = 1.0f;
        out->sigmaDepth = 0.05f;
    });
}

extern "C" bool hipptDenoise(const hipptDenoiseParams *params, unsigned int *pixels, float *rgba, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        return denoise_locked(params, pixels, rgba, err);
    });
}

namespace {
struct MeshOwner {
    hippt::MeshData data;
    std::vector<const char *> names;
};
}  // namespace

extern "C" bool hipptReadMesh(const char *path, hipptMesh *out, const char **err) {
    return abi_bool(kUnlocked, err, [&]() -> bool {
        if (!path || !out) return fail(err, "null argument");
        std::memset(out, 0, sizeof(*out));
        std::unique_ptr<MeshOwner> own(new MeshOwner);
        std::string msg;
        if (!hippt::read_mesh(path, own->data, msg)) {
            std::lock_guard<std::mutex> g(S().mu);
            return fail(err, msg);
        }
        for (const std::string &n : own->data.groups) own->names.push_back(n.c_str());
        out->verts = own->data.verts.data();
        out->triGroup = own->data.group.data();
        out->numTris = int(own->data.group.size());
        out->numGroups = int(own->data.groups.size());
        out->groupNames = own->names.data();
        out->owner_ = own.release();
        return true;
    });
}

extern "C" void hipptFreeMesh(hipptMesh *mesh) {
    abi_void(kUnlocked, [&] {
        if (!mesh) return;
        delete static_cast<MeshOwner *>(mesh->owner_);
        std::memset(mesh, 0, sizeof(*mesh));
    });
}

extern "C" bool hipptSetCamera(const hipptCamera *camera, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        if (!camera) return fail(err, "null camera");
        std::memcpy(&S().scene.cam, camera, sizeof(CameraF));
        S().scene.rawCamera = true;
        return true;
    });
}

// ---- devices ------------------------------------------------------------------------------------
extern "C" int hipptDeviceCount(void) {
    return abi_value(kUnlocked, 0, [&]() -> int {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) return 0;
        return n;
    });
}

extern "C" bool hipptSetDevices(const int *deviceIds, int numDevices, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        State &s = S();
        if (numDevices < 0 || (numDevices > 0 && !deviceIds)) return fail(err, "invalid device list");
        int avail = 0;
        HIP_TRY(hipGetDeviceCount(&avail));
        for (int i = 0; i < numDevices; ++i)
            if (deviceIds[i] < 0 || deviceIds[i] >= avail) return fail(err, "device id out of range");
        s.devices.assign(deviceIds, deviceIds + numDevices);
        return true;
    });
}

extern "C" bool hipptSetRowRange(int y0, int y1, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        if (y0 < 0 || (y1 > 0 && y1 < y0)) return fail(err, "invalid row range");
        S().rowY0 = y0;
        S().rowY1 = y1;
        S().rowPhase = 0;
        S().rowStride = 1;
        return true;
    });
}

extern "C" bool hipptSetRowInterleave(int phase, int stride, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        if (stride < 1 || phase < 0 || phase >= stride) return fail(err, "invalid row interleave");
        S().rowPhase = phase;
        S().rowStride = stride;
        S().rowY0 = 0;
        S().rowY1 = 0;
        return true;
    });
}

// ---- rendering ----------------------------------------------------------------------------------
extern "C" bool hipptRenderFrames(int firstFrame, int count, int maxDepth, const unsigned int **hostPixels,
                                  const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        return render_locked(firstFrame, count, maxDepth, hostPixels, err);
    });
}

extern "C" bool hipptRenderFramesAsync(int firstFrame, int count, int maxDepth, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        return enqueue_locked(firstFrame, count, maxDepth, false, err);
    });
}

extern "C" bool hipptSynchronize(const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        return sync_locked(err);
    });
}

extern "C" bool hipptRenderFramesPresent(int firstFrame, int count, int maxDepth, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        State &s = S();
        if (!s.ready) return fail(err, "HIP path tracer not initialized");
        const int b = s.presentNext;
        // mapped + coherent like State::host: the frame's kernel writes the hand-off frame itself
        if (!s.present[b])
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.present[b]), s.hostCount * sizeof(unsigned),
                                  hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
        if (!enqueue_locked(firstFrame, count, maxDepth, true, err, s.present[b])) return false;
        for (Ctx &c : s.ctxs) {
            HIP_TRY(hipSetDevice(c.device));
            if (!c.presentEv[b]) HIP_TRY(hipEventCreateWithFlags(&c.presentEv[b], hipEventDisableTiming));
            HIP_TRY(hipEventRecord(c.presentEv[b], c.stream));
            if (!harvest_locked(c, err)) return false;
        }
        if (s.latest == b) s.latest = -1;  // its image is being replaced
        s.presentPending[b] = true;
        s.presentSeq[b] = s.presentCalls++;
        s.presentFrames[b] = firstFrame + count;
        s.presentNext = b ^ 1;
        return true;
    });
}

extern "C" bool hipptLatestFrame(const unsigned int **hostPixels, int *frames, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        State &s = S();
        if (!s.ready) return fail(err, "HIP path tracer not initialized");
        for (int b = 0; b < 2; ++b) {
            if (!s.presentPending[b]) continue;
            bool done = true;
            for (Ctx &c : s.ctxs) {
                HIP_TRY(hipSetDevice(c.device));
                const hipError_t q = hipEventQuery(c.presentEv[b]);
                if (q == hipErrorNotReady) {
                    done = false;
                    break;
                }
                if (q != hipSuccess) return fail(err, std::string("hipEventQuery: ") + hipGetErrorString(q));
            }
            if (done) {
                s.presentPending[b] = false;
                if (s.latest < 0 || s.presentSeq[b] > s.presentSeq[s.latest]) s.latest = b;
            }
        }
        if (hostPixels) *hostPixels = s.latest >= 0 ? s.present[s.latest] : nullptr;
        if (frames) *frames = s.latest >= 0 ? s.presentFrames[s.latest] : 0;
        return true;
    });
}

extern "C" bool hipptReadback(unsigned int *pixels, float *accum, const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        State &s = S();
        if (!s.ready) return fail(err, "HIP path tracer not initialized");
        if (!sync_locked(err)) return false;
        for (Ctx &c : s.ctxs) {
            HIP_TRY(hipSetDevice(c.device));
            if (pixels && !copy_rows_async(c, pixels, c.out, sizeof(uint32_t), err)) return false;
            if (accum && !copy_rows_async(c, accum, c.accum, sizeof(float4), err)) return false;
            HIP_TRY(hipStreamSynchronize(c.stream));
        }
        return true;
    });
}

extern "C" bool hipptResetAccumulation(const char **err) {
    return abi_bool(kLocked, err, [&]() -> bool {
        State &s = S();
        if (!s.ready) return fail(err, "HIP path tracer not initialized");
        for (Ctx &c : s.ctxs) {
            if (!flush_deferred(c, err)) return false;
            HIP_TRY(hipSetDevice(c.device));
            const size_t px = size_t(c.rows) * size_t(s.width);
            HIP_TRY(hipMemsetAsync(c.accum, 0, px * sizeof(float4), c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
        }
        return true;
    });
}

// A context's launch counters summed over their kStatSlots copies (hippt_device.h).
bool read_stats(const Ctx &c, unsigned long long (&v)[kStatWords]) {
    std::vector<unsigned long long> all(size_t(kStatSlots) * kStatWords);
    std::memset(v, 0, sizeof(v));
    if (hipSetDevice(c.device) != hipSuccess) return false;
    if (hipMemcpy(all.data(), c.stats, kStatBytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int k = 0; k < kStatSlots; ++k)
        for (int i = 0; i < kStatWords; ++i) v[i] += all[size_t(k) * kStatWords + size_t(i)];
    return true;
}

// ---- counters / options -------------------------------------------------------------------------
extern "C" bool hipptGetStats(hipptStats *out) {
    return abi_value(kLocked, false, [&]() -> bool {
        State &s = S();
        if (!out) return false;
        std::memset(out, 0, sizeof(*out));
        const char *err = nullptr;
        if (s.ready && !sync_locked(&err)) return false;
        for (Ctx &c : s.ctxs) {
            unsigned long long v[kStatWords];
            if (!read_stats(c, v)) return false;
            out->segments += v[0] + c.hostSegments;
            out->pixelSamples += v[1] + c.hostSamples;
            out->nodeVisits += v[2];
            out->triTests += v[3];
        }
        out->traceMs = s.traceMs;
        out->combineMs = s.combineMs;
        out->traceLaunches = s.traceLaunches;
        out->combineLaunches = s.combineLaunches;
        out->bvhNodes = s.scene.kind == HIPPT_SCENE_MESH ? s.scene.numNodes : 0;
        out->bvhDepth = s.scene.kind == HIPPT_SCENE_MESH ? s.scene.levels : 0;
        out->numTris = s.scene.kind == HIPPT_SCENE_MESH ? s.scene.numTris : 0;
        out->numDevices = int(s.ctxs.size());
        return true;
    });
}

extern "C" int hipptGetCounters(unsigned long long *out, int n) {
    return abi_value(kLocked, 0, [&]() -> int {
        State &s = S();
        if (!out || n <= 0) return 0;
        n = std::min(n, kStatWords);
        std::memset(out, 0, sizeof(unsigned long long) * size_t(n));
        const char *err = nullptr;
        if (s.ready && !sync_locked(&err)) return 0;
        for (Ctx &c : s.ctxs) {
            unsigned long long v[kStatWords];
            if (!read_stats(c, v)) return 0;
            v[0] += c.hostSegments;
            v[1] += c.hostSamples;
            for (int i = 0; i < n; ++i) out[i] += v[i];
        }
        return n;
    });
}

extern "C" void hipptResetStats(void) {
    abi_void(kLocked, [&] {
        State &s = S();
        const char *err = nullptr;
        if (s.ready) sync_locked(&err);
        for (Ctx &c : s.ctxs) {
            (void)hipSetDevice(c.device);
            (void)hipMemset(c.stats, 0, kStatBytes);
            c.hostSamples = 0;
            c.hostSegments = 0;
        }
        s.traceMs = s.combineMs = 0;
        s.traceLaunches = s.combineLaunches = 0;
    });
}

namespace {
bool set_option_locked(int key, long long value) {
    State &s = S();
    switch (key) {
    case HIPPT_OPT_COUNT_TRAVERSAL: s.knobs.countTraversal = value != 0; return true;
    case HIPPT_OPT_WAVE_THRESHOLD:
        if (value < -1 || value > 64) return false;
        s.knobs.waveThreshold = int(value);
        return true;
    case HIPPT_OPT_SCRATCH_MB:
        if (value < 1) return false;
        s.scratchMB = value;
        return true;
    case HIPPT_OPT_CHUNK:
        if (value != 0 && (value < 64 || value > (1 << 20) || value % 64)) return false;
        s.knobs.chunk = unsigned(value);
        return true;
    case HIPPT_OPT_BLOCKS_PER_CU:
        if (value < 0 || value > 8) return false;
        s.blocksPerCu = int(value);
        return true;
    case HIPPT_OPT_LDS_SCENE: s.knobs.ldsScene = value != 0; return true;
    case HIPPT_OPT_PATH_MODE:
        if (value != 0 && value != 1) return false;
        s.knobs.pathMode = int(value);
        return true;
    case HIPPT_OPT_WAVEFRONT_SLOTS:
        if (value < 64 || value > (1LL << 28)) return false;
        s.wfSlots = unsigned(value);
        return true;
    case HIPPT_OPT_BVH_LEAF:
        if (value < 1 || value > 15) return false;
        s.bvh.maxLeaf = int(value);
        return true;
    case HIPPT_OPT_BVH_TRAVERSAL_COST:
        if (value < 1 || value > 100000) return false;
        s.bvh.traversalCost = float(value) / 100.0f;
        return true;
    case HIPPT_OPT_BVH_MAX_DEPTH:
        if (value < 1 || value > hippt::kStackDepth) return false;
        s.bvh.maxDepth = int(value);
        return true;
    case HIPPT_OPT_DEVICE_ROWS:
        if (value < 0 || value > 1) return false;
        s.deviceInterleave = value == 1;
        return true;
    case HIPPT_OPT_LEAF_EXIT:
        if (value < -1 || value > 64) return false;
        s.knobs.leafExit = int(value);
        return true;
    case HIPPT_OPT_NODE_EXIT:
        if (value < -1 || value > 64) return false;
        s.knobs.nodeExit = int(value);
        return true;
    case HIPPT_OPT_BVH_SAH:
        if (value != 0 && value != 1) return false;
        s.bvh.sahMode = int(value);
        return true;
    case HIPPT_OPT_BVH_WIDTH:
        if (value != 0 && value != 2 && value != 4) return false;
        s.knobs.bvhWidth = int(value);
        return true;
    case HIPPT_OPT_STACK_CAP:
        if (value != 0 && (value < 4 || value > plan::kLdsStackCap)) return false;
        s.knobs.stackCap = int(value);
        return true;
    case HIPPT_OPT_BVH_QUANT:
        if (value < -1 || value > 3) return false;
        s.knobs.bvhQuant = int(value);
        return true;
    case HIPPT_OPT_LDS_TOP_NODES:
        if (value < -1 || value > plan::kTopOrderNodes) return false;
        s.knobs.ldsTopNodes = int(value);
        return true;
    case HIPPT_OPT_BVH_COLLAPSE:
        if (value < -1 || value > 1) return false;
        s.bvh.collapse = int(value);
        return true;
    case HIPPT_OPT_BVH_NODE_COST:
        if (value < 1 || value > 100000) return false;
        s.bvh.nodeCost = float(value) / 100.0f;
        return true;
    case HIPPT_OPT_BVH_LEAF4:
        if (value < 1 || value > 15) return false;
        s.bvh.maxLeaf4 = int(value);
        return true;
    case HIPPT_OPT_RNG_TABLE:
        if (value != 0 && value != 1) return false;
        s.rngTable = value == 1;
        return true;
    case HIPPT_OPT_PIXEL_FORMAT:
        if (value != HIPPT_PIXEL_ARGB && value != HIPPT_PIXEL_RGBA8) return false;
        s.pixelFormat = int(value);
        return true;
    case HIPPT_OPT_CAMERA_POOL:
        if (value < -1 || value > 1) return false;
        s.knobs.cameraPool = int(value);
        return true;
    case HIPPT_OPT_FUSE_COMBINE:
        if (value < -1 || value > 1) return false;
        s.knobs.fuseCombine = int(value);
        return true;
    case HIPPT_OPT_ITEM_ORDER:
        if (value < -1 || value > 1) return false;
        s.itemOrder = int(value);
        return true;
    case HIPPT_OPT_WAVEFRONT_SORT:
        if (value != -1 && value != 0 && value != 3 && value != 6) return false;
        s.wfSort = int(value);
        return true;
    case HIPPT_OPT_CHAIN:
        if (value < -1 || value > 16) return false;
        s.knobs.chainBatches = int(value);
        return true;
    case HIPPT_OPT_CHAIN_AUDIT:
        if (value != 0 && value != 1) return false;
        s.chainAudit = value == 1;
        return true;
    case HIPPT_OPT_PIXEL_TILE:
        if (value != -1 && value != 0 && value != 8 && value != 16 && value != 32) return false;
        s.pixelTile = int(value);
        return true;
    case HIPPT_OPT_QUERY_SLICE:
        if (value < 0 || value > (1LL << 28)) return false;
        s.querySlice = value;
        return true;
    case HIPPT_OPT_RENDER_PAD:
        if (value != 0 && (value < hippt::slab::kRenderPadMin || value > hippt::slab::kRenderPadMax)) return false;
        s.knobs.renderPad = int(value);
        return true;
    case HIPPT_OPT_SKY_RECT:
        if (value != 0 && value != 1) return false;
        s.knobs.skyRect = value == 1;
        return true;
    case HIPPT_OPT_SKY_COMBINE:
        if (value != -1 && value != 0) return false;
        s.knobs.skyCombine = int(value);
        return true;
    case HIPPT_OPT_DENOISE_TIMING:
        if (value != 0 && value != 1) return false;
        s.denoiseTiming = value == 1;
        return true;
    case HIPPT_OPT_LIGHT_SAMPLING:  // the on/off form: 0 and 1 only, as before the mode existed
        if (value != 0 && value != 1) return false;
        s.lightSampling = int(value);
        return true;
    case HIPPT_OPT_LIGHT_SAMPLING_MODE:
        if (value != 0 && value != 1 && value != HIPPT_LIGHT_SAMPLING_MIS) return false;
        s.lightSampling = int(value);
        return true;
    case HIPPT_OPT_LIGHT_SELECT:
        if (value != 0 && value != HIPPT_LIGHT_SELECT_POWER) return false;
        s.lightSelect = int(value);
        return true;
    case HIPPT_OPT_ENV_SAMPLING:
        if (value != 0 && value != 1) return false;
        s.envSampling = int(value);
        return true;
    default: return false;
    }
}
}  // namespace

extern "C" bool hipptSetOption(int key, long long value) {
    return abi_value(kLocked, false, [&] { return set_option_locked(key, value); });
}

extern "C" int hipptActiveBvhWidth(void) {
    return abi_value(kLocked, 0, [&]() -> int {
        return S().activeWidth;
    });
}

namespace {
long long get_option_locked(int key) {
    State &s = S();
    switch (key) {
    case HIPPT_OPT_COUNT_TRAVERSAL: return s.knobs.countTraversal ? 1 : 0;
    case HIPPT_OPT_WAVE_THRESHOLD: return s.knobs.waveThreshold;
    case HIPPT_OPT_SCRATCH_MB: return s.scratchMB;
    case HIPPT_OPT_CHUNK: return s.knobs.chunk;
    case HIPPT_OPT_BLOCKS_PER_CU: return s.blocksPerCu;
    case HIPPT_OPT_LDS_SCENE: return s.knobs.ldsScene ? 1 : 0;
    case HIPPT_OPT_PATH_MODE: return s.knobs.pathMode;
    case HIPPT_OPT_WAVEFRONT_SLOTS: return s.wfSlots;
    case HIPPT_OPT_BVH_LEAF: return s.bvh.maxLeaf;
    case HIPPT_OPT_BVH_TRAVERSAL_COST: return (long long)std::lround(s.bvh.traversalCost * 100.0f);
    case HIPPT_OPT_BVH_MAX_DEPTH: return s.bvh.maxDepth;
    case HIPPT_OPT_DEVICE_ROWS: return s.deviceInterleave ? 1 : 0;
    case HIPPT_OPT_LEAF_EXIT: return s.knobs.leafExit;
    case HIPPT_OPT_NODE_EXIT: return s.knobs.nodeExit;
    case HIPPT_OPT_BVH_SAH: return s.bvh.sahMode;
    case HIPPT_OPT_BVH_WIDTH: return s.knobs.bvhWidth;
    case HIPPT_OPT_STACK_CAP: return s.knobs.stackCap;
    case HIPPT_OPT_BVH_QUANT: return s.knobs.bvhQuant;
    case HIPPT_OPT_LDS_TOP_NODES: return s.knobs.ldsTopNodes;
    case HIPPT_OPT_BVH_COLLAPSE: return s.bvh.collapse;
    case HIPPT_OPT_BVH_NODE_COST: return (long long)std::lround(s.bvh.nodeCost * 100.0f);
    case HIPPT_OPT_BVH_LEAF4: return s.bvh.maxLeaf4;
    case HIPPT_OPT_RNG_TABLE: return s.rngTable ? 1 : 0;
    case HIPPT_OPT_PIXEL_FORMAT: return s.pixelFormat;
    case HIPPT_OPT_CAMERA_POOL: return s.knobs.cameraPool;
    case HIPPT_OPT_FUSE_COMBINE: return s.knobs.fuseCombine;
    case HIPPT_OPT_ITEM_ORDER: return s.itemOrder;
    case HIPPT_OPT_WAVEFRONT_SORT: return s.wfSort;
    case HIPPT_OPT_CHAIN: return s.knobs.chainBatches;
    case HIPPT_OPT_CHAIN_AUDIT: return s.chainAudit ? 1 : 0;
    case HIPPT_OPT_PIXEL_TILE: return s.pixelTile;
    case HIPPT_OPT_QUERY_SLICE: return s.querySlice;
    case HIPPT_OPT_RENDER_PAD: return s.knobs.renderPad;
    case HIPPT_OPT_SKY_RECT: return s.knobs.skyRect ? 1 : 0;
    case HIPPT_OPT_SKY_COMBINE: return s.knobs.skyCombine;
    case HIPPT_INFO_LDS_TOP_BYTES: return s.activeTopBytes;
    case HIPPT_INFO_BLOCKS_PER_CU: return s.activeBlocksPerCu;
    case HIPPT_INFO_CHUNK: return s.activeChunk;
    case HIPPT_INFO_CHAIN_CAP: return s.activeChainCap;
    case HIPPT_INFO_RENDER_PAD: return s.activeRenderPad;
    case HIPPT_OPT_DENOISE_TIMING: return s.denoiseTiming ? 1 : 0;
    case HIPPT_OPT_LIGHT_SAMPLING:
    case HIPPT_OPT_LIGHT_SAMPLING_MODE: return s.lightSampling;
    case HIPPT_INFO_LIGHTS: return s.scene.kind == HIPPT_SCENE_MESH ? (long long)s.scene.lights.size() : 0;
    case HIPPT_INFO_LIGHT_SAMPLING: return s.activeLightSampling;
    case HIPPT_OPT_LIGHT_SELECT: return s.lightSelect;
    case HIPPT_INFO_LIGHT_SELECT: return s.activeLightSelect;
    case HIPPT_INFO_ENVIRONMENT: return s.activeEnv;
    case HIPPT_OPT_ENV_SAMPLING: return s.envSampling;
    case HIPPT_INFO_ENV_SAMPLING: return s.activeEnvSampling;
    case HIPPT_INFO_SKY_RECT_PIXELS: return s.activeSkyPixels;
    case HIPPT_INFO_SKY_COMBINE: {
        long long n = 0;
        for (const Ctx &c : s.ctxs) n += c.skyCombinePixels;
        return n;
    }
    case HIPPT_INFO_UPDATE_DROPPED:
        // the last update's count, from the first context that ran it (every context counts the same)
        for (Ctx &c : s.ctxs) {
            if (!c.rfUpdated) continue;
            unsigned w[2] = {0, 0};
            if (hipSetDevice(c.device) != hipSuccess || hipStreamSynchronize(c.stream) != hipSuccess ||
                hipMemcpy(w, c.rfWords, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                return -1;
            }
            return w[1];
        }
        return 0;
    default:
        if (key >= HIPPT_INFO_DENOISE_NS && key < HIPPT_INFO_DENOISE_NS + hippt::kDenoiseStages)
            return s.denoiseNs[key - HIPPT_INFO_DENOISE_NS];
        return -1;
    }
}
}  // namespace

extern "C" long long hipptGetOption(int key) {
    return abi_value(kLocked, -1LL, [&] { return get_option_locked(key); });
}

extern "C" int hipptChainAudit(unsigned int *words, int maxWords) {
    return abi_value(kLocked, -1, [&]() -> int {
        State &s = S();
        const char *e = nullptr;
        if (s.ready && !sync_locked(&e)) return -1;  // closes the open runs (their final flushes) first
        size_t n = 0;
        while (n < s.auditWords.size()) {
            const size_t recs = std::min(s.auditWords[n + 8], hippt::kAuditBatches) + 1u;
            const size_t len = (1 + recs) * hippt::kAuditWords;
            if (n + len > size_t(std::max(0, maxWords))) break;
            n += len;
        }
        if (words && n) std::memcpy(words, s.auditWords.data(), n * sizeof(unsigned));
        s.auditWords.erase(s.auditWords.begin(), s.auditWords.begin() + long(n));
        return int(n);
    });
}

extern "C" const char *hipptLastError(void) { return S().error; }

// ---- host BVH builder -----------------------------------------------------------------------------
extern "C" hipptBvh *hipptBvhBuild(const float *verts, int numTris, float extentHint, const char **err) {
    return abi_guard(
        kUnlocked,
        [&]() -> hipptBvh * {
            std::unique_ptr<hipptBvh> b(new hipptBvh());
            std::string msg;
            hippt::BvhParams params;
            {
                std::lock_guard<std::mutex> g(S().mu);
                params = S().bvh;  // the build options an upload would use
            }
            if (!verts || !hippt::build_bvh(verts, numTris, extentHint, b->bvh, msg, params)) {
                std::lock_guard<std::mutex> g(S().mu);
                fail(err, msg.empty() ? "null vertex pointer" : msg);
                return nullptr;
            }
            hippt::collapse_bvh4(b->bvh, b->bvh4, params);
            hippt::order_bvh4_top(b->bvh4, plan::kTopOrderNodes);
            (void)hippt::quantize_bvh4(b->bvh4, b->bvh4q);  // empty for boxes near +-FLT_MAX
            return b.release();
        },
        [err](const char *what) { return (fail_free(err, what), static_cast<hipptBvh *>(nullptr)); });
}

extern "C" bool hipptBvhRefit(hipptBvh *b, const float *verts, int numTris, float extentHint, const char **err) {
    return abi_bool(kUnlocked, err, [&]() -> bool {
        auto bad = [&](const std::string &m) {
            std::lock_guard<std::mutex> g(S().mu);
            return fail(err, m);
        };
        if (!b) return bad("null BVH");
        if (!verts) return bad("null vertex pointer");
        if (numTris <= 0 || size_t(numTris) != b->bvh.order.size()) return bad("refit: numTris differs from the build's");
        for (size_t k = 0; k < size_t(numTris) * 9; ++k)
            if (!std::isfinite(verts[k])) return bad("non-finite primitive coordinate");
        std::vector<float> boxes(size_t(numTris) * 6);
        triangle_boxes(verts, numTris, boxes.data());
        std::string msg;
        if (!hippt::refit_bvh(b->bvh, b->bvh4, boxes.data(), numTris, extentHint, msg)) return bad(msg);
        (void)hippt::quantize_bvh4(b->bvh4, b->bvh4q);  // linear in the nodes; empty for boxes near +-FLT_MAX
        return true;
    });
}

extern "C" int hipptBvhNodeCount(const hipptBvh *b) { return b ? int(b->bvh.nodes.size() / hippt::kNodeWords) : 0; }
extern "C" int hipptBvhDepth(const hipptBvh *b) { return b ? b->bvh.levels : 0; }
extern "C" void hipptBvhCopy(const hipptBvh *b, uint32_t *nodes, int *triOrder) {
    abi_void(kUnlocked, [&] {
        if (!b) return;
        if (nodes) std::memcpy(nodes, b->bvh.nodes.data(), b->bvh.nodes.size() * sizeof(uint32_t));
        if (triOrder) std::memcpy(triOrder, b->bvh.order.data(), b->bvh.order.size() * sizeof(int));
    });
}
extern "C" void hipptBvhFree(hipptBvh *b) { delete b; }
extern "C" int hipptBvh4NodeCount(const hipptBvh *b) {
    return abi_value(kUnlocked, 0, [&]() -> int {
        return b ? int(b->bvh4.nodes.size() / hippt::kNode4Words) : 0;
    });
}
extern "C" int hipptBvh4Depth(const hipptBvh *b) { return b ? b->bvh4.levels : 0; }
extern "C" int hipptBvh4StackBound(const hipptBvh *b) { return b ? b->bvh4.stackBound : 0; }
extern "C" void hipptBvh4Copy(const hipptBvh *b, uint32_t *nodes) {
    abi_void(kUnlocked, [&] {
        if (b && nodes) std::memcpy(nodes, b->bvh4.nodes.data(), b->bvh4.nodes.size() * sizeof(uint32_t));
    });
}
extern "C" int hipptBvh4QNodeCount(const hipptBvh *b) {
    return abi_value(kUnlocked, 0, [&]() -> int {
        return b ? int(b->bvh4q.size() / hippt::kNode4QWords) : 0;
    });
}
extern "C" void hipptBvh4QCopy(const hipptBvh *b, uint32_t *nodes) {
    abi_void(kUnlocked, [&] {
        if (b && nodes) std::memcpy(nodes, b->bvh4q.data(), b->bvh4q.size() * sizeof(uint32_t));
    });
}
