// hippt_plan.h — traversal planning: what a render batch or a ray query launches with, as pure
// functions of the scene's facts, the options and the LDS limits.  No HIP, no global state: the
// product (hippt_api.cpp) and a host-compiled driver (tests/native/plan_check.cpp) call the same
// code, and the kernels' launchers (hippt_kernels.hip, hippt_wavefront.hip, hippt_query.hip) take
// the LDS layout's arithmetic (mesh_lds_bytes) from here.
//
//   layout()  once per enqueue or query: tree width, LDS residency, stack, node format, the camera
//             pool, the top of the tree in LDS, the wave threshold and the two loop exits
//   batch()   once per batch: claim size, whether the batch may chain, whether it wants the sky
//             rectangle and the render pad's trim
//   ring_plan()  once per batch that may chain: the run's cap (chain_cap), its ring's slots
//             (ring_slots), the slot size and the ring's bytes within the scratch budget
//
// The measurement notes (r2w, r3al, r5s, r6ao, ...: DESIGN_LOG.md) stand beside the rule they justify.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace hippt {

constexpr int kMeshBlock = 256;
// LDS-resident scene copies: 2-wide nodes at an 80-byte stride, 4-wide nodes in the 128-byte
// global layout (the octant row addressing by or/xor needs 128-byte alignment; a 144- or
// 160-byte stride cut the LDS bank conflicts of node rows by 40% but not the kernel time, and
// the add-based addressing it needs costs registers: spills in the general kernels).
constexpr int kLdsNodeF4 = 5;
constexpr int kLdsNode4F4 = 8;
// camera-pool kernels: per-wave state words in LDS before each wave's pool (trace::WaveWords)
constexpr unsigned kWaveWords = 22;
// camera-ray pool words per ray: item, rng, direction (+ origin unless every ray starts at the
// camera origin)
constexpr int kPoolWordsPinhole = 5, kPoolWordsFull = 8;
// batches of at most 2^kChainMaxShift items chain (the slot bits above them, kNone above all)
constexpr unsigned kChainMaxShift = 27;
// the most ring slots of a chained run (hippt_device.h: the control block's slot blocks; plan::ring_slots)
constexpr unsigned kChainSlotsMax = 32;

// MeshParams::wide
enum { kWide2 = 0, kWideFloat = 1, kWideQuant = 2, kWideHybrid = 3, kWideHalf = 4 };

// Dynamic LDS of a traversal block.  Stack: one spare slot per lane above the deepest level for the
// speculative far-child write; then (LDS_SCENE) the scene copy, or the top of the tree; then the
// camera-ray pool.
// (poolWords != 0: each wave's pool block also holds its kWaveWords state words)
inline size_t mesh_lds_bytes(int stackDepth, int ldsNodes, int ldsTris, bool wide, unsigned topBytes = 0, int ldsMats = 0,
                             int poolWords = 0) {
    return size_t(stackDepth + 1) * kMeshBlock * sizeof(int) +
           size_t(ldsNodes) * (wide ? kLdsNode4F4 : kLdsNodeF4) * 16 + size_t(ldsTris) * (3 + 1) * 16 + topBytes +
           size_t(ldsMats) * 2 * 16 +
           (poolWords ? (size_t(poolWords) * 64 + kWaveWords) * (kMeshBlock / 64) * sizeof(float) : 0);
}

namespace plan {

// 4-wide traversal: LDS stack content capacity for scenes outside LDS (19 + 3 spare entries =
// 22 KB per 256-lane block: 7 blocks per CU in 160 KB).
constexpr int kWideStackCap = 19;
// a tree that spills anyway keeps 10 entries and gives the rest to the top of the tree (r3al,
// alternating on leaf-2 trees: blob70k 1080p +0.5%, 4K +0.6% over 13; r3q before: +0.6%)
constexpr int kSpillStackCap = 10;
// LDS-resident scenes, and the most HIPPT_OPT_STACK_CAP takes (stackCap + 2 <= kStackDepth)
constexpr int kLdsStackCap = 30;
// 4-wide trees are numbered breadth-first for their first kTopOrderNodes nodes, so that a prefix
// of the node array is the top of the tree; trees read from global memory keep such a prefix in
// LDS (HIPPT_OPT_LDS_TOP_NODES)
constexpr int kTopOrderNodes = 1365;  // 6 complete levels
// a whole 1080p/64 spp image and more: its batches take the big claim (batch()) and the chain cap 8
constexpr unsigned kWholeImageItems = 1u << 26;

// What the rules read of the uploaded scene.
struct Facts {
    int numNodes = 0, numNodes4 = 0;  // 2-wide and 4-wide tree
    int numTris = 0;                  // primitive records (triangles + spheres)
    int numMats = 0;
    int levels = 0;                   // 2-wide interior levels
    int stackBound4 = 0;              // the builder's exact bound of the 4-wide traversal stack
    bool full = false;                // spheres or non-Lambertian materials (general kernel)
    bool quantTree = false;           // the scene has an 8-bit tree (quantize_bvh4 succeeded)
    // The half-precision tree is usable.  It is built on use: the caller asks for it (and sets this)
    // only where wants_half() says the plan reads it.
    bool halfTree = false;
};

// The options the rules read (hipptSetOption / hipptGetOption; include/hippt.h HIPPT_OPT_*).
struct Knobs {
    int bvhWidth = 0;      // megakernel traversal over the 2- or 4-wide BVH; 0: 4-wide if it fits in LDS
    bool ldsScene = true;
    int stackCap = 0;      // 4-wide LDS stack entries (0: automatic)
    int bvhQuant = -1;     // 4-wide global-memory traversal over 8-bit child boxes (-1: automatic)
    int ldsTopNodes = -1;  // top-of-tree nodes copied into LDS for global-memory trees (-1: automatic)
    int cameraPool = -1;   // megakernel camera-ray pool (HIPPT_OPT_CAMERA_POOL; -1: automatic)
    int pathMode = 0;      // 0 megakernel, 1 wavefront
    int waveThreshold = -1;  // -1: automatic (24 for LDS scenes and the general kernel, 40 for Lambertian scenes over trees in global memory)
    int leafExit = -1;     // -1: automatic from the tree depth and LDS residency
    int nodeExit = -1;     // -1: automatic
    unsigned chunk = 0;    // work items per claim (0: automatic, see batch())
    // read by batch() only
    bool countTraversal = false;
    int fuseCombine = -1;   // combine inside the next megakernel launch (HIPPT_OPT_FUSE_COMBINE)
    int chainBatches = -1;  // batches a chained launch may trace (HIPPT_OPT_CHAIN; 0 off, -1 automatic)
    int renderPad = 0;      // HIPPT_OPT_RENDER_PAD (0: the builder's pad)
    bool skyRect = true;    // HIPPT_OPT_SKY_RECT
    int skyCombine = -1;    // HIPPT_OPT_SKY_COMBINE (-1 automatic, 0 off)
};

// LDS limits of the kernels as built (hippt_kernels.hip mesh_lds_scene_limit, mesh_lds_block_budget:
// the second depends on the kernels' SGPR budget).
struct Limits {
    size_t scene = 0;  // most bytes of an LDS scene copy
    size_t block = 0;  // LDS bytes per block that keep the persistent grid's resident blocks within a CU's LDS
};

// small scenes live in LDS (scene bytes beyond the stack under the limit)
inline bool fits_lds_scene(int numNodes, int numTris, bool wide, int numMats, size_t sceneLimit) {
    return mesh_lds_bytes(0, numNodes, numTris, wide, 0, numMats) <= sceneLimit;
}

// Low bits of a packed child key (trace::child_key_p) that give an LDS-resident 4-wide tree's child
// codes back when sign-extended: interior codes are node byte offsets < numNodes*128, leaf codes
// ~(first<<4 | count) with first + count <= numPrims; one more bit for the sign.  At most 16 for a
// scene that fits the LDS copy (24 KB: < 192 nodes, < 384 primitives), which leaves the entry
// distance 7 or more mantissa bits (Cornell-34: 12 bits, 11 mantissa bits) to order children by.
inline unsigned packed_ref_bits(int numNodes, int numPrims) {
    const unsigned long long maxMag =
        std::max<unsigned long long>((unsigned long long)std::max(numNodes, 1) * 128ull,
                                     ((unsigned long long)numPrims << 4) + 16ull);
    unsigned bits = 1;
    while ((1ull << (bits - 1)) < maxMag) ++bits;  // magnitude < 2^(bits-1)
    return std::max(bits, 8u);
}

struct Layout {
    bool wide = false;      // traversal over the 4-wide tree
    int numNodes = 0;       // of the tree traversed
    bool ldsScene = false;
    int stackCap = 0;       // 4-wide: LDS stack content capacity
    int stackDepth = 1;     // LDS stack entries per lane
    bool spills = false;    // 4-wide: the stack bound exceeds stackCap
    // 4-wide: entries per lane of a spill area.  (A render allocates one, and passes this on, only when
    // `spills`; the query kernel takes one always.)
    int spillCap = 0;
    int fmt = kWide2;       // node format (kWide*)
    int poolWords = 0;      // camera-ray pool words per ray (0: no pool)
    unsigned topBytes = 0;  // bytes of the node array's prefix kept in LDS
    unsigned poolOffset = 0;  // LDS byte offset of the pool (the layout's bytes before it)
    unsigned refBits = 0;
    int waveThreshold = 0;
    unsigned leafExit = 0, nodeExit = 0;
};

inline bool wide_tree(const Facts &f, const Knobs &k) {
    // Traversal over the 4-wide tree (HIPPT_OPT_BVH_WIDTH), megakernel and wavefront.
    // Automatic: 4-wide.  With near/far rows read by the ray's octant, 4-wide beats
    // 2-wide on LDS scenes (Cornell 31.7 -> 35.3 G) and on global-memory trees (blob70k
    // 14.2 -> 15.4 G: half the dependent node fetches, 18% fewer load instructions);
    // random_scene (spheres, general kernel) 20.6 vs 20.5 G.
    return f.numNodes4 > 0 && k.bvhWidth != 2;
}

inline bool lds_scene(const Facts &f, const Knobs &k, const Limits &lim) {
    const bool wide = wide_tree(f, k);
    return k.ldsScene && fits_lds_scene(wide ? f.numNodes4 : f.numNodes, f.numTris, wide, f.numMats, lim.scene);
}

// layout() reads Facts::halfTree (HIPPT_OPT_BVH_QUANT 3 over a 4-wide tree in global memory)
inline bool wants_half(const Facts &f, const Knobs &k, const Limits &lim) {
    return wide_tree(f, k) && !lds_scene(f, k, lim) && k.bvhQuant == 3;
}

// pinholeOffOrigin: the camera is a pinhole at a nonzero origin (its pool entries carry no origin)
inline Layout layout(const Facts &f, const Knobs &k, const Limits &lim, bool pinholeOffOrigin) {
    Layout L;
    const bool wide = L.wide = wide_tree(f, k);
    const int numNodes = L.numNodes = wide ? f.numNodes4 : f.numNodes;
    const bool ldsScene = L.ldsScene = lds_scene(f, k, lim);
    // LDS stack entries per lane: 2-wide = interior levels (+1 spare); 4-wide = the
    // builder's exact bound up to kWideStackCap (+3 spare; deeper stacks spill their
    // bottom half to global memory), so that 7 blocks of a big scene fit in LDS.  A
    // traversal of a tree in global memory whose bound exceeds kWideStackCap (it
    // spills anyway) keeps kSpillStackCap entries and gives the rest of its LDS to the
    // top of the tree (blob70k, float nodes: cap 19 + 4 top nodes 17.8 G, cap 13 + 52
    // top nodes 20.4 G; caps 9-15 within 1%, 7: -3%; r2w; cap 10 + 76 nodes +0.5%, r3al)
    const bool topTree = wide && !ldsScene;
    const int capLimit = k.stackCap > 0 ? k.stackCap
                         : ldsScene     ? kLdsStackCap
                         : topTree && f.stackBound4 > kWideStackCap ? kSpillStackCap
                                                                     : kWideStackCap;
    L.stackCap = wide ? std::max(1, std::min(f.stackBound4, capLimit)) : 0;
    L.stackDepth = wide ? L.stackCap + 2 : std::max(1, f.levels);
    L.spills = wide && f.stackBound4 > L.stackCap;
    L.spillCap = wide ? f.stackBound4 + 3 : 0;
    // 8-bit child boxes for trees read from global memory: 64-byte nodes, 4 vector loads
    // instead of 7 where the texture addresser bounds the traversal (blob70k: TA busy
    // 84%, 15.6 -> 17.7 G).  Automatic for the wavefront's Lambertian-triangle kernel
    // only: the megakernel reads the top of the tree (62-70% of the visits) from LDS,
    // where the float nodes need no decode (blob70k 19.0 G 8-bit, 20.4 G float, r2v).
    // (scenes with boxes near +-FLT_MAX have no 8-bit tree: quantize_bvh4 failed)
    // Hybrid (HIPPT_OPT_BVH_QUANT 2, megakernel): the top of the tree as float nodes in LDS
    // (no decode where most visits are) and 8-bit nodes below it (4 loads instead of 7
    // where the texture addresser binds); falls back to 8-bit nodes without a top.
    bool hybrid = topTree && f.quantTree && k.pathMode == 0 && k.bvhQuant == 2 && k.ldsTopNodes != 0;
    bool quant = topTree && f.quantTree &&
                 (k.bvhQuant == 1 || k.bvhQuant == 2 || (k.bvhQuant == -1 && !f.full && k.pathMode == 1));
    // Half-precision planes (HIPPT_OPT_BVH_QUANT 3, megakernel and wavefront extend): the
    // float nodes' size and codes, 4 reads per visit instead of 7
    // half planes unless the scene's planes leave the half range (then float nodes)
    const bool half = topTree && k.bvhQuant == 3 && f.halfTree;
    // The top of a global-memory tree in LDS (megakernel and wavefront extend): the
    // breadth-first prefix of the node array that the LDS budget of the resident blocks
    // leaves beside the stack (automatic), or HIPPT_OPT_LDS_TOP_NODES nodes.  The
    // wavefront keeps its 8-bit nodes (blob70k: 8.28 G 8-bit, 7.53 G float, r2za).
    // Camera-ray pool (megakernel, 4-wide float nodes): on by default for LDS-resident
    // scenes and for the Lambertian kernel over a tree in global memory (its pool's LDS
    // comes out of the top of the tree).
    // Pinhole cameras at a nonzero origin start every ray at cam.origin exactly
    // (origin + 0*offset), so their pool entries carry no origin.
    // (round 3, r6j: also for the Lambertian kernel over a tree in global memory,
    // blob70k +1.8% though the pool's LDS comes out of the top; the general kernel
    // there loses 10%, random_scene)
    const bool pool = k.pathMode == 0 && wide && !quant &&
                      (k.cameraPool == 1 || (k.cameraPool == -1 && (ldsScene || !f.full)));
    if (hybrid) quant = false;  // (pool: off, as for 8-bit nodes)
    L.poolWords = pool ? (pinholeOffOrigin ? kPoolWordsPinhole : kPoolWordsFull) : 0;
    if (topTree && k.ldsTopNodes != 0) {
        const size_t nodeBytes = quant ? 64 : 128;  // hybrid: a float top
        size_t n = size_t(std::min(numNodes, kTopOrderNodes));
        if (k.ldsTopNodes > 0) {
            n = std::min(n, size_t(k.ldsTopNodes));
        } else {
            const size_t stackBytes = mesh_lds_bytes(L.stackDepth, 0, 0, true, 0, 0, L.poolWords);
            n = std::min(n, lim.block > stackBytes ? (lim.block - stackBytes) / nodeBytes : 0);
        }
        L.topBytes = unsigned(n * nodeBytes);
    }
    if (hybrid && L.topBytes == 0) {  // no LDS left for a top: plain 8-bit nodes
        hybrid = false;
        quant = true;
    }
    L.fmt = !wide ? kWide2 : hybrid ? kWideHybrid : quant ? kWideQuant : half ? kWideHalf : kWideFloat;
    L.poolOffset = unsigned(mesh_lds_bytes(L.stackDepth, ldsScene ? numNodes : 0, ldsScene ? f.numTris : 0, wide,
                                           L.topBytes, ldsScene ? f.numMats : 0));
    L.refBits = ldsScene && wide ? packed_ref_bits(numNodes, f.numTris) : 0u;
    // shade once fewer than this many lanes still traverse (re-swept in round 3
    // under the sample-length item order, r5y-r6a: LDS scenes 24 with the exits
    // below, Cornell 48.4 -> 53.7 G; global-memory trees 32, blob70k 24 and 40
    // lower)
    // (the general megakernel over a tree in global memory: 24, random_scene
    // +5.8% over 32 with the exits below, r6c)
    // Re-swept on round 6's kernels (r6aj/r6ak, alternating passes): a whole
    // blob70k image 40 over 32 +0.5-0.7% (21,882 -> 22,031 M/s; 36 +0.5%, 44 and 48
    // slower), configs[3]'s 4K image +0.6%, but its 1/8 shares 2.433 -> 2.471 ms:
    // 40 with the loop exits 22 / 56 below (alone, 40 slowed the shares: r6ak);
    // Cornell 28/32 within 0.2% of 24.
    const bool fullMega = k.pathMode == 0 && f.full;
    // Lambertian batches over a tree in global memory, megakernel or wavefront (this
    // wave threshold and the loop exits below; the wavefront's configs[4] 14,243 ->
    // 14,436 M/s with 40 / 22 / 56, r6aq; blob70k's 1/4 and 1/8 row shares 4.705 ->
    // 4.612 and 2.433 -> 2.391 ms, r6at)
    const bool lambertGlobal = !ldsScene && !f.full;
    L.waveThreshold = k.waveThreshold >= 0   ? k.waveThreshold
                      : ldsScene || fullMega ? 24
                      : lambertGlobal        ? 40
                                             : 32;
    // Loop exits of the traversal round (measured): trees in global
    // memory leave the node loop once <= 17 lanes still search for a leaf (r2
    // sweep of the 4-wide kernels: blob70k, 21 levels, best at 17-18; blob64x34
    // and random_scene, 16 and 12 levels, best at 15) and the leaf loop once
    // <= 48 lanes hold a leaf; LDS scenes at 12 and 8 (round 3, with the item
    // order: node exit 4-16 x leaf exit 8-16 within 0.6% of the best, Cornell
    // 53.8 G; the round-2 values 4 and 48 gave 48.4 G), except that the general
    // kernel and the wavefront keep leaf exit 4 (cornell_mixed +1.4%, Cornell
    // wavefront +6% over 12; r6b)
    // The general megakernel over a tree in global memory: 12 and 16 (random_scene,
    // r6c).  The Lambertian kernels over a tree in global memory, with the wave
    // threshold 40: 22 and 56 (blob70k whole image, alternating passes: 22,057 ->
    // 22,372 M/s, +1.4%; 20-26 x 48-64 within 0.3% of it, 28 lower, r6ao/r6ap).
    const bool lambertMega = k.pathMode == 0 && !f.full;
    L.leafExit = unsigned(k.leafExit >= 0 ? k.leafExit
                          : ldsScene      ? (lambertMega ? 12 : 4)
                          : fullMega      ? 12
                          : lambertGlobal ? 22
                                          : 17);
    L.nodeExit = unsigned(k.nodeExit >= 0 ? k.nodeExit
                          : ldsScene      ? 8
                          : fullMega      ? 16
                          : lambertGlobal ? 56
                                          : 48);
    return L;
}

// The ray queries' profile (hippt_query.hip): the render rules of the wavefront extend kernel (its
// wave threshold and loop exits) over float nodes, without a camera pool; every other option as set.
inline Knobs query_knobs(Knobs k) {
    k.pathMode = 1;
    k.bvhQuant = 0;
    k.cameraPool = 0;
    return k;
}

// rays per claim of a query launch of m rays
inline unsigned query_chunk(unsigned m) { return m >= (1u << 20) ? 256u : 64u; }

// HIPPT_OPT_SKY_COMBINE: the megakernel variants whose fused combine has the sky branch (hippt_kernels.hip
// mesh_kernel SKYCOMB): the timed camera-pool kernels, less those that could take it only with new scratch
// bytes (profiles/sky_combine/regs.txt): the unchained general kernels over an LDS scene, or with the
// spilling stack.  A batch traced by another variant keeps the in-kernel path, and a launch of another
// variant leaves a pending sky-mode combine to combine_kernel.
constexpr bool sky_combine_kernel(bool count, bool lds, bool full, bool spill, bool pool, bool chain) {
    return pool && !count && !(full && !chain && (lds || spill));
}

// What depends on the batch.  A batch that may chain is chained once its ring is there (ring_plan
// below; hippt_api.cpp ensure_ring); the claim size and the sky rectangle depend on whether it was: [0] for a
// batch launched on its own, [1] for a chained one.
struct Batch {
    bool fuse = false;      // the megakernel takes the previous batch's combine along; other batches flush it
    bool mayChain = false;
    bool trimWanted = false;
    unsigned chunk[2] = {0, 0};
    bool skyWanted[2] = {false, false};
    // HIPPT_OPT_SKY_COMBINE's static part: the option, a rectangle wanted, not counted, a variant with the branch
    // (the rectangle itself, the item table and the audit are the caller's)
    bool skyCombine[2] = {false, false};
};

// copy: a blocking frame; total: the batch's work items
inline Batch batch(const Facts &f, const Knobs &k, const Layout &L, bool copy, int maxDepth, unsigned total) {
    Batch b;
    const bool cnt = k.countTraversal;
    b.fuse = maxDepth > 0 && k.pathMode == 0 && k.fuseCombine != 0;
    // chained batches (Ctx::chain): asynchronous camera-pool megakernel batches over
    // 4-wide float nodes whose items fit the ring's slot bits
    b.mayChain = b.fuse && !copy && !cnt && k.chainBatches != 0 && L.poolWords != 0 && L.fmt == kWideFloat &&
                 total <= (1u << kChainMaxShift);
    // the LDS scene copy's node boxes trimmed to the render pad (HIPPT_OPT_RENDER_PAD;
    // megakernel over an LDS-resident 4-wide float tree only)
    b.trimWanted = k.pathMode == 0 && L.ldsScene && L.fmt == kWideFloat && k.renderPad != 0;
    for (int chained = 0; chained < 2; ++chained) {
        // claim size: 512 items for the Lambertian kernels' chained and whole-image
        // batches (Cornell 1080p/64 spp 7.255 -> 7.199 ms, blob70k 18.94 -> 18.91,
        // r5s; chained 1/8 shares Cornell 1.062 -> 1.041, blob70k 2.546 -> 2.547,
        // r5ab); 256 for small unchained batches (1/8 shares: Cornell 1.112 -> 1.137
        // and blob70k 3.00 -> 3.22 with 512) and the general kernel (cornell_mixed
        // 12.06 -> 12.22)
        b.chunk[chained] = k.chunk > 0 ? k.chunk
                           : k.pathMode == 0 && !f.full && (chained || total >= kWholeImageItems) ? 512u
                                                                                                  : 256u;
        // camera-pool megakernels: samples of pixels that cannot see the scene skip the
        // traversal (HIPPT_OPT_SKY_RECT).
        // (the one camera-pool kernel without the sky path, hippt_kernels.hip SKY: the timed
        // unchained general LDS kernel with the spilling stack)
        b.skyWanted[chained] = k.pathMode == 0 && L.poolWords != 0 && k.skyRect &&
                               !(f.full && L.ldsScene && L.spills && !chained && !cnt);
        b.skyCombine[chained] = k.skyCombine != 0 && b.skyWanted[chained] &&
                                sky_combine_kernel(cnt, L.ldsScene, f.full, L.spills, L.poolWords != 0, chained != 0);
    }
    return b;
}

// The automatic cap's ceiling: 16 for trees in global memory, 8 for LDS-resident scenes.  A bigger
// cap makes a burst's groups bigger (a 1/8 row share's 20 steps: 3 launches instead of 4), and the
// launch after a group combines the whole group: hidden behind a global tree's slower batches
// (blob70k 1/8 share 2.538/2.539 -> 2.497/2.493 ms, 1/4 share 4.799/4.778 -> 4.754/4.754), exposed
// beside Cornell's (1/8 share 0.991/0.989 -> 1.025/1.015: the last launch's 16-batch combine adds
// ~0.9 ms), r6n.
// Batches of more than 2^26 samples (whole 1080p/64 spp images) take cap 8 (r6aw/r6ax: blob70k 22,302 ->
// 22,391 M/s against cap 3, cornell_mixed 35,314 -> 35,422, Cornell chained at 8 as above; cap 2 and 6
// lower or equal); the ring (16 slots) stays within the scratch budget (ring_plan) or the cap shrinks.
inline unsigned chain_cap(long long option, unsigned total, bool ldsScene) {
    if (option > 0) return unsigned(std::min<long long>(option, 16));
    const double c = total > kWholeImageItems ? 8.0 : std::round(4e8 / double(std::max(1u, total)));
    return unsigned(std::clamp(c, 2.0, ldsScene ? 8.0 : 16.0));
}

// The ring slots of a run whose launches trace up to `cap` batches: the power of two >= 2 x cap (a
// launch traces up to cap batches while up to cap batches before its own wait for its combine), at
// most kChainSlotsMax.  The one definition: ring_plan and the protocol model (tests/native/
// chain_model.cpp) size their rings with it.
inline unsigned ring_slots(unsigned cap) {
    unsigned slots = 2;
    while (slots < 2 * cap) slots <<= 1;
    return std::min(slots, kChainSlotsMax);
}

// The ring of a run of `total`-item batches: 2^shift samples per slot (the slot bits above them in
// an item), ring_slots(cap) slots, 12 bytes per sample.  The ring stays within the sample-scratch
// budget (HIPPT_OPT_SCRATCH_MB): the cap shrinks until it fits, and a batch whose smallest ring
// (2 slots) does not fit runs unchained (bytes = 0).  (blob70k at 1080p/64 spp and cap 8
// asked for 25.8 GB whatever the budget.)
struct RingPlan {
    unsigned cap = 0, slots = 0, shift = 0;
    size_t bytes = 0;
};
inline RingPlan ring_plan(unsigned total, long long option, bool ldsScene, size_t budget) {
    RingPlan r;
    r.shift = 6;
    while ((1u << r.shift) < total) ++r.shift;
    const size_t slotBytes = (size_t(1) << r.shift) * 3 * sizeof(float);
    for (unsigned cap = chain_cap(option, total, ldsScene); cap >= 1; --cap) {
        const unsigned slots = ring_slots(cap);
        if (size_t(slots) * slotBytes <= budget) {
            r.cap = cap;
            r.slots = slots;
            r.bytes = size_t(slots) * slotBytes;
            return r;
        }
    }
    return r;
}

}  // namespace plan
}  // namespace hippt
