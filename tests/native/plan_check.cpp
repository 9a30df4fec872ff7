// plan_check.cpp — traversal planning (qt-raytracer_amd/csrc/hippt_plan.h) from the host
// (tests/test_plan.py).  Host-compiled: the product's own planner, nothing else.
//
// usage: plan_check rows FILE
//            one case per line of FILE, integers: the facts (numNodes numNodes4 numTris numMats levels
//            stackBound4 full quantTree halfTree), the knobs (bvhWidth ldsScene stackCap bvhQuant
//            ldsTopNodes cameraPool pathMode waveThreshold leafExit nodeExit chunk countTraversal
//            fuseCombine chainBatches renderPad skyRect), the limits (scene block) and the call (profile:
//            0 the knobs as they are, 1 the ray queries' profile; pinhole copy maxDepth total).  Prints
//            the layout and the batch plan of each case, one line of integers.
//        plan_check sweep SCENE_LIMIT BLOCK_BUDGET
//            synthetic facts x knobs: every plan satisfies what launch_mesh (hippt_kernels.hip) and
//            launch_query (hippt_query.hip) check before they launch.  Prints the number of plans and
//            of violations (the first few in words); exit status 1 on any.
//        plan_check ring FILE
//            one case per line of FILE, integers: total option ldsScene budgetBytes.  Prints ring_plan's
//            answer for each: cap slots shift bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bvh_builder.h"  // kStackDepth
#include "hippt_plan.h"

namespace {
using namespace hippt;
using plan::Batch;
using plan::Facts;
using plan::Knobs;
using plan::Layout;
using plan::Limits;

int run_rows(const char *path) {
    FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    long long v[32];
    for (;;) {
        int n = 0;
        while (n < 32 && std::fscanf(f, "%lld", &v[n]) == 1) ++n;
        if (n == 0) break;
        if (n != 32) return 2;
        Facts a;
        a.numNodes = int(v[0]), a.numNodes4 = int(v[1]), a.numTris = int(v[2]), a.numMats = int(v[3]);
        a.levels = int(v[4]), a.stackBound4 = int(v[5]);
        a.full = v[6] != 0, a.quantTree = v[7] != 0, a.halfTree = v[8] != 0;
        Knobs k;
        k.bvhWidth = int(v[9]), k.ldsScene = v[10] != 0, k.stackCap = int(v[11]), k.bvhQuant = int(v[12]);
        k.ldsTopNodes = int(v[13]), k.cameraPool = int(v[14]), k.pathMode = int(v[15]);
        k.waveThreshold = int(v[16]), k.leafExit = int(v[17]), k.nodeExit = int(v[18]), k.chunk = unsigned(v[19]);
        k.countTraversal = v[20] != 0, k.fuseCombine = int(v[21]), k.chainBatches = int(v[22]);
        k.renderPad = int(v[23]), k.skyRect = v[24] != 0;
        const Limits lim{size_t(v[25]), size_t(v[26])};
        if (v[27]) k = plan::query_knobs(k);
        const Layout L = plan::layout(a, k, lim, v[28] != 0);
        const Batch b = plan::batch(a, k, L, v[29] != 0, int(v[30]), unsigned(v[31]));
        std::printf("%d %d %d %d %d %d %d %d %d %u %u %u %d %u %u %d %d %d %u %u %d %d %d\n", int(L.wide), L.numNodes,
                    int(L.ldsScene), L.stackCap, L.stackDepth, int(L.spills), L.spillCap, L.fmt, L.poolWords, L.topBytes,
                    L.poolOffset, L.refBits, L.waveThreshold, L.leafExit, L.nodeExit, int(b.fuse), int(b.mayChain),
                    int(b.trimWanted), b.chunk[0], b.chunk[1], int(b.skyWanted[0]), int(b.skyWanted[1]),
                    int(plan::wants_half(a, k, lim)));
    }
    std::fclose(f);
    return 0;
}

int run_ring(const char *path) {
    FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    long long total, option, lds;
    unsigned long long budget;
    while (std::fscanf(f, "%lld %lld %lld %llu", &total, &option, &lds, &budget) == 4) {
        const plan::RingPlan r = plan::ring_plan(unsigned(total), option, lds != 0, size_t(budget));
        std::printf("%u %u %u %llu\n", r.cap, r.slots, r.shift, (unsigned long long)r.bytes);
    }
    std::fclose(f);
    return 0;
}

long long plans = 0, violations = 0;

void violation(const char *what, const Facts &a, const Knobs &k, bool query) {
    if (++violations > 8) return;
    std::printf("VIOLATION %s%s: nodes %d/%d tris %d mats %d levels %d bound %d full %d quantTree %d halfTree %d | width %d "
                "lds %d cap %d quant %d top %d pool %d mode %d\n",
                what, query ? " (query profile)" : "", a.numNodes, a.numNodes4, a.numTris, a.numMats, a.levels,
                a.stackBound4, int(a.full), int(a.quantTree), int(a.halfTree), k.bvhWidth, int(k.ldsScene), k.stackCap,
                k.bvhQuant, k.ldsTopNodes, k.cameraPool, k.pathMode);
}

// launch_mesh's and launch_query's checks of the scalars a plan sets
void check(const Facts &a, const Knobs &k, const Limits &lim, bool pinhole, bool query) {
    const Layout L = plan::layout(a, k, lim, pinhole);
    ++plans;
#define NEED(c, what) \
    if (!(c)) violation(what, a, k, query)
    NEED(L.stackDepth >= 1 && L.stackDepth <= kStackDepth, "1 <= stackDepth <= kStackDepth");
    NEED(!L.wide || (L.stackCap >= 1 && L.stackCap + 2 <= L.stackDepth), "stackCap + 2 <= stackDepth");
    NEED(L.wide == (L.fmt != kWide2) && L.fmt >= kWide2 && L.fmt <= kWideHalf, "the format and the width agree");
    NEED(!(L.ldsScene && L.fmt >= kWideQuant), "LDS scenes read float nodes");
    const unsigned nodeShift = L.fmt == kWideQuant ? 6 : 7;  // whole nodes of the LDS-read format
    NEED(!L.topBytes || (!L.ldsScene && L.wide), "no top for LDS scenes or 2-wide trees");
    NEED(L.topBytes % (1u << nodeShift) == 0, "the top is whole nodes");
    NEED(L.topBytes <= (unsigned(L.numNodes) << nodeShift), "the top is at most the tree");
    NEED(L.fmt != kWideHybrid || L.topBytes > 0, "hybrid trees start in LDS");
    NEED(!(L.ldsScene && L.fmt == kWideFloat) || (L.refBits >= 8 && L.refBits <= 20), "8 <= refBits <= 20");
    NEED(!L.poolWords || ((L.fmt == kWideFloat || L.fmt == kWideHalf) &&
                          (L.poolWords == kPoolWordsPinhole || L.poolWords == kPoolWordsFull)),
         "a pool only over float or half nodes, of 5 or 8 words");
    const bool lds = L.ldsScene;
    const size_t bytes = mesh_lds_bytes(L.stackDepth, lds ? L.numNodes : 0, lds ? a.numTris : 0, L.wide, L.topBytes,
                                        lds ? a.numMats : 0, L.poolWords);
    NEED(!L.poolWords ||
             L.poolOffset == bytes - (size_t(L.poolWords) * 64 + kWaveWords) * (kMeshBlock / 64) * sizeof(float),
         "poolOffset is the layout's bytes before the pool");
    NEED(L.fmt != kWideQuant && L.fmt != kWideHybrid ? true : a.quantTree, "8-bit nodes need an 8-bit tree");
    NEED(L.fmt != kWideHalf || (a.halfTree && plan::wants_half(a, k, lim)), "half nodes need the half tree, asked for");
    NEED(L.spills == (L.wide && a.stackBound4 > L.stackCap), "spills");
    NEED(!L.spills || L.spillCap >= a.stackBound4, "the spill area holds the stack bound");
    NEED(L.waveThreshold >= 0 && L.waveThreshold <= 64 && L.leafExit <= 64 && L.nodeExit <= 64, "loop parameters");
    if (query) {  // launch_query: float nodes of either width, a top of 128-byte nodes, no pool
        NEED(L.fmt == kWide2 || L.fmt == kWideFloat, "queries read float nodes");
        NEED(L.poolWords == 0, "queries have no pool");
        NEED(!L.wide || L.spillCap > 0, "a 4-wide query has a spill area");
    }
    // the batch plan: a chained batch is a camera-pool batch over 4-wide float nodes, with both exits of
    // the claim size whole waves
    for (unsigned total : {768u, 1u << 26, (1u << 27) + 64u}) {
        const Batch b = plan::batch(a, k, L, false, 2, total);
        NEED(!b.mayChain || (L.poolWords && L.fmt == kWideFloat && total <= (1u << kChainMaxShift) && k.pathMode == 0),
             "only camera-pool float-node megakernel batches chain");
        NEED(b.chunk[0] >= 64 && b.chunk[0] % 64 == 0 && b.chunk[1] >= 64 && b.chunk[1] % 64 == 0, "claims are whole waves");
        NEED(!b.skyWanted[0] || L.poolWords, "the sky rectangle is the camera-pool kernels'");
        NEED(!b.trimWanted || (L.ldsScene && L.fmt == kWideFloat), "the trim is the LDS float tree's");
    }
#undef NEED
}

int run_sweep(size_t sceneLimit, size_t blockBudget) {
    const Limits lim{sceneLimit, blockBudget};
    // node counts of the 4-wide tree: 1 ... 200k, either side of the LDS scene limit (95 nodes of two
    // primitives each fit 24 KiB, 96 do not) and of kTopOrderNodes
    const int nodes4[] = {1, 7, 95, 96, 1364, 1365, 1366, 19144, 200000};
    // HIPPT_OPT_LDS_TOP_NODES takes -1 ... kTopOrderNodes: the ends, and values between
    const int tops[] = {-1, 0, 1, 16, plan::kTopOrderNodes};
    for (int n4 : nodes4)
        for (int bound = 1; bound <= 40; ++bound)
            for (int flags = 0; flags < 4; ++flags) {
                Facts a;
                a.numNodes4 = n4;
                a.numNodes = 2 * n4;
                a.numTris = 2 * n4;
                a.numMats = (flags & 1) ? 6 : 3;
                a.levels = bound < kStackDepth ? bound : kStackDepth;
                a.stackBound4 = bound;
                a.full = (flags & 1) != 0;
                a.quantTree = (flags & 2) != 0;
                for (int width : {0, 2, 4})
                    for (int lds = 0; lds < 2; ++lds)
                        for (int cap = 0; cap <= plan::kLdsStackCap; cap = cap ? cap + 1 : 4)
                            for (int quant = -1; quant <= 4; ++quant)  // 4: HIPPT_OPT_BVH_QUANT 3 with a half tree
                                for (int top : tops)
                                    for (int pool = -1; pool <= 1; ++pool)
                                        for (int mode = 0; mode < 2; ++mode) {
                                            Knobs k;
                                            k.bvhWidth = width, k.ldsScene = lds != 0, k.stackCap = cap;
                                            k.bvhQuant = quant == 4 ? 3 : quant;
                                            a.halfTree = quant == 4;
                                            k.ldsTopNodes = top, k.cameraPool = pool, k.pathMode = mode;
                                            check(a, k, lim, false, false);
                                            if (pool != 0 && mode == 0) check(a, k, lim, true, false);
                                            // (the query profile overrides these three)
                                            if (quant == -1 && pool == -1 && mode == 0)
                                                check(a, plan::query_knobs(k), lim, false, true);
                                        }
            }
    std::printf("plans=%lld violations=%lld\n", plans, violations);
    return violations ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "rows")) return run_rows(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "ring")) return run_ring(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "sweep")) return run_sweep(size_t(std::atoll(argv[2])), size_t(std::atoll(argv[3])));
    std::fprintf(stderr, "usage: plan_check rows FILE | plan_check ring FILE | plan_check sweep SCENE_LIMIT BLOCK_BUDGET\n");
    return 2;
}
