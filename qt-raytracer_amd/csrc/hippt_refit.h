// hippt_refit.h — launch interface of the device refit (hippt_refit.hip): new triangle vertices
// into the uploaded scene's primitive records and both float trees, in place and in stream order
// (include/hippt.h hipptUpdateVertices).  The definition the kernels are held to is the host's
// refit_bvh (bvh_builder.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "hippt_env.h"

namespace hippt {

constexpr int kRefitBlock = 256;

// Every pointer is memory of the launch's device.  The scene buffers are a context's (hippt_device.h
// MeshParams layouts: 4-wide interior codes are byte offsets); the rest is the refit's own.
struct RefitBuffers {
    const float *verts;  // numTris * 9 floats by triangle id (the upload's order)
    float4 *tris;        // primitive records in leaf order, 3 per primitive (id in [2].y, sphere tag in [2].z)
    float4 *shade;       // normal + material word per primitive
    uint32_t *nodes2;    // 2-wide float nodes
    uint32_t *nodes4;    // 4-wide float nodes
    float *pbox;         // numPrims * 6: unpadded primitive boxes in leaf order
    float *ubox2;        // numNodes2 * 12: unpadded slot boxes of the 2-wide tree
    float *ubox4;        // numNodes4 * 24: of the 4-wide tree
    unsigned *words;     // [0] bits of the largest |coordinate| of the update, [1] triangles dropped
    float *padOut;       // null, or the word that receives the pad the nodes are refitted with (MeshParams::padWord)
    const int *list2;    // RefitPlan::list2
    const int *list4;    // RefitPlan::list4
    int numPrims, numTris, numNodes2, numNodes4;
};

// Enqueues one update on `s`: the two words zeroed, the primitive pass, then one launch per level of
// each tree, deepest first (level k of a tree is list[level[k] .. level[k + 1]), RefitPlan).
// seedBits: bits of max(|extentHint|, the spheres' box coordinates), what the pad's maxabs starts
// from.
hipError_t launch_refit(const RefitBuffers &b, const std::vector<int> &level2, const std::vector<int> &level4,
                        unsigned seedBits, hipStream_t s);

// ---- the light selection table (include/hippt.h HIPPT_OPT_LIGHT_SELECT) ----------------
// Most lights a table is built for: q_j <= 4096 = 2^12, so the total T of 2^20 - 1 lights stays below 2^32.
// Above it there is no table and the light choice stays uniform.
constexpr int kLightSelectMax = (1 << 20) - 1;
// Whether a scene with n lights has a table: the one place that applies the limit.
constexpr bool light_table_fits(size_t n) { return n >= 1 && n <= size_t(kLightSelectMax); }

// The table's words for n lights and p primitives, as launch_light_table lays them out in one allocation.
constexpr size_t light_table_words(size_t n, size_t p) {
    return n + 4 * n + p + n + (n + kRefitBlock - 1) / kRefitBlock + 2;
}

// Every pointer is memory of the launch's device.  The scene buffers are a context's; the rest is the
// table's own (one allocation of light_table_words words, see light_table_buffers).
struct LightTableBuffers {
    const float4 *tris;   // primitive records in leaf order (RefitBuffers::tris)
    const float4 *shade;  // normal + material word per primitive
    const float4 *mats;   // MeshParams::mats: the emission in [2 m].xyz
    const int *lights;    // leaf-order indices of the emissive primitives by ascending id
    unsigned *cdf;        // numLights: c_j, dense for the search (T = cdf[numLights - 1])
    unsigned *records;    // numLights * 4: primitive id, q_j, c_j, bits of ip_j (hipptSceneDownload)
    float *ipPrim;        // numPrims: ip by primitive in leaf order; the build writes the lights' entries,
                          // the others are zeroed once by the owner
    float *weights;       // numLights: W_j (between the passes)
    unsigned *blockSums;  // one per block of kRefitBlock lights: the block's sum of q, then its offset
    unsigned *words;      // [0] bits of Wmax, [1] T
    int numLights, numPrims;
};

// The pointers of a table in `base` (light_table_words(n, p) words).
LightTableBuffers light_table_buffers(unsigned *base, int numLights, int numPrims);

// Enqueues one build on `s`: Wmax zeroed, then four launches (weights and Wmax, q and the blocks' scans,
// one block over the blocks' sums, offsets + ip + scatter).  light_table_fits(numLights).
hipError_t launch_light_table(const LightTableBuffers &b, hipStream_t s);

// ---- the environment's selection table (include/hippt.h HIPPT_OPT_ENV_SAMPLING) ----------
// The table's words for a map of size x size texels, as env_table_buffers lays them out in one allocation: 8
// bytes per texel (c, k), then per row C, m and, between the passes, V.
constexpr size_t env_table_words(size_t size) { return 2 * size * size + 3 * size; }

// Every pointer is memory of the launch's device.
struct EnvTableBuffers {
    const env::Texel *env;  // the map, size x size
    env::TexelSel *texels;  // size x size: c(x, y) and k(x, y)
    unsigned *rowC;         // size: C_y, dense for the search (T = rowC[size - 1])
    unsigned *rowM;         // size: m_y
    float *rowV;            // size: V_y (between the passes)
    int size;
};

// The pointers of a table in `base` (env_table_words(size) words, 8-byte aligned).
EnvTableBuffers env_table_buffers(const env::Texel *env, unsigned *base, int size);

// Enqueues one build on `s`: three launches (a block per row: W, Wmax, q, c, V; one block over the rows: Vmax,
// m, C; k per texel).
hipError_t launch_env_table(const EnvTableBuffers &b, hipStream_t s);

}  // namespace hippt
