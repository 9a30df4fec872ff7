// hippt_refit.h — launch interface of the device refit (hippt_refit.hip): new triangle vertices
// into the uploaded scene's primitive records and both float trees, in place and in stream order
// (include/hippt.h hipptUpdateVertices).  The definition the kernels are held to is the host's
// refit_bvh (bvh_builder.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

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

}  // namespace hippt
