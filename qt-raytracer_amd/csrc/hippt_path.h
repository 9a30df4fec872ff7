// hippt_path.h — launch interface of the path queries (hippt_path.hip): radiance along caller-supplied
// rays and the camera's own rays (include/hippt.h hipptTraceRadiance, hipptCameraRays).
#pragma once

#include "hippt_env.h"
#include "hippt_query.h"

namespace hippt {

// One launch runs the renderer's path from ray i of q.rays with RNG state seeds[i], i in [0, q.numRays),
// and writes radiance[i] = (L.r, L.g, L.b, a) and segments[i] (may be null).  `q` is a ray query's
// launch (hippt_query.h: scene, rays, claim counters, spill area, layout, shade records) whose result
// pointers (t, prim, occluded, hits) and camera are not used.  Every pointer is device memory of the
// launch's device.
//
// Light sampling (HIPPT_OPT_LIGHT_SAMPLING; DESIGN.md §2 "Light sampling", §16): with `lights` the launch
// makes one connection to a light at every Lambertian vertex (null: plain paths).  `lights`: the leaf-order
// indices of the scene's emissive primitives in ascending uploaded id, numLights >= 1 of them; q.full is
// set.  With `scratch` null it is a path query as above; with `scratch` (light sampling only) it is a
// render batch: sample i is camera_sample(q.cam, q.firstItem + i), its radiance goes to
// scratch[3 i .. 3 i + 2] (the combine's layout) and the segments and samples are added to `stats`
// (hippt_device.h kStatWords).  lightMode 2 (HIPPT_LIGHT_SAMPLING_MIS) weights the connection
// and the light met after a Lambertian scatter by the power heuristic; the routes are the same.
// Light selection (HIPPT_OPT_LIGHT_SELECT): with `lightCdf` (light sampling only) the connection
// picks its light by the device-built table (hippt_refit.h LightTableBuffers: cdf and ipPrim) in place of the
// uniform choice, and ip of the light replaces float(numLights); null: uniform, the bytes of before, from the
// kernels of before (the choice is a compile-time flag of the kernel, as MIS is).
// Environment (hipptSetEnvironment): with `env` a miss takes throughput x env(d) of the map
// (hippt_env.h) in place of the sky gradient, from the general kernels (as with `lights`, whatever q.full
// says), and `scratch` may be set without `lights`: a render batch of plain paths.  Null: the bytes of before,
// from the kernels of before (a compile-time flag again).
// Environment sampling (HIPPT_OPT_ENV_SAMPLING): with `envRowC` (under `env` and lightMode 1 or 2)
// every Lambertian vertex connects to the map by its selection table (hippt_refit.h EnvTableBuffers: rowC and
// texels), or by a fair coin to the map or to a light where the scene has lights; `lights` may then be null with
// numLights 0 (a scene without lights under a map).  Null: the bytes and the kernels of before (a flag again).
struct PathParams {
    QueryParams q;
    const float4 *mats;     // MeshParams::mats
    const unsigned *seeds;  // RNG state per ray
    float4 *radiance;
    int *segments;
    int maxDepth;
    const int *lights;
    int numLights;
    int lightMode;  // with `lights`: 1 plain, 2 with MIS (HIPPT_LIGHT_SAMPLING_MIS)
    float *scratch;
    unsigned long long *stats;
    const unsigned *lightCdf = nullptr;  // c_j of the numLights lights, or null (uniform)
    const float *lightIp = nullptr;      // with lightCdf: ip by primitive in leaf order
    const env::Texel *env = nullptr;     // the environment's size x size texels, or null (the sky gradient)
    int envSize = 0;
    const unsigned *envRowC = nullptr;         // with env and lightMode 1 or 2: C_y of the map's selection table, or null
    const env::TexelSel *envTexels = nullptr;  // with envRowC: (c, k) per texel
};

hipError_t launch_path(const PathParams &p, int blocks, hipStream_t s);
int path_blocks_per_cu(const PathParams &p);

// Writes camera_sample's ray of pixels firstItem .. firstItem + numRays - 1 of the image (cam: one frame,
// the whole image as one band) as (origin, 0.001) (direction, +inf) to rays[2 i], rays[2 i + 1] and the
// RNG state it leaves to seeds[i]; either output may be null.
struct CameraRaysParams {
    QueryCam cam;
    float4 *rays;
    unsigned *seeds;
    unsigned numRays, firstItem;
};

hipError_t launch_camera_rays(const CameraRaysParams &p, hipStream_t s);

}  // namespace hippt
