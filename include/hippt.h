/*
 * hippt.h — C ABI of libhippt.so, the MI355X-native (gfx950) path-tracing backend.
 *
 * Drop-in boundary.  The first three entry points are EXACTLY the reference's
 * CUDA backend ABI, so CudaPathTracer.cpp links unchanged with
 * ENABLE_CUDA_BACKEND defined:
 *
 *   cudaPathTracerInit      replaces CudaPathTracerKernel.cu:188-237  (declared CudaPathTracer.cpp:5)
 *   cudaPathTracerRender    replaces CudaPathTracerKernel.cu:239-276  (declared CudaPathTracer.cpp:6)
 *   cudaPathTracerShutdown  replaces CudaPathTracerKernel.cu:278-288  (declared CudaPathTracer.cpp:7)
 *
 * Semantics kept from the reference: Init frees previous buffers and may be called
 * repeatedly (RayTracerFboItem.cpp:520-521 re-inits on frame 0); Render renders ONE
 * sample per pixel for the caller-supplied frameIndex (running average,
 * CudaPathTracerKernel.cu:157-169), blocks until the frame is on the host and returns
 * a library-owned W*H ARGB array (row 0 = v = 0) valid until the next Init/Shutdown;
 * errors are `false` + a library-owned message (null out-pointers allowed); Shutdown is
 * idempotent.  Unlike the reference, every entry point is serialised by an internal
 * mutex (the reference is called from two Qt threads without a lock).
 *
 * The default scene is the reference kernel's built-in 4-sphere scene
 * (CudaPathTracerKernel.cu:113-116).  The hippt* extensions add triangle-mesh scenes
 * (host SAH BVH build + upload), batched multi-sample rendering, multi-GPU row bands,
 * and counters.  The GL-backend shape (GpuPathTracer.h:9-38: renderFrame(spp, depth),
 * resetAccumulation) maps onto hipptRenderFrames / hipptResetAccumulation.
 *
 * No torch types, no HIP types: plain pointers and sizes.
 */
#ifndef HIPPT_H
#define HIPPT_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference ABI (CudaPathTracer.cpp:4-8) ---------------------------------- */
bool cudaPathTracerInit(int width, int height, const char **errorMessage);
bool cudaPathTracerRender(int frameIndex, int maxDepth, const unsigned int **hostPixels,
                          const char **errorMessage);
void cudaPathTracerShutdown(void);

/* Same functions under backend-neutral names. */
bool hipPathTracerInit(int width, int height, const char **errorMessage);
bool hipPathTracerRender(int frameIndex, int maxDepth, const unsigned int **hostPixels,
                         const char **errorMessage);
void hipPathTracerShutdown(void);

/* ---- scene description ---------------------------------------------------------- */
/* Camera as the kernels consume it: RayTracer.h Camera (:545-561) computed in FP64 and
 * stored FP32.  Layout is part of the ABI (80 bytes). */
typedef struct hipptCamera {
    float origin[3], llc[3], horizontal[3], vertical[3], u[3], v[3];
    float lens_radius;
    float reserved;
} hipptCamera;

/* Builds a camera exactly like RayTracer.h Camera::Camera (:545-561). */
void hipptBuildCamera(const double lookfrom[3], const double lookat[3], const double vup[3], double vfovDeg,
                      double aspect, double aperture, double focusDist, hipptCamera *out);

enum { HIPPT_SCENE_SPHERE4 = 0, HIPPT_SCENE_MESH = 1 };

/* Selects the reference built-in 4-sphere scene (the default). */
bool hipptUseBuiltinScene(int sceneId, const char **errorMessage);

/* Triangle mesh: verts = numTris*9 floats (v0,v1,v2), triMaterial = numTris ints in
 * [0,numMaterials), albedo = numMaterials*3 floats (Lambertian, RayTracer.h:473-488).
 * Builds a binned-SAH BVH on the host and uploads it to every device on the next render.
 * The camera is given by RayTracer.h Camera parameters; the aspect ratio is width/height
 * of the current Init (as RayTracerFboItem.cpp:49-56 does). */
bool hipptUploadMesh(const float *verts, const int *triMaterial, int numTris, const float *albedo,
                     int numMaterials, const double lookfrom[3], const double lookat[3], const double vup[3],
                     double vfovDeg, double aperture, double focusDist, const char **errorMessage);

/* Materials of RayTracer.h :473-540.  LAMBERTIAN uses albedo; METAL albedo and fuzz (clamped
 * to <= 1 as Metal's constructor does, :494); DIELECTRIC the index of refraction ir.
 *
 * EMISSIVE is this library's own (the reference has no light): an area light.  albedo[3] holds the
 * emitted radiance (r, g, b), each finite and >= 0, and may exceed 1; fuzz and ir are ignored but must
 * be finite.  The material emits on both sides and never scatters.  Path rule, the same in the
 * renders and in hipptTraceRadiance: a segment whose closest hit is a primitive with an emissive
 * material ends the path there with L.c = throughput.c * emission.c (one float32 multiply per channel;
 * at segment 0 the emission itself).  The segment counts as any hit does, no RNG draw is consumed, and
 * a = 1 if it was segment 0.  The rule applies to every traced segment including the last one the
 * depth allows (the emission check comes before the depth check, as "Ray Tracing: The Next Week" adds
 * `emitted` before it asks whether to recurse): maxDepth = 1 shows lights as lit and everything else
 * black.  Emission (0, 0, 0) is an absorber, so an enclosing emissive sphere is a constant background
 * colour in place of the sky.  hipptUploadScene rejects a negative emission component, a non-finite
 * parameter and a kind outside 0..3 before any device call.  A scene without an emissive material
 * renders the same bytes from the same kernels as before the material existed.  Hit records are
 * unchanged (matFlags carries the material index); the denoiser's albedo' of an emissive hit is 1. */
enum { HIPPT_MAT_LAMBERTIAN = 0, HIPPT_MAT_METAL = 1, HIPPT_MAT_DIELECTRIC = 2, HIPPT_MAT_EMISSIVE = 3 };
typedef struct {
    int kind;
    float albedo[3];
    float fuzz;
    float ir;
} hipptMaterial;

/* General scene: triangles (as hipptUploadMesh) plus spheres = numSpheres*4 floats (center
 * xyz, radius; Sphere, RayTracer.h:274-322), each primitive with a material index into
 * materials[numMaterials].  Either count may be 0, not both.  Ties of the closest hit are
 * broken by primitive id: triangles 0..numTris-1, then spheres.  The reference app's scene
 * (random_scene(), RayTracer.h:599-643, which draws from a nondeterministic RNG) is uploaded
 * as its sphere list. */
bool hipptUploadScene(const float *verts, const int *triMaterial, int numTris, const float *spheres,
                      const int *sphereMaterial, int numSpheres, const hipptMaterial *materials, int numMaterials,
                      const double lookfrom[3], const double lookat[3], const double vup[3], double vfovDeg,
                      double aperture, double focusDist, const char **errorMessage);

/* Triangle mesh read from a Wavefront OBJ or PLY file (the reference has no mesh input):
 * verts = numTris*9 floats (polygons fan-triangulated), triGroup = numTris ints in
 * [0, numGroups): OBJ `usemtl` groups in order of first use (groupNames[g]; "" = faces before
 * any usemtl), PLY: 0.  Feed verts/triGroup to hipptUploadMesh/hipptUploadScene with one
 * material per group.  Library-owned; release with hipptFreeMesh. */
typedef struct {
    float *verts;
    int *triGroup;
    int numTris;
    int numGroups;
    const char *const *groupNames;
    void *owner_;
} hipptMesh;
bool hipptReadMesh(const char *path, hipptMesh *out, const char **errorMessage);
void hipptFreeMesh(hipptMesh *mesh);

/* Optional: replace the camera by a prebuilt one (used as-is, whatever the aspect).
 * Known limit: the BVH's boxes are padded for rays that start within M of the origin, M the largest
 * |coordinate| of the scene and of the camera the scene was uploaded with.  hipptRenderFrames covers a
 * camera moved out to 32 M (the host model of the box test, tests/test_far_rays_cpu.py, loses nothing up
 * to there and loses first hits from 48 M on); beyond that a render may lose
 * surfaces.  Remedy: upload the scene with the far camera, which sizes the pad for it.  The ray and
 * path queries below, the camera queries included, have no such limit. */
bool hipptSetCamera(const hipptCamera *camera, const char **errorMessage);

/* ---- vertex updates (animated or edited meshes) ------------------------------------------------ */
/* New triangle vertices for the uploaded scene, in place: verts = numTris*9 floats in the upload's
 * triangle order, numTris the uploaded scene's triangle count.  Spheres, materials, primitive ids,
 * camera and the BVH's topology stay as uploaded; the primitive records and the boxes of both float
 * trees are recomputed on every device by the builder's own rule (a refit, bit-identical to the
 * host's hipptBvhRefit), so every result is the one a fresh hipptUploadScene of these vertices gives:
 * the BVH only culls.  A refit keeps the topology, so the tree's quality decays under large
 * deformation; hipptUploadScene is the rebuild.
 * Stream order, no drain: every render and ray query enqueued later sees the new triangles, everything
 * enqueued earlier the old ones.  The call does not wait for queued work and reallocates nothing.
 * Host memory is copied into library-owned staging before the call returns.  With HIPPT_VERTS_DEVICE
 * (memory of one of the devices of hipptSetDevices; after an Init) the call returns once the work is
 * enqueued, and the caller keeps the memory unchanged until the next hipptSynchronize or blocking
 * render.  Before an Init, host vertices update the host copy of the scene only.
 * After an update the 8-bit, half-precision and hybrid trees (HIPPT_OPT_BVH_QUANT) are stale: every
 * path reads the float nodes until the next hipptUploadScene (same results).
 * A non-finite coordinate in host memory is rejected and leaves the scene unchanged; in device
 * memory the triangle becomes a record no ray hits, is kept out of every box, and is counted:
 * hipptGetOption(HIPPT_INFO_UPDATE_DROPPED) gives the last update's count (synchronises). */
enum { HIPPT_VERTS_DEVICE = 1 };   /* flags: verts is device memory of one of the contexts' devices */
bool hipptUpdateVertices(const float *verts, int numTris, int flags, const char **errorMessage);

/* Inspection aid (in the spirit of hipptChainAudit): copies context 0's device buffer (device layouts:
 * 2-wide nodes of 16 words as hipptBvhCopy; 4-wide float nodes of 32 words as hipptBvh4Copy except
 * that interior child codes are byte offsets, node * 128; primitive records of 12 words in BVH leaf
 * order, the primitive id in word 9, 1 in word 10 for a sphere; shading records of 4 words: normal and
 * material word) into dst after the queued work; dst null: returns the bytes needed.  -1 on error. */
enum { HIPPT_SCENE_NODES2 = 0, HIPPT_SCENE_NODES4 = 1, HIPPT_SCENE_PRIMS = 2, HIPPT_SCENE_SHADE = 3,
       /* the light selection table (HIPPT_OPT_LIGHT_SELECT below), as the device built it: one record of 4
          words per light in ascending primitive id: the primitive id as uploaded, q_j, c_j, the bits of
          ip_j; 0 bytes for a scene without lights or with more than 2^20 - 1 */
       HIPPT_SCENE_LIGHTS = 4,
       /* the environment (hipptSetEnvironment below) as context 0 holds it, whatever scene is current: one
          record of 16 bytes per texel, row-major, row y indexing w: r, g, b as float32 and a zero word; 0
          bytes without one */
       HIPPT_SCENE_ENVIRONMENT = 5,
       /* the environment's selection table (HIPPT_OPT_ENV_SAMPLING below) as context 0's device built it, for
          a map of S x S texels: S row records of 2 words (m_y, C_y), then S x S texel records of 3 words,
          row-major (q, c, the bits of k): (2 S + 3 S S) 32-bit words; 0 bytes without an environment */
       HIPPT_SCENE_ENV_TABLE = 6 };
long long hipptSceneDownload(int what, void *dst, long long bytes, const char **errorMessage);

/* ---- environment: a settable sky (tests/env_ref.py is the statement of record) ----
 * In place of the sky gradient, an uploaded scene's paths take a miss's radiance from an HDR environment
 * map: wherever a path rule above or below says "miss: thr x sky", thr.c * e.c stands instead, e = env(d):
 *   plain paths:                 L.c = thr.c * e.c               (one multiply)
 *   light sampling modes 1, 2:   L.c = Lacc.c + thr.c * e.c
 * d is the direction of the segment that missed, exactly as the path holds it, at any length: the caller's
 * own for segment 0 of hipptTraceRadiance, the camera's or the scatter's otherwise.  Nothing else changes:
 * the segments, the RNG chain, a, the depth rule, emissive hits and their MIS weights.  Only the scatter
 * sample finds the environment; no connection samples it unless HIPPT_OPT_ENV_SAMPLING (below, beside the
 * light-sampling rules) is set.
 *
 * The map is a square octahedral image of S x S texels E[y][x] (rgb, float32, finite, >= 0, may exceed 1),
 * 1 <= S <= 4096 (at 4096 the device's 16-byte texels are 256 MiB per context).  +y is up and the upper
 * hemisphere is the inner diamond.  The centre of texel (x, y) is u = (2x + 1)/S - 1, w = (2y + 1)/S - 1; its
 * direction has dy = 1 - |u| - |w| and (dx, dz) = (u, w) if dy >= 0, else ((1 - |w|) sg(u), (1 - |u|) sg(w)),
 * then normalised.  env(d) has no transcendental and no square, so a length from 2^-100 to 2^80 gives the
 * words of a unit direction; each line is one IEEE float32 operation in the association written:
 *   s  = (|dx| + |dy|) + |dz|
 *   u  = dx / s;   w = dz / s
 *   if dy < 0:  (u, w) = ((1 - |w|) * sg(u), (1 - |u|) * sg(w))   sg(x) = x < 0 ? -1 : 1, both from the old u, w
 *   h  = 0.5f * float(S)
 *   fx = fminf(fmaxf(fmaf(u, h, h) - 0.5f, 0.0f), float(S - 1))   fy the same from w (minNum/maxNum: NaN gives 0)
 *   x0 = int(fx); x1 = min(x0 + 1, S - 1); a = fx - float(x0)     y0, y1, b the same from fy
 *   per channel: top = fmaf(a, E[y0][x1] - E[y0][x0], E[y0][x0]); bot the same on row y1;
 *                e = fmaf(b, bot - top, top)
 * S = 1 is a constant background colour; equal neighbouring texels give that value exactly.  The filter is
 * bilinear with clamp to edge: across the lower hemisphere's fold lines (the square's border, where the
 * -y hemisphere's directions meet) it is not continuous within half a texel.
 *
 * hipptSetEnvironment: texels = size*size*3 floats, row-major, row y indexing w.  texels NULL with size 0
 * removes the environment: the gradient is back.  Host memory is validated and copied before the call
 * returns: a negative or non-finite texel, a size outside 1..4096 or unknown flags is rejected before any
 * device call, and a rejected call leaves the old environment in place.  With HIPPT_ENV_DEVICE the pointer
 * is memory of one of the contexts' devices (after an Init); it is fetched into the library's host copy and
 * not inspected.  Stream order, as hipptUpdateVertices: work enqueued earlier sees the old environment, work
 * enqueued later the new one.  A call of the size already set waits for nothing queued and reallocates no
 * device memory; a change of size may wait for the queued work of every context (the old buffer is freed),
 * and a device-memory call waits for its fetch.  The environment belongs to the library, not to a scene: it
 * stays across hipptUploadScene, a re-Init and hipptSetDevices until it is removed, and reaches every
 * context.  Before an Init the call sets the host copy only.  The built-in 4-sphere scene ignores it.
 *
 * A mesh render with an environment takes the ray-per-lane route of the light-sampling renders (a path
 * kernel launch per batch over the camera's own samples), whatever HIPPT_OPT_LIGHT_SAMPLING_MODE and
 * HIPPT_OPT_PATH_MODE say, under that route's conditions: no chaining, sky rectangle, render pad or item
 * order (their HIPPT_INFO_* read 0) and no traversal counts.  hipptGetOption(HIPPT_INFO_ENVIRONMENT): the
 * size the last render applied, 0 for the gradient or the built-in scene. */
enum { HIPPT_ENV_DEVICE = 1 };   /* flags: texels is device memory of one of the contexts' devices */
enum { HIPPT_INFO_ENVIRONMENT = 110 };
bool hipptSetEnvironment(const float *texels, int size, int flags, const char **errorMessage);
/* Host only: rgb[3 i ..] = env(dirs[3 i ..]) of the library's host copy, i < n, by the very text the kernels
 * compile (the hook by which a CPU test pins their arithmetic).  Fails without an environment. */
bool hipptEnvLookup(const float *dirs, long long n, float *rgb, const char **errorMessage);
/* dirs[3 (y size + x) ..]: the unit direction of texel (x, y)'s centre (computed in double, rounded once).
 * Nothing is written for a size outside 1..4096. */
void hipptEnvDirections(int size, float *dirs);
/* Host only, double precision: texels (size*size*3 floats) from a lat-long image rgb (width*height*3 floats,
 * row 0 at +y), sampled bilinearly at the texel-centre directions.  Pixel (c, r)'s centre is at
 * theta = pi (r + 1/2) / height from +y and phi = 2 pi (c + 1/2) / width - pi, direction
 * (sin theta cos phi, cos theta, sin theta sin phi); wraps in phi, clamps in theta.  No prefilter: an image
 * much larger than the map aliases. */
bool hipptEnvFromEquirect(const float *rgb, int width, int height, int size, float *texels, const char **errorMessage);

/* ---- devices and row bands ------------------------------------------------------- */
int hipptDeviceCount(void);
/* Render on these devices (one context per device, contiguous row bands); takes effect
 * at the next Init.  Default: the current HIP device only. */
bool hipptSetDevices(const int *deviceIds, int numDevices, const char **errorMessage);
/* Restrict this process to rows [y0, y1) of the image (one-process-per-GPU launch);
 * y1 <= 0 means "to the last row".  Takes effect at the next Init. */
bool hipptSetRowRange(int y0, int y1, const char **errorMessage);
/* Alternative: this process renders rows phase, phase+stride, phase+2*stride, ... (one process
 * per GPU with phase = rank, stride = world size balances the load: row bands of a scene differ
 * by up to 1.6x in cost).  Clears a row range; hipptSetRowRange clears the interleave.  Takes
 * effect at the next Init.  The image is bit-identical for any split. */
bool hipptSetRowInterleave(int phase, int stride, const char **errorMessage);

/* ---- rendering ------------------------------------------------------------------- */
/* Renders `count` samples per pixel as frames firstFrame..firstFrame+count-1; the
 * accumulation buffer ends exactly as after `count` single-frame Render calls.  Blocks
 * until the image is on the host (hostPixels may be null to skip the copy). */
bool hipptRenderFrames(int firstFrame, int count, int maxDepth, const unsigned int **hostPixels,
                       const char **errorMessage);
/* Enqueues the same work without waiting and without a device-to-host copy. */
bool hipptRenderFramesAsync(int firstFrame, int count, int maxDepth, const char **errorMessage);
bool hipptSynchronize(const char **errorMessage);
/* Interactive hand-off (replaces the blocking full-frame copy of CudaPathTracerKernel.cu:261-265
 * for hosts that can show the previous image): enqueues the frames, whose ARGB image lands in one
 * of two library-owned pinned frames (written by the kernel that produces it, or copied after
 * it), and returns without waiting. */
bool hipptRenderFramesPresent(int firstFrame, int count, int maxDepth, const char **errorMessage);
/* Never blocks: *hostPixels = the newest presented image whose transfer has completed (null if
 * none yet), *frames = the frame count accumulated in it.  The image stays valid until the
 * second hipptRenderFramesPresent call after the one that produced it (double buffering). */
bool hipptLatestFrame(const unsigned int **hostPixels, int *frames, const char **errorMessage);
/* Copies the current image (ARGB, W*H) and/or accumulation buffer (RGBA float, W*H*4)
 * of the process's row range into caller memory; rows outside the range are untouched. */
bool hipptReadback(unsigned int *pixels, float *accum, const char **errorMessage);
/* Zeroes the accumulation buffer (GpuPathTracer::resetAccumulation, GpuPathTracer.cpp:85-95). */
bool hipptResetAccumulation(const char **errorMessage);

/* ---- ray queries --------------------------------------------------------------------- */
/* Per-ray answers over the uploaded scene (hipptUploadMesh / hipptUploadScene; after an Init, which
 * creates the device contexts), by the renderer's contract: every t is computed with the renderer's
 * arithmetic, and the BVH only culls.  A call runs after the work already queued on its device,
 * waits for its own work only and leaves pending asynchronous frames, the image and the counters of
 * hipptGetStats untouched.  A ray with a non-finite origin, direction or tmin, a NaN tmax, an
 * all-zero direction, tmin < 0 or tmax <= tmin is a miss (tmax may be +inf).
 * Every other ray is answered exactly within this domain, which a caller can check (M: the largest
 * |coordinate| of the uploaded scene and its camera; omax, dmax: the largest |component| of the ray's
 * origin and direction; components of the direction may be zero or of any smaller size):
 *   omax <= 2^20 M  with  2^-20 <= dmax <= 2^20,   or   omax <= 8 M  with  2^-100 <= dmax <= 2^80.
 * tests/test_gpu_far_rays.py covers both to their edges.  Outside it a query may miss a surface.  One
 * exception inside it: a triangle whose corners lie on one line has no hit to report; the renderer's
 * arithmetic can still accept one from rounding noise, and a query may or may not. */
enum { HIPPT_RAYS_DEVICE = 1 };   /* flags: every pointer of the call is device memory */

/* rays: numRays x 8 floats: origin xyz, tmin, direction xyz (any length), tmax.
 * Closest hit over the uploaded scene by the renderer's contract: the lexicographic minimum of
 * (t, primitive id) over hits with tmin <= t < tmax; ids are the upload's (triangles 0..numTris-1,
 * then spheres).  t[i] = +inf and prim[i] = -1 on a miss.  t or prim may be null.  Blocking.
 * Host memory is cut into contiguous shares over the devices of hipptSetDevices and staged in
 * slices (HIPPT_OPT_QUERY_SLICE); with HIPPT_RAYS_DEVICE the pointers (rays 16-byte aligned) must
 * be memory of one of those devices, and the whole batch runs there unstaged. */
bool hipptTraceRays(const float *rays, long long numRays, int flags, float *t, int *prim, const char **errorMessage);
/* occluded[i] = 1 if any primitive is hit with tmin <= t < tmax, else 0 (stops at the first one found). */
bool hipptOccluded(const float *rays, long long numRays, int flags, unsigned char *occluded, const char **errorMessage);
/* The camera ray of sample `frame` of every pixel of the current Init (the ray hipptRenderFrames
 * starts that sample with: same seed, jitter and lens draw), traced with tmin 0.001, tmax inf:
 * t and prim hold width*height entries, row 0 = v = 0. */
bool hipptTraceCamera(int frame, int flags, float *t, int *prim, const char **errorMessage);

/* Hit records: everything the renderer knows about the closest hit, formed with the renderer's
 * arithmetic (bit for bit what its scatter step starts from).
 * One closest hit, 32 bytes.  A miss: t = +inf, prim = -1, normal/u/v = 0, matFlags = -1. */
typedef struct hipptHit {
    float t;          /* as hipptTraceRays */
    int   prim;       /* as hipptTraceRays */
    float normal[3];  /* the renderer's shading normal at the hit, faced against the ray: a triangle's
                       * unit normal as uploaded (or as the last hipptUpdateVertices refitted it), a
                       * sphere's (p - centre) / radius at p = origin + t * direction; negated unless
                       * dot(direction, normal) < 0 */
    float u, v;       /* triangles: hit point = (1-u-v) v0 + u v1 + v v2; spheres: 0 */
    int   matFlags;   /* bits 0..29 material index as uploaded; HIPPT_HIT_SPHERE; HIPPT_HIT_BACKFACE */
} hipptHit;
/* HIPPT_HIT_BACKFACE: the normal was negated (the ray met the side the stored normal points away from). */
enum { HIPPT_HIT_SPHERE = 1 << 30, HIPPT_HIT_BACKFACE = (int)(1u << 31) };
/* hipptTraceRays with a record per ray: rays, validity, tmin/tmax, ties, blocking, shares, slices and
 * HIPPT_RAYS_DEVICE as there (hits then 32-byte aligned memory of the rays' device). */
bool hipptTraceHits(const float *rays, long long numRays, int flags, hipptHit *hits, const char **errorMessage);
/* hipptTraceCamera with a record per pixel: width*height records, row 0 = v = 0. */
bool hipptTraceCameraHits(int frame, int flags, hipptHit *hits, const char **errorMessage);

/* ---- path queries -------------------------------------------------------------------------- */
/* Radiance along caller-supplied rays: the renderer's path started from ray i with
 * RNG state seeds[i] instead of from a camera sample: what a fisheye or orthographic camera, a light
 * probe or a lightmap texel sees, with the renderer's own bounce loop, materials, RNG chain and sky.
 * rays: as hipptTraceRays (layout, validity, tmin / tmax).  Segment 0 is the closest hit of ray i with
 * the ray's own tmin and exclusive tmax; every later segment uses tmin 0.001 and no tmax, as the
 * renderer does.  On a miss L = throughput x sky of the segment's direction; a hit on the segment with
 * depth + 1 >= maxDepth gives L = 0; otherwise the path scatters as the renderer's materials do, and an
 * absorbed path gives L = 0.
 * radiance[4i..4i+3] = (L.r, L.g, L.b, a), a = 1.0f if segment 0 hit something, else 0.0f;
 * segments[i] (segments may be null) = the closest-hit queries the path made.  An invalid ray (as
 * hipptTraceRays: non-finite origin, direction or tmin, NaN tmax, zero direction, tmin < 0,
 * tmax <= tmin) gives (0, 0, 0, 0) and 0 segments.
 * Every word is the renderer's arithmetic and the BVH only culls: no bit depends on the tree, its
 * width, where it lives, the slice size or the device split.
 * maxDepth < 1, a null rays, seeds or radiance with numRays > 0, a negative count, unknown flags, the
 * built-in scene or no Init return false with a message before any device call; numRays == 0 succeeds.
 * flags: HIPPT_RAYS_DEVICE as the ray queries (every pointer memory of one context's device; rays and
 * radiance 16-byte aligned, seeds and segments 4-byte aligned); host memory is shared over the devices
 * and staged in slices (HIPPT_OPT_QUERY_SLICE).  Blocking: runs behind the queued work, waits for its
 * own event only, and leaves pending frames, the image, hipptGetStats and the chain audit as if it had
 * not been made.  One sample per ray and call: repeat rays with different seeds and average. */
bool hipptTraceRadiance(const float *rays, const unsigned int *seeds, long long numRays, int maxDepth,
                        int flags, float *radiance, int *segments, const char **errorMessage);
/* The rays hipptRenderFrames starts sample `frame` of every pixel of the current Init with, and the RNG
 * state each is left with after the camera sample (jitter and lens draw): width*height rays (origin,
 * 0.001, direction, +inf) and seeds, row 0 = v = 0; either output may be null, not both.  Arguments,
 * state checks and flags as hipptTraceCamera.  hipptTraceRadiance of these rays and seeds is exactly
 * sample `frame` of hipptRenderFrames; callers can also bend the rays before tracing them. */
bool hipptCameraRays(int frame, int flags, float *rays, unsigned int *seeds, const char **errorMessage);

/* ---- denoiser ---------------------------------------------------------------------------- */
/* An edge-avoiding A-trous wavelet filter (Dammertz et al. 2010) over the accumulation buffer, on the
 * device, guided by the hit records of one camera sample (what hipptTraceCameraHits returns) and the
 * uploaded materials.  Per pixel p, with c(p) the accumulation's rgb, in IEEE float32 + - * / only:
 *   albedo'(p)  per channel the material's albedo where p is a hit of a HIPPT_MAT_LAMBERTIAN material
 *               and that channel is >= 2^-6, else 1;  i_0(p) = c(p) / albedo'(p)
 *   pass k      (k = 0 .. passes - 1, s = 2^k): a sky pixel keeps i_k(p); a hit pixel takes the 25 taps
 *               q = p + s * (dx, dy), dy = -2..2 outside, dx = -2..2 inside, skipping q outside the
 *               image or over the sky, each with the weight
 *                 w = ((K[|dy|] K[|dx|] * wn) * wz) * wc,   K = {3/8, 1/4, 1/16}
 *                 wn = max(0, n_p . n_q) squared normalPower times
 *                 wz = 1 / (1 + xz^2), xz = |t_p - t_q| / (sigmaDepth * (t_p * s))
 *               wc = 1 / (1 + |i_k(p) - i_k(q)|^2 / (sigmaColor / s)^2)
 *               and i_{k+1}(p) = sum(w i_k(q)) / sum(w), summed in tap order
 *   output      rgba(p) = (i_passes(p) * albedo'(p), 1); the pixel word is the renderer's own of it.
 * DESIGN.md section 13 has the order of every operation; the result is reproducible bit for bit.
 * The call flushes what readers of the image flush (as hipptReadback), reads the accumulation and writes
 * buffers of its own and the caller's outputs only: the accumulation, the image, the frame count, the
 * counters of hipptGetStats and the chain audit are as if it had not been made.  It needs an uploaded
 * scene (the built-in scene has no records) and one context that holds every row of the image: with
 * more than one device, a row range or a row interleave it fails. */
enum { HIPPT_DENOISE_NO_DEMODULATE = 1,   /* albedo' = 1 everywhere */
       HIPPT_DENOISE_DEVICE = 2 };        /* pixels / rgba are device memory of the context's device
                                             (rgba 16-byte aligned), checked as hipptTraceHits checks */
typedef struct hipptDenoiseParams {       /* 32 bytes, part of the ABI */
    int   passes;       /* 0..8; pass k uses tap spacing 2^k.  default 5 */
    int   guideFrame;   /* camera sample whose hit records guide the filter (>= 0).  default 0 */
    int   normalPower;  /* 0..10: normal weight = max(0, n_p.n_q)^(2^normalPower), by repeated squaring.  default 6 */
    int   flags;
    float sigmaColor;   /* > 0, finite.  default 1.0 */
    float sigmaDepth;   /* > 0, finite.  default 0.05 */
    float reserved[2];  /* must be 0 */
} hipptDenoiseParams;
void hipptDenoiseDefaults(hipptDenoiseParams *out);
/* params null = defaults.  pixels: W*H output words (current HIPPT_OPT_PIXEL_FORMAT), rgba: W*H*4 floats
 * (linear, alpha 1), row 0 = v = 0; either may be null, not both.  Blocking: runs after the work
 * already queued and waits for its own.  Every argument error returns false with a message before any
 * device call. */
bool hipptDenoise(const hipptDenoiseParams *params, unsigned int *pixels, float *rgba, const char **errorMessage);

/* ---- counters and options ---------------------------------------------------------- */
typedef struct hipptStats {
    unsigned long long segments;      /* closest-hit queries traced (rays x bounces) */
    unsigned long long pixelSamples;  /* pixel samples rendered */
    unsigned long long nodeVisits;    /* BVH interior nodes visited (HIPPT_OPT_COUNT_TRAVERSAL) */
    unsigned long long triTests;      /* ray-triangle tests (HIPPT_OPT_COUNT_TRAVERSAL) */
    double traceMs;                   /* summed device time of the path-trace kernel launches */
    double combineMs;                 /* summed device time of the accumulate kernel launches */
    int traceLaunches;
    int combineLaunches;
    int bvhNodes;                     /* scene info */
    int bvhDepth;
    int numTris;
    int numDevices;
} hipptStats;

bool hipptGetStats(hipptStats *out);
void hipptResetStats(void);
/* Raw device counters (profiling): [0] segments, [1] pixel samples, [2] node visits,
 * [3] triangle tests, [4 + 2k] / [5 + 2k] wave-level / lane-level passes of mesh-kernel
 * phase k (HIPPT_OPT_COUNT_TRAVERSAL builds only): 0 outer loop, 1 camera ray, 2 traversal
 * round, 3 interior node, 4 leaf, 5 triangle, 6 shading, 7 unit-sphere rejection.
 * Returns the number of words written (<= n, <= 32). */
int hipptGetCounters(unsigned long long *out, int n);

enum {
    HIPPT_OPT_COUNT_TRAVERSAL = 1,  /* 1: count node visits / triangle tests (slower) */
    HIPPT_OPT_WAVE_THRESHOLD = 2,   /* lanes still traversing below which a wave goes to shade; -1 (default):
                                       24 for LDS-resident scenes and spheres / Metal / Dielectric over trees
                                       in global memory, 40 for Lambertian scenes over trees in global memory
                                       (32 before round 6) */
    HIPPT_OPT_SCRATCH_MB = 3,       /* cap of the per-batch sample scratch per device (32768: one batch for 4K x 256 spp) */
    HIPPT_OPT_CHUNK = 4,            /* work items a wave takes from the global queue at once (64..2^20, a
                                       multiple of 64); 0 (default): automatic, 512 for chained or
                                       whole-image (>= 2^26 samples) batches of the Lambertian megakernel,
                                       else 256 */
    HIPPT_OPT_BLOCKS_PER_CU = 5,    /* persistent-grid residency (0 = occupancy query) */
    HIPPT_OPT_LDS_SCENE = 6,        /* 1 (default): small scenes are copied into LDS per block */
    HIPPT_OPT_PATH_MODE = 8,        /* 0 (default): persistent megakernel; 1: wavefront kernels */
    HIPPT_OPT_WAVEFRONT_SLOTS = 9,  /* wavefront path-state slots per device, 64..2^28 (default 2^27) */
    HIPPT_OPT_BVH_LEAF = 10,        /* max primitives per BVH leaf, 1..15 (default 2); applies at the next upload */
    HIPPT_OPT_BVH_TRAVERSAL_COST = 11, /* SAH node-step cost in 1/100 primitive tests; next upload */
    HIPPT_OPT_BVH_MAX_DEPTH = 12,   /* interior-level bound (LDS stack per lane), 1..32; next upload */
    HIPPT_OPT_DEVICE_ROWS = 13,     /* hipptSetDevices split: 1 (default) interleaved rows, 0 bands; next Init */
    HIPPT_OPT_LEAF_EXIT = 14        /* node loop yields to the leaf loop once <= this many lanes lack a
                                       leaf; -1 (default): automatic (LDS scenes 12, 4 for the general kernel
                                       and the wavefront; trees in global memory 12 for the general kernel,
                                       22 for Lambertian scenes (17 before round 6)) */
    , HIPPT_OPT_NODE_EXIT = 15      /* leaf loop yields to the node loop once <= this many lanes hold a leaf
                                       (0 = never); -1 (default): LDS scenes 8; trees in global memory 16 for
                                       the general kernel, 56 for Lambertian scenes (48 before round 6) */
    , HIPPT_OPT_BVH_SAH = 16        /* BVH split search: 1 (default) all axes, exact sweep SAH (32 bins on
                                       nodes over 65536 primitives); 0: 16 bins on the longest axis; next upload */
    , HIPPT_OPT_BVH_WIDTH = 17      /* traversal over the 4-wide (4) or 2-wide (2) BVH (megakernel and wavefront);
                                       0 (default): 4-wide */
    , HIPPT_OPT_STACK_CAP = 18      /* 4-wide traversal: LDS stack entries per lane, 4..30 (deeper stacks spill
                                       to global memory); 0 (default): the tree's bound, at most 19 (30 for
                                       LDS scenes; 13 for a megakernel over a tree in global memory
                                       whose bound exceeds 19, the rest of the LDS holding the top
                                       of the tree) */
    , HIPPT_OPT_BVH_QUANT = 19      /* 4-wide traversal of global-memory trees over 64-byte nodes with 8-bit
                                       child boxes (1) or 128-byte float nodes (0); 2: float top in LDS,
                                       8-bit nodes below (megakernel); 3: 128-byte nodes of half-precision
                                       planes, 4 reads per visit (megakernel and wavefront); -1 (default): 8-bit for
                                       the wavefront path's Lambertian-triangle scenes, else float */
    , HIPPT_OPT_LDS_TOP_NODES = 20  /* 4-wide traversal of global-memory trees: the top of the tree (this many
                                       nodes, breadth-first) is copied into every block's LDS and read from
                                       there; 0: none; -1 (default): automatic (what the LDS budget of the
                                       resident blocks leaves beside the stack) */
    , HIPPT_OPT_BVH_COLLAPSE = 21   /* 2-wide -> 4-wide collapse: 0 greedy (open the largest child), 1 SAH-optimal
                                       (dynamic programming), -1 (default) SAH-optimal for scenes that fit
                                       the LDS scene copy, else greedy; next upload (hipptBvhBuild: -1 =
                                       greedy) */
    , HIPPT_OPT_BVH_NODE_COST = 22  /* SAH-optimal collapse: a 4-wide node visit in 1/100 primitive tests; next upload */
    , HIPPT_OPT_BVH_LEAF4 = 23      /* SAH-optimal collapse: most primitives per 4-wide leaf, 1..15; next upload */
    , HIPPT_OPT_RNG_TABLE = 24      /* 1: random_in_unit_sphere's rejection loop as one lookup in a 16 GiB
                                       per-device table of its outcome for every 32-bit RNG state (built on
                                       first use); 0 (default): the loop.  Same results either way */
    , HIPPT_OPT_PIXEL_FORMAT = 25   /* output frame words of the hipptRenderFrames* calls: HIPPT_PIXEL_ARGB
                                       (default, the CUDA backend's) or HIPPT_PIXEL_RGBA8 (the GL / Vulkan
                                       backends'); cudaPathTracerRender always writes ARGB */
    , HIPPT_OPT_CAMERA_POOL = 26    /* megakernel over a 4-wide float-node tree: each wave generates the camera
                                       rays of its next 64 samples with all lanes at once into an LDS pool
                                       instead of one by one as paths end (1), or not (0); -1 (default):
                                       automatic (on except for the general kernel over a tree in global
                                       memory).  Same results either way */
    , HIPPT_OPT_FUSE_COMBINE = 27   /* megakernel: a batch's running average + tonemap runs inside the next
                                       batch's launch on the same device (beside its paths) instead of as a
                                       launch of its own, whenever nothing reads the image in between (1), or
                                       never (0); -1 (default): automatic.  Same results either way */
    , HIPPT_OPT_ITEM_ORDER = 28     /* megakernel: the work queues hand out runs of 64 pixels in order of an
                                       estimated sample length (camera rays and a few bounce directions on
                                       the host's tree), longest first, so that a wave's lanes hold samples
                                       of similar length (1), or in image order (0); -1 (default): automatic
                                       (on).  Same results either way */
    , HIPPT_OPT_WAVEFRONT_SORT = 29 /* wavefront: the shade kernel appends each block's scattered paths sorted by
                                       direction octant (3) or octant and a 2x2x2 cell of the scene box (6),
                                       so that a wave of the extend kernel traces rays of one kind; 0: in
                                       thread order; -1 (default): automatic (0).  Same results either way */
    , HIPPT_OPT_CHAIN = 30          /* megakernel, camera-pool kernels over 4-wide float nodes: asynchronous
                                       batches with the same scene, camera, rows and frames per batch (each
                                       the same frames again or the next ones) form a run, and a launch whose
                                       batch is drained goes on with the batches posted behind it, up to this
                                       many (1..16), so that the run pays the launch's tail once per that many
                                       batches; the next launch combines them beside its own paths and the
                                       image's readers flush the rest.  0: one launch per batch; -1
                                       (default): automatic (on; 8 batches for batches of more than 2^26
                                       samples, else 2..16 by the batch's size, at most 8 over LDS-resident
                                       scenes).  Same results either way */
    , HIPPT_OPT_CHAIN_AUDIT = 31    /* 1: chained launches record, per batch of each run, the work items they
                                       traced (count and a hash of their indices), the frames and the launch
                                       they traced them with, and the pixels, frames and launch of the batch's
                                       combine; read with hipptChainAudit.  0 (default): off.  Takes effect at
                                       the next run.  Same images either way (a testing aid) */
    , HIPPT_OPT_PIXEL_TILE = 32     /* the item order's (HIPPT_OPT_ITEM_ORDER) unit of 64 pixels: tiles of this
                                       many columns x 64 / it band rows (8, 16 or 32; the image width a
                                       multiple of it), or 64 consecutive pixels of a row (0); -1 (default):
                                       automatic (8 for a band of consecutive rows, 0 for interleaved row
                                       shares).  Same results either way */
    , HIPPT_OPT_QUERY_SLICE = 33    /* ray queries from host memory: rays per slice staged through a device's
                                       buffers, 64..2^28; 0 (default): automatic (2^22).  Same results either
                                       way */
    , HIPPT_OPT_RENDER_PAD = 34     /* render megakernel over an LDS-resident 4-wide float tree: the node boxes
                                       of its LDS scene copy keep a pad of M * 2^-value (17..21) of the
                                       builder's M * 2^-16 (M: the largest |coordinate| of the scene and the
                                       camera), so that a scattered ray's own flat leaf is culled at its
                                       parent's visit; 0: the builder's pad, no trim.  Default 19 (DESIGN.md
                                       §5).  Applied only where the pad's bound holds: the camera's origin (lens
                                       included; hipptSetCamera may move it) within that M, and every
                                       triangle's two edges from its first vertex meeting at a sine of at least
                                       0.3 (not known after a device-memory hipptUpdateVertices until the host
                                       copy has caught up); otherwise, and for trees in global memory, the
                                       wavefront path and the ray queries, the builder's pad stays
                                       (HIPPT_INFO_RENDER_PAD: 0).  Same results either way */
    , HIPPT_OPT_SKY_RECT = 35       /* camera-pool render megakernels: 1 (default) a sample whose pixel lies
                                       outside the screen rectangle the scene's bounding box projects into
                                       (widened by a pixel) is finished as a sky miss without a traversal,
                                       where a wave's 64 new work items are all of that kind; 0: every sample
                                       is traced.  The rectangle follows the camera (hipptSetCamera) and the
                                       scene; none for a lens camera (aperture != 0), a camera inside or beside
                                       the scene's box, a camera so far away for its focus distance that the
                                       rounding of a ray's direction is more than a quarter of a pixel, the one
                                       camera-pool kernel without the path (the unchained general kernel over an
                                       LDS-resident tree whose stack spills), or while a hipptUpdateVertices is ahead of the host copy
                                       (from device memory, or of a scene too large for the LDS copy;
                                       HIPPT_INFO_SKY_RECT_PIXELS: 0).  Same results either way;
                                       with HIPPT_OPT_COUNT_TRAVERSAL, nodeVisits counts only the traversals
                                       made */
    , HIPPT_OPT_SKY_COMBINE = 41    /* -1 (default, automatic): a batch that has a sky rectangle (HIPPT_OPT_SKY_RECT)
                                       and an item order table (HIPPT_OPT_ITEM_ORDER), is neither counted
                                       (HIPPT_OPT_COUNT_TRAVERSAL) nor audited (HIPPT_OPT_CHAIN_AUDIT) and renders
                                       under the built-in gradient sky leaves the 64-pixel runs that lie wholly
                                       outside the rectangle out of its work queues; the combine of that batch
                                       computes their samples' radiance (a function of pixel, frame and the
                                       batch's camera) instead of reading it.  0: such runs are finished by the
                                       tracing kernel, as before the option existed.  Same results and the same
                                       hipptGetStats counts either way (HIPPT_INFO_SKY_COMBINE: the band pixels of
                                       the last batch the combine finished, 0 when the mode did not apply).
                                       Other values are rejected */
    , HIPPT_OPT_DENOISE_TIMING = 36 /* 1: hipptDenoise brackets each of its stages with timing events and keeps
                                       their device times (HIPPT_INFO_DENOISE_NS); 0 (default): no events.
                                       Same results either way (a measuring aid) */
    , HIPPT_OPT_LIGHT_SAMPLING = 37 /* 1: next-event estimation: every Lambertian vertex of a path makes one
                                       connection to a light (the path rule below); 0 (default): a path finds
                                       a light only by hitting it, byte for byte as before the option
                                       existed, from the same kernels.  Takes effect at the next render or
                                       hipptTraceRadiance, without a new upload.  With 1 and no emissive
                                       primitive in the scene the option-off code runs.  Renders under it
                                       are traced by a ray-per-lane kernel into the batch scratch and
                                       combined by the deferred combine: no chaining, sky rectangle, render
                                       pad or item order (their HIPPT_INFO_* read 0), and
                                       HIPPT_OPT_COUNT_TRAVERSAL's counts are not reported.  Accepts 0 and 1
                                       only, as it always did; it is the on/off form of
                                       HIPPT_OPT_LIGHT_SAMPLING_MODE, sets the same word and reads it (so it
                                       reads 2 while the mode is HIPPT_LIGHT_SAMPLING_MIS) */
    , HIPPT_OPT_LIGHT_SAMPLING_MODE = 38 /* the light-sampling mode: 0 and 1 as HIPPT_OPT_LIGHT_SAMPLING;
                                       HIPPT_LIGHT_SAMPLING_MIS (2): the same connection and the light hit
                                       after a Lambertian scatter each weighted against the other (the second
                                       rule below), which bounds what one connection can add.  Everything
                                       said of HIPPT_OPT_LIGHT_SAMPLING 1 holds for 2: the render route, the
                                       next call without an upload, the option-off code for a scene without
                                       an emissive primitive */
    , HIPPT_OPT_LIGHT_SELECT = 39   /* how a connection picks its light under HIPPT_OPT_LIGHT_SAMPLING_MODE 1 and 2:
                                       0 (default) uniformly over the list, byte for byte as before the option
                                       existed; HIPPT_LIGHT_SELECT_POWER (1): in proportion to area x emission, by
                                       a table the device builds with the scene and rebuilds behind every
                                       hipptUpdateVertices in stream order (the third rule below).  Other values
                                       are rejected.  Takes effect at the next render or hipptTraceRadiance,
                                       without an upload; ignored while the light-sampling mode is 0 or the
                                       scene has no light, and uniform for more than 2^20 - 1 lights */
    , HIPPT_OPT_ENV_SAMPLING = 40   /* 0 (default): only the scatter sample finds the environment, byte for byte
                                       and kernel for kernel as before the option existed; 1: every Lambertian
                                       vertex connects to the map by a table over its texels that the device
                                       builds behind every hipptSetEnvironment in stream order (the fourth rule
                                       below).  Other values are rejected.  Takes effect at the next render or
                                       hipptTraceRadiance, without an upload or a new hipptSetEnvironment.  It
                                       applies only with an environment set and HIPPT_OPT_LIGHT_SAMPLING_MODE 1
                                       or 2, and then whether or not the scene holds a light: a scene without
                                       lights runs the light-sampling route with an empty light list */
};
/* Light sampling (HIPPT_OPT_LIGHT_SAMPLING 1; this library's own, as the emissive rule is; tests/nee_ref.py
 * restates it in numpy float32 and the GPU matches that bit for bit).  A path carries
 * Lacc = (0, 0, 0) and spec = true (the last scatter was not Lambertian, or there was none yet).
 *   light hit   ends the path, before the depth check: L = Lacc + thr * Le if spec, else L = Lacc
 *   miss        L = Lacc + thr * sky;   depth exhausted or absorbed: L = Lacc
 *   Metal, Dielectric scatter: unchanged; spec = true
 *   Lambertian scatter (a hit with depth + 1 < maxDepth): the renderer's scatter first (new origin p, faced
 *   normal n, thr' = thr * albedo, RNG advanced); spec = false; then, from the same RNG state:
 *     k = min(int(rand01 * float(nLights)), nLights - 1) over the emissive primitives in ascending id
 *     triangle (v0, e1, e2, unit normal ng): a = rand01, b = rand01, folded (a, b) -> (1 - a, 1 - b) if
 *       a + b > 1; q = fmaf(b, e2, fmaf(a, e1, v0)); A = 0.5f * sqrtf(|cross(e1, e2)|^2); nl = ng
 *     sphere (c, r): u = unit(random_in_unit_sphere), the Lambertian scatter's draw; q = fmaf(r, u, c);
 *       nl = u; A = (12.566371f * r) * r
 *     w = q - p; d2 = fdot(w, w); om = w * (1 / sqrtf(d2)); cosS = fdot(n, om); sL = fdot(nl, om)
 *     triangle: cosL = |sL| (two-sided); sphere: cosL = -sL if |p - c|^2 >= r * r, else sL
 *     unless cosS > 0, cosL > 0, d2 > 0 and A > 0 no shadow ray is traced (the draws are consumed)
 *     g = (((cosS * cosL) * A) * float(nLights)) / (3.14159274f * d2); Ld.c = (thr'.c * Le.c) * g
 *     the shadow ray (p, om), tmin 0.001, no tmax, is a closest-hit query: if its hit is light k,
 *     Lacc.c += Ld.c.  The path goes on along the scattered ray.
 * No MIS under 1 (HIPPT_LIGHT_SAMPLING_MIS below adds it); one light per vertex, uniform over the list
 * unless HIPPT_OPT_LIGHT_SELECT (the third rule below) says otherwise.  maxDepth means what it meant: the connection at
 * vertex d stands for the light hit of segment d + 1 and is made exactly when that segment would exist.
 * segments (hipptTraceRadiance, hipptGetStats) count every closest-hit query traced, shadow rays included. */
enum { HIPPT_LIGHT_SAMPLING_MIS = 2 /* a value of HIPPT_OPT_LIGHT_SAMPLING_MODE */ };
/* Light sampling with multiple importance sampling (HIPPT_OPT_LIGHT_SAMPLING_MODE HIPPT_LIGHT_SAMPLING_MIS; the
 * power heuristic, beta = 2, between the connection and the Lambertian scatter sample, whose solid-angle
 * density is exactly cos / pi; tests/mis_ref.py restates it in numpy float32 and the GPU matches that bit for
 * bit).  A path is the rule's above, with these changes.  It carries a float cb in place of
 * spec; cb = -1: the last scatter was not Lambertian, or there was none yet.
 *   Lambertian scatter: the renderer's scatter first, as above; then, with sd the scattered direction as the
 *     renderer stores it and n the faced normal, cb = fdot(n, sd) * (1 / sqrtf(fdot(sd, sd))).
 *     Metal, Dielectric: cb = -1.
 *   connection: the draws, k, q, A, cosS, cosL, d2, the skip conditions and g are the rule's above; one more
 *     skip condition: no shadow ray unless g < +inf; then Ld.c = (thr'.c * Le.c) * (g / fmaf(g, g, 1.0f)).
 *     (g = p_b / p_l with p_b = cosS / pi and p_l = d2 / (cosL * A * nLights); the weight
 *     p_l^2 / (p_l^2 + p_b^2) = 1 / (1 + g^2), so g / (1 + g^2) <= 0.5 and Ld.c <= thr'.c * Le.c / 2.)
 *   light hit with cb < 0 (segment 0, or after Metal or Dielectric): L = Lacc + thr * Le.
 *   light hit with cb >= 0, at t on the segment with direction d from the vertex:
 *     dd = fdot(d, d); d2 = (t * t) * dd; om = d * (1 / sqrtf(dd))
 *     nl = the triangle's stored unit normal, or the sphere's (hit point - c) / r as hipptHit forms it
 *     cosL = |fdot(nl, om)|; A as in the connection (a sphere: (12.566371f * r) * r)
 *     if cb > 0, cosL > 0, d2 > 0 and A > 0: gh = (((cb * cosL) * A) * float(nLights)) / (3.14159274f * d2),
 *       s = gh * gh, and if also s < +inf: wb = s / fmaf(gh, gh, 1.0f)
 *     in every other case wb = 1 (light sampling could not have produced that point)
 *     L.c = Lacc.c + (thr.c * Le.c) * wb.  The hit ends the path before the depth check, as before.
 * Everything else is the rule's above: miss, depth, absorbed paths, the segment counts with the shadow rays,
 * tmin 0.001, "is the closest hit light k", maxDepth.  Each product, sum, quotient and square root is one
 * float32 operation in the association written; 1 / sqrtf(x) is the quotient of 1 and the correctly rounded
 * root.  With maxDepth segments a path returns at most Le_max * (1 + (maxDepth - 1) / 2) when the sky is no
 * brighter than the lights: every connection adds at most thr' * Le / 2. */
enum { HIPPT_INFO_LIGHTS = 107          /* emissive primitives in the uploaded scene */,
       HIPPT_INFO_LIGHT_SAMPLING = 108  /* the value of HIPPT_OPT_LIGHT_SAMPLING_MODE (1 or 2) that the last render
                                           applied if it took the light-sampling route, else 0 */,
       HIPPT_INFO_LIGHT_SELECT = 109    /* the value of HIPPT_OPT_LIGHT_SELECT that the last render applied if it
                                           took the light-sampling route, else 0 (0 too above the light limit) */ };
enum { HIPPT_LIGHT_SELECT_POWER = 1 /* a value of HIPPT_OPT_LIGHT_SELECT */ };
/* Light selection by power (HIPPT_OPT_LIGHT_SELECT HIPPT_LIGHT_SELECT_POWER; tests/select_ref.py restates it in
 * numpy integers and float32 and the GPU matches that bit for bit, the table word for word).  It
 * replaces the selection draw and the factor float(nLights) of the two rules above; nothing else changes.
 * The table, over the lights j = 0 .. n-1 (the emissive primitives in ascending id), is made of integers, so
 * that no word depends on the order in which a parallel scan or reduction adds; each float operation is one
 * float32 operation in the association written:
 *   A_j    the light's area as the connection forms it (triangle: 0.5f * sqrtf(|cross(e1, e2)|^2) from the
 *          primitive record's edges; sphere: (12.566371f * r) * r)
 *   y_j    (Le.r + Le.g) + Le.b of its material
 *   lit_j  A_j > 0 and y_j > 0 (false for NaN);   W_j = lit_j ? A_j * y_j : 0
 *   Wmax   max_j W_j;   flat = not (Wmax > 0 and Wmax < +inf)
 *   q_j    not lit_j: 0;   flat: 1;   else min(4096, max(1, int((W_j / Wmax) * 4096.0f)))     (uint32)
 *   c_j    q_0 + ... + q_j (uint32, inclusive);   T = c_{n-1}
 *   ip_j   q_j > 0 ? float(T) / float(q_j) : 0     (the inverse of the selection probability)
 * n <= 2^20 - 1 keeps T below 2^32; above that there is no table and the choice stays uniform.
 *   selection draw: rng = hash32(rng), one draw, the state advancing exactly as rand01 advances it;
 *     x = (uint64(rng) * T) >> 32.  If T == 0 no light can add anything: no shadow ray is traced and no further
 *     draw is consumed.  Otherwise k is the light with the smallest j such that c_j > x.
 *   connection: the point draws, q, A, cosS, cosL, d2 and the skip conditions are unchanged;
 *     g = (((cosS * cosL) * A) * ip_j) / (3.14159274f * d2); Ld, the MIS weight g / fmaf(g, g, 1) and the
 *     g < +inf condition follow as written above.
 *   MIS, light hit with cb >= 0: gh = (((cb * cosL) * A) * ip_j) / (3.14159274f * d2) with the hit light's ip_j;
 *     a hit light with q_j == 0 gives wb = 1 (light sampling could not have produced that point).
 * Consequences: with equal weights q_j = 4096 and ip_j = float(n) exactly; with one lit light among one the
 * bytes are the uniform rule's (k = 0, ip = 1); a lit light always has q_j >= 1, so none has selection
 * probability 0.  A light's true selection probability differs from q_j / T by a relative amount below
 * T / (q_j * 2^32) (x takes 2^32 values over T cells); the uniform rule's int(u * n) has an error of the same
 * kind.  The table is rebuilt on the device from the refitted primitive records after every hipptUpdateVertices,
 * in stream order behind the refit: work enqueued earlier sees the old table, work enqueued later the new one.  A
 * triangle that a device-memory update dropped for a non-finite coordinate has area 0, hence q_j = 0. */
enum { HIPPT_INFO_ENV_SAMPLING = 111 /* 1 if the last render applied HIPPT_OPT_ENV_SAMPLING, else 0 */ };
/* Environment sampling (HIPPT_OPT_ENV_SAMPLING 1; tests/envs_ref.py restates it in numpy integers and float32 and
 * the GPU matches that bit for bit, the table word for word).  It adds a connection to the map to
 * the three rules above and replaces what a miss after a Lambertian scatter adds.  `fdot`, `rand01`, `hash32`,
 * `sg` and env(d) are the ones above; each float operation is one float32 operation in the association written.
 * The table over the map's texels E[y][x], S x S, is made of integers and of maxima, so that no word depends on
 * the order in which a parallel reduction or scan combines; it has two levels (texels within a row, 12 bits
 * against the row's heaviest; rows against each other, 16 bits), so that T and every R_y stay within 32 bits at
 * S = 4096 and a few sun texels are not buried under 2^24 sky texels at the floor of 1:
 *   uc = float(2x + 1) / float(S) - 1.0f;  wc the same from y                      (the texel's centre)
 *   dy = (1 - |uc|) - |wc|;  (dx, dz) = dy >= 0 ? (uc, wc) : ((1 - |wc|) * sg(uc), (1 - |uc|) * sg(wc))
 *   n2 = fdot(d, d);  J = 1.0f / (n2 * sqrtf(n2))        (solid angle per unit of (u, w) area: 1 / |p|^3)
 *   lum = (E.r + E.g) + E.b;  W = lum * J;  W = (W > 0 and W < +inf) ? W : 0     (NaN, negative, infinite: 0)
 *   per row y:  Wmax_y = max_x W;  q(x,y) = Wmax_y > 0 ? min(4096, max(1, int((W / Wmax_y) * 4096.0f))) : 1
 *               c(x,y) = q(0,y) + ... + q(x,y) (uint32, inclusive);  R_y = c(S-1, y)        (S <= R_y <= 2^24)
 *               V_y = (float(R_y) * 0.000244140625f) * Wmax_y
 *   over rows:  Vmax = max_y V_y;  flat = not (Vmax > 0 and Vmax < +inf)
 *               m_y = flat ? 1 : min(65536, max(1, int((V_y / Vmax) * 65536.0f)))
 *               C_y = m_0 + ... + m_y (uint32, inclusive);  T = C_{S-1}                     (S <= T <= 2^28)
 *   per texel:  k(x,y) = ((float(m_y) / float(T)) * (float(q) / float(R_y))) * (0.25f * (float(S) * float(S)))
 * Every texel and every row has at least 1, black ones included (the bilinear lookup lets a black texel's cell
 * read its lit neighbours), so an all-black map gives a uniform table and there is no T == 0 case.  The
 * solid-angle density of a direction d drawn this way is k(x,y) * |p|^3, p = d / (|dx| + |dy| + |dz|).
 *   connection, at a Lambertian vertex after the scatter (thr', faced normal n; nL emissive primitives):
 *     sel = 1
 *     if nL > 0:  c0 = rand01(rng); sel = 0.5f; if not c0 < 0.5f: the light connection of the mode and of
 *       HIPPT_OPT_LIGHT_SELECT as above, with (nl * 2.0f) where nl (float(nLights) or ip_k) stands; done
 *     rng = hash32(rng);  xr = (uint64(rng) * T) >> 32;    y = the smallest row with C_y > xr
 *     rng = hash32(rng);  xc = (uint64(rng) * R_y) >> 32;  x = the smallest column with c(x,y) > xc
 *     a = rand01(rng);  b = rand01(rng);  g2 = 2.0f / float(S)
 *     u = fmaf(float(x) + a, g2, -1.0f);  w = fmaf(float(y) + b, g2, -1.0f)
 *     dy = (1 - |u|) - |w|;  (dx, dz) as above from (u, w);  n2 = fdot(d, d);  om = d * (1.0f / sqrtf(n2))
 *     cosS = fdot(n, om);  pl = (k(x,y) * (n2 * sqrtf(n2))) * sel
 *     no shadow ray unless cosS > 0 and pl > 0     (the draws are consumed either way)
 *     g = cosS / (3.14159274f * pl)
 *     mode 1: Ld = (thr' * env(om)) * g
 *     mode 2: no shadow ray unless g < +inf;  Ld = (thr' * env(om)) * (g / fmaf(g, g, 1.0f))
 *     the shadow ray (p, om), tmin 0.001, no tmax: Lacc += Ld iff it has no hit at all; it counts as a segment
 *     and as a shadow ray.
 *   The coin is drawn whenever the scene holds a light; the * 2.0f also enters the MIS weight of a light hit.
 *   a segment of direction d, as the path holds it, that misses:
 *     no Lambertian scatter before it (mode 1: spec; mode 2: cb < 0):  L = Lacc + thr * env(d)
 *     mode 1, after a Lambertian scatter:  L = Lacc                     (the connection counted it)
 *     mode 2, after a Lambertian scatter:  L = Lacc + (thr * env(d)) * wb, wb = 1 unless
 *       s1 = (|dx| + |dy|) + |dz|;  r = sqrtf(fdot(d, d)) / s1;  r3 = (r * r) * r
 *       (u, w) = env(d)'s own octahedral coordinates (fold included);  h = 0.5f * float(S)
 *       x = int(fminf(fmaxf(fmaf(u, h, h), 0.0f), float(S - 1)));  y the same from w
 *       pl = (k(x,y) * r3) * sel;  cb > 0 and pl > 0: gh = cb / (3.14159274f * pl); s = gh * gh;
 *       s < +inf: wb = s / fmaf(gh, gh, 1.0f)
 * Depth, absorption, a, emissive hits and the segment counts are the rules' above. */
/* Records of the chained runs closed since the last call (HIPPT_OPT_CHAIN_AUDIT), as 32-bit words:
 * per run a 16-word header  [0] 0xC4A1D17 [1] run id [2] device [3] batch 0's first frame [4] frames
 * from one batch to the next (-1: one batch) [5] frames per batch [6] band pixels [7] items per batch
 * [8] batches [9] launches [10] slots [11] batches beyond the records (their records pooled in the
 * last one) [12..15] 0, then min(batches, 256) + 1 records of 16 words: [0] items traced [1] pixels
 * combined [2..3] sum of hash(item) [4..5] sum of hash(pixel) over the combine (64-bit, mod 2^64;
 * hash(i) = the RNG hash of i ^ 0x5bd1e995) [6] 1 + largest first frame an item was traced with
 * [7] ~smallest [8] 1 + latest launch that traced items [9] ~earliest [10] 1 + latest launch that
 * combined pixels (the run's last flush is launch `launches`) [11] ~earliest [12] 1 + largest first
 * frame the combine used [13] ~smallest [14..15] 0.  Writes at most maxWords words (whole runs) and
 * returns the number written; runs that did not fit are kept for the next call.  Synchronises. */
int hipptChainAudit(unsigned int *words, int maxWords);
/* Output frame word formats (HIPPT_OPT_PIXEL_FORMAT).  Both map an accumulated colour c to
 * sqrt(clamp(c, 0, 1)) per channel.
 *   ARGB:  0xAARRGGBB, channel = uint(x * 255) truncated (CudaPathTracerKernel.cu:171-178).
 *   RGBA8: bytes R, G, B, A in memory (0xAABBGGRR), channel = x * 255 rounded to nearest, ties to
 *          even: the RGBA8 UNORM texel the GL (GpuPathTracer.cpp:284-285, GL_RGBA8 image) and
 *          Vulkan (pathtrace_vulkan.comp:113-114, VK_FORMAT_R8G8B8A8_UNORM, copied to
 *          VulkanPathTracer::hostPixels) backends store. */
enum { HIPPT_PIXEL_ARGB = 0, HIPPT_PIXEL_RGBA8 = 1 };
/* Read-only (hipptGetOption) facts of the last megakernel render: LDS bytes of the top of the tree,
 * persistent-grid blocks per CU, work items per claim (HIPPT_OPT_CHUNK as applied), batches a launch
 * may trace (HIPPT_OPT_CHAIN as applied: 0 = the batch was not chained), the node-box pad exponent of
 * the LDS scene copy (HIPPT_OPT_RENDER_PAD as applied: 0 = the builder's pad, no trim), the image
 * pixels outside the sky rectangle (HIPPT_OPT_SKY_RECT as applied: 0 = no rectangle, every sample
 * traced). */
enum { HIPPT_INFO_LDS_TOP_BYTES = 100, HIPPT_INFO_BLOCKS_PER_CU = 101, HIPPT_INFO_CHUNK = 102,
       HIPPT_INFO_CHAIN_CAP = 103,
       HIPPT_INFO_UPDATE_DROPPED = 104 /* triangles the last device-memory hipptUpdateVertices dropped
                                          for a non-finite coordinate; reading it synchronises */,
       HIPPT_INFO_RENDER_PAD = 105,
       HIPPT_INFO_SKY_RECT_PIXELS = 106,
       HIPPT_INFO_SKY_COMBINE = 112 /* HIPPT_OPT_SKY_COMBINE as applied: band pixels of the last batch, over all
                                       devices, whose samples the combine finished (0: none) */,
       /* device time in nanoseconds of stage k of the last hipptDenoise made under
          HIPPT_OPT_DENOISE_TIMING, key HIPPT_INFO_DENOISE_NS + k: 0 the guide query, 1 prepare,
          2..9 passes 0..7, 10 finish (0: the stage did not run) */
       HIPPT_INFO_DENOISE_NS = 200 };
bool hipptSetOption(int key, long long value);
long long hipptGetOption(int key);
/* BVH width (2 or 4) the last mesh render traversed (0 before any): what nodeVisits count. */
int hipptActiveBvhWidth(void);

const char *hipptLastError(void);

/* ---- host BVH builder (exposed for C++ hosts and tests) ------------------------------- */
/* Node = 16 x 32-bit words: child-0 box (lo xyz, hi xyz), child-1 box, child0, child1,
 * 2 reserved.  child >= 0: interior node index; child < 0: leaf, ~child = first<<4 | count. */
typedef struct hipptBvh hipptBvh;
hipptBvh *hipptBvhBuild(const float *verts, int numTris, float extentHint, const char **errorMessage);
int hipptBvhNodeCount(const hipptBvh *bvh);
int hipptBvhDepth(const hipptBvh *bvh);
/* nodes: NodeCount*16 words; triOrder: numTris ints (leaf order -> original triangle index). */
void hipptBvhCopy(const hipptBvh *bvh, uint32_t *nodes, int *triOrder);
void hipptBvhFree(hipptBvh *bvh);
/* New boxes for the same topology (what hipptUpdateVertices does to the uploaded scene): every used
 * slot's box of the 2-wide, 4-wide and 8-bit trees becomes the union of the triangle boxes below it,
 * each side moved out once by the pad of the new vertices and extentHint, as a build pads; codes and
 * triangle order stay.  numTris must be the build's; a non-finite coordinate is an error and leaves
 * the trees unchanged. */
bool hipptBvhRefit(hipptBvh *bvh, const float *verts, int numTris, float extentHint, const char **errorMessage);
/* The 4-wide tree the megakernel traverses (HIPPT_OPT_BVH_WIDTH 4), collapsed from the 2-wide
 * one (same leaves and triangle order).  Node = 32 words: lo.x[4] hi.x[4] lo.y[4] hi.y[4]
 * lo.z[4] hi.z[4] (floats), child[4] (codes as above; an unused slot holds an empty leaf under
 * a box far outside the scene), 4 reserved.  Depth = nodes on the deepest path; StackBound =
 * the most traversal-stack entries any ray can need. */
int hipptBvh4NodeCount(const hipptBvh *bvh);
int hipptBvh4Depth(const hipptBvh *bvh);
int hipptBvh4StackBound(const hipptBvh *bvh);
void hipptBvh4Copy(const hipptBvh *bvh, uint32_t *nodes);
/* The same 4-wide tree with 8-bit child boxes (HIPPT_OPT_BVH_QUANT), Bvh4NodeCount nodes of 16
 * words: origin xyz (float), scale x; lo.x hi.x lo.y hi.y lo.z hi.z (4 bytes each, byte i =
 * child i, plane = origin + byte * scale); scale y; scale z; child[4].  Every decoded box
 * contains the float box of hipptBvh4Copy; an unused slot has lo bytes 255 and hi bytes 0. */
void hipptBvh4QCopy(const hipptBvh *bvh, uint32_t *nodes);
/* Nodes of that 8-bit tree: Bvh4NodeCount, or 0 when the scene has none (boxes near +-FLT_MAX,
 * which no finite grid covers; the kernels then read the float nodes). */
int hipptBvh4QNodeCount(const hipptBvh *bvh);

#ifdef __cplusplus
}
#endif
#endif
