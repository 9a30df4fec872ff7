// HipPathTracer.h — C++ host object over libhippt.so's C ABI (include/hippt.h).
//
// Same public interface and frame-index bookkeeping as the reference's CudaPathTracer
// (src/backends/CudaPathTracer.h:6-23, CudaPathTracer.cpp:14-57): initialize(w, h) re-inits and
// restarts the frame count, renderFrame(maxDepth) renders one sample per pixel for the current
// frame index and advances it, hostPixels() is the library-owned ARGB frame (row 0 = bottom),
// lastError() the last message.  Qt-free (std::string instead of QString) so it builds and runs
// without Qt; RayTracerFboItem's "hip" backend string constructs it exactly like
// m_cudaTracer.  Extensions: scenes, batched frames, non-blocking hand-off.
#pragma once

#include <string>
#include <vector>

#include "hippt.h"

class HipPathTracer {
public:
    HipPathTracer() = default;
    ~HipPathTracer();
    HipPathTracer(const HipPathTracer &) = delete;
    HipPathTracer &operator=(const HipPathTracer &) = delete;

    // --- CudaPathTracer interface -------------------------------------------------------------
    bool initialize(int width, int height);
    bool renderFrame(int maxDepth);
    const unsigned int *hostPixels() const { return m_hostPixels; }
    int frameIndex() const { return m_frameIndex; }
    std::string lastError() const { return m_lastError; }

    // --- extensions ----------------------------------------------------------------------------
    // Triangle mesh from an OBJ/PLY file, one Lambertian material per group (albedo: 3 floats per
    // group; empty = white 0.73), camera as RayTracer.h Camera parameters.  emit: "NAME=r,g,b[;NAME=r,g,b...]"
    // makes those OBJ `usemtl` groups area lights (HIPPT_MAT_EMISSIVE with that radiance; the scene is then
    // uploaded through hipptUploadScene).
    bool loadMeshFile(const std::string &path, const std::vector<float> &albedo, const double lookfrom[3],
                      const double lookat[3], const double vup[3], double vfovDeg, double aperture, double focus,
                      const std::string &emit = std::string());
    bool uploadScene(const std::vector<float> &verts, const std::vector<int> &triMaterial,
                     const std::vector<float> &spheres, const std::vector<int> &sphereMaterial,
                     const std::vector<hipptMaterial> &materials, const double lookfrom[3], const double lookat[3],
                     const double vup[3], double vfovDeg, double aperture, double focus);
    bool useBuiltinScene();  // the reference kernel's 4 spheres (the default)
    // New vertices (9 floats per triangle, the upload's triangle order and count) for the uploaded
    // scene, in place and in stream order: the frames rendered next show them; nothing queued is
    // drained.  The BVH is refitted, not rebuilt (hipptUpdateVertices): uploadScene is the rebuild.
    bool updateVertices(const std::vector<float> &verts);
    // hipptSetEnvironment: an octahedral environment map of size x size rgb texels (size*size*3 floats) in place
    // of the sky gradient for every uploaded scene, in stream order; an empty vector with size 0 removes it.
    bool setEnvironment(const std::vector<float> &texels, int size);
    // samplesPerFrame frames in one call (GpuPathTracer::renderFrame(spp, depth) shape).
    bool renderFrames(int samplesPerFrame, int maxDepth);
    // Enqueue frames + copy to a hand-off frame; latestFrame() never blocks.
    bool presentFrames(int samplesPerFrame, int maxDepth);
    const unsigned int *latestFrame(int *frames);
    bool setOption(int key, long long value);
    // Ray queries over the uploaded scene (include/hippt.h "ray queries"): rays = 8 floats each (origin
    // xyz, tmin, direction xyz, tmax); t and prim get one entry per ray (+inf, -1 on a miss).
    bool traceRays(const std::vector<float> &rays, std::vector<float> &t, std::vector<int> &prim);
    // The same query with a hit record per ray (hipptHit: t, prim, the shading normal faced against the
    // ray, the barycentrics, material index | HIPPT_HIT_SPHERE | HIPPT_HIT_BACKFACE).
    bool traceHits(const std::vector<float> &rays, std::vector<hipptHit> &hits);
    // Path queries (include/hippt.h "path queries"): the renderer's path from each ray (8 floats, as
    // traceRays; tmin and tmax hold for the first segment) with RNG state seeds[i]: radiance gets 4 floats
    // per ray (rgb and 1 where the first segment hit), segments the closest-hit queries each path made.
    bool traceRadiance(const std::vector<float> &rays, const std::vector<unsigned> &seeds, int maxDepth,
                       std::vector<float> &radiance, std::vector<int> &segments);
    // The rays renderFrames starts sample `frame` of every pixel with (8 floats each, row 0 = v = 0) and
    // the RNG state each is left with: traceRadiance of them is that sample of the renderer.
    bool cameraRays(int frame, std::vector<float> &rays, std::vector<unsigned> &seeds);
    // The primitive under pixel (x, y) and its distance, for sample `frame`'s camera ray; y counts rows
    // as hostPixels() does (row 0 = v = 0, the bottom row: a viewport click at yTop is height - 1 - yTop).
    // *prim = -1 and *t = +inf over the sky.
    bool pick(int x, int y, int *prim, float *t = nullptr, int frame = 0);
    // The accumulated image denoised on the device (hipptDenoise: an edge-avoiding A-trous wavelet guided
    // by the first hits' normals, depths and albedos): width * height frame words as hostPixels() has
    // them.  params null: the defaults (hipptDenoiseDefaults).  Needs an uploaded scene; the
    // accumulation and hostPixels() stay as they are.
    bool denoise(const hipptDenoiseParams *params, std::vector<unsigned> &pixels);

private:
    bool fail(const char *err, const char *fallback);

    int m_width = 0;
    int m_height = 0;
    int m_frameIndex = 0;
    const unsigned int *m_hostPixels = nullptr;
    std::string m_lastError;
};
