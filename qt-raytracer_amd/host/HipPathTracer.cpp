// HipPathTracer.cpp — see HipPathTracer.h.
#include "HipPathTracer.h"

#include <algorithm>
#include <cstdio>

HipPathTracer::~HipPathTracer() { cudaPathTracerShutdown(); }

bool HipPathTracer::fail(const char *err, const char *fallback) {
    m_lastError = err ? err : fallback;
    return false;
}

bool HipPathTracer::initialize(int width, int height) {
    m_width = width;
    m_height = height;
    m_frameIndex = 0;
    m_hostPixels = nullptr;
    const char *err = nullptr;
    if (!cudaPathTracerInit(width, height, &err)) return fail(err, "HIP initialization failed");
    return true;
}

bool HipPathTracer::renderFrame(int maxDepth) {
    const char *err = nullptr;
    const unsigned int *pixels = nullptr;
    if (!cudaPathTracerRender(m_frameIndex, maxDepth, &pixels, &err)) return fail(err, "HIP render failed");
    m_hostPixels = pixels;
    ++m_frameIndex;
    return true;
}

bool HipPathTracer::loadMeshFile(const std::string &path, const std::vector<float> &albedo,
                                 const double lookfrom[3], const double lookat[3], const double vup[3],
                                 double vfovDeg, double aperture, double focus, const std::string &emit) {
    hipptMesh mesh;
    const char *err = nullptr;
    if (!hipptReadMesh(path.c_str(), &mesh, &err)) return fail(err, "mesh read failed");
    std::vector<float> alb(albedo);
    if (alb.empty())
        for (int g = 0; g < mesh.numGroups; ++g) alb.insert(alb.end(), {0.73f, 0.73f, 0.73f});
    bool ok = int(alb.size()) == 3 * mesh.numGroups;
    if (!ok) {
        m_lastError = "albedo needs 3 floats per mesh group";
    } else if (!emit.empty()) {
        // NAME=r,g,b[;NAME=r,g,b...]: those groups emit; the scene goes through hipptUploadScene
        std::vector<hipptMaterial> mats;
        for (int g = 0; g < mesh.numGroups; ++g)
            mats.push_back(hipptMaterial{HIPPT_MAT_LAMBERTIAN, {alb[3 * g], alb[3 * g + 1], alb[3 * g + 2]}, 0.0f, 1.0f});
        for (size_t at = 0; ok && at < emit.size();) {
            const size_t end = std::min(emit.find(';', at), emit.size());
            const std::string item = emit.substr(at, end - at);
            at = end + 1;
            const size_t eq = item.rfind('=');
            float c[3];
            int g = 0;
            while (eq != std::string::npos && g < mesh.numGroups && item.compare(0, eq, mesh.groupNames[g]) != 0) ++g;
            ok = eq != std::string::npos && g < mesh.numGroups &&
                 std::sscanf(item.c_str() + eq + 1, "%f,%f,%f", &c[0], &c[1], &c[2]) == 3;
            if (ok) mats[size_t(g)] = hipptMaterial{HIPPT_MAT_EMISSIVE, {c[0], c[1], c[2]}, 0.0f, 1.0f};
            else m_lastError = "emit needs NAME=r,g,b of a usemtl group of the mesh: " + item;
        }
        if (ok) {
            ok = hipptUploadScene(mesh.verts, mesh.triGroup, mesh.numTris, nullptr, nullptr, 0, mats.data(), mesh.numGroups,
                                  lookfrom, lookat, vup, vfovDeg, aperture, focus, &err);
            if (!ok) fail(err, "scene upload failed");
        }
    } else {
        ok = hipptUploadMesh(mesh.verts, mesh.triGroup, mesh.numTris, alb.data(), mesh.numGroups, lookfrom, lookat, vup,
                             vfovDeg, aperture, focus, &err);
        if (!ok) fail(err, "mesh upload failed");
    }
    hipptFreeMesh(&mesh);
    return ok;
}

bool HipPathTracer::uploadScene(const std::vector<float> &verts, const std::vector<int> &triMaterial,
                                const std::vector<float> &spheres, const std::vector<int> &sphereMaterial,
                                const std::vector<hipptMaterial> &materials, const double lookfrom[3],
                                const double lookat[3], const double vup[3], double vfovDeg, double aperture,
                                double focus) {
    const char *err = nullptr;
    if (!hipptUploadScene(verts.data(), triMaterial.data(), int(triMaterial.size()), spheres.data(),
                          sphereMaterial.data(), int(sphereMaterial.size()), materials.data(), int(materials.size()),
                          lookfrom, lookat, vup, vfovDeg, aperture, focus, &err))
        return fail(err, "scene upload failed");
    return true;
}

bool HipPathTracer::useBuiltinScene() {
    const char *err = nullptr;
    if (!hipptUseBuiltinScene(HIPPT_SCENE_SPHERE4, &err)) return fail(err, "scene selection failed");
    return true;
}

bool HipPathTracer::updateVertices(const std::vector<float> &verts) {
    if (verts.size() % 9 != 0) {
        m_lastError = "vertices need 9 floats per triangle";
        return false;
    }
    const char *err = nullptr;
    if (!hipptUpdateVertices(verts.data(), int(verts.size() / 9), 0, &err)) return fail(err, "vertex update failed");
    return true;
}

bool HipPathTracer::setEnvironment(const std::vector<float> &texels, int size) {
    if (size < 0 || texels.size() != size_t(size) * size_t(size) * 3) {
        m_lastError = "an environment needs size*size*3 floats";
        return false;
    }
    const char *err = nullptr;
    if (!hipptSetEnvironment(size ? texels.data() : nullptr, size, 0, &err)) return fail(err, "setting the environment failed");
    return true;
}

bool HipPathTracer::renderFrames(int samplesPerFrame, int maxDepth) {
    const char *err = nullptr;
    const unsigned int *pixels = nullptr;
    if (!hipptRenderFrames(m_frameIndex, samplesPerFrame, maxDepth, &pixels, &err)) return fail(err, "HIP render failed");
    m_hostPixels = pixels;
    m_frameIndex += samplesPerFrame;
    return true;
}

bool HipPathTracer::presentFrames(int samplesPerFrame, int maxDepth) {
    const char *err = nullptr;
    if (!hipptRenderFramesPresent(m_frameIndex, samplesPerFrame, maxDepth, &err)) return fail(err, "HIP render failed");
    m_frameIndex += samplesPerFrame;
    return true;
}

const unsigned int *HipPathTracer::latestFrame(int *frames) {
    const char *err = nullptr;
    const unsigned int *pixels = nullptr;
    if (!hipptLatestFrame(&pixels, frames, &err)) {
        fail(err, "latest frame failed");
        return nullptr;
    }
    return pixels;
}

bool HipPathTracer::traceRays(const std::vector<float> &rays, std::vector<float> &t, std::vector<int> &prim) {
    if (rays.size() % 8 != 0) {
        m_lastError = "rays need 8 floats each";
        return false;
    }
    const long long n = (long long)(rays.size() / 8);
    t.resize(size_t(n));
    prim.resize(size_t(n));
    const char *err = nullptr;
    if (n > 0 && !hipptTraceRays(rays.data(), n, 0, t.data(), prim.data(), &err)) return fail(err, "ray query failed");
    return true;
}

bool HipPathTracer::traceHits(const std::vector<float> &rays, std::vector<hipptHit> &hits) {
    if (rays.size() % 8 != 0) {
        m_lastError = "rays need 8 floats each";
        return false;
    }
    const long long n = (long long)(rays.size() / 8);
    hits.resize(size_t(n));
    const char *err = nullptr;
    if (n > 0 && !hipptTraceHits(rays.data(), n, 0, hits.data(), &err)) return fail(err, "hit query failed");
    return true;
}

bool HipPathTracer::traceRadiance(const std::vector<float> &rays, const std::vector<unsigned> &seeds, int maxDepth,
                                  std::vector<float> &radiance, std::vector<int> &segments) {
    if (rays.size() % 8 != 0 || seeds.size() != rays.size() / 8) {
        m_lastError = "rays need 8 floats and one seed each";
        return false;
    }
    const long long n = (long long)(rays.size() / 8);
    radiance.resize(size_t(n) * 4);
    segments.resize(size_t(n));
    const char *err = nullptr;
    if (!hipptTraceRadiance(rays.data(), seeds.data(), n, maxDepth, 0, radiance.data(), segments.data(), &err))
        return fail(err, "path query failed");
    return true;
}

bool HipPathTracer::cameraRays(int frame, std::vector<float> &rays, std::vector<unsigned> &seeds) {
    const size_t n = size_t(std::max(0, m_width)) * size_t(std::max(0, m_height));
    rays.resize(n * 8);
    seeds.resize(n);
    const char *err = nullptr;
    if (!hipptCameraRays(frame, 0, rays.data(), seeds.data(), &err)) return fail(err, "camera rays failed");
    return true;
}

bool HipPathTracer::denoise(const hipptDenoiseParams *params, std::vector<unsigned> &pixels) {
    pixels.resize(size_t(m_width > 0 ? m_width : 0) * size_t(m_height > 0 ? m_height : 0));
    const char *err = nullptr;
    if (!hipptDenoise(params, pixels.data(), nullptr, &err)) return fail(err, "denoise failed");
    return true;
}

bool HipPathTracer::pick(int x, int y, int *prim, float *t, int frame) {
    if (x < 0 || y < 0 || x >= m_width || y >= m_height || !prim) {
        m_lastError = "pick outside the image";
        return false;
    }
    std::vector<float> ts(size_t(m_width) * size_t(m_height));
    std::vector<int> prims(ts.size());
    const char *err = nullptr;
    if (!hipptTraceCamera(frame, 0, ts.data(), prims.data(), &err)) return fail(err, "camera query failed");
    const size_t i = size_t(y) * size_t(m_width) + size_t(x);
    *prim = prims[i];
    if (t) *t = ts[i];
    return true;
}

bool HipPathTracer::setOption(int key, long long value) {
    if (!hipptSetOption(key, value)) {
        m_lastError = "invalid option";
        return false;
    }
    return true;
}
