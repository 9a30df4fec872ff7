// hippt_render.cpp — Qt-free C++ caller of libhippt.so through HipPathTracer: the render loop of
// RayTracerFboItem (updatePaintNode → m_cudaTracer->renderFrame(maxDepth) once per frame,
// RayTracerFboItem.cpp:516-575) without the scene graph.
//
//   hippt_render [--backend cuda|vulkan|gl] [--mesh FILE.obj|.ply] [--albedo r,g,b[;r,g,b...]]
//                [--emit NAME=r,g,b[;NAME=r,g,b...]] [--width W] [--height H] [--spp N] [--depth D] [--per-frame] [--present]
//                [--out FILE] [--ppm FILE.ppm] [--pick X,Y] [--denoise PASSES]
//                [--radiance-in FILE|camera --radiance-out FILE] [--light-sampling] [--mis]
//                [--light-select power|uniform] [--background r,g,b | --env FILE.pfm [--env-size N]] [--env-sampling]
//
// --backend cuda (default): HipPathTracer, the CudaPathTracer interface.  Without --mesh: the
// reference kernel's built-in 4-sphere scene, one renderFrame per frame (the CUDA backend's
// loop).  With --mesh: the file's triangles (hipptReadMesh) under the Cornell camera, all N
// frames in one renderFrames call, or one call per frame with --per-frame, or through the
// non-blocking hand-off with --present.
// --emit (with --mesh): the named OBJ `usemtl` groups are area lights of that radiance (HIPPT_MAT_EMISSIVE).
// --light-sampling: HIPPT_OPT_LIGHT_SAMPLING 1 (next-event estimation towards those lights) for the render
// and --radiance-out.  --mis: HIPPT_OPT_LIGHT_SAMPLING_MODE HIPPT_LIGHT_SAMPLING_MIS (light sampling with the scatter sample weighed in by
// the power heuristic); it implies --light-sampling.
// --light-select power: HIPPT_OPT_LIGHT_SELECT HIPPT_LIGHT_SELECT_POWER (a connection picks its light in proportion
// to area x emission); uniform (default): over the list.  Meaningful with --light-sampling or --mis; it implies neither.
// --background r,g,b (with --mesh): a constant environment of that radiance (hipptSetEnvironment, size 1) in place
// of the sky gradient.  --env FILE.pfm (with --mesh): a lat-long colour PFM (little-endian, rows bottom to top)
// resampled by hipptEnvFromEquirect to an octahedral map of --env-size texels a side (default 256).
// --env-sampling: HIPPT_OPT_ENV_SAMPLING 1 (every Lambertian vertex connects to the environment map by its selection
// table).  It needs --env or --background together with --light-sampling or --mis, and implies none of them.
// --backend vulkan: HipVulkanPathTracer, one renderFrame(depth) per frame (the app's "vulkan"
// branch, RayTracerFboItem.cpp:576-600).  --backend gl: HipGpuPathTracer, initialize + resize,
// then renderFrame(N, depth) once (or per frame with --per-frame), as the GL branch calls it.
// --out writes the frame words (cuda: ARGB; vulkan / gl: RGBA8; row 0 = bottom, little endian),
// --ppm an image (top row first).  --pick X,Y (cuda backend, with --mesh): after the render,
// HipPathTracer::pick at that pixel (row 0 = bottom) and the pixel centre's pinhole ray through
// HipPathTracer::traceRays and HipPathTracer::traceHits, reported as "pick": {x, y, prim, t_bits,
// ray_prim, ray_t_bits, ray_hit_words (the hipptHit's 8 words)}.  --denoise PASSES (cuda backend, with
// --mesh): --out and --ppm get HipPathTracer::denoise's image (that many passes, the other parameters
// at their defaults) in place of the rendered one.
// --radiance-in FILE --radiance-out FILE (cuda backend, with --mesh): after the render,
// HipPathTracer::traceRadiance at --depth over the file's rays (records of 9 words: the ray's 8 floats and
// its RNG state; "camera": HipPathTracer::cameraRays of frame 0) written as records of 5 words (the
// radiance's 4 floats and the segment count), reported as "radiance_rays".
// Prints one JSON line.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "HipComputeTracers.h"
#include "HipPathTracer.h"
#include "env_io.h"

namespace {

int usage() {
    std::fprintf(stderr,
                 "usage: hippt_render [--backend cuda|vulkan|gl] [--mesh FILE] [--albedo r,g,b[;...]] [--width W]\n"
                 "                    [--emit NAME=r,g,b[;...]]\n"
                 "                    [--height H] [--spp N] [--depth D] [--per-frame] [--present] [--out FILE]\n"
                 "                    [--ppm FILE.ppm] [--pick X,Y] [--update-mesh FILE] [--denoise PASSES]\n"
                 "                    [--radiance-in FILE|camera --radiance-out FILE] [--light-sampling] [--mis]\n"
                 "                    [--light-select power|uniform] [--background r,g,b | --env FILE.pfm [--env-size N]]\n"
                 "                    [--env-sampling]\n");
    return 2;
}

std::vector<float> parse_floats(const std::string &s) {
    std::vector<float> v;
    std::string tok;
    for (char ch : s + ",") {
        if (ch == ',' || ch == ';') {
            if (!tok.empty()) v.push_back(std::strtof(tok.c_str(), nullptr));
            tok.clear();
        } else {
            tok += ch;
        }
    }
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    std::string mesh, out, ppm, albedoArg, emitArg, pickArg, updateMesh, radianceIn, radianceOut, backend = "cuda";
    std::string lightSelect = "uniform", background, envFile;
    int envSize = 256;
    int width = 320, height = 180, spp = 16, depth = 8, denoise = -1;
    bool perFrame = false, present = false, lightSampling = false, mis = false, envSampling = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        const char *v = nullptr;
        if (a == "--per-frame") perFrame = true;
        else if (a == "--present") present = true;
        else if (a == "--light-sampling") lightSampling = true;
        else if (a == "--mis") mis = true;
        else if (a == "--env-sampling") envSampling = true;
        else if ((v = next()) == nullptr) return usage();
        else if (a == "--backend") backend = v;
        else if (a == "--mesh") mesh = v;
        else if (a == "--albedo") albedoArg = v;
        else if (a == "--emit") emitArg = v;
        else if (a == "--width") width = std::atoi(v);
        else if (a == "--height") height = std::atoi(v);
        else if (a == "--spp") spp = std::atoi(v);
        else if (a == "--depth") depth = std::atoi(v);
        else if (a == "--out") out = v;
        else if (a == "--ppm") ppm = v;
        else if (a == "--pick") pickArg = v;
        else if (a == "--update-mesh") updateMesh = v;
        else if (a == "--denoise") denoise = std::atoi(v);
        else if (a == "--radiance-in") radianceIn = v;
        else if (a == "--radiance-out") radianceOut = v;
        else if (a == "--light-select") lightSelect = v;
        else if (a == "--background") background = v;
        else if (a == "--env") envFile = v;
        else if (a == "--env-size") envSize = std::atoi(v);
        else return usage();
    }
    if (backend != "cuda" && backend != "vulkan" && backend != "gl") return usage();
    if (lightSelect != "power" && lightSelect != "uniform") return usage();
    if (!background.empty() && !envFile.empty()) return usage();
    if (envSampling && ((background.empty() && envFile.empty()) || !(lightSampling || mis))) {
        std::fprintf(stderr, "hippt_render: --env-sampling needs --env or --background together with --light-sampling or --mis\n");
        return 1;
    }
    HipPathTracer tracer;
    if (!background.empty()) {
        const std::vector<float> c = parse_floats(background);
        if (c.size() != 3 || !tracer.setEnvironment(c, 1)) {
            std::fprintf(stderr, "hippt_render: --background: %s\n", c.size() != 3 ? "needs r,g,b" : tracer.lastError().c_str());
            return 1;
        }
    }
    if (!envFile.empty()) {
        std::vector<float> img;
        int w = 0, h = 0;
        std::string msg;
        if (!hippt::envio::read_pfm(envFile, img, w, h, &msg)) {
            std::fprintf(stderr, "hippt_render: --env: %s\n", msg.c_str());
            return 1;
        }
        const char *err = nullptr;
        std::vector<float> texels(envSize > 0 && envSize <= 4096 ? size_t(envSize) * size_t(envSize) * 3 : 0);
        if (!hipptEnvFromEquirect(img.data(), w, h, envSize, texels.data(), &err) || !tracer.setEnvironment(texels, envSize)) {
            std::fprintf(stderr, "hippt_render: --env: %s\n", err ? err : tracer.lastError().c_str());
            return 1;
        }
    }
    hipptSetOption(HIPPT_OPT_LIGHT_SELECT, lightSelect == "power" ? HIPPT_LIGHT_SELECT_POWER : 0);
    hipptSetOption(HIPPT_OPT_ENV_SAMPLING, envSampling ? 1 : 0);
    hipptSetOption(HIPPT_OPT_LIGHT_SAMPLING_MODE, mis ? HIPPT_LIGHT_SAMPLING_MIS : lightSampling ? 1 : 0);
    if (!mesh.empty()) {
        // the scene is the library's (shared by every interface)
        const double from[3] = {278, 278, -800}, at[3] = {278, 278, 0}, up[3] = {0, 1, 0};
        if (!tracer.loadMeshFile(mesh, parse_floats(albedoArg), from, at, up, 40.0, 0.0, 10.0, emitArg)) {
            std::fprintf(stderr, "hippt_render: %s\n", tracer.lastError().c_str());
            return 1;
        }
    }
    const bool rgba = backend != "cuda";
    const size_t n = size_t(std::max(0, width)) * size_t(std::max(0, height));
    std::vector<unsigned int> frame;
    int frames = 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::string error;
    bool ok = true;
    hipptStats st{};  // read before the tracer object (and with it the library state) goes
    if (backend == "vulkan") {
        HipVulkanPathTracer vk;
        ok = vk.initialize(width, height);
        for (int f = 0; f < spp && ok; ++f) ok = vk.renderFrame(depth);
        if (ok) frame.assign(vk.hostPixels(), vk.hostPixels() + n);
        hipptGetStats(&st);
        frames = vk.frameIndex();
        error = vk.lastError();
    } else if (backend == "gl") {
        HipGpuPathTracer gl;
        ok = gl.initialize() && gl.resize(width, height);
        if (perFrame)
            for (int f = 0; f < spp && ok; ++f) ok = gl.renderFrame(1, depth);
        else
            ok = ok && gl.renderFrame(spp, depth);
        if (ok) frame.assign(gl.hostPixels(), gl.hostPixels() + n);
        hipptGetStats(&st);
        frames = gl.frameIndex();
        error = gl.lastError();
    }
    if (rgba) {
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!ok) {
            std::fprintf(stderr, "hippt_render: %s\n", error.empty() ? "render failed" : error.c_str());
            return 1;
        }
        if (!out.empty()) {
            FILE *f = std::fopen(out.c_str(), "wb");
            if (!f || std::fwrite(frame.data(), sizeof(unsigned int), n, f) != n) return 1;
            std::fclose(f);
        }
        if (!ppm.empty()) {
            FILE *f = std::fopen(ppm.c_str(), "wb");
            if (!f) return 1;
            std::fprintf(f, "P6\n%d %d\n255\n", width, height);
            for (int y = height - 1; y >= 0; --y)
                for (int x = 0; x < width; ++x) {
                    const unsigned p = frame[size_t(y) * width + x];  // bytes R, G, B, A
                    const unsigned char rgb[3] = {(unsigned char)p, (unsigned char)(p >> 8), (unsigned char)(p >> 16)};
                    std::fwrite(rgb, 1, 3, f);
                }
            std::fclose(f);
        }
        // the process-wide word format is back to its default after the RGBA8 interfaces' renders
        std::printf("{\"backend\": \"%s\", \"frames\": %d, \"seconds\": %.6f, \"segments\": %llu, "
                    "\"pixel_samples\": %llu, \"pixel_format_after\": %lld}\n",
                    backend.c_str(), frames, secs, (unsigned long long)st.segments,
                    (unsigned long long)st.pixelSamples, hipptGetOption(HIPPT_OPT_PIXEL_FORMAT));
        return 0;
    }
    if (!tracer.initialize(width, height)) {
        std::fprintf(stderr, "hippt_render: %s\n", tracer.lastError().c_str());
        return 1;
    }
    const unsigned int *pixels = nullptr;
    if (mesh.empty() || perFrame) {
        for (int f = 0; f < spp && ok; ++f) ok = tracer.renderFrame(depth);  // the app's per-paint call
        pixels = tracer.hostPixels();
    } else if (present) {
        int shown = 0, frames = 0;
        for (int f = 0; f < spp && ok; f += 4) {
            ok = tracer.presentFrames(std::min(4, spp - f), depth);
            if (ok && tracer.latestFrame(&frames)) ++shown;  // a UI would draw this image now
        }
        const char *err = nullptr;
        ok = ok && hipptSynchronize(&err);
        pixels = ok ? tracer.latestFrame(&frames) : nullptr;
        ok = ok && pixels && frames == spp;
        if (ok) std::fprintf(stderr, "hippt_render: %d intermediate images were ready without waiting\n", shown);
    } else if (!updateMesh.empty()) {
        // an animated mesh: sample 0 over --mesh, then the same triangles at --update-mesh's vertices
        // (HipPathTracer::updateVertices) for the remaining samples
        hipptMesh m{};
        const char *err = nullptr;
        ok = tracer.renderFrames(1, depth);
        if (ok && !hipptReadMesh(updateMesh.c_str(), &m, &err)) {
            std::fprintf(stderr, "hippt_render: %s\n", err ? err : "cannot read the update mesh");
            return 1;
        }
        if (ok) {
            ok = tracer.updateVertices(std::vector<float>(m.verts, m.verts + size_t(m.numTris) * 9));
            hipptFreeMesh(&m);
        }
        ok = ok && tracer.renderFrames(spp - 1, depth);
        pixels = tracer.hostPixels();
    } else {
        ok = tracer.renderFrames(spp, depth);
        pixels = tracer.hostPixels();
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!ok || !pixels) {
        std::fprintf(stderr, "hippt_render: %s\n", tracer.lastError().c_str());
        return 1;
    }
    std::vector<unsigned> clean;
    if (denoise >= 0) {
        hipptDenoiseParams dp;
        hipptDenoiseDefaults(&dp);
        dp.passes = denoise;
        if (!tracer.denoise(&dp, clean)) {
            std::fprintf(stderr, "hippt_render: denoise: %s\n", tracer.lastError().c_str());
            return 1;
        }
        pixels = clean.data();
    }
    if (!out.empty()) {
        FILE *f = std::fopen(out.c_str(), "wb");
        if (!f || std::fwrite(pixels, sizeof(unsigned int), n, f) != n) return 1;
        std::fclose(f);
    }
    if (!ppm.empty()) {
        FILE *f = std::fopen(ppm.c_str(), "wb");
        if (!f) return 1;
        std::fprintf(f, "P6\n%d %d\n255\n", width, height);
        for (int y = height - 1; y >= 0; --y)
            for (int x = 0; x < width; ++x) {
                const unsigned p = pixels[size_t(y) * width + x];
                const unsigned char rgb[3] = {(unsigned char)(p >> 16), (unsigned char)(p >> 8), (unsigned char)p};
                std::fwrite(rgb, 1, 3, f);
            }
        std::fclose(f);
    }
    std::string pickJson;
    if (!pickArg.empty()) {
        const std::vector<float> xy = parse_floats(pickArg);
        int prim = -1;
        float t = 0.0f;
        if (xy.size() != 2 || !tracer.pick(int(xy[0]), int(xy[1]), &prim, &t)) {
            std::fprintf(stderr, "hippt_render: pick: %s\n", tracer.lastError().c_str());
            return 1;
        }
        // the pinhole ray through the pixel's centre, as a host would build one
        hipptCamera cam;
        const double from[3] = {278, 278, -800}, at[3] = {278, 278, 0}, up[3] = {0, 1, 0};
        hipptBuildCamera(from, at, up, 40.0, double(width) / double(height), 0.0, 10.0, &cam);
        const float s = (xy[0] + 0.5f) / float(std::max(1, width - 1)), v = (xy[1] + 0.5f) / float(std::max(1, height - 1));
        std::vector<float> ray(8), ts;
        std::vector<int> prims;
        for (int k = 0; k < 3; ++k) {
            ray[size_t(k)] = cam.origin[k];
            ray[size_t(4 + k)] = cam.llc[k] + s * cam.horizontal[k] + v * cam.vertical[k] - cam.origin[k];
        }
        ray[3] = 0.001f;
        ray[7] = std::numeric_limits<float>::infinity();
        if (!tracer.traceRays(ray, ts, prims)) {
            std::fprintf(stderr, "hippt_render: traceRays: %s\n", tracer.lastError().c_str());
            return 1;
        }
        std::vector<hipptHit> hits;
        if (!tracer.traceHits(ray, hits)) {
            std::fprintf(stderr, "hippt_render: traceHits: %s\n", tracer.lastError().c_str());
            return 1;
        }
        unsigned tb, rb, hw[8];
        std::memcpy(&tb, &t, 4);
        std::memcpy(&rb, &ts[0], 4);
        static_assert(sizeof(hipptHit) == sizeof hw, "hipptHit is 8 words");
        std::memcpy(hw, &hits[0], sizeof hw);
        char buf[400];
        std::snprintf(buf, sizeof buf, ", \"pick\": {\"x\": %d, \"y\": %d, \"prim\": %d, \"t_bits\": %u, \"ray_prim\": %d, "
                      "\"ray_t_bits\": %u, \"ray_hit_words\": [%u, %u, %u, %u, %u, %u, %u, %u]}", int(xy[0]), int(xy[1]), prim,
                      tb, prims[0], rb, hw[0], hw[1], hw[2], hw[3], hw[4], hw[5], hw[6], hw[7]);
        pickJson = buf;
    }
    if (!radianceIn.empty()) {
        std::vector<float> rays, radiance;
        std::vector<unsigned> seeds;
        std::vector<int> segments;
        if (radianceIn == "camera") {
            if (!tracer.cameraRays(0, rays, seeds)) {
                std::fprintf(stderr, "hippt_render: cameraRays: %s\n", tracer.lastError().c_str());
                return 1;
            }
        } else {
            FILE *f = std::fopen(radianceIn.c_str(), "rb");
            unsigned rec[9];
            while (f && std::fread(rec, sizeof rec, 1, f) == 1) {
                float r8[8];
                std::memcpy(r8, rec, sizeof r8);
                rays.insert(rays.end(), r8, r8 + 8);
                seeds.push_back(rec[8]);
            }
            if (!f) return 1;
            std::fclose(f);
        }
        if (!tracer.traceRadiance(rays, seeds, depth, radiance, segments)) {
            std::fprintf(stderr, "hippt_render: traceRadiance: %s\n", tracer.lastError().c_str());
            return 1;
        }
        FILE *f = radianceOut.empty() ? nullptr : std::fopen(radianceOut.c_str(), "wb");
        if (!f) return 1;
        for (size_t i = 0; i < segments.size(); ++i) {
            unsigned rec[5];
            std::memcpy(rec, &radiance[4 * i], 16);
            std::memcpy(rec + 4, &segments[i], 4);
            if (std::fwrite(rec, sizeof rec, 1, f) != 1) return 1;
        }
        std::fclose(f);
        pickJson += ", \"radiance_rays\": " + std::to_string(segments.size());
    }
    hipptGetStats(&st);
    std::printf("{\"backend\": \"cuda\", \"frames\": %d, \"seconds\": %.6f, \"segments\": %llu, "
                "\"pixel_samples\": %llu%s}\n",
                tracer.frameIndex(), secs, (unsigned long long)st.segments, (unsigned long long)st.pixelSamples,
                pickJson.c_str());
    return 0;
}
