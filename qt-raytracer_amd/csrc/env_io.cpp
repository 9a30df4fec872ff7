// env_io.cpp — see env_io.h.
#include "env_io.h"

#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

namespace hippt {
namespace envio {
namespace {

bool fail(std::string *err, const std::string &msg) {
    if (err) *err = msg;
    return false;
}

constexpr double kPi = 3.14159265358979323846;

}  // namespace

void texel_direction(int size, int x, int y, double d[3]) {
    const double u = (2.0 * x + 1.0) / size - 1.0, w = (2.0 * y + 1.0) / size - 1.0;
    const double dy = 1.0 - std::fabs(u) - std::fabs(w);
    double dx = u, dz = w;
    if (dy < 0.0) {
        dx = (1.0 - std::fabs(w)) * (u < 0.0 ? -1.0 : 1.0);
        dz = (1.0 - std::fabs(u)) * (w < 0.0 ? -1.0 : 1.0);
    }
    const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
    d[0] = dx / len;
    d[1] = dy / len;
    d[2] = dz / len;
}

void directions(int size, float *dirs) {
    if (size < 1 || size > kMaxEnvSize || !dirs) return;
    for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x) {
            double d[3];
            texel_direction(size, x, y, d);
            float *o = dirs + 3 * (size_t(y) * size_t(size) + size_t(x));
            o[0] = float(d[0]);
            o[1] = float(d[1]);
            o[2] = float(d[2]);
        }
}

bool from_equirect(const float *rgb, int width, int height, int size, float *texels, std::string *err) {
    if (!rgb || !texels) return fail(err, "environment resampling: null pointer");
    if (width < 1 || height < 1 || width > kMaxImageSide || height > kMaxImageSide)
        return fail(err, "environment resampling: image dimensions must be in 1.." + std::to_string(kMaxImageSide));
    if (size < 1 || size > kMaxEnvSize)
        return fail(err, "environment resampling: size must be in 1.." + std::to_string(kMaxEnvSize));
    const size_t W = size_t(width);
    for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x) {
            double d[3];
            texel_direction(size, x, y, d);
            const double theta = std::acos(std::fmin(1.0, std::fmax(-1.0, d[1])));
            const double phi = std::atan2(d[2], d[0]);
            const double rf = theta / kPi * height - 0.5, cf = (phi + kPi) / (2.0 * kPi) * width - 0.5;
            const double r0f = std::floor(rf), c0f = std::floor(cf);
            const double fr = rf - r0f, fc = cf - c0f;
            const long long r0 = (long long)r0f, c0 = (long long)c0f;
            const size_t ra = size_t(r0 < 0 ? 0 : r0 > height - 1 ? height - 1 : r0);
            const size_t rb = size_t(r0 + 1 < 0 ? 0 : r0 + 1 > height - 1 ? height - 1 : r0 + 1);
            const size_t ca = size_t(((c0 % width) + width) % width), cb = size_t((((c0 + 1) % width) + width) % width);
            float *o = texels + 3 * (size_t(y) * size_t(size) + size_t(x));
            for (int k = 0; k < 3; ++k) {
                const double top = (1.0 - fc) * rgb[3 * (ra * W + ca) + k] + fc * rgb[3 * (ra * W + cb) + k];
                const double bot = (1.0 - fc) * rgb[3 * (rb * W + ca) + k] + fc * rgb[3 * (rb * W + cb) + k];
                o[k] = float((1.0 - fr) * top + fr * bot);
            }
        }
    return true;
}

bool read_pfm(const std::string &path, std::vector<float> &rgb, int &width, int &height, std::string *err) {
    std::unique_ptr<FILE, int (*)(FILE *)> f(std::fopen(path.c_str(), "rb"), std::fclose);
    if (!f) return fail(err, "cannot open " + path);
    // the header: three whitespace-separated tokens ("PF", "width height" as two, scale), then one
    // whitespace byte, then the rows
    auto token = [&](std::string &out) -> bool {
        out.clear();
        int c = std::fgetc(f.get());
        while (c != EOF && std::isspace(c)) c = std::fgetc(f.get());
        while (c != EOF && !std::isspace(c)) {
            if (out.size() >= 32) return false;
            out.push_back(char(c));
            c = std::fgetc(f.get());
        }
        return !out.empty() && c != EOF;  // (the byte after the token is its separator)
    };
    std::string magic, ws, hs, ss;
    if (!token(magic)) return fail(err, path + ": truncated PFM header");
    if (magic == "Pf") return fail(err, path + ": a grey PFM (Pf); a colour one (PF) is needed");
    if (magic != "PF") return fail(err, path + ": not a PFM file");
    if (!token(ws) || !token(hs) || !token(ss)) return fail(err, path + ": truncated PFM header");
    auto integer = [](const std::string &t, long long &v) -> bool {
        if (t.empty() || t.size() > 9) return false;
        v = 0;
        for (char ch : t) {
            if (ch < '0' || ch > '9') return false;
            v = v * 10 + (ch - '0');
        }
        return true;
    };
    long long w = 0, h = 0;
    if (!integer(ws, w) || !integer(hs, h)) return fail(err, path + ": malformed PFM dimensions");
    if (w < 1 || h < 1 || w > kMaxImageSide || h > kMaxImageSide)
        return fail(err, path + ": PFM dimensions must be in 1.." + std::to_string(kMaxImageSide));
    char *end = nullptr;
    const double scale = std::strtod(ss.c_str(), &end);
    if (end == ss.c_str() || *end != '\0' || !std::isfinite(scale) || scale == 0.0)
        return fail(err, path + ": malformed PFM scale");
    if (scale > 0.0) return fail(err, path + ": a big-endian PFM; a little-endian one (negative scale) is needed");
    const size_t row = size_t(w) * 3;
    // the data's size against the file's, before anything is allocated for it
    const long at = std::ftell(f.get());
    if (at < 0 || std::fseek(f.get(), 0, SEEK_END) != 0) return fail(err, path + ": cannot seek");
    const long fileEnd = std::ftell(f.get());
    if (fileEnd < at || std::fseek(f.get(), at, SEEK_SET) != 0) return fail(err, path + ": cannot seek");
    if ((unsigned long long)(fileEnd - at) < (unsigned long long)row * (unsigned long long)h * sizeof(float))
        return fail(err, path + ": PFM data is shorter than its header says");
    std::vector<float> out(row * size_t(h));
    for (long long r = h - 1; r >= 0; --r) {  // the file's rows run bottom to top
        float *dst = out.data() + size_t(r) * row;
        if (std::fread(dst, sizeof(float), row, f.get()) != row) return fail(err, path + ": PFM data is shorter than its header says");
    }
    static_assert(sizeof(float) == 4, "PFM samples are 32-bit floats");
    const uint16_t one = 1;
    unsigned char lo;
    std::memcpy(&lo, &one, 1);
    if (!lo)  // a big-endian host: swap the little-endian samples
        for (float &v : out) {
            unsigned char b[4];
            std::memcpy(b, &v, 4);
            const unsigned char s[4] = {b[3], b[2], b[1], b[0]};
            std::memcpy(&v, s, 4);
        }
    rgb.swap(out);
    width = int(w);
    height = int(h);
    return true;
}

}  // namespace envio
}  // namespace hippt
