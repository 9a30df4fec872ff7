// env_sample_check.cpp — a stand-alone check of the environment sampling arithmetic of
// qt-raytracer_amd/csrc/hippt_env.h (HIPPT_OPT_ENV_SAMPLING), the text the kernels compile: the
// table's per-texel and per-row words, the draw with its density, the connection's factor and the weight of a miss,
// against the words tests/envs_ref.py wrote.  No HIP, no library: tests/test_envs_ref_cpu.py compiles it by one
// compiler call and runs it; built with -fsanitize=address,undefined it is the sanitizer run of that code.
//
//   env_sample_check FILE
//
// FILE, 32-bit little-endian words: S, nDraw, nMiss, 0; the map E (S * S * 3 floats); the expected rows (S x (m, C));
// the expected texels (S * S x (q, c, bits of k)); nDraw x (rng, n.x, n.y, n.z, sel, mis) and their expected
// (rng after, x, y, om.x, om.y, om.z, n3, k, shadow ray?, factor); nMiss x (d.x, d.y, d.z, cb, sel) and their
// expected wb.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hippt_env.h"

using namespace hippt::env;

static int failures = 0;

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float fl(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static void same(uint32_t got, uint32_t want, const char *what, long i) {
    if (got != want && failures++ < 20) std::printf("FAIL %s %ld: %08x, wanted %08x\n", what, i, got, want);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::printf("usage: env_sample_check FILE\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::printf("FAIL cannot read %s\n", argv[1]);
        return 1;
    }
    std::vector<uint32_t> w;
    uint32_t buf[4096];
    for (size_t n; (n = std::fread(buf, 4, 4096, f)) > 0;) w.insert(w.end(), buf, buf + n);
    std::fclose(f);
    if (w.size() < 4) {
        std::printf("FAIL short file\n");
        return 1;
    }
    const size_t S = w[0], nDraw = w[1], nMiss = w[2];
    const size_t need = 4 + S * S * 3 + S * 2 + S * S * 3 + nDraw * 16 + nMiss * 6;
    if (S < 1 || S > size_t(kMaxSize) || w.size() != need) {
        std::printf("FAIL the file has %zu words, its header says %zu\n", w.size(), need);
        return 1;
    }
    const uint32_t *E = &w[4], *rows = E + S * S * 3, *tex = rows + S * 2, *draws = tex + S * S * 3;
    const uint32_t *drawsWant = draws + nDraw * 6, *miss = drawsWant + nDraw * 10, *missWant = miss + nMiss * 5;

    // the table, serially, by the header's per-texel and per-row functions
    std::vector<TexelSel> sel(S * S);
    std::vector<unsigned> rowC(S), rowM(S);
    std::vector<float> rowV(S);
    std::vector<float> W(S);
    for (size_t y = 0; y < S; ++y) {
        float Wmax = 0.0f;
        for (size_t x = 0; x < S; ++x) {
            const uint32_t *e = E + 3 * (y * S + x);
            W[x] = texel_weight(Texel{fl(e[0]), fl(e[1]), fl(e[2]), 0.0f}, int(x), int(y), int(S));
            if (W[x] > Wmax) Wmax = W[x];
        }
        unsigned c = 0;
        for (size_t x = 0; x < S; ++x) {
            const unsigned q = texel_q(W[x], Wmax);
            same(q, tex[3 * (y * S + x)], "q", long(y * S + x));
            c += q;
            sel[y * S + x].c = c;
            same(c, tex[3 * (y * S + x) + 1], "c", long(y * S + x));
        }
        rowV[y] = row_value(c, Wmax);
    }
    float Vmax = 0.0f;
    for (size_t y = 0; y < S; ++y)
        if (rowV[y] > Vmax) Vmax = rowV[y];
    unsigned C = 0;
    for (size_t y = 0; y < S; ++y) {
        rowM[y] = row_m(rowV[y], Vmax);
        C += rowM[y];
        rowC[y] = C;
        same(rowM[y], rows[2 * y], "m", long(y));
        same(C, rows[2 * y + 1], "C", long(y));
    }
    for (size_t y = 0; y < S; ++y)
        for (size_t x = 0; x < S; ++x) {
            const size_t i = y * S + x;
            const unsigned q = sel[i].c - (x ? sel[i - 1].c : 0u);
            sel[i].k = texel_k(rowM[y], C, q, sel[y * S + S - 1].c, int(S));
            same(bits(sel[i].k), tex[3 * i + 2], "k", long(i));
        }

    // draws and the connection's factor
    for (size_t i = 0; i < nDraw; ++i) {
        const uint32_t *in = draws + 6 * i, *want = drawsWant + 10 * i;
        unsigned rng = in[0];
        const Draw d = draw(rowC.data(), sel.data(), int(S), rng);
        same(rng, want[0], "draw rng", long(i));
        same(uint32_t(d.x), want[1], "draw x", long(i));
        same(uint32_t(d.y), want[2], "draw y", long(i));
        same(bits(d.ox), want[3], "draw om.x", long(i));
        same(bits(d.oy), want[4], "draw om.y", long(i));
        same(bits(d.oz), want[5], "draw om.z", long(i));
        same(bits(d.n3), want[6], "draw n3", long(i));
        same(bits(d.k), want[7], "draw k", long(i));
        float g = 0.0f;
        const bool ok = connect_factor(d, fdot3(fl(in[1]), fl(in[2]), fl(in[3]), d.ox, d.oy, d.oz), fl(in[4]), in[5] != 0, g);
        same(ok ? 1u : 0u, want[8], "shadow ray", long(i));
        if (ok) same(bits(g), want[9], "factor", long(i));
    }

    // the weight of a miss
    for (size_t i = 0; i < nMiss; ++i) {
        const uint32_t *in = miss + 5 * i;
        const float wb = miss_weight(sel.data(), int(S), fl(in[0]), fl(in[1]), fl(in[2]), fl(in[3]), fl(in[4]));
        same(bits(wb), missWant[i], "wb", long(i));
    }

    if (failures) {
        std::printf("env_sample_check: %d words differ\n", failures);
        return 1;
    }
    std::printf("env_sample_check ok: S %zu, %zu draws, %zu misses\n", S, nDraw, nMiss);
    return 0;
}
