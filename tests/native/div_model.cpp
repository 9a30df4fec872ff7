// div_model.cpp — host restatement (not product code) of the kernels' short division sequences
// (qt-raytracer_amd/csrc/hippt_trace.h div_core, div_rn, avg_div, avg_div_guard) with fmaf and
// 1.0f / b, which rcp_nr equals on its verified range, against the compiler's IEEE a / b.
// Stand-alone: tests/test_division_model.py builds and runs it; no GPU.
//
//   grid      every divisor mantissa at three exponents x 64 numerator mantissas
//   exponents every pair of biased exponents 0..255 x 0..255 (zeros, denormals, infinities and NaN
//             included) x eight mantissa pairs x four sign pairs
//   random    10^7 hashed pairs over all exponents
//   average   the combine's shape: the divisors float(n) of the GPU test's list against the special
//             numerators and 2^16 hashed ones each
// Each prints its mismatch counts: the guarded function everywhere, the bare sequence on its claimed
// domain.  Exit status 0 when all are zero.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <thread>
#include <vector>

namespace {

float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
uint32_t hash32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// ---- the helpers, restated (rcp_nr(b) == 1.0f / b for 2^-126 <= |b| < 2^126) ----
float div_core(float a, float b, float y) {
    const float q = a * y;
    return fmaf(fmaf(-b, q, a), y, q);
}
bool in_core_domain(float a, float b) {
    const float aa = fabsf(a), ab = fabsf(b), qq = fabsf(a / b);
    return ab >= 0x1p-126f && ab < 0x1p126f && aa >= 0x1p-102f && aa < INFINITY && qq >= 0x1p-126f && qq < INFINITY;
}
float div_rn(float a, float b) {
    const float aa = fabsf(a), ab = fabsf(b);
    if (aa >= 0x1p-62f && aa <= 0x1p62f && ab >= 0x1p-62f && ab <= 0x1p62f) return div_core(a, b, 1.0f / b);
    return a / b;
}
float avg_div(float a, float fc, float y) {
    const float q = a * y;
    return fmaf(fmaf(fc, q, -a), -y, q);
}
bool avg_div_guard(float ax, float ay, float az, float qx, float qy, float qz) {
    const uint32_t ux = (bits(ax) << 1) - 1u, uy = (bits(ay) << 1) - 1u, uz = (bits(az) << 1) - 1u;
    return std::min(ux, std::min(uy, uz)) < 2u * 0x10800000u - 1u || !(fabsf(qx) + fabsf(qy) + fabsf(qz) < INFINITY);
}
bool in_avg_domain(float a) { return a == 0.0f || (fabsf(a) >= 0x1p-94f && fabsf(a) < INFINITY); }
// the combine's rule for one sample (a in channel k, the other two numerators +0 and 1): the fast quotient
// unless the guard fires
float avg_guarded(float a, float fc, int k) {
    const float y = 1.0f / fc, r = avg_div(a, fc, y), one = avg_div(1.0f, fc, y);
    const bool g = k == 0 ? avg_div_guard(a, 0.0f, 1.0f, r, 0.0f, one)
                 : k == 1 ? avg_div_guard(1.0f, a, 0.0f, one, r, 0.0f) : avg_div_guard(0.0f, 1.0f, a, 0.0f, one, r);
    return g ? a / fc : r;
}

struct Counts {
    unsigned long long guarded = 0, core = 0, inDomain = 0, pairs = 0;
    void add(const Counts &o) { guarded += o.guarded, core += o.core, inDomain += o.inDomain, pairs += o.pairs; }
};

void check_pair(float a, float b, Counts &c) {
    const float ref = a / b;
    ++c.pairs;
    c.guarded += !same(div_rn(a, b), ref);
    if (in_core_domain(a, b)) {
        ++c.inDomain;
        c.core += !same(div_core(a, b, 1.0f / b), ref);
    }
}

uint32_t numerator_mantissa(unsigned k, uint32_t seed) {
    switch (k) {
    case 0: return 0u;
    case 1: return 1u;
    case 2: return 0x7fffffu;
    case 3: return 0x3fffffu;
    case 4: return 0x400001u;
    default: return hash32(seed * 64u + k) & 0x7fffffu;
    }
}

template <typename F>
Counts parallel(unsigned long long n, F body) {
    const unsigned nt = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<Counts> part(nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            for (unsigned long long i = t; i < n; i += nt) body(i, part[t]);
        });
    Counts c;
    for (unsigned t = 0; t < nt; ++t) th[t].join(), c.add(part[t]);
    return c;
}

Counts grid() {
    const uint32_t exps[3] = {1u, 127u, 252u};  // 2^-126, 1, 2^125: the ends of rcp_nr's range and the middle
    return parallel(3ull << 23, [&](unsigned long long i, Counts &c) {
        const uint32_t eb = exps[i >> 23], mb = uint32_t(i) & 0x7fffffu;
        const float b = from_bits((eb << 23) | mb);
        for (unsigned k = 0; k < 64; ++k) {
            const uint32_t h = hash32(uint32_t(i) ^ (k * 0x9E3779B9u));
            int ea = int(eb) + int(h % 49u) - 24;  // the quotient's exponent within +-24 of zero
            ea = ea < 1 ? 1 : ea > 254 ? 254 : ea;
            const float a = from_bits(((h >> 31) << 31) | (uint32_t(ea) << 23) | numerator_mantissa(k, uint32_t(i)));
            check_pair(a, b, c);
        }
    });
}

Counts exponents() {
    return parallel(256ull * 256ull, [&](unsigned long long i, Counts &c) {
        const uint32_t ea = uint32_t(i) >> 8, eb = uint32_t(i) & 255u;
        const uint32_t h0 = hash32(uint32_t(i) * 2u + 1u), h1 = hash32(uint32_t(i) * 2u + 2u);
        const uint32_t ma[8] = {0u, 0x7fffffu, 0u, 0x7fffffu, 1u, 0x400000u, h0 & 0x7fffffu, h1 & 0x7fffffu};
        const uint32_t mb[8] = {0u, 0x7fffffu, 0x7fffffu, 0u, 0x7ffffeu, 1u, h1 >> 9, h0 >> 9};
        for (unsigned k = 0; k < 8; ++k)
            for (uint32_t s = 0; s < 4; ++s)
                check_pair(from_bits(((s & 1u) << 31) | (ea << 23) | ma[k]), from_bits(((s >> 1) << 31) | (eb << 23) | mb[k]), c);
    });
}

Counts random_pairs() {
    return parallel(10000000ull, [&](unsigned long long i, Counts &c) {
        check_pair(from_bits(hash32(uint32_t(i) * 2u + 0x1234567u)), from_bits(hash32(uint32_t(i) * 2u + 0x89abcdeu)), c);
    });
}

// the GPU test's divisors: n = 1..128, and 2^k - 1, 2^k, 2^k + 1 for k = 8..31 as float(int) rounds them
std::vector<float> average_divisors() {
    std::vector<float> d;
    for (int n = 1; n <= 128; ++n) d.push_back(float(n));
    for (int k = 8; k <= 31; ++k)
        for (long long n = (1ll << k) - 1; n <= (1ll << k) + 1; ++n) d.push_back(float(n));
    return d;
}

Counts average() {
    const std::vector<float> d = average_divisors();
    return parallel(d.size(), [&](unsigned long long i, Counts &c) {
        const float fc = d[i];
        auto one = [&](float a) {
            const float ref = a / fc;
            ++c.pairs;
            for (int k = 0; k < 3; ++k) c.guarded += bits(avg_guarded(a, fc, k)) != bits(ref);
            if (in_avg_domain(a)) {
                ++c.inDomain;
                c.core += bits(avg_div(a, fc, 1.0f / fc)) != bits(ref);  // bitwise: both zeros keep their sign
            }
        };
        for (uint32_t e = 0; e < 256; ++e)
            for (uint32_t m : {0u, 1u, 0x7fffffu, 0x400000u, 0x3fffffu, 0x555555u})
                for (uint32_t s = 0; s < 2; ++s) one(from_bits((s << 31) | (e << 23) | m));
        for (uint32_t k = 0; k < 65536u; ++k) one(from_bits(hash32(uint32_t(i) * 65536u + k)));
        // the multiples of fc and their neighbours, down into the denormals (exact quotients and ties)
        for (uint32_t k = 1; k < 4096u; ++k)
            for (int e = -149; e <= -120; e += 1) {
                const float a = ldexpf(float(k), e) * fc;
                one(a), one(nextafterf(a, 0.0f)), one(nextafterf(a, INFINITY));
                one(ldexpf(float(k), e) * fc * 0.5f);
            }
    });
}

int report(const char *name, const Counts &c) {
    std::printf("%s pairs %llu in_domain %llu guarded_mismatch %llu core_mismatch %llu\n", name, c.pairs, c.inDomain, c.guarded,
                c.core);
    return (c.guarded || c.core) ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "all";
    const bool all = !std::strcmp(what, "all");
    int bad = 0, ran = 0;
    if (all || !std::strcmp(what, "grid")) bad |= report("grid", grid()), ++ran;
    if (all || !std::strcmp(what, "exponents")) bad |= report("exponents", exponents()), ++ran;
    if (all || !std::strcmp(what, "random")) bad |= report("random", random_pairs()), ++ran;
    if (all || !std::strcmp(what, "average")) bad |= report("average", average()), ++ran;
    if (!ran) {
        std::fprintf(stderr, "usage: div_model [all|grid|exponents|random|average]\n");
        return 2;
    }
    return bad;
}
