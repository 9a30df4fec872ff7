// div_selftest.hip — test helper (not product code): checks the kernels' short division sequences
// (qt-raytracer_amd/csrc/hippt_trace.h div_core, div_rn, avg_div, avg_div_guard) against
// hipcc's IEEE a / b on the GPU.  Used by tests/test_gpu_division.py through ctypes.
#include <hip/hip_runtime.h>

#include "hippt_trace.h"

#pragma clang fp contract(off)

using namespace hippt::trace;

namespace {

constexpr int kCounts = 32;
// counts[] (mismatches unless said otherwise):
//   the running average's shape, every bit pattern of a against each divisor float(n):
//   0  the combine's rule (avg_div, or a / fc where avg_div_guard fires; a in each channel in turn, the other two
//      numerators +0 and 1) != a / fc, bitwise
//   1  avg_div != a / fc bitwise on its domain: a = +-0 or 2^-94 <= |a| < inf
//   2  avg_div of a NaN that is not a NaN
//   3  avg_div of a NaN that is not the division's NaN bit for bit (reported, the rule above never uses it)
//   4  pairs inside avg_div's domain (a count, not a mismatch)
//   general pairs, sweep s = 0 hashed, 1 grid, 2 exponent pairs, at 8 + 4 s:
//   +0 div_rn != a / b bitwise (every pair)
//   +1 div_core != a / b on its domain: 2^-126 <= |b| < 2^126, 2^-102 <= |a| < inf, 2^-126 <= |a / b| < inf
//   +2 unused
//   +3 pairs inside div_core's domain (a count)

__device__ __forceinline__ bool bitwise(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

__device__ __forceinline__ void flush(unsigned long long *counts, int k, unsigned long long c) {
    if (c) atomicAdd(&counts[k], c);
}

__global__ __launch_bounds__(256) void average_check(unsigned long long *counts, float fc, unsigned long long base,
                                                     unsigned long long n) {
    unsigned c[5] = {0, 0, 0, 0, 0};
    const float y = rcp_nr(fc);
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
        const float a = __uint_as_float(unsigned(base + i));
        const float ref = a / fc;
        const float fast = avg_div(a, fc, y);
        const float one = avg_div(1.0f, fc, y);
        const bool g[3] = {avg_div_guard(a, 0.0f, 1.0f, fast, 0.0f, one), avg_div_guard(1.0f, a, 0.0f, one, fast, 0.0f),
                           avg_div_guard(0.0f, 1.0f, a, 0.0f, one, fast)};
#pragma unroll
        for (int k = 0; k < 3; ++k) c[0] += !bitwise(g[k] ? a / fc : fast, ref);
        if (a == 0.0f || (fabsf(a) >= 0x1p-94f && fabsf(a) < INFINITY)) {
            c[1] += !bitwise(fast, ref);
            ++c[4];
        }
        if (a != a) {
            c[2] += !(fast != fast);
            c[3] += !bitwise(fast, ref);
        }
    }
    for (int k = 0; k < 5; ++k) flush(counts, k, c[k]);
}

__device__ __forceinline__ void check_pair(float a, float b, unsigned *c) {
    const float ref = a / b;
    c[0] += !bitwise(div_rn(a, b), ref);
    const float aa = fabsf(a), ab = fabsf(b), qq = fabsf(ref);
    if (ab >= 0x1p-126f && ab < 0x1p126f && aa >= 0x1p-102f && aa < INFINITY && qq >= 0x1p-126f && qq < INFINITY) {
        c[1] += !bitwise(div_core(a, b, rcp_nr(b)), ref);
        ++c[3];
    }
}

__device__ __forceinline__ uint32_t numerator_mantissa(unsigned k, uint32_t seed) {
    switch (k) {
    case 0: return 0u;
    case 1: return 1u;
    case 2: return 0x7fffffu;
    case 3: return 0x3fffffu;
    case 4: return 0x400001u;
    default: return hash32(seed * 64u + k) & 0x7fffffu;
    }
}

// SWEEP 0: pair i of a counter hash over all bit patterns.  1: divisor mantissa i mod 2^23 at exponent
// i >> 23 of (2^-126, 1, 2^125) against 64 numerators.  2: biased exponents (i >> 8, i & 255), eight mantissa
// pairs and four sign pairs.
template <int SWEEP>
__global__ __launch_bounds__(256) void general_check(unsigned long long *counts, unsigned long long base, unsigned long long n) {
    unsigned c[4] = {0, 0, 0, 0};
    for (unsigned long long j = blockIdx.x * 256ull + threadIdx.x; j < n; j += gridDim.x * 256ull) {
        const unsigned long long i = base + j;
        if (SWEEP == 0) {
            const uint32_t lo = uint32_t(i), hi = uint32_t(i >> 32);
            const uint32_t ua = hash32(lo ^ 0x1234567u) ^ hi, ub = hash32(hash32(lo + 0x9E3779B9u) ^ 0x89abcdeu);
            check_pair(__uint_as_float(ua), __uint_as_float(ub), c);
        } else if (SWEEP == 1) {
            const uint32_t exps[3] = {1u, 127u, 252u};
            const uint32_t eb = exps[i >> 23], mb = uint32_t(i) & 0x7fffffu;
            const float b = __uint_as_float((eb << 23) | mb);
            for (unsigned k = 0; k < 64; ++k) {
                const uint32_t h = hash32(uint32_t(i) ^ (k * 0x9E3779B9u));
                int ea = int(eb) + int(h % 49u) - 24;
                ea = ea < 1 ? 1 : ea > 254 ? 254 : ea;
                check_pair(__uint_as_float(((h >> 31) << 31) | (uint32_t(ea) << 23) | numerator_mantissa(k, uint32_t(i))), b, c);
            }
        } else {
            const uint32_t ea = uint32_t(i) >> 8, eb = uint32_t(i) & 255u;
            const uint32_t h0 = hash32(uint32_t(i) * 2u + 1u), h1 = hash32(uint32_t(i) * 2u + 2u);
            const uint32_t ma[8] = {0u, 0x7fffffu, 0u, 0x7fffffu, 1u, 0x400000u, h0 & 0x7fffffu, h1 & 0x7fffffu};
            const uint32_t mb[8] = {0u, 0x7fffffu, 0x7fffffu, 0u, 0x7ffffeu, 1u, h1 >> 9, h0 >> 9};
            for (unsigned k = 0; k < 8; ++k)
                for (uint32_t s = 0; s < 4; ++s)
                    check_pair(__uint_as_float(((s & 1u) << 31) | (ea << 23) | ma[k]),
                               __uint_as_float(((s >> 1) << 31) | (eb << 23) | mb[k]), c);
        }
    }
    for (int k = 0; k < 4; ++k) flush(counts, 8 + 4 * SWEEP + k, c[k]);
}

bool fetch(unsigned long long *d, unsigned long long *host) {
    return hipDeviceSynchronize() == hipSuccess &&
           hipMemcpy(host, d, kCounts * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
}

}  // namespace

// The running average's shape: every bit pattern of a against n = 1..128 and 2^k - 1, 2^k, 2^k + 1 for
// k = 8..31 as float(int) rounds them.  hostCounts: kCounts words.
extern "C" int div_selftest_average(unsigned long long *hostCounts) {
    unsigned long long *d = nullptr;
    if (hipMalloc(&d, kCounts * sizeof(unsigned long long)) != hipSuccess) return 1;
    (void)hipMemset(d, 0, kCounts * sizeof(unsigned long long));
    auto sweep = [&](float fc) { hipLaunchKernelGGL(average_check, dim3(8192), dim3(256), 0, 0, d, fc, 0ull, 1ull << 32); };
    for (int n = 1; n <= 128; ++n) sweep(float(n));
    for (int k = 8; k <= 31; ++k)
        for (long long n = (1ll << k) - 1; n <= (1ll << k) + 1; ++n) sweep(float(n));
    const bool ok = fetch(d, hostCounts);
    (void)hipFree(d);
    return ok ? 0 : 2;
}

// The general shape: 2^32 hashed pairs, the divisor-mantissa grid, the exponent pairs.
extern "C" int div_selftest_general(unsigned long long *hostCounts) {
    unsigned long long *d = nullptr;
    if (hipMalloc(&d, kCounts * sizeof(unsigned long long)) != hipSuccess) return 1;
    (void)hipMemset(d, 0, kCounts * sizeof(unsigned long long));
    const unsigned long long chunk = 1ull << 28;
    for (unsigned long long b = 0; b < (1ull << 32); b += chunk)
        hipLaunchKernelGGL(general_check<0>, dim3(8192), dim3(256), 0, 0, d, b, chunk);
    hipLaunchKernelGGL(general_check<1>, dim3(8192), dim3(256), 0, 0, d, 0ull, 3ull << 23);
    hipLaunchKernelGGL(general_check<2>, dim3(256), dim3(256), 0, 0, d, 0ull, 65536ull);
    const bool ok = fetch(d, hostCounts);
    (void)hipFree(d);
    return ok ? 0 : 2;
}
