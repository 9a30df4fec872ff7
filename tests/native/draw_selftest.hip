// draw_selftest.hip — test helper (not product code): runs the kernels' unit-sphere draw
// (qt-raytracer_amd/csrc/hippt_trace.h rius, the loop without the table) on entry states given by
// the host, one block of 256 threads (four waves), each wave under its own lane mask, and returns
// every lane's exit state, coordinates and |p|^2.  Used by tests/test_gpu_unit_draw.py through ctypes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hippt_trace.h"

#pragma clang fp contract(off)

using namespace hippt::trace;

namespace {

constexpr int kLanes = 256;

// active[w]: the lanes of wave w that call rius (the others keep state in, x = y = z = 0, r2 = -1)
__global__ __launch_bounds__(kLanes) void draw(const uint32_t *in, const unsigned long long *active, uint32_t *state,
                                               float4 *out) {
    const unsigned i = threadIdx.x;
    uint32_t s = in[i];
    float x = 0.0f, y = 0.0f, z = 0.0f, r2 = -1.0f;
    if ((active[i >> 6] >> (i & 63u)) & 1ull) r2 = rius<false>(s, x, y, z, nullptr);
    state[i] = s;
    out[i] = make_float4(x, y, z, r2);
}

}  // namespace

// in[256], active[4] -> state[256], out[256][4] (x, y, z, r2).  0 = ok.
extern "C" int draw_selftest(const uint32_t *in, const unsigned long long *active, uint32_t *state, float *out) {
    uint32_t *dIn = nullptr, *dState = nullptr;
    unsigned long long *dAct = nullptr;
    float4 *dOut = nullptr;
    bool ok = hipMalloc(&dIn, kLanes * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&dState, kLanes * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&dAct, 4 * sizeof(unsigned long long)) == hipSuccess &&
              hipMalloc(&dOut, kLanes * sizeof(float4)) == hipSuccess;
    ok = ok && hipMemcpy(dIn, in, kLanes * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dAct, active, 4 * sizeof(unsigned long long), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(draw, dim3(1), dim3(kLanes), 0, 0, dIn, dAct, dState, dOut);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(state, dState, kLanes * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(out, dOut, kLanes * sizeof(float4), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(dIn);
    (void)hipFree(dState);
    (void)hipFree(dAct);
    (void)hipFree(dOut);
    return ok ? 0 : 1;
}
