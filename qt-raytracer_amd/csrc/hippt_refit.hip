// hippt_refit.hip — device refit of an uploaded scene to new triangle vertices (hippt_refit.h).
//
// Three kinds of launch, all plain stream-ordered kernels (no launch waits on another block; the
// hand-off between tree levels is the kernel boundary):
//   refit_prims   one lane per primitive record in leaf order: the triangle's record and normal as
//                 hipptUploadScene writes them (same operations in the same order: explicit fmaf only,
//                 IEEE sqrt and division; the library is built with -ffp-contract=off), its unpadded
//                 box, and the largest |coordinate| folded into one word by an integer max of the
//                 float's bits (non-negative floats order like their bits)
//   refit_level   one lane per child slot of one level of a tree: the slot's unpadded box = the union
//                 of its leaf's primitive boxes or of its child node's unpadded slot boxes (written
//                 by the previous launch), kept on the side, and the node's box = that moved out once
//                 by the pad of the update's largest |coordinate| (bvh_builder.h refit_bvh)
// and, behind them for a scene with lights, the four launches that rebuild the light selection table
// from the refitted primitive records (HIPPT_OPT_LIGHT_SELECT; below).  The environment's selection table
// (HIPPT_OPT_ENV_SAMPLING), built behind every hipptSetEnvironment, sits beside it: it shares the block scan.
#include "hippt_refit.h"

#include <algorithm>

#include "bvh_builder.h"
#include "hippt_device.h"

namespace hippt {
namespace {

__device__ inline float f_of(unsigned u) { return __uint_as_float(u); }
__device__ inline int i_of(float f) { return __float_as_int(f); }

__global__ __launch_bounds__(kRefitBlock) void refit_prims(RefitBuffers B) {
    const int k = int(blockIdx.x) * kRefitBlock + int(threadIdx.x);
    unsigned maxBits = 0u;
    if (k < B.numPrims) {
        const float4 r2 = B.tris[3 * size_t(k) + 2];
        const int id = i_of(r2.y);
        float lo[3], hi[3];
        bool have = true;
        if (i_of(r2.z) == 1) {  // sphere: its record stays; the upload's box
            const float4 q = B.tris[3 * size_t(k)];
            const float c[3] = {q.x, q.y, q.z};
            const float r = fabsf(q.w) * (1.0f + 1.0f / 4096.0f);
            for (int a = 0; a < 3; ++a) {
                lo[a] = c[a] - r;
                hi[a] = c[a] + r;
            }
        } else {
            float v[9];
            bool finite = unsigned(id) < unsigned(B.numTris);
            for (int j = 0; j < 9; ++j) {
                v[j] = finite ? B.verts[9 * size_t(id) + j] : 0.0f;
                finite = finite && isfinite(v[j]);
            }
            const float w = B.shade[k].w;  // the material word
            if (!finite) {
                // a non-finite vertex the host could not see: the upload's degenerate record with v0
                // zeroed (no ray hits it), no box, counted
                have = false;
                B.tris[3 * size_t(k)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                B.tris[3 * size_t(k) + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                B.tris[3 * size_t(k) + 2] = make_float4(0.0f, r2.y, 0.0f, 0.0f);
                B.shade[k] = make_float4(0.0f, 0.0f, 0.0f, w);
                atomicAdd(&B.words[1], 1u);
            } else {
                float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
                float e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
                float cr[3], n[3];
                cr[0] = fmaf(e1[1], e2[2], -(e1[2] * e2[1]));
                cr[1] = fmaf(e1[2], e2[0], -(e1[0] * e2[2]));
                cr[2] = fmaf(e1[0], e2[1], -(e1[1] * e2[0]));
                const float len = sqrtf(fmaf(cr[0], cr[0], fmaf(cr[1], cr[1], cr[2] * cr[2])));
                if (!(len > 0.0f)) {
                    e1[0] = e1[1] = e1[2] = 0.0f;
                    e2[0] = e2[1] = e2[2] = 0.0f;
                    n[0] = n[1] = n[2] = 0.0f;
                } else {
                    const float inv = 1.0f / len;
                    for (int a = 0; a < 3; ++a) n[a] = cr[a] * inv;
                }
                B.tris[3 * size_t(k)] = make_float4(v[0], v[1], v[2], e1[0]);
                B.tris[3 * size_t(k) + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
                B.tris[3 * size_t(k) + 2] = make_float4(e2[2], r2.y, 0.0f, 0.0f);
                B.shade[k] = make_float4(n[0], n[1], n[2], w);
                for (int a = 0; a < 3; ++a) {
                    lo[a] = fminf(v[a], fminf(v[3 + a], v[6 + a]));
                    hi[a] = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
                }
            }
        }
        if (!have)
            for (int a = 0; a < 3; ++a) {
                lo[a] = INFINITY;
                hi[a] = -INFINITY;
            }
        float2 *pb = reinterpret_cast<float2 *>(B.pbox + 6 * size_t(k));
        pb[0] = make_float2(lo[0], lo[1]);
        pb[1] = make_float2(lo[2], hi[0]);
        pb[2] = make_float2(hi[1], hi[2]);
        if (have)
            for (int a = 0; a < 3; ++a)
                maxBits = max(maxBits, max(__float_as_uint(fabsf(lo[a])), __float_as_uint(fabsf(hi[a]))));
    }
    // one atomic per wave
    for (int d = 32; d > 0; d >>= 1) maxBits = max(maxBits, unsigned(__shfl_xor(int(maxBits), d)));
    if ((threadIdx.x & 63u) == 0u && maxBits) atomicMax(&B.words[0], maxBits);
}

// WIDTH 2: 16-word nodes, codes are node indices.  WIDTH 4: 32-word nodes, interior codes are byte
// offsets (node * 128).
template <int WIDTH>
__global__ __launch_bounds__(kRefitBlock) void refit_level(uint32_t *nodes, const int *list, int count,
                                                          const float *pbox, float *ubox, const unsigned *words,
                                                          unsigned seedBits, int numNodes, int numPrims,
                                                          float *padOut) {
    constexpr int NW = WIDTH == 2 ? kNodeWords : kNode4Words;
    const int lane = int(blockIdx.x) * kRefitBlock + int(threadIdx.x);
    if (lane >= count * WIDTH) return;
    const float pad = fmaxf(f_of(max(words[0], seedBits)), 1e-3f) * (1.0f / 65536.0f);
    // the update's pad for the renderer (every level's launch writes the same value)
    if (lane == 0 && padOut) *padOut = pad;
    const int node = list[lane / WIDTH], slot = lane % WIDTH;
    if (unsigned(node) >= unsigned(numNodes)) return;
    uint32_t *w = nodes + size_t(node) * NW;
    const int code = int(w[node_code_word(WIDTH, slot)]);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool used = true;
    if (code < 0) {
        const int first = (~code) >> 4, n = (~code) & 15;
        used = n != 0;
        if (first + n <= numPrims)
            for (int p = first; p < first + n; ++p) {
                const float *b = pbox + 6 * size_t(p);
                for (int a = 0; a < 3; ++a) {
                    lo[a] = fminf(lo[a], b[a]);
                    hi[a] = fmaxf(hi[a], b[3 + a]);
                }
            }
    } else {
        const int child = WIDTH == 2 ? code : code >> 7;
        if (unsigned(child) < unsigned(numNodes)) {
            const float *u = ubox + size_t(child) * WIDTH * 6;
            for (int c = 0; c < WIDTH; ++c)
                for (int a = 0; a < 3; ++a) {
                    lo[a] = fminf(lo[a], u[6 * c + a]);
                    hi[a] = fmaxf(hi[a], u[6 * c + 3 + a]);
                }
        }
    }
    float2 *ub = reinterpret_cast<float2 *>(ubox + (size_t(node) * WIDTH + slot) * 6);
    ub[0] = make_float2(lo[0], lo[1]);
    ub[1] = make_float2(lo[2], hi[0]);
    ub[2] = make_float2(hi[1], hi[2]);
    if (!used) return;  // an unused slot keeps its box
    const bool have = lo[0] <= hi[0];
    const float farPoint[3] = {kFarPoint[0], kFarPoint[1], kFarPoint[2]};  // every primitive below dropped
    for (int a = 0; a < 3; ++a) {
        w[node_lo_word(WIDTH, slot, a)] = __float_as_uint(have ? lo[a] - pad : farPoint[a]);
        w[node_hi_word(WIDTH, slot, a)] = __float_as_uint(have ? hi[a] + pad : farPoint[a]);
    }
}

template <int WIDTH>
void launch_levels(uint32_t *nodes, const int *list, const std::vector<int> &level, const RefitBuffers &b, float *ubox,
                   unsigned seedBits, int numNodes, float *padOut, hipStream_t s) {
    for (size_t k = 0; k + 1 < level.size(); ++k) {
        const int count = level[k + 1] - level[k];
        if (count <= 0) continue;
        const int blocks = (count * WIDTH + kRefitBlock - 1) / kRefitBlock;
        hipLaunchKernelGGL(refit_level<WIDTH>, dim3(blocks), dim3(kRefitBlock), 0, s, nodes, list + level[k], count,
                           b.pbox, ubox, b.words, seedBits, numNodes, b.numPrims, padOut);
    }
}

// ---- the light selection table (hippt_refit.h; the rule: include/hippt.h, tests/select_ref.py) ----
// Four launches in stream order over the light list, a lane per light; the hand-off between them is the
// kernel boundary (no block waits for another).  Everything summed is an integer, and the one maximum is
// an integer maximum of non-negative floats' bits, so no word depends on the order of arrival.

// Inclusive scan of v over the block's kRefitBlock threads, all of which call it; `total`: the block's sum.
__device__ inline unsigned block_scan(unsigned v, unsigned *waveSums, unsigned &total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned d = 1; d < 64; d <<= 1) {
        const unsigned o = unsigned(__shfl_up(int(v), d));
        if (lane >= d) v += o;
    }
    if (lane == 63u) waveSums[wave] = v;
    __syncthreads();
    total = 0;
    for (unsigned w = 0; w < unsigned(kRefitBlock) / 64u; ++w) {
        const unsigned s = waveSums[w];
        if (w < wave) v += s;
        total += s;
    }
    __syncthreads();  // (the sums may be written again)
    return v;
}

// W_j = A_j * y_j of a lit light (A_j > 0 and y_j > 0), -1 for an unlit one, and Wmax.
__global__ __launch_bounds__(kRefitBlock) void light_weights(LightTableBuffers B) {
    const int j = int(blockIdx.x) * kRefitBlock + int(threadIdx.x);
    unsigned maxBits = 0u;
    if (j < B.numLights) {
        const int k = B.lights[j];
        float W = -1.0f;
        if (unsigned(k) < unsigned(B.numPrims)) {
            const float4 A = B.tris[3 * size_t(k)];
            const int mw = i_of(B.shade[k].w);
            float area;
            if (mw & kShadeSphere) {
                area = (12.566371f * A.w) * A.w;
            } else {  // the path kernel's light_area
                const float4 E = B.tris[3 * size_t(k) + 1];
                const float e1x = A.w, e1y = E.x, e1z = E.y;
                const float e2x = E.z, e2y = E.w, e2z = B.tris[3 * size_t(k) + 2].x;
                const float cx = fmaf(e1y, e2z, -(e1z * e2y)), cy = fmaf(e1z, e2x, -(e1x * e2z)),
                            cz = fmaf(e1x, e2y, -(e1y * e2x));
                area = 0.5f * sqrtf(fmaf(cx, cx, fmaf(cy, cy, cz * cz)));
            }
            const float4 le = B.mats[2 * size_t(mw & ~kShadeSphere)];
            const float y = (le.x + le.y) + le.z;
            if (area > 0.0f && y > 0.0f) {
                W = area * y;
                maxBits = __float_as_uint(W);
            }
        }
        B.weights[j] = W;
    }
    // one atomic per wave
    for (int d = 32; d > 0; d >>= 1) maxBits = max(maxBits, unsigned(__shfl_xor(int(maxBits), d)));
    if ((threadIdx.x & 63u) == 0u && maxBits) atomicMax(&B.words[0], maxBits);
}

// q_j, its inclusive sum within the block, and the block's sum.
__global__ __launch_bounds__(kRefitBlock) void light_scan_blocks(LightTableBuffers B) {
    __shared__ unsigned waveSums[kRefitBlock / 64];
    const int j = int(blockIdx.x) * kRefitBlock + int(threadIdx.x);
    unsigned q = 0u;
    if (j < B.numLights) {
        const float W = B.weights[j], Wmax = f_of(B.words[0]);
        if (W >= 0.0f) {
            const bool flat = !(Wmax > 0.0f && Wmax < INFINITY);
            q = flat ? 1u : unsigned(min(4096, max(1, int((W / Wmax) * 4096.0f))));
        }
    }
    unsigned total;
    const unsigned c = block_scan(q, waveSums, total);
    if (j < B.numLights) {
        B.cdf[j] = c;
        B.records[4 * size_t(j) + 1] = q;
    }
    if (threadIdx.x == 0u) B.blockSums[blockIdx.x] = total;
}

// One block: the blocks' sums become the blocks' offsets (their exclusive sums), and T.
__global__ __launch_bounds__(kRefitBlock) void light_scan_sums(LightTableBuffers B) {
    __shared__ unsigned waveSums[kRefitBlock / 64];
    const int blocks = (B.numLights + kRefitBlock - 1) / kRefitBlock;
    const int per = (blocks + kRefitBlock - 1) / kRefitBlock;
    const int first = min(int(threadIdx.x) * per, blocks), last = min(first + per, blocks);
    unsigned sum = 0u;
    for (int i = first; i < last; ++i) sum += B.blockSums[i];
    unsigned total;
    unsigned at = block_scan(sum, waveSums, total) - sum;
    for (int i = first; i < last; ++i) {
        const unsigned s = B.blockSums[i];
        B.blockSums[i] = at;
        at += s;
    }
    if (threadIdx.x == 0u) B.words[1] = total;
}

// c_j with its block's offset, ip_j, the record, and ip by primitive.
__global__ __launch_bounds__(kRefitBlock) void light_finish(LightTableBuffers B) {
    const int j = int(blockIdx.x) * kRefitBlock + int(threadIdx.x);
    if (j >= B.numLights) return;
    const unsigned q = B.records[4 * size_t(j) + 1];
    const unsigned c = B.cdf[j] + B.blockSums[blockIdx.x];
    const float ip = q > 0u ? float(B.words[1]) / float(q) : 0.0f;
    const int k = B.lights[j];
    const bool have = unsigned(k) < unsigned(B.numPrims);
    B.cdf[j] = c;
    B.records[4 * size_t(j)] = have ? unsigned(i_of(B.tris[3 * size_t(k) + 2].y)) : ~0u;
    B.records[4 * size_t(j) + 2] = c;
    B.records[4 * size_t(j) + 3] = __float_as_uint(ip);
    if (have) B.ipPrim[k] = ip;
}

// ---- the environment's selection table (hippt_refit.h; the rule: include/hippt.h, tests/envs_ref.py) ----
// Three launches in stream order; the hand-off between them is the kernel boundary.  The per-texel arithmetic
// is hippt_env.h's.  Every reduction is a maximum of non-negative floats' bits or a sum of integers, so no word
// depends on the order in which it combines.

// The largest v over the block's kRefitBlock threads, all of which call it.
__device__ inline unsigned block_max(unsigned v, unsigned *waveMax) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, unsigned(__shfl_xor(int(v), d)));
    if ((threadIdx.x & 63u) == 0u) waveMax[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned m = 0u;
    for (unsigned w = 0; w < unsigned(kRefitBlock) / 64u; ++w) m = max(m, waveMax[w]);
    __syncthreads();  // (the words may be written again)
    return m;
}

// A block per row y, a thread per run of at most 16 texels: Wmax_y, q and c along the row, V_y.
__global__ __launch_bounds__(kRefitBlock) void env_table_rows(EnvTableBuffers B) {
    __shared__ unsigned waveWords[kRefitBlock / 64];
    const int size = B.size, y = int(blockIdx.x);
    const int per = (size + kRefitBlock - 1) / kRefitBlock;
    const int first = min(int(threadIdx.x) * per, size), last = min(first + per, size);
    const env::Texel *in = B.env + size_t(y) * size_t(size);
    env::TexelSel *out = B.texels + size_t(y) * size_t(size);
    unsigned maxBits = 0u;
#pragma unroll 1
    for (int x = first; x < last; ++x) maxBits = max(maxBits, __float_as_uint(env::texel_weight(in[x], x, y, size)));
    const float Wmax = f_of(block_max(maxBits, waveWords));
    unsigned sum = 0u;
#pragma unroll 1
    for (int x = first; x < last; ++x) {
        const unsigned q = env::texel_q(env::texel_weight(in[x], x, y, size), Wmax);
        out[x].c = q;
        sum += q;
    }
    unsigned total;
    unsigned at = block_scan(sum, waveWords, total) - sum;
#pragma unroll 1
    for (int x = first; x < last; ++x) {
        at += out[x].c;
        out[x].c = at;
    }
    if (threadIdx.x == 0u) B.rowV[y] = env::row_value(total, Wmax);
}

// One block over the rows, a thread per run of at most 16: Vmax, m_y, C_y.
__global__ __launch_bounds__(kRefitBlock) void env_table_scan_rows(EnvTableBuffers B) {
    __shared__ unsigned waveWords[kRefitBlock / 64];
    const int size = B.size;
    const int per = (size + kRefitBlock - 1) / kRefitBlock;
    const int first = min(int(threadIdx.x) * per, size), last = min(first + per, size);
    unsigned maxBits = 0u;
#pragma unroll 1
    for (int y = first; y < last; ++y) maxBits = max(maxBits, __float_as_uint(B.rowV[y]));
    const float Vmax = f_of(block_max(maxBits, waveWords));
    unsigned sum = 0u;
#pragma unroll 1
    for (int y = first; y < last; ++y) {
        const unsigned m = env::row_m(B.rowV[y], Vmax);
        B.rowM[y] = m;
        sum += m;
    }
    unsigned total;
    unsigned at = block_scan(sum, waveWords, total) - sum;
#pragma unroll 1
    for (int y = first; y < last; ++y) {
        at += B.rowM[y];
        B.rowC[y] = at;
    }
}

// k(x, y), a lane per texel, grid stride.
__global__ __launch_bounds__(kRefitBlock) void env_table_finish(EnvTableBuffers B) {
    const unsigned size = unsigned(B.size), count = size * size;  // (<= 2^24)
    const unsigned T = B.rowC[size - 1u];
    for (unsigned i = blockIdx.x * unsigned(kRefitBlock) + threadIdx.x; i < count; i += gridDim.x * unsigned(kRefitBlock)) {
        const unsigned y = i / size, x = i - y * size;
        const unsigned c = B.texels[i].c, q = x ? c - B.texels[i - 1u].c : c;
        B.texels[i].k = env::texel_k(B.rowM[y], T, q, B.texels[size_t(y) * size + size - 1u].c, int(size));
    }
}

}  // namespace

EnvTableBuffers env_table_buffers(const env::Texel *env, unsigned *base, int size) {
    const size_t n = size_t(size);
    EnvTableBuffers b{};
    b.env = env;
    b.texels = reinterpret_cast<env::TexelSel *>(base);
    b.rowC = base + 2 * n * n;
    b.rowM = b.rowC + n;
    b.rowV = reinterpret_cast<float *>(b.rowM + n);
    b.size = size;
    return b;
}

hipError_t launch_env_table(const EnvTableBuffers &b, hipStream_t s) {
    if (b.size < 1 || b.size > env::kMaxSize || !b.env || !b.texels) return hipErrorInvalidValue;
    const unsigned count = unsigned(b.size) * unsigned(b.size);
    const unsigned blocks = std::min(4096u, (count + unsigned(kRefitBlock) - 1u) / unsigned(kRefitBlock));
    hipLaunchKernelGGL(env_table_rows, dim3(b.size), dim3(kRefitBlock), 0, s, b);
    hipLaunchKernelGGL(env_table_scan_rows, dim3(1), dim3(kRefitBlock), 0, s, b);
    hipLaunchKernelGGL(env_table_finish, dim3(blocks), dim3(kRefitBlock), 0, s, b);
    return hipGetLastError();
}

LightTableBuffers light_table_buffers(unsigned *base, int numLights, int numPrims) {
    const size_t n = size_t(numLights), p = size_t(numPrims);
    LightTableBuffers b{};
    b.cdf = base;
    b.records = b.cdf + n;
    b.ipPrim = reinterpret_cast<float *>(b.records + 4 * n);
    b.weights = b.ipPrim + p;
    b.blockSums = reinterpret_cast<unsigned *>(b.weights + n);
    b.words = b.blockSums + (n + kRefitBlock - 1) / kRefitBlock;
    b.numLights = numLights;
    b.numPrims = numPrims;
    return b;
}

hipError_t launch_light_table(const LightTableBuffers &b, hipStream_t s) {
    if (b.numLights <= 0 || !light_table_fits(size_t(b.numLights)) || b.numPrims <= 0) return hipErrorInvalidValue;
    if (!b.tris || !b.shade || !b.mats || !b.lights || !b.cdf) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(b.words, 0, 2 * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const dim3 grid((b.numLights + kRefitBlock - 1) / kRefitBlock), block(kRefitBlock);
    hipLaunchKernelGGL(light_weights, grid, block, 0, s, b);
    hipLaunchKernelGGL(light_scan_blocks, grid, block, 0, s, b);
    hipLaunchKernelGGL(light_scan_sums, dim3(1), block, 0, s, b);
    hipLaunchKernelGGL(light_finish, grid, block, 0, s, b);
    return hipGetLastError();
}

hipError_t launch_refit(const RefitBuffers &b, const std::vector<int> &level2, const std::vector<int> &level4,
                        unsigned seedBits, hipStream_t s) {
    if (b.numPrims <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(b.words, 0, 2 * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refit_prims, dim3((b.numPrims + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, s, b);
    launch_levels<2>(b.nodes2, b.list2, level2, b, b.ubox2, seedBits, b.numNodes2, nullptr, s);
    launch_levels<4>(b.nodes4, b.list4, level4, b, b.ubox4, seedBits, b.numNodes4, b.padOut, s);
    return hipGetLastError();
}

}  // namespace hippt
