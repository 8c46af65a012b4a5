// Microbenchmark (GPU box): the skeleton of pn_trunk_filter_kernel's conv3 loop on v_mfma_f32_32x32x16_f16 (SHAPE 0, the kernel's)
// and on v_mfma_f32_16x16x32_f16 (SHAPE 1), same output tile per wave and chunk (64 points x 64 channels, K = 128), with what
// makes the real loop what it is: 256-thread workgroups, two per CU (the kernel's LDS request), the W3 fragments read from LDS every
// chunk (16 ds_read_b128 per wave and chunk in both shapes, the kernel's swizzle), the A operand in registers, per 16 scores of a
// lane the kernel's top-two chain (16 v_and_or_b32 + the v_max3 / v_med3 groups of three: 40 vector instructions) under the NEXT
// block's MFMAs, the pair stored to the LDS ring, one workgroup barrier per chunk, random fp16 data.  Not in it: the W3 chunk's
// restaging (4 global loads + 4 LDS writes per lane and chunk: measured 0 % in the kernel) and the publishes.
// SHAPE 1 issues 64 MFMAs of 8 passes per wave and chunk where SHAPE 0 issues 32 of 16: the same matrix cycles, twice the
// matrix-instruction issue, in a loop that is vector-issue bound.
// Output per run (>= 2 s of back-to-back launches): wall time per tile and workgroup slot, the in-kernel clock (s_memtime over
// s_memrealtime, median over the workgroups of the last launch), cycles per tile.  Three runs per shape, alternating.
//   hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize tools/microbench/pn_loop_shape.hip -o pn_loop_shape
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int STAGE = 64 * 256;                            // one W3 chunk: 64 channels x 128 k fp16
constexpr int OFF_RING = 2 * STAGE;                        // [4 chunks][16 groups][2][64] fp32
constexpr int SLOT = 16 * 2 * 64;
constexpr int LDS_BYTES = 76672;                           // the trunk kernel's F_LDS: two workgroups per CU
constexpr float NEG_BIG = -3.0e38f;

__device__ __forceinline__ float max_nc(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, 3.0e38f); }
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}
__device__ __forceinline__ f16x8 w3_frag(const char* stage, int row, int chunk) {
    return *reinterpret_cast<const f16x8*>(stage + row * 256 + 16 * (chunk ^ (row & 15)));
}
// the kernel's F_CHAIN_BLOCK: id | ring tag into the low mantissa bits (one v_and_or_b32 per score, the id a scalar), the two largest
// of sixteen in groups of three
__device__ __forceinline__ void chain16(const float (&s)[16], unsigned id_mask, const unsigned* ctag, float& m1, float& m2) {
    float x[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = __uint_as_float((__float_as_uint(s[e]) & id_mask) | ctag[e]);
    m1 = fmaxf(fmaxf(x[0], x[1]), x[2]);
    m2 = __builtin_amdgcn_fmed3f(x[0], x[1], x[2]);
#pragma unroll
    for (int g = 3; g < 15; g += 3) {
        const float g1 = fmaxf(fmaxf(x[g], x[g + 1]), x[g + 2]);
        const float g2 = max_nc(m2, __builtin_amdgcn_fmed3f(x[g], x[g + 1], x[g + 2]));
        m2 = __builtin_amdgcn_fmed3f(m1, g1, g2);
        m1 = max_nc(m1, g1);
    }
    m2 = __builtin_amdgcn_fmed3f(m1, m2, x[15]);
    m1 = max_nc(m1, x[15]);
}

template <int SHAPE>
__global__ __launch_bounds__(256, 2) void k(const _Float16* __restrict__ a_g, const _Float16* __restrict__ w_g, float* __restrict__ out,
                                            unsigned long long* __restrict__ clk, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char fl[];
    float* ring = reinterpret_cast<float*>(fl + OFF_RING);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 2 * STAGE / 16; i += 256) reinterpret_cast<uint4*>(fl)[i] = reinterpret_cast<const uint4*>(w_g)[i];
    f16x8 a3[16];                                          // 64 points x K = 128 of the wave: 64 registers in both shapes
#pragma unroll
    for (int i = 0; i < 16; ++i) a3[i] = *reinterpret_cast<const f16x8*>(a_g + ((long)(blockIdx.x & 63) * 256 + tid) * 128 + 8 * i);
    unsigned id_mask = ~127u;
    asm volatile("" : "+v"(id_mask));
    float acc_sum = 0.f;
    lds_barrier();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    if constexpr (SHAPE == 0) {
        const int r = lane & 31, h = lane >> 5;
        f32x16 accP;
#pragma unroll
        for (int e = 0; e < 16; ++e) accP[e] = 0.f;
#pragma unroll 1
        for (int c = 0; c < 16 * tiles; c += 2) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                unsigned ctag[32];
#pragma unroll
                for (int e = 0; e < 32; ++e) asm("s_or_b32 %0, %1, %2" : "=s"(ctag[e]) : "s"((unsigned)(((c >> 2) & 3) << 5)), "i"(e));
                const unsigned *ct0 = ctag, *ct1 = ctag + 16;
                lds_barrier();
                const char* st = fl + u * STAGE;
                float* slot = ring + ((c >> 0) & 2) * SLOT + u * SLOT;   // ring slot (c + u) & 3
                f16x8 wf0[8], wf1[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) wf0[s] = w3_frag(st, r, 2 * s + h);
#pragma unroll
                for (int s = 0; s < 8; ++s) wf1[s] = w3_frag(st, 32 + r, 2 * s + h);
                f32x16 accA, accB;
                float m1, m2;
#define MFMA_BLOCK(ACC, PB, WF)                                                                                \
    do {                                                                                                       \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) ACC[e] = 0.f;                                           \
        _Pragma("unroll") for (int s = 0; s < 8; ++s)                                                          \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(a3[8 * (PB) + s], WF[s], ACC, 0, 0, 0);               \
    } while (0)
#define CHAIN_BLOCK(ACC, CT, JN, PB)                                                                           \
    do {                                                                                                       \
        float s_[16];                                                                                          \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) s_[e] = ACC[e];                                         \
        chain16(s_, id_mask, CT, m1, m2);                                                                      \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                        \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);                                                 \
        }                                                                                                      \
        float* dst = slot + ((wave * 2 + (PB)) * 2 + h) * 128 + 32 * (JN) + r;                                 \
        dst[0] = m1;                                                                                           \
        dst[64] = m2;                                                                                          \
    } while (0)
                MFMA_BLOCK(accA, 0, wf0);
                CHAIN_BLOCK(accP, ct1, 1, 1);              // the previous chunk's last block (its slot: this one's -- a skeleton)
                MFMA_BLOCK(accB, 1, wf0);
                CHAIN_BLOCK(accA, ct0, 0, 0);
                MFMA_BLOCK(accA, 0, wf1);
                CHAIN_BLOCK(accB, ct1, 0, 1);
                MFMA_BLOCK(accP, 1, wf1);
                CHAIN_BLOCK(accA, ct0, 1, 0);
#undef MFMA_BLOCK
#undef CHAIN_BLOCK
            }
        }
        acc_sum = accP[0] + accP[15];
    } else {
        // lane: channel lane & 15 of a column block, the points 16 rb + 4 (lane >> 4) + e of the four row blocks; A fragment of row
        // block rb and k-step ks: a3[4 rb + ks] (row lane & 15, k chunk lane >> 4)
        const int l16 = lane & 15, q = lane >> 4;
        f32x4 accP[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) accP[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int c = 0; c < 16 * tiles; c += 2) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                unsigned ctag[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) asm("s_or_b32 %0, %1, %2" : "=s"(ctag[e]) : "s"((unsigned)(((c >> 2) & 3) << 5)), "i"(e));
                lds_barrier();
                const char* st = fl + u * STAGE;
                float* slot = ring + ((c >> 0) & 2) * SLOT + u * SLOT;
                f16x8 wf[4][4];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) wf[cb][ks] = w3_frag(st, 16 * cb + l16, 4 * ks + q);
                f32x4 accA[4], accB[4];
                float m1, m2;
#define MFMA_BLOCK(ACC, CB)                                                                                    \
    do {                                                                                                       \
        _Pragma("unroll") for (int rb = 0; rb < 4; ++rb) ACC[rb] = f32x4{0.f, 0.f, 0.f, 0.f};                  \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                       \
            _Pragma("unroll") for (int rb = 0; rb < 4; ++rb)                                                   \
                ACC[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a3[4 * rb + ks], wf[CB][ks], ACC[rb], 0, 0, 0); \
    } while (0)
#define CHAIN_BLOCK(ACC, CB)                                                                                   \
    do {                                                                                                       \
        float s_[16];                                                                                          \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) s_[e] = ACC[e >> 2][e & 3];                             \
        chain16(s_, id_mask, ctag, m1, m2);                                                                    \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) {   /* 16 MFMAs of half the length: one per 2.5 chain instructions */ \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                                 \
        }                                                                                                      \
        float* dst = slot + (wave * 4 + q) * 128 + 16 * (CB) + l16;                                            \
        dst[0] = m1;                                                                                           \
        dst[64] = m2;                                                                                          \
    } while (0)
                MFMA_BLOCK(accA, 0);
                CHAIN_BLOCK(accP, 3);
                MFMA_BLOCK(accB, 1);
                CHAIN_BLOCK(accA, 0);
                MFMA_BLOCK(accA, 2);
                CHAIN_BLOCK(accB, 1);
                MFMA_BLOCK(accP, 3);
                CHAIN_BLOCK(accA, 2);
#undef MFMA_BLOCK
#undef CHAIN_BLOCK
            }
        }
        acc_sum = accP[0][0] + accP[3][3];
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    lds_barrier();
    if (tid == 0) { clk[2 * blockIdx.x] = t1 - t0; clk[2 * blockIdx.x + 1] = r1 - r0; }
    float s = acc_sum;
    for (int i = 0; i < 4 * SLOT / 256; ++i) s += ring[i * 256 + tid];
    out[(long)blockIdx.x * 256 + tid] = s;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

struct Result { double us_per_tile, mhz, cyc_per_tile; };
template <int SHAPE>
Result run(const _Float16* a, const _Float16* w, float* out, unsigned long long* clk, int grid, int tiles, double seconds) {
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k<SHAPE>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL((k<SHAPE>), dim3(grid), dim3(256), LDS_BYTES, 0, a, w, out, clk, tiles);
    CK(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    long launches = 0;
    double el = 0.0;
    do {                                                   // batches of eight launches back to back until the time is up
        for (int i = 0; i < 8; ++i) hipLaunchKernelGGL((k<SHAPE>), dim3(grid), dim3(256), LDS_BYTES, 0, a, w, out, clk, tiles);
        launches += 8;
        CK(hipDeviceSynchronize());
        el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (el < seconds);
    std::vector<unsigned long long> h(2 * grid);
    CK(hipMemcpy(h.data(), clk, h.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> mhz(grid), cyc(grid);
    for (int i = 0; i < grid; ++i) { mhz[i] = 100.0 * (double)h[2 * i] / (double)(h[2 * i + 1] + 1); cyc[i] = (double)h[2 * i] / tiles; }
    std::sort(mhz.begin(), mhz.end());
    std::sort(cyc.begin(), cyc.end());
    return {el * 1e6 / ((double)launches * tiles), mhz[grid / 2], cyc[grid / 2]};
}

int main(int argc, char** argv) {
    const double seconds = argc > 1 ? atof(argv[1]) : 2.0;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = 2 * prop.multiProcessorCount, tiles = 128;
    const size_t na = 64L * 256 * 128, nw = 2L * 64 * 128;
    std::vector<_Float16> ha(na), hw(nw);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xFFFF) / 32768.0f - 1.0f; };
    for (auto& v : ha) v = (_Float16)(rnd() * 4.0f);
    for (auto& v : hw) v = (_Float16)rnd();
    _Float16 *a, *w; float* out; unsigned long long* clk;
    CK(hipMalloc(&a, na * 2)); CK(hipMalloc(&w, nw * 2)); CK(hipMalloc(&out, (size_t)grid * 256 * 4)); CK(hipMalloc(&clk, (size_t)grid * 16));
    CK(hipMemcpy(a, ha.data(), na * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(w, hw.data(), nw * 2, hipMemcpyHostToDevice));
    printf("%s, %d workgroups of 256 (two per CU), %d tiles of 16 chunks per workgroup and launch, >= %.1f s per run\n", prop.gcnArchName, grid, tiles, seconds);
    for (int rep = 0; rep < 3; ++rep) {
        const Result r0 = run<0>(a, w, out, clk, grid, tiles, seconds);
        const Result r1 = run<1>(a, w, out, clk, grid, tiles, seconds);
        printf("pair %d  32x32x16: %8.3f us per tile, %6.0f MHz, %7.0f cycles per tile   16x16x32: %8.3f us per tile, %6.0f MHz, %7.0f cycles per tile   16x16x32 / 32x32x16 wall time: %.4f\n",
               rep, r0.us_per_tile, r0.mhz, r0.cyc_per_tile, r1.us_per_tile, r1.mhz, r1.cyc_per_tile, r1.us_per_tile / r0.us_per_tile);
        fflush(stdout);
    }
    return 0;
}
