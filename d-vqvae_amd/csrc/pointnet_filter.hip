// PointNet trunk, filtered: conv1 -> conv2 -> [conv3 -> max over the points] with conv3 evaluated TWICE at very different
// cost (PointNetEncoder.forward, network/pointnet_encoder.py:147-164; STN3d.forward :30-35):
//
//   1. pn_trunk_filter_kernel: conv1 (vector ALU) and conv2 (split-bf16, six matrix-core products, fp32-accurate) as in
//      pn_trunk_kernel; the fp32 h2 rows [point][128] go to HBM only with DVQ_PN_RECOMPUTE=0 (default: pn_exact_kernel recomputes
//      the rows it reads with the same device function, pn_conv12_block).  conv3 (94 % of the trunk's FLOPs) is then evaluated as ONE
//      fp16 product per term on CENTRED rows: d_p = h2_p - c (c = pn_center_kernel's mean of four rows of the sample; the
//      argmax over the points does not depend on it), d scaled by a per-wave power of two, W3 by a per-channel power of
//      two, both rounded to fp16.  Every lane keeps, per 16-channel column block (its 16 points of one channel: four per row block), the TWO largest
//      approximate scores with the id of their point in the low mantissa bits; per (sample, 256-point tile, channel) the kernel
//      emits the FIVE largest of those 32 values and one flag per 16-point group that may hold further points in range whose
//      ids were not kept.
//   2. pn_exact_kernel: per (sample, channel) the estimate of a point's score is  approx + exact_dot(w_n, c)  with
//      |estimate - exact_dot(w_n, h2_p)| <= E_t = |r_n| max_p |d_p| + |w_n| max_p |rd_p| + C_ID |w_n| max_p |d_p|
//      + 2 DELTA |w_n| max_p |h2_p|, maxima over the tile; r_n = w_n - fp16 image (norm measured by the packer), rd_p =
//      d_p - fp16 image (norm measured by the trunk kernel), C_ID: id bits + matrix-core accumulation, DELTA: rounding of
//      one exact_dot; pn_exact_kernel adds a floor for the id bits of a score that is zero (E_ID_FLOOR, bound_of).  Every tracked
//      point whose upper bound reaches the best lower bound is re-evaluated in fp32 (exact_dot: a fixed-order fp32 FMA dot
//      of W3[n,:] and the stored h2 row) and the maximum of THOSE values + bias is the feature -- bit-identical to the
//      maximum of exact_dot over ALL points (tests: DVQ_PN_EXHAUSTIVE=1 evaluates exactly that).  The 16 points of a flagged
//      group are all evaluated.
//
// Matrix-core cost per (32 points x 32 channels x K=128): 16 x v_mfma_f32_16x16x32_f16 (the matrix cycles of eight 32x32x16: the
// chip holds a higher clock on the small shape, tools/microbench/pn_loop_shape.hip) instead of 48 bf16 MFMAs; the
// kernel is bound by vector-instruction issue: 2.5 instructions per score (id; max3 / med3 per group of three) since round 6 -- a top-two per 16-point
// group flags about as many points for re-evaluation as the top-three per 32 points of round 4 did.
#include "dvq_internal.h"
#include "pn_filter.h"
#include <vector>

namespace {

typedef __bf16 qbf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 qf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 qf16x2 __attribute__((ext_vector_type(2)));
typedef float qf32x2 __attribute__((ext_vector_type(2)));

// beyond the two measured rounding residuals, relative to |w| max|d|: the 8 id bits 2^-15 (3.05e-5); the matrix core's fp32
// accumulation of the 128 exact products -- at most 128 additions of 2^-23 each even if they truncated (1.53e-5; round to
// nearest: half of that); the product of the two residuals (2^-22); rounded up.  Nothing in it depends on the ORDER in which the
// instruction sums its products: the same constant held for v_mfma_f32_32x32x16_f16 (8 steps of 16) and holds for 16x16x32 (4 of 32)
constexpr float C_ID = 5.0e-5f;
// |exact_dot(w, h) - w.h| <= DELTA |w| |h|: 8 chained FMAs + 4 butterfly adds = 12 roundings (7.2e-7), + the fp32 add of
// the centre term
constexpr float DELTA = 1.0e-6f;
constexpr float NEG_BIG = -3.0e38f;
// the id and tag bits of a score that is zero or denormal: 2 x 2^-141 in scaled units, doubled for the rounding of a denormal product
// (bound_of in pn_exact_kernel)
constexpr float E_ID_FLOOR = 0x1p-139f;

constexpr int F_STAGE2 = 2 * 64 * 128;                    // conv2: one half of W2's two fp16 planes (2 x 64 rows x 128 B)
// the filter image of a trunk (dvq_pointnet_pack_filter): conv3 [1024][128] fp16 | 1 / scale [1024] | |w_n| [1024] | |w_n - image| [1024]
// | conv2 as two fp16 planes [2][128][64] of w * 2^t_n (the second: the remainder * 2^11) | 2^-t_n [128]
constexpr int IMG_OFF_TI = 1024 * 256, IMG_OFF_WN = IMG_OFF_TI + 4096, IMG_OFF_RN = IMG_OFF_WN + 4096;
constexpr int IMG_OFF_W2 = IMG_OFF_RN + 4096, IMG_OFF_K2 = IMG_OFF_W2 + 2 * 128 * 128, IMG_BYTES = IMG_OFF_K2 + 512;
constexpr int F_STAGE3 = 64 * 256;                        // conv3: 64 channels x 128 k fp16
constexpr int F_OFF_TB = 2 * F_STAGE3;                    // conv3 phase: record ring [4 chunks][4 waves][4 lane quarters][2][64] fp32 (32 KiB) behind the two W3 stages
constexpr int F_SLOT = 4 * 2 * 2 * 2 * 64;                // floats per chunk slot of the ring
constexpr int F_OFF_W1 = F_OFF_TB + 8 * 4 * 4 * 64 * 4;   // [64][4] fp32
constexpr int F_OFF_B1 = F_OFF_W1 + 64 * 4 * 4;           // [64]
constexpr int F_OFF_B2 = F_OFF_B1 + 64 * 4;               // [128]
constexpr int F_OFF_K2 = F_OFF_B2 + 128 * 4;              // [128] 2^-t_n of conv2's weight rows
constexpr int F_OFF_SC = F_OFF_K2 + 128 * 4;              // [4] 1 / (wave scale)
constexpr int F_OFF_TI = F_OFF_SC + 64;                   // [1024] 1 / (channel scale)
constexpr int F_OFF_CS = F_OFF_TI + 4096;                 // [128] centre of the sample
constexpr int F_OFF_WS = F_OFF_CS + 512;                  // [3][4] per-wave |h|max, |d|max, |rd|max
constexpr int F_OFF_E2 = F_OFF_WS + 64;                   // [1024] 2 E of the tile per channel ([4][1024] in the tail kernel: a tile per wave)
constexpr int F_LDS = F_OFF_E2 + 4096;                    // 76 672 B -> 2 workgroups per CU
constexpr int F_LDS_TAIL = F_LDS + 3 * 4096 + 4 * 512;    // tail kernel: three more e2 tables, one centre per wave (its own sample) behind them
static_assert(F_OFF_W1 >= 2 * F_STAGE2, "the conv3 stages and the triple buffer cover the W2 region");

__device__ __forceinline__ float max_nc(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, 3.0e38f); }
__device__ __forceinline__ float min_nc(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, NEG_BIG); }

// Eight values x and a power of two s -> the two fp16 pieces of the three-product split of x s (csrc/gemm_f16x2.hip's, the second
// piece NOT scaled by 2^11 here): p1 = fp16(x s), p2 = fp16(x s - p1), each ONE rounding of an exact fma (v_fma_mixlo / mixhi_f16) --
// two vector instructions per value, no separate scaling or conversion.  (|p2| <= 2^-11 |p1|: with the point's largest activation in
// [2^14, 2^15) a second piece below fp16's normal range belongs to an activation 2^-17 of the largest; what is lost there is 2^-40 of it.)
__device__ __forceinline__ void q_split2(const float (&v)[8], float s, qf16x8& p1, qf16x8& p2) {
    unsigned hb[4], lb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a0 = v[2 * j], a1 = v[2 * j + 1];
        asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "=v"(hb[j]) : "v"(a0), "v"(s));
        asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "+v"(hb[j]) : "v"(a1), "v"(s));
        asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(lb[j]) : "v"(a0), "v"(s), "v"(hb[j]));
        asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lb[j]) : "v"(a1), "v"(s), "v"(hb[j]));
    }
    p1 = __builtin_bit_cast(qf16x8, uint4{hb[0], hb[1], hb[2], hb[3]});
    p2 = __builtin_bit_cast(qf16x8, uint4{lb[0], lb[1], lb[2], lb[3]});
}

// W2 planes [2][128][64] fp16: rows of 128 B, chunk c of row r lands at c ^ ((r >> 1) & 7); one half = 64 rows of both planes =
// sixteen 1 KiB DMA pieces, four per wave
__device__ __forceinline__ void w2_issue(const uint16_t* __restrict__ planes, int row0, char* stage, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = wave * 4 + i;
        const int pl = id >> 3, rb = id & 7;
        const int row = rb * 8 + (lane >> 3);
        const uint16_t* src = planes + pl * (128L * 64) + (long)(row0 + row) * 64 + 8 * ((lane & 7) ^ ((row >> 1) & 7));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(stage + (pl * 64 + rb * 8) * 128), 16, 0, 0);
    }
}
__device__ __forceinline__ qf16x8 w2_frag(const char* stage, int pl, int row, int chunk) {
    return *reinterpret_cast<const qf16x8*>(stage + (pl * 64 + row) * 128 + 16 * (chunk ^ ((row >> 1) & 7)));
}

// W3 filter image: [1024][128] fp16, rows of 256 B = 16 chunks; in LDS chunk c of row r sits at chunk c ^ (r & 15).
// One 64-channel chunk = 16 KiB: every lane moves 4 x 16 B through registers (global loads at the top of a chunk, LDS writes
// at its end -- an LDS-DMA piece costs the issuing wave ~150 cycles, a load + a write a few).
struct W3Regs { uint4 a, b, c, d; };
__device__ __forceinline__ const uint4* w3_src(const char* __restrict__ w3h, int ch0, int wave, int lane, int i) {
    // uniform 64-bit base + 32-bit lane offset: the load takes the base from scalar registers (no 64-bit vector add per load)
    const char* base = w3h + (long)(ch0 + (wave * 4 + i) * 4) * 256;
    const unsigned off = (unsigned)(lane >> 4) * 256u + 16u * (unsigned)(lane & 15);
    return reinterpret_cast<const uint4*>(base + off);
}
__device__ __forceinline__ W3Regs w3_load(const char* __restrict__ w3h, int ch0, int wave, int lane) {
    W3Regs v;
    v.a = *w3_src(w3h, ch0, wave, lane, 0);
    v.b = *w3_src(w3h, ch0, wave, lane, 1);
    v.c = *w3_src(w3h, ch0, wave, lane, 2);
    v.d = *w3_src(w3h, ch0, wave, lane, 3);
    return v;
}
__device__ __forceinline__ uint4* w3_dst(char* stage, int wave, int lane, int i) {
    const int row = (wave * 4 + i) * 4 + (lane >> 4);
    return reinterpret_cast<uint4*>(stage + row * 256 + 16 * ((lane & 15) ^ (row & 15)));
}
__device__ __forceinline__ void w3_store(char* stage, int wave, int lane, const W3Regs& v) {
    *w3_dst(stage, wave, lane, 0) = v.a;
    *w3_dst(stage, wave, lane, 1) = v.b;
    *w3_dst(stage, wave, lane, 2) = v.c;
    *w3_dst(stage, wave, lane, 3) = v.d;
}
__device__ __forceinline__ qf16x8 w3_frag(const char* stage, int row, int chunk) {
    return *reinterpret_cast<const qf16x8*>(stage + row * 256 + 16 * (chunk ^ (row & 15)));
}

// top three of the union of two descending triples
__device__ __forceinline__ void merge3(float& a1, float& a2, float& a3, float b1, float b2, float b3) {
    const float x = min_nc(a1, b1), y = max_nc(a2, b2), z = min_nc(a2, b2), w = max_nc(a3, b3);
    a1 = max_nc(a1, b1);
    a2 = max_nc(x, y);
    a3 = max_nc(min_nc(x, y), max_nc(z, w));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// (point_of_slot, slot_of_id and the groups of a tile: csrc/pn_slots.h)

// Wave reductions without ds_bpermute (__shfl_xor: an LDS-crossbar instruction, an lgkmcnt wait and an address register per pattern):
// lanes l and l ^ 32 through v_permlane32_swap, rows through DPP, the four rows through v_readlane.
__device__ __forceinline__ float g_half_sum(float v) {    // v[l] + v[l ^ 32], in every lane
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float g_half_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
template <int CTRL>
__device__ __forceinline__ float g_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float g_wave_max(float v) {    // uniform result
    v = fmaxf(v, g_dpp<0xB1>(v));
    v = fmaxf(v, g_dpp<0x4E>(v));
    v = fmaxf(v, g_dpp<0x141>(v));
    v = fmaxf(v, g_dpp<0x140>(v));                         // every lane: the maximum of its row of 16
    v = g_half_max(v);                                     // rows 0 | 2, 1 | 3
    return fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16)));
}
__device__ __forceinline__ float g_wave_sum(float v) {    // uniform result
    v += g_dpp<0xB1>(v);
    v += g_dpp<0x4E>(v);
    v += g_dpp<0x141>(v);
    v += g_dpp<0x140>(v);
    v = g_half_sum(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
}
// One point of a cloud as conv1 sees it: pc [C][N] of the sample at ``src`` (= its point's first coordinate), xyz @ trans (t: [9] or
// null) in front (pointnet_encoder.py:146).  The trunk kernel and pn_exact_kernel's recompute both read their points through here.
template <int C>
__device__ __forceinline__ void pn_point_in(const float* __restrict__ src, int N, const float* __restrict__ t, float (&x)[4]) {
    float x0 = src[0], x1 = src[N], x2 = src[2L * N];
    const float x3 = (C > 3) ? src[3L * N] : 0.f;
    if (t) {
        const float n0 = fmaf(x2, t[6], fmaf(x1, t[3], x0 * t[0]));
        const float n1 = fmaf(x2, t[7], fmaf(x1, t[4], x0 * t[1]));
        const float n2 = fmaf(x2, t[8], fmaf(x1, t[5], x0 * t[2]));
        x0 = n0; x1 = n1; x2 = n2;
    }
    x[0] = x0; x[1] = x1; x[2] = x2; x[3] = x3;
}

// THE definition of a conv2 row: conv1 + conv2 of one 32-point block of a wave (lanes l and l + 32 work on point l & 31: lane half
// h holds rows k = 16 s + 8 h + j of conv1's 64 activations).  conv1: the FMAs in their order; conv2 on the fp16 three-product split
// of csrc/gemm_f16x2.hip: weights as two fp16 planes of w * 2^t_n (per output row), the activations of a point as two fp16 pieces of
// h1 * s_p with s_p a power of two that puts the POINT's largest activation in [2^14, 2^15) -- a function of the point alone, so a
// row's bits do not depend on which points share its wave (tail tile == full tile, batched == single, recomputed == spilled);
// acc = a1 w2 + a2 w1 + a1 w1 in ONE fp32 accumulator per 32 channels (second pieces unscaled; the eight small products first, the
// four large ones after), h2 = relu(acc / s_p 2^-t_n + b2).  Parameterised only by where its operands live: w1 [64][4], b1 [64],
// k2 [128] (2^-t_n), b2 [128] in the LDS (trunk) or in global memory (exact stage); frag(t4, plane, s) = the W2 fragment of channel
// row 32 t4 + (l & 31), k chunk 2 s + h -- from the trunk's LDS stages or from the filter image.  emit(t4, o): the lane's sixteen
// channels 32 t4 + (e & 3) + 8 (e >> 2) + 4 h of its point.  The instruction shape and the k-to-lane assignment define the bits.
// Two halves: pn_conv1_split (conv1 -> the point's two fp16 pieces and 1 / s_p) and pn_conv2_block (32 channels); pn_conv12_block is
// both for all 128 channels, written out (the trunk kernel); pn_exact_kernel keeps the loop over the channel blocks rolled.
template <int C>
__device__ __forceinline__ void pn_conv1_split(const float (&xin)[4], const float* w1s, const float* b1s, int h_op, qf16x8 (&h1a)[4], qf16x8 (&h1b)[4],
                                               float& r_p_out) {
    float v[4][8];
    float amax = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(w1s + 32 * h_op + 64 * s + 4 * j);   // row k = 16 s + 8 h + j
            float a = fmaf(xin[0], w[0], (b1s + 8 * h_op)[16 * s + j]);
            a = fmaf(xin[1], w[1], a);
            a = fmaf(xin[2], w[2], a);
            if constexpr (C > 3) a = fmaf(xin[3], w[3], a);
            v[s][j] = fmaxf(a, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 8; j += 2) amax = fmaxf(fmaxf(amax, v[s][j]), v[s][j + 1]);   // v_max3_f32 (a NaN is dropped here and reaches the products through the pieces)
    }
    amax = g_half_max(amax);                          // the lane halves hold the two halves of a point's 64 activations
    float s_p = 1.f, r_p = 1.f;
    {
        const int ex = (int)((__float_as_uint(amax) >> 23) & 255u);              // amax in [2^(ex-127), 2^(ex-126))
        if (ex > 20 && ex < 235) {
            s_p = __uint_as_float((unsigned)(127 + 15 - (ex - 126)) << 23);
            r_p = __uint_as_float((unsigned)(127 - 15 + (ex - 126)) << 23);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) q_split2(v[s], s_p, h1a[s], h1b[s]);
    r_p_out = r_p;
}
template <class Frag, class Emit>
__device__ __forceinline__ void pn_conv2_block(const qf16x8 (&h1a)[4], const qf16x8 (&h1b)[4], float r_p, int t4, const float* k2s, const float* b2s,
                                               int h_op, Frag frag, Emit emit) {
    {
        // ONE fp32 accumulator: the eight small products (a1 w2, a2 w1: 2^-11 of the large ones) first, the four large ones after
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        qf16x8 w1f[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            w1f[s] = frag(t4, 0, s);
            const qf16x8 w2f = frag(t4, 1, s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2f, h1a[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1f[s], h1b[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1f[s], h1a[s], acc, 0, 0, 0);
        float o[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ch = 32 * t4 + (e & 3) + 8 * (e >> 2);       // + 4 h
            o[e] = fmaxf(fmaf(acc[e] * r_p, (k2s + 4 * h_op)[ch], (b2s + 4 * h_op)[ch]), 0.f);
        }
        emit(t4, o);
    }
}
template <int C, class Frag, class Emit>
__device__ __forceinline__ void pn_conv12_block(const float (&xin)[4], const float* w1s, const float* b1s, const float* k2s, const float* b2s,
                                                int h_op, Frag frag, Emit emit) {
    qf16x8 h1a[4], h1b[4];
    float r_p;
    pn_conv1_split<C>(xin, w1s, b1s, h_op, h1a, h1b, r_p);
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) pn_conv2_block(h1a, h1b, r_p, t4, k2s, b2s, h_op, frag, emit);
}
// the lane's sixteen channels of block t4 to its row (dst = row + 32 t4 + 4 h): natural channel order, 4 consecutive channels per 16-byte store
__device__ __forceinline__ void pn_store_row16(float* dst, const float (&o)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(dst + 8 * g) = f32x4{o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
}

// TAIL = false: one workgroup per (sample, dealt tile), blockIdx.x = sample * deal + tile (no workgroup for a tail tile: launched
// and left at once they would all sit on two of the eight XCDs -- blockIdx % 4 == 3 -- and idle a quarter of the chip).  TAIL = true: the tail tiles of FOUR samples per workgroup, one per wave (one 32-point block each;
// the staged W2 / W3 images are shared, everything per sample is per wave: centre, scales, records).
template <int C, bool TAIL>
__global__ __launch_bounds__(256, 2) void pn_trunk_filter_kernel(const float* __restrict__ pc, const float* __restrict__ trans,
                                                                 int N, int Npad, int tiles, int deal, long B, const float* __restrict__ W1,
                                                                 const float* __restrict__ b1,
                                                                 const float* __restrict__ b2, const char* __restrict__ w3f,
                                                                 float* __restrict__ h2buf, f32x4* __restrict__ part, qf32x2* __restrict__ part2,
                                                                 unsigned* __restrict__ tstat, const float* __restrict__ cbuf,
                                                                 int abl_arg /* timing diagnostics only (DVQ_PN_ABL, -DDVQ_DIAG builds) */) {
    const int abl = DVQ_DIAG_ON ? abl_arg : 0;
    extern __shared__ __attribute__((aligned(16))) char fl[];
    float* tb = reinterpret_cast<float*>(fl + F_OFF_TB);
    float* w1s = reinterpret_cast<float*>(fl + F_OFF_W1);
    float* b1s = reinterpret_cast<float*>(fl + F_OFF_B1);
    float* b2s = reinterpret_cast<float*>(fl + F_OFF_B2);
    float* scs = reinterpret_cast<float*>(fl + F_OFF_SC);
    float* tis = reinterpret_cast<float*>(fl + F_OFF_TI);
    float* wst = reinterpret_cast<float*>(fl + F_OFF_WS);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    // The lane half enters the LDS addresses of the small tables through an opaque copy: knowing h in {0, 1}, the compiler turns
    // "base + 32 h + constant" into "(base | 32 h) | constant", cannot fold the constant into the instruction's offset field any more
    // and keeps one address REGISTER per constant -- 32 of them for conv1's weights alone, live across both point blocks.
    int h_op = h;
    asm("" : "+v"(h_op));
    constexpr int NPB = TAIL ? 1 : 2;                       // 32-point blocks per wave
    const long b_raw = TAIL ? (long)blockIdx.x * 4 + wave : (long)(blockIdx.x / deal);
    const bool live = !TAIL || b_raw < B;                  // tail: the last workgroup's surplus waves work on sample B - 1, store nothing
    const long b = live ? b_raw : B - 1;
    const int tile = TAIL ? deal : (int)(blockIdx.x % deal);
    const long rec = b * tiles + tile;                     // (sample, tile) record
    float* cs = reinterpret_cast<float*>(fl + (TAIL ? F_LDS + 3 * 4096 + 512 * wave : F_OFF_CS));
    float* e2s = reinterpret_cast<float*>(fl + F_OFF_E2) + (TAIL ? 1024 * wave : 0);

    const unsigned long long t_start = (abl & PN_ABL_STAMPS) ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long r_start = (abl & PN_ABL_CLOCK) ? __builtin_amdgcn_s_memrealtime() : 0ull;   // 100 MHz: with 4096 | 8192 the record's word 3 holds the CLOCK
    unsigned long long t_a = 0, t_b = 0, t_c = 0;
    const uint16_t* w2pl = reinterpret_cast<const uint16_t*>(w3f + IMG_OFF_W2);
    w2_issue(w2pl, 0, fl, wave, lane);
    w2_issue(w2pl, 64, fl + F_STAGE2, wave, lane);
    float* k2s = reinterpret_cast<float*>(fl + F_OFF_K2);
    if (tid < 128) k2s[tid] = reinterpret_cast<const float*>(w3f + IMG_OFF_K2)[tid];
    w1s[tid] = W1[tid];
    if (tid < 64) b1s[tid] = b1[tid];
    if (tid < 128) b2s[tid] = b2[tid];
    *reinterpret_cast<f32x4*>(tis + 4 * tid) = *reinterpret_cast<const f32x4*>(w3f + IMG_OFF_TI + 16 * tid);
    if (TAIL) { cs[lane] = cbuf[b * 128 + lane]; cs[64 + lane] = cbuf[b * 128 + 64 + lane]; }
    else if (tid < 128) cs[tid] = cbuf[b * 128 + tid];

    float xin[NPB][4];
    int pidx[NPB];
    bool badpt = false;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
        int p = point_of_slot(tile, TAIL ? r : wave * 64 + pb * 32 + r, deal);
        pidx[pb] = p;
        if (p >= N) p %= N;                               // padding slots repeat real points cyclically (a max ignores repeats; a point
                                                          // repeated once costs nothing: both copies carry ids that map back to it)
        pn_point_in<C>(pc + b * (long)C * N + p, N, trans ? trans + b * 9 : nullptr, xin[pb]);
        const float x0 = xin[pb][0], x1 = xin[pb][1], x2 = xin[pb][2], x3 = xin[pb][3];
        // a non-finite coordinate (after the transform): the reference's features of such a cloud are NaN in every channel -- affine
        // layers and torch.max propagate it.  ReLU as fmaxf(x, 0) squashes it here, and the cloud would go on as a DEGENERATE one
        // (all its points tie: every group flagged, every channel evaluated over all points by one workgroup -- the straggler of its
        // launch).  The tile says so instead (word 3 of its maxima) and pn_exact_kernel writes the NaNs.
        badpt = badpt || !(fabsf(x0) < 3.0e38f) || !(fabsf(x1) < 3.0e38f) || !(fabsf(x2) < 3.0e38f) || !(fabsf(x3) < 3.0e38f);
    }
    dvq_dma_barrier();                                    // W1/b1/b2 visible, W2 planes landed
    // The same wait once more in a form the compiler's counter model sees (vmcnt(0), the other counters untouched).  Without it the
    // FIRST use of the second point block's coordinates -- loaded above, consumed after the first block's sixteen h2 stores -- gets an
    // "s_waitcnt vmcnt(3)": the stores sit in a branch (padding slots store nothing), the compiler takes the smaller count of the two
    // paths, and the wave waits for thirteen of its sixteen stores to be ACKNOWLEDGED before it goes on (round 5: -11 % of the kernel
    // with the stores ablated, all of it this wait).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (abl & PN_ABL_STAMPS) t_a = __builtin_amdgcn_s_memtime();
    float cnorm;                                          // |c| (every wave for itself: no ordering between the waves needed)
    {
        const float cq = fmaf(cs[lane], cs[lane], cs[64 + lane] * cs[64 + lane]);
        cnorm = sqrtf(g_wave_sum(cq)) * 1.0001f;
    }

    // ---- conv1 + conv2 (pn_conv12_block, W2 from the LDS stages), h2 = relu(conv2 + b2) kept in fp32: hv[pb][16 t4 + e]
    float hv[NPB][64];
    if (abl & PN_ABL_CONSUMER) {                                    // timing only: a "consumer" workgroup -- no conv1 / conv2, rows from thin air
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int i = 0; i < 64; ++i) hv[pb][i] = xin[pb][i & 3] * (float)(i + 1);
    } else
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
        // (h2buf == nullptr, workgroup-uniform: the rows are not spilled -- pn_exact_kernel recomputes the ones it needs, DVQ_PN_RECOMPUTE)
        const bool spill = pidx[pb] < N && live && h2buf != nullptr && !(abl & PN_ABL_NO_H2_STORE);
        pn_conv12_block<C>(xin[pb], w1s, b1s, k2s, b2s, h_op,
                           [&](int t4, int pl, int s) { return w2_frag(fl + (t4 >> 1) * F_STAGE2, pl, 32 * (t4 & 1) + r, 2 * s + h); },
                           [&](int t4, const float (&o)[16]) {
#pragma unroll
                               for (int e = 0; e < 16; ++e) hv[pb][16 * t4 + e] = o[e];
                               if (spill) pn_store_row16(h2buf + ((b * Npad + pidx[pb]) * 128 + 32 * t4 + 4 * h), o);
                           });
    }
    if (abl & PN_ABL_STAMPS) t_b = __builtin_amdgcn_s_memtime();
    // ---- centre the rows on the sample's centre (pn_center_kernel)
    float dn2 = 0.f;
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cs + 4 * h_op + 32 * t4 + 8 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb) hv[pb][16 * t4 + 4 * g + i] -= c4[i];
            }
        }
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < 64; ++i) sq = fmaf(hv[pb][i], hv[pb][i], sq);
        sq = g_half_sum(sq);                              // the two lane halves hold the two halves of a point's channels
        dn2 = fmaxf(dn2, sq);
    }
    dn2 = g_wave_max(dn2);
    // per-wave power-of-two scale: (largest row norm) * s in [2^14, 2^15) -- every element is at most its row's norm
    float s_w = 1.f;
    const float dnorm = sqrtf(dn2) * 1.0001f;
    {
        const int ex = (int)((__float_as_uint(dnorm) >> 23) & 255u);             // dnorm in [2^(ex-127), 2^(ex-126))
        if (ex > 20 && ex < 235) s_w = __uint_as_float((unsigned)(127 + 15 - (ex - 126)) << 23);
    }
    // conv3's A operand, one fp16 plane: step = 2 t4 + q, k order inside a step as conv2's accumulator delivers it;
    // rn2 = largest squared norm of a row's rounding residual (scaled units)
    qf16x8 a3[NPB][8];
    float rn2 = 0.f;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
        float sq = 0.f;
        const float s_pb = s_w;
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            unsigned pk[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                // fp16(d s) and the rounding residual d s - fp16(d s), each one instruction on the exact product (s a power of two)
                const float d0 = hv[pb][8 * st + 2 * j2], d1 = hv[pb][8 * st + 2 * j2 + 1];
                asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "=v"(pk[j2]) : "v"(d0), "v"(s_pb));
                asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "+v"(pk[j2]) : "v"(d1), "v"(s_pb));
                float r0, r1;
                asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(r0) : "v"(d0), "v"(s_pb), "v"(pk[j2]));
                asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r1) : "v"(d1), "v"(s_pb), "v"(pk[j2]));
                sq = fmaf(r0, r0, sq);
                sq = fmaf(r1, r1, sq);
            }
            a3[pb][st] = __builtin_bit_cast(qf16x8, uint4{pk[0], pk[1], pk[2], pk[3]});
        }
        sq = g_half_sum(sq);
        rn2 = fmaxf(rn2, sq);
    }
    rn2 = g_wave_max(rn2);
    // conv3 runs on v_mfma_f32_16x16x32_f16: an A fragment wants lane (quarter q, row l) to hold 8 k of row l of ONE 16-point row
    // block, the four quarters four different k chunks.  Here lane rows {0, 2} (h = 0, 1) hold points 0 .. 15 of the point block and
    // rows {1, 3} points 16 .. 31, each 8 k per step st.  v_permlane16_swap_b32 exchanges the odd rows of its first operand with
    // the even rows of its second: applied to the steps (2 ks, 2 ks + 1) it leaves in a3[pb][2 ks + hb] the complete fragment of row
    // block 2 pb + hb and MFMA step ks -- quarter q with the k chunk of step 2 ks + (q & 1), lane half q >> 1, i.e. chunk
    // 4 ks + 2 (q & 1) + (q >> 1) of W3's image, which is how the loop reads its B fragments (the image keeps its order).
    // 16 swaps per point block, once per tile; the per-point reductions above ran on conv2's layout.
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 x = __builtin_bit_cast(uint4, a3[pb][2 * ks]), y = __builtin_bit_cast(uint4, a3[pb][2 * ks + 1]);
            unsigned* xp = reinterpret_cast<unsigned*>(&x);
            unsigned* yp = reinterpret_cast<unsigned*>(&y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const auto sw = __builtin_amdgcn_permlane16_swap(xp[j], yp[j], false, false);
                xp[j] = sw[0];
                yp[j] = sw[1];
            }
            a3[pb][2 * ks] = __builtin_bit_cast(qf16x8, x);
            a3[pb][2 * ks + 1] = __builtin_bit_cast(qf16x8, y);
        }
    const int l16 = lane & 15, q4 = lane >> 4;             // conv3: column (channel of a column block) and lane quarter
    // conv3's first W3 chunk: requested BEFORE the three atomics below -- the wait for these loads then leaves the atomics (younger,
    // in the in-order counter) pending instead of sitting out their round trip (600 .. 3 000 cycles each under load)
    const char* w3h = w3f;
    W3Regs wreg = w3_load(w3h, 0, wave, lane);
    const bool any_bad = __any(badpt);
    static_assert(F_SLOT == PN_GROUPS * 2 * 64, "ring slot: a pair of 64 channels per group");
    if (lane == 0) {              // per-tile maxima; non-negative floats (and NaN, above all of them) order as integers
        const float dmx = sqrtf(dn2), rdm = sqrtf(rn2) / s_w;
        const float hm = (dmx + cnorm) * 1.0001f;          // |h_p| <= |h_p - c| + |c|
        scs[wave] = 1.0f / s_w;
        wst[wave] = hm; wst[4 + wave] = dmx; wst[8 + wave] = rdm;
        if (live) {
            if (any_bad && !(abl & PN_ABL_STAMPS)) atomicMax(tstat + 4 * rec + 3, 1u);
            atomicMax(tstat + 4 * rec + 0, __float_as_uint(hm));
            atomicMax(tstat + 4 * rec + 1, __float_as_uint(dmx));
            atomicMax(tstat + 4 * rec + 2, __float_as_uint(rdm));
        }
    }
    dvq_lds_barrier();                                      // everybody is done with W2 in the stages; scs visible
    if (abl & PN_ABL_STAMPS) t_c = __builtin_amdgcn_s_memtime();

    // ---- conv3, filtered: 16 chunks of 64 channels, one fp16 product, top two scores per channel and 16-point group
    w3_store(fl, wave, lane, wreg);
    {
        // 2 E of this tile for every channel, once, into the LDS (the publishing waves used to fetch the two weight norms of their
        // channels from global memory at the top of every publish: an L2 round trip in front of four idle waves, four times)
        const float* wnorm_g = reinterpret_cast<const float*>(w3f + IMG_OFF_WN);
        const float* rnorm_g = reinterpret_cast<const float*>(w3f + IMG_OFF_RN);
        // the tile's maxima: over its four waves -- over the wave alone where every wave is a tile of its own (TAIL)
        const float hm = (TAIL ? wst[wave] : fmaxf(fmaxf(wst[0], wst[1]), fmaxf(wst[2], wst[3]))) * 1.00001f;
        const float dmx = (TAIL ? wst[4 + wave] : fmaxf(fmaxf(wst[4], wst[5]), fmaxf(wst[6], wst[7]))) * 1.00001f;
        const float rdm = (TAIL ? wst[8 + wave] : fmaxf(fmaxf(wst[8], wst[9]), fmaxf(wst[10], wst[11]))) * 1.00001f;
        constexpr int PER = TAIL ? 16 : 4;                 // channels per lane: a wave fills its own table (TAIL), the workgroup one
#pragma unroll
        for (int i = 0; i < PER; i += 4) {
            float wn[4], rn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = (TAIL ? lane : tid) + (TAIL ? 64 : 256) * (i + u);
                wn[u] = wnorm_g[n];
                rn[u] = rnorm_g[n];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = (TAIL ? lane : tid) + (TAIL ? 64 : 256) * (i + u);
                e2s[n] = 2.0f * fmaf(rn[u], dmx, fmaf(wn[u], rdm, fmaf(C_ID * wn[u], dmx, 2.0f * DELTA * wn[u] * hm)));
            }
        }
    }
    // Per channel of chunk c the publishing wave merges the sorted PAIRS of the sixteen 16-point groups (4 waves x 4 lane
    // quarters) into the tile's FIVE largest id-carrying scores (real units: three + the flags in a 16-byte record, the fourth and
    // fifth in an 8-byte one that pn_exact_kernel reads only where the third is in range) and one flag per group "may hold a point
    // within 2 E of the tile's largest score that is not among the five".  The ring holds four chunks: after chunks 3, 7, 11 and 15
    // every wave publishes one (all four busy at the same time: no wave waits for a publisher at the chunk barriers).
    auto publish = [&](int c) {
        const float* src = tb + (c & 3) * F_SLOT;          // [wave][lane quarter][k][channel]: every lane's own sorted pair, as finish() left it
        const float ti = tis[64 * c + lane];
        // all sixteen pairs first (one trip to the LDS), in real units, with the rest of their ids: bits [3:0] row block + register
        // (the chain's), [5:4] lane quarter, [7:6] wave (pn_slots.h)
        constexpr int NG = TAIL ? 4 : PN_GROUPS;           // groups: 4 w + quarter (TAIL: the publishing wave's four lane quarters, "wave 0")
        float t1[NG], t2[NG];
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int w = TAIL ? 0 : gi >> 2, qq = gi & 3;
            const int ws = TAIL ? wave : w;                // whose pairs (TAIL: one wave = the whole tile)
            const float* q = src + ((ws * 4 + qq) * 2) * 64 + ((lane + 16 * qq) & 63);   // finish()'s rotation
            t1[gi] = q[0];
            t2[gi] = q[64];
        }
        // Run-time check of the hand-over: finish() stamps bits [6:5] of what it stores with (chunk / 4) mod 4, so a value left in
        // this ring slot by an earlier chunk -- a store that did not happen or was not seen -- shows.  One stale input and the record
        // cannot be trusted: every group is flagged (pn_exact_kernel then evaluates the whole tile for this channel) and bit 16 says
        // why (counted: dvq_pointnet_fault_counters).  The pair of a group is ONE LDS store: checking its first value covers both.
        unsigned tagdiff = 0;
#pragma unroll
        for (int gi = 0; gi + 1 < NG; gi += 2)             // v_xor_b32 + v_or3_b32 per two groups
            tagdiff = tagdiff | (__float_as_uint(t1[gi]) ^ (unsigned)(((c >> 2) & 3) << 5)) | (__float_as_uint(t1[gi]) ^ __float_as_uint(t1[gi + 1]));
        const bool suspect = (tagdiff & 0x60u) != 0;
        unsigned tag_mask = ~0xF0u;
        asm volatile("" : "+v"(tag_mask));
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int w = TAIL ? 0 : gi >> 2, qq = gi & 3;
            const float sc = scs[TAIL ? wave : w] * ti;     // a power of two
            unsigned tag;                                   // pn_group_tag(w, qq) as a SCALAR and the mask in a vector register: one
            asm("s_mov_b32 %0, %1" : "=s"(tag) : "i"((w << 6) | (qq << 4)));   // v_and_or_b32 per value instead of v_and + v_or
            t1[gi] = __uint_as_float((__float_as_uint(t1[gi] * sc) & tag_mask) | tag);
            t2[gi] = __uint_as_float((__float_as_uint(t2[gi] * sc) & tag_mask) | tag);
        }
        const float e2 = e2s[64 * c + lane];               // 2 E of the tile for this channel (filled once, before the loop)
        float c1 = NEG_BIG, c2 = NEG_BIG, c3 = NEG_BIG, c4 = NEG_BIG, c5 = NEG_BIG;   // the tile's FIVE largest id-carrying scores
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            float x = t1[gi];
            c5 = __builtin_amdgcn_fmed3f(c4, c5, x); c4 = __builtin_amdgcn_fmed3f(c3, c4, x);
            c3 = __builtin_amdgcn_fmed3f(c2, c3, x); c2 = __builtin_amdgcn_fmed3f(c1, c2, x); c1 = max_nc(c1, x);
            x = t2[gi];                                    // <= t1[gi] <= c1: never the new largest
            c5 = __builtin_amdgcn_fmed3f(c4, c5, x); c4 = __builtin_amdgcn_fmed3f(c3, c4, x);
            c3 = __builtin_amdgcn_fmed3f(c2, c3, x); c2 = __builtin_amdgcn_fmed3f(c1, c2, x);
        }
        const float thr = c1 - e2;                         // NaN -> no flag here; pn_exact_kernel sees the non-finite bound
        // bit 4 w + quarter: that 16-point group may hold a point in range that is not among the five: its SECOND is in range (a
        // third could be: the lanes keep two), or its first is in range and was not kept (six in range in the tile).  With t1 >= t2
        // that is "u >= thr" for u = t1 if t1 was not kept (t1 < c5), else t2 -- no branches, no second trip to the LDS.
        unsigned flags = 0;
#pragma unroll
        for (int gi = NG - 1; gi >= 0; --gi) {
            const float u = t1[gi] < c5 ? t1[gi] : t2[gi];
            flags = flags + flags + (unsigned)(u >= thr);
        }
        if (suspect) flags = 0x1FFFFu;
        if ((abl & PN_ABL_INJECT_LIE) && c == 5 && lane == 7) c1 = fabsf(c1) * 1.0e3f + 1.0f;   // diagnostics: a record that lies about its tile
        if (live) {
            part[rec * 1024 + 64 * c + lane] = f32x4{c1, c2, c3, __uint_as_float(flags)};
            part2[rec * 1024 + 64 * c + lane] = qf32x2{c4, c5};
        }
    };
    // one column block of a chunk: 16 channels x the wave's NRB row blocks of 16 points, K = 128 in four steps of
    // v_mfma_f32_16x16x32_f16 (4 passes each: 16 MFMAs are the matrix cycles of eight 32x32x16) -- NRB accumulators of four registers;
    // the fragment of row block rb and step ks is a3[rb >> 1][2 ks + (rb & 1)] (see the swaps above).  The lane's 4 NRB scores
    // (ONE channel, rows 4 q + e of every row block) go through the top-two chain (2.5 vector instructions per score) while the
    // NEXT column block's MFMAs run: 16 MFMAs per 40 chain instructions
    constexpr int NRB = TAIL ? 2 : 4;                      // 16-point row blocks per wave
#define F_MFMA_BLOCK(ACC, WF)                                                                                  \
    do {                                                                                                       \
        _Pragma("unroll") for (int rb = 0; rb < NRB; ++rb) ACC[rb] = f32x4{0.f, 0.f, 0.f, 0.f};                \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                       \
            _Pragma("unroll") for (int rb = 0; rb < NRB; ++rb)                                                 \
                ACC[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a3[rb >> 1][2 * ks + (rb & 1)], WF[ks], ACC[rb], 0, 0, 0); \
    } while (0)
    /* CT: id (4 rb + e, pn_chain_id) | the ring tag of the chunk (bits [6:5], uniform): set HERE, with the id, by the one instruction */ \
    /* per score that is needed anyway -- finish() used to set the tag on the block's winner with an instruction of its own           */
#define F_CHAIN_BLOCK(ACC, M1, M2, CT)                                                                         \
    do {                                                                                                       \
        if (abl & PN_ABL_NO_CHAIN) { M1 = ACC[0][0]; M2 = ACC[NRB - 1][3]; } else   /* timing only: no chain */            \
        {                                                                                                      \
            /* round 6: groups of three -- v_max3 / v_med3 give a group's two largest, merged into the running pair by          */ \
            /* second = med3(M1, g1, max(M2, g2)): 40 instead of 48 instructions per 16 scores, the same pair                    */ \
            constexpr int NS_ = 4 * NRB;                                                                       \
            float x_[NS_];                                                                                     \
            _Pragma("unroll") for (int e = 0; e < NS_; ++e)                                                    \
                x_[e] = __uint_as_float((__float_as_uint(ACC[e >> 2][e & 3]) & id_mask) | (CT)[e]);           \
            M1 = fmaxf(fmaxf(x_[0], x_[1]), x_[2]);                                                            \
            M2 = __builtin_amdgcn_fmed3f(x_[0], x_[1], x_[2]);                                                 \
            _Pragma("unroll") for (int g = 3; g + 2 < NS_; g += 3) {                                           \
                const float g1_ = fmaxf(fmaxf(x_[g], x_[g + 1]), x_[g + 2]);                                   \
                const float g2_ = max_nc(M2, __builtin_amdgcn_fmed3f(x_[g], x_[g + 1], x_[g + 2]));            \
                M2 = __builtin_amdgcn_fmed3f(M1, g1_, g2_);                                                    \
                M1 = max_nc(M1, g1_);                                                                          \
            }                                                                                                  \
            _Pragma("unroll") for (int e = 3 * (NS_ / 3); e < NS_; ++e) {                                      \
                M2 = __builtin_amdgcn_fmed3f(M1, M2, x_[e]);                                                   \
                M1 = max_nc(M1, x_[e]);                                                                        \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
    /* twice as many, half as long MFMAs as on 32x32x16: one MFMA per 2.5 chain instructions */
#define F_INTERLEAVE()                                                                                         \
    do {                                                                                                       \
        _Pragma("unroll") for (int i = 0; i < 2 * NRB; ++i) {                                                  \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                 \
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                                 \
        }                                                                                                      \
    } while (0)
    // every lane hands its own sorted pair of a column block over (its NRB x 4 points of one channel); the publishing wave merges the
    // sixteen groups of a (tile, channel) -- one lane per channel there
    // (a group's row of 64 channels is rotated by 16 per lane quarter: the quarters of a store then hit different banks)
    const int fin_row = (wave * 4 + q4) * 128, fin_rot = 16 * q4 + l16;
    auto finish = [&](int c, int cb, float m1, float m2) {
        if ((abl & PN_ABL_INJECT_LOST) && c == 9 && wave == 2 && cb == 0) return;   // diagnostics: a hand-over that does not happen
        float* dst = tb + (c & 3) * F_SLOT + fin_row + ((16 * cb + fin_rot) & 63);
        dst[0] = m1;                                        // bits [6:5] of both: the chunk's ring tag (F_CHAIN_BLOCK), checked by publish()
        dst[64] = m2;
    };
    // (the mask in a vector register: id | tag is a scalar, and one v_and_or_b32 takes one scalar operand)
    unsigned id_mask = ~127u;
    asm volatile("" : "+v"(id_mask));
    // B fragments of a chunk: column block cb, step ks -- channel row 16 cb + l16, chunk 4 ks + 2 (q & 1) + (q >> 1) of the row (the
    // k the swapped A fragment holds in this quarter).  Conflict-free under the image's swizzle (chunk ^ (row & 15)): a 16-lane
    // group of a ds_read_b128 ({0-3, 12-15, 20-27}, ...) covers rows {0-3, 12-15} of one chunk and rows {4-11} of the chunk 2 further
    // -- chunk ^ row takes sixteen different values.
    const int qchunk = 2 * (q4 & 1) + (q4 >> 1);
    int stage = 0;
    if constexpr (TAIL) {
        // one point block (two row blocks) per wave: four MFMA blocks of 8 and four chains of 8 scores per chunk; every wave
        // publishes the eight chunks of ITS sample after chunk 7 and after chunk 15
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
            dvq_lds_barrier();                              // chunk c is in its stage; the other stage and tb parity are free
            if (c + 1 < 16) wreg = w3_load(w3h, 64 * (c + 1), wave, lane);
            if ((c & 3) == 0 && c > 0) {                  // the ring's four chunks are complete (barrier above)
#pragma unroll 1
                for (int q = c - 4; q < c; ++q) publish(q);
                dvq_lds_barrier();                          // before this chunk's pairs overwrite slot 0
            }
            const char* st = fl + stage * F_STAGE3;
            qf16x8 wf[4][4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) wf[cb][ks] = w3_frag(st, 16 * cb + l16, 4 * ks + qchunk);
            f32x4 accA[NRB], accB[NRB];
            float m1, m2;
            unsigned ctag_c[16];                          // id | ring tag per accumulator register, as scalars (see ctag4 below)
#pragma unroll
            for (int e = 0; e < 16; ++e) asm("s_or_b32 %0, %1, %2" : "=s"(ctag_c[e]) : "s"((unsigned)(((c >> 2) & 3) << 5)), "i"(e));
            F_MFMA_BLOCK(accA, wf[0]);
            F_MFMA_BLOCK(accB, wf[1]);
            F_CHAIN_BLOCK(accA, m1, m2, ctag_c);
            F_INTERLEAVE();
            finish(c, 0, m1, m2);
            F_MFMA_BLOCK(accA, wf[2]);
            F_CHAIN_BLOCK(accB, m1, m2, ctag_c);
            F_INTERLEAVE();
            finish(c, 1, m1, m2);
            F_MFMA_BLOCK(accB, wf[3]);
            F_CHAIN_BLOCK(accA, m1, m2, ctag_c);
            F_INTERLEAVE();
            finish(c, 2, m1, m2);
            F_CHAIN_BLOCK(accB, m1, m2, ctag_c);
            finish(c, 3, m1, m2);
            if (c + 1 < 16) w3_store(fl + (stage ^ 1) * F_STAGE3, wave, lane, wreg);
            stage ^= 1;
        }
    } else {
    f32x4 accP[NRB];                                      // the chunk's last accumulator block, scored under the next chunk's first MFMAs
    // Four chunks per trip of the rolled loop, the four written out: the ring slot (c & 3), the stage (c & 1), "is a chain pending"
    // and "is this a publishing chunk" are compile-time constants then -- LDS addresses become instruction offsets instead of vector
    // additions per access, the conditions disappear (round 5: the kernel is vector-issue bound).
#pragma unroll 1
    for (int c4 = 0; c4 < ((abl & PN_ABL_NO_CONV3) ? 0 : 16); c4 += 4) {
    // id (row block, register) | ring tag of this trip's four chunks, one SCALAR per accumulator register: the chain's one instruction
    // per score is then v_and_or_b32 (score, mask in a vector register, this scalar).  (Written as "id | tag" in the expression the
    // compiler makes it v_and_b32 + v_or3_b32: two vector instructions per score.)
    unsigned ctag4[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) asm("s_or_b32 %0, %1, %2" : "=s"(ctag4[e]) : "s"((unsigned)(((c4 >> 2) & 3) << 5)), "i"(e));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = c4 + u;
        const int stage = u & 1;
        const bool pending = u != 0;
        if (!(abl & PN_ABL_NO_CHUNK_BARRIER)) dvq_lds_barrier();              // chunk c is in its stage; the other stage and tb parity are free
        if (c + 1 < 16 && !(abl & PN_ABL_NO_W3_LOADS)) wreg = w3_load(w3h, 64 * (c + 1), wave, lane);
        if (u == 0 && c > 0 && !(abl & PN_ABL_NO_PUBLISH)) {              // the ring's four chunks are complete (barrier above): one per wave
            publish(c - 4 + wave);
            dvq_lds_barrier();                              // before this chunk's pairs overwrite slot 0
        }
        const char* st = fl + stage * F_STAGE3;
        qf16x8 wf[4][4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) wf[cb][ks] = w3_frag(st, 16 * cb + l16, 4 * ks + qchunk);
        // Four MFMA blocks (column blocks) and four chain blocks per chunk, each chain under the MFMAs of the block that follows its
        // own.  The last chain of a chunk (channels 48..63: accP) has no successor inside the chunk: it runs under the FIRST MFMA
        // block of the next chunk, except before a publish (c = 3, 7, 11, 15).
        f32x4 accA[NRB], accB[NRB];
        float m1, m2;
        F_MFMA_BLOCK(accA, wf[0]);
        if (pending) {
            F_CHAIN_BLOCK(accP, m1, m2, ctag4);
            F_INTERLEAVE();
            if (!(abl & PN_ABL_NO_HANDOVER)) finish(c - 1, 3, m1, m2);
            else if (m1 + m2 == 12345.f) tb[lane] = m1;
        }
        F_MFMA_BLOCK(accB, wf[1]);
        F_CHAIN_BLOCK(accA, m1, m2, ctag4);
        F_INTERLEAVE();
        if (!(abl & PN_ABL_NO_HANDOVER)) finish(c, 0, m1, m2);
        else if (m1 + m2 == 12345.f) tb[lane] = m1;
        F_MFMA_BLOCK(accA, wf[2]);
        F_CHAIN_BLOCK(accB, m1, m2, ctag4);
        F_INTERLEAVE();
        if (!(abl & PN_ABL_NO_HANDOVER)) finish(c, 1, m1, m2);
        else if (m1 + m2 == 12345.f) tb[lane] = m1;
        F_MFMA_BLOCK(accP, wf[3]);
        F_CHAIN_BLOCK(accA, m1, m2, ctag4);
        F_INTERLEAVE();
        if (!(abl & PN_ABL_NO_HANDOVER)) finish(c, 2, m1, m2);
        else if (m1 + m2 == 12345.f) tb[lane] = m1;
        if (u == 3) {                                     // nothing to cover it before a publish
            F_CHAIN_BLOCK(accP, m1, m2, ctag4);
            if (!(abl & PN_ABL_NO_HANDOVER)) finish(c, 3, m1, m2);
            else if (m1 + m2 == 12345.f) tb[lane] = m1;
        }
        if (c + 1 < 16 && !(abl & PN_ABL_NO_W3_LOADS)) w3_store(fl + (stage ^ 1) * F_STAGE3, wave, lane, wreg);
    }
    }
    }
#undef F_MFMA_BLOCK
#undef F_CHAIN_BLOCK
#undef F_INTERLEAVE
    dvq_lds_barrier();
    if constexpr (TAIL) {
#pragma unroll 1
        for (int q = 12; q < 16; ++q) publish(q);
    } else if (!(abl & PN_ABL_NO_PUBLISH)) {
        publish(12 + wave);
    }
    if ((abl & PN_ABL_STAMPS) && tid == 0) {                        // diagnostics: phase durations in units of 64 ticks, 8 bits each
        const unsigned long long t_end = __builtin_amdgcn_s_memtime();
        auto q = [](unsigned long long d) { d >>= 6; return (unsigned)(d > 255 ? 255 : d); };
        tstat[4 * rec + 3] = q(t_a - t_start) | (q(t_b - t_a) << 8) | (q(t_c - t_b) << 16) | (q((t_end - t_c) >> 3) << 24);
        if (abl & PN_ABL_CLOCK) {                                   // in-kernel clock in MHz: shader cycles per 100 MHz tick over the workgroup's life
            const unsigned long long r_end = __builtin_amdgcn_s_memrealtime();
            tstat[4 * rec + 3] = (unsigned)((t_end - t_start) * 100ull / (r_end - r_start + 1));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// exact_dot: THE definition of a conv3 score on this path.  16 lanes per dot, lane j owns k = 4j .. 4j+3 and 64+4j .. 64+4j+3 (fixed
// FMA order), then a 16-lane butterfly (every lane gets the same bits).  (The two 16-byte pieces of a lane are 256 B apart so that the
// sixteen lanes of a load read 256 CONTIGUOUS bytes: with k = 8j .. 8j+7 -- until round 5 -- every load touched four cache lines
// and used half of each, and the exact stage's candidate dots ran at what the CU's vector memory path gives to such gathers.)
template <int CTRL>
__device__ __forceinline__ float q_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float exact_dot_regs(const f32x4& w0, const f32x4& w1, const f32x4& a, const f32x4& c) {
    float s = w0[0] * a[0];
    s = fmaf(w0[1], a[1], s);
    s = fmaf(w0[2], a[2], s);
    s = fmaf(w0[3], a[3], s);
    s = fmaf(w1[0], c[0], s);
    s = fmaf(w1[1], c[1], s);
    s = fmaf(w1[2], c[2], s);
    s = fmaf(w1[3], c[3], s);
    s += q_dpp<0xB1>(s);
    s += q_dpp<0x4E>(s);
    s += q_dpp<0x141>(s);
    s += q_dpp<0x140>(s);
    return s;
}
__device__ __forceinline__ float exact_dot(const f32x4& w0, const f32x4& w1, const float* __restrict__ hrow, int j) {
    return exact_dot_regs(w0, w1, *reinterpret_cast<const f32x4*>(hrow + 4 * j), *reinterpret_cast<const f32x4*>(hrow + 4 * j + 64));
}
// torch.max semantics: a NaN wins
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

// order-preserving map float -> unsigned (for atomicMax on LDS)
__device__ __forceinline__ unsigned f2key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Run-time consistency counters (dvq_pointnet_fault_counters): [0] tile records the trunk kernel marked suspect (a ring value whose
// chunk tag is not the published chunk's: stale or missing input of the merge), [1] channels whose exact maximum lies outside the
// interval the tile records promise (max_t (top_t - E_t) <= max - w.c <= max_t (top_t + E_t)).  Either way the channel is evaluated
// over ALL the points concerned, so the feature is right; a non-zero counter says the filter's bookkeeping was not.
__device__ unsigned long long g_pn_faults[2];

// One workgroup per sample, 16 groups of 16 lanes.
//   phase A1 (one thread per channel): best lower bound lb over the tiles and the ANCHOR of the channel, the top kept point of the
//           tile that sets lb (always in range); the anchors in point order, exact_dot of each: x1, an exact score of the channel;
//   phase A2 (one thread per channel): every other kept score whose upper bound reaches L = max(lb, x1 - w.c) becomes a
//           (channel, point) pair; flagged 16-point groups of tiles in contention whose hidden points can still reach L become
//           (channel, tile, group) entries (rules 1 and 2);
//   phase B (one group per pair, point order): exact_dot, maximum;
//   phase C (one wave per entry, no barrier): the 16 points of a flagged group; then, whole workgroup per channel, every
//           point for the channels on the "everything" list (DVQ_PN_EXHAUSTIVE / non-finite inputs).
// stats (optional): channels with one candidate, with another count, wave entries, candidates; phase cycles; distinct rows, clouds.
//
// recompute != 0 (DVQ_PN_RECOMPUTE): the trunk kernel has NOT spilled its conv2 rows.  In front of every place that reads rows the
// workgroup then produces exactly the distinct points named there -- the anchors; the pairs and the 16 points of every flagged group;
// every point for the "everything" list and the interval check's repair -- with the trunk's own pn_conv12_block (W2 fragments from
// the filter image in L2, b2 / 2^-t_n from global memory, W1 / b1 staged in the LDS), 32 points per wave and batch, into their natural place h2[p] of
// the cloud's block of the scratch set: dots(), phase C and eval_all_list read them as they read spilled rows.  A bit per point says
// which rows exist.  A row's bits do not depend on its wave-mates, so they are the trunk's (DVQ_PN_EXHAUSTIVE=1 keeps the spilled
// rows and checks that).  Producer -> consumer inside the workgroup: every wave waits for its stores (vmcnt(0)) before the barrier
// that precedes the reads; the waves of a workgroup share their CU's L1, which the stores write through.
constexpr int PAIR_CAP = 2048;                            // (channel, point) pairs beyond the anchors; more: their 16-point groups instead
constexpr int FB_CAP = 512;
constexpr unsigned short NO_ANCHOR = 0xFFFFu;              // a channel on the "everything" list
constexpr int TODO_CAP = 2 * PAIR_CAP;                     // points of one recompute round (16-bit entries in pair_list's bytes); more: the whole cloud
template <int C>
__global__ __launch_bounds__(256, 4) void pn_exact_kernel(const f32x4* __restrict__ part, const qf32x2* __restrict__ part2, int tiles, int deal,
                                                       float* h2buf /* read; written too under ``recompute`` */, int recompute,
                                                       const float* __restrict__ pc, const float* __restrict__ trans,
                                                       const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ b2,
                                                       const char* __restrict__ w3f,
                                                       int N, int Npad, const float* __restrict__ w3, const float* __restrict__ b3,
                                                       const float* __restrict__ wnorm, const float* __restrict__ rnorm,
                                                       const unsigned* __restrict__ tstat, const float* __restrict__ cbuf, int relu, int exhaustive,
                                                       int pair_cap, int fb_cap, float* __restrict__ feat, long ld_feat,
                                                       unsigned long long* __restrict__ stats, int abl_arg) {
    const int abl = DVQ_DIAG_ON ? abl_arg : 0;
    __shared__ unsigned short anchor[1024];                // the channel's anchor point
    __shared__ int pair_list[PAIR_CAP];
    __shared__ int fb_list[FB_CAP];
    __shared__ short all_list[1024];
    __shared__ int pair_count, fb_count, all_count;
    __shared__ float fb_part[4][16];
    __shared__ float hm[PN_MAX_TILES], dm[PN_MAX_TILES], rd[PN_MAX_TILES], ef[PN_MAX_TILES];   // ef: the id bits' floor of E_t (bound_of)
    __shared__ unsigned best_k[1024];
    __shared__ float wcs[1024];                            // w_n . c per channel (rule 2, consistency check)
    __shared__ int pcnt[1024];                             // pairs per point -> first slot of the point -> fill cursor
    __shared__ unsigned sorted[PAIR_CAP];                  // channel | point << 10, grouped by point: the anchors, then the pairs
    __shared__ int wave_tot[4];
    __shared__ unsigned row_mask[32];                      // statistics: points that were somebody's anchor
    __shared__ unsigned done_mask[PN_MAX_POINTS / 32];     // recompute: bit p = row p of this cloud exists
    __shared__ int todo_count;                             // recompute: points claimed so far (never reset: a round's list starts at todo_base)
    __shared__ __attribute__((aligned(16))) float w1s[64 * 4 + 64];   // recompute: conv1's weights [64][4] and bias [64] (from global memory the compiler requests all 32 rows ahead: 128 registers)
    static_assert(PAIR_CAP >= 1024, "sorted[] holds the 1 024 anchors");
    static_assert(PN_MAX_POINTS <= 65536, "a point fits a 16-bit list entry");
    const int tid = threadIdx.x, g = tid >> 4, j = tid & 15;
    const long b = blockIdx.x;
    if (tid == 0) { pair_count = 0; fb_count = 0; all_count = 0; todo_count = 0; }
    if (tid < 32) row_mask[tid] = 0;
    done_mask[tid] = 0; done_mask[tid + 256] = 0;
    w1s[tid] = W1[tid];
    if (tid < 64) w1s[256 + tid] = b1[tid];
#pragma unroll
    for (int i = 0; i < 4; ++i) pcnt[tid + 256 * i] = 0;
    int nonfinite_point = 0;
    if (tid < tiles) {
        const unsigned* ts = tstat + 4 * (b * tiles + tid);
        hm[tid] = __uint_as_float(ts[0]) * 1.00001f;
        dm[tid] = __uint_as_float(ts[1]) * 1.00001f;
        rd[tid] = __uint_as_float(ts[2]) * 1.00001f;
        ef[tid] = E_ID_FLOOR * fmaxf(1.0f, 0x1p-13f * (__uint_as_float(ts[1]) * 1.00001f));
        nonfinite_point = ts[3] != 0 && !(abl & PN_ABL_STAMPS);      // (word 3 holds the phase stamps of the diagnostics build otherwise)
    }
    if (__syncthreads_or(nonfinite_point)) {
        // a cloud with a NaN / Inf coordinate: NaN in every channel, as the reference's affine layers and torch.max make it (the trunk
        // kernel's ReLU squashed it; see there)
        for (int n = tid; n < 1024; n += 256) feat[b * ld_feat + n] = __builtin_nanf("");
        return;
    }
    float* h2 = h2buf + b * (long)Npad * 128;
    const bool wrap_small = Npad <= 2 * N;                  // a padding slot's index is below 2 N: one subtraction instead of a division
    const f32x4* pt = part + b * (long)tiles * 1024;
    const qf32x2* pt2 = part2 + b * (long)tiles * 1024;     // the fourth and fifth id-carrying scores
    const bool stamps = DVQ_DIAG_ON && stats && (abl & PN_ABL_STAMPS);   // diagnostics: cycles per phase (tid 0's clock), summed into stats[4..7]
    unsigned long long tp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (stamps) tp[0] = __builtin_amdgcn_s_memtime();
    unsigned n_single = 0, n_multi = 0, n_cand = 0, n_wave = 0, n_suspect = 0;
    // E_t of channel (wn, rn).  C_ID covers the id bits RELATIVE to a score: 2^-15 of a normal number.  A score that is zero (or
    // denormal) in the trunk kernel's scaled units carries them as an ABSOLUTE 2^-141, which becomes 2^-141 / (s_w 2^t_n) in real
    // units, and the group tag replaces bits of the real value once more.  For a conv3 row of zeros (a channel whose BatchNorm gamma is
    // 0: w_n = r_n = 0, 2^t_n = 1) every other term is 0 and the records' interval was the single value "id bits" -- the exact maximum,
    // 0, lay outside it, and every such channel was counted and re-evaluated over all points.  1 / s_w <= max(1, 2^-13 max|d_p|)
    // (the wave's largest row norm times s_w is at least 2^14; s_w = 1 outside the exponent guard), hence the floor; rows with weights
    // have 2^-t_n <= 2^-14 |w_n| in front of it, far below the C_ID term.
    // (the floor is the innermost addend: a NaN / Inf term stays one and sends the channel to the "everything" path)
    auto bound_of = [&](float wn, float rn, int t) { return fmaf(rn, dm[t], fmaf(wn, rd[t], fmaf(C_ID * wn, dm[t], fmaf(2.0f * DELTA * wn, hm[t], ef[t])))); };
    // The interval the records promise for (max - w.c) of channel n: lb = max_t (c1_t - E_t), ub = max_t (c1_t + E_t); the first tile
    // that attains lb and its top score (the anchor); the largest bound.  top0 .. top3: c1 of the first four tiles (N <= 1024: all of
    // them), requested by the caller ahead of time; the tiles beyond are read here, in blocks of four.  A non-finite bound or top score
    // in ANY tile sends the channel to the "everything" path (fmaxf drops a NaN: tested apart).  Phases A1 and A2 both call this: the
    // same instructions on the same inputs, the same lb and anchor.
    struct Scan { float lb, ub, e_all, top_star; int t_star; bool all; };
    auto scan_tiles = [&](int n, float wn, float rn, float top0, float top1, float top2, float top3) {
        Scan s;
        bool nonfinite = false;
        auto fold = [&](int t, float top) {
            const float e = bound_of(wn, rn, t), l = top - e;
            nonfinite = nonfinite || !(e < 3.0e38f) || !(fabsf(top) < 3.0e38f);
            s.e_all = fmaxf(s.e_all, e);
            if (l > s.lb) { s.t_star = t; s.top_star = top; }
            s.lb = fmaxf(s.lb, l);
            s.ub = fmaxf(s.ub, top + e);
        };
        {
            const float e0 = bound_of(wn, rn, 0);
            s.e_all = e0;
            s.lb = top0 - e0;
            s.ub = top0 + e0;
            s.t_star = 0;
            s.top_star = top0;
            nonfinite = !(e0 < 3.0e38f) || !(fabsf(top0) < 3.0e38f);
            if (tiles > 1) fold(1, top1);
            if (tiles > 2) fold(2, top2);
            if (tiles > 3) fold(3, top3);
        }
        for (int t0 = 4; t0 < tiles; t0 += 4) {
            float top[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) top[u] = pt[min(t0 + u, tiles - 1) * 1024 + n][0];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (t0 + u < tiles) fold(t0 + u, top[u]);
        }
        s.all = exhaustive || nonfinite || !(s.e_all < 3.0e38f) || !(s.lb > NEG_BIG) || !(s.lb < 3.0e38f);   // non-finite inputs: evaluate everything
        return s;
    };
    // the point of a kept score of tile t
    auto point_of_score = [&](int t, float v) {
        int p = point_of_slot(t, slot_of_id(__float_as_uint(v) & 255u), deal);
        if (p >= N) p = wrap_small ? p - N : p % N;      // a padding slot: the real point it repeats
        if (abl & PN_ABL_FEW_ROWS) p &= 63;
        return p;
    };
    // ---- recompute: claim(p) puts point p on the round's list unless its row exists; fill_rows() ends the round: the listed rows
    // (all = false), or every row of the cloud that does not exist yet (all = true: a round without claims; a list beyond TODO_CAP:
    // every row, whatever the bits say), 32 points per wave and batch; a batch with fewer points repeats its last one and stores it once.  The list lives
    // in pair_list's bytes: free before phase A2 fills it and again once the pairs are sorted.
    unsigned short* todo = reinterpret_cast<unsigned short*>(pair_list);
    int todo_base = 0;
    auto claim = [&](int p) {
        const unsigned bit = 1u << (p & 31);
        if (atomicOr(&done_mask[p >> 5], bit) & bit) return;
        const int slot = atomicAdd(&todo_count, 1) - todo_base;
        if (slot < TODO_CAP) todo[slot] = (unsigned short)p;
    };
    auto fill_rows = [&](bool all) {
        dvq_lds_barrier();                                  // the round's claims are complete
        const int end = __builtin_amdgcn_readfirstlane(todo_count), listed = end - todo_base;   // (uniform: scalar registers)
        todo_base = end;
        const bool forced = listed > TODO_CAP;
        const bool whole = all || forced;
        const int cnt = whole ? N : listed;
        const int lane = tid & 63, r = lane & 31, h = lane >> 5;
        const float* k2g = reinterpret_cast<const float*>(w3f + IMG_OFF_K2);
        const uint16_t* w2pl = reinterpret_cast<const uint16_t*>(w3f + IMG_OFF_W2);
        for (int i0 = 32 * __builtin_amdgcn_readfirstlane(tid >> 6); i0 < cnt; i0 += 128) {
            if (whole && !forced && done_mask[i0 >> 5] == ~0u) continue;   // (i0 >> 5: the word of points i0 .. i0 + 31)
            // the lane half as an opaque value (see the trunk kernel), made opaque again in every batch: the reads of conv1's weights
            // do not depend on the batch otherwise, and the compiler moves all of them in front of the loop and spills them
            int h_op = h;
            asm volatile("" : "+v"(h_op));
            const int i = min(i0 + r, cnt - 1);
            const int p = whole ? i : (int)todo[i];
            float x[4];
            pn_point_in<C>(pc + b * (long)C * N + p, N, trans ? trans + b * 9 : nullptr, x);
            float* row = h2 + (long)p * 128 + 4 * h;
            const bool mine = i0 + r < cnt;
            qf16x8 h1a[4], h1b[4];
            float r_p;
            pn_conv1_split<C>(x, w1s, w1s + 256, h_op, h1a, h1b, r_p);
#pragma unroll 1
            for (int t4 = 0; t4 < 4; ++t4)                  // (rolled: 128 registers, and the code is there twice)
                pn_conv2_block(h1a, h1b, r_p, t4, k2g, b2, h_op,
                               [&](int t, int pl, int s) { return *reinterpret_cast<const qf16x8*>(w2pl + pl * (128 * 64) + (32 * t + r) * 64 + 8 * (2 * s + h)); },
                               [&](int t, const float (&o)[16]) { if (mine) pn_store_row16(row + 32 * t, o); });
            if (whole && lane == 0) done_mask[i0 >> 5] = ~0u;
            if (stats && lane == 0) {                        // statistics: batches and rows (straight to memory: no counter held across the kernel)
                atomicAdd(stats + 10, 1ull);
                atomicAdd(stats + 11, (unsigned long long)min(32, cnt - i0));
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows have left it ...
        dvq_lds_barrier();                                  // ... before anybody of the workgroup reads one
    };
    // Counting sort in the LDS of count codes (channel | point << 10; ~0u: none) by point into sorted[]; pcnt is zero on entry.  A
    // cloud's 1 024 channels take their maxima at ~100-200 distinct points: evaluated channel by channel every pair fetched its
    // 512-byte row from HBM again (the kernel ran at the HBM roofline); grouped by point a row is fetched once and found in the
    // L1 by the pairs that follow.  Returns the number of codes.
    auto sort_by_point = [&](auto code_at, int count, bool first) {
        for (int i = tid; i < count; i += 256) {
            const unsigned code = code_at(i);
            if (code != ~0u) atomicAdd(&pcnt[(code >> 10) & 1023], 1);       // N > 1024: points 1024 apart share a slot range
        }
        dvq_lds_barrier();
        const int c0 = pcnt[4 * tid], c1 = pcnt[4 * tid + 1], c2 = pcnt[4 * tid + 2], c3 = pcnt[4 * tid + 3];
        if (stats) {                                        // distinct rows: points with an anchor, then points with pairs only
            const unsigned m = (unsigned)(c0 != 0) | (unsigned)(c1 != 0) << 1 | (unsigned)(c2 != 0) << 2 | (unsigned)(c3 != 0) << 3;
            const int sh = 4 * (tid & 7);
            int rows;                                       // (straight to memory: no counter held across the kernel)
            if (first) { if (m) atomicOr(&row_mask[tid >> 3], m << sh); rows = __popc(m); }
            else rows = __popc(m & ~(row_mask[tid >> 3] >> sh));
            if (rows) atomicAdd(stats + 8, (unsigned long long)rows);
        }
        int incl = c0 + c1 + c2 + c3;
        // (the lane as an opaque value per sort: the six shuffle addresses are then formed here, not kept -- spilled -- from the first
        // sort to the second across the recompute; a lane below o reads some lane's value and ignores it)
        int lane_op = tid & 63;
        asm volatile("" : "+v"(lane_op));
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __builtin_amdgcn_ds_bpermute(4 * (lane_op - o), incl);
            if ((tid & 63) >= o) incl += v;
        }
        if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
        dvq_lds_barrier();
        int base = 0;
        for (int w = 0; w < (tid >> 6); ++w) base += wave_tot[w];
        const int total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        const int excl = base + incl - (c0 + c1 + c2 + c3);
        pcnt[4 * tid] = excl;
        pcnt[4 * tid + 1] = excl + c0;
        pcnt[4 * tid + 2] = excl + c0 + c1;
        pcnt[4 * tid + 3] = excl + c0 + c1 + c2;
        dvq_lds_barrier();
        for (int i = tid; i < count; i += 256) {
            const unsigned code = code_at(i);
            if (code != ~0u) sorted[atomicAdd(&pcnt[(code >> 10) & 1023], 1)] = code;
        }
        dvq_lds_barrier();
        return total;
    };
    // The first ``total`` entries of sorted[]: every 16-lane group takes a contiguous share of the list, four pairs in flight.
    // first: the anchors -- one per channel: plain stores, and the centre term of the channel with them.
    auto dots = [&](int total, bool first) {
        const int per = (total + 15) >> 4, i0 = g * per, i1 = min(total, i0 + per);
        f32x4 cen_a = {0.f, 0.f, 0.f, 0.f}, cen_b = cen_a;   // the centre's slice: the anchors' pass only (not held across the other phases)
        if (first) { cen_a = *reinterpret_cast<const f32x4*>(cbuf + b * 128 + 4 * j); cen_b = *reinterpret_cast<const f32x4*>(cbuf + b * 128 + 4 * j + 64); }
        for (int i = i0; i < i1; i += 4) {
            f32x4 w0[4], w1[4], ha[4], hb[4];
            int nn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned code = sorted[min(i + u, i1 - 1)];
                nn[u] = (int)(code & 1023u);
                // (uniform base + 32-bit offset: the loads take the base from scalar registers, no 64-bit vector add per row)
                const unsigned woff = (code & 1023u) * 512u + 16u * (unsigned)j, hoff = (code >> 10) * 512u + 16u * (unsigned)j;
                w0[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(w3) + woff);
                w1[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(w3) + woff + 256);
                ha[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(h2) + hoff);
                hb[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(h2) + hoff + 256);
            }
            float v[4], wc[4];                              // all the chains first (independent: they interleave), the LDS updates after
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = exact_dot_regs(w0[u], w1[u], ha[u], hb[u]);
                wc[u] = first ? exact_dot_regs(w0[u], w1[u], cen_a, cen_b) : 0.f;
            }
            if (j == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i + u < i1) {
                        if (first) { best_k[nn[u]] = f2key(v[u]); wcs[nn[u]] = wc[u]; }
                        else atomicMax(&best_k[nn[u]], f2key(v[u]));
                    }
            }
        }
    };
    // ---- phase A1: lower bound and anchor of every channel
    {
        float top[4][4], wn[4], rn[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const int n = tid + 256 * ci;
#pragma unroll
            for (int u = 0; u < 4; ++u) top[ci][u] = pt[min(u, tiles - 1) * 1024 + n][0];
            wn[ci] = wnorm[n]; rn[ci] = rnorm[n];
        }
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const int n = tid + 256 * ci;
            const Scan s = scan_tiles(n, wn[ci], rn[ci], top[ci][0], top[ci][1], top[ci][2], top[ci][3]);
            best_k[n] = f2key(NEG_BIG);
            wcs[n] = 0.f;
            if (s.all) {
                all_list[atomicAdd(&all_count, 1)] = (short)n;
                anchor[n] = NO_ANCHOR;
            } else
                anchor[n] = (unsigned short)point_of_score(s.t_star, s.top_star);
        }
    }
    dvq_lds_barrier();
    if (stamps) tp[1] = __builtin_amdgcn_s_memtime();
    auto anchor_code = [&](int n) { const unsigned p = anchor[n]; return p == NO_ANCHOR ? ~0u : (unsigned)n | (p << 10); };
    const int n_anchor = sort_by_point(anchor_code, 1024, true);
#pragma unroll
    for (int i = 0; i < 4; ++i) pcnt[tid + 256 * i] = 0;   // (the next sort's histogram: after the barrier that ends this one)
    if (stamps) tp[2] = __builtin_amdgcn_s_memtime();
    if (recompute) {                                        // the anchors' rows (sorted[] is grouped by point: one claim per run)
        for (int i = tid; i < n_anchor; i += 256) {
            const int p = (int)(sorted[i] >> 10);
            if (i == 0 || (int)(sorted[i - 1] >> 10) != p) claim(p);
        }
        fill_rows(false);
    }
    if (!(abl & PN_ABL_NO_DOTS)) dots(n_anchor, true);
    dvq_lds_barrier();
    if (stamps) tp[3] = __builtin_amdgcn_s_memtime();
    // ---- phase A2
    // the interval the records promise for (max - w.c) of channels tid + 256 i; lo > hi: not checked.  Eight scalars updated through
    // selects: the channel loop below stays ROLLED (unrolled it was 12 k instructions, 80 KB of code for a 64 KB instruction cache
    // shared by two CUs) without turning an indexed array into scratch memory.
    float lo_0 = 1.f, lo_1 = 1.f, lo_2 = 1.f, lo_3 = 1.f, hi_0 = 0.f, hi_1 = 0.f, hi_2 = 0.f, hi_3 = 0.f;
    // the next channel's records (the first four tiles' entries -- N <= 1024: all of them) and norms are requested before the current
    // channel is worked on: one exposed trip to memory instead of four
    f32x4 nf0 = pt[tid], nf1 = pt[min(1, tiles - 1) * 1024 + tid], nf2 = pt[min(2, tiles - 1) * 1024 + tid], nf3 = pt[min(3, tiles - 1) * 1024 + tid];
    // (the fourth and fifth scores with them: read where the third is in range, that was a trip to memory inside the tile loop whenever
    // ONE lane of the wave needed it -- most iterations)
    qf32x2 ng0 = pt2[tid], ng1 = pt2[min(1, tiles - 1) * 1024 + tid], ng2 = pt2[min(2, tiles - 1) * 1024 + tid], ng3 = pt2[min(3, tiles - 1) * 1024 + tid];
    float nwn = wnorm[tid], nrn = rnorm[tid];
#pragma unroll 1
    for (int ci = 0; ci < 4; ++ci) {
        const int n = tid + 256 * ci;
        const float wn = nwn, rn = nrn;
        const f32x4 f0 = nf0, f1 = nf1, f2 = nf2, f3 = nf3;
        const qf32x2 g0 = ng0, g1 = ng1, g2 = ng2, g3 = ng3;
        if (ci < 3) {
            const int nx = n + 256;
            nf0 = pt[nx]; nf1 = pt[min(1, tiles - 1) * 1024 + nx]; nf2 = pt[min(2, tiles - 1) * 1024 + nx]; nf3 = pt[min(3, tiles - 1) * 1024 + nx];
            ng0 = pt2[nx]; ng1 = pt2[min(1, tiles - 1) * 1024 + nx]; ng2 = pt2[min(2, tiles - 1) * 1024 + nx]; ng3 = pt2[min(3, tiles - 1) * 1024 + nx];
            nwn = wnorm[nx]; nrn = rnorm[nx];
        }
        const Scan s = scan_tiles(n, wn, rn, f0[0], f1[0], f2[0], f3[0]);
        if (s.all) continue;                               // on the "everything" list since phase A1
        const float lb = s.lb;
        // Rule 2: x1 = exact_dot(w_n, h2[anchor]) - w_n . c is the score of a point of the set the feature is the maximum over, so
        // nothing whose upper bound is below it can change that maximum.  The slack (the form of the consistency check's) keeps the
        // fp32 subtraction's own rounding from lifting L above x1's real value; a NaN (Inf - Inf) leaves lb: fmaxf drops it.
        float L = lb;
        if (!(abl & PN_ABL_NO_RULE2)) {
            const float v1 = key2f(best_k[n]), wc1 = wcs[n];
            L = fmaxf(lb, (v1 - wc1) - 4.0e-7f * (fabsf(v1) + fabsf(wc1)));
        }
        int cands = 1;                                     // the anchor
        bool whole = false;
        float lo_c = lb, hi_c = s.ub;
        auto consider = [&](int t, const f32x4& q, const qf32x2& q45) {
            const float et = bound_of(wn, rn, t);
            const unsigned suspect = (__float_as_uint(q[3]) >> 16) & 1u;   // the trunk kernel did not trust its own merge: it flagged every group
            n_suspect += suspect;
            // the tile's largest score is out of range: so is the rest of it -- unless the record is suspect: then its scores prove
            // nothing about the tile and all its points are evaluated (a bogus top score that RAISES lb is caught by the check below)
            if (!suspect && !(q[0] + et >= L)) return;
            unsigned flags = __float_as_uint(q[3]) & 0xFFFFu;   // one bit per 16-point group: 4 wave + lane quarter (pn_slots.h)
            unsigned forced = suspect ? 0xFFFFu : 0u;           // groups that rule 1 must not gate
            // a kept score in range: its point becomes a pair of the channel.  (No search for a point that is already one: only
            // padding slots repeat a point, a repeated candidate costs one more dot, and the search was a third of this phase.)
            auto take = [&](float v) {
                const int p = point_of_score(t, v);
                const int slot = atomicAdd(&pair_count, 1);
                if (slot < pair_cap) pair_list[slot] = n | (p << 10);
                else {                                           // list full (never seen): evaluate its 16-point group instead
                    const unsigned bit = 1u << pn_group_of_id(__float_as_uint(v));
                    flags |= bit;
                    forced |= bit;
                }
                ++cands;
            };
            // descending scores: the ones in range are a prefix of (c1 .. c5); the anchor has been evaluated
            const float sc5[5] = {q[0], q[1], q[2], q45[0], q45[1]};
#pragma unroll 1
            for (int k = (t == s.t_star ? 1 : 0); k < 5; ++k) {
                const float v = k == 0 ? sc5[0] : k == 1 ? sc5[1] : k == 2 ? sc5[2] : k == 3 ? sc5[3] : sc5[4];
                if (!(v + et >= L)) break;
                take(v);
            }
            while (flags) {
                const int wh = __ffs(flags) - 1;             // the group: 4 * wave + lane quarter
                flags &= flags - 1;
                if (!((forced >> wh) & 1u) && !(abl & PN_ABL_NO_RULE1)) {
                    // Rule 1: a point of group wh that is not among the five scores at most u: the smaller of the group's published
                    // pair where both were kept (its third is bounded by its second only -- and may well exceed c5), else c5 (one
                    // of the pair did not make the five).  Descending scores: the LAST one of the group is its second.  Written so
                    // that a NaN keeps the group.
                    auto of_group = [&](float v) { return pn_group_of_id(__float_as_uint(v)) == wh; };
                    const bool m0 = of_group(sc5[0]), m1 = of_group(sc5[1]), m2 = of_group(sc5[2]), m3 = of_group(sc5[3]), m4 = of_group(sc5[4]);
                    const float second = m4 ? sc5[4] : m3 ? sc5[3] : m2 ? sc5[2] : m1 ? sc5[1] : sc5[0];
                    const float u = (int)m0 + (int)m1 + (int)m2 + (int)m3 + (int)m4 >= 2 ? second : sc5[4];
                    if (u + et < L) continue;
                }
                const int slot = atomicAdd(&fb_count, 1);
                if (slot < fb_cap) fb_list[slot] = n | (t << 10) | (wh << 20);
                else if (!whole) {                           // list full (never seen): the channel goes on the "everything" list
                    whole = true;
                    all_list[atomicAdd(&all_count, 1)] = (short)n;
                }
                ++n_wave;
            }
        };
        // one copy of the code above for every tile (rolled: see lo_0 .. hi_3); tiles beyond the first four are loaded in blocks of four
        f32x4 q0 = f0, q1 = f1, q2 = f2, q3 = f3;
        qf32x2 h0 = g0, h1 = g1, h2q = g2, h3 = g3;
#pragma unroll 1
        for (int t0 = 0; t0 < tiles; t0 += 4) {
            if (t0 > 0) {
                q0 = pt[min(t0, tiles - 1) * 1024 + n]; q1 = pt[min(t0 + 1, tiles - 1) * 1024 + n];
                q2 = pt[min(t0 + 2, tiles - 1) * 1024 + n]; q3 = pt[min(t0 + 3, tiles - 1) * 1024 + n];
                h0 = pt2[min(t0, tiles - 1) * 1024 + n]; h1 = pt2[min(t0 + 1, tiles - 1) * 1024 + n];
                h2q = pt2[min(t0 + 2, tiles - 1) * 1024 + n]; h3 = pt2[min(t0 + 3, tiles - 1) * 1024 + n];
            }
#pragma unroll 1
            for (int u = 0; u < 4 && t0 + u < tiles; ++u) {
                const f32x4 q = u == 0 ? q0 : u == 1 ? q1 : u == 2 ? q2 : q3;
                const qf32x2 q45 = u == 0 ? h0 : u == 1 ? h1 : u == 2 ? h2q : h3;
                consider(t0 + u, q, q45);
            }
        }
        if (whole) { lo_c = 1.f; hi_c = 0.f; }              // evaluated in full below: nothing to check
        lo_0 = ci == 0 ? lo_c : lo_0; hi_0 = ci == 0 ? hi_c : hi_0;
        lo_1 = ci == 1 ? lo_c : lo_1; hi_1 = ci == 1 ? hi_c : hi_1;
        lo_2 = ci == 2 ? lo_c : lo_2; hi_2 = ci == 2 ? hi_c : hi_2;
        lo_3 = ci == 3 ? lo_c : lo_3; hi_3 = ci == 3 ? hi_c : hi_3;
        n_single += cands == 1;
        n_multi += cands != 1;
        n_cand += cands;
    }
    dvq_lds_barrier();
    if (stamps) tp[4] = __builtin_amdgcn_s_memtime();
    // ---- phase C: everything (NaN-propagating maximum, torch.max semantics): the channels on all_list over ALL points, four channels
    // per sweep of the rows (a row's slice is loaded once for the four)
    auto eval_all_list = [&](int count) {
        for (int i = 0; i < count; i += 4) {
            f32x4 w0[4], w1[4];
            float best[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = all_list[min(i + u, count - 1)];
                w0[u] = *reinterpret_cast<const f32x4*>(w3 + n * 128 + 4 * j);
                w1[u] = *reinterpret_cast<const f32x4*>(w3 + n * 128 + 4 * j + 64);
                best[u] = NEG_BIG;
            }
            for (int p = g; p < N; p += 16) {
                const float* hr = reinterpret_cast<const float*>(reinterpret_cast<const char*>(h2) + ((unsigned)p * 512u + 16u * (unsigned)j));
                const f32x4 ha = *reinterpret_cast<const f32x4*>(hr), hb = *reinterpret_cast<const f32x4*>(hr + 64);
#pragma unroll
                for (int u = 0; u < 4; ++u) best[u] = max_nan(best[u], exact_dot_regs(w0[u], w1[u], ha, hb));
                // a NaN stays a NaN (torch.max): four NaN maxima need no more points.  A cloud that is non-finite as a whole -- the row
                // of a grasp whose decoder output left fp16's range, on its way to the per-row fallback of GenNet.gen -- sent ONE
                // workgroup through 1 024 channels x all points, the straggler of its launch (20 ms at the benchmark's batch).
                if (best[0] != best[0] && best[1] != best[1] && best[2] != best[2] && best[3] != best[3]) break;
            }
            if (j == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) fb_part[u][g] = best[u];
            }
            dvq_lds_barrier();
            if (tid < 4 && i + tid < count) {
                float v = fb_part[tid][0];
                for (int k = 1; k < 16; ++k) v = max_nan(v, fb_part[tid][k]);
                best_k[all_list[i + tid]] = (v != v) ? 0xffffffffu : f2key(v);       // NaN: the largest key, decoded below
            }
            dvq_lds_barrier();
        }
    };
    // ---- phases B and C, then the consistency check and its repair, as two trips of ONE rolled loop: the recompute and the sweep of the
    // "everything" list exist once in the code (the instruction cache: see lo_0 .. hi_3)
    unsigned n_bad = 0;
    int n_sorted = 0, nfb = 0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) {
            // ---- phase B: the pairs in point order
            const int npairs = min(pair_count, pair_cap);
            n_sorted = sort_by_point([&](int i) { return (unsigned)pair_list[i]; }, npairs, false);
            if (stamps) tp[5] = __builtin_amdgcn_s_memtime();
            nfb = (abl & PN_ABL_NO_GROUPS) ? 0 : min(fb_count, fb_cap);
            // the rows of the pairs (grouped by point: one claim per run) and of the flagged groups -- unless the "everything" list has
            // entries (complete since phase A2): every row is produced then, and a claim would mark a row that is not there yet
            if (recompute && all_count == 0) {
                for (int i = tid; i < n_sorted; i += 256) {
                    const int p = (int)(sorted[i] >> 10);
                    if (i == 0 || (int)(sorted[i - 1] >> 10) != p) claim(p);
                }
                for (int i = tid; i < 16 * nfb; i += 256) {
                    const int code = fb_list[i >> 4];
                    int p = point_of_slot((code >> 10) & 1023, pn_group_slot((code >> 20) & 15, i & 15), deal);
                    if (p >= N) p %= N;
                    claim(p);
                }
            }
        } else {
            // ---- consistency: the exact maximum of a channel must lie where its tile records said it would.  |approx + w.c - exact| <= E_t
            // for every point of tile t, so  max_t (top_t - E_t) <= max - w.c <= max_t (top_t + E_t).  A maximum outside that interval means a
            // record did not describe its tile (a wrong score or id; a missing input that was the tile's best shows up in the trunk kernel's
            // own tag check instead): such a channel is evaluated over all points, and counted.
            dvq_lds_barrier();                               // best_k / wcs complete; all_list free again
            if (tid == 0) all_count = 0;
            dvq_lds_barrier();
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const int n = tid + 256 * ci;
                const float lo_c = ci == 0 ? lo_0 : ci == 1 ? lo_1 : ci == 2 ? lo_2 : lo_3, hi_c = ci == 0 ? hi_0 : ci == 1 ? hi_1 : ci == 2 ? hi_2 : hi_3;
                if (!(lo_c <= hi_c) || (abl & ~PN_ABL_VALID)) continue;   // (the timing ablations -- of either kernel -- leave maxima that are not maxima)
                const float v = key2f(best_k[n]), wc = wcs[n];
                const float x = v - wc, slack = 4.0e-7f * (fabsf(v) + fabsf(wc));   // the subtraction's own rounding
                if (!(x >= lo_c - slack && x <= hi_c + slack)) {
                    all_list[atomicAdd(&all_count, 1)] = (short)n;
                    ++n_bad;
                }
            }
            dvq_lds_barrier();
        }
        const int n_all = __builtin_amdgcn_readfirstlane(all_count);
        if (recompute && (pass == 0 || n_all > 0)) fill_rows(n_all > 0);
        if (pass == 0) {
            if (!(abl & PN_ABL_NO_DOTS)) dots(n_sorted, false);
            if (stamps) tp[6] = __builtin_amdgcn_s_memtime();
            // ---- phase C: flagged 16-point groups, one wave of the workgroup per entry, its four 16-lane groups take 4 points each
            for (int i = tid >> 6; i < nfb; i += 4) {
                const int code = fb_list[i];
                const int n = code & 1023, t = (code >> 10) & 1023, grp = (code >> 20) & 15;
                const float* wr = reinterpret_cast<const float*>(reinterpret_cast<const char*>(w3) + ((unsigned)n * 512u + 16u * (unsigned)j));
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(wr), w1 = *reinterpret_cast<const f32x4*>(wr + 64);
                float best = NEG_BIG;
                {
                    f32x4 ha[4], hb[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {                   // this lane group's 4 of the group's 16 points: row block g & 3, register u
                        int p = point_of_slot(t, pn_group_slot(grp, 4 * (g & 3) + u), deal);   // tail tile: row blocks 2, 3 repeat 0, 1
                        if (p >= N) p %= N;
                        const float* hr = reinterpret_cast<const float*>(reinterpret_cast<const char*>(h2) + ((unsigned)p * 512u + 16u * (unsigned)j));
                        ha[u] = *reinterpret_cast<const f32x4*>(hr);
                        hb[u] = *reinterpret_cast<const f32x4*>(hr + 64);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) best = fmaxf(best, exact_dot_regs(w0, w1, ha[u], hb[u]));
                }
                if (j == 0) atomicMax(&best_k[n], f2key(best));
            }
            dvq_lds_barrier();
        }
        eval_all_list(n_all);
    }
    if (n_suspect) atomicAdd(&g_pn_faults[0], (unsigned long long)n_suspect);
    if (n_bad) atomicAdd(&g_pn_faults[1], (unsigned long long)n_bad);
    int tid_op = tid;                                       // (opaque: the channel offsets are formed again here instead of being kept -- spilled -- since phase A2)
    asm volatile("" : "+v"(tid_op));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = tid_op + 256 * i;
        const unsigned k = best_k[n];
        const float v = (k == 0xffffffffu ? __builtin_nanf("") : key2f(k)) + b3[n];
        feat[b * ld_feat + n] = relu ? (v != v ? v : fmaxf(v, 0.f)) : v;
    }
    if (stamps && tid == 0) {
        const unsigned long long t_end = __builtin_amdgcn_s_memtime();
        atomicAdd(stats + 4, (tp[1] - tp[0]) + (tp[4] - tp[3])); atomicAdd(stats + 5, (tp[2] - tp[1]) + (tp[5] - tp[4]));
        atomicAdd(stats + 6, (tp[3] - tp[2]) + (tp[6] - tp[5])); atomicAdd(stats + 7, t_end - tp[6]);
        atomicAdd(stats + 9, tp[3] - tp[0]);               // of the above: lower bounds, anchors, their sort and dots (rule 2's extra pass)
    }
    if (stats) {
        if (n_single) atomicAdd(stats + 0, (unsigned long long)n_single);
        if (n_multi) atomicAdd(stats + 1, (unsigned long long)n_multi);
        if (n_wave) atomicAdd(stats + 2, (unsigned long long)n_wave);
        if (n_cand) atomicAdd(stats + 3, (unsigned long long)n_cand);
    }
}

// Centre of a sample: mean of the conv2 rows of the points 0, N/4, N/2, 3N/4, plain fp32 (any vector would do -- it shifts
// every score of a channel by the same w.c -- but one close to the rows makes the fp16 residuals, hence the bounds, small).
// One workgroup takes CENTER_SPB samples: W2 (32 KB) is staged in the LDS once (transposed, conflict-free) for all of them.
constexpr int CENTER_SPB = 4;                             // (8: 80 us per launch of 3 641 samples, 4: 61, 2: 64, 1: 65 -- round 6)
template <int C>
__global__ __launch_bounds__(256) void pn_center_kernel(const float* __restrict__ pc, const float* __restrict__ trans, int N, long B,
                                                        const float* __restrict__ W1, const float* __restrict__ b1,
                                                        const float* __restrict__ W2, const float* __restrict__ b2,
                                                        float* __restrict__ cbuf, unsigned* __restrict__ tstat, int tiles) {
    __shared__ float w2t[64][129];                         // w2t[k][ch] = W2[ch][k] (row stride 129: conflict-free both ways)
    __shared__ float h1c[4][64];
    __shared__ float h2c[4][128];
    const int tid = threadIdx.x, q = tid >> 6, k = tid & 63;
    for (int i = tid; i < 128 * 64; i += 256) w2t[i & 63][i >> 6] = W2[i];
    for (int sb = 0; sb < CENTER_SPB; ++sb) {
        const long b = (long)blockIdx.x * CENTER_SPB + sb;
        if (b >= B) break;
        for (int i = tid; i < 4 * tiles; i += 256) tstat[b * 4 * tiles + i] = 0u;   // the sample's tile records start from zero (the trunk kernel's atomicMax targets): no memset launch
        {
            const int p = (int)(((long)q * N) / 4);
            const float* src = pc + b * (long)C * N + p;
            float x0 = src[0], x1 = src[N], x2 = src[2L * N];
            const float x3 = (C > 3) ? src[3L * N] : 0.f;
            if (trans) {
                const float* t = trans + b * 9;
                const float n0 = fmaf(x2, t[6], fmaf(x1, t[3], x0 * t[0]));
                const float n1 = fmaf(x2, t[7], fmaf(x1, t[4], x0 * t[1]));
                const float n2 = fmaf(x2, t[8], fmaf(x1, t[5], x0 * t[2]));
                x0 = n0; x1 = n1; x2 = n2;
            }
            const float* w = W1 + 4 * k;
            float a = x0 * w[0];
            a = fmaf(x1, w[1], a);
            a = fmaf(x2, w[2], a);
            a = fmaf(x3, w[3], a);
            h1c[q][k] = fmaxf(a + b1[k], 0.f);
        }
        dvq_lds_barrier();                                   // h1c (and, the first time, w2t) complete
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int ch = k + 64 * half;
            float a = 0.f;
            for (int i = 0; i < 64; ++i) a = fmaf(w2t[i][ch], h1c[q][i], a);
            h2c[q][ch] = fmaxf(a + b2[ch], 0.f);
        }
        dvq_lds_barrier();
        if (tid < 128) cbuf[b * 128 + tid] = 0.25f * ((h2c[0][tid] + h2c[1][tid]) + (h2c[2][tid] + h2c[3][tid]));
        // the next sample's h1c writes come after this barrier pair: h2c reads above are done before its second barrier
    }
}

// One wave per conv3 output channel: fp16 image (k permuted to conv2's accumulator order, scaled by a power of two so that
// the row maximum lies in [2^14, 2^15)), 1 / scale, |w| rounded up.
__global__ __launch_bounds__(256) void pn_filter_pack_kernel(const float* __restrict__ w3, _Float16* __restrict__ wh,
                                                             float* __restrict__ tinv, float* __restrict__ wnorm,
                                                             float* __restrict__ rnorm) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const float a = w3[n * 128 + lane], c = w3[n * 128 + 64 + lane];
    const float amax = wave_max(fmaxf(fabsf(a), fabsf(c)));
    float sq = fmaf(a, a, c * c);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o);
    float t = 1.f;
    const int ex = (int)((__float_as_uint(amax) >> 23) & 255u);
    if (ex > 20 && ex < 235) t = __uint_as_float((unsigned)(127 + 15 - (ex - 126)) << 23);
    // image position pos = 16 blk + q holds channel 16 blk + perm(q), perm = (0 1 2 3 8 9 10 11 4 5 6 7 12 13 14 15)
    float rs = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int pos = 64 * half + lane;
        const int q = pos & 15;
        const int k = (pos & ~15) + ((q & 3) | ((q & 4) << 1) | ((q & 8) >> 1));
        const float v = w3[n * 128 + k] * t;
        const _Float16 hv = (_Float16)v;
        wh[n * 128 + pos] = hv;
        const float res = v - (float)hv;
        rs = fmaf(res, res, rs);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) rs += __shfl_xor(rs, o);
    if (lane == 0) {
        tinv[n] = 1.0f / t;
        wnorm[n] = sqrtf(sq) * 1.00001f;
        rnorm[n] = sqrtf(rs) / t * 1.00001f;
    }
}

// One wave per conv2 output channel (128 rows of 64): the two fp16 planes of w * 2^t_n (row maximum in [2^14, 2^15)) -- the second the
// remainder as it is (csrc/gemm_f16x2.hip's packer scales it by 2^11 for a second accumulator; conv2 here has one) -- and 2^-t_n.
__global__ __launch_bounds__(256) void pn_filter_pack_w2_kernel(const float* __restrict__ w2, _Float16* __restrict__ planes,
                                                                float* __restrict__ kinv) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const float v = w2[n * 64 + lane];
    const float amax = wave_max(fabsf(v));
    float t = 1.f;
    const int ex = (int)((__float_as_uint(amax) >> 23) & 255u);
    if (ex > 20 && ex < 235) t = __uint_as_float((unsigned)(127 + 15 - (ex - 126)) << 23);
    const float vs = v * t;
    const _Float16 p1 = (_Float16)vs;
    const _Float16 p2 = (_Float16)(vs - (float)p1);
    planes[n * 64 + lane] = p1;
    planes[128 * 64 + n * 64 + lane] = p2;
    if (lane == 0) kinv[n] = 1.0f / t;
}

}  // namespace

size_t dvq_pn_filter_image_bytes() { return (size_t)IMG_BYTES; }

int dvq_launch_pn_filter_pack(const float* w2, const float* w3, void* image, hipStream_t st) {
    char* im = (char*)image;
    DVQ_LAUNCH(pn_filter_pack_kernel, dim3(256), dim3(256), 0, st, w3, reinterpret_cast<_Float16*>(im),
               reinterpret_cast<float*>(im + IMG_OFF_TI), reinterpret_cast<float*>(im + IMG_OFF_WN),
               reinterpret_cast<float*>(im + IMG_OFF_RN));
    DVQ_CHECK_LAUNCH("pn_filter_pack");
    DVQ_LAUNCH(pn_filter_pack_w2_kernel, dim3(32), dim3(256), 0, st, w2, reinterpret_cast<_Float16*>(im + IMG_OFF_W2),
               reinterpret_cast<float*>(im + IMG_OFF_K2));
    DVQ_CHECK_LAUNCH("pn_filter_pack_w2");
    return DVQ_OK;
}

// The scratch set of a launch (pn_filter.h): h2 [B][Npad][128] fp32, part [B][tiles][1024] float4, part2 [B][tiles][1024] float2, tstat
// [B][tiles][4] (zeroed by pn_center_kernel), cbuf [B][128].
static int filter_geometry(int N, PnGeometry* g) {
    *g = pn_geometry(N, dvq_knobs().pn_tail != 0);
    DVQ_REQUIRE(g->tiles <= PN_MAX_TILES, "pointnet: the filtered trunk takes at most %d points", PN_MAX_POINTS);
    return DVQ_OK;
}
#ifdef DVQ_DIAG
static int pn_abl() { const char* e = getenv("DVQ_PN_ABL"); return e ? atoi(e) : 0; }   // a sum of PnAbl bits (pn_filter.h): diagnostics build only
#else
static constexpr int pn_abl() { return 0; }
#endif

// the instances of the two kernels templated on the channel count (3 or 4)
using TrunkFilterKernel = decltype(&pn_trunk_filter_kernel<3, false>);
static TrunkFilterKernel trunk_filter_kernel(int C, bool tail) {
    static const TrunkFilterKernel k[2][2] = {{&pn_trunk_filter_kernel<3, false>, &pn_trunk_filter_kernel<3, true>},
                                              {&pn_trunk_filter_kernel<4, false>, &pn_trunk_filter_kernel<4, true>}};
    return k[C == 4][tail];
}
static decltype(&pn_center_kernel<3>) center_kernel(int C) { return C == 4 ? &pn_center_kernel<4> : &pn_center_kernel<3>; }
static decltype(&pn_exact_kernel<3>) exact_kernel(int C) { return C == 4 ? &pn_exact_kernel<4> : &pn_exact_kernel<3>; }
// DVQ_PN_RECOMPUTE: the trunk kernel does not spill its conv2 rows, pn_exact_kernel produces the ones it reads.  Front and back of a
// launch both ask here.  The exhaustive evaluation (DVQ_PN_EXHAUSTIVE=1) always takes spilled rows: it stays an independent check,
// and "filtered == exhaustive" then also says that recomputed rows have the trunk's bits.
static bool pn_recompute() { return dvq_knobs().pn_recompute && !dvq_knobs().pn_exhaustive; }

int dvq_launch_pn_filter_front(const PnBatch& in, const PnTrunkWeights& w, const PnSlot& sl, unsigned long long* stats, hipStream_t st) {
    PnGeometry g;
    DVQ_PROPAGATE(filter_geometry(in.N, &g));
    static DvqOncePerDevice attr_once[2][2];
    for (int c = 0; c < 2; ++c)
        for (int tail = 0; tail < 2; ++tail)
            DVQ_PROPAGATE(dvq_lds_limit(attr_once[c][tail], reinterpret_cast<const void*>(trunk_filter_kernel(3 + c, tail)),
                                        tail ? F_LDS_TAIL : (DVQ_DIAG_ON ? 100 * 1024 : F_LDS), "pointnet"));
    const long B = in.B, grid = B * g.deal;
    DVQ_REQUIRE(B * g.tiles < (1L << 31), "pointnet: grid too large");
    if (stats && hipMemsetAsync(stats, 0, PN_STATS_BYTES, st) != hipSuccess) {       // statistics runs only; tstat is zeroed by pn_center_kernel
        dvq_set_error("pointnet: hipMemsetAsync failed");
        return DVQ_ELAUNCH;
    }
    {
        DVQ_PROF("pn_center", 2.0 * (double)B * 4 * (4.0 * 64 + 64.0 * 128), (double)B * (64 + 512), st);
        DVQ_LAUNCH(center_kernel(in.C), dim3((unsigned)((B + CENTER_SPB - 1) / CENTER_SPB)), dim3(256), 0, st, in.pc, in.trans, in.N, B, w.w1,
                   w.b1, w.w2, w.b2, sl.cbuf, sl.tstat, g.tiles);
    }
    DVQ_CHECK_LAUNCH("pn_center");
    const double pts = (double)B * g.slots;
    const int abl = pn_abl();
    float* h2 = pn_recompute() ? nullptr : sl.h2;          // nullptr: no spill
    // one launch of the trunk kernel: the full-tile grid (a workgroup per sample and dealt tile) or the tail grid (four samples each)
    auto launch = [&](bool tail, int lds, hipStream_t s, int abl_arg) {
        DVQ_LAUNCH(trunk_filter_kernel(in.C, tail), dim3((unsigned)(tail ? (B + 3) / 4 : grid)), dim3(256), lds, s, in.pc, in.trans, in.N, g.Npad,
                   g.tiles, g.deal, B, w.w1, w.b1, w.b2, (const char*)w.w3f, h2, (f32x4*)sl.part, (qf32x2*)sl.part2, sl.tstat, sl.cbuf, abl_arg);
    };
    {
        DVQ_PROF("pn_trunk", 2.0 * pts * (4.0 * 64 + 64.0 * 128 + 128.0 * 1024), pts * (16 + (h2 ? 512 : 0)) + (double)grid * 16384, st);
#ifdef DVQ_DIAG
        if ((abl & PN_ABL_SPLIT) && in.C == 4) {
            // timing only (results INVALID): what splitting the trunk into a producer kernel (conv1 / conv2 / centring / conversion) and a
            // consumer kernel (conv3 loop) would buy if the two ran BESIDE each other: the same grid twice, the halves of the work on two streams
            static hipStream_t side = nullptr;
            static hipEvent_t ev0 = nullptr, ev1 = nullptr;
            if (!side) { (void)hipStreamCreateWithFlags(&side, hipStreamNonBlocking); (void)hipEventCreateWithFlags(&ev0, hipEventDisableTiming); (void)hipEventCreateWithFlags(&ev1, hipEventDisableTiming); }
            (void)hipEventRecord(ev0, st);
            (void)hipStreamWaitEvent(side, ev0, 0);
            launch(false, F_LDS, st, (abl & ~PN_ABL_SPLIT) | PN_ABL_NO_CONV3);
            launch(false, F_LDS, side, (abl & ~PN_ABL_SPLIT) | PN_ABL_CONSUMER | PN_ABL_NO_H2_STORE);
            (void)hipEventRecord(ev1, side);
            (void)hipStreamWaitEvent(st, ev1, 0);
            return DVQ_OK;
        }
#endif
        launch(false, (abl & PN_ABL_ONE_PER_CU) ? 100 * 1024 : F_LDS, st, abl);
        if (g.has_tail()) launch(true, F_LDS_TAIL, st, abl);
    }
    DVQ_CHECK_LAUNCH("pn_trunk_filter");
    return DVQ_OK;
}

int dvq_launch_pn_filter_back(const PnBatch& in, const PnTrunkWeights& w, const PnSlot& sl, float* feat, long ld_feat,
                              unsigned long long* stats, hipStream_t st) {
    PnGeometry g;
    DVQ_PROPAGATE(filter_geometry(in.N, &g));
    const long B = in.B;
    const int N = in.N, tiles = g.tiles;
    const unsigned* tstat = sl.tstat;
    const int abl = pn_abl();
    const DvqKnobs& kn = dvq_knobs();
    const int exhaustive = kn.pn_exhaustive;
    int pair_cap = PAIR_CAP, fb_cap = FB_CAP;              // tests shrink the lists to reach the overflow paths
    if (kn.pn_caps[0] >= 0) {
        pair_cap = kn.pn_caps[0] > PAIR_CAP ? PAIR_CAP : kn.pn_caps[0];
        fb_cap = kn.pn_caps[1] > FB_CAP ? FB_CAP : kn.pn_caps[1];
    }
    const int recompute = pn_recompute();
    {
        // rows: one read per candidate point (about 1 024 of them with repeats); recomputed rows are written first, and their points read
        DVQ_PROF("pn_exact", 2.0 * (double)B * 1024 * 128, (double)B * (tiles * 16384.0 + 1024.0 * 512 * (recompute ? 2 : 1) + 4096), st);
        DVQ_LAUNCH(exact_kernel(in.C), dim3((unsigned)B), dim3(256), 0, st, (const f32x4*)sl.part, (const qf32x2*)sl.part2, tiles, g.deal, sl.h2,
                   recompute, in.pc, in.trans, w.w1, w.b1, w.b2, (const char*)w.w3f, N, g.Npad, w.w3, w.b3, reinterpret_cast<const float*>((const char*)w.w3f + IMG_OFF_WN),
                   reinterpret_cast<const float*>((const char*)w.w3f + IMG_OFF_RN), tstat, sl.cbuf, w.relu3, exhaustive, pair_cap, fb_cap,
                   feat, ld_feat, stats, abl);
    }
    DVQ_CHECK_LAUNCH("pn_exact");
    if (stats && (abl & PN_ABL_STAMPS)) {
        const long nrec = B * tiles;                       // a tail tile's record carries its workgroup's stamps too
        std::vector<unsigned> ts((size_t)nrec * 4);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(ts.data(), tstat, ts.size() * 4, hipMemcpyDeviceToHost);
        double a = 0, b2_ = 0, c = 0, d = 0;
        for (long i = 0; i < nrec; ++i) {
            const unsigned v = ts[4 * i + 3];
            a += v & 255; b2_ += (v >> 8) & 255; c += (v >> 16) & 255; d += (v >> 24) & 255;
        }
        if (abl & PN_ABL_CLOCK) {
            double mhz = 0;
            for (long i = 0; i < nrec; ++i) mhz += ts[4 * i + 3];
            fprintf(stderr, "[dvq pn] in-kernel clock of the trunk kernel: %.0f MHz (s_memtime over s_memrealtime, mean over %ld workgroups)\n", mhz / nrec, nrec);
        } else
        fprintf(stderr, "[dvq pn] mean phase ticks per workgroup (s_memtime): start->loaded %.0f, conv1+conv2 %.0f, centre/convert %.0f, conv3 loop %.0f\n",
                a / nrec * 64, b2_ / nrec * 64, c / nrec * 64, d / nrec * 512);
    }
    if (stats) {                                          // diagnostics (DVQ_PN_STATS=1): synchronises
        unsigned long long h[PN_STATS_BYTES / 8] = {};
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h, stats, sizeof h, hipMemcpyDeviceToHost);
        (void)hipMemset((void*)stats, 0, sizeof h);
        const double tot = (double)B * 1024;
        fprintf(stderr, "[dvq pn] B=%ld N=%d: one candidate %.4f, other counts %.4f of the channels, flagged 16-point groups %.5f per channel; %.3f candidate dots per channel\n",
                B, N, h[0] / tot, h[1] / tot, h[2] / tot, h[3] / tot);
        // the non-empty slots of the point histograms + 16 per flagged group (an upper bound: a group's points may be candidates too)
        fprintf(stderr, "[dvq pn] B=%ld N=%d: distinct conv2 rows fetched per cloud <= %.1f (%.1f candidate points + 16 per flagged group)\n",
                B, N, (double)(h[8] + 16 * h[2]) / B, (double)h[8] / B);
        if (recompute)
            fprintf(stderr, "[dvq pn] B=%ld N=%d: recomputed per cloud: %.2f batches of 32 points, %.1f conv2 rows\n", B, N, (double)h[10] / B, (double)h[11] / B);
        if (abl & PN_ABL_STAMPS)
            fprintf(stderr, "[dvq pn] exact stage, mean cycles per workgroup: records -> candidates %.0f, sort by point %.0f, candidate dots %.0f, flagged groups + checks + store %.0f; of these the anchor pass %.0f\n",
                    (double)h[4] / B, (double)h[5] / B, (double)h[6] / B, (double)h[7] / B, (double)h[9] / B);
    }
    return DVQ_OK;
}

// host side of the consistency counters: [0] suspect tile records, [1] channels outside their records' interval (per device)
int dvq_pn_fault_counters(unsigned long long* out2, int reset) {
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_pn_faults), 16) != hipSuccess) {
        dvq_set_error("pointnet_fault_counters: reading the device counters failed");
        return DVQ_ELAUNCH;
    }
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_pn_faults), z, 16) != hipSuccess) {
            dvq_set_error("pointnet_fault_counters: resetting the device counters failed");
            return DVQ_ELAUNCH;
        }
    }
    return DVQ_OK;
}
