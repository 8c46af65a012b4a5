// dvq_segment_diverse: greedy farthest-point (k-centre) selection inside each object's quality pool -- the definition is the ABI
// text of include/dvq.h.  One workgroup of 256 threads per object; no workspace; nothing depends on O or on scheduling.
#include "dvq_internal.h"

// Every product, difference and sum below is rounded on its own: plain operators, one per statement, under this pragma -- no fused
// multiply-add in the listing with the compiler's default (-ffp-contract=fast-honor-pragmas), with =on and with =off (the Makefile's).
// __fmul_rn / __fadd_rn / __fsub_rn would NOT do: they are plain operators inside a header, outside the pragma's reach, and fuse
// under the default (seen in the listing).  An explicit -ffp-contract=fast overrides every pragma; the bitwise GPU tests catch it.
#pragma clang fp contract(off)

namespace {

constexpr int DIV_T = 256;
constexpr int DIV_MAX = 4096;               // M, P and D
constexpr int DIV_HDR = 32;                 // floats in front of the arrays: the waves' winners [2][4] (64 B), the pool check [4]
constexpr int DIV_LDS_FLOATS = 40960;       // 160 KiB: what one workgroup may hold on gfx950 (ops.SEGMENT_DIVERSE_LDS_FLOATS)

__device__ __forceinline__ bool div_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void div_step(float& acc, float a, float b) {
    const float t = a - b;
    const float q = t * t;
    acc = acc + q;
}

// eight consecutive floats of a row; W floats per load (the caller has checked the alignment W needs)
template <int W>
__device__ __forceinline__ void div_load8(const float* __restrict__ a, float (&x)[8]) {
    if constexpr (W == 4) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(a), v = *reinterpret_cast<const f32x4*>(a + 4);
        x[0] = u[0], x[1] = u[1], x[2] = u[2], x[3] = u[3], x[4] = v[0], x[5] = v[1], x[6] = v[2], x[7] = v[3];
    } else if constexpr (W == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2 u = *reinterpret_cast<const float2*>(a + 2 * k);
            x[2 * k] = u.x, x[2 * k + 1] = u.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = a[k];
    }
}

// d(a, b) of dvq.h: eight chains acc[j mod 8] over ascending j, combined ((0+1)+(2+3)) + ((4+5)+(6+7))
template <int W>
__device__ __forceinline__ float div_dist(const float* __restrict__ a, const float* __restrict__ b, int D) {
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int j = 0;
#pragma unroll 2
    for (; j + 8 <= D; j += 8) {
        float x[8];
        div_load8<W>(a + j, x);
#pragma unroll
        for (int k = 0; k < 8; ++k) div_step(acc[k], x[k], b[j + k]);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k)                                   // j is a multiple of 8: element j + k belongs to chain k
        if (j + k < D) div_step(acc[k], a[j + k], b[j + k]);
    const float s01 = acc[0] + acc[1], s23 = acc[2] + acc[3], s45 = acc[4] + acc[5], s67 = acc[6] + acc[7];
    const float lo = s01 + s23, hi = s45 + s67;
    return lo + hi;
}

template <int W>
__device__ __forceinline__ bool div_valid(const float* __restrict__ a, int D) {
    bool ok = true;
    int j = 0;
    for (; j + 8 <= D; j += 8) {
        float x[8];
        div_load8<W>(a + j, x);
#pragma unroll
        for (int k = 0; k < 8; ++k) ok &= div_finite(x[k]);
    }
    for (; j < D; ++j) ok &= div_finite(a[j]);
    return ok;
}

// Per pool position i one float of state m, touched by the owning thread (i mod 256) only:
//   -2    picked;   NaN   an invalid row, or a valid one whose distance to pick 0 is NaN: key -1;   otherwise mind[i] >= +0.0
// The argmax word: key bits in the high half (picked 0, key -1 -> 1, a distance -> its bits with the sign bit set: monotone for
// non-negative floats, +inf included), 4095 - position in the low half, so that a plain unsigned max is the documented order.
//
// RESIDENT: the P pooled rows sit in LDS at an odd stride S (64 lanes on element j of 64 rows: 64 banks; the pick's row is a
// broadcast); one barrier per step (the winners' slots alternate).  Otherwise every step copies the pick's row into LDS (two
// alternating buffers of S floats) and each thread reads its own rows from global memory, W floats per load: two barriers per step.
template <bool RESIDENT, int W>
__global__ __launch_bounds__(DIV_T) void segment_diverse_kernel(const float* __restrict__ feat, long ld, int D,
                                                                const int64_t* __restrict__ pool, int M, int P, int keep, int S,
                                                                int64_t* __restrict__ sel, int* __restrict__ rank,
                                                                float* __restrict__ gap, int* err) {
    extern __shared__ __attribute__((aligned(16))) float div_lds[];
    unsigned long long* win = reinterpret_cast<unsigned long long*>(div_lds);
    int* bad_s = reinterpret_cast<int*>(div_lds + 16);
    float* m_s = div_lds + DIV_HDR;
    float* rows = m_s + ((P + 3) & ~3);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long o = blockIdx.x;
    const int64_t* pl = pool + o * P;
    const float* fo = feat + o * M * ld;

    // a pool entry outside [0, M): the error flag and a defined result (-1 everywhere), before any row is read
    bool bad = false;
    for (int i = t; i < P; i += DIV_T) {
        const int64_t c = pl[i];
        bad |= c < 0 || c >= M;
    }
    const bool wave_bad = __ballot(bad) != 0;
    if (lane == 0) bad_s[wave] = wave_bad ? 1 : 0;
    dvq_lds_barrier();
    if (bad_s[0] | bad_s[1] | bad_s[2] | bad_s[3]) {
        for (int r = t; r < keep; r += DIV_T) {
            sel[o * keep + r] = -1;
            rank[o * keep + r] = -1;
            gap[o * keep + r] = -1.0f;
        }
        if (t == 0) atomicOr(err, 1);
        return;
    }

    if (RESIDENT) {
        const int total = P * D;
        for (int e = t; e < total; e += DIV_T) {
            const int i = e / D, j = e - i * D;
            rows[i * S + j] = fo[pl[i] * ld + j];
        }
        dvq_lds_barrier();
    }
    for (int i = t; i < P; i += DIV_T) {
        const bool ok = RESIDENT ? div_valid<1>(rows + i * S, D) : div_valid<W>(fo + pl[i] * ld, D);
        m_s[i] = ok ? 0.0f : __uint_as_float(0x7fc00000u);
    }

    int p = 0;
    float g = -1.0f;
    for (int r = 0;; ++r) {
        if (t == 0) {
            sel[o * keep + r] = pl[p];
            rank[o * keep + r] = p;
            gap[o * keep + r] = g;
        }
        if (r + 1 == keep) break;
        const float* b;
        if (RESIDENT) {
            b = rows + p * S;
        } else {
            float* buf = rows + (r & 1) * S;
            const float* src = fo + pl[p] * ld;
            for (int j = t; j < D; j += DIV_T) buf[j] = src[j];
            dvq_lds_barrier();
            b = buf;
        }
        unsigned long long best = 0;
        for (int i = t; i < P; i += DIV_T) {
            float m = m_s[i];
            if (i == p) {
                m = -2.0f;
            } else if (m >= 0.0f) {                                // neither picked nor NaN
                const float d = RESIDENT ? div_dist<1>(rows + i * S, b, D) : div_dist<W>(fo + pl[i] * ld, b, D);
                m = (r == 0 || d < m) ? d : m;
            }
            m_s[i] = m;
            const unsigned hi = (m != m) ? 1u : (m < 0.0f ? 0u : (__float_as_uint(m) | 0x80000000u));
            const unsigned long long w = ((unsigned long long)hi << 32) | (unsigned)(DIV_MAX - 1 - i);
            best = w > best ? w : best;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned long long x = __shfl_xor(best, s, 64);
            best = x > best ? x : best;
        }
        unsigned long long* slot = win + (r & 1) * 4;
        if (lane == 0) slot[wave] = best;
        dvq_lds_barrier();
        const unsigned long long a0 = slot[0], a1 = slot[1], a2 = slot[2], a3 = slot[3];
        const unsigned long long b0 = a0 > a1 ? a0 : a1, b1 = a2 > a3 ? a2 : a3;
        const unsigned long long top = b0 > b1 ? b0 : b1;
        p = DIV_MAX - 1 - (int)(unsigned)(top & 0xffffffffull);
        const unsigned hi = (unsigned)(top >> 32);
        g = (hi & 0x80000000u) ? __uint_as_float(hi & 0x7fffffffu) : -1.0f;
    }
}

template <int W>
int launch_streaming(const float* feat, long ld, int D, const int64_t* pool, int64_t O, int M, int P, int keep, int64_t* sel,
                     int32_t* rank, float* gap, int32_t* err, hipStream_t st) {
    const int S = (D + 3) & ~3;
    const size_t lds = (size_t)(DIV_HDR + ((P + 3) & ~3) + 2 * S) * 4;        // at most 49 280 B
    DVQ_LAUNCH((segment_diverse_kernel<false, W>), dim3((unsigned)O), dim3(DIV_T), lds, st, feat, ld, D, pool, M, P, keep, S, sel, rank,
               gap, err);
    return DVQ_OK;
}

}  // namespace

extern "C" int dvq_segment_diverse(const float* feat, int64_t ld, int D, const int64_t* pool, int64_t O, int M, int P, int keep,
                                   int64_t* sel, int32_t* rank, float* gap, int32_t* err, dvq_stream_t stream) {
    DVQ_REQUIRE(O >= 0 && keep >= 1 && keep <= P && P <= M && M <= DIV_MAX && D >= 1 && D <= DIV_MAX && ld >= D,
                "segment_diverse: need O >= 0, 1 <= keep <= P <= M <= %d, 1 <= D <= %d, ld >= D (got O=%ld M=%d P=%d keep=%d D=%d ld=%ld)",
                DIV_MAX, DIV_MAX, (long)O, M, P, keep, D, (long)ld);
    if (O == 0) return DVQ_OK;
    DVQ_REQUIRE(feat && pool && sel && rank && gap && err, "segment_diverse: null pointer");
    DVQ_REQUIRE(O <= 0x7fffffffLL, "segment_diverse: O too large");
    hipStream_t st = (hipStream_t)stream;
    const double flops = 3.0 * (double)O * keep * P * D, out_bytes = (double)O * ((double)P * 8 + (double)keep * 16);
    const int S = D | 1;
    const long need = DIV_HDR + ((P + 3) & ~3) + (long)P * S;
    if (need <= DIV_LDS_FLOATS) {
        static DvqOncePerDevice attr_once;
        DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&segment_diverse_kernel<true, 1>), (size_t)DIV_LDS_FLOATS * 4,
                                    "segment_diverse"));
        DVQ_PROF("segment_diverse", flops, (double)O * P * D * 4 + out_bytes, st);           // every pooled row once
        DVQ_LAUNCH((segment_diverse_kernel<true, 1>), dim3((unsigned)O), dim3(DIV_T), (size_t)need * 4, st, feat, (long)ld, D, pool, M, P,
                   keep, S, sel, rank, gap, err);
    } else {
        // the validity pass and keep - 1 steps read every pooled row (L2-resident); each step reads the pick's row once more
        DVQ_PROF("segment_diverse", flops, (double)O * keep * ((double)P + 1) * D * 4 + out_bytes, st);
        if (dvq_aligned16(feat) && ld % 4 == 0)
            launch_streaming<4>(feat, (long)ld, D, pool, O, M, P, keep, sel, rank, gap, err, st);
        else if ((reinterpret_cast<uintptr_t>(feat) & 7) == 0 && ld % 2 == 0)
            launch_streaming<2>(feat, (long)ld, D, pool, O, M, P, keep, sel, rank, gap, err, st);
        else
            launch_streaming<1>(feat, (long)ld, D, pool, O, M, P, keep, sel, rank, gap, err, st);
    }
    DVQ_CHECK_LAUNCH("segment_diverse");
    return DVQ_OK;
}
