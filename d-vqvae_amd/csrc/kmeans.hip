// dvq_segment_kmeans: Lloyd's k-means inside each segment of M rows -- the definition is the ABI text of include/dvq.h.  One
// workgroup of 256 threads per segment, the whole loop in one launch; no workspace; nothing depends on O or on scheduling.
#include "dvq_internal.h"

// Every difference, product and sum below is rounded on its own (see diverse.hip: plain operators under this pragma).
#pragma clang fp contract(off)

namespace {

constexpr int KM_T = 256;                   // threads, and rows per tile
constexpr int KM_MAX_K = 64;
constexpr int KM_MAX_D = 64;
constexpr int KM_MAX_M = 262144;            // ops.SEGMENT_KMEANS_MAX_M
constexpr int KM_HDR = 528;                 // floats in front of the arrays: flags [4][4], counts [4][64], the tile's assignments [256]
constexpr int KM_LDS_FLOATS = 40960;        // 160 KiB: what one workgroup may hold on gfx950

__device__ __forceinline__ bool km_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void km_step(float& acc, float a, float b) {
    const float t = a - b;
    const float q = t * t;
    acc = acc + q;
}

// d(x, c) of dvq.h with the row in registers and the centre in LDS (every lane reads the same address: a broadcast).  Both are
// zero-padded from D to DP: a padded element adds (+0 - +0)^2 = +0.0 to a sum that is never -0.0, which leaves its bits alone.
template <int DP>
__device__ __forceinline__ float km_dist(const float (&x)[DP], const float* c) {
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < DP; j += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(c + j);
        km_step(acc[j & 7], x[j], v[0]);
        km_step(acc[(j + 1) & 7], x[j + 1], v[1]);
        km_step(acc[(j + 2) & 7], x[j + 2], v[2]);
        km_step(acc[(j + 3) & 7], x[j + 3], v[3]);
    }
    const float s01 = acc[0] + acc[1], s23 = acc[2] + acc[3], s45 = acc[4] + acc[5], s67 = acc[6] + acc[7];
    const float lo = s01 + s23, hi = s45 + s67;
    return lo + hi;
}

// OR of a per-thread predicate over the workgroup through four LDS words (one barrier)
__device__ __forceinline__ bool km_any(bool p, int* slot, int lane, int wave) {
    const bool w = __ballot(p) != 0;
    if (lane == 0) slot[wave] = w ? 1 : 0;
    dvq_lds_barrier();
    return (slot[0] | slot[1] | slot[2] | slot[3]) != 0;
}

// One pass over the segment does both halves of a Lloyd step on a tile of 256 rows held in LDS: thread r assigns row r to its
// nearest centre, then thread (g = wave, j = lane) adds feature j of the tile's rows r = g (mod 4), in ascending order, to its own
// accumulator of the row's centre -- the sums the NEXT centres are made of, and, in lane c, the count of centre c in chain g.
// The tile sits at the odd stride DP + 1: 64 lanes on element j of 64 rows, and 64 lanes on 64 elements of one row, hit 64 banks.
template <int DP>
__global__ __launch_bounds__(KM_T) void segment_kmeans_kernel(const float* __restrict__ feat, long ld, int D,
                                                              const int64_t* __restrict__ init, int M, int k, int iters,
                                                              float* __restrict__ centres, int* __restrict__ counts,
                                                              int* __restrict__ assign, float* __restrict__ dist,
                                                              int* __restrict__ iters_used, int* err) {
    extern __shared__ __attribute__((aligned(16))) float km_lds[];
    constexpr int S = DP + 1;
    int* flag_s = reinterpret_cast<int*>(km_lds);                 // [4][4]: bad init, invalid init row, changed (two alternating)
    int* cnt_s = reinterpret_cast<int*>(km_lds + 16);             // [4][64]: chain g's count of centre c
    int* asg_s = reinterpret_cast<int*>(km_lds + 16 + 256);       // [256]: the tile's assignments
    float* cen = km_lds + KM_HDR;                                 // [k][DP], zero-padded
    float* acc = cen + k * DP;                                    // [k][4][64]: centre c, chain g, feature j
    float* tile = acc + k * 256;                                  // [256][S]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long o = blockIdx.x;
    const int64_t* in = init + o * k;
    const float* fo = feat + o * M * ld;
    int* asg = assign + o * M;
    float* dst = dist + o * M;
    const float nan = __uint_as_float(0x7fc00000u);

    // init: every entry inside [0, M) and no two equal, before any row is read; then the k rows themselves must be valid
    bool bad = false;
    if (t < k) {
        const int64_t c = in[t];
        bad = c < 0 || c >= M;
        for (int q = 0; q < k; ++q) bad |= q != t && in[q] == c;
    }
    bad = km_any(bad, flag_s, lane, wave);
    if (!bad) {
        for (int e = t; e < k * DP; e += KM_T) {
            const int c = e / DP, j = e % DP;
            cen[e] = j < D ? fo[in[c] * ld + j] : 0.0f;
        }
        dvq_lds_barrier();
        bool inval = false;
        if (t < k)
            for (int j = 0; j < D; ++j) inval |= !km_finite(cen[t * DP + j]);
        bad = km_any(inval, flag_s + 4, lane, wave);
    }
    if (bad) {                                                     // the error flag and a defined result
        for (int i = t; i < M; i += KM_T) {
            asg[i] = -1;
            dst[i] = nan;
        }
        for (int e = t; e < k * D; e += KM_T) centres[o * k * D + e] = nan;
        if (t < k) counts[o * k + t] = -1;
        if (t == 0) {
            iters_used[o] = -1;
            atomicOr(err, 1);
        }
        return;
    }

    int used = iters;
    for (int p = 0;; ++p) {                                        // pass p assigns with the centres of update p
        for (int c = 0; c < k; ++c) acc[(c * 4 + wave) * 64 + lane] = 0.0f;      // this thread's own accumulators
        int cnt = 0;
        bool chg = false;
        for (int base = 0; base < M; base += KM_T) {
            const int rows = M - base < KM_T ? M - base : KM_T;
#pragma unroll 8
            for (int e = t; e < KM_T * DP; e += KM_T) {            // the tile, coalesced; zero beyond D and beyond the segment
                const int r = e / DP, j = e % DP;
                float v = 0.0f;
                if (j < D && r < rows) v = fo[(long)(base + r) * ld + j];
                tile[r * S + j] = v;
            }
            dvq_lds_barrier();
            if (t < rows) {
                float x[DP];
                bool ok = true;
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    x[j] = tile[t * S + j];
                    ok &= km_finite(x[j]);
                }
                int best = -1;
                float bd = nan;
                if (ok) {
                    best = 0;
                    bd = km_dist<DP>(x, cen);
                    for (int c = 1; c < k; ++c) {
                        const float d = km_dist<DP>(x, cen + c * DP);
                        if (d < bd || (bd != bd && d == d)) {
                            best = c;
                            bd = d;
                        }
                    }
                }
                if (p > 0) chg |= asg[base + t] != best;           // this thread's own store of the pass before
                asg[base + t] = best;
                dst[base + t] = bd;
                asg_s[t] = best;
            }
            dvq_lds_barrier();
            for (int r = wave; r < rows; r += 4) {
                const int c = asg_s[r];
                if (c >= 0) {
                    cnt += c == lane ? 1 : 0;
                    if (lane < D) {
                        float* a = acc + (c * 4 + wave) * 64 + lane;
                        const float v = tile[r * S + lane];
                        *a = *a + v;
                    }
                }
            }
            dvq_lds_barrier();                                     // the tile and its assignments are free again
        }
        cnt_s[t] = cnt;
        const bool changed = km_any(chg, flag_s + 8 + (p & 1) * 4, lane, wave);   // also publishes cnt_s and acc
        if (p > 0 && !changed) {
            used = p;
            break;
        }
        if (p == iters) break;
        for (int e = t; e < k * DP; e += KM_T) {                   // update: centre c, feature j
            const int c = e / DP, j = e % DP;
            const int n = (cnt_s[c] + cnt_s[64 + c]) + (cnt_s[128 + c] + cnt_s[192 + c]);
            if (j < D && n > 0) {
                const float* a = acc + c * 256 + j;
                const float s01 = a[0] + a[64], s23 = a[128] + a[192];
                const float s = s01 + s23;
                cen[e] = s / (float)n;
            }
        }
        dvq_lds_barrier();
    }
    for (int e = t; e < k * D; e += KM_T) centres[o * k * D + e] = cen[(e / D) * DP + e % D];
    if (t < k) counts[o * k + t] = (cnt_s[t] + cnt_s[64 + t]) + (cnt_s[128 + t] + cnt_s[192 + t]);
    if (t == 0) iters_used[o] = used;
}

template <int DP>
int km_launch(const float* feat, long ld, int D, const int64_t* init, int64_t O, int M, int k, int iters, float* centres,
              int32_t* counts, int32_t* assign, float* dist, int32_t* iters_used, int32_t* err, hipStream_t st) {
    const size_t floats = (size_t)KM_HDR + (size_t)k * DP + (size_t)k * 256 + (size_t)KM_T * (DP + 1);
    if (floats > (size_t)KM_LDS_FLOATS) {
        dvq_set_error("segment_kmeans: %zu floats of LDS", floats);
        return DVQ_EINVAL;
    }
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&segment_kmeans_kernel<DP>), (size_t)KM_LDS_FLOATS * 4,
                                "segment_kmeans"));
    DVQ_LAUNCH((segment_kmeans_kernel<DP>), dim3((unsigned)O), dim3(KM_T), floats * 4, st, feat, ld, D, init, M, k, iters, centres,
               counts, assign, dist, iters_used, err);
    return DVQ_OK;
}

}  // namespace

extern "C" int dvq_segment_kmeans(const float* feat, int64_t ld, int D, const int64_t* init, int64_t O, int M, int k, int iters,
                                  float* centres, int32_t* counts, int32_t* assign, float* dist, int32_t* iters_used, int32_t* err,
                                  dvq_stream_t stream) {
    DVQ_REQUIRE(O >= 0 && k >= 1 && k <= KM_MAX_K && k <= M && M <= KM_MAX_M && D >= 1 && D <= KM_MAX_D && ld >= D && iters >= 0,
                "segment_kmeans: need O >= 0, 1 <= k <= %d, k <= M <= %d, 1 <= D <= %d, ld >= D, iters >= 0 (got O=%ld M=%d k=%d D=%d "
                "ld=%ld iters=%d)", KM_MAX_K, KM_MAX_M, KM_MAX_D, (long)O, M, k, D, (long)ld, iters);
    if (O == 0) return DVQ_OK;
    DVQ_REQUIRE(feat && init && centres && counts && assign && dist && iters_used && err, "segment_kmeans: null pointer");
    DVQ_REQUIRE(O <= 0x7fffffffLL, "segment_kmeans: O too large");
    hipStream_t st = (hipStream_t)stream;
    // an upper bound: iters + 1 passes, each reading every row once and taking 3 FLOPs per (row, centre, feature) and one per (row, feature)
    const double passes = (double)iters + 1.0, rows = (double)O * M;
    DVQ_PROF("segment_kmeans", passes * rows * D * (3.0 * k + 1.0), passes * rows * ((double)D * 4 + 8) + (double)O * k * (D + 1) * 4, st);
    int rc;
    if (D <= 8)
        rc = km_launch<8>(feat, (long)ld, D, init, O, M, k, iters, centres, counts, assign, dist, iters_used, err, st);
    else if (D <= 16)
        rc = km_launch<16>(feat, (long)ld, D, init, O, M, k, iters, centres, counts, assign, dist, iters_used, err, st);
    else if (D <= 32)
        rc = km_launch<32>(feat, (long)ld, D, init, O, M, k, iters, centres, counts, assign, dist, iters_used, err, st);
    else
        rc = km_launch<64>(feat, (long)ld, D, init, O, M, k, iters, centres, counts, assign, dist, iters_used, err, st);
    DVQ_PROPAGATE(rc);
    DVQ_CHECK_LAUNCH("segment_kmeans");
    return DVQ_OK;
}
