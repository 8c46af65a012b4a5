// dvq_grasp_self: the hand against ITSELF -- for every vertex of a part its nearest vertex among the parts it is tested against, the
// interior test of grasp_scan.h against that vertex's tangent plane, and from those the per-part counts, depths, clearances and pair
// bits and a bit per vertex -- in ONE kernel, one workgroup of 256 threads per grasp.  The definition is the ABI (include/dvq.h); this
// file only says how the kernel is laid out.
//
// The six planes of grasp_scan.h hold the hand and its normals (its loaders, unchanged); a seventh plane holds every vertex's part bit
// as a TARGET (1u << label, 0 = no part; the padding up to VP is 0).  Every thread keeps four SOURCE vertices (v0 + t + 256 k) in
// registers with the word of parts each is tested against (pairs[label]; 0 for a slot beyond V, an unlabelled vertex or one that is
// no source: such a slot meets no target) and scans the planes sixteen bytes at a time: the walk of grasp_scan.h with one AND and one
// select more per pair -- a target that is not allowed contributes +inf, which is never below the running best.  A hand of more than
// 1024 vertices takes a second pass.
//
// Per-part results are LDS atomics on integers and on the integer image of non-negative floats (min / max / add / or): no float sum,
// no order to fix.  The mask words come from wave ballots (the 64 lanes of a wave hold 64 consecutive vertices: two words).
//
// A row with a non-finite coordinate has no figure: the flag the hand's load sets is final after the barrier that publishes the
// planes, and the whole workgroup takes the status = 1 exit before the normals and before any scan.  With every coordinate finite no
// distance is a NaN (a difference may overflow to +-inf, its square is +inf), so the walk of grasp_scan.h is the whole scan; a
// source all of whose targets lie at +inf takes the lowest target after the scan (the minimum is +inf, attained by every target).
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GSELF_SLOTS = GRASP_THREADS * GRASP_P;        // 1024 source vertices per pass over the planes
constexpr int GSELF_MAX_P = 32;                             // parts: one bit each (ops.GRASP_SELF_MAX_P)
constexpr int GSELF_ROWS = 5;                               // rows of 32 after the seventh plane: pairs, counts, depths, gaps, pair bits
static_assert(GSELF_SLOTS % 64 == 0 && GRASP_MAX_V % 32 == 0, "a wave's ballot is two whole mask words");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct SelfPairs {
    unsigned w[GSELF_MAX_P];                                // bit b of w[a]: part a's vertices are tested against part b
};

// floats after the six planes: the seventh, the parts' rows, the flag
__host__ __device__ constexpr int gself_more_floats(int V) { return grasp_vp(V) + GSELF_ROWS * GSELF_MAX_P + 4; }

// The part of vertex v as a SOURCE: its label if that lies in [0, P) and the vertex may count, else -1 (also beyond V).
__device__ __forceinline__ int src_label(const int* __restrict__ part_of_vertex, const int* __restrict__ source_of_vertex, int V, int P,
                                         int v) {
    if (v >= V) return -1;
    const int l = part_of_vertex[v];
    return (l >= 0 && l < P && source_of_vertex[v] != 0) ? l : -1;
}

// The walk's aux: vertex j's part bit as a target.
struct SelfTargets {
    const unsigned* tb;
    __device__ __forceinline__ u32x4 load4(int j) const { return *reinterpret_cast<const u32x4*>(tb + j); }
    __device__ __forceinline__ unsigned at(u32x4 T, int u) const { return T[u]; }
    __device__ __forceinline__ unsigned load1(int j) const { return tb[j]; }
};

// amdgpu_waves_per_eu(6): left to itself the scheduler spends 101 VGPRs on the scan (four waves per SIMD); asked for the siblings' six
// waves it needs 53 and spills nothing.
__global__ __launch_bounds__(GRASP_THREADS) __attribute__((amdgpu_waves_per_eu(6))) void grasp_self_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                   const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                                                   const int* __restrict__ part_of_vertex,
                                                                   const int* __restrict__ source_of_vertex, int P, SelfPairs pairs,
                                                                   float reach2, float margin, int* __restrict__ pen_count,
                                                                   float* __restrict__ pen_depth, float* __restrict__ gap_min,
                                                                   int* __restrict__ pair_bits, int* __restrict__ mask,
                                                                   int* __restrict__ status) {
    extern __shared__ __align__(16) float gself_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gself_lds, V, hx, hy, hz, nx, ny, nz);
    const int VP = grasp_vp(V);
    unsigned* tb = reinterpret_cast<unsigned*>(gself_lds + grasp_hand_floats(V));   // [VP] the seventh plane: the target's part bit
    unsigned* pw = tb + VP;                                      // [32] pairs
    int* cnt = reinterpret_cast<int*>(pw + GSELF_MAX_P);         // [32] penetrating vertices
    unsigned* dep = reinterpret_cast<unsigned*>(cnt + GSELF_MAX_P);   // [32] the largest depth (> margin >= 0: its integer image orders it)
    unsigned* gap = dep + GSELF_MAX_P;                           // [32] the smallest d (>= +0.0)
    unsigned* pb = gap + GSELF_MAX_P;                            // [32] OR of the targets' part bits
    int* flag = reinterpret_cast<int*>(pb + GSELF_MAX_P);        // [1]: a coordinate of the row is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const int W = (V + 31) >> 5;
    if (t == 0) *flag = 0;
    if (t < GSELF_MAX_P) {
        pw[t] = t < P ? pairs.w[t] : 0u;
        cnt[t] = 0;
        dep[t] = 0u;                                             // +0.0f
        gap[t] = 0x7f800000u;                                    // +inf
        pb[t] = 0u;
    }
    for (int i = t; i < VP; i += GRASP_THREADS) {
        const int l = i < V ? part_of_vertex[i] : -1;
        tb[i] = (l >= 0 && l < P) ? 1u << l : 0u;
    }
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) *flag = 1;
    dvq_lds_barrier();
    if (*flag != 0) {                                            // the whole workgroup: no figure
        if (t < P) {
            pen_count[b * P + t] = -1;
            pen_depth[b * P + t] = NAN;
            gap_min[b * P + t] = NAN;
            pair_bits[b * P + t] = 0;
        }
        for (int w = t; w < W; w += GRASP_THREADS) mask[b * W + w] = 0;
        if (t == 0) status[b] = 1;
        return;
    }
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);
    dvq_lds_barrier();
    for (int v0 = 0; v0 < V; v0 += GSELF_SLOTS) {                // sources v0 + t + 256 k: one pass over the planes
        float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P];
        f32x4 best;                                              // (vectors, updated by element: grasp_walk4's comment)
        i32x4 bi;
        unsigned am[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int v = v0 + t + k * GRASP_THREADS;
            const bool in = v < V;
            const int vv = in ? v : 0;
            sx[k] = hx[vv];
            sy[k] = hy[vv];
            sz[k] = hz[vv];
            const int l = src_label(part_of_vertex, source_of_vertex, V, P, v);   // a label outside [0, P): no part
            am[k] = l >= 0 ? pw[l] : 0u;
            best[k] = INFINITY;
            bi[k] = -1;
        }
        grasp_walk4(hx, hy, hz, V, sx, sy, sz, SelfTargets{tb}, [&](int k, int j, float d, unsigned T) {
            const float da = (T & am[k]) ? d : INFINITY;
            const bool better = da < best[k];
            best[k] = better ? da : best[k];
            bi[k] = better ? j : bi[k];
        });
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            if (bi[k] < 0 && am[k] != 0u) {                      // every target at +inf (or none in the hand): the lowest target, if any
                for (int j = 0; j < V; ++j) {
                    if (tb[j] & am[k]) {
                        bi[k] = j;
                        break;
                    }
                }
            }
            bool pen = false;
            const int lab = src_label(part_of_vertex, source_of_vertex, V, P, v0 + t + k * GRASP_THREADS);   // read again: not kept across the scan
            if (lab >= 0) {
                atomicMin(&gap[lab], __float_as_uint(best[k]));
                if (bi[k] >= 0) {
                    const int j = bi[k];
                    const float wx = hx[j] - sx[k], wy = hy[j] - sy[k], wz = hz[j] - sz[k];
                    const float depth = fmaf(wz, nz[j], fmaf(wy, ny[j], wx * nx[j]));   // grasp_inside's expression
                    pen = best[k] < reach2 && depth > margin;
                    if (pen) {
                        atomicAdd(&cnt[lab], 1);
                        atomicMax(&dep[lab], __float_as_uint(depth));
                        atomicOr(&pb[lab], tb[j]);
                    }
                }
            }
            const unsigned long long bits = __ballot(pen);       // the wave's 64 vertices: two mask words
            if ((t & 63) == 0) {
                const int w = (v0 + k * GRASP_THREADS + t) >> 5;
                if (w < W) mask[b * W + w] = (int)(unsigned)(bits & 0xffffffffull);
                if (w + 1 < W) mask[b * W + w + 1] = (int)(unsigned)(bits >> 32);
            }
        }
    }
    dvq_lds_barrier();
    if (t < P) {
        pen_count[b * P + t] = cnt[t];
        pen_depth[b * P + t] = __uint_as_float(dep[t]);
        gap_min[b * P + t] = __uint_as_float(gap[t]);
        pair_bits[b * P + t] = (int)pb[t];
    }
    if (t == 0) status[b] = 0;
}

}  // namespace

extern "C" int dvq_grasp_self(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                              const int32_t* part_of_vertex, const int32_t* source_of_vertex, int P, const uint32_t* pairs, int64_t B,
                              float reach2, float margin, int32_t* pen_count, float* pen_depth, float* gap_min, int32_t* pair_bits,
                              int32_t* mask, int32_t* status, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && V >= 1 && V <= GRASP_MAX_V && P >= 1 && P <= GSELF_MAX_P,
                "grasp_self: need B >= 0, 1 <= V <= %d, 1 <= P <= %d (got B=%ld V=%d P=%d)", GRASP_MAX_V, GSELF_MAX_P, (long)B, V, P);
    DVQ_REQUIRE(reach2 > 0.0f && reach2 < INFINITY && margin >= 0.0f && margin < INFINITY,
                "grasp_self: reach2 must be finite and positive, margin finite and >= 0 (got %g, %g)", (double)reach2, (double)margin);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && part_of_vertex && source_of_vertex && pairs && pen_count && pen_depth && gap_min &&
                    pair_bits && mask && status,
                "grasp_self: null pointer");
    SelfPairs pw = {};
    for (int a = 0; a < P; ++a) {
        const uint32_t w = pairs[a];
        DVQ_REQUIRE(!((w >> a) & 1u), "grasp_self: pairs[%d] tests part %d against itself", a, a);
        DVQ_REQUIRE(P == 32 || (w >> P) == 0u, "grasp_self: pairs[%d] = 0x%x names a part at or above P = %d", a, (unsigned)w, P);
        pw.w[a] = w;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t W = (V + 31) / 32;
    const size_t lds = grasp_lds_bytes(V, gself_more_floats(V));
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_self_kernel),
                                grasp_lds_bytes(GRASP_MAX_V, gself_more_floats(GRASP_MAX_V)), "grasp_self"));
    const double slots = (double)((V + GSELF_SLOTS - 1) / GSELF_SLOTS) * GSELF_SLOTS;
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // per (source slot, target) pair 8 FLOPs as in grasp_scores; in: the hand, the labels and the topology once per grasp; out: the
        // parts' four rows, the mask, the status
        DVQ_PROF("grasp_self", 8.0 * nb * V * slots, (double)nb * (12.0 * V + 8.0 * V + 16.0 * P + 4.0 * W + 4), st);
        DVQ_LAUNCH(grasp_self_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   part_of_vertex, source_of_vertex, P, pw, reach2, margin, pen_count + b0 * P, pen_depth + b0 * P, gap_min + b0 * P,
                   pair_bits + b0 * P, mask + b0 * W, status + b0);
    });
    DVQ_CHECK_LAUNCH("grasp_self");
    return DVQ_OK;
}
