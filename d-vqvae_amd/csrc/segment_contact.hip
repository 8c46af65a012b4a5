// dvq_segment_contact: contact from the object's side -- for every point of an object's cloud, how many of the object's grasps touch
// it, how many have it inside the hand, the nearest any hand comes and the summed touching distances -- in ONE kernel.  The
// definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// grasp_scores_kernel (contact.hip) holds a hand still and walks the object points; this kernel turns the scan round: one workgroup
// of 256 threads per (segment, tile of SC_TILE = 1024 points) keeps its four points per thread still, with their accumulators in
// registers (two counts, the minimum, four chains each), and walks the segment's rows.  Per row: the hand into the LDS planes
// (grasp_load_hand), the row's validity, the normals (grasp_normals), then grasp_scan4 and grasp_inside -- the helpers of
// grasp_scan.h, so the per-point bits are those of dvq_grasp_scores.  The segment's outputs are written once at the end: no atomics
// on them, no memset, no workspace.  The normals are rebuilt once per tile and row (three times at N = 3000).
//
// Row validity needs the whole cloud, not only the tile: every tile's workgroup tests the row's cloud itself (3 N loads spread over
// 256 threads beside a scan of 4 V distance evaluations per thread: a few per cent, and no second launch whose result the first
// would have to wait for).  An invalid row is skipped before its normals are built, so the scan never sees a non-finite
// coordinate and runs with slow = false.
//
// The chain of a row is its segment position mod 4, which the whole workgroup knows: the four chains of a point are updated under a
// comparison with that number, so the accumulators stay in registers (no indexed register array).
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int SC_TILE = GRASP_THREADS * GRASP_P;            // 1024 points per workgroup (ops.SEGMENT_CONTACT_TILE)
constexpr int SC_MAX_K = 262144;                            // rows per segment (ops.SEGMENT_CONTACT_MAX_K)
constexpr int SC_MORE = 4;                                  // ints after the planes: two alternating row flags, the bad-index flag

__global__ __launch_bounds__(GRASP_THREADS) void segment_contact_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                        const int* __restrict__ vf_off, const int* __restrict__ vf_face,
                                                                        int V, const float* __restrict__ obj, long osb, long osp, long osc,
                                                                        long B, int N, const int64_t* __restrict__ rows, long o0, int K,
                                                                        float thr, int* __restrict__ touch, int* __restrict__ inside,
                                                                        float* __restrict__ dmin, float* __restrict__ near_sum,
                                                                        int* __restrict__ n_valid, int* __restrict__ row_status, int* err) {
    extern __shared__ __align__(16) float sc_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(sc_lds, V, hx, hy, hz, nx, ny, nz);
    int* flag = reinterpret_cast<int*>(sc_lds + grasp_hand_floats(V));   // [0], [1]: this row is invalid (alternating); [2]: a bad index
    const int t = threadIdx.x;
    const long o = o0 + blockIdx.y;                              // the segment
    const long p_tile = (long)blockIdx.x * SC_TILE;              // the tile's first point
    const bool first_tile = blockIdx.x == 0;                     // writes what the segment has once: n_valid, row_status, the error bit
    const int64_t* seg = rows ? rows + o * K : nullptr;
    const float nan = __uint_as_float(0x7fc00000u);

    // every entry of the segment inside [0, B), before anything is read through one
    if (t == 0) flag[2] = 0;
    dvq_lds_barrier();
    if (seg) {
        bool bad = false;
        for (int i = t; i < K; i += GRASP_THREADS) {
            const int64_t r = seg[i];
            bad |= r < 0 || r >= B;
        }
        if (bad) flag[2] = 1;
    }
    dvq_lds_barrier();
    if (flag[2] != 0) {                                          // the refusal values and the error bit
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const long p = p_tile + t + k * GRASP_THREADS;
            if (p < N) {
                touch[o * N + p] = -1;
                inside[o * N + p] = -1;
                dmin[o * N + p] = nan;
                near_sum[o * N + p] = nan;
            }
        }
        if (first_tile) {
            for (int i = t; i < K; i += GRASP_THREADS) row_status[o * K + i] = -1;
            if (t == 0) {
                n_valid[o] = -1;
                atomicOr(err, 1);
            }
        }
        return;
    }

    int n_touch[GRASP_P], n_in[GRASP_P];
    float best_d[GRASP_P], c0[GRASP_P], c1[GRASP_P], c2[GRASP_P], c3[GRASP_P];
#pragma unroll
    for (int k = 0; k < GRASP_P; ++k) {
        n_touch[k] = 0;
        n_in[k] = 0;
        best_d[k] = INFINITY;
        c0[k] = c1[k] = c2[k] = c3[k] = 0.0f;
    }
    int valid = 0;
    for (int i = 0; i < K; ++i) {                                // the segment's rows, in segment order
        const long r = seg ? (long)seg[i] : o * K + i;
        const float* ob = obj + r * osb;
        int* bad_row = flag + (i & 1);                           // alternating: a wave still reading row i - 1's flag is not disturbed
        if (t == 0) *bad_row = 0;
        dvq_lds_barrier();                                       // every wave is through with the planes of the row before
        bool odd = grasp_load_hand(hand + r * V * 3, V, t, hx, hy, hz);
        for (long p = t; p < N; p += GRASP_THREADS)              // the whole cloud of the row, not only this tile
            odd |= !grasp_finite(ob[p * osp], ob[p * osp + osc], ob[p * osp + 2 * osc]);
        if (odd) *bad_row = 1;
        dvq_lds_barrier();                                       // the vertices and the flag are published
        const bool invalid = *bad_row != 0;                      // the same for the whole workgroup
        if (first_tile && t == 0) row_status[o * K + i] = invalid ? 1 : 0;
        if (invalid) continue;
        ++valid;
        grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);
        float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P];
        int bi[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const long p = p_tile + t + k * GRASP_THREADS;
            const bool in = p < N;
            sx[k] = in ? ob[p * osp] : 0.f;
            sy[k] = in ? ob[p * osp + osc] : 0.f;
            sz[k] = in ? ob[p * osp + 2 * osc] : 0.f;
        }
        grasp_scan4(hx, hy, hz, V, false, sx, sy, sz, best, bi);
        dvq_lds_barrier();                                       // the normals are published
        const int g = i & 3;                                     // the row's chain
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const float d = best[k];
            const bool in_hand = grasp_inside(hx, hy, hz, nx, ny, nz, bi[k], sx[k], sy[k], sz[k]);
            const bool tch = d < thr;
            const float s = sqrtf(d);
            n_in[k] += in_hand ? 1 : 0;
            n_touch[k] += tch ? 1 : 0;
            best_d[k] = d < best_d[k] ? d : best_d[k];
            c0[k] = (tch && g == 0) ? c0[k] + s : c0[k];
            c1[k] = (tch && g == 1) ? c1[k] + s : c1[k];
            c2[k] = (tch && g == 2) ? c2[k] + s : c2[k];
            c3[k] = (tch && g == 3) ? c3[k] + s : c3[k];
        }
    }
#pragma unroll
    for (int k = 0; k < GRASP_P; ++k) {
        const long p = p_tile + t + k * GRASP_THREADS;
        if (p < N) {
            const float s01 = c0[k] + c1[k], s23 = c2[k] + c3[k];
            touch[o * N + p] = n_touch[k];
            inside[o * N + p] = n_in[k];
            dmin[o * N + p] = best_d[k];
            near_sum[o * N + p] = s01 + s23;
        }
    }
    if (first_tile && t == 0) n_valid[o] = valid;
}

}  // namespace

extern "C" int dvq_segment_contact(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                   const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                   int64_t B, int N, const int64_t* rows, int64_t O, int K, float contact_threshold, int32_t* touch,
                                   int32_t* inside, float* dmin, float* near_sum, int32_t* n_valid, int32_t* row_status, int32_t* err,
                                   dvq_stream_t stream) {
    DVQ_REQUIRE(O >= 0 && K >= 1 && K <= SC_MAX_K && N >= 1 && V >= 1 && V <= GRASP_MAX_V && contact_threshold > 0.0f &&
                    contact_threshold < INFINITY,
                "segment_contact: need O >= 0, 1 <= K <= %d, N >= 1, 1 <= V <= %d and a finite contact_threshold > 0 (got O=%ld K=%d "
                "N=%d V=%d contact_threshold=%g)", SC_MAX_K, GRASP_MAX_V, (long)O, K, N, V, (double)contact_threshold);
    if (O == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && touch && inside && dmin && near_sum && n_valid && row_status && err,
                "segment_contact: null pointer");
    DVQ_REQUIRE(rows || B == O * (int64_t)K, "segment_contact: without rows B must be O * K (got B=%ld O=%ld K=%d)", (long)B, (long)O, K);
    DVQ_REQUIRE(B >= 0, "segment_contact: B must be >= 0 (got %ld)", (long)B);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = grasp_lds_bytes(V, SC_MORE);
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&segment_contact_kernel), grasp_lds_bytes(GRASP_MAX_V, SC_MORE),
                                "segment_contact"));
    const unsigned tiles = (unsigned)(((long)N + SC_TILE - 1) / SC_TILE);
    dvq_for_row_chunks(O, [&](int64_t o0, int64_t no) {
        // per (row, point, vertex) 8 FLOPs as in grasp_scores, over the tile's 1024 point slots; in: per tile and row the hand, the
        // topology and the whole cloud (the validity test); out: 16 B per point, 4 B per row
        DVQ_PROF("segment_contact", 8.0 * no * K * (double)tiles * SC_TILE * V,
                 (double)no * K * tiles * ((double)(V + N) * 12) + (double)no * ((double)N * 16 + (double)K * 12 + 4), st);
        DVQ_LAUNCH(segment_contact_kernel, dim3(tiles, (unsigned)no), dim3(GRASP_THREADS), lds, st, hand, faces, vf_off, vf_face, V, obj,
                   (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, (long)B, N, rows, (long)o0, K,
                   contact_threshold, touch, inside, dmin, near_sum, n_valid, row_status, err);
    });
    DVQ_CHECK_LAUNCH("segment_contact");
    return DVQ_OK;
}
