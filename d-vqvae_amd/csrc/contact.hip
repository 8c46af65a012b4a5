// Contact / penetration proxies after the generation path: the reference's
// utils/utils_loss.py:7-45 (get_NN, get_interior) and the penetration term of utils/loss.py:144-160 (TTT_loss).
//
//   nn_points    : for every source point the nearest target point of the same batch element -- squared distance and
//                  index.  The reference calls pytorch3d.ops.knn_points(K=1) (third-party, absent here): brute force
//                  over all targets.  Canonical arithmetic of this build: dx = s.x - t.x (fp32), d = fma(dz, dz,
//                  fma(dy, dy, dx * dx)); first minimum wins, a NaN distance beats everything (torch.argmin order,
//                  as in vq_argmin).  Bit-exact against oracle/contact_oracle.py.
//   vertex_normals: area-weighted vertex normals of a triangle mesh shared by the batch (MANO: 778 verts, 1538 faces):
//                  n_v = sum over the faces incident to v, in ascending face order, of cross(v1 - v0, v2 - v0);
//                  normalised with max(|n|, 1e-6).  (pytorch3d's Meshes.verts_normals_packed accumulates the same
//                  vectors with three atomics-based index_add calls, i.e. in no fixed order; this order is fixed.)
//   interior     : (hand[nn] - obj) . normal[nn] > 0   (utils_loss.py:27-45).
//
// One workgroup per (batch element, 256 source points); the element's target cloud sits in LDS as x|y|z planes and is
// read by broadcast (all lanes the same address), so the loop is pure vector work: HBM traffic is the algorithmic
// (N1 + N2) * 12 B in, N1 * 12 B out per element.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int NN_MAX_TRG = 4096;            // 48 KB of LDS

__global__ __launch_bounds__(256) void nn_points_kernel(const float* __restrict__ src, long ssb, long ssp, long ssc,
                                                        const float* __restrict__ trg, long tsb, long tsp, long tsc,
                                                        int N1, int N2, float* __restrict__ dist, int64_t* __restrict__ idx) {
    extern __shared__ float t_s[];                               // [3][N2]
    const long b = blockIdx.y;
    const float* tb = trg + b * tsb;
    for (int i = threadIdx.x; i < N2; i += 256) {
        t_s[i] = tb[i * tsp];
        t_s[N2 + i] = tb[i * tsp + tsc];
        t_s[2 * N2 + i] = tb[i * tsp + 2 * tsc];
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N1) return;
    const float* sp = src + b * ssb + p * ssp;
    const float sx = sp[0], sy = sp[ssc], sz = sp[2 * ssc];
    float best = INFINITY;
    int bi = 0x7fffffff;
#pragma unroll 4
    for (int j = 0; j < N2; ++j) {
        const float dx = sx - t_s[j], dy = sy - t_s[N2 + j], dz = sz - t_s[2 * N2 + j];
        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        if (dvq_argmin_better(d, j, best, bi)) { best = d; bi = j; }
    }
    dist[b * N1 + p] = best;
    idx[b * N1 + p] = bi;
}

__global__ void vertex_normals_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                      const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                      float* __restrict__ out) {
    const long b = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float* vb = verts + b * V * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int q = vf_off[v]; q < vf_off[v + 1]; ++q) {
        const int f = vf_face[q];
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        const float ax = vb[3 * i1] - vb[3 * i0], ay = vb[3 * i1 + 1] - vb[3 * i0 + 1], az = vb[3 * i1 + 2] - vb[3 * i0 + 2];
        const float bx = vb[3 * i2] - vb[3 * i0], by = vb[3 * i2 + 1] - vb[3 * i0 + 1], bz = vb[3 * i2 + 2] - vb[3 * i0 + 2];
        nx += ay * bz - az * by;                                 // (no contraction: -ffp-contract=off)
        ny += az * bx - ax * bz;
        nz += ax * by - ay * bx;
    }
    const float len = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx)));
    const float inv = 1.0f / fmaxf(len, 1e-6f);
    float* o = out + (b * V + v) * 3;
    o[0] = nx * inv;
    o[1] = ny * inv;
    o[2] = nz * inv;
}

__global__ void interior_kernel(const float* __restrict__ normals, const float* __restrict__ hand, int V,
                                const float* __restrict__ obj, long osb, long osp, long osc, const int64_t* __restrict__ nn_idx,
                                int N, uint8_t* __restrict__ interior) {
    const long b = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    const long j = nn_idx[b * N + p];
    const float* h = hand + (b * V + j) * 3;
    const float* n = normals + (b * V + j) * 3;
    const float* o = obj + b * osb + p * osp;
    const float vx = h[0] - o[0], vy = h[1] - o[osc], vz = h[2] - o[2 * osc];
    const float dot = fmaf(vz, n[2], fmaf(vy, n[1], vx * n[0]));
    interior[b * N + p] = dot > 0.f ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- fused per-grasp scores
// dvq_grasp_scores: vertex_normals + nn_points (object points against the hand) + interior + the three per-grasp reductions of
// contact.grasp_proxies in ONE kernel, one workgroup of 256 threads per grasp; nothing of size [B,N] or [B,V,3] reaches HBM.
// LDS: the hand's vertices and normals as x|y|z planes of VP = V rounded up to 4 floats (16-byte broadcast reads of four
// vertices), then the reduction arrays.  Per-point results are the bits of the three kernels above (same expressions, same
// order); the reduction order is fixed (include/dvq.h), so a grasp's result does not depend on B or on its row.
// Everything up to the per-point results is grasp_scan.h's, shared with grasp_refine_kernel and grasp_wrench_kernel; this kernel's
// own part is the three accumulators and their tree.
__global__ __launch_bounds__(GRASP_THREADS) void grasp_scores_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                     const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                                                     const float* __restrict__ obj, long osb, long osp, long osc, int N,
                                                                     float thr, float* __restrict__ penetration,
                                                                     int* __restrict__ n_interior, int* __restrict__ n_contact) {
    extern __shared__ __align__(16) float gs_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gs_lds, V, hx, hy, hz, nx, ny, nz);
    float* part = gs_lds + grasp_hand_floats(V);                 // [256] partial sums
    int* cnt_in = reinterpret_cast<int*>(part + GRASP_THREADS);  // [256]
    int* cnt_ct = cnt_in + GRASP_THREADS;                        // [256]
    int* flag = cnt_ct + GRASP_THREADS;                          // [1]: a vertex coordinate is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    if (t == 0) *flag = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) *flag = 1;
    dvq_lds_barrier();
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);
    dvq_lds_barrier();
    const bool hand_odd = *flag != 0;
    const float* ob = obj + b * osb;
    float sum = 0.0f;
    int n_in = 0, n_ct = 0;
    for (long p0 = t; p0 < N; p0 += GRASP_THREADS * GRASP_P) {   // points p0 + k * 256: thread t's points, ascending
        float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P];
        int bi[GRASP_P];
        const bool slow = grasp_points4(ob, osp, osc, N, p0, sx, sy, sz) || hand_odd;
        grasp_scan4(hx, hy, hz, V, slow, sx, sy, sz, best, bi);
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            if (p0 + k * GRASP_THREADS < N) {
                const float d = best[k];
                const bool inside = grasp_inside(hx, hy, hz, nx, ny, nz, bi[k], sx[k], sy[k], sz[k]);
                sum += grasp_pen_term(inside, d);
                n_in += inside ? 1 : 0;
                n_ct += d < thr ? 1 : 0;
            }
        }
    }
    part[t] = sum;
    cnt_in[t] = n_in;
    cnt_ct[t] = n_ct;
    dvq_lds_barrier();
    for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {           // the canonical tree: part[t] += part[t + s] for t < s
        if (t < s) {
            part[t] += part[t + s];
            cnt_in[t] += cnt_in[t + s];
            cnt_ct[t] += cnt_ct[t + s];
        }
        dvq_lds_barrier();
    }
    if (t == 0) {
        penetration[b] = part[0];
        n_interior[b] = cnt_in[0];
        n_contact[b] = cnt_ct[0];
    }
}

// ---------------------------------------------------------------------------------------------- per-object top-k
// dvq_segment_topk: one workgroup per object; every candidate's rank is the number of candidates before it in the total order
// (cls, key, index) -- counted against all M, O(M^2), no workspace, no order left to the hardware.
constexpr int TOPK_MAX_M = 4096;            // 32 KB of LDS

// (cls, key) as one unsigned 64-bit word whose order is the documented one: cls as a signed integer, then the key with
// -0.0 == +0.0 and every NaN after +inf.
__device__ __forceinline__ unsigned long long topk_word(int cls, float key) {
    unsigned u = __float_as_uint(key);
    if (key != key) u = 0xffffffffu;
    else {
        if (key == 0.0f) u = 0u;
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)((unsigned)cls ^ 0x80000000u) << 32) | u;
}

__global__ __launch_bounds__(256) void segment_topk_kernel(const int* __restrict__ cls, const float* __restrict__ key, int M, int keep,
                                                           int64_t* __restrict__ sel) {
    __shared__ unsigned long long w_s[TOPK_MAX_M];
    const long o = blockIdx.x;
    for (int i = threadIdx.x; i < M; i += 256) w_s[i] = topk_word(cls[o * M + i], key[o * M + i]);
    __syncthreads();
    for (int i = threadIdx.x; i < M; i += 256) {
        const unsigned long long w = w_s[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) {
            const unsigned long long x = w_s[j];
            rank += (x < w || (x == w && j < i)) ? 1 : 0;
        }
        if (rank < keep) sel[o * keep + rank] = i;               // the ranks of an object are a permutation of 0 .. M-1
    }
}

}  // namespace

extern "C" int dvq_nn_points(const float* src, int64_t src_batch_stride, int64_t src_point_stride, int64_t src_coord_stride,
                             const float* trg, int64_t trg_batch_stride, int64_t trg_point_stride, int64_t trg_coord_stride,
                             int64_t B, int N1, int N2, float* dist, int64_t* idx, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N1 >= 0 && N2 >= 1 && N2 <= NN_MAX_TRG, "nn_points: need 1 <= N2 <= %d (got B=%ld N1=%d N2=%d)",
                NN_MAX_TRG, (long)B, N1, N2);
    if (B == 0 || N1 == 0) return DVQ_OK;
    DVQ_REQUIRE(src && trg && dist && idx, "nn_points: null pointer");
    DVQ_REQUIRE(B <= 65535LL * 65535LL, "nn_points: B too large");
    hipStream_t st = (hipStream_t)stream;
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&nn_points_kernel), (size_t)NN_MAX_TRG * 12, "nn_points"));
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        DVQ_PROF("nn_points", 8.0 * nb * N1 * N2, (double)nb * (N1 + N2) * 12 + (double)nb * N1 * 12, st);
        DVQ_LAUNCH(nn_points_kernel, dim3((N1 + 255) / 256, (unsigned)nb), dim3(256), (size_t)N2 * 12, st,
                           src + b0 * src_batch_stride, (long)src_batch_stride, (long)src_point_stride, (long)src_coord_stride,
                           trg + b0 * trg_batch_stride, (long)trg_batch_stride, (long)trg_point_stride, (long)trg_coord_stride,
                           N1, N2, dist + b0 * N1, idx + b0 * N1);
    });
    DVQ_CHECK_LAUNCH("nn_points");
    return DVQ_OK;
}

extern "C" int dvq_vertex_normals(const float* verts, int64_t B, int V, const int32_t* faces, const int32_t* vf_off,
                                  const int32_t* vf_face, float* normals, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && V >= 1, "vertex_normals: bad sizes");
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(verts && faces && vf_off && vf_face && normals, "vertex_normals: null pointer");
    hipStream_t st = (hipStream_t)stream;
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        DVQ_LAUNCH(vertex_normals_kernel, dim3((V + 127) / 128, (unsigned)nb), dim3(128), 0, st,
                           verts + b0 * V * 3, faces, vf_off, vf_face, V, normals + b0 * V * 3);
    });
    DVQ_CHECK_LAUNCH("vertex_normals");
    return DVQ_OK;
}

extern "C" int dvq_interior(const float* normals, const float* hand, int V, const float* obj, int64_t obj_batch_stride,
                            int64_t obj_point_stride, int64_t obj_coord_stride, const int64_t* nn_idx, int64_t B, int N,
                            uint8_t* interior, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 0 && V >= 1, "interior: bad sizes");
    if (B == 0 || N == 0) return DVQ_OK;
    DVQ_REQUIRE(normals && hand && obj && nn_idx && interior, "interior: null pointer");
    hipStream_t st = (hipStream_t)stream;
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        DVQ_LAUNCH(interior_kernel, dim3((N + 255) / 256, (unsigned)nb), dim3(256), 0, st, normals + b0 * V * 3,
                           hand + b0 * V * 3, V, obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride,
                           (long)obj_coord_stride, nn_idx + b0 * N, N, interior + b0 * N);
    });
    DVQ_CHECK_LAUNCH("interior");
    return DVQ_OK;
}

extern "C" int dvq_grasp_scores(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                int64_t B, int N, float contact_threshold, float* penetration, int32_t* n_interior,
                                int32_t* n_contact, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V, "grasp_scores: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)",
                GRASP_MAX_V, (long)B, N, V);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && penetration && n_interior && n_contact, "grasp_scores: null pointer");
    hipStream_t st = (hipStream_t)stream;
    constexpr int more = 3 * GRASP_THREADS + 4;                  // floats after the planes: the reduction arrays and the flag
    const size_t lds = grasp_lds_bytes(V, more);
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_scores_kernel), grasp_lds_bytes(GRASP_MAX_V, more),
                                "grasp_scores"));
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // per (point, vertex) pair 3 subtractions, 1 product, 2 fmas = 8 FLOPs; in: the hand, the cloud and the topology once per
        // grasp; out: 12 B per grasp
        DVQ_PROF("grasp_scores", 8.0 * nb * N * V, (double)nb * ((double)(V + N) * 12 + 12), st);
        DVQ_LAUNCH(grasp_scores_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, penetration + b0, n_interior + b0, n_contact + b0);
    });
    DVQ_CHECK_LAUNCH("grasp_scores");
    return DVQ_OK;
}

extern "C" int dvq_segment_topk(const int32_t* cls, const float* key, int64_t O, int M, int keep, int64_t* sel, dvq_stream_t stream) {
    DVQ_REQUIRE(O >= 0 && keep >= 1 && keep <= M && M <= TOPK_MAX_M, "segment_topk: need O >= 0, 1 <= keep <= M <= %d (got O=%ld M=%d keep=%d)",
                TOPK_MAX_M, (long)O, M, keep);
    if (O == 0) return DVQ_OK;
    DVQ_REQUIRE(cls && key && sel, "segment_topk: null pointer");
    DVQ_REQUIRE(O <= 0x7fffffffLL, "segment_topk: O too large");
    hipStream_t st = (hipStream_t)stream;
    DVQ_PROF("segment_topk", 0.0, (double)O * ((double)M * 8 + (double)keep * 8), st);
    DVQ_LAUNCH(segment_topk_kernel, dim3((unsigned)O), dim3(256), 0, st, cls, key, M, keep, sel);
    DVQ_CHECK_LAUNCH("segment_topk");
    return DVQ_OK;
}
