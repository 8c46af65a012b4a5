// dvq_grasp_wrench: a force-closure proxy of generated grasps -- the sums behind the net wrench of unit contact forces and behind
// the grasp matrix's smallest singular value -- together with the three scores of contact.hip (dvq_grasp_scores), in ONE kernel,
// one workgroup of 256 threads per grasp.  The definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// The hand's vertices and normals sit in LDS as x|y|z planes (grasp_scan.h).  Before the scan one pass over the cloud
// gives the centre (three canonical sums, their columns in the tail of the LDS block).  The scan is grasp_scan.h's; a point
// within the contact threshold then adds its wrench w = (n[j], r x n[j]) and the upper triangle of w w^T to 27 accumulators in
// registers -- a point outside the threshold would add +0.0f to every one, which changes no bit of a sum that started from +0.0f
// (such a sum is never -0.0f), so it is skipped.  After the scan the hand is dead: the 27 columns of partial sums overlay its
// planes (LDS = max(planes, 27 KB) + 3 KB, 30 KB at MANO's 778 vertices, five workgroups per CU) and all columns go through the
// canonical tree side by side, eight barriers for the lot.
//
// The planes, the hand load, the normals, the pair scan and the interior test are grasp_scan.h's, shared with grasp_scores_kernel and
// grasp_refine_kernel: the first three outputs are the bits of dvq_grasp_scores because they come from the same text.  This kernel's
// own part is the centre pass, the 27 columns and the overlay of the planes.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GW_SUMS = 27;                 // w[0..5], then w[a] * w[b] for a <= b, row-major
constexpr int GW_TAIL = 3 * GRASP_THREADS + 4; // floats after the overlay region: three columns (centre, later the scores) and the flag

// floats of the region that holds the hand during the scan and the 27 columns after it
__host__ __device__ constexpr int gw_region(int V) {
    return grasp_hand_floats(V) > GW_SUMS * GRASP_THREADS ? grasp_hand_floats(V) : GW_SUMS * GRASP_THREADS;
}

__global__ __launch_bounds__(GRASP_THREADS) void grasp_wrench_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                     const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                                                     const float* __restrict__ obj, long osb, long osp, long osc, int N,
                                                                     float thr, float inv_length, float* __restrict__ penetration,
                                                                     int* __restrict__ n_interior, int* __restrict__ n_contact,
                                                                     float* __restrict__ centre, float* __restrict__ sums,
                                                                     float* __restrict__ key) {
    extern __shared__ __align__(16) float gw_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gw_lds, V, hx, hy, hz, nx, ny, nz);
    float* col = gw_lds;                                         // [27][256] partial sums: over the planes, after the scan
    float* tail = gw_lds + gw_region(V);                         // [3][256]: the centre's columns, later penetration and the counts
    int* cnt = reinterpret_cast<int*>(tail + GRASP_THREADS);     // [2][256] (the second life of tail's columns 1 and 2)
    int* flag = reinterpret_cast<int*>(tail + 3 * GRASP_THREADS);   // [1]: a vertex coordinate is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const float* ob = obj + b * osb;
    if (t == 0) *flag = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) *flag = 1;
    {
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;                   // the centre: thread t's points in ascending p
        for (long p = t; p < N; p += GRASP_THREADS) {
            cx += ob[p * osp];
            cy += ob[p * osp + osc];
            cz += ob[p * osp + 2 * osc];
        }
        tail[t] = cx;
        tail[GRASP_THREADS + t] = cy;
        tail[2 * GRASP_THREADS + t] = cz;
    }
    dvq_lds_barrier();
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);
    for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {           // the canonical tree over the centre's three columns
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) tail[c * GRASP_THREADS + t] += tail[c * GRASP_THREADS + t + s];
        }
        dvq_lds_barrier();                                       // (the first of these also publishes the normals)
    }
    const float fn = (float)N;
    const float cx = tail[0] / fn, cy = tail[GRASP_THREADS] / fn, cz = tail[2 * GRASP_THREADS] / fn;
    const bool hand_odd = *flag != 0;
    float sum = 0.0f;
    int n_in = 0, n_ct = 0;
    float acc[GW_SUMS];
#pragma unroll
    for (int c = 0; c < GW_SUMS; ++c) acc[c] = 0.0f;
    for (long p0 = t; p0 < N; p0 += GRASP_THREADS * GRASP_P) {   // points p0 + k * 256: thread t's points, ascending
        float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P];
        int bi[GRASP_P];
        const bool slow = grasp_points4(ob, osp, osc, N, p0, sx, sy, sz) || hand_odd;
        grasp_scan4(hx, hy, hz, V, slow, sx, sy, sz, best, bi);
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            if (p0 + k * GRASP_THREADS < N) {
                const int j = bi[k];                             // 0 <= j < V: the scan always takes j = 0
                const float d = best[k];
                const float fx = nx[j], fy = ny[j], fz = nz[j];  // (grasp_inside reads the same three: one load each in the listing)
                const bool inside = grasp_inside(hx, hy, hz, nx, ny, nz, j, sx[k], sy[k], sz[k]);
                sum += grasp_pen_term(inside, d);
                n_in += inside ? 1 : 0;
                if (d < thr) {                                   // a contact point: few of the cloud's
                    n_ct += 1;
                    const float rx = (sx[k] - cx) * inv_length, ry = (sy[k] - cy) * inv_length, rz = (sz[k] - cz) * inv_length;
                    float w[6];
                    w[0] = fx;
                    w[1] = fy;
                    w[2] = fz;
                    w[3] = ry * fz - rz * fy;                    // (no contraction: -ffp-contract=off)
                    w[4] = rz * fx - rx * fz;
                    w[5] = rx * fy - ry * fx;
                    int c = 6;
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        acc[a] += w[a];
#pragma unroll
                        for (int e = a; e < 6; ++e) acc[c++] += w[a] * w[e];
                    }
                }
            }
        }
    }
    dvq_lds_barrier();                                           // every wave is through with the hand: its planes become the columns
#pragma unroll
    for (int c = 0; c < GW_SUMS; ++c) col[c * GRASP_THREADS + t] = acc[c];
    tail[t] = sum;
    cnt[t] = n_in;
    cnt[GRASP_THREADS + t] = n_ct;
    dvq_lds_barrier();
    for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {           // the canonical tree, each sum on its own: part[t] += part[t + s] for t < s
        if (t < s) {
#pragma unroll
            for (int c = 0; c < GW_SUMS; ++c) col[c * GRASP_THREADS + t] += col[c * GRASP_THREADS + t + s];
            tail[t] += tail[t + s];
            cnt[t] += cnt[t + s];
            cnt[GRASP_THREADS + t] += cnt[GRASP_THREADS + t + s];
        }
        dvq_lds_barrier();
    }
    if (t < GW_SUMS) sums[b * GW_SUMS + t] = col[t * GRASP_THREADS];
    if (t == 0) {
        const float pen = tail[0];
        const int c_ct = cnt[GRASP_THREADS];
        penetration[b] = pen;
        n_interior[b] = cnt[0];
        n_contact[b] = c_ct;
        centre[3 * b] = cx;
        centre[3 * b + 1] = cy;
        centre[3 * b + 2] = cz;
        const float s0 = col[0], s1 = col[GRASP_THREADS], s2 = col[2 * GRASP_THREADS], s3 = col[3 * GRASP_THREADS], s4 = col[4 * GRASP_THREADS],
                    s5 = col[5 * GRASP_THREADS];
        const float q = fmaf(s5, s5, fmaf(s4, s4, fmaf(s3, s3, fmaf(s2, s2, fmaf(s1, s1, s0 * s0)))));
        const float nf = (float)c_ct;
        key[b] = pen != pen ? pen : (c_ct == 0 ? INFINITY : q / (nf * nf));
    }
}

}  // namespace

extern "C" int dvq_grasp_wrench(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                int64_t B, int N, float contact_threshold, float inv_length, float* penetration, int32_t* n_interior,
                                int32_t* n_contact, float* centre, float* sums, float* key, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V, "grasp_wrench: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)",
                GRASP_MAX_V, (long)B, N, V);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && penetration && n_interior && n_contact && centre && sums && key,
                "grasp_wrench: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(gw_region(V) + GW_TAIL) * 4;
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_wrench_kernel), (size_t)(gw_region(GRASP_MAX_V) + GW_TAIL) * 4,
                                "grasp_wrench"));
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // per (point, vertex) pair 8 FLOPs as in grasp_scores, plus 3 additions per point for the centre; the work on the contact
        // points (at most 63 FLOPs each) depends on the data and is not counted.  in: the hand and the topology once, the cloud twice
        // (the centre's pass and the scan); out: 12 + 12 + 108 + 4 B per grasp
        DVQ_PROF("grasp_wrench", 8.0 * nb * N * V + 3.0 * nb * N, (double)nb * ((double)(V + 2 * (double)N) * 12 + 136), st);
        DVQ_LAUNCH(grasp_wrench_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, inv_length, penetration + b0, n_interior + b0, n_contact + b0, centre + 3 * b0,
                   sums + GW_SUMS * b0, key + b0);
    });
    DVQ_CHECK_LAUNCH("grasp_wrench");
    return DVQ_OK;
}
