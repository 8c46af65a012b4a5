// dvq_grasp_wrench: a force-closure proxy of generated grasps -- the sums behind the net wrench of unit contact forces and behind
// the grasp matrix's smallest singular value -- together with the three scores of contact.hip (dvq_grasp_scores), in ONE kernel,
// one workgroup of 256 threads per grasp.  The definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// The hand's vertices and normals sit in LDS as x|y|z planes, as in grasp_scores_kernel.  Before the scan one pass over the cloud
// gives the centre (three canonical sums, their columns in the tail of the LDS block).  The scan is grasp_scores_kernel's; a point
// within the contact threshold then adds its wrench w = (n[j], r x n[j]) and the upper triangle of w w^T to 27 accumulators in
// registers -- a point outside the threshold would add +0.0f to every one, which changes no bit of a sum that started from +0.0f
// (such a sum is never -0.0f), so it is skipped.  After the scan the hand is dead: the 27 columns of partial sums overlay its
// planes (LDS = max(planes, 27 KB) + 3 KB, 30 KB at MANO's 778 vertices, five workgroups per CU) and all columns go through the
// canonical tree side by side, eight barriers for the lot.
//
// The pair scan is a copy of grasp_scores_kernel's, not shared code: contact.hip compiles to what it compiled to before.
#include "dvq_internal.h"

namespace {

constexpr int GW_MAX_V = 2048;              // 6 planes * 2048 * 4 B = 48 KB, + 3 KB of reduction columns
constexpr int GW_THREADS = 256;
constexpr int GW_P = 4;                     // object points per thread and pass: every LDS read serves four points
constexpr int GW_SUMS = 27;                 // w[0..5], then w[a] * w[b] for a <= b, row-major
constexpr int GW_TAIL = 3 * GW_THREADS + 4; // floats after the overlay region: three columns (centre, later the scores) and the flag

// floats of the region that holds the hand during the scan and the 27 columns after it
__host__ __device__ constexpr int gw_region(int V) {
    return 6 * ((V + 3) & ~3) > GW_SUMS * GW_THREADS ? 6 * ((V + 3) & ~3) : GW_SUMS * GW_THREADS;
}

// Nearest vertex of one point, every case (NaN distances included): nn_points_kernel's loop.
__device__ __forceinline__ void gw_scan_exact(const float* hx, const float* hy, const float* hz, int V, float sx, float sy, float sz,
                                              float& best, int& bi) {
    best = INFINITY;
    bi = 0x7fffffff;
    for (int j = 0; j < V; ++j) {
        const float dx = sx - hx[j], dy = sy - hy[j], dz = sz - hz[j];
        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        if (dvq_argmin_better(d, j, best, bi)) { best = d; bi = j; }
    }
}

__global__ __launch_bounds__(GW_THREADS) void grasp_wrench_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                  const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                                                  const float* __restrict__ obj, long osb, long osp, long osc, int N,
                                                                  float thr, float inv_length, float* __restrict__ penetration,
                                                                  int* __restrict__ n_interior, int* __restrict__ n_contact,
                                                                  float* __restrict__ centre, float* __restrict__ sums,
                                                                  float* __restrict__ key) {
    extern __shared__ __align__(16) float gw_lds[];
    const int VP = (V + 3) & ~3;
    float* hx = gw_lds;                                          // hand vertices, planes
    float* hy = hx + VP;
    float* hz = hy + VP;
    float* nx = hz + VP;                                         // vertex normals, planes
    float* ny = nx + VP;
    float* nz = ny + VP;
    float* col = gw_lds;                                         // [27][256] partial sums: over the planes, after the scan
    float* tail = gw_lds + gw_region(V);                         // [3][256]: the centre's columns, later penetration and the counts
    int* cnt = reinterpret_cast<int*>(tail + GW_THREADS);        // [2][256] (the second life of tail's columns 1 and 2)
    int* flag = reinterpret_cast<int*>(tail + 3 * GW_THREADS);   // [1]: a vertex coordinate is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const float* vb = hand + b * V * 3;
    const float* ob = obj + b * osb;
    if (t == 0) *flag = 0;
    dvq_lds_barrier();
    bool odd = false;
    for (int i = t; i < V; i += GW_THREADS) {
        const float x = vb[3 * i], y = vb[3 * i + 1], z = vb[3 * i + 2];
        hx[i] = x;
        hy[i] = y;
        hz[i] = z;
        odd |= !(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY) || !(fabsf(z) < INFINITY);
    }
    if (odd) *flag = 1;
    {
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;                   // the centre: thread t's points in ascending p
        for (long p = t; p < N; p += GW_THREADS) {
            cx += ob[p * osp];
            cy += ob[p * osp + osc];
            cz += ob[p * osp + 2 * osc];
        }
        tail[t] = cx;
        tail[GW_THREADS + t] = cy;
        tail[2 * GW_THREADS + t] = cz;
    }
    dvq_lds_barrier();
    for (int v = t; v < V; v += GW_THREADS) {                    // vertex_normals_kernel's expression on the LDS copy
        float mx = 0.f, my = 0.f, mz = 0.f;
        for (int q = vf_off[v]; q < vf_off[v + 1]; ++q) {
            const int f = vf_face[q];
            const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            const float ax = hx[i1] - hx[i0], ay = hy[i1] - hy[i0], az = hz[i1] - hz[i0];
            const float bx = hx[i2] - hx[i0], by = hy[i2] - hy[i0], bz = hz[i2] - hz[i0];
            mx += ay * bz - az * by;                            // (no contraction: -ffp-contract=off)
            my += az * bx - ax * bz;
            mz += ax * by - ay * bx;
        }
        const float len = sqrtf(fmaf(mz, mz, fmaf(my, my, mx * mx)));
        const float inv = 1.0f / fmaxf(len, 1e-6f);
        nx[v] = mx * inv;
        ny[v] = my * inv;
        nz[v] = mz * inv;
    }
    for (int s = GW_THREADS / 2; s >= 1; s >>= 1) {              // the canonical tree over the centre's three columns
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) tail[c * GW_THREADS + t] += tail[c * GW_THREADS + t + s];
        }
        dvq_lds_barrier();                                       // (the first of these also publishes the normals)
    }
    const float fn = (float)N;
    const float cx = tail[0] / fn, cy = tail[GW_THREADS] / fn, cz = tail[2 * GW_THREADS] / fn;
    const bool hand_odd = *flag != 0;
    const int V4 = V & ~3;
    float sum = 0.0f;
    int n_in = 0, n_ct = 0;
    float acc[GW_SUMS];
#pragma unroll
    for (int c = 0; c < GW_SUMS; ++c) acc[c] = 0.0f;
    for (long p0 = t; p0 < N; p0 += GW_THREADS * GW_P) {         // points p0 + k * 256: thread t's points, ascending
        float sx[GW_P], sy[GW_P], sz[GW_P], best[GW_P];
        int bi[GW_P];
        bool slow = hand_odd;
#pragma unroll
        for (int k = 0; k < GW_P; ++k) {
            const long p = p0 + k * GW_THREADS;
            const bool in = p < N;
            sx[k] = in ? ob[p * osp] : 0.f;
            sy[k] = in ? ob[p * osp + osc] : 0.f;
            sz[k] = in ? ob[p * osp + 2 * osc] : 0.f;
            slow |= !(fabsf(sx[k]) < INFINITY) || !(fabsf(sy[k]) < INFINITY) || !(fabsf(sz[k]) < INFINITY);
            best[k] = INFINITY;
            bi[k] = 0;
        }
        if (!slow) {
            // Every coordinate finite: no distance is NaN, and over ascending j dvq_argmin_better(d, j, best, bi) from
            // (INFINITY, 0x7fffffff) takes j = 0 and afterwards exactly the j with d < best -- the loop below.
            for (int j = 0; j < V4; j += 4) {
                const f32x4 X = *reinterpret_cast<const f32x4*>(hx + j);
                const f32x4 Y = *reinterpret_cast<const f32x4*>(hy + j);
                const f32x4 Z = *reinterpret_cast<const f32x4*>(hz + j);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int k = 0; k < GW_P; ++k) {
                        const float dx = sx[k] - X[u], dy = sy[k] - Y[u], dz = sz[k] - Z[u];
                        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        const bool better = d < best[k];
                        best[k] = better ? d : best[k];
                        bi[k] = better ? j + u : bi[k];
                    }
                }
            }
            for (int j = V4; j < V; ++j) {
#pragma unroll
                for (int k = 0; k < GW_P; ++k) {
                    const float dx = sx[k] - hx[j], dy = sy[k] - hy[j], dz = sz[k] - hz[j];
                    const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    const bool better = d < best[k];
                    best[k] = better ? d : best[k];
                    bi[k] = better ? j : bi[k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < GW_P; ++k) gw_scan_exact(hx, hy, hz, V, sx[k], sy[k], sz[k], best[k], bi[k]);
        }
#pragma unroll
        for (int k = 0; k < GW_P; ++k) {
            if (p0 + k * GW_THREADS < N) {
                const int j = bi[k];                             // 0 <= j < V: the scan always takes j = 0
                const float d = best[k];
                const float fx = nx[j], fy = ny[j], fz = nz[j];
                const float vx = hx[j] - sx[k], vy = hy[j] - sy[k], vz = hz[j] - sz[k];
                const float dot = fmaf(vz, fz, fmaf(vy, fy, vx * fx));   // interior_kernel
                const bool inside = dot > 0.f;
                sum += (inside || d != d) ? d : 0.0f;
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
    for (int c = 0; c < GW_SUMS; ++c) col[c * GW_THREADS + t] = acc[c];
    tail[t] = sum;
    cnt[t] = n_in;
    cnt[GW_THREADS + t] = n_ct;
    dvq_lds_barrier();
    for (int s = GW_THREADS / 2; s >= 1; s >>= 1) {              // the canonical tree, each sum on its own: part[t] += part[t + s] for t < s
        if (t < s) {
#pragma unroll
            for (int c = 0; c < GW_SUMS; ++c) col[c * GW_THREADS + t] += col[c * GW_THREADS + t + s];
            tail[t] += tail[t + s];
            cnt[t] += cnt[t + s];
            cnt[GW_THREADS + t] += cnt[GW_THREADS + t + s];
        }
        dvq_lds_barrier();
    }
    if (t < GW_SUMS) sums[b * GW_SUMS + t] = col[t * GW_THREADS];
    if (t == 0) {
        const float pen = tail[0];
        const int c_ct = cnt[GW_THREADS];
        penetration[b] = pen;
        n_interior[b] = cnt[0];
        n_contact[b] = c_ct;
        centre[3 * b] = cx;
        centre[3 * b + 1] = cy;
        centre[3 * b + 2] = cz;
        const float s0 = col[0], s1 = col[GW_THREADS], s2 = col[2 * GW_THREADS], s3 = col[3 * GW_THREADS], s4 = col[4 * GW_THREADS],
                    s5 = col[5 * GW_THREADS];
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
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GW_MAX_V, "grasp_wrench: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)",
                GW_MAX_V, (long)B, N, V);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && penetration && n_interior && n_contact && centre && sums && key,
                "grasp_wrench: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(gw_region(V) + GW_TAIL) * 4;
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_wrench_kernel), (size_t)(gw_region(GW_MAX_V) + GW_TAIL) * 4,
                                "grasp_wrench"));
    for (int64_t b0 = 0; b0 < B; b0 += 65535) {                  // the grid-dimension limit the neighbouring entry points chunk by
        const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
        // per (point, vertex) pair 8 FLOPs as in grasp_scores, plus 3 additions per point for the centre; the work on the contact
        // points (at most 63 FLOPs each) depends on the data and is not counted.  in: the hand and the topology once, the cloud twice
        // (the centre's pass and the scan); out: 12 + 12 + 108 + 4 B per grasp
        DVQ_PROF("grasp_wrench", 8.0 * nb * N * V + 3.0 * nb * N, (double)nb * ((double)(V + 2 * (double)N) * 12 + 136), st);
        DVQ_LAUNCH(grasp_wrench_kernel, dim3((unsigned)nb), dim3(GW_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, inv_length, penetration + b0, n_interior + b0, n_contact + b0, centre + 3 * b0,
                   sums + GW_SUMS * b0, key + b0);
    }
    DVQ_CHECK_LAUNCH("grasp_wrench");
    return DVQ_OK;
}
