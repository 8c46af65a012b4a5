// The per-grasp hand in LDS, written once for the kernels that run one workgroup of 256 threads per grasp: grasp_scores_kernel
// (contact.hip), grasp_refine_kernel, grasp_wrench_kernel and, for the hand load alone, grasp_volume_kernel.  The hand's vertices
// and its vertex normals sit in LDS as x|y|z planes of VP = V rounded up to 4 floats (16-byte broadcast reads of four vertices);
// every object point finds its nearest vertex by a scan of the planes.  Per point the results are the bits of nn_points_kernel,
// vertex_normals_kernel and interior_kernel (contact.hip: same expressions, same order), and because the three kernels take them
// from here, their three scores are the same bits too.
//
// No helper contains a barrier: where the planes are published is visible in each kernel.
#pragma once
#include "dvq_internal.h"

constexpr int GRASP_THREADS = 256;          // threads of the workgroup
constexpr int GRASP_P = 4;                  // object points per thread and pass: every LDS read serves four points
constexpr int GRASP_MAX_V = 2048;           // 6 planes * 2048 * 4 B = 48 KB, + the kernel's reduction arrays

__host__ __device__ constexpr int grasp_vp(int V) { return (V + 3) & ~3; }
__host__ __device__ constexpr int grasp_hand_floats(int V) { return 6 * grasp_vp(V); }   // the six planes; a kernel's arrays follow
__host__ __device__ constexpr size_t grasp_lds_bytes(int V, int more_floats) { return (size_t)(grasp_hand_floats(V) + more_floats) * 4; }

__device__ __forceinline__ bool grasp_finite(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// The six planes of a hand of V vertices at `lds`: vertices, then normals.
__device__ __forceinline__ void grasp_planes(float* lds, int V, float*& hx, float*& hy, float*& hz, float*& nx, float*& ny, float*& nz) {
    const int VP = grasp_vp(V);
    hx = lds;
    hy = hx + VP;
    hz = hy + VP;
    nx = hz + VP;
    ny = nx + VP;
    nz = ny + VP;
}

// Thread t's share of the hand vb[V][3] into the planes; true if one of its coordinates is not finite.
__device__ __forceinline__ bool grasp_load_hand(const float* __restrict__ vb, int V, int t, float* hx, float* hy, float* hz) {
    bool odd = false;
    for (int i = t; i < V; i += GRASP_THREADS) {
        const float x = vb[3 * i], y = vb[3 * i + 1], z = vb[3 * i + 2];
        hx[i] = x;
        hy[i] = y;
        hz[i] = z;
        odd |= !grasp_finite(x, y, z);
    }
    return odd;
}

// Thread t's share of the vertex normals: vertex_normals_kernel's expression on the LDS copy (the vertices must be published).
__device__ __forceinline__ void grasp_normals(const int* __restrict__ faces, const int* __restrict__ vf_off, const int* __restrict__ vf_face,
                                              int V, int t, const float* hx, const float* hy, const float* hz, float* nx, float* ny,
                                              float* nz) {
    for (int v = t; v < V; v += GRASP_THREADS) {
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
}

// Nearest vertex of one point, every case (NaN distances included): nn_points_kernel's loop.
__device__ __forceinline__ void grasp_scan_exact(const float* hx, const float* hy, const float* hz, int V, float sx, float sy, float sz,
                                                 float& best, int& bi) {
    best = INFINITY;
    bi = 0x7fffffff;
    for (int j = 0; j < V; ++j) {
        const float dx = sx - hx[j], dy = sy - hy[j], dz = sz - hz[j];
        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        if (dvq_argmin_better(d, j, best, bi)) { best = d; bi = j; }
    }
}

// Nearest vertices of four points.  `slow`: a coordinate of the hand or of one of the points is not finite.  (The results are
// local arrays, handed over at the end: with the caller's arrays updated in place through the references grasp_scores_kernel
// needs one register more than the 80 that give it six waves per SIMD.)
__device__ __forceinline__ void grasp_scan4(const float* hx, const float* hy, const float* hz, int V, bool slow, const float (&sx)[GRASP_P],
                                            const float (&sy)[GRASP_P], const float (&sz)[GRASP_P], float (&best_out)[GRASP_P],
                                            int (&bi_out)[GRASP_P]) {
    float best[GRASP_P];
    int bi[GRASP_P];
#pragma unroll
    for (int k = 0; k < GRASP_P; ++k) {
        best[k] = INFINITY;
        bi[k] = 0;
    }
    if (!slow) {
        // Every coordinate finite: no distance is NaN, and over ascending j dvq_argmin_better(d, j, best, bi) from
        // (INFINITY, 0x7fffffff) takes j = 0 and afterwards exactly the j with d < best -- the loop below.
        const int V4 = V & ~3;
        for (int j = 0; j < V4; j += 4) {
            const f32x4 X = *reinterpret_cast<const f32x4*>(hx + j);
            const f32x4 Y = *reinterpret_cast<const f32x4*>(hy + j);
            const f32x4 Z = *reinterpret_cast<const f32x4*>(hz + j);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int k = 0; k < GRASP_P; ++k) {
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
            for (int k = 0; k < GRASP_P; ++k) {
                const float dx = sx[k] - hx[j], dy = sy[k] - hy[j], dz = sz[k] - hz[j];
                const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                const bool better = d < best[k];
                best[k] = better ? d : best[k];
                bi[k] = better ? j : bi[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) grasp_scan_exact(hx, hy, hz, V, sx[k], sy[k], sz[k], best[k], bi[k]);
    }
#pragma unroll
    for (int k = 0; k < GRASP_P; ++k) {
        best_out[k] = best[k];
        bi_out[k] = bi[k];
    }
}

// interior_kernel's test of a point s against its nearest vertex j (0 <= j < V: the scan always takes j = 0).
__device__ __forceinline__ bool grasp_inside(const float* hx, const float* hy, const float* hz, const float* nx, const float* ny,
                                             const float* nz, int j, float sx, float sy, float sz) {
    const float vx = hx[j] - sx, vy = hy[j] - sy, vz = hz[j] - sz;
    const float dot = fmaf(vz, nz[j], fmaf(vy, ny[j], vx * nx[j]));
    return dot > 0.f;
}

// The penetration term of a point at squared distance d: a NaN distance counts, inside or not.
__device__ __forceinline__ float grasp_pen_term(bool inside, float d) { return (inside || d != d) ? d : 0.0f; }
