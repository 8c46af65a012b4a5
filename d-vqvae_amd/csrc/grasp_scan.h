// The per-grasp hand in LDS, written once for the kernels that run one workgroup of 256 threads per grasp.  The hand's vertices and
// its vertex normals sit in LDS as x|y|z planes of VP = V rounded up to 4 floats (16-byte broadcast reads of four vertices); every
// point finds its nearest vertex by a walk over the planes (grasp_walk4: the distance expression, the block / tail split and the
// ascending order stand there and in grasp_scan_exact, nowhere else).  Per point the results are the bits of nn_points_kernel,
// vertex_normals_kernel and interior_kernel (contact.hip: same expressions, same order), and because the kernels take them from
// here, the scores they share are the same bits too.  Who takes what:
//   grasp_scores_kernel (contact.hip), grasp_wrench_kernel: the planes, the hand load, the normals, the tile load grasp_points4,
//     grasp_scan4, the interior test, the penetration term;
//   grasp_refine_kernel (three levels), segment_contact_kernel: the same with a tile load of their own (refine subtracts its offset
//     and tests the moved point; with grasp_points4 the scan loops of both come out in another order than they had: DESIGN.md);
//   grasp_ttt_kernel: the planes, the hand load, the normals, the interior test, the penetration term, grasp_scan4's exact path for a
//     row that is not finite; its two minima come from a COPY of the walk and of the tile load (through the helpers its launch
//     with the gradient measured slower: DESIGN.md);
//   grasp_self_kernel: the planes, the hand load, the normals; the walk with a part word per vertex for its masked minimum;
//   grasp_parts_kernel: grasp_scan4 with a tile of object points as the planes and the hand's vertices as the points;
//   grasp_volume_kernel, grasp_mesh_volume_kernel: the hand load (the rest of what they share is grasp_raster.h);
//   grasp_mesh_kernel: GRASP_THREADS, GRASP_P and GRASP_MAX_V.
//
// No helper contains a barrier: where the planes are published is visible in each kernel.
#pragma once
#include "dvq_internal.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));   // the indices of four running minima (f32x4: their values)

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

// The four points p0 + k * GRASP_THREADS of the strided cloud ob[N] into sx|sy|sz (a slot beyond N: 0); true if one of the loaded
// coordinates is not finite.
__device__ __forceinline__ bool grasp_points4(const float* __restrict__ ob, long osp, long osc, int N, long p0, float (&sx)[GRASP_P],
                                              float (&sy)[GRASP_P], float (&sz)[GRASP_P]) {
    bool odd = false;
#pragma unroll
    for (int k = 0; k < GRASP_P; ++k) {
        const long p = p0 + k * GRASP_THREADS;
        const bool in = p < N;
        sx[k] = in ? ob[p * osp] : 0.f;
        sy[k] = in ? ob[p * osp + osc] : 0.f;
        sz[k] = in ? ob[p * osp + 2 * osc] : 0.f;
        odd |= !grasp_finite(sx[k], sy[k], sz[k]);
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

// The vertex walk, once: for every vertex j of the planes, ascending, and every k < GRASP_P, pair(k, j, d, a) with d the squared
// distance of point k to vertex j and a what `aux` holds for vertex j.  Four vertices per 16-byte broadcast read up to V & ~3, then
// the tail one by one.  An aux has load4(j) (the block's word or words), at(T, u) (element u of them) and load1(j) (a tail vertex).
// A caller keeps its running minima in an f32x4 / i32x4 pair that the lambda updates by element, not in arrays: that is the form in
// which the compiler held the arrays while the loops stood in the kernels; with arrays behind the lambda it holds eight scalars, and
// every kernel's scan loop is scheduled differently (measured: a few tenths of a per cent slower in two kernels).
template <class Aux, class Pair>
__device__ __forceinline__ void grasp_walk4(const float* hx, const float* hy, const float* hz, int V, const float (&sx)[GRASP_P],
                                            const float (&sy)[GRASP_P], const float (&sz)[GRASP_P], Aux aux, Pair pair) {
    const int V4 = V & ~3;
    for (int j = 0; j < V4; j += 4) {
        const f32x4 X = *reinterpret_cast<const f32x4*>(hx + j);
        const f32x4 Y = *reinterpret_cast<const f32x4*>(hy + j);
        const f32x4 Z = *reinterpret_cast<const f32x4*>(hz + j);
        const auto T = aux.load4(j);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const auto a = aux.at(T, u);
#pragma unroll
            for (int k = 0; k < GRASP_P; ++k) {
                const float dx = sx[k] - X[u], dy = sy[k] - Y[u], dz = sz[k] - Z[u];
                const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                pair(k, j + u, d, a);
            }
        }
    }
    for (int j = V4; j < V; ++j) {
        const auto a = aux.load1(j);
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const float dx = sx[k] - hx[j], dy = sy[k] - hy[j], dz = sz[k] - hz[j];
            const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            pair(k, j, d, a);
        }
    }
}

// The aux of a walk that needs nothing per vertex.
struct GraspNoAux {
    __device__ __forceinline__ int load4(int) const { return 0; }
    __device__ __forceinline__ int at(int, int) const { return 0; }
    __device__ __forceinline__ int load1(int) const { return 0; }
};

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
        // (INFINITY, 0x7fffffff) takes j = 0 and afterwards exactly the j with d < best -- the walk with this pair.
        static_assert(GRASP_P == 4, "the running minima are 4-vectors");
        f32x4 vb = INFINITY;
        i32x4 vi = 0;
        grasp_walk4(hx, hy, hz, V, sx, sy, sz, GraspNoAux{}, [&](int k, int j, float d, int) {
            const bool better = d < vb[k];
            vb[k] = better ? d : vb[k];
            vi[k] = better ? j : vi[k];
        });
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            best[k] = vb[k];
            bi[k] = vi[k];
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
