// dvq_grasp_closure: force-closure quality of generated grasps with Coulomb friction -- the support function of the contacts' friction
// cones over a table of D directions in wrench space, its minimum (an upper bound of the L1 Ferrari-Canny quality) and the direction
// that attains it -- in ONE kernel, one workgroup of 256 threads per grasp.  The definition is the ABI (include/dvq.h); this file only
// says how the kernel is laid out.
//
// The first half is grasp_wrench_kernel's: the hand's vertices and normals in LDS as x|y|z planes, one pass over the cloud for the
// centre (three canonical sums), the normals, then grasp_scan.h's scan in tiles of 1024 points, four per thread.  The contacts cannot
// be folded into a fixed number of sums: after a tile's scan every contact writes its six floats (n, r) into a compacted list in LDS
// -- its place is a wave-ballot prefix plus the totals of the waves before it, no atomic -- and every thread walks the tile's list
// with broadcast reads for the directions it owns, t, t + 256, ... (at most four), their running maxima in registers.  Only maxima
// follow, so the order of the list does not reach a result.  The list has a region of its own: the planes stay live until the last
// tile.  LDS = planes + 24 KB + 3 KB, 45 KB at MANO's 778 vertices, three workgroups per CU.  At the end the per-thread minima (lowest
// direction first) go through a workgroup tree of (value, index) pairs in the tail's columns.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GC_TILE = GRASP_THREADS * GRASP_P;         // points per tile: what one pass of the scan covers
constexpr int GC_MAX_DIRS = DVQ_GRASP_CLOSURE_MAX_DIRS;
constexpr int GC_Q = GC_MAX_DIRS / GRASP_THREADS;        // directions per thread, at most
constexpr int GC_WAVES = GRASP_THREADS / 64;
constexpr int GC_LIST = 6 * GC_TILE;                     // floats of the contact list: (n.x, n.y, n.z, r.x, r.y, r.z) per contact
constexpr int GC_TAIL = 3 * GRASP_THREADS + GC_WAVES + 4;   // three columns (the centre's, later the minima and their indices), the waves' totals, two flags
static_assert(GC_MAX_DIRS % GRASP_THREADS == 0 && GC_Q == 4, "a thread owns at most four directions");

__host__ __device__ constexpr int gc_lds_floats(int V) { return grasp_hand_floats(V) + GC_LIST + GC_TAIL; }

__device__ __forceinline__ float gc_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// The tile's contacts against thread t's directions t + q * 256, q < Q: sup[q] = max(sup[q], h) with h as include/dvq.h defines it.
// A thread whose direction lies beyond D works on zeros; its maxima are never read.
template <int Q>
__device__ __forceinline__ void gc_walk(const float* __restrict__ dirs, int D, int t, const float* list, int total, float mu,
                                        float (&sup)[GC_Q]) {
    float u[Q][6];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = q * GRASP_THREADS + t;
#pragma unroll
        for (int c = 0; c < 6; ++c) u[q][c] = k < D ? dirs[6 * (long)k + c] : 0.0f;
    }
    for (int i = 0; i < total; ++i) {
        const float* e = list + 6 * i;                           // the same address in every lane: broadcast reads
        const float nx = e[0], ny = e[1], nz = e[2], rx = e[3], ry = e[4], rz = e[5];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float ax = u[q][0] + (u[q][4] * rz - u[q][5] * ry);    // a = uf + cross(ut, r)  (no contraction: -ffp-contract=off)
            const float ay = u[q][1] + (u[q][5] * rx - u[q][3] * rz);
            const float az = u[q][2] + (u[q][3] * ry - u[q][4] * rx);
            const float s = gc_dot(nx, ny, nz, ax, ay, az);
            const float cx = ny * az - nz * ay, cy = nz * ax - nx * az, cz = nx * ay - ny * ax;   // c = cross(n, a)
            const float h = fmaf(mu, sqrtf(gc_dot(cx, cy, cz, cx, cy, cz)), s);
            sup[q] = h > sup[q] ? h : sup[q];                    // a NaN never replaces
        }
    }
}

__global__ __launch_bounds__(GRASP_THREADS) void grasp_closure_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                      const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                                                      const float* __restrict__ obj, long osb, long osp, long osc, int N,
                                                                      float thr, float inv_length, float mu, const float* __restrict__ dirs,
                                                                      int D, float* __restrict__ quality, int* __restrict__ worst_dir,
                                                                      int* __restrict__ status, int* __restrict__ n_contact,
                                                                      float* __restrict__ centre, float* __restrict__ support) {
    extern __shared__ __align__(16) float gc_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gc_lds, V, hx, hy, hz, nx, ny, nz);
    float* list = gc_lds + grasp_hand_floats(V);                 // [1024][6]: the tile's contacts, compacted
    float* tail = list + GC_LIST;                                // [3][256]: the centre's columns, later the minima and their indices
    int* wtot = reinterpret_cast<int*>(tail + 3 * GRASP_THREADS);   // [4]: the tile's contacts per wave
    int* flag = wtot + GC_WAVES;                                 // [2]: a coordinate of the hand / of the cloud is not finite
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long b = blockIdx.x;
    const float* ob = obj + b * osb;
    if (t < 2) flag[t] = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) flag[0] = 1;
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
    const bool hand_odd = flag[0] != 0;
    const int Q = (D + GRASP_THREADS - 1) / GRASP_THREADS;       // 1 .. 4, the same in every thread
    float sup[GC_Q];
#pragma unroll
    for (int q = 0; q < GC_Q; ++q) sup[q] = -INFINITY;
    int n_ct = 0;                                                // of the whole grasp, the same in every thread
    for (long base = 0; base < N; base += GC_TILE) {             // every thread runs every tile: the barriers below are the workgroup's
        const long p0 = base + t;                                // points p0 + k * 256: grasp_scores_kernel's assignment
        float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P];
        int bi[GRASP_P];
        const bool odd = grasp_points4(ob, osp, osc, N, p0, sx, sy, sz);
        if (odd) flag[1] = 1;
        grasp_scan4(hx, hy, hz, V, odd || hand_odd, sx, sy, sz, best, bi);
        bool ct[GRASP_P];
        int at[GRASP_P], mine = 0;                               // a contact's place among its wave's, the wave's total
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            ct[k] = p0 + k * GRASP_THREADS < N && best[k] < thr;
            const unsigned long long m = __ballot(ct[k]);
            at[k] = mine + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            mine += __popcll(m);
        }
        if (lane == 0) wtot[wave] = mine;
        dvq_lds_barrier();
        int first = 0, total = 0;                                // where this wave's contacts start, the tile's contacts: at most 1024
#pragma unroll
        for (int w = 0; w < GC_WAVES; ++w) {
            const int c = wtot[w];
            first += w < wave ? c : 0;
            total += c;
        }
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            if (ct[k]) {
                const int j = bi[k];                             // 0 <= j < V: the scan always takes j = 0
                float* e = list + 6 * (first + at[k]);
                e[0] = nx[j];
                e[1] = ny[j];
                e[2] = nz[j];
                e[3] = (sx[k] - cx) * inv_length;
                e[4] = (sy[k] - cy) * inv_length;
                e[5] = (sz[k] - cz) * inv_length;
            }
        }
        n_ct += total;
        dvq_lds_barrier();
        switch (Q) {
            case 1: gc_walk<1>(dirs, D, t, list, total, mu, sup); break;
            case 2: gc_walk<2>(dirs, D, t, list, total, mu, sup); break;
            case 3: gc_walk<3>(dirs, D, t, list, total, mu, sup); break;
            default: gc_walk<4>(dirs, D, t, list, total, mu, sup); break;
        }
        dvq_lds_barrier();                                       // every wave is through with the list and the totals: the next tile's may come
    }
    const int st = (flag[0] | flag[1]) != 0 ? 2 : (n_ct == 0 ? 1 : 0);   // (the last barrier published every flag)
    float bv = INFINITY;                                         // thread t's smallest support, the lowest direction first
    int bk = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < GC_Q; ++q) {
        const int k = q * GRASP_THREADS + t;
        if (k < D) {
            const float s = sup[q] + 0.0f;                       // never NaN; -inf without a contact; a zero is +0.0f whichever contact came first
            if (support) support[b * D + k] = st == 2 ? NAN : s;
            if (s < bv || (s == bv && k < bk)) { bv = s; bk = k; }
        }
    }
    int* idx = reinterpret_cast<int*>(tail + GRASP_THREADS);
    tail[t] = bv;
    idx[t] = bk;
    dvq_lds_barrier();
    for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {           // the minimum, and among equals the lowest direction
        if (t < s) {
            const float ov = tail[t + s], mv = tail[t];
            const int oi = idx[t + s], mi = idx[t];
            if (ov < mv || (ov == mv && oi < mi)) {
                tail[t] = ov;
                idx[t] = oi;
            }
        }
        dvq_lds_barrier();
    }
    if (t == 0) {
        quality[b] = st == 2 ? NAN : tail[0];                    // st == 1: every support is -inf, and so is their minimum
        worst_dir[b] = st == 0 ? idx[0] : -1;
        status[b] = st;
        n_contact[b] = n_ct;
        centre[3 * b] = cx;
        centre[3 * b + 1] = cy;
        centre[3 * b + 2] = cz;
    }
}

}  // namespace

extern "C" int dvq_grasp_closure(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                 const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                 int64_t B, int N, float contact_threshold, float inv_length, float mu, const float* dirs, int D,
                                 float* quality, int32_t* worst_dir, int32_t* status, int32_t* n_contact, float* centre, float* support,
                                 dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V, "grasp_closure: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)",
                GRASP_MAX_V, (long)B, N, V);
    DVQ_REQUIRE(D >= 1 && D <= GC_MAX_DIRS && mu >= 0.0f && mu < INFINITY, "grasp_closure: need 1 <= D <= %d and mu finite and >= 0 (got D=%d mu=%g)",
                GC_MAX_DIRS, D, (double)mu);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && dirs && quality && worst_dir && status && n_contact && centre,
                "grasp_closure: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)gc_lds_floats(V) * 4;
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_closure_kernel), (size_t)gc_lds_floats(GRASP_MAX_V) * 4,
                                "grasp_closure"));
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // per (point, vertex) pair 8 FLOPs as in grasp_scores, plus 3 additions per point for the centre; the work on the contacts
        // (about 30 FLOPs per contact and direction) depends on the data and is not counted.  in: the hand and the topology once, the
        // cloud twice (the centre's pass and the scan), the table once per grasp (24 D B); out: 28 B per grasp, 4 D more with support
        DVQ_PROF("grasp_closure", 8.0 * nb * N * V + 3.0 * nb * N,
                 (double)nb * ((double)(V + 2 * (double)N) * 12 + 24.0 * D + 28 + (support ? 4.0 * D : 0.0)), st);
        DVQ_LAUNCH(grasp_closure_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, inv_length, mu, dirs, D, quality + b0, worst_dir + b0, status + b0, n_contact + b0, centre + 3 * b0,
                   support ? support + b0 * D : nullptr);
    });
    DVQ_CHECK_LAUNCH("grasp_closure");
    return DVQ_OK;
}
