// dvq_grasp_refine_rigid: rigid push-out of generated grasps -- grasp_refine.hip's descent with the other half of a rigid motion: the
// state is a translation t AND a unit quaternion q about a pivot c (the wrist), in ONE kernel, one workgroup of 256 threads per
// grasp.  The definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// The hand never moves and never turns: the inverse motion is applied to every object point instead (o' = R^T (obj - t - c) + c), so
// the hand's vertices and its normals -- which turn with the hand, and so stay what they are in the hand's frame -- are loaded and
// computed ONCE per grasp and stay in LDS as x|y|z planes for all steps (grasp_scan.h).  The object points are re-read from global
// memory every step.  Every step is the pair scan of grasp_scan.h plus, per point, the pull vector g = o' - hand[j] and the arm
// r = hand[j] - c, added as g, r, cross(r, g) and |r|^2 to one of two sets of ten accumulators; 21 fp32 sums and three counts go
// through the canonical tree together.  After the tree every thread reads the 24 totals and takes the same decision (key, step,
// turn, early end): nothing but LDS carries state between threads, and nothing leaves the grasp's workgroup.
//
// Until the first turn (always at k = 0, and always with spin = 0) o' = obj - t is grasp_refine_kernel's expression, and the scan, the
// interior test, the masks and the translation step are the same text: spin = 0 gives the bits of dvq_grasp_refine and steps = 0
// those of dvq_grasp_scores.  Everything this kernel adds is single fp32 operations (the build has -ffp-contract=off: nothing
// fuses), IEEE division and square root, no library function.
//
// Resources (hipcc, gfx950, the Makefile's flags): 127 VGPRs, 106 SGPRs and 26 more kept in VGPR lanes, no scratch, 4 waves per SIMD.
// LDS: 24 arrays of 256 and the flag = 24 592 B beside the hand's planes (73 744 B at V = 2048, 43 312 B at V = 778: three workgroups
// per CU, which is what bounds the occupancy; DESIGN.md has the measured cost against grasp_refine_kernel).
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GRR_MAX_STEPS = 64;
constexpr int GRR_SET = 10;                 // per set: G[3], A[3], X[3], Q
constexpr int GRR_SUMS = 1 + 2 * GRR_SET;   // penetration, the inside set, the near set
constexpr int GRR_CNTS = 3;                 // n_in, n_ct, n_nr
constexpr int GRR_RED = (GRR_SUMS + GRR_CNTS) * GRASP_THREADS + 4;   // floats of LDS after the planes: the arrays and the flag

// The rotation matrix of the quaternion (w, x, y, z), row-major, in the operation order of include/dvq.h.
__device__ __forceinline__ void grr_matrix(float w, float x, float y, float z, float (&R)[9]) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0f - 2.0f * (yy + zz);
    R[1] = 2.0f * (xy - wz);
    R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);
    R[4] = 1.0f - 2.0f * (xx + zz);
    R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);
    R[7] = 2.0f * (yz + wx);
    R[8] = 1.0f - 2.0f * (xx + yy);
}

// One set's share of the turn: om[c] += factor * ((X - cross(A, m))[c] / Q) with m = G / n, the quotients of the translation step.
__device__ __forceinline__ void grr_turn(const float* S, float n, float factor, float (&om)[3]) {
    const float m[3] = {S[0] / n, S[1] / n, S[2] / n};
    const float* A = S + 3;
    const float* X = S + 6;
    const float Q = S[9];
    const float tau[3] = {X[0] - (A[1] * m[2] - A[2] * m[1]), X[1] - (A[2] * m[0] - A[0] * m[2]), X[2] - (A[0] * m[1] - A[1] * m[0])};
#pragma unroll
    for (int c = 0; c < 3; ++c) om[c] = om[c] + factor * (tau[c] / Q);
}

__global__ __launch_bounds__(GRASP_THREADS) void grasp_refine_rigid_kernel(
    const float* __restrict__ hand, const int* __restrict__ faces, const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
    const float* __restrict__ obj, long osb, long osp, long osc, int N, const float* __restrict__ pivot, float thr, int steps, float push,
    float pull, float spin, int min_contact, float* __restrict__ offset, float* __restrict__ quat, int* __restrict__ iter,
    float* __restrict__ penetration, int* __restrict__ n_interior, int* __restrict__ n_contact) {
    extern __shared__ __align__(16) float grr_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(grr_lds, V, hx, hy, hz, nx, ny, nz);
    float* part = grr_lds + grasp_hand_floats(V);                // [GRR_SUMS][256] partial sums
    int* cnt = reinterpret_cast<int*>(part + GRR_SUMS * GRASP_THREADS);   // [GRR_CNTS][256]
    int* flag = cnt + GRR_CNTS * GRASP_THREADS;                  // [1]: a vertex coordinate is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    if (t == 0) *flag = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) *flag = 1;
    dvq_lds_barrier();
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);   // once per grasp: they turn with the hand
    dvq_lds_barrier();
    const bool hand_odd = *flag != 0;
    const float* ob = obj + b * osb;
    const float cx = pivot[3 * b], cy = pivot[3 * b + 1], cz = pivot[3 * b + 2];
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;                       // the state of iterate k: translation, quaternion, its matrix
    float qw = 1.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f;
    float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    bool turned = false;
    float best_tx = 0.0f, best_ty = 0.0f, best_tz = 0.0f, best_pen = 0.0f;
    float best_qw = 1.0f, best_qx = 0.0f, best_qy = 0.0f, best_qz = 0.0f;
    int best_k = 0, best_cls = 0, best_in = 0, best_ct = 0;
    for (int k = 0;; ++k) {
        float sum = 0.0f;
        float acc[2 * GRR_SET];                                  // the inside set, then the near set: G, A, X, Q
#pragma unroll
        for (int c = 0; c < 2 * GRR_SET; ++c) acc[c] = 0.0f;
        int n_in = 0, n_ct = 0, n_nr = 0;
        for (long p0 = t; p0 < N; p0 += GRASP_THREADS * GRASP_P) {   // points p0 + u * 256: thread t's points, ascending
            float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P];
            int bi[GRASP_P];
            bool slow = hand_odd;
#pragma unroll
            for (int u = 0; u < GRASP_P; ++u) {
                const long p = p0 + u * GRASP_THREADS;
                const bool in = p < N;
                const float ux = (in ? ob[p * osp] : 0.f) - tx;  // u = obj - t; obj itself at k = 0 (t = +0)
                const float uy = (in ? ob[p * osp + osc] : 0.f) - ty;
                const float uz = (in ? ob[p * osp + 2 * osc] : 0.f) - tz;
                if (turned) {                                    // uniform over the workgroup: o' = R^T (u - c) + c
                    const float wx = ux - cx, wy = uy - cy, wz = uz - cz;
                    sx[u] = ((R[0] * wx + R[3] * wy) + R[6] * wz) + cx;
                    sy[u] = ((R[1] * wx + R[4] * wy) + R[7] * wz) + cy;
                    sz[u] = ((R[2] * wx + R[5] * wy) + R[8] * wz) + cz;
                } else {
                    sx[u] = ux, sy[u] = uy, sz[u] = uz;
                }
                slow |= !grasp_finite(sx[u], sy[u], sz[u]);
            }
            grasp_scan4(hx, hy, hz, V, slow, sx, sy, sz, best, bi);
#pragma unroll
            for (int u = 0; u < GRASP_P; ++u) {
                if (p0 + u * GRASP_THREADS < N) {
                    const int j = bi[u];                         // 0 <= j < V: the scan always takes j = 0
                    const float d = best[u];
                    const bool inside = grasp_inside(hx, hy, hz, nx, ny, nz, j, sx[u], sy[u], sz[u]);
                    const bool near = !inside && d < thr;
                    const float vx = hx[j], vy = hy[j], vz = hz[j];
                    const float g[3] = {sx[u] - vx, sy[u] - vy, sz[u] - vz};   // the pull vector
                    const float r[3] = {vx - cx, vy - cy, vz - cz};            // the arm from the pivot
                    const float term[GRR_SET] = {g[0], g[1], g[2], r[0], r[1], r[2],
                                                 r[1] * g[2] - r[2] * g[1], r[2] * g[0] - r[0] * g[2], r[0] * g[1] - r[1] * g[0],
                                                 (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]};
                    sum += grasp_pen_term(inside, d);
#pragma unroll
                    for (int c = 0; c < GRR_SET; ++c) {
                        acc[c] += inside ? term[c] : 0.0f;
                        acc[GRR_SET + c] += near ? term[c] : 0.0f;
                    }
                    n_in += inside ? 1 : 0;
                    n_ct += d < thr ? 1 : 0;
                    n_nr += near ? 1 : 0;
                }
            }
        }
        part[t] = sum;
#pragma unroll
        for (int c = 0; c < 2 * GRR_SET; ++c) part[(1 + c) * GRASP_THREADS + t] = acc[c];
        cnt[t] = n_in;
        cnt[GRASP_THREADS + t] = n_ct;
        cnt[2 * GRASP_THREADS + t] = n_nr;
        dvq_lds_barrier();
        for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {       // the canonical tree, each sum on its own: part[t] += part[t + s] for t < s
            if (t < s) {
#pragma unroll
                for (int c = 0; c < GRR_SUMS; ++c) part[c * GRASP_THREADS + t] += part[c * GRASP_THREADS + t + s];
#pragma unroll
                for (int c = 0; c < GRR_CNTS; ++c) cnt[c * GRASP_THREADS + t] += cnt[c * GRASP_THREADS + t + s];
            }
            dvq_lds_barrier();
        }
        const float pen = part[0];
        float tot[2 * GRR_SET];
#pragma unroll
        for (int c = 0; c < 2 * GRR_SET; ++c) tot[c] = part[(1 + c) * GRASP_THREADS];
        const int c_in = cnt[0], c_ct = cnt[GRASP_THREADS], c_nr = cnt[2 * GRASP_THREADS];
        dvq_lds_barrier();                                       // every thread has the totals before the next step's partial sums land
        // from here on every thread holds the same values: the decisions below are uniform over the workgroup
        const int cls = pen != pen ? 2 : (c_ct < min_contact ? 1 : 0);
        if (k == 0 || cls < best_cls || (cls == best_cls && pen < best_pen)) {   // strictly smaller key; a NaN compares false
            best_tx = tx, best_ty = ty, best_tz = tz;
            best_qw = qw, best_qx = qx, best_qy = qy, best_qz = qz;
            best_k = k, best_cls = cls, best_pen = pen, best_in = c_in, best_ct = c_ct;
        }
        if (k == steps || pen != pen) break;
        float st[3] = {0.0f, 0.0f, 0.0f}, om[3] = {0.0f, 0.0f, 0.0f};
        if (c_in > 0) {
            const float n = (float)c_in;
#pragma unroll
            for (int c = 0; c < 3; ++c) st[c] = st[c] + push * (tot[c] / n);
            if (spin > 0.0f && tot[9] > 0.0f) grr_turn(tot, n, push, om);
        }
        if (c_nr > 0) {
            const float n = (float)c_nr;
#pragma unroll
            for (int c = 0; c < 3; ++c) st[c] = st[c] + pull * (tot[GRR_SET + c] / n);
            if (spin > 0.0f && tot[GRR_SET + 9] > 0.0f) grr_turn(tot + GRR_SET, n, pull, om);
        }
        if (spin > 0.0f) {
#pragma unroll
            for (int c = 0; c < 3; ++c) om[c] = spin * om[c];
        }
        if (st[0] == 0.0f && st[1] == 0.0f && st[2] == 0.0f && om[0] == 0.0f && om[1] == 0.0f && om[2] == 0.0f)
            break;                                               // the state stays: every later iterate repeats this one
        if (turned) {                                            // the step is the hand's frame's: R st in the world
            tx = tx + ((R[0] * st[0] + R[1] * st[1]) + R[2] * st[2]);
            ty = ty + ((R[3] * st[0] + R[4] * st[1]) + R[5] * st[2]);
            tz = tz + ((R[6] * st[0] + R[7] * st[1]) + R[8] * st[2]);
        } else {
            tx = tx + st[0];
            ty = ty + st[1];
            tz = tz + st[2];
        }
        if (!(om[0] == 0.0f && om[1] == 0.0f && om[2] == 0.0f)) {   // q <- normalised q (x) (1, om / 2): the turn is the hand's frame's
            const float h0 = 0.5f * om[0], h1 = 0.5f * om[1], h2 = 0.5f * om[2];
            const float pw = ((qw - qx * h0) - qy * h1) - qz * h2;
            const float px = ((qx + qw * h0) + qy * h2) - qz * h1;
            const float py = ((qy + qw * h1) - qx * h2) + qz * h0;
            const float pz = ((qz + qw * h2) + qx * h1) - qy * h0;
            const float n2 = ((pw * pw + px * px) + py * py) + pz * pz;
            const float inv = 1.0f / sqrtf(n2);
            qw = pw * inv, qx = px * inv, qy = py * inv, qz = pz * inv;
            turned = true;
            grr_matrix(qw, qx, qy, qz, R);
        }
    }
    if (t == 0) {
        offset[3 * b] = best_tx;
        offset[3 * b + 1] = best_ty;
        offset[3 * b + 2] = best_tz;
        quat[4 * b] = best_qw;
        quat[4 * b + 1] = best_qx;
        quat[4 * b + 2] = best_qy;
        quat[4 * b + 3] = best_qz;
        iter[b] = best_k;
        penetration[b] = best_pen;
        n_interior[b] = best_in;
        n_contact[b] = best_ct;
    }
}

}  // namespace

extern "C" int dvq_grasp_refine_rigid(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                      const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                      int64_t B, int N, const float* pivot, float contact_threshold, int steps, float push, float pull,
                                      float spin, int min_contact, float* offset, float* quat, int32_t* iter, float* penetration,
                                      int32_t* n_interior, int32_t* n_contact, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V,
                "grasp_refine_rigid: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)", GRASP_MAX_V, (long)B, N, V);
    DVQ_REQUIRE(steps >= 0 && steps <= GRR_MAX_STEPS, "grasp_refine_rigid: need 0 <= steps <= %d (got %d)", GRR_MAX_STEPS, steps);
    DVQ_REQUIRE(push >= 0.0f && push < INFINITY && pull >= 0.0f && pull < INFINITY && spin >= 0.0f && spin < INFINITY,
                "grasp_refine_rigid: push, pull and spin must be finite and >= 0 (got %g, %g, %g)", (double)push, (double)pull,
                (double)spin);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && pivot && offset && quat && iter && penetration && n_interior && n_contact,
                "grasp_refine_rigid: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = grasp_lds_bytes(V, GRR_RED);
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_refine_rigid_kernel),
                                grasp_lds_bytes(GRASP_MAX_V, GRR_RED), "grasp_refine_rigid"));
    for (int64_t b0 = 0; b0 < B; b0 += 65535) {                  // the grid-dimension limit the neighbouring entry points chunk by
        const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
        // at most steps + 1 scans of 8 FLOPs per (point, vertex) pair (a grasp may end early); in: the hand, the pivot and the
        // topology once, the cloud once per scan; out: 44 B per grasp
        DVQ_PROF("grasp_refine_rigid", 8.0 * nb * N * V * (steps + 1),
                 (double)nb * ((double)V * 12 + 12 + (double)N * 12 * (steps + 1) + 44), st);
        DVQ_LAUNCH(grasp_refine_rigid_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face,
                   V, obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   pivot + 3 * b0, contact_threshold, steps, push, pull, spin, min_contact, offset + 3 * b0, quat + 4 * b0, iter + b0,
                   penetration + b0, n_interior + b0, n_contact + b0);
    }
    DVQ_CHECK_LAUNCH("grasp_refine_rigid");
    return DVQ_OK;
}
