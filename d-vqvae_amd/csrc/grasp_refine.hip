// dvq_grasp_refine, dvq_grasp_refine_rigid, dvq_grasp_refine_fingers: the push-out of generated grasps -- a few steps of descent on the
// penetration / contact proxies of contact.hip (dvq_grasp_scores), in ONE kernel per call, one workgroup of 256 threads per grasp.  The
// definitions are the ABI (include/dvq.h); this file only says how the kernel is laid out.  There is ONE kernel text, a template over
// three levels, each of which adds to the state of the one before:
//
//   GR_SHIFT    the translation t.  Per point the pull vector g = o' - hand[j] goes to one of two sets (inside, near) of three sums.
//   GR_RIGID    t AND a unit quaternion q about a pivot c (the wrist).  Per point also the arm r = hand[j] - c: a set is the ten sums
//               G = g, A = r, X = cross(r, g), Q = |r|^2.
//   GR_FINGERS  that, and one unit quaternion q_f per finger: a turn of the finger about its knuckle c_f.  Per point, for the finger f
//               of the nearest vertex, w (a x g) and w^2 |a|^2 (a = hand[j] - c_f) go to the four sums of (set, f).
//
// Everything a level does not need stands under `if constexpr`; what a level shares with the one below is the same text, so curl = 0
// gives the bits of dvq_grasp_refine_rigid, spin = 0 those of dvq_grasp_refine and steps = 0 those of dvq_grasp_scores (the planes, the
// hand load, the normals, the pair scan and the interior test are grasp_scan.h's, shared with grasp_scores_kernel).  Until the first turn
// (always at k = 0, and always with spin = 0) o' = obj - t is the shift level's expression.  Everything the two upper levels add is
// single fp32 operations (the build has -ffp-contract=off: nothing fuses), IEEE division and square root, no library function.
//
// The hand stays put: a rigid motion of the hand changes neither the hand nor its normals in the hand's own frame, so the INVERSE motion
// is applied to every object point instead (o' = R^T (obj - t - c) + c) and the hand's vertices and normals are loaded and computed ONCE
// per grasp and stay in LDS as x|y|z planes for all steps.  The object points are re-read from global memory every step (a grasp's cloud
// is 12 KB at N = 1024 and stays in L2; keeping them in registers would tie the register count to N).  A finger's turn does change the
// hand in its own frame, so once a finger has turned the vertex planes are rebuilt from the hand as given (re-read from global memory:
// 9 KB per grasp and step out of the L2, no three further LDS planes) as base + w (R_f (base - c_f) + c_f - base), and the normals are
// recomputed from them (grasp_normals, as at the start).  That happens only after a step in which some finger's turn was accepted:
// every other step leaves the planes' bits as they are.
//
// Every step is the pair scan of grasp_scan.h plus the sums above; the penetration, the two sets and three counts go through the
// canonical tree together.  After the tree every thread reads the totals and takes the same decision (key, step, turn, early end):
// nothing but LDS carries state between threads, and nothing leaves the grasp's workgroup.  The 8 P finger sums are accumulated in
// registers (a select per finger, no indexed array) and go through the tree in two more rounds over the SAME LDS arrays (the inside
// set's 4 P columns, then the near set's).  The uniform finger state -- q_f, R_f, c_f, the best iterate's q_f and two flags per finger --
// lives in 448 B of LDS behind the arrays, not in registers: thread f < P takes finger f's decision and publishes it, one barrier later
// every thread knows whether any finger moved.
//
// Resources per level (hipcc, gfx950, the Makefile's flags; no scratch anywhere; LDS beside the hand's planes, 18 720 B at V = 778):
//   GR_SHIFT     95 VGPRs, 106 SGPRs, 5 waves per SIMD; 10 arrays of 256 and the flag = 10 256 B
//   GR_RIGID    127 VGPRs, 106 SGPRs and 26 more kept in VGPR lanes, 4 waves per SIMD; 24 arrays and the flag = 24 592 B (43 312 B with the
//               planes at V = 778: three workgroups per CU, which is what bounds the occupancy)
//   GR_FINGERS  166 VGPRs, 106 SGPRs and 74 more kept in VGPR lanes, 3 waves per SIMD; the rigid level's 24 592 B and the 448 B of finger
//               state (43 760 B at V = 778: three workgroups per CU)
// The kernel takes its parameters one by one, every pointer __restrict__, and every level takes the whole list (a level's unused ones
// are null and cost it nothing): passed as one struct the fingers level needs 169 VGPRs, one more than three waves per SIMD allow.
// DESIGN.md has the measured cost of each level against the one below and of this text against the three it replaced.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

enum { GR_SHIFT = 0, GR_RIGID = 1, GR_FINGERS = 2 };

constexpr int GR_MAX_STEPS = 64;
constexpr int GR_MAX_P = 5;                 // fingers
constexpr int GR_CNTS = 3;                  // n_in, n_ct, n_nr
constexpr int GR_FSET = 4;                  // per (set, finger): X[3], Q
constexpr int gr_set(int level) { return level == GR_SHIFT ? 3 : 10; }   // per set: G[3], and from GR_RIGID on A[3], X[3], Q
constexpr int gr_sums(int level) { return 1 + 2 * gr_set(level); }       // penetration, the inside set, the near set
constexpr int gr_red(int level) { return (gr_sums(level) + GR_CNTS) * GRASP_THREADS + 4; }   // floats of LDS after the planes: the arrays and the flag
// the finger state behind them, in floats: q_f [P][4], the best iterate's [P][4], c_f [P][3], R_f [P][9], turned [P], moved [P]
constexpr int GR_QF = 0, GR_BQ = 20, GR_CF = 40, GR_RF = 55, GR_TURNED = 100, GR_MOVED = 105, GR_STATE = 112;
constexpr int gr_lds_floats(int level) { return gr_red(level) + (level == GR_FINGERS ? GR_STATE : 0); }
static_assert(GR_FSET * GR_MAX_P <= gr_sums(GR_FINGERS), "a round of finger columns must fit into the rigid level's arrays");

// The rotation matrix of the quaternion (w, x, y, z), row-major, in the operation order of include/dvq.h.
__device__ __forceinline__ void gr_matrix(float w, float x, float y, float z, float* R) {
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

// One set's share of the wrist's turn: om[c] += factor * ((X - cross(A, m))[c] / Q) with m = G / n, the quotients of the translation step.
__device__ __forceinline__ void gr_turn(const float* S, float n, float factor, float (&om)[3]) {
    const float m[3] = {S[0] / n, S[1] / n, S[2] / n};
    const float* A = S + 3;
    const float* X = S + 6;
    const float Q = S[9];
    const float tau[3] = {X[0] - (A[1] * m[2] - A[2] * m[1]), X[1] - (A[2] * m[0] - A[0] * m[2]), X[2] - (A[0] * m[1] - A[1] * m[0])};
#pragma unroll
    for (int c = 0; c < 3; ++c) om[c] = om[c] + factor * (tau[c] / Q);
}

template <int LEVEL>
__global__ __launch_bounds__(GRASP_THREADS) void grasp_refine_kernel(
    const float* __restrict__ hand, const int* __restrict__ faces, const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
    const int* __restrict__ vert_part, const float* __restrict__ vert_w, int P, const float* __restrict__ obj, long osb, long osp, long osc,
    int N, const float* __restrict__ pivot, const float* __restrict__ knuckle, float thr, int steps, float push, float pull, float spin,
    float curl, float min_w, int min_contact, float* __restrict__ offset, float* __restrict__ quat, float* __restrict__ finger_quat,
    int* __restrict__ iter, float* __restrict__ penetration, int* __restrict__ n_interior, int* __restrict__ n_contact,
    float* __restrict__ penetration0, int* __restrict__ n_interior0, int* __restrict__ n_contact0) {
    constexpr bool RIGID = LEVEL >= GR_RIGID, FINGERS = LEVEL == GR_FINGERS;
    constexpr int SET = gr_set(LEVEL), SUMS = gr_sums(LEVEL);
    extern __shared__ __align__(16) float gr_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gr_lds, V, hx, hy, hz, nx, ny, nz);
    float* part = gr_lds + grasp_hand_floats(V);                 // [SUMS][256] partial sums
    int* cnt = reinterpret_cast<int*>(part + SUMS * GRASP_THREADS);   // [GR_CNTS][256]
    int* flag = cnt + GR_CNTS * GRASP_THREADS;                   // [1]: a vertex coordinate is not finite
    float* fs = part + gr_red(LEVEL);                            // the finger state (GR_FINGERS alone has it)
    float* qf = fs + GR_QF;
    float* bq = fs + GR_BQ;
    float* cf = fs + GR_CF;
    float* Rf = fs + GR_RF;
    int* turnedf = reinterpret_cast<int*>(fs + GR_TURNED);
    int* moved = reinterpret_cast<int*>(fs + GR_MOVED);
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const float* hb = hand + b * V * 3;
    const bool fingers = FINGERS && curl > 0.0f;
    if (t == 0) *flag = 0;
    if constexpr (FINGERS) {
        if (t < 4 * P) {
            const float one = (t & 3) == 0 ? 1.0f : 0.0f;
            qf[t] = one;
            bq[t] = one;
        }
        if (t < 3 * P) cf[t] = knuckle[b * 3 * P + t];
        if (t < P) {
            turnedf[t] = 0;
            moved[t] = 0;
        }
    }
    dvq_lds_barrier();
    if (grasp_load_hand(hb, V, t, hx, hy, hz)) *flag = 1;
    dvq_lds_barrier();
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);   // once per grasp: they turn with the hand
    dvq_lds_barrier();
    bool hand_odd = *flag != 0;
    const float* ob = obj + b * osb;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;                       // the pivot
    if constexpr (RIGID) cx = pivot[3 * b], cy = pivot[3 * b + 1], cz = pivot[3 * b + 2];
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;                       // the state of iterate k: translation, quaternion, its matrix
    float qw = 1.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f;
    float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    bool turned = false;
    float best_tx = 0.0f, best_ty = 0.0f, best_tz = 0.0f, best_pen = 0.0f;
    float best_qw = 1.0f, best_qx = 0.0f, best_qy = 0.0f, best_qz = 0.0f;
    int best_k = 0, best_cls = 0, best_in = 0, best_ct = 0;
    float pen0 = 0.0f;
    int in0 = 0, ct0 = 0;
    for (int k = 0;; ++k) {
        float sum = 0.0f;
        float acc[2 * SET];                                      // the inside set, then the near set
        float fin[GR_FSET * GR_MAX_P], fnr[GR_FSET * GR_MAX_P];  // per finger: X, Q of the inside set, of the near set
#pragma unroll
        for (int c = 0; c < 2 * SET; ++c) acc[c] = 0.0f;
#pragma unroll
        for (int c = 0; c < GR_FSET * GR_MAX_P; ++c) fin[c] = 0.0f, fnr[c] = 0.0f;
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
                if (RIGID && turned) {                           // uniform over the workgroup: o' = R^T (u - c) + c
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
                    float term[SET];
                    term[0] = g[0], term[1] = g[1], term[2] = g[2];
                    if constexpr (RIGID) {
                        const float r[3] = {vx - cx, vy - cy, vz - cz};        // the arm from the pivot
                        term[3] = r[0], term[4] = r[1], term[5] = r[2];
                        term[6] = r[1] * g[2] - r[2] * g[1], term[7] = r[2] * g[0] - r[0] * g[2], term[8] = r[0] * g[1] - r[1] * g[0];
                        term[9] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                    }
                    sum += grasp_pen_term(inside, d);
#pragma unroll
                    for (int c = 0; c < SET; ++c) {
                        acc[c] += inside ? term[c] : 0.0f;
                        acc[SET + c] += near ? term[c] : 0.0f;
                    }
                    n_in += inside ? 1 : 0;
                    n_ct += d < thr ? 1 : 0;
                    n_nr += near ? 1 : 0;
                    if (fingers) {                               // uniform
                        const int fv = vert_part[j];
                        const int f = fv < P ? fv : -1;          // -1: no finger, the point adds +0 to every finger's sums
                        const int fc = f < 0 ? 0 : f;
                        const float wj = vert_w[j];
                        const float a[3] = {vx - cf[3 * fc], vy - cf[3 * fc + 1], vz - cf[3 * fc + 2]};   // the arm from the knuckle
                        const float ft[GR_FSET] = {wj * (a[1] * g[2] - a[2] * g[1]), wj * (a[2] * g[0] - a[0] * g[2]),
                                                   wj * (a[0] * g[1] - a[1] * g[0]),
                                                   (wj * wj) * ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])};
                        float fi[GR_FSET], fn[GR_FSET];
#pragma unroll
                        for (int c = 0; c < GR_FSET; ++c) fi[c] = inside ? ft[c] : 0.0f, fn[c] = near ? ft[c] : 0.0f;
#pragma unroll
                        for (int ff = 0; ff < GR_MAX_P; ++ff) {
#pragma unroll
                            for (int c = 0; c < GR_FSET; ++c) {
                                fin[GR_FSET * ff + c] += f == ff ? fi[c] : 0.0f;
                                fnr[GR_FSET * ff + c] += f == ff ? fn[c] : 0.0f;
                            }
                        }
                    }
                }
            }
        }
        part[t] = sum;
#pragma unroll
        for (int c = 0; c < 2 * SET; ++c) part[(1 + c) * GRASP_THREADS + t] = acc[c];
        cnt[t] = n_in;
        cnt[GRASP_THREADS + t] = n_ct;
        cnt[2 * GRASP_THREADS + t] = n_nr;
        dvq_lds_barrier();
        for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {       // the canonical tree, each sum on its own: part[t] += part[t + s] for t < s
            if (t < s) {
#pragma unroll
                for (int c = 0; c < SUMS; ++c) part[c * GRASP_THREADS + t] += part[c * GRASP_THREADS + t + s];
#pragma unroll
                for (int c = 0; c < GR_CNTS; ++c) cnt[c * GRASP_THREADS + t] += cnt[c * GRASP_THREADS + t + s];
            }
            dvq_lds_barrier();
        }
        const float pen = part[0];
        float tot[2 * SET];
#pragma unroll
        for (int c = 0; c < 2 * SET; ++c) tot[c] = part[(1 + c) * GRASP_THREADS];
        const int c_in = cnt[0], c_ct = cnt[GRASP_THREADS], c_nr = cnt[2 * GRASP_THREADS];
        dvq_lds_barrier();                                       // every thread has the totals before the arrays are written again
        // from here on every thread holds the same values: the decisions below are uniform over the workgroup
        const int cls = pen != pen ? 2 : (c_ct < min_contact ? 1 : 0);
        if (k == 0) pen0 = pen, in0 = c_in, ct0 = c_ct;
        if (k == 0 || cls < best_cls || (cls == best_cls && pen < best_pen)) {   // strictly smaller key; a NaN compares false
            best_tx = tx, best_ty = ty, best_tz = tz;
            best_qw = qw, best_qx = qx, best_qy = qy, best_qz = qz;
            best_k = k, best_cls = cls, best_pen = pen, best_in = c_in, best_ct = c_ct;
            if constexpr (FINGERS) {
                if (t < 4 * P) bq[t] = qf[t];                    // (thread t alone ever touches bq[t]; qf is rewritten two barriers on)
            }
        }
        if (k == steps || pen != pen) break;
        float st[3] = {0.0f, 0.0f, 0.0f}, om[3] = {0.0f, 0.0f, 0.0f};
        if (c_in > 0) {
            const float n = (float)c_in;
#pragma unroll
            for (int c = 0; c < 3; ++c) st[c] = st[c] + push * (tot[c] / n);
            if constexpr (RIGID) {
                if (spin > 0.0f && tot[9] > 0.0f) gr_turn(tot, n, push, om);
            }
        }
        if (c_nr > 0) {
            const float n = (float)c_nr;
#pragma unroll
            for (int c = 0; c < 3; ++c) st[c] = st[c] + pull * (tot[SET + c] / n);
            if constexpr (RIGID) {
                if (spin > 0.0f && tot[SET + 9] > 0.0f) gr_turn(tot + SET, n, pull, om);
            }
        }
        if (RIGID && spin > 0.0f) {
#pragma unroll
            for (int c = 0; c < 3; ++c) om[c] = spin * om[c];
        }
        bool any_moved = false;
        if (fingers) {
            float fx[2][GR_FSET];                                // thread f < P: finger f's totals of the inside set, of the near set
#pragma unroll
            for (int set = 0; set < 2; ++set) {                  // two more rounds of the tree over the same arrays
#pragma unroll
                for (int c = 0; c < GR_FSET * GR_MAX_P; ++c)     // (the columns of fingers >= P hold +0 and are not summed)
                    part[c * GRASP_THREADS + t] = set == 0 ? fin[c] : fnr[c];
                dvq_lds_barrier();
#pragma unroll 1
                for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {   // (rolled: unrolled, its hoisted masks cost a hundred SGPRs)
                    if (t < s) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)   // (no packed fp32 here: csrc/Makefile has the trail)
                        for (int c = 0; c < GR_FSET * P; ++c) part[c * GRASP_THREADS + t] += part[c * GRASP_THREADS + t + s];
                    }
                    dvq_lds_barrier();
                }
#pragma unroll
                for (int c = 0; c < GR_FSET; ++c) fx[set][c] = t < P ? part[(GR_FSET * t + c) * GRASP_THREADS] : 0.0f;
                dvq_lds_barrier();
            }
            if (t < P) {                                         // finger t's turn: the least-squares small rotation about its knuckle
                float of[3] = {0.0f, 0.0f, 0.0f};
                if (fx[0][3] > 0.0f) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) of[c] = of[c] + push * (fx[0][c] / fx[0][3]);
                }
                if (fx[1][3] > 0.0f) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) of[c] = of[c] + pull * (fx[1][c] / fx[1][3]);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) of[c] = curl * of[c];
                int mv = 0;
                if (!(of[0] == 0.0f && of[1] == 0.0f && of[2] == 0.0f)) {   // the candidate: normalised (1, of / 2) (x) q_f
                    const float h0 = 0.5f * of[0], h1 = 0.5f * of[1], h2 = 0.5f * of[2];
                    const float a0 = qf[4 * t], a1 = qf[4 * t + 1], a2 = qf[4 * t + 2], a3 = qf[4 * t + 3];
                    const float pw = ((a0 - h0 * a1) - h1 * a2) - h2 * a3;
                    const float px = ((a1 + h0 * a0) + h1 * a3) - h2 * a2;
                    const float py = ((a2 + h1 * a0) - h0 * a3) + h2 * a1;
                    const float pz = ((a3 + h2 * a0) + h0 * a2) - h1 * a1;
                    const float n2 = ((pw * pw + px * px) + py * py) + pz * pz;
                    const float inv = 1.0f / sqrtf(n2);
                    const float e0 = pw * inv, e1 = px * inv, e2 = py * inv, e3 = pz * inv;
                    if (e0 >= min_w) {                           // within max_curl of the hand as generated; a NaN refuses
                        qf[4 * t] = e0, qf[4 * t + 1] = e1, qf[4 * t + 2] = e2, qf[4 * t + 3] = e3;
                        gr_matrix(e0, e1, e2, e3, Rf + 9 * t);
                        turnedf[t] = 1;
                        mv = 1;
                    }
                }
                moved[t] = mv;
            }
            dvq_lds_barrier();
            for (int f = 0; f < P; ++f) any_moved |= moved[f] != 0;
        }
        if (st[0] == 0.0f && st[1] == 0.0f && st[2] == 0.0f && om[0] == 0.0f && om[1] == 0.0f && om[2] == 0.0f && !any_moved)
            break;                                               // the state stays: every later iterate repeats this one
        if (RIGID && turned) {                                   // the step is the hand's frame's: R st in the world
            tx = tx + ((R[0] * st[0] + R[1] * st[1]) + R[2] * st[2]);
            ty = ty + ((R[3] * st[0] + R[4] * st[1]) + R[5] * st[2]);
            tz = tz + ((R[6] * st[0] + R[7] * st[1]) + R[8] * st[2]);
        } else {
            tx = tx + st[0];
            ty = ty + st[1];
            tz = tz + st[2];
        }
        if (RIGID && !(om[0] == 0.0f && om[1] == 0.0f && om[2] == 0.0f)) {   // q <- normalised q (x) (1, om / 2): the turn is the hand's frame's
            const float h0 = 0.5f * om[0], h1 = 0.5f * om[1], h2 = 0.5f * om[2];
            const float pw = ((qw - qx * h0) - qy * h1) - qz * h2;
            const float px = ((qx + qw * h0) + qy * h2) - qz * h1;
            const float py = ((qy + qw * h1) - qx * h2) + qz * h0;
            const float pz = ((qz + qw * h2) + qx * h1) - qy * h0;
            const float n2 = ((pw * pw + px * px) + py * py) + pz * pz;
            const float inv = 1.0f / sqrtf(n2);
            qw = pw * inv, qx = px * inv, qy = py * inv, qz = pz * inv;
            turned = true;
            gr_matrix(qw, qx, qy, qz, R);
        }
        if (any_moved) {                                         // the hand of the next iterate: rebuilt from the hand as given
            bool odd = false;
            for (int v = t; v < V; v += GRASP_THREADS) {
                const float bx = hb[3 * v], by = hb[3 * v + 1], bz = hb[3 * v + 2];
                float x = bx, y = by, z = bz;
                const int f = vert_part[v];
                if (f >= 0 && f < P && turnedf[f] != 0) {
                    const float w = vert_w[v];
                    const float* M = Rf + 9 * f;
                    const float kx = cf[3 * f], ky = cf[3 * f + 1], kz = cf[3 * f + 2];
                    const float dx = bx - kx, dy = by - ky, dz = bz - kz;
                    const float rx = ((M[0] * dx + M[1] * dy) + M[2] * dz) + kx;
                    const float ry = ((M[3] * dx + M[4] * dy) + M[5] * dz) + ky;
                    const float rz = ((M[6] * dx + M[7] * dy) + M[8] * dz) + kz;
                    x = bx + w * (rx - bx);
                    y = by + w * (ry - by);
                    z = bz + w * (rz - bz);
                }
                hx[v] = x;
                hy[v] = y;
                hz[v] = z;
                odd |= !grasp_finite(x, y, z);
            }
            if (odd) *flag = 1;
            dvq_lds_barrier();
            grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);   // recomputed, not rotated: the blend is no rigid motion
            dvq_lds_barrier();
            hand_odd = *flag != 0;
        }
    }
    if constexpr (FINGERS) {
        if (t < 4 * P) finger_quat[b * 4 * P + t] = bq[t];       // thread t's own writes
    }
    if (t == 0) {
        offset[3 * b] = best_tx;
        offset[3 * b + 1] = best_ty;
        offset[3 * b + 2] = best_tz;
        if constexpr (RIGID) {
            quat[4 * b] = best_qw;
            quat[4 * b + 1] = best_qx;
            quat[4 * b + 2] = best_qy;
            quat[4 * b + 3] = best_qz;
        }
        iter[b] = best_k;
        penetration[b] = best_pen;
        n_interior[b] = best_in;
        n_contact[b] = best_ct;
        if constexpr (FINGERS) {
            penetration0[b] = pen0;
            n_interior0[b] = in0;
            n_contact0[b] = ct0;
        }
    }
}

template <class T>
T* gr_at(T* p, int64_t i) { return p ? p + i : p; }              // a level's unused pointers are null and stay null

// One level's launches: `what` is the entry point's name without dvq_, `bytes` its traffic per grasp; the other parameters are
// dvq_grasp_refine_fingers' (a lower level passes null and zero for what it does not have).
template <int LEVEL>
int gr_launch(const char* what, double bytes, const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
              const int32_t* vert_part, const float* vert_w, int P, const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride,
              int64_t obj_coord_stride, int64_t B, int N, const float* pivot, const float* knuckle, float contact_threshold, int steps,
              float push, float pull, float spin, float curl, float min_w, int min_contact, float* offset, float* quat, float* finger_quat,
              int32_t* iter, float* penetration, int32_t* n_interior, int32_t* n_contact, float* penetration0, int32_t* n_interior0,
              int32_t* n_contact0, dvq_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = grasp_lds_bytes(V, gr_lds_floats(LEVEL));
    static DvqOncePerDevice attr_once;                           // one per level
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_refine_kernel<LEVEL>),
                                grasp_lds_bytes(GRASP_MAX_V, gr_lds_floats(LEVEL)), what));
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // at most steps + 1 scans of 8 FLOPs per (point, vertex) pair (a grasp may end early)
        DVQ_PROF(what, 8.0 * nb * N * V * (steps + 1), (double)nb * bytes, st);
        DVQ_LAUNCH(grasp_refine_kernel<LEVEL>, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face,
                   V, vert_part, vert_w, P, obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride,
                   (long)obj_coord_stride, N, gr_at(pivot, 3 * b0), gr_at(knuckle, 3 * P * b0), contact_threshold, steps, push, pull, spin,
                   curl, min_w, min_contact, offset + 3 * b0, gr_at(quat, 4 * b0), gr_at(finger_quat, 4 * P * b0), iter + b0,
                   penetration + b0, n_interior + b0, n_contact + b0, gr_at(penetration0, b0), gr_at(n_interior0, b0),
                   gr_at(n_contact0, b0));
    });
    DVQ_CHECK_LAUNCH(what);
    return DVQ_OK;
}

}  // namespace

extern "C" int dvq_grasp_refine(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                int64_t B, int N, float contact_threshold, int steps, float push, float pull, int min_contact,
                                float* offset, int32_t* iter, float* penetration, int32_t* n_interior, int32_t* n_contact,
                                dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V, "grasp_refine: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)",
                GRASP_MAX_V, (long)B, N, V);
    DVQ_REQUIRE(steps >= 0 && steps <= GR_MAX_STEPS, "grasp_refine: need 0 <= steps <= %d (got %d)", GR_MAX_STEPS, steps);
    DVQ_REQUIRE(push >= 0.0f && push < INFINITY && pull >= 0.0f && pull < INFINITY,
                "grasp_refine: push and pull must be finite and >= 0 (got %g, %g)", (double)push, (double)pull);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && offset && iter && penetration && n_interior && n_contact,
                "grasp_refine: null pointer");
    // in: the hand and the topology once, the cloud once per scan; out: 28 B per grasp
    return gr_launch<GR_SHIFT>("grasp_refine", (double)V * 12 + (double)N * 12 * (steps + 1) + 28, hand, faces, vf_off, vf_face, V,
                               /*vert_part*/ nullptr, /*vert_w*/ nullptr, /*P*/ 0, obj, obj_batch_stride, obj_point_stride,
                               obj_coord_stride, B, N, /*pivot*/ nullptr, /*knuckle*/ nullptr, contact_threshold, steps, push, pull,
                               /*spin*/ 0.0f, /*curl*/ 0.0f, /*min_w*/ 0.0f, min_contact, offset, /*quat*/ nullptr, /*finger_quat*/ nullptr,
                               iter, penetration, n_interior, n_contact, /*iterate 0's scores*/ nullptr, nullptr, nullptr, stream);
}

extern "C" int dvq_grasp_refine_rigid(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                      const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                                      int64_t B, int N, const float* pivot, float contact_threshold, int steps, float push, float pull,
                                      float spin, int min_contact, float* offset, float* quat, int32_t* iter, float* penetration,
                                      int32_t* n_interior, int32_t* n_contact, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V,
                "grasp_refine_rigid: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)", GRASP_MAX_V, (long)B, N, V);
    DVQ_REQUIRE(steps >= 0 && steps <= GR_MAX_STEPS, "grasp_refine_rigid: need 0 <= steps <= %d (got %d)", GR_MAX_STEPS, steps);
    DVQ_REQUIRE(push >= 0.0f && push < INFINITY && pull >= 0.0f && pull < INFINITY && spin >= 0.0f && spin < INFINITY,
                "grasp_refine_rigid: push, pull and spin must be finite and >= 0 (got %g, %g, %g)", (double)push, (double)pull,
                (double)spin);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && pivot && offset && quat && iter && penetration && n_interior && n_contact,
                "grasp_refine_rigid: null pointer");
    // in: the hand, the pivot and the topology once, the cloud once per scan; out: 44 B per grasp
    return gr_launch<GR_RIGID>("grasp_refine_rigid", (double)V * 12 + 12 + (double)N * 12 * (steps + 1) + 44, hand, faces, vf_off, vf_face, V,
                               /*vert_part*/ nullptr, /*vert_w*/ nullptr, /*P*/ 0, obj, obj_batch_stride, obj_point_stride,
                               obj_coord_stride, B, N, pivot, /*knuckle*/ nullptr, contact_threshold, steps, push, pull, spin,
                               /*curl*/ 0.0f, /*min_w*/ 0.0f, min_contact, offset, quat, /*finger_quat*/ nullptr, iter, penetration,
                               n_interior, n_contact, /*iterate 0's scores*/ nullptr, nullptr, nullptr, stream);
}

extern "C" int dvq_grasp_refine_fingers(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                                        const int32_t* vert_part, const float* vert_w, int P, const float* obj, int64_t obj_batch_stride,
                                        int64_t obj_point_stride, int64_t obj_coord_stride, int64_t B, int N, const float* pivot,
                                        const float* knuckle, float contact_threshold, int steps, float push, float pull, float spin,
                                        float curl, float min_w, int min_contact, float* offset, float* quat, float* finger_quat,
                                        int32_t* iter, float* penetration, int32_t* n_interior, int32_t* n_contact, float* penetration0,
                                        int32_t* n_interior0, int32_t* n_contact0, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V,
                "grasp_refine_fingers: need B >= 0, N >= 1, 1 <= V <= %d (got B=%ld N=%d V=%d)", GRASP_MAX_V, (long)B, N, V);
    DVQ_REQUIRE(P >= 1 && P <= GR_MAX_P, "grasp_refine_fingers: need 1 <= P <= %d (got %d)", GR_MAX_P, P);
    DVQ_REQUIRE(steps >= 0 && steps <= GR_MAX_STEPS, "grasp_refine_fingers: need 0 <= steps <= %d (got %d)", GR_MAX_STEPS, steps);
    DVQ_REQUIRE(push >= 0.0f && push < INFINITY && pull >= 0.0f && pull < INFINITY && spin >= 0.0f && spin < INFINITY && curl >= 0.0f &&
                    curl < INFINITY,
                "grasp_refine_fingers: push, pull, spin and curl must be finite and >= 0 (got %g, %g, %g, %g)", (double)push, (double)pull,
                (double)spin, (double)curl);
    DVQ_REQUIRE(min_w >= 0.0f && min_w <= 1.0f, "grasp_refine_fingers: need 0 <= min_w <= 1, the cosine of half of max_curl (got %g)",
                (double)min_w);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && vert_part && vert_w && obj && pivot && knuckle && offset && quat && finger_quat &&
                    iter && penetration && n_interior && n_contact && penetration0 && n_interior0 && n_contact0,
                "grasp_refine_fingers: null pointer");
    // in: the topology, the pivot and the knuckles once, the cloud once per scan, the hand once and again after every step that curls a
    // finger; out: 56 + 16 P B
    return gr_launch<GR_FINGERS>("grasp_refine_fingers",
                                 (double)V * 12 * (steps + 1) + 12 + 12.0 * P + (double)N * 12 * (steps + 1) + 56 + 16.0 * P, hand, faces,
                                 vf_off, vf_face, V, vert_part, vert_w, P, obj, obj_batch_stride, obj_point_stride, obj_coord_stride, B, N,
                                 pivot, knuckle, contact_threshold, steps, push, pull, spin, curl, min_w, min_contact, offset, quat,
                                 finger_quat, iter, penetration, n_interior, n_contact, penetration0, n_interior0, n_contact0, stream);
}
