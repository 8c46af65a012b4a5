// dvq_grasp_refine: translation push-out of generated grasps -- a few steps of descent on the penetration / contact proxies of
// contact.hip (dvq_grasp_scores) with respect to the hand's rigid translation, in ONE kernel, one workgroup of 256 threads per
// grasp.  The definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// The hand never moves: the translation t is subtracted from every object point instead (o' = obj - t), so the hand's vertices
// and its normals -- which a translation does not change -- are loaded and computed ONCE per grasp and stay in LDS as x|y|z
// planes for all steps (grasp_scan.h).  The object points are re-read from global memory every step (a grasp's
// cloud is 12 KB at N = 1024 and stays in L2; keeping them in registers would tie the register count to N).  Every step is the
// pair scan of grasp_scan.h plus, per point, the pull vector g = o' - hand[j] added to one of two accumulators; seven fp32
// sums and three counts go through the canonical tree together.  After the tree every thread reads the ten totals and takes the
// same decision (key, step, early end): nothing but LDS carries state between threads, and nothing leaves the grasp's workgroup.
//
// The planes, the hand load, the normals, the pair scan and the interior test are grasp_scan.h's, shared with grasp_scores_kernel and
// grasp_wrench_kernel: steps = 0 gives the bits of dvq_grasp_scores because it runs the same text.  This kernel's own part is
// o' = obj - t, the pull vectors and the step rule.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GR_MAX_STEPS = 64;
constexpr int GR_SUMS = 7;                  // penetration, S_in[3], S_nr[3]
constexpr int GR_CNTS = 3;                  // n_in, n_ct, n_nr
constexpr int GR_RED = (GR_SUMS + GR_CNTS) * GRASP_THREADS + 4; // floats of LDS after the planes: the arrays and the flag (10 KB)

__global__ __launch_bounds__(GRASP_THREADS) void grasp_refine_kernel(const float* __restrict__ hand, const int* __restrict__ faces,
                                                                     const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
                                                                     const float* __restrict__ obj, long osb, long osp, long osc, int N,
                                                                     float thr, int steps, float push, float pull, int min_contact,
                                                                     float* __restrict__ offset, int* __restrict__ iter,
                                                                     float* __restrict__ penetration, int* __restrict__ n_interior,
                                                                     int* __restrict__ n_contact) {
    extern __shared__ __align__(16) float gr_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gr_lds, V, hx, hy, hz, nx, ny, nz);
    float* part = gr_lds + grasp_hand_floats(V);                 // [GR_SUMS][256] partial sums
    int* cnt = reinterpret_cast<int*>(part + GR_SUMS * GRASP_THREADS);   // [GR_CNTS][256]
    int* flag = cnt + GR_CNTS * GRASP_THREADS;                   // [1]: a vertex coordinate is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    if (t == 0) *flag = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) *flag = 1;
    dvq_lds_barrier();
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);   // once per grasp
    dvq_lds_barrier();
    const bool hand_odd = *flag != 0;
    const float* ob = obj + b * osb;
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;                       // the translation of iterate k
    float best_tx = 0.0f, best_ty = 0.0f, best_tz = 0.0f, best_pen = 0.0f;
    int best_k = 0, best_cls = 0, best_in = 0, best_ct = 0;
    for (int k = 0;; ++k) {
        float sum = 0.0f, ix = 0.0f, iy = 0.0f, iz = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f;
        int n_in = 0, n_ct = 0, n_nr = 0;
        for (long p0 = t; p0 < N; p0 += GRASP_THREADS * GRASP_P) {   // points p0 + u * 256: thread t's points, ascending
            float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P];
            int bi[GRASP_P];
            bool slow = hand_odd;
#pragma unroll
            for (int u = 0; u < GRASP_P; ++u) {
                const long p = p0 + u * GRASP_THREADS;
                const bool in = p < N;
                sx[u] = (in ? ob[p * osp] : 0.f) - tx;           // o' = obj - t; obj itself at k = 0 (t = +0)
                sy[u] = (in ? ob[p * osp + osc] : 0.f) - ty;
                sz[u] = (in ? ob[p * osp + 2 * osc] : 0.f) - tz;
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
                    const float gx = sx[u] - hx[j], gy = sy[u] - hy[j], gz = sz[u] - hz[j];   // the pull vector
                    sum += grasp_pen_term(inside, d);
                    ix += inside ? gx : 0.0f;
                    iy += inside ? gy : 0.0f;
                    iz += inside ? gz : 0.0f;
                    rx += near ? gx : 0.0f;
                    ry += near ? gy : 0.0f;
                    rz += near ? gz : 0.0f;
                    n_in += inside ? 1 : 0;
                    n_ct += d < thr ? 1 : 0;
                    n_nr += near ? 1 : 0;
                }
            }
        }
        part[t] = sum;
        part[GRASP_THREADS + t] = ix;
        part[2 * GRASP_THREADS + t] = iy;
        part[3 * GRASP_THREADS + t] = iz;
        part[4 * GRASP_THREADS + t] = rx;
        part[5 * GRASP_THREADS + t] = ry;
        part[6 * GRASP_THREADS + t] = rz;
        cnt[t] = n_in;
        cnt[GRASP_THREADS + t] = n_ct;
        cnt[2 * GRASP_THREADS + t] = n_nr;
        dvq_lds_barrier();
        for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {       // the canonical tree, each sum on its own: part[t] += part[t + s] for t < s
            if (t < s) {
#pragma unroll
                for (int c = 0; c < GR_SUMS; ++c) part[c * GRASP_THREADS + t] += part[c * GRASP_THREADS + t + s];
#pragma unroll
                for (int c = 0; c < GR_CNTS; ++c) cnt[c * GRASP_THREADS + t] += cnt[c * GRASP_THREADS + t + s];
            }
            dvq_lds_barrier();
        }
        const float pen = part[0];
        const float s_in[3] = {part[GRASP_THREADS], part[2 * GRASP_THREADS], part[3 * GRASP_THREADS]};
        const float s_nr[3] = {part[4 * GRASP_THREADS], part[5 * GRASP_THREADS], part[6 * GRASP_THREADS]};
        const int c_in = cnt[0], c_ct = cnt[GRASP_THREADS], c_nr = cnt[2 * GRASP_THREADS];
        dvq_lds_barrier();                                       // every thread has the totals before the next step's partial sums land
        // from here on every thread holds the same values: the decisions below are uniform over the workgroup
        const int cls = pen != pen ? 2 : (c_ct < min_contact ? 1 : 0);
        if (k == 0 || cls < best_cls || (cls == best_cls && pen < best_pen)) {   // strictly smaller key; a NaN compares false
            best_tx = tx, best_ty = ty, best_tz = tz;
            best_k = k, best_cls = cls, best_pen = pen, best_in = c_in, best_ct = c_ct;
        }
        if (k == steps || pen != pen) break;
        float st[3] = {0.0f, 0.0f, 0.0f};
        if (c_in > 0) {
            const float n = (float)c_in;
#pragma unroll
            for (int c = 0; c < 3; ++c) st[c] = st[c] + push * (s_in[c] / n);
        }
        if (c_nr > 0) {
            const float n = (float)c_nr;
#pragma unroll
            for (int c = 0; c < 3; ++c) st[c] = st[c] + pull * (s_nr[c] / n);
        }
        if (st[0] == 0.0f && st[1] == 0.0f && st[2] == 0.0f) break;   // t stays: every later iterate repeats this one
        tx = tx + st[0];
        ty = ty + st[1];
        tz = tz + st[2];
    }
    if (t == 0) {
        offset[3 * b] = best_tx;
        offset[3 * b + 1] = best_ty;
        offset[3 * b + 2] = best_tz;
        iter[b] = best_k;
        penetration[b] = best_pen;
        n_interior[b] = best_in;
        n_contact[b] = best_ct;
    }
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
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = grasp_lds_bytes(V, GR_RED);
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_refine_kernel), grasp_lds_bytes(GRASP_MAX_V, GR_RED),
                                "grasp_refine"));
    for (int64_t b0 = 0; b0 < B; b0 += 65535) {                  // the grid-dimension limit the neighbouring entry points chunk by
        const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
        // at most steps + 1 scans of 8 FLOPs per (point, vertex) pair (a grasp may end early); in: the hand and the topology once,
        // the cloud once per scan; out: 28 B per grasp
        DVQ_PROF("grasp_refine", 8.0 * nb * N * V * (steps + 1), (double)nb * ((double)V * 12 + (double)N * 12 * (steps + 1) + 28), st);
        DVQ_LAUNCH(grasp_refine_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, steps, push, pull, min_contact, offset + 3 * b0, iter + b0, penetration + b0, n_interior + b0,
                   n_contact + b0);
    }
    DVQ_CHECK_LAUNCH("grasp_refine");
    return DVQ_OK;
}
