// dvq_grasp_ttt: the two terms of the reference's test-time loss (utils/loss.py: TTT_loss -- the penetration term and the hand-centric
// Contact_loss) AND their gradient with respect to the hand's vertices in ONE kernel, one workgroup of 256 threads per grasp; nothing
// of size [B,N] or [B,N,V] reaches HBM.  The definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// LDS: the six planes of grasp_scan.h (its loaders, unchanged), one packed word per object point, three reduction rows of 256, the
// flag, and a seventh plane of one BYTE per vertex: 1 where the vertex is a contact target (the padding up to VP is 0).  At V = 778,
// N = 1024 that is 18 720 + 4096 + 3072 + 16 + 780 = 26 684 B: six workgroups share the 160 KB of a CU.
//
// Scan phase.  A COPY of the walk of grasp_scan.h (grasp_walk4: keep the two in step) and of its tile load, with a second running
// minimum.  Called through the helpers the kernel gives the same bits and the same scan and gather loops, but its launch with the
// gradient measured 0.6 - 0.7 % slower at N = 3000 in two sessions and the listing does not say why ("The walk against the
// parent, measured"); with this text the kernel's listing is the one it had.  A vertex that is no target contributes +inf to the
// second minimum, which is never below the running best (one bit test per vertex, one select more per pair).  Both minima come out
// of the one pass over the planes.  Every point leaves one word: bits 0..11 the vertex its penetration term pulls on (j_p if
// inside_p, else 0xfff), bits 12..23 the vertex its contact term pulls on (jc_p if contact_p, else 0xfff).  The three scores and
// the contact sum are reduced as dvq_grasp_scores reduces (the two counts share one integer: both are at most 16 384).
//
// Gather phase (only with grad_hand).  Thread t owns the vertices t, t + 256, ...; it walks the words in ascending p -- every lane
// reads the same address, a broadcast -- and adds hand[v] - obj[p] for the points that name one of its vertices: two compares per
// point find them (v & 255 == t), the rest runs only on a hit.  No atomics: every sum has one owner and one order.  A hand of more
// than 1024 vertices takes a second walk.
//
// A row with a non-finite coordinate: the points of such a row go through grasp_scan4's exact path, so the three scores are
// dvq_grasp_scores'; the flag (set by the hand's load or by the thread that meets the point) is final after the scan, and the whole
// workgroup writes NaN to contact_sum and to the row's gradient.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GTTT_MAX_N = DVQ_GRASP_TTT_MAX_N;             // one word per point: 64 KB at the limit
constexpr int GTTT_SLOTS = GRASP_THREADS * GRASP_P;         // 1024 vertices per walk of the gather phase
constexpr unsigned GTTT_NONE = 0xfffu;                      // a field that names no vertex (a vertex index is at most 2047)
static_assert(GRASP_MAX_V <= 2048 && GRASP_THREADS == 256, "a field is 12 bits: 8 of the owner thread, 3 of its slot, 0xfff = none");
static_assert(GTTT_MAX_N <= 65535, "the two counts share one integer");

// bytes after the six planes: the words, three reduction rows, the flag, the seventh plane (bytes)
__host__ __device__ constexpr size_t gttt_lds_bytes(int V, int N) {
    return grasp_lds_bytes(V, N + 3 * GRASP_THREADS + 4) + (size_t)grasp_vp(V);
}
static_assert(gttt_lds_bytes(GRASP_MAX_V, GTTT_MAX_N) <= 160 * 1024, "the largest case must fit a workgroup's LDS");

// amdgpu_waves_per_eu(6): the LDS of the model's shapes admits six workgroups per CU; the scan is asked to fit their registers.
__global__ __launch_bounds__(GRASP_THREADS) __attribute__((amdgpu_waves_per_eu(6))) void grasp_ttt_kernel(
    const float* __restrict__ hand, const int* __restrict__ faces, const int* __restrict__ vf_off, const int* __restrict__ vf_face, int V,
    const float* __restrict__ obj, long osb, long osp, long osc, int N, float thr, const int* __restrict__ target_of_vertex,
    const float* __restrict__ w_pen, const float* __restrict__ w_con, int mean_contact, float* __restrict__ penetration,
    float* __restrict__ contact_sum, int* __restrict__ n_interior, int* __restrict__ n_contact, float* __restrict__ grad_hand) {
    extern __shared__ __align__(16) float gt_lds[];
    float *hx, *hy, *hz, *nx, *ny, *nz;
    grasp_planes(gt_lds, V, hx, hy, hz, nx, ny, nz);
    const int VP = grasp_vp(V);
    unsigned* words = reinterpret_cast<unsigned*>(gt_lds + grasp_hand_floats(V));   // [N] one per point
    float* part = reinterpret_cast<float*>(words + N);           // [256] penetration
    float* csum = part + GRASP_THREADS;                          // [256] contact sum
    int* cnt = reinterpret_cast<int*>(csum + GRASP_THREADS);     // [256] n_interior << 16 | n_contact
    int* flag = cnt + GRASP_THREADS;                             // [2] (of 4): a coordinate of the hand, of the cloud is not finite
    unsigned* tw = reinterpret_cast<unsigned*>(flag + 4);        // [VP / 4] the seventh plane, four vertices' bytes per word
    unsigned char* tb = reinterpret_cast<unsigned char*>(tw);    // [VP]
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    if (t < 2) flag[t] = 0;
    for (int i = t; i < VP; i += GRASP_THREADS) tb[i] = (i < V && (target_of_vertex == nullptr || target_of_vertex[i] != 0)) ? 1 : 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, hx, hy, hz)) flag[0] = 1;
    dvq_lds_barrier();
    grasp_normals(faces, vf_off, vf_face, V, t, hx, hy, hz, nx, ny, nz);
    dvq_lds_barrier();
    const bool hand_odd = flag[0] != 0;
    const float* ob = obj + b * osb;
    float sum = 0.0f, sumc = 0.0f;
    int n_both = 0;
    for (long p0 = t; p0 < N; p0 += GRASP_THREADS * GRASP_P) {   // points p0 + k * 256: thread t's points, ascending
        float sx[GRASP_P], sy[GRASP_P], sz[GRASP_P], best[GRASP_P], bc[GRASP_P];
        int bi[GRASP_P], bic[GRASP_P];
        bool slow = hand_odd;
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const long p = p0 + k * GRASP_THREADS;
            const bool in = p < N;
            sx[k] = in ? ob[p * osp] : 0.f;
            sy[k] = in ? ob[p * osp + osc] : 0.f;
            sz[k] = in ? ob[p * osp + 2 * osc] : 0.f;
            slow |= !grasp_finite(sx[k], sy[k], sz[k]);
            bc[k] = INFINITY;
            bic[k] = -1;
        }
        if (!slow) {
            // grasp_walk4's two loops (every coordinate finite: no distance is NaN) with the target-restricted minimum beside them
#pragma unroll
            for (int k = 0; k < GRASP_P; ++k) {
                best[k] = INFINITY;
                bi[k] = 0;
            }
            const int V4 = V & ~3;
            for (int j = 0; j < V4; j += 4) {
                const f32x4 X = *reinterpret_cast<const f32x4*>(hx + j);
                const f32x4 Y = *reinterpret_cast<const f32x4*>(hy + j);
                const f32x4 Z = *reinterpret_cast<const f32x4*>(hz + j);
                const unsigned T = tw[j >> 2];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool target = (T >> (8 * u)) & 1u;
#pragma unroll
                    for (int k = 0; k < GRASP_P; ++k) {
                        const float dx = sx[k] - X[u], dy = sy[k] - Y[u], dz = sz[k] - Z[u];
                        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        const bool better = d < best[k];
                        best[k] = better ? d : best[k];
                        bi[k] = better ? j + u : bi[k];
                        const float da = target ? d : INFINITY;
                        const bool betterc = da < bc[k];
                        bc[k] = betterc ? da : bc[k];
                        bic[k] = betterc ? j + u : bic[k];
                    }
                }
            }
            for (int j = V4; j < V; ++j) {
                const bool target = tb[j] != 0;
#pragma unroll
                for (int k = 0; k < GRASP_P; ++k) {
                    const float dx = sx[k] - hx[j], dy = sy[k] - hy[j], dz = sz[k] - hz[j];
                    const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    const bool better = d < best[k];
                    best[k] = better ? d : best[k];
                    bi[k] = better ? j : bi[k];
                    const float da = target ? d : INFINITY;
                    const bool betterc = da < bc[k];
                    bc[k] = betterc ? da : bc[k];
                    bic[k] = betterc ? j : bic[k];
                }
            }
        } else {
            flag[1] = 1;                                         // the row has no contact sum and no gradient; its scores are grasp_scores'
            grasp_scan4(hx, hy, hz, V, true, sx, sy, sz, best, bi);
        }
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const long p = p0 + k * GRASP_THREADS;
            if (p < N) {
                const float d = best[k];
                const bool inside = grasp_inside(hx, hy, hz, nx, ny, nz, bi[k], sx[k], sy[k], sz[k]);
                const bool contact = d < thr;
                sum += grasp_pen_term(inside, d);
                n_both += (inside ? 1 << 16 : 0) + (contact ? 1 : 0);
                if (!slow && bic[k] < 0) {                       // every target at +inf: the lowest target, if there is one
                    for (int j = 0; j < V; ++j) {
                        if (tb[j] != 0) {
                            bic[k] = j;
                            break;
                        }
                    }
                }
                sumc += contact ? bc[k] : 0.0f;
                const unsigned fp = (inside && !slow) ? (unsigned)bi[k] : GTTT_NONE;
                const unsigned fc = (contact && bic[k] >= 0) ? (unsigned)bic[k] : GTTT_NONE;
                words[p] = fp | (fc << 12);
            }
        }
    }
    part[t] = sum;
    csum[t] = sumc;
    cnt[t] = n_both;
    dvq_lds_barrier();
    for (int s = GRASP_THREADS / 2; s >= 1; s >>= 1) {           // the canonical tree: part[t] += part[t + s] for t < s
        if (t < s) {
            part[t] += part[t + s];
            csum[t] += csum[t + s];
            cnt[t] += cnt[t + s];
        }
        dvq_lds_barrier();
    }
    const bool odd = (flag[0] | flag[1]) != 0;                   // final: every write to it lies before the tree's barriers
    const int n_ct = cnt[0] & 0xffff;
    if (t == 0) {
        penetration[b] = part[0];
        contact_sum[b] = odd ? NAN : csum[0];
        n_interior[b] = cnt[0] >> 16;
        n_contact[b] = n_ct;
    }
    if (grad_hand == nullptr) return;
    float* gb = grad_hand + b * V * 3;
    if (odd) {
        for (int i = t; i < 3 * V; i += GRASP_THREADS) gb[i] = NAN;
        return;
    }
    const float a = 2.0f * (w_pen != nullptr ? w_pen[b] : 1.0f);
    const float c2 = 2.0f * (w_con != nullptr ? w_con[b] : 1.0f);
    const float c = mean_contact != 0 ? c2 / (float)(n_ct > 1 ? n_ct : 1) : c2;
    const unsigned ut = (unsigned)t;
    for (int v0 = 0; v0 < V; v0 += GTTT_SLOTS) {                 // the vertices v0 + t + 256 k: one walk over the words
        const unsigned walk = (unsigned)(v0 / GTTT_SLOTS);
        float gp[GRASP_P][3], gc[GRASP_P][3];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                gp[k][e] = 0.0f;
                gc[k][e] = 0.0f;
            }
        }
        for (int p = 0; p < N; ++p) {
            const unsigned w = words[p];                         // wave-uniform address: a broadcast
            const unsigned fp = w & 0xfffu, fc = w >> 12;
            const bool hp = (fp & 255u) == ut && (fp >> 10) == walk;   // 0xfff: slot 15, walk 3 -- no thread's
            const bool hc = (fc & 255u) == ut && (fc >> 10) == walk;
            if (hp || hc) {
                const float ox = ob[p * osp], oy = ob[p * osp + osc], oz = ob[p * osp + 2 * osc];
                if (hp) {
                    const float ex = hx[fp] - ox, ey = hy[fp] - oy, ez = hz[fp] - oz;
                    const unsigned slot = (fp >> 8) & 3u;
#pragma unroll
                    for (int k = 0; k < GRASP_P; ++k) {
                        if (slot == (unsigned)k) {
                            gp[k][0] += ex;
                            gp[k][1] += ey;
                            gp[k][2] += ez;
                        }
                    }
                }
                if (hc) {
                    const float ex = hx[fc] - ox, ey = hy[fc] - oy, ez = hz[fc] - oz;
                    const unsigned slot = (fc >> 8) & 3u;
#pragma unroll
                    for (int k = 0; k < GRASP_P; ++k) {
                        if (slot == (unsigned)k) {
                            gc[k][0] += ex;
                            gc[k][1] += ey;
                            gc[k][2] += ez;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int v = v0 + t + k * GRASP_THREADS;
            if (v < V) {
#pragma unroll
                for (int e = 0; e < 3; ++e) gb[3 * v + e] = fmaf(c, gc[k][e], a * gp[k][e]);
            }
        }
    }
}

}  // namespace

extern "C" int dvq_grasp_ttt(const float* hand, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                             const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride, int64_t B,
                             int N, float contact_threshold, const int32_t* target_of_vertex, const float* w_pen, const float* w_con,
                             int mean_contact, float* penetration, float* contact_sum, int32_t* n_interior, int32_t* n_contact,
                             float* grad_hand, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && N <= GTTT_MAX_N && V >= 1 && V <= GRASP_MAX_V,
                "grasp_ttt: need B >= 0, 1 <= N <= %d, 1 <= V <= %d (got B=%ld N=%d V=%d)", GTTT_MAX_N, GRASP_MAX_V, (long)B, N, V);
    DVQ_REQUIRE(mean_contact == 0 || mean_contact == 1, "grasp_ttt: mean_contact must be 0 or 1 (got %d)", mean_contact);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && faces && vf_off && vf_face && obj && penetration && contact_sum && n_interior && n_contact,
                "grasp_ttt: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = gttt_lds_bytes(V, N);
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_ttt_kernel), gttt_lds_bytes(GRASP_MAX_V, GTTT_MAX_N),
                                "grasp_ttt"));
    const double walks = grad_hand != nullptr ? (double)((V + GTTT_SLOTS - 1) / GTTT_SLOTS) : 0.0;
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // per (point, vertex) pair the 8 FLOPs of grasp_scores (the second minimum is compares and selects); in: the hand, the cloud
        // and the topology once per grasp (the cloud's hit points a second time, from cache); out: 16 B and the gradient per grasp
        DVQ_PROF("grasp_ttt", 8.0 * nb * N * V, (double)nb * ((double)(V + N) * 12 + 16 + walks * 12.0 * V), st);
        DVQ_LAUNCH(grasp_ttt_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), lds, st, hand + b0 * V * 3, faces, vf_off, vf_face, V,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, target_of_vertex, w_pen ? w_pen + b0 : nullptr, w_con ? w_con + b0 : nullptr, mean_contact,
                   penetration + b0, contact_sum + b0, n_interior + b0, n_contact + b0, grad_hand ? grad_hand + b0 * V * 3 : nullptr);
    });
    DVQ_CHECK_LAUNCH("grasp_ttt");
    return DVQ_OK;
}
