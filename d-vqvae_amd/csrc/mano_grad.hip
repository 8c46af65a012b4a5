// Backward pass of the MANO layer (mano.hip): the vector-Jacobian product from grad_verts / grad_joints to the gradients of betas,
// the PCA pose, global_orient and transl.  The forward state is RECOMPUTED, not saved: X, A and V of a chunk come from the forward's
// own pose kernel and blendshape GEMM (dvq_mano_chunk_state), so a call that needs no gradient keeps nothing alive.
// Three more launches per chunk of samples:
//   mano_skin_bwd_kernel  one workgroup per sample, grad_verts and V through LDS:
//                         dV[b][v] = T_r^T g[b][v] (T = sum_j w[v][j] A[b][j]) -> dV [B,2336], columns 2334 and 2335 written as zero;
//                         dA[b][j][i][c] = sum_v w[v][j] g[v][i] [V[v];1][c] and sum_v g[v]: one thread per output element, v = 0..777
//                         in order with a compensated (Kahan) accumulator -- no reduction tree, no atomics, one summation order
//   GEMM                  dX[B,160] = dV[B,2336] . blend_wt^T (blend_wt [160][2336]: blend_w transposed, zero-padded; no weight image:
//                         the operands are split on the fly into the exact bf16 pieces, or run as fp32 with DVQ_GEMM=fp32)
//   mano_pose_bwd_kernel  one wave per sample: backward of A = G with the rest joint removed, the kinematic chain in reverse, the pose
//                         feature, Rodrigues (1 - cos a taken as 2 sin^2(a/2)), the PCA basis and the joint regressor
// With grad_verts null (grad_joints alone) only the last kernel runs.
#include "dvq_internal.h"

namespace {

constexpr int NV = 778, NJ = 16, NB = 10, NP = 45;      // as in mano.hip
constexpr int XK = 160;                    // row stride of X and dX
constexpr int VLD = 2336;                  // row stride of V and dV: 2334 padded to 73 * 32, the GEMM's reduction length
constexpr long CHUNK = 16384;              // samples per pass, the forward's (scratch: 21.5 KB per sample)
constexpr int WPB = 4;                     // waves (samples) per pose block

// s += x with the rounding error of every addition carried in c (Kahan): the 778-term vertex sums come out within an ulp or two of
// their exact value whatever their partial sums do, in one fixed order
__device__ __forceinline__ void kahan_add(float& s, float& c, float x) {
    const float y = x - c;
    const float t = s + y;
    c = (t - s) - y;
    s = t;
}

__global__ __launch_bounds__(256) void mano_skin_bwd_kernel(const float* __restrict__ weights, const float* __restrict__ V,
                                                            const float* __restrict__ A, const float* __restrict__ gverts, int layout,
                                                            float* __restrict__ dV, float* __restrict__ dA, float* __restrict__ gsum) {
    __shared__ float s_g[NV * 3];          // the sample's upstream gradient, [v][3] whatever the layout
    __shared__ float s_V[NV * 3];
    __shared__ float s_A[NJ][12];
    const long b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* gp = gverts + b * (NV * 3);
    for (int e = tid; e < NV * 3; e += 256) {
        const float g = gp[e];
        if (layout == 0) s_g[e] = g;
        else s_g[3 * (e % NV) + e / NV] = g;            // [3][778] -> [778][3]
        s_V[e] = V[b * VLD + e];
    }
    if (tid < NJ * 12) s_A[tid / 12][tid % 12] = A[b * (NJ * 12) + tid];
    dvq_lds_barrier();
    // dV[v] = T_r^T g[v]
    for (int v = tid; v < NV; v += 256) {
        float T[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) T[i] = 0.f;
        for (int j = 0; j < NJ; ++j) {
            const float wj = weights[v * NJ + j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) T[i * 3 + c] = fmaf(wj, s_A[j][i * 4 + c], T[i * 3 + c]);
        }
        const float gx = s_g[3 * v], gy = s_g[3 * v + 1], gz = s_g[3 * v + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) dV[b * VLD + 3 * v + c] = T[c] * gx + T[3 + c] * gy + T[6 + c] * gz;
    }
    if (tid < VLD - NV * 3) dV[b * VLD + NV * 3 + tid] = 0.f;   // the pad columns meet zero weights: garbage there would turn into NaN
    // dA[j][i][c] = sum_v w[v][j] g[v][i] [V[v];1][c]  (192 sums), sum_v g[v][i]  (3 sums)
    if (tid < NJ * 12) {
        const int j = tid / 12, i = (tid % 12) / 4, c = tid % 4;
        const int cc = c < 3 ? c : 2;        // column 3 of [V;1] is the constant 1: the load is made anyway and its value replaced, no branch
        float s = 0.f, k = 0.f;
        // the weights come from L2: WU loads are issued ahead of the WU additions that consume them (one load per addition, waited for
        // in turn, made this loop 3.3 ms per 16 384 samples); the order of the additions is v = 0 .. 777 either way
        constexpr int WU = 16;
        int v = 0;
        for (; v + WU <= NV; v += WU) {
            float wv[WU];
#pragma unroll
            for (int u = 0; u < WU; ++u) wv[u] = weights[(v + u) * NJ + j];
#pragma unroll
            for (int u = 0; u < WU; ++u) {
                const float wg = wv[u] * s_g[3 * (v + u) + i];
                kahan_add(s, k, wg * (c < 3 ? s_V[3 * (v + u) + cc] : 1.0f));
            }
        }
        for (; v < NV; ++v) {
            const float wg = weights[v * NJ + j] * s_g[3 * v + i];
            kahan_add(s, k, wg * (c < 3 ? s_V[3 * v + cc] : 1.0f));
        }
        dA[b * (NJ * 12) + tid] = s;
    } else if (tid < NJ * 12 + 3) {
        const int i = tid - NJ * 12;
        float s = 0.f, k = 0.f;
        for (int v = 0; v < NV; ++v) kahan_add(s, k, s_g[3 * v + i]);
        gsum[b * 4 + i] = s;
    }
}

// One wave per sample.  Recomputes full_pose, the rest joints, R and the chain (mano_pose_kernel's steps, 1 - cos a in the stable form),
// then walks them backwards.  dA / dX / gsum are null when there is no grad_verts, gjoints is null when there is no grad_joints.
__global__ __launch_bounds__(64 * WPB) void mano_pose_bwd_kernel(dvq_mano_model m, const float* __restrict__ betas, long ldb,
                                                                const float* __restrict__ pose, long ldp,
                                                                const float* __restrict__ gorient, long ldg, long B,
                                                                const float* __restrict__ dA, const float* __restrict__ dX,
                                                                const float* __restrict__ gsum, const float* __restrict__ gjoints,
                                                                float* __restrict__ gbetas, float* __restrict__ gpose,
                                                                float* __restrict__ ggo, float* __restrict__ gtr) {
    __shared__ float s_beta[WPB][NB];
    __shared__ float s_pose[WPB][NP];
    __shared__ float s_full[WPB][48];
    __shared__ float s_R[WPB][NJ][9];
    __shared__ float s_J[WPB][NJ][3];
    __shared__ float s_G[WPB][NJ][12];    // world transforms, rows of [R | t]
    __shared__ float s_D[WPB][NJ][12];    // dA on entry, then the gradient of G: rows of [dGr | dGt]
    __shared__ float s_gj[WPB][48];
    __shared__ float s_dR[WPB][NJ][9];
    __shared__ float s_dJ[WPB][48];
    __shared__ float s_dfull[WPB][48];
    const int w = threadIdx.x >> 6, t = threadIdx.x & 63;
    const long b = (long)blockIdx.x * WPB + w;
    const bool live = b < B;
    const long bb = live ? b : B - 1;
    if (t < NB) s_beta[w][t] = betas[bb * ldb + t];
    if (t < NP) s_pose[w][t] = pose[bb * ldp + t];
    for (int u = t; u < NJ * 12; u += 64) s_D[w][u / 12][u % 12] = dA ? dA[bb * (NJ * 12) + u] : 0.f;
    if (t < 48) s_gj[w][t] = gjoints ? gjoints[bb * 48 + t] : 0.f;
    dvq_lds_barrier();
    if (t < 48) {
        float v;
        if (t < 3) {
            v = gorient ? gorient[bb * ldg + t] : 0.f;
        } else {
            v = 0.f;
            for (int i = 0; i < NP; ++i) v = fmaf(s_pose[w][i], m.comps[i * NP + (t - 3)], v);
        }
        s_full[w][t] = v + m.pose_mean[t];
        float j = m.j_template[t];
        for (int l = 0; l < NB; ++l) j = fmaf(s_beta[w][l], m.j_shapedirs[l * 48 + t], j);
        s_J[w][t / 3][t % 3] = j;
    }
    dvq_lds_barrier();
    // Rodrigues of joint t (lanes 0..15); angle, axis, sin and 2 sin^2(a/2) stay in registers for the backward step below
    float ex = 0.f, ey = 0.f, ez = 0.f, angle = 1.f, ax = 0.f, ay = 0.f, az = 0.f, sn = 0.f, c1 = 0.f;
    float K[9], K2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) K[i] = K2[i] = 0.f;
    if (t < NJ) {
        const float rx = s_full[w][3 * t], ry = s_full[w][3 * t + 1], rz = s_full[w][3 * t + 2];
        ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
        angle = sqrtf(ex * ex + ey * ey + ez * ez);
        ax = rx / angle, ay = ry / angle, az = rz / angle;
        sn = sinf(angle);
        const float sh = sinf(0.5f * angle);
        c1 = 2.0f * sh * sh;
        K[1] = -az, K[2] = ay, K[3] = az, K[5] = -ax, K[6] = -ay, K[7] = ax;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) K2[i * 3 + j] = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
#pragma unroll
        for (int i = 0; i < 9; ++i) s_R[w][t][i] = ((i % 4 == 0) ? 1.0f : 0.0f) + sn * K[i] + c1 * K2[i];
    }
    dvq_lds_barrier();
    if (t == 0) {
        // the chain forwards, as in mano_pose_kernel
#pragma clang loop vectorize(disable)
        for (int j = 0; j < NJ; ++j) {
            const int p = m.parents[j];
            float rel[3];
            for (int i = 0; i < 3; ++i) rel[i] = s_J[w][j][i] - (p >= 0 ? s_J[w][p][i] : 0.f);
            if (p < 0) {
                for (int i = 0; i < 3; ++i) {
                    for (int c = 0; c < 3; ++c) s_G[w][j][i * 4 + c] = s_R[w][j][i * 3 + c];
                    s_G[w][j][i * 4 + 3] = rel[i];
                }
            } else {
                for (int i = 0; i < 3; ++i) {
                    for (int c = 0; c < 3; ++c)
                        s_G[w][j][i * 4 + c] = s_G[w][p][i * 4] * s_R[w][j][c] + s_G[w][p][i * 4 + 1] * s_R[w][j][3 + c] +
                                               s_G[w][p][i * 4 + 2] * s_R[w][j][6 + c];
                    s_G[w][j][i * 4 + 3] = s_G[w][p][i * 4] * rel[0] + s_G[w][p][i * 4 + 1] * rel[1] + s_G[w][p][i * 4 + 2] * rel[2] +
                                           s_G[w][p][i * 4 + 3];
                }
            }
        }
        // (no loop vectorisation here: the joints of this loop are independent, and two of them at a time come out as packed-fp32
        // instructions, which the tree keeps out of every kernel but the GEMM epilogues)
        // A_j = [Gr_j | Gt_j - Gr_j J_j]:  dGr_j = dAr_j - dAt_j (x) J_j,  dJ_j = -Gr_j^T dAt_j,  dGt_j = dAt_j + grad_joints_j
#pragma clang loop vectorize(disable)
        for (int j = 0; j < NJ; ++j) {
            float at[3];
            for (int i = 0; i < 3; ++i) at[i] = s_D[w][j][i * 4 + 3];
            for (int i = 0; i < 3; ++i)
                for (int c = 0; c < 3; ++c) s_D[w][j][i * 4 + c] = s_D[w][j][i * 4 + c] - at[i] * s_J[w][j][c];
            for (int c = 0; c < 3; ++c)
                s_dJ[w][3 * j + c] = -(s_G[w][j][c] * at[0] + s_G[w][j][4 + c] * at[1] + s_G[w][j][8 + c] * at[2]);
            for (int i = 0; i < 3; ++i) s_D[w][j][i * 4 + 3] = at[i] + s_gj[w][3 * j + i];
        }
        // the chain backwards: a joint's children have larger indices, so D[j] is complete when j is reached
#pragma clang loop vectorize(disable)
        for (int j = NJ - 1; j >= 0; --j) {
            const int p = m.parents[j];
            if (p < 0) {
                for (int i = 0; i < 3; ++i) {
                    for (int c = 0; c < 3; ++c) s_dR[w][j][i * 3 + c] = s_D[w][j][i * 4 + c];
                    s_dJ[w][3 * j + i] = s_dJ[w][3 * j + i] + s_D[w][j][i * 4 + 3];
                }
                continue;
            }
            float rel[3], dt[3];
            for (int i = 0; i < 3; ++i) {
                rel[i] = s_J[w][j][i] - s_J[w][p][i];
                dt[i] = s_D[w][j][i * 4 + 3];
            }
            // Gr_j = Gr_p R_j:  dR_j = Gr_p^T dGr_j
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c)
                    s_dR[w][j][k * 3 + c] = s_G[w][p][k] * s_D[w][j][c] + s_G[w][p][4 + k] * s_D[w][j][4 + c] + s_G[w][p][8 + k] * s_D[w][j][8 + c];
            // dGr_p += dGr_j R_j^T + dGt_j (x) (J_j - J_p),  dGt_p += dGt_j
            for (int i = 0; i < 3; ++i) {
                for (int k = 0; k < 3; ++k)
                    s_D[w][p][i * 4 + k] = s_D[w][p][i * 4 + k] + (s_D[w][j][i * 4] * s_R[w][j][k * 3] + s_D[w][j][i * 4 + 1] * s_R[w][j][k * 3 + 1] +
                                                                   s_D[w][j][i * 4 + 2] * s_R[w][j][k * 3 + 2]) + dt[i] * rel[k];
                s_D[w][p][i * 4 + 3] = s_D[w][p][i * 4 + 3] + dt[i];
            }
            // Gt_j = Gr_p (J_j - J_p) + Gt_p:  d(J_j - J_p) = Gr_p^T dGt_j
            for (int k = 0; k < 3; ++k) {
                const float dr = s_G[w][p][k] * dt[0] + s_G[w][p][4 + k] * dt[1] + s_G[w][p][8 + k] * dt[2];
                s_dJ[w][3 * j + k] = s_dJ[w][3 * j + k] + dr;
                s_dJ[w][3 * p + k] = s_dJ[w][3 * p + k] - dr;
            }
        }
    }
    dvq_lds_barrier();
    if (t < NJ) {
        // dR of joint t: the chain's, plus the pose feature's share (joints 1..15)
        float dR[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) dR[i] = s_dR[w][t][i] + ((dX && t >= 1) ? dX[bb * XK + NB + 9 * (t - 1) + i] : 0.f);
        // R = I + s K + c1 K^2
        float ds = 0.f, dc = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            ds = ds + dR[i] * K[i];
            dc = dc + dR[i] * K2[i];
        }
        float dK[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float a1 = dR[i * 3] * K[j * 3] + dR[i * 3 + 1] * K[j * 3 + 1] + dR[i * 3 + 2] * K[j * 3 + 2];   // dR K^T
                const float a2 = K[i] * dR[j] + K[3 + i] * dR[3 + j] + K[6 + i] * dR[6 + j];                           // K^T dR
                dK[i * 3 + j] = sn * dR[i * 3 + j] + c1 * (a1 + a2);
            }
        const float dax = dK[7] - dK[5], day = dK[2] - dK[6], daz = dK[3] - dK[1];
        // d(sin a) = cos a, d(2 sin^2(a/2)) = sin a;  axis = r / a;  a = ||r + 1e-8||
        const float da = ds * cosf(angle) + dc * sn - (dax * ax + day * ay + daz * az) / angle;
        s_dfull[w][3 * t] = dax / angle + da * (ex / angle);
        s_dfull[w][3 * t + 1] = day / angle + da * (ey / angle);
        s_dfull[w][3 * t + 2] = daz / angle + da * (ez / angle);
    }
    dvq_lds_barrier();
    if (!live) return;
    if (ggo && t < 3) ggo[b * 3 + t] = s_dfull[w][t];
    if (gpose && t < NP) {      // full_pose[3:] = pose . comps + mean
        float v = 0.f;
        for (int i = 0; i < NP; ++i) v = fmaf(m.comps[t * NP + i], s_dfull[w][3 + i], v);
        gpose[b * NP + t] = v;
    }
    if (gbetas && t < NB) {     // betas reach the vertices through X[0:10] and the rest joints
        float v = 0.f;
        for (int i = 0; i < 48; ++i) v = fmaf(m.j_shapedirs[t * 48 + i], s_dJ[w][i], v);
        gbetas[b * NB + t] = (dX ? dX[b * XK + t] : 0.f) + v;
    }
    if (gtr && t < 3) {         // transl is added to every vertex and every joint
        float v = 0.f;
        for (int j = 0; j < NJ; ++j) v = v + s_gj[w][3 * j + t];
        gtr[b * 3 + t] = (gsum ? gsum[b * 4 + t] : 0.f) + v;
    }
}

struct Scratch {
    float *X, *V, *A, *dV, *dA, *dX, *gsum;
    size_t bytes;
};

// the arrays of a pass of c samples inside the workspace (base may be null: only `bytes` is read then)
Scratch carve(void* base, long c) {
    Scratch s;
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    const uintptr_t p0 = p;
    auto take = [&](size_t floats) {
        float* r = reinterpret_cast<float*>(p);
        p += dvq_round_up(floats * 4, 256);
        return r;
    };
    s.X = take((size_t)c * XK);
    s.V = take((size_t)c * VLD);
    s.A = take((size_t)c * NJ * 12);
    s.dV = take((size_t)c * VLD);
    s.dA = take((size_t)c * NJ * 12);
    s.dX = take((size_t)c * XK);
    s.gsum = take((size_t)c * 4);
    s.bytes = (size_t)(p - p0);
    return s;
}

}  // namespace

extern "C" size_t dvq_mano_backward_workspace_bytes(int64_t B) {
    return carve(nullptr, B < CHUNK ? (B > 0 ? B : 1) : CHUNK).bytes;
}

extern "C" int dvq_mano_backward(const dvq_mano_model* m, const float* blend_wt, const float* betas, int64_t ldb, const float* pose,
                                 int64_t ldp, const float* global_orient, int64_t ldg, const float* transl, int64_t ldt, int64_t B,
                                 const float* grad_verts, int layout, const float* grad_joints, float* grad_betas, float* grad_pose,
                                 float* grad_global_orient, float* grad_transl, void* workspace, size_t workspace_bytes,
                                 dvq_stream_t stream) {
    DVQ_REQUIRE(m && blend_wt && betas && pose, "mano_backward: null pointer");
    DVQ_REQUIRE(m->v_template && m->blend_w && m->j_template && m->j_shapedirs && m->weights && m->comps && m->pose_mean,
                "mano_backward: incomplete model");
    DVQ_REQUIRE(grad_verts || grad_joints, "mano_backward: grad_verts and grad_joints are both null");
    DVQ_REQUIRE(layout == 0 || layout == 1, "mano_backward: layout must be 0 ([B,778,3]) or 1 ([B,3,778])");
    DVQ_REQUIRE(B >= 0 && ldb >= 10 && ldp >= 45 && (!global_orient || ldg >= 3) && (!transl || ldt >= 3), "mano_backward: bad strides");
    for (int j = 0; j < 16; ++j) DVQ_REQUIRE(m->parents[j] < j, "mano_backward: parents[%d]=%d is not an ancestor index", j, m->parents[j]);
    DVQ_REQUIRE(dvq_aligned16(blend_wt), "mano_backward: unaligned blend_wt");
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(workspace && dvq_aligned16(workspace), "mano_backward: null/unaligned workspace");
    if (workspace_bytes < dvq_mano_backward_workspace_bytes(B)) {
        dvq_set_error("mano_backward: workspace %zu < %zu bytes", workspace_bytes, dvq_mano_backward_workspace_bytes(B));
        return DVQ_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const Scratch s = carve(workspace, B < CHUNK ? B : CHUNK);
    for (long b0 = 0; b0 < B; b0 += CHUNK) {
        const long nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        const float* go = global_orient ? global_orient + b0 * ldg : nullptr;
        if (grad_verts) {
            // transl moves neither X, A nor V (the forward adds it while skinning): the recomputation leaves it out
            DVQ_PROPAGATE(dvq_mano_chunk_state(m, betas + b0 * ldb, ldb, pose + b0 * ldp, ldp, go, ldg, nullptr, 0, nb, s.X, s.V, s.A, nullptr, st));
            {
                DVQ_PROF("mano_skin_bwd", (double)nb * NV * (NJ * 18 + 15 + 12 * NJ * 6), (double)nb * (NV * 3 * 2 + VLD + NJ * 24) * 4, st);
                DVQ_LAUNCH(mano_skin_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, st, m->weights, s.V, s.A, grad_verts + b0 * NV * 3, layout,
                           s.dV, s.dA, s.gsum);
            }
            DVQ_CHECK_LAUNCH("mano_skin_bwd");
            GemmParams g = {};
            g.src[0] = GemmSrc{s.dV, blend_wt, VLD, VLD, VLD, DVQ_PLANES_BF16X3, nullptr, 0, nullptr};
            g.nsrc = 1;
            g.M = nb;
            g.N = XK;
            g.out = s.dX;
            g.ldo = XK;
            DVQ_PROPAGATE(dvq_launch_gemm(g, EPI_BIAS, st));
        }
        {
            DVQ_PROF("mano_pose_bwd", (double)nb * 4.0e4, (double)nb * (55 + XK + NJ * 12 + 48 + 61) * 4, st);
            DVQ_LAUNCH(mano_pose_bwd_kernel, dim3((unsigned)((nb + WPB - 1) / WPB)), dim3(64 * WPB), 0, st, *m, betas + b0 * ldb, (long)ldb,
                       pose + b0 * ldp, (long)ldp, go, (long)ldg, nb, grad_verts ? s.dA : nullptr, grad_verts ? s.dX : nullptr,
                       grad_verts ? s.gsum : nullptr, grad_joints ? grad_joints + b0 * 48 : nullptr,
                       grad_betas ? grad_betas + b0 * NB : nullptr, grad_pose ? grad_pose + b0 * NP : nullptr,
                       grad_global_orient ? grad_global_orient + b0 * 3 : nullptr, grad_transl ? grad_transl + b0 * 3 : nullptr);
        }
        DVQ_CHECK_LAUNCH("mano_pose_bwd");
    }
    return DVQ_OK;
}
