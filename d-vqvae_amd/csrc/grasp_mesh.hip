// dvq_grasp_mesh: the hand vertices inside the object's closed triangle mesh (parity along +z) and, of those, the largest distance to
// the surface, in ONE kernel, one workgroup of 256 threads per grasp.  The definition is the ABI (include/dvq.h); this file only says
// how the kernel is laid out.  The result is a parity, minima and one maximum: nothing below has to keep an order.
//
// As in grasp_parts.hip every thread holds four hand vertices (slots t + 256 k) in registers, in the object's frame, and the FACES go
// through LDS in tiles of GM_TILE = 256, one face per thread and tile, gathered once from mesh_verts through the face indices:
//   pass 1  (every vertex against every face: the parity)  a face is five 16-byte words that all vertices share -- the xy bounds, the
//           three edges in canonical direction (start point, difference), the three heights and a word of bits (which edges the face
//           traverses backwards, which side an edge value of 0 counts for, which side belongs to the face).  Every lane reads the
//           same face: broadcast reads.  The bounds word alone rejects most (vertex, face) pairs.
//   pass 2  (only when the pass has inside vertices: the distances)  the inside slots are compacted with ballots into a list; the
//           workgroup is split into G groups of S = 256 / G threads, G = the list's length rounded up to a power of two (at most
//           256): thread j of group g takes vertices g, g + G, ... of the list (at most four) and the faces j, j + S, ... of every
//           tile, so a row with ONE inside vertex still has 256 threads on it.  The tile is nine planes (a, b, c as x|y|z of all
//           faces: neighbouring lanes read neighbouring words).  A thread's best (dist2, face) over its slices goes into the slot's
//           64-bit key in LDS with one integer atomic minimum -- dist2's bits above the face index: non-negative floats order as
//           integers, so the key's minimum is the smallest dist2 and among equals the lowest face.
// The row's deepest vertex is a 64-bit atomic maximum of (dist2's bits, ~vertex index) in the same way.  A hand of more than 1024
// vertices takes a second pass over both passes.  LDS: 20 KB tile + 12 KB slots + 8 KB keys + 4 KB list = 44 KB, three workgroups
// per CU.  No tile is skipped yet: a box per tile against the hand's (pass 1) or the running minima (pass 2) would change no bit.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GM_TILE = GRASP_THREADS;                      // faces per tile: one per thread (ops.GRASP_MESH_TILE)
constexpr int GM_SLOTS = GRASP_THREADS * GRASP_P;           // 1024 hand vertices per pass over the faces
constexpr int GM_MAX_FACES = DVQ_GRASP_MESH_MAX_FACES;      // per object
constexpr int GM_W1 = 20;                                   // words of a face in pass 1
constexpr int GM_W2 = 9;                                    // planes of the tile in pass 2
constexpr unsigned long long GM_NONE = 0x7f800000ffffffffull;   // (+inf, face -1): what a slot's key starts from
static_assert(GM_W2 <= GM_W1 && GM_TILE == GRASP_THREADS, "one tile buffer, one face per thread");
static_assert(GM_SLOTS % 64 == 0 && GRASP_MAX_V % 32 == 0, "a wave's ballot is two whole mask words");

// bits of a face's word in pass 1: edge i (1: a-b, 2: b-c, 3: c-a) is traversed backwards | its value 0 counts as positive | its
// positive side belongs to the face
constexpr int GM_REV = 0, GM_TIE = 3, GM_SIDE = 6;

__device__ __forceinline__ float gm_dot(float ux, float uy, float uz, float wx, float wy, float wz) {
    return fmaf(uz, wz, fmaf(uy, wy, ux * wx));
}

// step 3 of the definition: the squared distance of p to the closest point of the triangle (a, b, c)
__device__ __forceinline__ float gm_tri_d2(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz,
                                           float cx, float cy, float cz) {
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d1 = gm_dot(abx, aby, abz, apx, apy, apz), d2 = gm_dot(acx, acy, acz, apx, apy, apz);
    const float d3 = gm_dot(abx, aby, abz, bpx, bpy, bpz), d4 = gm_dot(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = gm_dot(abx, aby, abz, cpx, cpy, cpz), d6 = gm_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float u = d4 - d3, w = d5 - d6;
    float qx, qy, qz;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        qx = ax, qy = ay, qz = az;
    } else if (d3 >= 0.0f && d4 <= d3) {
        qx = bx, qy = by, qz = bz;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float s = d1 / (d1 - d3);
        qx = fmaf(s, abx, ax), qy = fmaf(s, aby, ay), qz = fmaf(s, abz, az);
    } else if (d6 >= 0.0f && d5 <= d6) {
        qx = cx, qy = cy, qz = cz;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float s = d2 / (d2 - d6);
        qx = fmaf(s, acx, ax), qy = fmaf(s, acy, ay), qz = fmaf(s, acz, az);
    } else if (va <= 0.0f && u >= 0.0f && w >= 0.0f) {
        const float s = u / (u + w);
        qx = fmaf(s, cx - bx, bx), qy = fmaf(s, cy - by, by), qz = fmaf(s, cz - bz, bz);
    } else {
        const float n = (va + vb) + vc;
        const float s = vb / n, r = vc / n;
        qx = fmaf(r, acx, fmaf(s, abx, ax)), qy = fmaf(r, acy, fmaf(s, aby, ay)), qz = fmaf(r, acz, fmaf(s, abz, az));
    }
    const float ex = px - qx, ey = py - qy, ez = pz - qz;
    return gm_dot(ex, ey, ez, ex, ey, ez);
}

__global__ __launch_bounds__(GRASP_THREADS) void grasp_mesh_kernel(const float* __restrict__ hand, int V, const float* __restrict__ mverts,
                                                                   int n_mv, const int* __restrict__ vert_off,
                                                                   const int* __restrict__ mfaces, int n_mf,
                                                                   const int* __restrict__ face_off, long O,
                                                                   const int64_t* __restrict__ obj_of_row, const float* __restrict__ R,
                                                                   const float* __restrict__ tr, int* __restrict__ n_inside,
                                                                   float* __restrict__ depth, int* __restrict__ deep_vertex,
                                                                   int* __restrict__ deep_face, int* __restrict__ mask,
                                                                   int* __restrict__ status, float* __restrict__ vert_d2,
                                                                   int* __restrict__ vert_face, int* err_flag) {
    __shared__ __align__(16) float gm_tile[GM_TILE * GM_W1];     // pass 1: [face][20]; pass 2: [9][GM_TILE]
    __shared__ float gm_px[GM_SLOTS], gm_py[GM_SLOTS], gm_pz[GM_SLOTS];   // the pass's slots in the object's frame
    __shared__ unsigned long long gm_key[GM_SLOTS];              // per slot: dist2's bits << 32 | face
    __shared__ int gm_list[GM_SLOTS];                            // the inside slots, compacted
    __shared__ unsigned long long gm_row;                        // the row's deepest: dist2's bits << 32 | ~vertex; 0 = none
    __shared__ int gm_small[2 + 16];                             // 0: a coordinate is not finite, 1: deep_face, 2 ..: [k][wave] inside counts
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const float* hb = hand + b * V * 3;
    const int W = (V + 31) >> 5;
    const float nanf_ = __builtin_nanf("");

    // a row without vertices inside, or without a figure: everything but the status and the three scalars is the same fill
    auto fill = [&](int st, int n, float d, float vd) {
        if (t == 0) {
            n_inside[b] = n;
            depth[b] = d;
            deep_vertex[b] = -1;
            deep_face[b] = -1;
            status[b] = st;
        }
        for (int w = t; w < W; w += GRASP_THREADS) mask[b * W + w] = 0;
        for (int v = t; v < V; v += GRASP_THREADS) {
            if (vert_d2) vert_d2[b * V + v] = vd;
            if (vert_face) vert_face[b * V + v] = -1;
        }
    };

    const int64_t o = obj_of_row[b];
    int vbase = 0, nv = -1, fbase = 0, nf = -1;
    if (o >= 0 && o < O) {
        vbase = vert_off[o];
        nv = vert_off[o + 1] - vbase;
        fbase = face_off[o];
        nf = face_off[o + 1] - fbase;
    }
    if (nv < 0 || nf < 0 || nf > GM_MAX_FACES || vbase < 0 || vbase > n_mv - nv || fbase < 0 || fbase > n_mf - nf) {   // uniform
        if (t == 0) atomicOr(err_flag, (o >= 0 && o < O) ? 2 : 1);
        fill(4, -1, nanf_, nanf_);
        return;
    }
    if (t == 0) {
        gm_small[0] = 0;
        gm_small[1] = -1;
        gm_row = 0ull;
    }
    dvq_lds_barrier();
    {
        bool odd = false;                                        // the whole hand, up front: later passes' vertices included
        for (int i = t; i < 3 * V; i += GRASP_THREADS) odd |= !(fabsf(hb[i]) < INFINITY);
        if (odd) gm_small[0] = 1;
    }
    dvq_lds_barrier();
    if (gm_small[0]) {
        fill(3, -1, nanf_, nanf_);
        return;
    }
    if (nf == 0) {
        fill(1, 0, 0.0f, INFINITY);
        return;
    }
    const float* mv = mverts + (long)vbase * 3;
    const int* mf = mfaces + (long)fbase * 3;
    float r[9], tt[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = R ? R[b * 9 + i] : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) tt[i] = tr ? tr[i] : 0.0f;
    const f32x4* tile4 = reinterpret_cast<const f32x4*>(gm_tile);
    const int lane = t & 63, wave = t >> 6;
    int n_total = 0;

    for (int v0 = 0; v0 < V; v0 += GM_SLOTS) {                   // vertices v0 + t + 256 k: one pass over the faces, or two
        float x[GRASP_P], y[GRASP_P], z[GRASP_P];
        bool par[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int slot = t + k * GRASP_THREADS, v = v0 + slot;
            const bool in = v < V;
            float hx = in ? hb[3 * v] : 0.f, hy = in ? hb[3 * v + 1] : 0.f, hz = in ? hb[3 * v + 2] : 0.f;
            if (R) {                                             // step 2 of dvq_grasp_volume
                const float u0 = tr ? hx - tt[0] : hx, u1 = tr ? hy - tt[1] : hy, u2 = tr ? hz - tt[2] : hz;
                hx = fmaf(r[6], u2, fmaf(r[3], u1, r[0] * u0));
                hy = fmaf(r[7], u2, fmaf(r[4], u1, r[1] * u0));
                hz = fmaf(r[8], u2, fmaf(r[5], u1, r[2] * u0));
            }
            x[k] = in ? hx : nanf_;                              // a slot without a vertex is in no face's bounds
            y[k] = hy;
            z[k] = hz;
            par[k] = false;
            gm_px[slot] = hx;
            gm_py[slot] = hy;
            gm_pz[slot] = hz;
            gm_key[slot] = GM_NONE;
        }
        // ---------------------------------------------------------------------------------------- pass 1: the parity
        for (int p0 = 0; p0 < nf; p0 += GM_TILE) {
            const int n = nf - p0 < GM_TILE ? nf - p0 : GM_TILE;
            dvq_lds_barrier();                                   // every wave is through with the tile before
            if (t < n) {
                const int f = p0 + t;
                const int a = mf[3 * f], bb = mf[3 * f + 1], c = mf[3 * f + 2];
                const bool ok = (unsigned)a < (unsigned)nv && (unsigned)bb < (unsigned)nv && (unsigned)c < (unsigned)nv;
                if (!ok && v0 == 0) atomicOr(err_flag, 2);
                const int ia = ok ? a : 0, ib = ok ? bb : 0, ic = ok ? c : 0;     // (nothing is read for a skipped face)
                const float ax = ok ? mv[3 * ia] : 0.f, ay = ok ? mv[3 * ia + 1] : 0.f, az = ok ? mv[3 * ia + 2] : 0.f;
                const float bx = ok ? mv[3 * ib] : 0.f, by = ok ? mv[3 * ib + 1] : 0.f, bz = ok ? mv[3 * ib + 2] : 0.f;
                const float cx = ok ? mv[3 * ic] : 0.f, cy = ok ? mv[3 * ic + 1] : 0.f, cz = ok ? mv[3 * ic + 2] : 0.f;
                const float A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
                const bool live = ok && (A > 0.0f || A < 0.0f);
                // the three edges in canonical direction: e1 of (a,b), e2 of (b,c), e3 of (c,a); rev: the face runs Q -> P
                const bool r1 = a > bb, r2 = bb > c, r3 = c > a;
                const float p1x = r1 ? bx : ax, p1y = r1 ? by : ay, d1x = r1 ? ax - bx : bx - ax, d1y = r1 ? ay - by : by - ay;
                const float p2x = r2 ? cx : bx, p2y = r2 ? cy : by, d2x = r2 ? bx - cx : cx - bx, d2y = r2 ? by - cy : cy - by;
                const float p3x = r3 ? ax : cx, p3y = r3 ? ay : cy, d3x = r3 ? cx - ax : ax - cx, d3y = r3 ? cy - ay : ay - cy;
                const bool up = A > 0.0f;
                const bool z1 = d1y < 0.0f || (d1y == 0.0f && d1x > 0.0f), z2 = d2y < 0.0f || (d2y == 0.0f && d2x > 0.0f),
                           z3 = d3y < 0.0f || (d3y == 0.0f && d3x > 0.0f);
                const int bits = (r1 ? 1 : 0) << GM_REV | (r2 ? 2 : 0) << GM_REV | (r3 ? 4 : 0) << GM_REV | (z1 ? 1 : 0) << GM_TIE |
                                 (z2 ? 2 : 0) << GM_TIE | (z3 ? 4 : 0) << GM_TIE | (up != r1 ? 1 : 0) << GM_SIDE |
                                 (up != r2 ? 2 : 0) << GM_SIDE | (up != r3 ? 4 : 0) << GM_SIDE;
                f32x4* w4 = reinterpret_cast<f32x4*>(gm_tile) + t * (GM_W1 / 4);
                f32x4 q;
                q[0] = live ? fminf(ax, fminf(bx, cx)) : INFINITY;   // a face that covers nothing: empty bounds
                q[1] = live ? fmaxf(ax, fmaxf(bx, cx)) : -INFINITY;
                q[2] = fminf(ay, fminf(by, cy));
                q[3] = fmaxf(ay, fmaxf(by, cy));
                w4[0] = q;
                q[0] = p1x, q[1] = p1y, q[2] = d1x, q[3] = d1y;
                w4[1] = q;
                q[0] = p2x, q[1] = p2y, q[2] = d2x, q[3] = d2y;
                w4[2] = q;
                q[0] = p3x, q[1] = p3y, q[2] = d3x, q[3] = d3y;
                w4[3] = q;
                q[0] = az, q[1] = bz, q[2] = cz, q[3] = __int_as_float(bits);
                w4[4] = q;
            }
            dvq_lds_barrier();
            for (int f = 0; f < n; ++f) {
                const f32x4 bd = tile4[f * (GM_W1 / 4)];
                bool in[GRASP_P], any = false;
#pragma unroll
                for (int k = 0; k < GRASP_P; ++k) {
                    in[k] = bd[0] <= x[k] && x[k] <= bd[1] && bd[2] <= y[k] && y[k] <= bd[3];
                    any |= in[k];
                }
                if (!any) continue;
                const f32x4 g1 = tile4[f * (GM_W1 / 4) + 1], g2 = tile4[f * (GM_W1 / 4) + 2], g3 = tile4[f * (GM_W1 / 4) + 3],
                            hz = tile4[f * (GM_W1 / 4) + 4];
                const int bits = __float_as_int(hz[3]);
                const bool r1 = (bits >> GM_REV) & 1, r2 = (bits >> GM_REV) & 2, r3 = (bits >> GM_REV) & 4;
                const bool z1 = (bits >> GM_TIE) & 1, z2 = (bits >> GM_TIE) & 2, z3 = (bits >> GM_TIE) & 4;
                const bool t1 = (bits >> GM_SIDE) & 1, t2 = (bits >> GM_SIDE) & 2, t3 = (bits >> GM_SIDE) & 4;
#pragma unroll
                for (int k = 0; k < GRASP_P; ++k) {
                    if (!in[k]) continue;
                    const float e1 = g1[2] * (y[k] - g1[1]) - g1[3] * (x[k] - g1[0]);
                    const float e2 = g2[2] * (y[k] - g2[1]) - g2[3] * (x[k] - g2[0]);
                    const float e3 = g3[2] * (y[k] - g3[1]) - g3[3] * (x[k] - g3[0]);
                    const bool s1 = e1 > 0.0f || (e1 == 0.0f && z1), s2 = e2 > 0.0f || (e2 == 0.0f && z2),
                               s3 = e3 > 0.0f || (e3 == 0.0f && z3);
                    if (s1 != t1 || s2 != t2 || s3 != t3) continue;
                    if (e1 != e1 || e2 != e2 || e3 != e3) continue;
                    const float wc = r1 ? -e1 : e1, wa = r2 ? -e2 : e2, wb = r3 ? -e3 : e3;
                    const float zc = ((wa * hz[0] + wb * hz[1]) + wc * hz[2]) / ((wa + wb) + wc);
                    par[k] ^= zc > z[k];
                }
            }
        }
        // ---------------------------------------------------------------------------------------- the mask, the compacted list
        unsigned long long bal[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            bal[k] = __ballot(par[k]);                           // the wave's 64 vertices: two mask words
            if (lane == 0) {
                const int w = (v0 + k * GRASP_THREADS + t) >> 5;
                if (w < W) mask[b * W + w] = (int)(unsigned)(bal[k] & 0xffffffffull);
                if (w + 1 < W) mask[b * W + w + 1] = (int)(unsigned)(bal[k] >> 32);
                gm_small[2 + k * 4 + wave] = __popcll(bal[k]);
            }
        }
        dvq_lds_barrier();                                       // (and every wave is through with pass 1's last tile)
        int n_in = 0;                                            // the list's order: k, then the wave, then the lane
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            int base = n_in;
#pragma unroll
            for (int w = 0; w < GRASP_THREADS / 64; ++w) {
                const int c = gm_small[2 + k * 4 + w];
                base += w < wave ? c : 0;
                n_in += c;
            }
            if (par[k]) gm_list[base + __popcll(bal[k] & ((1ull << lane) - 1ull))] = t + k * GRASP_THREADS;
        }
        n_total += n_in;
        // ---------------------------------------------------------------------------------------- pass 2: the distances
        if (n_in > 0) {                                          // uniform
            int G = 1;
            while (G < n_in && G < GRASP_THREADS) G <<= 1;
            const int S = GRASP_THREADS / G, g = t / S, j = t - g * S;
            dvq_lds_barrier();                                   // the list is complete
            float qx[GRASP_P], qy[GRASP_P], qz[GRASP_P], best[GRASP_P];
            int bf[GRASP_P], slot[GRASP_P];
            bool mine[GRASP_P];
#pragma unroll
            for (int k = 0; k < GRASP_P; ++k) {
                const int i = g + k * G;
                mine[k] = i < n_in;
                slot[k] = mine[k] ? gm_list[i] : 0;
                qx[k] = gm_px[slot[k]];
                qy[k] = gm_py[slot[k]];
                qz[k] = gm_pz[slot[k]];
                best[k] = INFINITY;
                bf[k] = -1;
            }
            for (int p0 = 0; p0 < nf; p0 += GM_TILE) {
                const int n = nf - p0 < GM_TILE ? nf - p0 : GM_TILE;
                dvq_lds_barrier();                               // every wave is through with the tile before
                if (t < n) {
                    const int f = p0 + t;
                    const int a = mf[3 * f], bb = mf[3 * f + 1], c = mf[3 * f + 2];
                    const bool ok = (unsigned)a < (unsigned)nv && (unsigned)bb < (unsigned)nv && (unsigned)c < (unsigned)nv;
                    const int ia = ok ? a : 0, ib = ok ? bb : 0, ic = ok ? c : 0;
#pragma unroll
                    for (int c3 = 0; c3 < 3; ++c3) {             // a skipped face is all NaN: never nearest
                        gm_tile[c3 * GM_TILE + t] = ok ? mv[3 * ia + c3] : nanf_;
                        gm_tile[(3 + c3) * GM_TILE + t] = ok ? mv[3 * ib + c3] : nanf_;
                        gm_tile[(6 + c3) * GM_TILE + t] = ok ? mv[3 * ic + c3] : nanf_;
                    }
                }
                dvq_lds_barrier();
                for (int f = j; f < n; f += S) {
                    const float ax = gm_tile[f], ay = gm_tile[GM_TILE + f], az = gm_tile[2 * GM_TILE + f];
                    const float bx = gm_tile[3 * GM_TILE + f], by = gm_tile[4 * GM_TILE + f], bz = gm_tile[5 * GM_TILE + f];
                    const float cx = gm_tile[6 * GM_TILE + f], cy = gm_tile[7 * GM_TILE + f], cz = gm_tile[8 * GM_TILE + f];
#pragma unroll
                    for (int k = 0; k < GRASP_P; ++k) {
                        if (!mine[k]) continue;
                        const float d = gm_tri_d2(qx[k], qy[k], qz[k], ax, ay, az, bx, by, bz, cx, cy, cz);
                        const bool better = d < best[k];         // strictly less, ascending faces: the lowest index of the slice
                        best[k] = better ? d : best[k];
                        bf[k] = better ? p0 + f : bf[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < GRASP_P; ++k) {
                if (mine[k] && bf[k] >= 0)
                    atomicMin(&gm_key[slot[k]], ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned)bf[k]);
            }
            dvq_lds_barrier();                                   // the keys are final
        }
        // ---------------------------------------------------------------------------------------- per vertex, and the row's deepest
        unsigned long long cand[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int slot = t + k * GRASP_THREADS, v = v0 + slot;
            const unsigned long long key = gm_key[slot];         // an outside slot's is untouched: +inf, -1
            if (v < V && vert_d2) vert_d2[b * V + v] = __uint_as_float((unsigned)(key >> 32));
            if (v < V && vert_face) vert_face[b * V + v] = (int)(unsigned)(key & 0xffffffffull);
            cand[k] = (key & 0xffffffff00000000ull) | (0xffffffffu - (unsigned)v);
            if (par[k]) atomicMax(&gm_row, cand[k]);
        }
        dvq_lds_barrier();
        {
            const unsigned long long top = gm_row;
#pragma unroll
            for (int k = 0; k < GRASP_P; ++k)
                if (par[k] && cand[k] == top) gm_small[1] = (int)(unsigned)(gm_key[t + k * GRASP_THREADS] & 0xffffffffull);
        }
    }
    dvq_lds_barrier();
    if (t == 0) {
        const unsigned long long top = gm_row;
        n_inside[b] = n_total;
        depth[b] = top ? sqrtf(__uint_as_float((unsigned)(top >> 32))) : 0.0f;
        deep_vertex[b] = top ? (int)(0xffffffffu - (unsigned)(top & 0xffffffffull)) : -1;
        deep_face[b] = top ? gm_small[1] : -1;
        status[b] = 0;
    }
}

}  // namespace

extern "C" int dvq_grasp_mesh(const float* hand, int V, const float* mesh_verts, int n_mv, const int32_t* vert_off,
                              const int32_t* mesh_faces, int n_mf, const int32_t* face_off, int64_t O, const int64_t* obj_of_row,
                              const float* R, const float* t, int64_t B, int32_t* n_inside, float* depth, int32_t* deep_vertex,
                              int32_t* deep_face, int32_t* inside_mask, int32_t* status, float* vert_d2, int32_t* vert_face,
                              int32_t* err_flag, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && V >= 1 && V <= GRASP_MAX_V && O >= 0 && n_mv >= 0 && n_mf >= 0,
                "grasp_mesh: need B >= 0, 1 <= V <= %d, O >= 0, n_mv >= 0, n_mf >= 0 (got B=%ld V=%d O=%ld n_mv=%d n_mf=%d)", GRASP_MAX_V,
                (long)B, V, (long)O, n_mv, n_mf);
    DVQ_REQUIRE(R || !t, "grasp_mesh: t without R");
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && (mesh_verts || n_mv == 0) && vert_off && (mesh_faces || n_mf == 0) && face_off && obj_of_row && n_inside && depth &&
                    deep_vertex && deep_face && inside_mask && status && err_flag,
                "grasp_mesh: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t W = (V + 31) / 32;
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // the work depends on the data (each row's face count lives on the device, pass 2 runs for inside vertices only): reported
        // as 0 FLOPs.  in: the hand twice (the check, the registers); out: the five scalars, the mask and, when asked for, 8 B per vertex
        DVQ_PROF("grasp_mesh", 0.0, (double)nb * (24.0 * V + 20 + 4.0 * W + (vert_d2 ? 4.0 * V : 0) + (vert_face ? 4.0 * V : 0)), st);
        DVQ_LAUNCH(grasp_mesh_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), 0, st, hand + b0 * V * 3, V, mesh_verts, n_mv, vert_off,
                   mesh_faces, n_mf, face_off, (long)O, obj_of_row + b0, R ? R + b0 * 9 : nullptr, t, n_inside + b0, depth + b0,
                   deep_vertex + b0, deep_face + b0, inside_mask + b0 * W, status + b0, vert_d2 ? vert_d2 + b0 * V : nullptr,
                   vert_face ? vert_face + b0 * V : nullptr, err_flag);
    });
    DVQ_CHECK_LAUNCH("grasp_mesh");
    return DVQ_OK;
}
