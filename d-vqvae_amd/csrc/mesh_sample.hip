// dvq_mesh_sample: area-weighted points on the surfaces of a call's triangle meshes; dvq_cloud_fps: farthest-point subsampling of a
// 3-D pool.  Both definitions are the ABI text of include/dvq.h; this file only says how the kernels are laid out.  Nothing below
// depends on O, on which objects share a call or on scheduling: the weights are integers (their prefix sum is exact in any order), a
// draw is a function of (seed, stream id, sample index), and the selection is a chain of maxima with the position as the tie-break.
//
// mesh_cdf_kernel     one workgroup of 1024 threads per object, the faces in chunks of 1024, one face per thread.  Pass A: the face's
//                     w (its float bits parked in the face's own cdf word, which the same thread reads back) and the object's largest
//                     w.  Pass B: q from w / amax, an inclusive scan of the chunk (six shuffles per wave, the 16 wave totals through
//                     LDS in two alternating rows: one barrier per chunk) on top of a running uint64 carry.
// mesh_points_kernel  one thread per (object, sample), 256 samples per workgroup: Philox, a binary search of the object's cdf (at most
//                     18 dependent reads, L2 resident), the face's three vertices, the point.
// cloud_fps_kernel    one workgroup of 1024 threads per object, pool position i = slot k * 1024 + thread t in registers (16 slots: x, y,
//                     z and the running minimum, 64 registers of the 128 a wave may hold at 16 waves per workgroup).  A step is 16
//                     distances per thread, a 64-bit maximum of (the minimum's bits, 16383 - position) across the wave, ONE barrier,
//                     and 16 broadcast reads: every wave's winner leaves its key AND its coordinates in LDS (two alternating rows), so
//                     the next pick's point needs no second exchange and no trip to memory.
#include "dvq_internal.h"

// every product, difference and sum rounded on its own (diverse.hip has the note on why the pragma and not __fmul_rn)
#pragma clang fp contract(off)

namespace {

constexpr int MS_T = 1024;                                  // threads of the cdf kernel = faces per scan chunk (ops.MESH_SAMPLE_CHUNK)
constexpr int MS_WAVES = MS_T / 64;
constexpr int MS_BLOCK = 256;                               // samples per workgroup of the points kernel
constexpr int MS_MAX_FACES = DVQ_GRASP_MESH_MAX_FACES;
constexpr int MS_MAX_S = DVQ_MESH_SAMPLE_MAX_S;
constexpr unsigned MS_TAG = 0xFFFFFFF0u;                    // first counter word: the prior's noise has a column quad < 2^31 there
constexpr float MS_SCALE = 1048575.0f;                      // 2^20 - 1

constexpr int FPS_T = 1024;
constexpr int FPS_SLOTS = 16;
constexpr int FPS_MAX_P = DVQ_CLOUD_FPS_MAX_P;
constexpr int FPS_WAVES = FPS_T / 64;
static_assert(FPS_T * FPS_SLOTS == FPS_MAX_P, "the pool fits the registers of one workgroup");

// Philox4x32-10 as misc.hip states it for dvq_exp1_noise: the same rounds, constants and key schedule
__device__ __forceinline__ void ms_philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ bool ms_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the face weight w of dvq.h; 0 for a face with an index outside [0, nv) (ok = false: nothing is read through it)
__device__ __forceinline__ float ms_face_w(const float* __restrict__ mv, const int* __restrict__ mf, int f, int nv, bool& ok) {
    const int a = mf[3 * f], b = mf[3 * f + 1], c = mf[3 * f + 2];
    ok = (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
    if (!ok) return 0.0f;
    const float ax = mv[3 * a], ay = mv[3 * a + 1], az = mv[3 * a + 2];
    const float e1x = mv[3 * b] - ax, e1y = mv[3 * b + 1] - ay, e1z = mv[3 * b + 2] - az;
    const float e2x = mv[3 * c] - ax, e2y = mv[3 * c + 1] - ay, e2z = mv[3 * c + 2] - az;
    const float yz = e1y * e2z, zy = e1z * e2y, zx = e1z * e2x, xz = e1x * e2z, xy = e1x * e2y, yx = e1y * e2x;
    const float nx = yz - zy, ny = zx - xz, nz = xy - yx;
    const float xx = nx * nx, yy = ny * ny, zz = nz * nz;
    const float s = xx + yy;
    const float w = sqrtf(s + zz);
    return ms_finite(w) ? w : 0.0f;
}

__global__ __launch_bounds__(MS_T) void mesh_cdf_kernel(const float* __restrict__ mverts, int n_mv, const int* __restrict__ vert_off,
                                                        const int* __restrict__ mfaces, int n_mf, const int* __restrict__ face_off,
                                                        const int64_t* __restrict__ stream_ids, unsigned long long* __restrict__ cdf,
                                                        int* __restrict__ status, int* err_flag) {
    __shared__ unsigned ms_tot[2][MS_WAVES];                 // the waves' chunk totals (pass A: their largest w), two alternating rows
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long o = blockIdx.x;
    const int vbase = vert_off[o], nv = vert_off[o + 1] - vbase, fbase = face_off[o], nf = face_off[o + 1] - fbase;
    const int64_t sid = stream_ids[o];
    const bool ranges = !(nv < 0 || nf < 0 || nf > MS_MAX_FACES || vbase < 0 || vbase > n_mv - nv || fbase < 0 || fbase > n_mf - nf);
    const bool keyed = sid >= 0 && sid <= (int64_t)0xFFFFFFFFLL;
    if (!ranges || !keyed) {                                 // uniform
        if (t == 0) {
            atomicOr(err_flag, (ranges ? 0 : 2) | (keyed ? 0 : 1));
            status[o] = 4;
        }
        return;
    }
    const float* mv = mverts + (long)vbase * 3;
    const int* mf = mfaces + (long)fbase * 3;
    unsigned long long* cd = cdf + fbase;

    // ---------------------------------------------------------------------------------------- pass A: w per face, the largest
    unsigned top = 0;                                        // w >= +0.0 and finite: its bits order as unsigned integers
    bool any_bad = false;
    for (int f = t; f < nf; f += MS_T) {
        bool ok;
        const unsigned wb = __float_as_uint(ms_face_w(mv, mf, f, nv, ok));
        any_bad |= !ok;
        cd[f] = wb;                                          // read back by this thread in pass B
        top = wb > top ? wb : top;
    }
    if (any_bad) atomicOr(err_flag, 2);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned x = __shfl_xor(top, s, 64);
        top = x > top ? x : top;
    }
    if (lane == 0) ms_tot[1][wave] = top;                    // row 1: pass B's first chunk writes row 0
    dvq_lds_barrier();
#pragma unroll
    for (int w = 0; w < MS_WAVES; ++w) top = ms_tot[1][w] > top ? ms_tot[1][w] : top;
    const float amax = __uint_as_float(top);

    // ---------------------------------------------------------------------------------------- pass B: q, the inclusive scan
    unsigned long long carry = 0;
    int chunk = 0;
    for (int f0 = 0; f0 < nf; f0 += MS_T, ++chunk) {
        const int f = f0 + t;
        unsigned q = 0;
        if (f < nf) {
            const float w = __uint_as_float((unsigned)cd[f]);
            if (w != 0.0f) {
                const float share = w / amax;
                const float scaled = share * MS_SCALE;
                q = 1u + (unsigned)truncf(scaled);
            }
        }
        unsigned run = q;                                    // a chunk's sum is at most 1024 * 2^20: 32 bits hold it
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned x = __shfl_up(run, s, 64);
            run += lane >= s ? x : 0u;
        }
        unsigned* tot = ms_tot[chunk & 1];
        if (lane == 63) tot[wave] = run;
        dvq_lds_barrier();                                   // the one barrier of the chunk: chunk + 2 writes this row again
        unsigned before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < MS_WAVES; ++w) {
            const unsigned x = tot[w];
            before += w < wave ? x : 0u;
            all += x;
        }
        if (f < nf) cd[f] = carry + before + run;
        carry += all;
    }
    if (t == 0) status[o] = carry == 0 ? 1 : 0;
}

__global__ __launch_bounds__(MS_BLOCK) void mesh_points_kernel(const float* __restrict__ mverts, const int* __restrict__ vert_off,
                                                               const int* __restrict__ mfaces, const int* __restrict__ face_off,
                                                               int S, int blocks_per_object, unsigned long long seed,
                                                               const int64_t* __restrict__ stream_ids,
                                                               const unsigned long long* __restrict__ cdf, const int* __restrict__ status,
                                                               float* __restrict__ points, int* __restrict__ face) {
    const long o = blockIdx.x / blocks_per_object;
    const int s = (int)(blockIdx.x - o * blocks_per_object) * MS_BLOCK + threadIdx.x;
    if (s >= S) return;
    float* p = points + (o * S + s) * 3;
    if (status[o] != 0) {                                    // uniform: no range of this object is looked at
        const float nanf_ = __builtin_nanf("");
        p[0] = nanf_, p[1] = nanf_, p[2] = nanf_;
        face[o * S + s] = -1;
        return;
    }
    const int vbase = vert_off[o], fbase = face_off[o], nf = face_off[o + 1] - fbase;
    const unsigned long long* cd = cdf + fbase;
    const unsigned long long T = cd[nf - 1];
    unsigned c[4] = {MS_TAG, (unsigned)s, 0u, (unsigned)stream_ids[o]};
    ms_philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned long long target = __umul64hi(((unsigned long long)c[0] << 32) | c[1], T);      // < T
    int lo = 0, hi = nf - 1;                                 // the smallest f with cdf[f] > target: cdf[nf - 1] = T is one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cd[mid] > target) hi = mid; else lo = mid + 1;
    }
    const float* mv = mverts + (long)vbase * 3;
    const int* mf = mfaces + ((long)fbase + lo) * 3;
    const int ia = mf[0], ib = mf[1], ic = mf[2];           // a drawn face has weight: its indices were checked
    float r1 = ((float)(c[2] >> 8) + 0.5f) * 5.9604644775390625e-08f;
    float r2 = ((float)(c[3] >> 8) + 0.5f) * 5.9604644775390625e-08f;
    const float both = r1 + r2;
    if (both > 1.0f) {
        r1 = 1.0f - r1;
        r2 = 1.0f - r2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = mv[3 * ia + k];
        const float e1 = mv[3 * ib + k] - a, e2 = mv[3 * ic + k] - a;
        const float u = r1 * e1, v = r2 * e2;
        const float au = a + u;
        p[k] = au + v;
    }
    face[o * S + s] = lo;
}

__global__ __launch_bounds__(FPS_T) void cloud_fps_kernel(const float* __restrict__ pts, int P, int keep, int* __restrict__ sel,
                                                          float* __restrict__ gap, int* __restrict__ status) {
    __shared__ __align__(16) unsigned long long fps_key[2][FPS_WAVES];     // the waves' winners, two alternating rows
    __shared__ float fps_xyz[2][3][FPS_WAVES];                             // and their coordinates
    __shared__ int fps_bad[FPS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long o = blockIdx.x;
    const float* po = pts + o * P * 3;
    int* so = sel + o * keep;
    float* go = gap + o * keep;

    float x[FPS_SLOTS], y[FPS_SLOTS], z[FPS_SLOTS], m[FPS_SLOTS];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < FPS_SLOTS; ++k) {
        const int i = k * FPS_T + t;
        const bool in = i < P;
        x[k] = in ? po[3 * i] : 0.0f;
        y[k] = in ? po[3 * i + 1] : 0.0f;
        z[k] = in ? po[3 * i + 2] : 0.0f;
        m[k] = in ? INFINITY : -1.0f;                        // -1: no point in this slot, or picked
        bad |= !(ms_finite(x[k]) && ms_finite(y[k]) && ms_finite(z[k]));
    }
    const bool wave_bad = __ballot(bad) != 0;
    if (lane == 0) fps_bad[wave] = wave_bad ? 1 : 0;
    dvq_lds_barrier();
    int any = 0;
#pragma unroll
    for (int w = 0; w < FPS_WAVES; ++w) any |= fps_bad[w];
    if (any) {                                               // uniform
        for (int r = t; r < keep; r += FPS_T) {
            so[r] = -1;
            go[r] = -1.0f;
        }
        if (t == 0) status[o] = 1;
        return;
    }
    if (t == 0) {
        status[o] = 0;
        so[0] = 0;
        go[0] = -1.0f;
        m[0] = -1.0f;
    }
    float cx = po[0], cy = po[1], cz = po[2];                // pick 0 is position 0 (P >= 1)
    for (int r = 1; r < keep; ++r) {
        float bm = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;   // this thread's largest minimum, in ascending positions: the lowest of equals
        int bk = 0;
#pragma unroll
        for (int k = 0; k < FPS_SLOTS; ++k) {
            const float dx = x[k] - cx, dy = y[k] - cy, dz = z[k] - cz;
            const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const float xy = xx + yy;
            const float d = xy + zz;
            const bool live = m[k] >= 0.0f;
            m[k] = (live && d < m[k]) ? d : m[k];
            const bool better = m[k] > bm;                   // a slot without a point, or picked, holds -1: never better
            bm = better ? m[k] : bm;
            bk = better ? k : bk;
            bx = better ? x[k] : bx;
            by = better ? y[k] : by;
            bz = better ? z[k] : bz;
        }
        // (minimum's bits | sign bit, 16383 - position): an unsigned maximum is the documented order; 0: nothing unpicked here
        const unsigned long long best =
            bm >= 0.0f ? ((unsigned long long)(__float_as_uint(bm) | 0x80000000u) << 32) | (unsigned)(FPS_MAX_P - 1 - (bk * FPS_T + t)) : 0ull;
        unsigned long long top = best;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned long long v = __shfl_xor(top, s, 64);
            top = v > top ? v : top;
        }
        const int row = r & 1;
        if (best == top && top != 0ull) {                    // one lane: the positions differ
            fps_key[row][wave] = top;
            fps_xyz[row][0][wave] = bx;
            fps_xyz[row][1][wave] = by;
            fps_xyz[row][2][wave] = bz;
        } else if (lane == 0 && top == 0ull) {
            fps_key[row][wave] = 0ull;
        }
        dvq_lds_barrier();                                   // the one barrier of the step: step r + 2 writes this row again
        unsigned long long win = 0;
#pragma unroll
        for (int w = 0; w < FPS_WAVES; ++w) {
            const unsigned long long v = fps_key[row][w];
            win = v > win ? v : win;
        }
        const int pos = FPS_MAX_P - 1 - (int)(unsigned)(win & 0xffffffffull);      // keep <= P: a step always has an unpicked position
        const int ww = (pos & (FPS_T - 1)) >> 6;
        cx = fps_xyz[row][0][ww];
        cy = fps_xyz[row][1][ww];
        cz = fps_xyz[row][2][ww];
        if ((pos & (FPS_T - 1)) == t) {
            const int slot = pos >> 10;
#pragma unroll
            for (int k = 0; k < FPS_SLOTS; ++k) m[k] = k == slot ? -1.0f : m[k];
            so[r] = pos;
            go[r] = __uint_as_float((unsigned)(win >> 32) & 0x7fffffffu);
        }
    }
}

}  // namespace

extern "C" int dvq_mesh_sample(const float* mesh_verts, int n_mv, const int32_t* vert_off, const int32_t* mesh_faces, int n_mf,
                               const int32_t* face_off, int64_t O, int S, uint64_t seed, const int64_t* stream_ids, uint64_t* cdf,
                               float* points, int32_t* face, int32_t* status, int32_t* err_flag, dvq_stream_t stream) {
    DVQ_REQUIRE(O >= 0 && S >= 1 && S <= MS_MAX_S && n_mv >= 0 && n_mf >= 0,
                "mesh_sample: need O >= 0, 1 <= S <= %d, n_mv >= 0, n_mf >= 0 (got O=%ld S=%d n_mv=%d n_mf=%d)", MS_MAX_S, (long)O, S, n_mv,
                n_mf);
    if (O == 0) return DVQ_OK;
    DVQ_REQUIRE((mesh_verts || n_mv == 0) && vert_off && (mesh_faces || n_mf == 0) && face_off && stream_ids && (cdf || n_mf == 0) && points &&
                    face && status && err_flag,
                "mesh_sample: null pointer");
    const int64_t blocks_per_object = (S + MS_BLOCK - 1) / MS_BLOCK;
    DVQ_REQUIRE(O <= 0x7fffffffLL / blocks_per_object, "mesh_sample: O * ceil(S / %d) must stay below 2^31 (got O=%ld S=%d)", MS_BLOCK, (long)O,
                S);
    hipStream_t st = (hipStream_t)stream;
    {
        // in: every face's indices and (gathered) vertices once; out and in again: the cdf word written twice and read once
        DVQ_PROF("mesh_sample_cdf", 0.0, (double)n_mf * (12.0 + 36.0 + 24.0), st);
        DVQ_LAUNCH(mesh_cdf_kernel, dim3((unsigned)O), dim3(MS_T), 0, st, mesh_verts, n_mv, vert_off, mesh_faces, n_mf, face_off, stream_ids,
                   reinterpret_cast<unsigned long long*>(cdf), status, err_flag);
    }
    DVQ_CHECK_LAUNCH("mesh_sample");
    {
        DVQ_PROF("mesh_sample_points", 0.0, (double)O * S * (16.0 + 12.0 + 36.0), st);
        DVQ_LAUNCH(mesh_points_kernel, dim3((unsigned)(O * blocks_per_object)), dim3(MS_BLOCK), 0, st, mesh_verts, vert_off, mesh_faces,
                   face_off, S, (int)blocks_per_object, (unsigned long long)seed, stream_ids,
                   reinterpret_cast<const unsigned long long*>(cdf), status, points, face);
    }
    DVQ_CHECK_LAUNCH("mesh_sample");
    return DVQ_OK;
}

extern "C" int dvq_cloud_fps(const float* points, int64_t O, int P, int keep, int32_t* sel, float* gap, int32_t* status,
                             dvq_stream_t stream) {
    DVQ_REQUIRE(O >= 0 && keep >= 1 && keep <= P && P <= FPS_MAX_P, "cloud_fps: need O >= 0, 1 <= keep <= P <= %d (got O=%ld P=%d keep=%d)",
                FPS_MAX_P, (long)O, P, keep);
    if (O == 0) return DVQ_OK;
    DVQ_REQUIRE(points && sel && gap && status, "cloud_fps: null pointer");
    DVQ_REQUIRE(O <= 0x7fffffffLL, "cloud_fps: O too large");
    hipStream_t st = (hipStream_t)stream;
    DVQ_PROF("cloud_fps", 8.0 * (double)O * (keep - 1) * FPS_MAX_P, (double)O * (12.0 * P + 8.0 * keep + 4), st);
    DVQ_LAUNCH(cloud_fps_kernel, dim3((unsigned)O), dim3(FPS_T), 0, st, points, P, keep, sel, gap, status);
    DVQ_CHECK_LAUNCH("cloud_fps");
    return DVQ_OK;
}
