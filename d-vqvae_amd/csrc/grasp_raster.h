// The sealed hand on the object's lattice, written once for the two voxel kernels (grasp_volume.hip: the hand against the object's
// convex hull; grasp_mesh_volume.hip: against the object's mesh): steps 1 - 8 of dvq_grasp_volume (include/dvq.h).  The hand's
// V + L vertices sit in LDS in the object's frame as x|y|z planes; the box of cells is walked in tiles of columns; per tile a plane
// of bit words, word-major (word w of all columns side by side), takes ONE toggled bit per (triangle, covered column) at the last
// cell below the crossing, so that "an odd number of crossings above cell k" is the suffix parity of the column's bits.
//
// No helper contains a barrier: where the planes and the bit words are published is visible in each kernel.
#pragma once
#include "dvq_internal.h"
#include "grasp_scan.h"

constexpr int GV_THREADS = GRASP_THREADS;   // (the hand load is grasp_scan.h's)
constexpr int GV_MAX_V = GRASP_MAX_V;
constexpr int GV_MAX_L = 64;
constexpr int GV_MAX_F = 8192;
constexpr int GV_MAX_CELLS = 1024;          // per axis of the box
constexpr int GV_IDX_LIMIT = 4194302;       // |cell index| up to here: (float)i + 0.5f is exact
constexpr int GV_MASK_WORDS = 4096;         // bit words of a tile
constexpr int GV_MAX_COLS = 2048;           // columns of a tile
constexpr int GV_TILE_X = 64;
constexpr int GV_SMALL = 16;                // ints: flags and the count

__host__ __device__ constexpr int gv_vp(int V, int L) { return (V + L + 3) & ~3; }

__device__ __forceinline__ float gv_c(int i, float h) { return ((float)i + 0.5f) * h; }

// the number of cells kk in [0, nk) with c(lo + kk) < z (STRICT) or <= z: c is non-decreasing in kk, so a guess and two walks
template <bool STRICT>
__device__ __forceinline__ int gv_cells(float z, float h, int lo, int nk) {
    if (z != z) return 0;
    const float gf = floorf(z / h - 0.5f) - (float)lo + 1.0f;
    int g = gf < 0.0f ? 0 : (gf > (float)nk ? nk : (int)gf);
    // (a step or two each; kept scalar: the loop vectoriser would turn them into eight-wide searches with packed-fp32 arithmetic)
#pragma clang loop vectorize(disable) interleave(disable)
    while (g < nk && (STRICT ? gv_c(lo + g, h) < z : gv_c(lo + g, h) <= z)) ++g;
#pragma clang loop vectorize(disable) interleave(disable)
    while (g > 0 && !(STRICT ? gv_c(lo + g - 1, h) < z : gv_c(lo + g - 1, h) <= z)) --g;
    return g;
}

__device__ __forceinline__ bool gv_index_ok(float f) { return fabsf(f) <= (float)GV_IDX_LIMIT; }   // false for a NaN

// Step 1: thread t < L writes the fan centre of loop t, in the row's frame (the hand must be published).
__device__ __forceinline__ void gv_fan_centre(int t, const int32_t* __restrict__ loop_off, const int32_t* __restrict__ loop_vert, int n_loop,
                                              int V, float* vx, float* vy, float* vz, int32_t* err_flag) {
    int q0 = loop_off[t], q1 = loop_off[t + 1];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (q0 < 0 || q1 > n_loop) q0 = q1 = 0;                               // offsets outside loop_vert: an empty loop
    bool bad = q1 <= q0;
    for (int q = q0; q < q1; ++q) {
        const int v = loop_vert[q];
        if ((unsigned)v >= (unsigned)V) {
            bad = true;
            continue;
        }
        sx += vx[v];
        sy += vy[v];
        sz += vz[v];
    }
    const float len = (float)(q1 - q0);
    vx[V + t] = q1 > q0 ? sx / len : 0.0f;
    vy[V + t] = q1 > q0 ? sy / len : 0.0f;
    vz[V + t] = q1 > q0 ? sz / len : 0.0f;
    if (bad) atomicOr(err_flag, 2);
}

// Step 2 and the extent of step 3: thread t's share of the VT vertices into the object's frame, each vertex by its owner, and the
// smallest / largest components it saw (a NaN from R goes into mn[0]: the box is refused).
__device__ __forceinline__ void gv_object_frame(int t, long b, int VT, const float* __restrict__ R, const float* __restrict__ tr, float* vx,
                                                float* vy, float* vz, float (&mn)[3], float (&mx)[3]) {
    float r[9], tt[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = R ? R[b * 9 + i] : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) tt[i] = tr ? tr[i] : 0.0f;
    for (int i = t; i < VT; i += GV_THREADS) {
        float x = vx[i], y = vy[i], z = vz[i];
        if (R) {
            const float u0 = tr ? x - tt[0] : x, u1 = tr ? y - tt[1] : y, u2 = tr ? z - tt[2] : z;
            x = fmaf(r[6], u2, fmaf(r[3], u1, r[0] * u0));
            y = fmaf(r[7], u2, fmaf(r[4], u1, r[1] * u0));
            z = fmaf(r[8], u2, fmaf(r[5], u1, r[2] * u0));
            vx[i] = x;
            vy[i] = y;
            vz[i] = z;
        }
        mn[0] = x < mn[0] ? x : mn[0];
        mn[1] = y < mn[1] ? y : mn[1];
        mn[2] = z < mn[2] ? z : mn[2];
        mx[0] = x > mx[0] ? x : mx[0];
        mx[1] = y > mx[1] ? y : mx[1];
        mx[2] = z > mx[2] ? z : mx[2];
        if (x != x || y != y || z != z) mn[0] = __builtin_nanf("");       // a NaN from R: the box is refused below
    }
}

// One step of the workgroup's reduction of the six extent columns of red[.][GV_THREADS] (0 .. 2: minima, a NaN sticks; 3 .. 5: maxima).
__device__ __forceinline__ void gv_reduce_extent(float* red, int t, int s) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = red[c * GV_THREADS + t], a2 = red[c * GV_THREADS + t + s];
        red[c * GV_THREADS + t] = (a2 < a || a2 != a2) ? a2 : a;          // a NaN sticks
        const float m = red[(3 + c) * GV_THREADS + t], m2 = red[(3 + c) * GV_THREADS + t + s];
        red[(3 + c) * GV_THREADS + t] = m2 > m ? m2 : m;
    }
}

// Step 3 from the reduced extent: the box (lo, n per axis); false when it is refused (status 2).
__device__ __forceinline__ bool gv_box(const float* red, float h, int (&lo)[3], int (&n)[3]) {
    bool fits = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float fl = floorf(red[c * GV_THREADS] / h), fh = floorf(red[(3 + c) * GV_THREADS] / h);
        const bool ok = gv_index_ok(fl) && gv_index_ok(fh);
        lo[c] = ok ? (int)fl - 1 : 0;
        n[c] = ok ? ((int)fh + 1) - lo[c] + 1 : GV_MAX_CELLS + 1;
        fits &= n[c] <= GV_MAX_CELLS;
    }
    return fits;
}

// The tile split of a box of nx x ny columns of nk cells: W bit words per column, tiles of TX x TY columns.
struct GvTiles {
    int W, TX, TY;
};
__device__ __forceinline__ GvTiles gv_tiles(int nx, int ny, int nk) {
    GvTiles g;
    g.W = (nk + 31) >> 5;                                                  // <= 32 bit words per column
    const int per_tile = GV_MASK_WORDS / g.W < GV_MAX_COLS ? GV_MASK_WORDS / g.W : GV_MAX_COLS;   // >= 128
    g.TX = nx < GV_TILE_X ? nx : GV_TILE_X;
    g.TY = per_tile / g.TX < ny ? per_tile / g.TX : ny;                    // >= 1: per_tile >= 128 >= TX
    return g;
}

// Rules 4 - 7 for ONE triangle with a non-zero projected area A, scattered: every column (i, j) of [i0, i1] x [j0, j1] -- a range
// inside the tile (ia, ja: its first column; tw: its width; ncol: its columns) -- that the triangle covers and for which live(col)
// holds gets one bit of `mask` toggled at the last cell below the crossing.  a, bb, c: the indices that give the edges their
// canonical direction.
template <class Live>
__device__ __forceinline__ void gv_scatter_face(int a, int bb, int c, float ax, float ay, float az, float bx, float by, float bz, float cx,
                                                float cy, float cz, float A, float xmn, float xmx, float ymn, float ymx, int i0, int i1,
                                                int j0, int j1, int ia, int ja, int tw, int ncol, float h, int klo, int nk, unsigned* mask,
                                                Live live) {
    // the three edges in canonical direction: e1 of (a,b), e2 of (b,c), e3 of (c,a); rev: the triangle runs Q -> P
    const bool r1 = a > bb, r2 = bb > c, r3 = c > a;
    const float p1x = r1 ? bx : ax, p1y = r1 ? by : ay, d1x = r1 ? ax - bx : bx - ax, d1y = r1 ? ay - by : by - ay;
    const float p2x = r2 ? cx : bx, p2y = r2 ? cy : by, d2x = r2 ? bx - cx : cx - bx, d2y = r2 ? by - cy : cy - by;
    const float p3x = r3 ? ax : cx, p3y = r3 ? ay : cy, d3x = r3 ? cx - ax : ax - cx, d3y = r3 ? cy - ay : ay - cy;
    const bool up = A > 0.0f;
    // what an edge value of exactly 0 counts as: its sign at the column moved by (eps, eps^2)
    const bool z1 = d1y < 0.0f || (d1y == 0.0f && d1x > 0.0f), z2 = d2y < 0.0f || (d2y == 0.0f && d2x > 0.0f),
               z3 = d3y < 0.0f || (d3y == 0.0f && d3x > 0.0f);
    for (int j = j0; j <= j1; ++j) {
        const float y = gv_c(j, h);
        if (!(ymn <= y && y <= ymx)) continue;
        for (int i = i0; i <= i1; ++i) {
            const float x = gv_c(i, h);
            if (!(xmn <= x && x <= xmx)) continue;
            const int col = (j - ja) * tw + (i - ia);
            if (!live(col)) continue;
            const float e1 = d1x * (y - p1y) - d1y * (x - p1x);
            const float e2 = d2x * (y - p2y) - d2y * (x - p2x);
            const float e3 = d3x * (y - p3y) - d3y * (x - p3x);
            // the positive side of an edge belongs to the triangle iff (A > 0) != (it runs Q -> P)
            const bool s1 = e1 > 0.0f || (e1 == 0.0f && z1), s2 = e2 > 0.0f || (e2 == 0.0f && z2), s3 = e3 > 0.0f || (e3 == 0.0f && z3);
            if (s1 != (up != r1) || s2 != (up != r2) || s3 != (up != r3)) continue;
            if (e1 != e1 || e2 != e2 || e3 != e3) continue;
            const float wc = r1 ? -e1 : e1, wa = r2 ? -e2 : e2, wb = r3 ? -e3 : e3;
            const float zc = ((wa * az + wb * bz) + wc * cz) / ((wa + wb) + wc);
            const int m = gv_cells<true>(zc, h, klo, nk);                 // cells 0 .. m-1 lie below the crossing
            if (m > 0) atomicXor(&mask[((m - 1) >> 5) * ncol + col], 1u << ((m - 1) & 31));
        }
    }
}

// Phase R of a tile for the hand: every thread takes TRIANGLES of the sealed list (scatter, not gather) and walks the columns of the
// triangle's xy box inside the tile (columns ia .. ib, ja .. jb).  A face with an index outside [0, VT) is skipped.
template <class Live>
__device__ __forceinline__ void gv_raster_hand(int t, const int32_t* __restrict__ faces, int F, int VT, const float* vx, const float* vy,
                                               const float* vz, float h, int ia, int ib, int ja, int jb, int klo, int nk, unsigned* mask,
                                               Live live) {
    const int tw = ib - ia + 1, ncol = tw * (jb - ja + 1);
    for (int f = t; f < F; f += GV_THREADS) {
        const int a = faces[3 * f], bb = faces[3 * f + 1], c = faces[3 * f + 2];
        if ((unsigned)a >= (unsigned)VT || (unsigned)bb >= (unsigned)VT || (unsigned)c >= (unsigned)VT) {
            continue;                                                      // (reported once, before the tiles)
        }
        const float ax = vx[a], ay = vy[a], az = vz[a], bx = vx[bb], by = vy[bb], bz = vz[bb], cx = vx[c], cy = vy[c], cz = vz[c];
        const float A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
        if (!(A > 0.0f) && !(A < 0.0f)) continue;
        const float xmn = fminf(ax, fminf(bx, cx)), xmx = fmaxf(ax, fmaxf(bx, cx));
        const float ymn = fminf(ay, fminf(by, cy)), ymx = fmaxf(ay, fmaxf(by, cy));
        int i0 = (int)floorf(xmn / h) - 1, i1 = (int)floorf(xmx / h) + 1;   // inside the box: the box is made of these values
        int j0 = (int)floorf(ymn / h) - 1, j1 = (int)floorf(ymx / h) + 1;
        i0 = i0 < ia ? ia : i0;
        i1 = i1 > ib ? ib : i1;
        j0 = j0 < ja ? ja : j0;
        j1 = j1 > jb ? jb : j1;
        if (i0 > i1 || j0 > j1) continue;
        gv_scatter_face(a, bb, c, ax, ay, az, bx, by, bz, cx, cy, cz, A, xmn, xmx, ymn, ymx, i0, i1, j0, j1, ia, ja, tw, ncol, h, klo, nk,
                        mask, live);
    }
}

// Thread t's share of the check of the sealed face list: an index outside [0, VT) sets bit 1 of the error flag.
__device__ __forceinline__ void gv_check_faces(int t, const int32_t* __restrict__ faces, int F, int VT, int32_t* err_flag) {
    for (int f = t; f < F; f += GV_THREADS) {
        if ((unsigned)faces[3 * f] >= (unsigned)VT || (unsigned)faces[3 * f + 1] >= (unsigned)VT || (unsigned)faces[3 * f + 2] >= (unsigned)VT)
            atomicOr(err_flag, 2);
    }
}

// Bit i of the result = the parity of the bits i .. 31 of v.
__device__ __forceinline__ unsigned gv_suffix_parity(unsigned v) {
    unsigned s = v;
    s ^= s >> 1;
    s ^= s >> 2;
    s ^= s >> 4;
    s ^= s >> 8;
    s ^= s >> 16;
    return s;
}
