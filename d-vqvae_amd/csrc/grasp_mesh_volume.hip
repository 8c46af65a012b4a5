// dvq_grasp_mesh_volume: the voxels shared by the sealed hand mesh and the object's closed triangle MESH (not its hull: a finger in
// the hollow of a cup shares nothing with the cup), in ONE kernel, one workgroup of 256 threads per grasp.  The definition is the ABI
// (include/dvq.h); this file only says how the kernel is laid out.  The count is an integer, so nothing below has to keep an order.
//
// The hand's side is grasp_volume.hip's, from grasp_raster.h: the V + L vertices in LDS in the object's frame as x|y|z planes, the
// box of cells walked in tiles of columns, a plane of bit words per tile.  The object's side is a SECOND plane of bit words, filled
// the same way from the object's faces (global memory, gathered through the face indices): one thread per face, one integer
// atomicXor in LDS at the last cell below the crossing.  Per tile:
//   O  the object's faces are scattered into the object plane.  A face's column range is clamped to the tile IN FLOAT before any
//      conversion to int: object coordinates are arbitrary, (int)floorf(x / h) of a far vertex is undefined.
//   L  every thread takes columns: a column with a set object bit holds an object voxel (its highest set bit is one), any other
//      holds none.  A tile without such a column is done -- the hand is not rasterised there; most of a hand's box is free.
//   R  grasp_raster.h's hand scatter into the hand plane, for the live columns only.
//   C  every thread takes columns again: the two suffix parities from the top word down, ANDed, popcount.
// Walking all faces of the object once per tile would be tiles x faces gathers per grasp (a box has about 50 tiles at 1 mm), so the
// faces are culled ONCE per grasp: those whose column range meets the box and that are not wholly at or below its lowest cell centre
// (rule 9' skips them by definition) go into an index list of GMV_LIST entries in LDS, and phase O walks the list.  When the list
// overflows, phase O walks all faces with the same two tests: both paths toggle the same bits.
// LDS: 12 (V + L) + 2 x 16 KB of bit words + 8 KB of column flags + 8 KB of list = 57 KB at MANO's 779 vertices, 73 KB at the largest
// hand (above 64 KB: the launcher raises the kernel's limit); two workgroups per CU of 160 KB in both cases.
#include "dvq_internal.h"
#include "grasp_raster.h"

namespace {

constexpr int GMV_MAX_FACES = DVQ_GRASP_MESH_MAX_FACES;   // per object
constexpr int GMV_LIST = 2048;                            // culled face indices kept in LDS (ops.GRASP_MESH_VOLUME_LIST)
static_assert(6 * GV_THREADS <= GV_MASK_WORDS, "the box's reduction columns borrow the hand's bit words");

__host__ __device__ constexpr size_t gmv_lds_bytes(int V, int L) {
    return (size_t)(3 * gv_vp(V, L) + 2 * GV_MASK_WORDS + GV_MAX_COLS + GMV_LIST + GV_SMALL) * 4;
}

// A face's column range along one axis, floorf(mn / h) - 1 .. floorf(mx / h) + 1, clamped to [a, b] in float (a, b are cell indices
// of the box: exact as floats; a NaN or an infinity clamps like any other value): false when it is empty.
__device__ __forceinline__ bool gmv_range(float mn, float mx, float h, int a, int b, int& i0, int& i1) {
    const float f0 = fmaxf(floorf(mn / h) - 1.0f, (float)a), f1 = fminf(floorf(mx / h) + 1.0f, (float)b);
    if (!(f0 <= f1)) return false;
    i0 = (int)f0;
    i1 = (int)f1;
    return true;
}

// The nine coordinates of object face f (its indices in [0, nv): checked by the caller).
struct GmvFace {
    int a, b, c;
    float ax, ay, az, bx, by, bz, cx, cy, cz;
};
__device__ __forceinline__ bool gmv_load_face(const float* __restrict__ mv, const int* __restrict__ mf, int nv, int f, GmvFace& q) {
    q.a = mf[3 * f], q.b = mf[3 * f + 1], q.c = mf[3 * f + 2];
    if ((unsigned)q.a >= (unsigned)nv || (unsigned)q.b >= (unsigned)nv || (unsigned)q.c >= (unsigned)nv) return false;
    q.ax = mv[3 * q.a], q.ay = mv[3 * q.a + 1], q.az = mv[3 * q.a + 2];
    q.bx = mv[3 * q.b], q.by = mv[3 * q.b + 1], q.bz = mv[3 * q.b + 2];
    q.cx = mv[3 * q.c], q.cy = mv[3 * q.c + 1], q.cz = mv[3 * q.c + 2];
    return true;
}

// Rule 9' for one object face against the columns ia .. ib, ja .. jb (the box for the cull, a tile for phase O): false for a face
// that takes part in none of them -- no area, all three heights at or below zbot, or a column range that misses.
struct GmvSpan {
    float A, xmn, xmx, ymn, ymx;
    int i0, i1, j0, j1;
};
__device__ __forceinline__ bool gmv_span(const GmvFace& q, float h, float zbot, int ia, int ib, int ja, int jb, GmvSpan& s) {
    s.A = (q.bx - q.ax) * (q.cy - q.ay) - (q.by - q.ay) * (q.cx - q.ax);
    if (!(s.A > 0.0f) && !(s.A < 0.0f)) return false;
    if (q.az <= zbot && q.bz <= zbot && q.cz <= zbot) return false;       // (a NaN height keeps the face: its crossing is a NaN)
    s.xmn = fminf(q.ax, fminf(q.bx, q.cx)), s.xmx = fmaxf(q.ax, fmaxf(q.bx, q.cx));
    s.ymn = fminf(q.ay, fminf(q.by, q.cy)), s.ymx = fmaxf(q.ay, fmaxf(q.by, q.cy));
    return gmv_range(s.xmn, s.xmx, h, ia, ib, s.i0, s.i1) && gmv_range(s.ymn, s.ymx, h, ja, jb, s.j0, s.j1);
}

__global__ __launch_bounds__(GV_THREADS) void grasp_mesh_volume_kernel(const float* __restrict__ hand, int V, const int32_t* __restrict__ faces,
                                                                       int F, const int32_t* __restrict__ loop_off,
                                                                       const int32_t* __restrict__ loop_vert, int L, int n_loop,
                                                                       const float* __restrict__ mverts, int n_mv,
                                                                       const int32_t* __restrict__ vert_off, const int32_t* __restrict__ mfaces,
                                                                       int n_mf, const int32_t* __restrict__ face_off, long O,
                                                                       const int64_t* __restrict__ obj_of_row, const float* __restrict__ R,
                                                                       const float* __restrict__ tr, float h, int32_t* __restrict__ count,
                                                                       int32_t* __restrict__ status, int32_t* err_flag) {
    extern __shared__ __align__(16) float gmv_lds[];
    const int VT = V + L, VP = gv_vp(V, L);
    float* vx = gmv_lds;
    float* vy = vx + VP;
    float* vz = vy + VP;
    unsigned* hmask = reinterpret_cast<unsigned*>(vz + VP);                // [GV_MASK_WORDS]: the hand's crossings
    unsigned* omask = hmask + GV_MASK_WORDS;                               // [GV_MASK_WORDS]: the object's crossings
    int* live = reinterpret_cast<int*>(omask + GV_MASK_WORDS);             // [GV_MAX_COLS]: the column holds an object voxel
    int* list = live + GV_MAX_COLS;                                        // [GMV_LIST]: the culled faces, in any order
    float* red = reinterpret_cast<float*>(hmask);                          // [6][256]: the box's columns, before the first tile
    int* small = list + GMV_LIST;                  // 0: not finite, 1: count, 2 .. 4: a tile has a live column, 5: faces kept, 6: object seen
    const int t = threadIdx.x;
    const long b = blockIdx.x;

    const int64_t o = obj_of_row[b];
    int vbase = 0, nv = -1, fbase = 0, nf = -1;
    if (o >= 0 && o < O) {
        vbase = vert_off[o];
        nv = vert_off[o + 1] - vbase;
        fbase = face_off[o];
        nf = face_off[o + 1] - fbase;
    }
    if (nv < 0 || nf < 0 || nf > GMV_MAX_FACES || vbase < 0 || vbase > n_mv - nv || fbase < 0 || fbase > n_mf - nf) {   // uniform
        if (t == 0) {
            atomicOr(err_flag, (o >= 0 && o < O) ? 2 : 1);
            count[b] = -1;
            status[b] = 4;
        }
        return;
    }
    if (t < GV_SMALL) small[t] = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, vx, vy, vz)) small[0] = 1;    // the hand as given, and whether it is finite
    dvq_lds_barrier();
    if (small[0] || nf == 0) {
        if (t == 0) {
            count[b] = small[0] ? -1 : 0;
            status[b] = small[0] ? 3 : 1;
        }
        return;
    }
    const float* mv = mverts + (long)vbase * 3;
    const int* mf = mfaces + (long)fbase * 3;
    if (t < L) gv_fan_centre(t, loop_off, loop_vert, n_loop, V, vx, vy, vz, err_flag);   // in the row's frame
    dvq_lds_barrier();
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    gv_object_frame(t, b, VT, R, tr, vx, vy, vz, mn, mx);                 // each vertex by its owner
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        red[c * GV_THREADS + t] = mn[c];
        red[(3 + c) * GV_THREADS + t] = mx[c];
    }
    dvq_lds_barrier();                                                     // every vertex is in place
    for (int s = GV_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) gv_reduce_extent(red, t, s);
        dvq_lds_barrier();
    }
    int lo[3], n[3];
    if (!gv_box(red, h, lo, n)) {
        if (t == 0) {
            count[b] = -1;
            status[b] = 2;
        }
        return;
    }
    const int nx = n[0], ny = n[1], nk = n[2], ilo = lo[0], jlo = lo[1], klo = lo[2];
    const GvTiles tiles = gv_tiles(nx, ny, nk);
    const int W = tiles.W, TX = tiles.TX, TY = tiles.TY;
    const float zbot = gv_c(klo, h);
    gv_check_faces(t, faces, F, VT, err_flag);
    // the cull, once per grasp: the faces that take part in a column of the box, and the one report of a face index out of range
    for (int f = t; f < nf; f += GV_THREADS) {
        GmvFace q;
        GmvSpan s;
        if (!gmv_load_face(mv, mf, nv, f, q)) {
            atomicOr(err_flag, 2);
            continue;
        }
        if (!gmv_span(q, h, zbot, ilo, ilo + nx - 1, jlo, jlo + ny - 1, s)) continue;
        const int at = atomicAdd(&small[5], 1);
        if (at < GMV_LIST) list[at] = f;
    }
    dvq_lds_barrier();                                                     // (and every thread is through with the reduction columns)
    const int kept = small[5];
    const bool listed = kept <= GMV_LIST;
    const int n_walk = listed ? kept : nf;                                 // overflow: all faces, with the same tests
    int mine = 0, seen = 0, tile = 0;
    for (int ty0 = 0; ty0 < ny && kept > 0; ty0 += TY) {
        for (int tx0 = 0; tx0 < nx; tx0 += TX, ++tile) {
            const int tw = nx - tx0 < TX ? nx - tx0 : TX, th = ny - ty0 < TY ? ny - ty0 : TY;
            const int ncol = tw * th;
            const int ia = ilo + tx0, ib = ia + tw - 1, ja = jlo + ty0, jb = ja + th - 1;
            int* flag = small + 2 + tile % 3;
            if (t == 0) small[2 + (tile + 1) % 3] = 0;                    // the next tile's flag: last read two barriers ago
            for (int i = t; i < ncol * W; i += GV_THREADS) omask[i] = 0u;
            dvq_lds_barrier();
            // O: every object face toggles one bit in each column it covers
            for (int i = t; i < n_walk; i += GV_THREADS) {
                GmvFace q;
                GmvSpan s;
                if (!gmv_load_face(mv, mf, nv, listed ? list[i] : i, q)) continue;   // (reported once, by the cull)
                if (!gmv_span(q, h, zbot, ia, ib, ja, jb, s)) continue;
                gv_scatter_face(q.a, q.b, q.c, q.ax, q.ay, q.az, q.bx, q.by, q.bz, q.cx, q.cy, q.cz, s.A, s.xmn, s.xmx, s.ymn, s.ymx, s.i0,
                                s.i1, s.j0, s.j1, ia, ja, tw, ncol, h, klo, nk, omask, [](int) { return true; });
            }
            dvq_lds_barrier();
            // L: the columns that hold an object voxel
            bool any = false;
            for (int c = t; c < ncol; c += GV_THREADS) {
                unsigned bits = 0u;
                for (int w = 0; w < W; ++w) bits |= omask[w * ncol + c];
                live[c] = bits != 0u;
                any |= bits != 0u;
            }
            if (any) *flag = 1;
            dvq_lds_barrier();
            if (*flag == 0) continue;                                      // uniform: no object voxel in the tile
            seen = 1;
            for (int i = t; i < ncol * W; i += GV_THREADS) hmask[i] = 0u;
            dvq_lds_barrier();
            // R: every triangle of the hand toggles one bit in each live column it covers
            gv_raster_hand(t, faces, F, VT, vx, vy, vz, h, ia, ib, ja, jb, klo, nk, hmask, [&](int col) { return live[col] != 0; });
            dvq_lds_barrier();
            // C: the two suffix parities from the top word down, ANDed
            for (int c = t; c < ncol; c += GV_THREADS) {
                if (live[c] == 0) continue;
                unsigned hcarry = 0u, ocarry = 0u;
                for (int w = W - 1; w >= 0; --w) {
                    const unsigned hv = hmask[w * ncol + c], ov = omask[w * ncol + c];
                    mine += __popc((gv_suffix_parity(hv) ^ hcarry) & (gv_suffix_parity(ov) ^ ocarry));
                    hcarry ^= (__popc(hv) & 1) ? 0xffffffffu : 0u;
                    ocarry ^= (__popc(ov) & 1) ? 0xffffffffu : 0u;
                }
            }
            dvq_lds_barrier();                                             // the next tile rewrites the flags and the bit words
        }
    }
    if (mine) atomicAdd(&small[1], mine);
    if (seen) small[6] = 1;
    dvq_lds_barrier();
    if (t == 0) {
        count[b] = small[1];
        status[b] = small[6] ? 0 : 1;
    }
}

}  // namespace

extern "C" int dvq_grasp_mesh_volume(const float* hand, int V, const int32_t* faces, int F, const int32_t* loop_off,
                                     const int32_t* loop_vert, int L, int n_loop, const float* mesh_verts, int n_mv,
                                     const int32_t* vert_off, const int32_t* mesh_faces, int n_mf, const int32_t* face_off, int64_t O,
                                     const int64_t* obj_of_row, const float* R, const float* t, int64_t B, float h, int32_t* count,
                                     int32_t* status, int32_t* err_flag, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && V >= 1 && V <= GV_MAX_V && F >= 0 && F <= GV_MAX_F && L >= 0 && L <= GV_MAX_L && O >= 0 && n_loop >= 0 && n_mv >= 0 &&
                    n_mf >= 0,
                "grasp_mesh_volume: need B >= 0, 1 <= V <= %d, 0 <= F <= %d, 0 <= L <= %d, O >= 0, n_loop >= 0, n_mv >= 0, n_mf >= 0 (got B=%ld "
                "V=%d F=%d L=%d O=%ld n_loop=%d n_mv=%d n_mf=%d)",
                GV_MAX_V, GV_MAX_F, GV_MAX_L, (long)B, V, F, L, (long)O, n_loop, n_mv, n_mf);
    DVQ_REQUIRE(h > 0.0f && h < INFINITY, "grasp_mesh_volume: the lattice spacing must be finite and positive (got %g)", (double)h);
    DVQ_REQUIRE(R || !t, "grasp_mesh_volume: t without R");
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && (faces || F == 0) && loop_off && (loop_vert || n_loop == 0) && (mesh_verts || n_mv == 0) && vert_off &&
                    (mesh_faces || n_mf == 0) && face_off && obj_of_row && count && status && err_flag,
                "grasp_mesh_volume: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = gmv_lds_bytes(V, L);
    static DvqOncePerDevice attr_once;                                     // 73 KB at the largest hand: above the default limit
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&grasp_mesh_volume_kernel), gmv_lds_bytes(GV_MAX_V, GV_MAX_L),
                                "grasp_mesh_volume"));
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // the work depends on the data (the box, each row's face count, how much of the box the object meets): reported as 0 FLOPs.
        // in: the hand; out: 8 B per grasp
        DVQ_PROF("grasp_mesh_volume", 0.0, (double)nb * ((double)V * 12 + 8), st);
        DVQ_LAUNCH(grasp_mesh_volume_kernel, dim3((unsigned)nb), dim3(GV_THREADS), lds, st, hand + b0 * V * 3, V, faces, F, loop_off,
                   loop_vert, L, n_loop, mesh_verts, n_mv, vert_off, mesh_faces, n_mf, face_off, (long)O, obj_of_row + b0,
                   R ? R + b0 * 9 : nullptr, t, h, count + b0, status + b0, err_flag);
    });
    DVQ_CHECK_LAUNCH("grasp_mesh_volume");
    return DVQ_OK;
}
