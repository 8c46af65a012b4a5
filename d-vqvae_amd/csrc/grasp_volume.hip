// dvq_grasp_volume: the voxels shared by the sealed hand mesh and the object's convex hull, and the deepest vertex inside the hull,
// in ONE kernel, one workgroup of 256 threads per grasp.  The definition is the ABI (include/dvq.h); this file only says how the
// kernel is laid out.  The count is an integer, so nothing below has to keep an order.
//
// The hand's side -- steps 1 - 8: the planes, the box, the tile split, phase R -- is grasp_raster.h's, shared with grasp_mesh_volume.hip.
//
// The hand's V + L vertices sit in LDS in the object's frame as x|y|z planes.  The box of cells is walked in tiles of columns.
// Per tile:
//   H  every thread takes columns and intersects them with the object's half-spaces (planes from global memory, the same address
//      in every lane; a column leaves the loop as soon as its interval is empty or misses the box): the cells of the column inside
//      the hull are one range [ka, kb), kept in LDS.  A tile without such a column is done -- most of a hand's box is.
//   R  every thread takes TRIANGLES (not columns: scatter, not gather) and walks the columns of the triangle's xy box inside the
//      tile; a covered column gets ONE bit toggled (an integer atomicXor in LDS) at the last cell below the crossing.  "An odd
//      number of crossings above cell k" is then the suffix parity of the column's bits.
//   C  every thread takes columns again: suffix parity of the bit words from the top, masked by [ka, kb), popcount.
// The bit words of a tile are laid out word-major (word w of all columns side by side), so phase C reads without bank conflicts.
// LDS: 12 (V + L) + 16 KB of bit words (the box's and the depth's reduction columns borrow them first) + 8 KB of ranges: 33 KB at
// MANO's 779 vertices (four workgroups per CU), 49 KB at the largest hand.
#include "dvq_internal.h"
#include "grasp_raster.h"

namespace {

constexpr int GV_MAX_P = 8192;
static_assert(7 * GV_THREADS <= GV_MASK_WORDS, "the box's and the depth's reduction columns borrow the bit words");

__host__ __device__ constexpr size_t gv_lds_bytes(int V, int L) {
    return (size_t)(3 * gv_vp(V, L) + GV_MASK_WORDS + GV_MAX_COLS + GV_SMALL) * 4;
}

__global__ __launch_bounds__(GV_THREADS) void grasp_volume_kernel(const float* __restrict__ hand, int V, const int32_t* __restrict__ faces,
                                                                  int F, const int32_t* __restrict__ loop_off,
                                                                  const int32_t* __restrict__ loop_vert, int L, int n_loop,
                                                                  const float* __restrict__ planes, int n_planes,
                                                                  const int32_t* __restrict__ plane_off, long O, const int64_t* __restrict__ obj_of_row,
                                                                  const float* __restrict__ R, const float* __restrict__ tr, float h,
                                                                  int32_t* __restrict__ count, float* __restrict__ depth,
                                                                  int32_t* __restrict__ status, int32_t* err_flag) {
    extern __shared__ __align__(16) float gv_lds[];
    const int VT = V + L, VP = gv_vp(V, L);
    float* vx = gv_lds;
    float* vy = vx + VP;
    float* vz = vy + VP;
    unsigned* mask = reinterpret_cast<unsigned*>(vz + VP);                 // [GV_MASK_WORDS]
    int* range = reinterpret_cast<int*>(mask + GV_MASK_WORDS);             // [GV_MAX_COLS]: ka | kb << 16
    float* red = reinterpret_cast<float*>(mask);                           // [7][256]: box and depth columns, before the first tile
    int* small = range + GV_MAX_COLS;                                      // 0: not finite, 1: count, 2 .. 4: a tile has a hull column
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const float nanf_ = __builtin_nanf("");

    const int64_t o = obj_of_row[b];
    int p0 = 0, P = -1;
    if (o >= 0 && o < O) {
        p0 = plane_off[o];
        P = plane_off[o + 1] - p0;
    }
    if (P < 0 || P > GV_MAX_P || p0 < 0 || p0 > n_planes - P) {                                 // uniform over the workgroup
        if (t == 0) {
            atomicOr(err_flag, (o >= 0 && o < O) ? 2 : 1);
            count[b] = -1;
            depth[b] = nanf_;
            status[b] = 4;
        }
        return;
    }
    const f32x4* pl = reinterpret_cast<const f32x4*>(planes) + p0;

    if (t < GV_SMALL) small[t] = 0;
    dvq_lds_barrier();
    if (grasp_load_hand(hand + b * V * 3, V, t, vx, vy, vz)) small[0] = 1;    // the hand as given, and whether it is finite
    dvq_lds_barrier();
    if (small[0]) {
        if (t == 0) {
            count[b] = -1;
            depth[b] = nanf_;
            status[b] = 3;
        }
        return;
    }
    if (t < L) gv_fan_centre(t, loop_off, loop_vert, n_loop, V, vx, vy, vz, err_flag);   // in the row's frame
    dvq_lds_barrier();
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    gv_object_frame(t, b, VT, R, tr, vx, vy, vz, mn, mx);                 // each vertex by its owner
    dvq_lds_barrier();                                                     // every vertex is in place
    float deep = 0.0f;                                                     // depth: thread t's vertices against every plane
    for (int i = t; i < V; i += GV_THREADS) {
        const float x = vx[i], y = vy[i], z = vz[i];
        float g = INFINITY;
        for (int p = 0; p < P; ++p) {
            const f32x4 q = pl[p];
            const float e = q[3] - fmaf(q[2], z, fmaf(q[1], y, q[0] * x));
            g = e < g ? e : g;
        }
        deep = g > deep ? g : deep;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        red[c * GV_THREADS + t] = mn[c];
        red[(3 + c) * GV_THREADS + t] = mx[c];
    }
    red[6 * GV_THREADS + t] = deep;
    dvq_lds_barrier();
    for (int s = GV_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            gv_reduce_extent(red, t, s);
            const float d = red[6 * GV_THREADS + t], d2 = red[6 * GV_THREADS + t + s];
            red[6 * GV_THREADS + t] = d2 > d ? d2 : d;
        }
        dvq_lds_barrier();
    }
    deep = red[6 * GV_THREADS];
    if (P == 0) {
        if (t == 0) {
            count[b] = 0;
            depth[b] = 0.0f;
            status[b] = 1;
        }
        return;
    }
    int lo[3], n[3];
    const bool fits = gv_box(red, h, lo, n);
    if (!fits) {
        if (t == 0) {
            count[b] = -1;
            depth[b] = deep;
            status[b] = 2;
        }
        return;
    }
    const int nx = n[0], ny = n[1], nk = n[2], ilo = lo[0], jlo = lo[1], klo = lo[2];
    const GvTiles tiles = gv_tiles(nx, ny, nk);
    const int W = tiles.W, TX = tiles.TX, TY = tiles.TY;
    const float zbot = gv_c(klo, h), ztop = gv_c(klo + nk - 1, h);
    int mine = 0, hull_seen = 0, tile = 0;
    gv_check_faces(t, faces, F, VT, err_flag);
    for (int ty0 = 0; ty0 < ny; ty0 += TY) {
        for (int tx0 = 0; tx0 < nx; tx0 += TX, ++tile) {
            const int tw = nx - tx0 < TX ? nx - tx0 : TX, th = ny - ty0 < TY ? ny - ty0 : TY;
            const int ncol = tw * th;
            int* flag = small + 2 + tile % 3;
            if (t == 0) small[2 + (tile + 1) % 3] = 0;                    // the next tile's flag: last read two barriers ago
            // H: the cells of every column inside the hull
            bool any = false;
            for (int c = t; c < ncol; c += GV_THREADS) {
                const float x = gv_c(ilo + tx0 + c % tw, h), y = gv_c(jlo + ty0 + c / tw, h);
                float zlo = -INFINITY, zhi = INFINITY;
                bool in = true;
                for (int p = 0; p < P && in; ++p) {
                    const f32x4 q = pl[p];
                    const float s = q[0] * x + q[1] * y;
                    const float r = q[3] - s;
                    if (q[2] < 0.0f) {
                        const float z = r / q[2];
                        zlo = z > zlo ? z : zlo;
                    } else if (q[2] > 0.0f) {
                        const float z = r / q[2];
                        zhi = z < zhi ? z : zhi;
                    } else {
                        in = s <= q[3];
                    }
                    in = in && zlo <= zhi && zlo <= ztop && zbot <= zhi;  // (an interval that misses the box holds no cell of it)
                }
                int ka = 0, kb = 0;
                if (in) {
                    ka = gv_cells<true>(zlo, h, klo, nk);                 // cells below zlo are out
                    kb = gv_cells<false>(zhi, h, klo, nk);                // cells up to zhi are in
                    if (kb <= ka) ka = kb = 0;
                }
                range[c] = ka | (kb << 16);
                any |= kb > ka;
            }
            if (any) *flag = 1;
            dvq_lds_barrier();
            const bool live = *flag != 0;
            if (!live) continue;                                           // uniform: no column of the tile meets the hull
            hull_seen = 1;
            for (int i = t; i < ncol * W; i += GV_THREADS) mask[i] = 0u;
            dvq_lds_barrier();
            // R: every triangle toggles one bit in each column it covers
            gv_raster_hand(t, faces, F, VT, vx, vy, vz, h, ilo + tx0, ilo + tx0 + tw - 1, jlo + ty0, jlo + ty0 + th - 1, klo, nk, mask,
                           [&](int col) { return range[col] != 0; });     // (a column without a cell in the hull takes no bit)
            dvq_lds_barrier();
            // C: suffix parity from the top word down, cut to the hull's cells
            for (int c = t; c < ncol; c += GV_THREADS) {
                const int rg = range[c];
                if (rg == 0) continue;
                const int ka = rg & 0xffff, kb = rg >> 16;
                unsigned carry = 0u;
                for (int w = W - 1; w >= (ka >> 5); --w) {
                    const unsigned v = mask[w * ncol + c];
                    unsigned s = gv_suffix_parity(v);                      // bit i = parity of the bits i .. 31
                    s ^= carry;
                    carry ^= (__popc(v) & 1) ? 0xffffffffu : 0u;
                    const int base = w << 5;
                    if (base >= kb) continue;
                    unsigned keep = 0xffffffffu;
                    if (ka > base) keep &= 0xffffffffu << (ka - base);
                    if (kb < base + 32) keep &= 0xffffffffu >> (base + 32 - kb);
                    mine += __popc(s & keep);
                }
            }
            dvq_lds_barrier();                                             // the next tile rewrites ranges and bit words
        }
    }
    if (mine) atomicAdd(&small[1], mine);
    dvq_lds_barrier();
    if (t == 0) {
        count[b] = hull_seen ? small[1] : 0;
        depth[b] = hull_seen ? deep : 0.0f;
        status[b] = hull_seen ? 0 : 1;
    }
}

}  // namespace

extern "C" int dvq_grasp_volume(const float* hand, int V, const int32_t* faces, int F, const int32_t* loop_off, const int32_t* loop_vert,
                                int L, int n_loop, const float* planes, int n_planes, const int32_t* plane_off, int64_t O, const int64_t* obj_of_row, const float* R,
                                const float* t, int64_t B, float h, int32_t* count, float* depth, int32_t* status, int32_t* err_flag,
                                dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && V >= 1 && V <= GV_MAX_V && F >= 0 && F <= GV_MAX_F && L >= 0 && L <= GV_MAX_L && O >= 0 && n_loop >= 0 && n_planes >= 0,
                "grasp_volume: need B >= 0, 1 <= V <= %d, 0 <= F <= %d, 0 <= L <= %d, O >= 0 (got B=%ld V=%d F=%d L=%d O=%ld)", GV_MAX_V,
                GV_MAX_F, GV_MAX_L, (long)B, V, F, L, (long)O);
    DVQ_REQUIRE(h > 0.0f && h < INFINITY, "grasp_volume: the lattice spacing must be finite and positive (got %g)", (double)h);
    DVQ_REQUIRE(R || !t, "grasp_volume: t without R");
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && (faces || F == 0) && loop_off && (loop_vert || n_loop == 0) && (planes || n_planes == 0) && plane_off && obj_of_row && count && depth &&
                    status && err_flag,
                "grasp_volume: null pointer");
    DVQ_REQUIRE((reinterpret_cast<uintptr_t>(planes) & 15) == 0, "grasp_volume: planes must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = gv_lds_bytes(V, L);                                 // <= 49 KB: below the default limit, no attribute to set
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // the work depends on the data (the box, the hull's planes, how much of the box the hull meets): only the depth's part is
        // known here, 8 FLOPs per (vertex, plane) pair with the plane count unknown to the host -- reported as 0 FLOPs.  in: the hand;
        // out: 12 B per grasp
        DVQ_PROF("grasp_volume", 0.0, (double)nb * ((double)V * 12 + 12), st);
        DVQ_LAUNCH(grasp_volume_kernel, dim3((unsigned)nb), dim3(GV_THREADS), lds, st, hand + b0 * V * 3, V, faces, F, loop_off, loop_vert,
                   L, n_loop, planes, n_planes, plane_off, (long)O, obj_of_row + b0, R ? R + b0 * 9 : nullptr, t, h, count + b0, depth + b0, status + b0,
                   err_flag);
    });
    DVQ_CHECK_LAUNCH("grasp_volume");
    return DVQ_OK;
}
