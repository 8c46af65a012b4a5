// dvq_grasp_parts: contact from the hand's side -- for every hand vertex its nearest object point, and from those the per-part
// minima, the per-part counts of touching vertices and a bit per vertex -- in ONE kernel, one workgroup of 256 threads per grasp.
// The definition is the ABI (include/dvq.h); this file only says how the kernel is laid out.
//
// The roles of grasp_scan.h are swapped: the CLOUD goes through LDS, in tiles of GP_TILE points as x|y|z planes (24 KB, six
// workgroups per CU, one tile at N = 1024), and every thread holds four hand vertices (t + 256 k) in registers and scans the tile
// with grasp_scan4 -- the tile as "the planes", the vertices as "the points".  The running best is merged across tiles with a
// strict <, the tile's offset added: the lowest index wins, as in nn_points_kernel.  A hand of more than 1024 vertices takes a
// second pass over the cloud.
//
// After the last tile of a pass the tile is dead: d[v] and the labels overlay it, 256 threads reduce them as 8 segments x 32
// parts, and threads 0 .. 31 fold the segments into the part's running minimum and count, which they keep in registers across
// passes.  Only minima, integer counts and bits: no float sum, so no order to fix.  The mask words come from wave ballots (the 64
// lanes of a wave hold 64 consecutive vertices: two words).
//
// The scan runs with slow = false whatever the data: a row with a non-finite coordinate has no figure and is overwritten at the
// end from a flag that the loads set (the hand is checked up front, the cloud while pass 0 loads its tiles), so by the time
// anything is written the flag is final.  No index of the scan leaves [0, tile) even on NaNs.
#include "dvq_internal.h"
#include "grasp_scan.h"

namespace {

constexpr int GP_TILE = 2048;                               // points per tile (ops.GRASP_PARTS_TILE)
constexpr int GP_SLOTS = GRASP_THREADS * GRASP_P;           // 1024 hand vertices per pass over the cloud
constexpr int GP_MAX_P = 32;                                // parts
constexpr int GP_SEGS = GRASP_THREADS / GP_MAX_P;           // 8 segments of 128 slots in the part reduction
static_assert(GP_TILE % GRASP_THREADS == 0 && GP_TILE % 4 == 0, "the planes are read sixteen bytes at a time");
static_assert(2 * GP_SLOTS + 2 * GP_SEGS * GP_MAX_P <= 3 * GP_TILE, "the reduction arrays overlay the tile");
static_assert(GP_SLOTS % 64 == 0 && GRASP_MAX_V % 32 == 0, "a wave's ballot is two whole mask words");

__global__ __launch_bounds__(GRASP_THREADS) void grasp_parts_kernel(const float* __restrict__ hand, const int* __restrict__ part_of_vertex,
                                                                    int V, int P, const float* __restrict__ obj, long osb, long osp,
                                                                    long osc, int N, float thr, float* __restrict__ part_min,
                                                                    int* __restrict__ part_count, int* __restrict__ mask,
                                                                    int* __restrict__ status, float* __restrict__ vert_dist,
                                                                    int* __restrict__ vert_idx) {
    __shared__ __align__(16) float gp_lds[3 * GP_TILE + 4];
    float* px = gp_lds;                                          // the tile: x|y|z planes
    float* py = px + GP_TILE;
    float* pz = py + GP_TILE;
    float* sd = gp_lds;                                          // [1024] d of the pass's slots: over the tile, after the scan
    int* sl = reinterpret_cast<int*>(gp_lds + GP_SLOTS);         // [1024] their labels, -1 = no part
    float* pm = gp_lds + 2 * GP_SLOTS;                           // [8][32] the segments' minima
    int* pc = reinterpret_cast<int*>(pm + GP_SEGS * GP_MAX_P);   // [8][32] the segments' counts
    int* flag = reinterpret_cast<int*>(gp_lds + 3 * GP_TILE);    // [1]: a coordinate of the row is not finite
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const float* hb = hand + b * V * 3;
    const float* ob = obj + b * osb;
    const int W = (V + 31) >> 5;
    if (t == 0) *flag = 0;
    dvq_lds_barrier();
    {
        bool odd = false;                                        // the whole hand, up front: later passes' vertices included
        for (int i = t; i < 3 * V; i += GRASP_THREADS) odd |= !(fabsf(hb[i]) < INFINITY);
        if (odd) *flag = 1;
    }
    float run_min = INFINITY;                                    // threads 0 .. 31: part t over the passes so far
    int run_cnt = 0;
    bool bad = false;
    for (int v0 = 0; v0 < V; v0 += GP_SLOTS) {                   // vertices v0 + t + 256 k: one pass over the cloud
        float vx[GRASP_P], vy[GRASP_P], vz[GRASP_P], rbest[GRASP_P];
        int ridx[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int v = v0 + t + k * GRASP_THREADS;
            const bool in = v < V;
            vx[k] = in ? hb[3 * v] : 0.f;
            vy[k] = in ? hb[3 * v + 1] : 0.f;
            vz[k] = in ? hb[3 * v + 2] : 0.f;
            rbest[k] = INFINITY;
            ridx[k] = 0;
        }
        for (long p0 = 0; p0 < N; p0 += GP_TILE) {
            const int n = N - p0 < GP_TILE ? (int)(N - p0) : GP_TILE;
            dvq_lds_barrier();                                   // every wave is through with the tile before (or the reduction arrays)
            bool odd = false;
            for (int i = t; i < n; i += GRASP_THREADS) {
                const long p = p0 + i;
                const float x = ob[p * osp], y = ob[p * osp + osc], z = ob[p * osp + 2 * osc];
                px[i] = x;
                py[i] = y;
                pz[i] = z;
                odd |= !grasp_finite(x, y, z);
            }
            if (odd) *flag = 1;
            dvq_lds_barrier();
            float best[GRASP_P];
            int bi[GRASP_P];
            grasp_scan4(px, py, pz, n, false, vx, vy, vz, best, bi);
#pragma unroll
            for (int k = 0; k < GRASP_P; ++k) {                  // strictly less: among equals the earlier tile's, the lower index
                const bool better = best[k] < rbest[k];
                rbest[k] = better ? best[k] : rbest[k];
                ridx[k] = better ? (int)p0 + bi[k] : ridx[k];
            }
        }
        dvq_lds_barrier();                                       // the last tile is dead: d and the labels go over it
        int lab[GRASP_P];
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int v = v0 + t + k * GRASP_THREADS;
            int l = v < V ? part_of_vertex[v] : -1;
            l = (l >= 0 && l < P) ? l : -1;                      // a label outside [0, P): no part
            lab[k] = l;
            sd[t + k * GRASP_THREADS] = rbest[k];
            sl[t + k * GRASP_THREADS] = l;
        }
        dvq_lds_barrier();                                       // ... and the flag is final: pass 0 has loaded every tile
        bad = *flag != 0;
#pragma unroll
        for (int k = 0; k < GRASP_P; ++k) {
            const int v = v0 + t + k * GRASP_THREADS;
            const bool in = v < V;
            const bool touch = in && !bad && rbest[k] < thr;
            const unsigned long long bits = __ballot(touch);     // the wave's 64 vertices: two mask words
            if ((t & 63) == 0) {
                const int w = (v0 + k * GRASP_THREADS + t) >> 5;
                if (w < W) mask[b * W + w] = (int)(unsigned)(bits & 0xffffffffull);
                if (w + 1 < W) mask[b * W + w + 1] = (int)(unsigned)(bits >> 32);
            }
            if (in && vert_dist) vert_dist[b * V + v] = bad ? NAN : rbest[k];
            if (in && vert_idx) vert_idx[b * V + v] = bad ? -1 : ridx[k];
        }
        {
            const int q = t & (GP_MAX_P - 1), seg = t / GP_MAX_P;   // part q over the slots of segment seg: broadcast reads
            float m = INFINITY;
            int c = 0;
            const int i0 = seg * (GP_SLOTS / GP_SEGS);
            for (int i = i0; i < i0 + GP_SLOTS / GP_SEGS; ++i) {
                const float d = sd[i];
                const bool mine = sl[i] == q;
                m = (mine && d < m) ? d : m;
                c += (mine && d < thr) ? 1 : 0;
            }
            pm[seg * GP_MAX_P + q] = m;
            pc[seg * GP_MAX_P + q] = c;
        }
        dvq_lds_barrier();
        if (t < GP_MAX_P) {
#pragma unroll
            for (int s = 0; s < GP_SEGS; ++s) {
                const float m = pm[s * GP_MAX_P + t];
                run_min = m < run_min ? m : run_min;
                run_cnt += pc[s * GP_MAX_P + t];
            }
        }
    }
    if (t < P) {
        part_min[b * P + t] = bad ? NAN : run_min;
        part_count[b * P + t] = bad ? -1 : run_cnt;
    }
    if (t == 0) status[b] = bad ? 1 : 0;
}

}  // namespace

extern "C" int dvq_grasp_parts(const float* hand, const int32_t* part_of_vertex, int V, int P, const float* obj,
                               int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride, int64_t B, int N,
                               float contact_threshold, float* part_min, int32_t* part_count, int32_t* mask, int32_t* status,
                               float* vert_dist, int32_t* vert_idx, dvq_stream_t stream) {
    DVQ_REQUIRE(B >= 0 && N >= 1 && V >= 1 && V <= GRASP_MAX_V && P >= 1 && P <= GP_MAX_P,
                "grasp_parts: need B >= 0, N >= 1, 1 <= V <= %d, 1 <= P <= %d (got B=%ld N=%d V=%d P=%d)", GRASP_MAX_V, GP_MAX_P, (long)B,
                N, V, P);
    if (B == 0) return DVQ_OK;
    DVQ_REQUIRE(hand && part_of_vertex && obj && part_min && part_count && mask && status, "grasp_parts: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t W = (V + 31) / 32;
    const double slots = (double)((V + GP_SLOTS - 1) / GP_SLOTS) * GP_SLOTS;
    dvq_for_row_chunks(B, [&](int64_t b0, int64_t nb) {
        // per (vertex slot, point) pair 8 FLOPs as in grasp_scores; in: the hand twice (the check, the registers), the cloud once per
        // pass of 1024 vertices; out: the parts, the mask and, when asked for, 8 B per vertex
        DVQ_PROF("grasp_parts", 8.0 * nb * N * slots,
                 (double)nb * (24.0 * V + 12.0 * N * (slots / GP_SLOTS) + 8.0 * P + 4.0 * W + 4 + (vert_dist ? 4.0 * V : 0) + (vert_idx ? 4.0 * V : 0)),
                 st);
        DVQ_LAUNCH(grasp_parts_kernel, dim3((unsigned)nb), dim3(GRASP_THREADS), 0, st, hand + b0 * V * 3, part_of_vertex, V, P,
                   obj + b0 * obj_batch_stride, (long)obj_batch_stride, (long)obj_point_stride, (long)obj_coord_stride, N,
                   contact_threshold, part_min + b0 * P, part_count + b0 * P, mask + b0 * W, status + b0,
                   vert_dist ? vert_dist + b0 * V : nullptr, vert_idx ? vert_idx + b0 * V : nullptr);
    });
    DVQ_CHECK_LAUNCH("grasp_parts");
    return DVQ_OK;
}
