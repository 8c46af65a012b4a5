// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fmaf chain)
// with the path's epilogues fused: bias/ReLU, residual, gated activation (tanh*sigmoid over
// gate-packed channel pairs + class-conditional bias), and the PointNet per-tile column max.
//
//   C[M,N] = sum_s A_s[M,K_s] * W_s[N,K_s]^T          (both operands K-contiguous, like nn.Linear)
//
// Tile: 128x128x32 per 256-thread workgroup (4 waves as 2(M) x 2(N), each 64x64 = 2x2 MFMA tiles),
// LDS rows padded to 36 floats (ds_read_b128 conflict-free: 36*m mod 64 distinct over a lane group),
// global->register->LDS double buffering (one barrier per K-tile), 2 workgroups per CU.
// Accumulation order is canonical: for every output, k runs 0,1,2,... across all sources in order
// (lane half h feeds k = 2t+h at MFMA step t), so results do not depend on the tiling.
// Block -> tile map is XCD-aware: the column tiles of one 128-row panel run on one XCD (blocks b and
// b+8 share an XCD), so the A panel is fetched into one L2 only.
#include "dvq_internal.h"
#include "gemm_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 32, LDT = BK + 4;
constexpr int TILE_FLOATS = (BM + BN) * LDT;            // one stage: A tile + W tile
constexpr size_t SMEM_BYTES = 2 * TILE_FLOATS * sizeof(float);

struct TileRegs {
    f32x4 a[4];
    f32x4 w[4];
};

__device__ __forceinline__ void load_tile(const GemmParams& p, int s, int k0, long m0, int n0, int tid,
                                          TileRegs& t) {
    const GemmSrc& src = p.src[s];
    const int c4 = tid & 7;
    const int r0 = tid >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + 32 * i;
        const long m = m0 + row;
        t.a[i] = (m < p.M) ? *reinterpret_cast<const f32x4*>(src.A + m * src.lda + k0 + c4 * 4)
                           : f32x4{0.f, 0.f, 0.f, 0.f};
        const int n = n0 + row;
        t.w[i] = (n < p.N) ? *reinterpret_cast<const f32x4*>(src.W + (long)n * src.ldw + k0 + c4 * 4)
                           : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

__device__ __forceinline__ void store_tile(float* stage, int tid, const TileRegs& t) {
    const int c4 = tid & 7;
    const int r0 = tid >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + 32 * i;
        *reinterpret_cast<f32x4*>(stage + row * LDT + c4 * 4) = t.a[i];
        *reinterpret_cast<f32x4*>(stage + (BM + row) * LDT + c4 * 4) = t.w[i];
    }
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles_n = (p.N + BN - 1) / BN;
    const long tiles_m = (p.M + BM - 1) / BM;
    // XCD-aware map: panel (m-tile) index = 8 * (j / tiles_n) + (b % 8).  With fewer than eight row panels (round 6: the VQ argmin's
    // K / 128 = 1 .. 4 codebook panels against thousands of column tiles of z rows) that map leaves 8 - tiles_m of the eight XCDs
    // without work -- the exact argmin took 410 us per 65 536 rows whether K was 128 or 512 --: there the COLUMN tiles are dealt over
    // the XCDs instead and the few row panels of one column tile follow each other on one XCD (its z rows are fetched into one L2).
    const long b = blockIdx.x;
    const long j = b >> 3;
    long mt;
    int nt;
    if (tiles_m < 8) {
        mt = j % tiles_m;
        nt = (int)((j / tiles_m) * 8 + (b & 7));
        if (nt >= tiles_n) return;
    } else {
        mt = (j / tiles_n) * 8 + (b & 7);
        nt = (int)(j % tiles_n);
        if (mt >= tiles_m) return;
    }
    const long m0 = mt * BM;
    const int n0 = nt * BN;

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jn][e] = 0.f;

    // flattened (source, k-tile) iteration
    int s = 0, k0 = 0;
    TileRegs regs;
    load_tile(p, 0, 0, m0, n0, tid, regs);
    store_tile(smem, tid, regs);
    __syncthreads();
    int stage = 0;
    while (true) {
        // advance to the next (source, k-tile)
        int s_next = s, k_next = k0 + BK;
        if (k_next >= p.src[s].K) { s_next = s + 1; k_next = 0; }
        const bool has_next = s_next < p.nsrc;
        if (has_next) load_tile(p, s_next, k_next, m0, n0, tid, regs);

        const float* As = smem + stage * TILE_FLOATS + (wm * 64 + r) * LDT;
        const float* Ws = smem + stage * TILE_FLOATS + (BM + wn * 64 + r) * LDT;
#pragma unroll
        for (int u = 0; u < BK / 4; ++u) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(As + 4 * u);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(As + 32 * LDT + 4 * u);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(Ws + 4 * u);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(Ws + 32 * LDT + 4 * u);
            // MFMA step t consumes k = 2t + h: lane half 0 takes the even element, half 1 the odd one
            const float a0e = h ? a0[1] : a0[0], a0o = h ? a0[3] : a0[2];
            const float a1e = h ? a1[1] : a1[0], a1o = h ? a1[3] : a1[2];
            const float w0e = h ? w0[1] : w0[0], w0o = h ? w0[3] : w0[2];
            const float w1e = h ? w1[1] : w1[0], w1o = h ? w1[3] : w1[2];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0e, w0e, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0e, w1e, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1e, w0e, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1e, w1e, acc[1][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0o, w0o, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0o, w1o, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1o, w0o, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1o, w1o, acc[1][1], 0, 0, 0);
        }
        if (!has_next) break;
        store_tile(smem + (stage ^ 1) * TILE_FLOATS, tid, regs);
        __syncthreads();
        stage ^= 1;
        s = s_next;
        k0 = k_next;
    }

    gemm_epilogue<EPI>(p, acc, m0, n0, mt, nt, tid, smem);
}

// workgroups of gemm_f32_kernel's two block -> tile maps
inline long f32_grid(long tiles_m, long tiles_n) { return tiles_m < 8 ? tiles_m * ((tiles_n + 7) / 8 * 8) : gemm_padded_grid(tiles_m, tiles_n); }

template <int EPI>
int launch(const GemmParams& p, hipStream_t stream) {
    static DvqOncePerDevice attr_once;
    DVQ_PROPAGATE(dvq_lds_limit(attr_once, reinterpret_cast<const void*>(&gemm_f32_kernel<EPI>), SMEM_BYTES, "gemm"));
    const long grid = f32_grid((p.M + BM - 1) / BM, (p.N + BN - 1) / BN);
    const double ksum = gemm_ksum(p);
    {
        DVQ_PROF(gemm_prof_name(EPI, 0), 2.0 * (double)p.M * p.N * ksum, ((double)p.M + p.N) * ksum * 4, stream);
        DVQ_LAUNCH(gemm_f32_kernel<EPI>, dim3((unsigned)grid), dim3(256), SMEM_BYTES, stream, p);
    }
    DVQ_CHECK_LAUNCH("gemm_f32");
    return DVQ_OK;
}

}  // namespace

int dvq_gemm_mode() {
    static int mode = -1;
    if (mode < 0) {
        const char* e = getenv("DVQ_GEMM");                 // "fp32": the exact fp32 chain; "bf16x3" / "f16x2" / unset: follow the weight images
        mode = (e && (e[0] == 'f' || e[0] == 'F') && (e[1] == 'p' || e[1] == 'P')) ? 0 : 1;
    }
    return mode;
}

static int check_gemm(const GemmParams& p) {
    DVQ_REQUIRE(p.nsrc >= 1 && p.nsrc <= DVQ_MAX_SRC, "gemm: nsrc=%d out of range", p.nsrc);
    DVQ_REQUIRE(p.M > 0 && p.N > 0, "gemm: empty problem M=%ld N=%d", p.M, p.N);
    // every kernel of the three files tiles 128 rows and >= 128 columns: the fp32 kernel's grid (either of its maps) and the padded
    // grid of the 128 x 128 kernels bound them all
    const long tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    DVQ_REQUIRE(f32_grid(tiles_m, tiles_n) < (1L << 31) && gemm_padded_grid(tiles_m, tiles_n) < (1L << 31), "gemm: grid too large");
    for (int s = 0; s < p.nsrc; ++s) {
        const GemmSrc& g = p.src[s];
        DVQ_REQUIRE(g.A && g.W, "gemm: null operand in source %d", s);
        DVQ_REQUIRE(g.K > 0 && g.K % BK == 0, "gemm: K=%d of source %d is not a multiple of %d", g.K, s, BK);
        DVQ_REQUIRE(dvq_aligned16(g.A) && dvq_aligned16(g.W) && g.lda % 4 == 0 && g.ldw % 4 == 0,
                    "gemm: source %d rows are not 16-byte aligned", s);
    }
    return DVQ_OK;
}

// fp16 three-product planes (the default packing): every source must carry them, with one row-scale array for the launch.
// *use = 1 when the problem runs on them (validated), 0 when no source carries them.
static int check_f16x2_planes(const GemmParams& p, GemmEpilogue epi, int* use) {
    *use = 0;
    int n16 = 0;
    for (int s = 0; s < p.nsrc; ++s) n16 += (p.src[s].Wp && p.src[s].wp_kind == DVQ_PLANES_F16X2) ? 1 : 0;
    if (!n16) return DVQ_OK;
    DVQ_REQUIRE(n16 == p.nsrc, "gemm: %d of %d sources carry fp16 planes (all or none)", n16, p.nsrc);
    DVQ_REQUIRE(p.out && (epi != EPI_RESID || p.resid), "gemm: null output/residual");
    DVQ_REQUIRE(epi != EPI_GATE || (p.N % BN == 0 && (!p.cls || p.label)), "gemm: gated epilogue needs N %% 128 == 0 (N=%d) and labels with a class bias", p.N);
    *use = 1;
    return DVQ_OK;
}

int dvq_launch_gemm_gate_group(const GemmParams* ps, int n, hipStream_t stream) {
    DVQ_REQUIRE(ps && n >= 1 && n <= DVQ_GEMM_GROUP_MAX, "gemm group: %d problems", n);
    bool one = n >= 2 && dvq_gemm_mode() == 1;
    for (int i = 0; i < n && one; ++i) {
        int use = 0;
        DVQ_PROPAGATE(check_gemm(ps[i]));
        DVQ_PROPAGATE(check_f16x2_planes(ps[i], EPI_GATE, &use));
        one = use && ps[i].M == ps[0].M && ps[i].N == ps[0].N;
    }
    if (one) {
        const int rc = dvq_launch_gemm_f16x2_gate_group(ps, n, stream);
        if (rc >= 0) return rc;
    }
    for (int i = 0; i < n; ++i) DVQ_PROPAGATE(dvq_launch_gemm(ps[i], EPI_GATE, stream));
    return DVQ_OK;
}

int dvq_launch_gemm(const GemmParams& p, GemmEpilogue epi, hipStream_t stream) {
    DVQ_PROPAGATE(check_gemm(p));
    const bool split = dvq_gemm_mode() == 1 && epi != EPI_ARGMIN;     // the exact VQ argmin stays on the fp32 chain
    if (split && (epi == EPI_BIAS || epi == EPI_RESID || epi == EPI_GATE || epi == EPI_STATE)) {
        int use = 0;
        DVQ_PROPAGATE(check_f16x2_planes(p, epi, &use));
        if (use) return dvq_launch_gemm_f16x2(p, epi, stream);
    }
    DVQ_REQUIRE(epi != EPI_STATE && !p.acc_hi, "gemm: accumulator states exist on the fp16-plane kernels only");
    // what is left runs the three-plane bf16 kernels (or, with DVQ_GEMM=fp32, ignores the images): an image of another kind -- fp16
    // planes on an epilogue the fp16 kernels do not have, an unknown kind -- would be read as three bf16 planes (wrong products,
    // the third plane past the end of a two-plane buffer)
    for (int s = 0; s < p.nsrc && split; ++s)                  // (DVQ_GEMM=fp32 reads no image at all)
        DVQ_REQUIRE(!p.src[s].Wp || p.src[s].wp_kind == DVQ_PLANES_BF16X3,
                    "gemm: source %d carries a weight image of kind %d, which epilogue %d cannot run on (bf16x3 images only)", s, p.src[s].wp_kind, (int)epi);
    for (int s = 0; s < p.nsrc; ++s) DVQ_REQUIRE(!p.src[s].arow, "gemm: row-indexed activations need the fp16-plane kernels (source %d)", s);
    switch (epi) {
        case EPI_BIAS:
            DVQ_REQUIRE(p.out, "gemm: null output");
            if (split) return dvq_launch_gemm_bf16x3(p, epi, stream);
            return launch<EPI_BIAS>(p, stream);
        case EPI_RESID:
            DVQ_REQUIRE(p.out && p.resid, "gemm: null output/residual");
            if (split) return dvq_launch_gemm_bf16x3(p, epi, stream);
            return launch<EPI_RESID>(p, stream);
        case EPI_GATE:
            DVQ_REQUIRE(p.out, "gemm: null output");
            DVQ_REQUIRE(p.N % BN == 0, "gemm: gated epilogue needs N %% 128 == 0 (N=%d)", p.N);
            DVQ_REQUIRE(!p.cls || p.label, "gemm: class bias without labels");
            if (split) return dvq_launch_gemm_bf16x3(p, epi, stream);
            return launch<EPI_GATE>(p, stream);
        case EPI_ARGMIN:
        case EPI_STATE:                                   // (fp16-plane kernels only: rejected above)
            break;
        case EPI_COLMAX:
            DVQ_REQUIRE(p.partial && p.rows_per_group > 0 && p.rows_per_group % BM == 0 && p.valid_rows > 0,
                        "gemm: bad column-max grouping");
            if (split) return dvq_launch_gemm_bf16x3(p, epi, stream);
            return launch<EPI_COLMAX>(p, stream);
    }
    if (epi == EPI_ARGMIN) {
        DVQ_REQUIRE(p.row_norm && p.col_norm && p.part_val && p.part_idx, "gemm: null argmin buffers");
        return launch<EPI_ARGMIN>(p, stream);
    }
    dvq_set_error("gemm: unknown epilogue %d", (int)epi);
    return DVQ_EINVAL;
}

extern "C" int dvq_linear(const dvq_gemm_src* src, int nsrc, int64_t M, int N, const float* bias, int act,
                          float* y, int64_t ldy, dvq_stream_t stream) {
    DVQ_REQUIRE(src && nsrc >= 1 && nsrc <= DVQ_MAX_SRC, "dvq_linear: nsrc=%d out of range", nsrc);
    DVQ_REQUIRE(act == DVQ_ACT_NONE || act == DVQ_ACT_RELU, "dvq_linear: unknown activation %d", act);
    if (M == 0) return DVQ_OK;
    GemmParams p = {};
    for (int s = 0; s < nsrc; ++s)
        DVQ_REQUIRE(!src[s].wp || src[s].wp_kind == DVQ_PLANES_BF16X3 || src[s].wp_kind == DVQ_PLANES_F16X2,
                    "dvq_linear: source %d: unknown weight-image kind %d", s, src[s].wp_kind);
    for (int s = 0; s < nsrc; ++s)
        p.src[s] = GemmSrc{src[s].x, src[s].w, (long)src[s].ldx, (long)src[s].ldw, src[s].K, src[s].wp_kind, src[s].wp, (long)src[s].wp_plane};
    for (int s = 1; s < nsrc; ++s)
        DVQ_REQUIRE(src[s].wp_kind != DVQ_PLANES_F16X2 || !src[s].wp || src[s].w_scale == src[0].w_scale,
                    "dvq_linear: the fp16 planes of one call share ONE row-scale array (source %d has another)", s);
    p.wscale = src[0].w_scale;
    p.nsrc = nsrc;
    p.M = M;
    p.N = N;
    p.bias = bias;
    p.out = y;
    p.ldo = ldy;
    p.relu = act == DVQ_ACT_RELU;
    return dvq_launch_gemm(p, EPI_BIAS, (hipStream_t)stream);
}

// Decoder / Encoder MLP (three Linear layers, ReLU after the first two: network/DVQVAE.py:145-185) as ONE entry point: the
// hidden activations live in the caller's workspace, the three GEMMs are enqueued back to back on the stream.
extern "C" size_t dvq_mlp3_workspace_bytes(int64_t M, int n0, int n1) {
    return dvq_round_up((size_t)(M > 0 ? M : 0) * (size_t)n0 * 4, 256) + dvq_round_up((size_t)(M > 0 ? M : 0) * (size_t)n1 * 4, 256) + 256;
}

extern "C" int dvq_mlp3(const float* x, int64_t ldx, int64_t M, const dvq_mlp_layer* L, float* y, int64_t ldy, void* workspace,
                        size_t workspace_bytes, dvq_stream_t stream) {
    DVQ_REQUIRE(L && M >= 0, "dvq_mlp3: bad arguments");
    if (M == 0) return DVQ_OK;
    DVQ_REQUIRE(x && y && workspace && dvq_aligned16(workspace), "dvq_mlp3: null/unaligned pointer");
    for (int i = 0; i < 3; ++i)
        DVQ_REQUIRE(!L[i].wp || L[i].wp_kind == DVQ_PLANES_BF16X3 || L[i].wp_kind == DVQ_PLANES_F16X2,
                    "dvq_mlp3: layer %d: unknown weight-image kind %d", i, L[i].wp_kind);
    DVQ_REQUIRE(L[1].k_in == L[0].n_out && L[2].k_in == L[1].n_out, "dvq_mlp3: layer sizes %d->%d, %d->%d, %d->%d do not chain", L[0].k_in,
                L[0].n_out, L[1].k_in, L[1].n_out, L[2].k_in, L[2].n_out);
    if (workspace_bytes < dvq_mlp3_workspace_bytes(M, L[0].n_out, L[1].n_out)) {
        dvq_set_error("dvq_mlp3: workspace %zu < %zu bytes", workspace_bytes, dvq_mlp3_workspace_bytes(M, L[0].n_out, L[1].n_out));
        return DVQ_EWORKSPACE;
    }
    float* h0 = (float*)workspace;
    float* h1 = (float*)((char*)workspace + dvq_round_up((size_t)M * L[0].n_out * 4, 256));
    const float* in[3] = {x, h0, h1};
    const long ldi[3] = {(long)ldx, (long)L[0].n_out, (long)L[1].n_out};
    float* out[3] = {h0, h1, y};
    const long ldo[3] = {(long)L[0].n_out, (long)L[1].n_out, (long)ldy};
    for (int i = 0; i < 3; ++i) {
        GemmParams p = {};
        p.src[0] = GemmSrc{in[i], L[i].w, ldi[i], (long)L[i].k_in, L[i].k_in, L[i].wp_kind, L[i].wp, (long)L[i].n_out * L[i].k_in};
        p.wscale = L[i].w_scale;
        p.nsrc = 1;
        p.M = M;
        p.N = L[i].n_out;
        p.bias = L[i].b;
        p.out = out[i];
        p.ldo = ldo[i];
        p.relu = i < 2;
        DVQ_PROPAGATE(dvq_launch_gemm(p, EPI_BIAS, (hipStream_t)stream));
    }
    return DVQ_OK;
}
