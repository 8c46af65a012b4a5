/*
 * dvq.h -- C ABI of libdvq_hip.so: the MI355X (gfx950) implementation of the D-VQVAE batched
 * grasp-generation hot path (reference: network/gen_net.py:78-125, `GenNet.gen`).
 *
 * The reference is pure Python/PyTorch and has NO FFI/plugin layer: its "operator
 * interface" for this path is the set of nn.Module methods cited on each entry point below.  These
 * entry points are what a ctypes binding added to the reference would call (INTEGRATION.md shows the
 * stub); the host-side mirror in d-vqvae_amd/network/ is exactly such a binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP global memory) unless the name ends in _host;
 *   - tensors are dense row-major fp32 / int64 exactly as the reference holds them;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises,
 *     nothing allocates: scratch comes from the caller (`*_workspace_bytes` tells how much);
 *   - return value: 0 = DVQ_OK, otherwise a dvq_status; dvq_last_error() gives the text
 *     (thread-local).  Invalid shapes/alignments are rejected (never silently clamped).
 *   - out-of-range code indices (>= K) are reported through a device-side error flag that the host
 *     mirror turns into the reference's RuntimeError (quantizer.py:72 scatter_ bounds).
 */
#ifndef DVQ_H
#define DVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dvq_stream_t; /* hipStream_t */

typedef enum {
    DVQ_OK = 0,
    DVQ_EINVAL = 1,   /* bad shape / alignment / null pointer */
    DVQ_EWORKSPACE = 2, /* workspace too small */
    DVQ_ELAUNCH = 3,  /* HIP launch error */
    DVQ_ENODEVICE = 4
} dvq_status;

/* The version of this header.  dvq_abi_version() returns the library's: a binding checks the two for equality at load time
 * (struct layouts change between versions). */
#define DVQ_ABI_VERSION 10
/* Entry points added since 10 without touching a struct or a signature of it (a compatible extension: bindings of 10 keep
 * working, the version stays): dvq_pixelcnn_sample_ctl, dvq_grasp_scores, dvq_segment_topk, dvq_segment_diverse,
 * dvq_grasp_refine, dvq_segment_kmeans, dvq_grasp_wrench, dvq_grasp_volume, dvq_grasp_parts, dvq_grasp_refine_rigid,
 * dvq_grasp_refine_fingers, dvq_grasp_self, dvq_mano_backward_workspace_bytes, dvq_mano_backward, dvq_grasp_ttt,
 * dvq_pixelcnn_beam_workspace_bytes, dvq_pixelcnn_beam, dvq_grasp_mesh, dvq_segment_contact, dvq_mesh_sample, dvq_cloud_fps,
 * dvq_grasp_mesh_volume, dvq_grasp_closure. */
int dvq_abi_version(void);
const char* dvq_last_error(void);
/* number of visible HIP devices, or -1; does not create a context */
int dvq_device_count(void);
/* The library reads its environment knobs (tile/chunk choices and the PointNet test switches DVQ_PN_FILTER / _EXHAUSTIVE /
 * _CAPS: none changes a result) ONCE, at first use; this re-reads them (tests that flip a knob in-process call it). */
int dvq_reload_env(void);

/* ------------------------------------------------------------------ generic dense layer (MFMA fp32)
 * y[M,N] = act( sum_s x_s[M,K_s] @ w_s[N,K_s]^T + bias[N] ) -- nn.Linear / 1x1 conv / conv taps.
 * Replaces: Decoder.forward (network/DVQVAE.py:183-185), STN3d fc1..fc3 (pointnet_encoder.py:35-37),
 * Encoder.forward (DVQVAE.py:161-166).  K_s % 32 == 0, 16-byte aligned rows.
 * Arithmetic: fp32 operands on the 16-bit matrix cores, fp32 accumulation, fp32-GEMM-class accuracy (<= 4e-6 * sum|x w| against
 * fp64, measured ~1e-7).  What runs follows the weight image handed over in `wp`:
 *   DVQ_PLANES_F16X2  (dvq_split_f16x2; what the host mirror packs by default): w * 2^t[n] (one power of two per output row) as
 *       two fp16 planes, the second holding the remainder * 2^11; activations are split the same way while they are staged;
 *       THREE products per fp32 product in two accumulators: out = (x1 w1 + (x1 w2 + x2 w1) * 2^-11) * 2^-t[n].  |x| < 65 520
 *       (fp16 range): a row beyond it comes out NaN, never silently wrong.
 *   DVQ_PLANES_BF16X3 (dvq_split_bf16x3), or no image at all (split on the fly): every operand split EXACTLY into three bf16
 *       pieces, the six partial products of weight >= 2^-24: fp32's range, twice the matrix work.
 * DVQ_GEMM=fp32 in the environment ignores the images and runs v_mfma_f32_32x32x2_f32 (exact fp32 chain). */
#define DVQ_PLANES_BF16X3 0
#define DVQ_PLANES_F16X2 1
typedef struct {
    const float* x; /* [M, K] row stride ldx */
    const float* w; /* [N, K] row stride ldw */
    int64_t ldx, ldw;
    int32_t K;
    int32_t wp_kind;    /* DVQ_PLANES_* of `wp` */
    const uint16_t* wp; /* optional: w pre-split into planes [3 or 2][N][ldw]; DVQ_PLANES_F16X2: the OPAQUE image of dvq_split_f16x2,
                           whole [N][K] blocks only (ldw == K) */
    int64_t wp_plane;   /* elements between planes */
    const float* w_scale; /* DVQ_PLANES_F16X2: [N] row scales 2^-t[n] (dvq_split_f16x2); ONE array for all sources of a call */
} dvq_gemm_src;

#define DVQ_MAX_SRC 8
#define DVQ_ACT_NONE 0
#define DVQ_ACT_RELU 1

int dvq_linear(const dvq_gemm_src* src_host, int nsrc, int64_t M, int N, const float* bias,
               int act, float* y, int64_t ldy, dvq_stream_t stream);
/* Decoder.forward / Encoder.forward (network/DVQVAE.py:161-166, 183-185): Linear + ReLU, Linear + ReLU, Linear as one entry
 * point (SURVEY.md 8b `mlp3`): 2560 -> 1024 -> 256 -> 55, 2048 -> 1024 -> 128 -> 6, 1024 -> 1024 -> 512 -> 256.  Weights [n_out, k_in]
 * dense row-major (nn.Linear's layout), `wp` optional pre-split planes (dvq_split_bf16x3); hidden sizes % 32 == 0. */
typedef struct {
    const float* w;      /* [n_out, k_in] */
    const float* b;      /* [n_out] or NULL */
    const uint16_t* wp;  /* optional planes [3 or 2][n_out][k_in] */
    int32_t n_out, k_in;
    const float* w_scale; /* DVQ_PLANES_F16X2: [n_out] */
    int32_t wp_kind;     /* DVQ_PLANES_* */
    int32_t _pad;
} dvq_mlp_layer;
size_t dvq_mlp3_workspace_bytes(int64_t M, int n0, int n1);
int dvq_mlp3(const float* x, int64_t ldx, int64_t M, const dvq_mlp_layer* layers_host /* [3] */, float* y, int64_t ldy,
             void* workspace, size_t workspace_bytes, dvq_stream_t stream);
/* planes[p][i] (p = 0,1,2; bf16 bit patterns) with w[i] == planes[0][i] + planes[1][i] + planes[2][i] exactly */
int dvq_split_bf16x3(const float* w, int64_t n, uint16_t* planes, dvq_stream_t stream);
/* The fp16 image of a weight tensor w [outer][N][K] (dense; outer = conv taps, 1 for nn.Linear), N = output rows:
 *   dvq_f16x2_row_absmax: row_absmax[n] = max(row_absmax[n], max_{o,k} |w[o][n][k]|)  -- the caller zeroes row_absmax [N] and
 *       calls this once per tensor whose products are summed into the same outputs (all taps of a conv; horiz_stack and
 *       vert_to_horiz of a gated layer, models.py:76-81);
 *   dvq_split_f16x2: t[n] = largest power of two with row_absmax[n] * 2^t < 2^15; planes[0] = fp16(w * 2^t[n]),
 *       planes[1] = fp16((w * 2^t[n] - planes[0]) * 2^11), both [outer][N][K]; row_scale[n] = 2^-t[n].
 *       The image is OPAQUE and made by this call only: a plane keeps the size and the [outer] blocks of w (block o starts at
 *       o * N * K, the planes lie outer * N * K apart), but inside a block the elements stand in K-TILE ORDER, the order the GEMM
 *       kernels read them in -- element (n, k) at (k / 32) * N * 32 + n * 32 + k % 32: the 32 k of a row that one K-tile
 *       multiplies are 64 contiguous bytes, and the rows of a K-tile follow each other, so sixteen rows are eight whole 128-byte
 *       lines.  (A K that is no multiple of 32 keeps the natural [N][K] order; no kernel takes such an image: K_s % 32 == 0.)
 *       A GEMM source hands over a whole block: wp = planes + o * N * K, wp_plane = outer * N * K, ldw = K. */
int dvq_f16x2_row_absmax(const float* w, int64_t outer, int N, int K, float* row_absmax, dvq_stream_t stream);
int dvq_split_f16x2(const float* w, int64_t outer, int N, int K, const float* row_absmax, uint16_t* planes /* [2][outer][N][K] */,
                    float* row_scale /* [N] */, dvq_stream_t stream);

/* ------------------------------------------------------------------ VQ codebook nearest neighbour
 * VectorQuantizer.forward(z, istrain=False), network/vqvae/quantizer.py:46-49:
 *   d[m,k] = (sum_j z[m,j]^2 + sum_j E[k,j]^2) - 2 * sum_j z[m,j] E[k,j];  idx[m] = argmin_k d[m,k]
 * evaluated in fp32 in that association, every sum a k-ordered fmaf chain (the "canonical order",
 * oracle/vq_canonical.c); first minimum wins, a NaN distance wins over everything (torch.argmin).
 * dvq_vq_argmin is the exact fp32 kernel for any K and D % 32 == 0 (fp32 MFMA, canonical order).
 * workspace: dvq_vq_argmin_workspace_bytes(M, K). dmin (optional, [M]) receives the winning distance. */
size_t dvq_vq_argmin_workspace_bytes(int64_t M, int K);
int dvq_vq_argmin(const float* z, int64_t ldz, const float* E, int64_t M, int K, int D,
                  int64_t* idx, float* dmin, void* workspace, size_t workspace_bytes,
                  dvq_stream_t stream);

/* Fast path for the headline shape (K = 512, D = 256, dense z) and, since round 6, for codebooks of K = 32, 64 ... 480 entries at
 * D = 256 (the model's six K = 128 codebooks: the image is padded to 512 entries that never win): returns the SAME indices as
 * dvq_vq_argmin, bit for bit.  One persistent kernel (one workgroup per CU, the fp16 codebook image held in registers): z is read from
 * HBM once and streamed under an fp16-MFMA filter with a proven error bound that keeps every row's candidate entries (the
 * exact fp32 argmin is always among them); rows with one candidate are decided, the rest are re-evaluated in the
 * canonical fp32 order inside the same workgroup (DESIGN.md "vq_argmin").  `packed` is the codebook image built once
 * per codebook by dvq_vq_pack (fp16 image of -2 sE E in MFMA-fragment order, canonical |e_k|^2, max |e_k|, measured
 * rounding error).  Rows are not rescaled: fp16 overflow (|z_j| > 65504), NaN/Inf rows and codebooks with magnitudes
 * outside 2^+-40 take the all-entries path.
 * `slow_rows` (device, may be NULL, never reset by the library): the kernel adds the number of rows that cost far more
 * than a filtered row: all-entries scans and rows with 32 or more candidate pairs.  A caller that sees a large fraction
 * there (ill-conditioned input: |z| >> codebook spread) should use dvq_vq_argmin instead. */
int dvq_vq_fast_supported(int K, int D);
size_t dvq_vq_pack_bytes(int K, int D);
int dvq_vq_pack(const float* E, int K, int D, void* packed, size_t packed_bytes, dvq_stream_t stream);
size_t dvq_vq_fast_workspace_bytes(int64_t M, int K, int D);
int dvq_vq_argmin_fast(const float* z, const float* E, const void* packed, int64_t M, int K, int D,
                       int64_t* idx, unsigned long long* slow_rows, void* workspace, size_t workspace_bytes,
                       dvq_stream_t stream);

/* VectorQuantizer.get_emb / one-hot @ E (quantizer.py:50-53,68-75): out[m, :] = E[idx[m], :].
 * *err_flag (device int32, caller zeroes it) is set to 1 if any idx is outside [0,K). */
int dvq_vq_lookup(const float* E, const int64_t* idx, int64_t idx_stride, int64_t M, int K, int D,
                  float* out, int64_t ldo, int32_t* err_flag, dvq_stream_t stream);

/* ------------------------------------------------------------------ PointNet encoder
 * PointNetEncoder.forward (global_feat=True, feature_transform=False), pointnet_encoder.py:140-169
 * with STN3d.forward :27-45.  BatchNorm (eval) is folded into the preceding conv/fc by the host
 * packer in fp64; fc3's bias has the 3x3 identity folded in. */
typedef struct {
    int32_t C; /* 3 or 4 input channels */
    int32_t _pad;
    /* STN trunk */
    const float *s_w1, *s_b1; /* [64,4]  (C padded to 4 with zeros) */
    const float *s_w2, *s_b2; /* [128,64] */
    const float *s_w3, *s_b3; /* [1024,128] */
    const float *s_f1, *s_c1; /* [512,1024] */
    const float *s_f2, *s_c2; /* [256,512] */
    const float *s_f3, *s_c3; /* [9,256], bias + identity */
    /* main trunk */
    const float *w1, *b1;     /* [64,4] */
    const float *w2, *b2;     /* [128,64] */
    const float *w3, *b3;     /* [1024,128] */
    /* optional split-bf16 planes ([3][out][in], dvq_split_bf16x3) of the GEMM weights; all-or-nothing */
    const uint16_t *s_w2p, *s_w3p, *s_f1p, *s_f2p, *s_f3p, *w2p, *w3p;
    /* optional filter images of a trunk's conv2 / conv3 weights (dvq_pointnet_pack_filter); with them (and the planes) the trunk
     * runs conv3 + max as an fp16 matrix-core filter followed by an exact fp32 re-evaluation of the candidate points */
    const void *s_w3f, *w3f;
} dvq_pointnet_weights;

/* Run-time consistency counters of the filtered trunk on the current device (v8): out[0] = tile records the trunk kernel marked
 * suspect (an input of its merge was stale), out[1] = channels whose exact maximum lay outside the interval their tile records
 * promised.  Both kinds are re-evaluated over all the points concerned (the features stay right); a non-zero count means the
 * filter's bookkeeping failed and should be reported.  Synchronises the device.  reset != 0: zero them after reading. */
int dvq_pointnet_fault_counters(uint64_t* out /* [2] */, int reset);
/* Filter image of one trunk (device pointers; dvq_pointnet_filter_bytes() bytes): conv3's weights w3 [1024,128] as fp16 rows scaled by
 * a per-row power of two in the k order the trunk kernel consumes, the inverse scales and the row norms; and (v8) conv2's weights
 * w2 [128,64] (BatchNorm folded) as the two fp16 planes of the three-product split of dvq_split_f16x2 with their row scales:
 * the filtered trunk multiplies conv2 on them (six bf16 products per fp32 product before). */
size_t dvq_pointnet_filter_bytes(void);
int dvq_pointnet_pack_filter(const float* w2, const float* w3, void* image, dvq_stream_t stream);

size_t dvq_pointnet_workspace_bytes(int64_t B, int N);
/* pc [B,C,N] (channel-major per sample, as the datasets emit it) -> feat [B,1024], trans [B,3,3] */
int dvq_pointnet_encode(const dvq_pointnet_weights* w_host, const float* pc, int64_t B, int N,
                        float* feat, int64_t ld_feat, float* trans /* optional */,
                        void* workspace, size_t workspace_bytes, dvq_stream_t stream);

/* ------------------------------------------------------------------ gated PixelCNN prior sampler
 * GatedPixelCNN.generate (network/pixelcnn/models.py:176-198) on the 3x3 latent grid, as an
 * incremental (cached) sampler: the network is exactly causal, so each grid position is evaluated
 * once (1/9 of the reference's FLOPs, identical math).  The draw at each position is
 * argmax_k softmax(logits)_k / q_k with q ~ Exp(1) supplied by the caller -- the exponential race
 * torch.multinomial(1) evaluates (models.py:195).  Packed layout: d-vqvae_amd/packing.py. */
typedef struct {
    const float* wv;   /* vertical taps   [n_vtaps][2*dim (gate-packed)][dim]            */
    const float* bv;   /* [2*dim] gate-packed                                              */
    const float* wh;   /* horizontal taps [n_htaps][2*dim (gate-packed)][dim]              */
    const float* wv2h; /* [2*dim (gate-packed)][2*dim (gate-packed input order)]           */
    const float* bh;   /* horiz_stack.bias + vert_to_horiz.bias, gate-packed               */
    const float* cls;  /* class_cond_embedding [n_classes][2*dim] gate-packed              */
    const float* wr;   /* horiz_resid [dim][dim]                                           */
    const float* br;   /* [dim]                                                            */
    /* optional weight images of the whole tensors (kind: dvq_pixelcnn_weights.planes_kind): [3 or 2][n_taps][2*dim][dim] for wv / wh */
    const uint16_t *wv_p, *wh_p, *wv2h_p, *wr_p;
    /* DVQ_PLANES_F16X2: row scales of the three GEMMs of a layer: vertical [2*dim], horizontal [2*dim] (wh and wv2h are summed
     * into the same outputs: their images share one absmax), residual [dim] */
    const float *sv, *sh, *sr;
} dvq_pixelcnn_layer;

typedef struct {
    int32_t n_layers, dim, n_in /* tokens */, n_classes, n_hidden /* 2048 */;
    int32_t planes_kind;        /* DVQ_PLANES_* of every *_p image below and in the layers */
    const float* tok_emb;       /* embedding.weight [n_in][dim] */
    const dvq_pixelcnn_layer* layers_host; /* host array [n_layers]; layer 0: mask A applied, k=5 */
    const float *w0, *b0;       /* output_conv.0 [n_hidden][dim] */
    const float *w2, *b2;       /* output_conv.2 [n_in][n_hidden] */
    const uint16_t *w0_p, *w2_p; /* optional weight images */
    const float *s0, *s2;        /* DVQ_PLANES_F16X2: their row scales [n_hidden], [n_in] */
    /* optional (DVQ_PLANES_F16X2 images only): the class tables of dvq_pixelcnn_build_tables for EXACTLY these weights.  With them
     * every call -- B = 1 included -- reads what depends on the class label only (grid row 0's vertical stack, position (0, 0),
     * the accumulator states of the sources that follow from them) instead of computing it; without them calls of at least two
     * rows per class build them per call in the workspace.  The results are the same bits either way. */
    const void* class_tables;
} dvq_pixelcnn_weights;

/* Class tables of a packed prior (weights only: build once per model).  dvq_pixelcnn_tables_bytes() = 0 when the weight images
 * are not DVQ_PLANES_F16X2 or the process runs DVQ_GEMM=fp32 (the tables are read by the fp16-plane kernels). */
size_t dvq_pixelcnn_tables_bytes(const dvq_pixelcnn_weights* w_host);
int dvq_pixelcnn_build_tables(const dvq_pixelcnn_weights* w_host, void* tables, size_t tables_bytes, dvq_stream_t stream);

size_t dvq_pixelcnn_workspace_bytes(const dvq_pixelcnn_weights* w_host, int64_t B);
/* label [B] int64 in [0,n_classes), noise q [B,9,n_in] -> codes [B,9] int64 (raster order).
 * logits_out (optional) [B,9,n_in] receives the logits each draw was made from.
 * *err_flag (device int32, caller zeroes it): bit 0 = a label / token out of range; bit 2 = a draw from logits that were all NaN
 * (that position's entry of `codes` is -1 then (v8; 0 before), the sampler itself continues from token 0): with fp16 weight
 * images, an activation beyond +-65 504 made the row NaN -- run the rows that hold a -1 again with bf16x3 images. */
int dvq_pixelcnn_sample(const dvq_pixelcnn_weights* w_host, const int64_t* label, const float* noise,
                        int64_t B, int64_t* codes, float* logits_out, int32_t* err_flag,
                        void* workspace, size_t workspace_bytes, dvq_stream_t stream);
/* The same sampler with controls on the draw (models.py:186-196 draws from softmax(logits) as it is).  Per grid position, l = the
 * fp32 logits, q = the row's noise, s = l / temperature (fp32 division; 1: s = l bit for bit):
 *   top_k in (0, n_in): the kept set S = the top_k largest s, ties towards the lowest index (|S| = top_k); 0 or >= n_in: all.
 *   code = argmax_{k in S} p_k / q_k, lowest k on ties, p = softmax of s over S (max-subtracted, excluded terms add +0.0f).
 *   given [B,9] int64 (optional): an entry >= 0 IS that position's code (range-checked: bit 0 of the flag), a negative one is
 *     drawn; positions mix freely in a row.  The network is exactly causal: a given code changes no earlier position's draw.
 *   logp_model_out [B,9] (optional) = l[c] - logsumexp_k l[k]: the untempered prior's log-likelihood of the code c, drawn or given.
 *   logp_draw_out  [B,9] (optional) = s[c] - logsumexp_{k in S} s[k]: -inf for a given code outside S, 0 when top_k = 1.
 * A row whose logits hold a NaN at a drawn position: code -1, bit 2, as dvq_pixelcnn_sample; both log-probabilities NaN there.
 * With temperature 1, top_k 0 and no given codes the codes and logits_out are dvq_pixelcnn_sample's, bit for bit.
 * noise may be null when given is not: a negative entry then counts as a token out of range (bit 0). */
typedef struct {
    float temperature;        /* finite, > 0 */
    int32_t top_k;            /* >= 0 */
    const int64_t* given;     /* optional [B,9], raster order */
    float* logp_model_out;    /* optional [B,9] */
    float* logp_draw_out;     /* optional [B,9] */
} dvq_pixelcnn_ctl;
int dvq_pixelcnn_sample_ctl(const dvq_pixelcnn_weights* w_host, const int64_t* label, const float* noise,
                            int64_t B, const dvq_pixelcnn_ctl* ctl, int64_t* codes, float* logits_out, int32_t* err_flag,
                            void* workspace, size_t workspace_bytes, dvq_stream_t stream);
/* GatedPixelCNN.forward (models.py:161-174) for given tokens x [B,9] (raster order): logits [B,9,n_in]
 * (position-major; the host mirror permutes to the reference's [B,n_in,3,3]) */
int dvq_pixelcnn_forward(const dvq_pixelcnn_weights* w_host, const int64_t* x, const int64_t* label,
                         int64_t B, float* logits /* [B,9,n_in] */, int32_t* err_flag,
                         void* workspace, size_t workspace_bytes, dvq_stream_t stream);
/* Beam search over the prior: for each of S labels (segments) the `width` most probable distinct code grids, in rank order, with
 * no noise.  Positions 0 .. 8 are visited in the sampler's (raster) order; before position 0 a segment has one live beam of score
 * +0.0f.  At position p every live beam b (b = its rank) has logits l_b: the bits dvq_pixelcnn_forward returns at position p for
 * any grid that starts with b's prefix.  Candidate (b, k), flat index b * n_in + k, has score
 *     score_b + lm,   lm = (l_b[k] - mx) - logf(sum)
 * with mx and sum as dvq_pixelcnn_sample_ctl computes them for logp_model at temperature 1 without top-k (same per-lane stride,
 * same butterfly order), and one float32 addition.  The min(width, live * n_in) candidates with the largest scores survive; the
 * comparison is on the integer order key of the float32 score (-0 counts as +0), ties go to the lower flat index.  Survivors are
 * stored in rank order: score descending, then flat index ascending.
 *   codes [S,W,9] int64 (raster order), score [S,W] f32 = the sum of the nine lm in position order, n_live [S] int32; rows beyond
 *   n_live hold code -1 and score -INFINITY.
 * *err_flag: a NaN candidate score (a NaN logit) in any live row of a segment sets bit 2; that segment comes out with n_live = 0
 * and every code -1, the others are unaffected.  A label out of range sets bit 0 and the segment proceeds from label 0.
 * 1 <= width <= 1024, fp16 weight images (DVQ_PLANES_F16X2) only: anything else is DVQ_EINVAL before any launch.
 * trace (optional, each array optional): what every position selected -- parent [9,S,W] int32 (the parent's rank; -1 beyond the
 * live count), token [9,S,W] int32, score [9,S,W] f32, live [9,S] int32 (after the position), logits [9,S,W,n_in] f32 (the rows'
 * logits BEFORE the position's selection: meaningful for the ranks below the previous live count, 1 at position 0). */
typedef struct {
    int32_t* parent;
    int32_t* token;
    float* score;
    int32_t* live;
    float* logits;
} dvq_pixelcnn_beam_trace;
size_t dvq_pixelcnn_beam_workspace_bytes(const dvq_pixelcnn_weights* w_host, int64_t S, int32_t width);
int dvq_pixelcnn_beam(const dvq_pixelcnn_weights* w_host, const int64_t* label /* [S] */, int64_t S, int32_t width,
                      int64_t* codes /* [S,W,9] */, float* score /* [S,W] */, int32_t* n_live /* [S] */,
                      const dvq_pixelcnn_beam_trace* trace /* or null */, int32_t* err_flag,
                      void* workspace, size_t workspace_bytes, dvq_stream_t stream);

/* ------------------------------------------------------------------ MANO layer (third-party `mano`
 * package at network/gen_net.py:116-118 and gen_diverse_grasp_obman.py:252-253; restated, unpinned)
 * use_pca=True, 45 comps, flat_hand_mean folded into pose_mean by the packer. */
typedef struct {
    const float* v_template;  /* [778,3] = the blendshape GEMM's bias [2334] */
    const float* blend_w;     /* [2334][160]: row e = [shapedirs[.,e] (10) | posedirs[.,e] (135) | 0 (15)]: V = X . blend_w^T */
    const uint16_t* blend_w_planes;   /* optional weight image of blend_w, [3 or 2][2334][160] (planes_kind) */
    const float* j_template;  /* [16,3]   J_regressor @ v_template */
    const float* j_shapedirs; /* [10][48] J_regressor @ shapedirs */
    const float* weights;     /* [778,16] */
    const float* comps;       /* [45,45] hands_components */
    const float* pose_mean;   /* [48] */
    int32_t parents[16];
    const float* blend_w_scale;       /* DVQ_PLANES_F16X2: [2334] row scales */
    int32_t planes_kind;              /* DVQ_PLANES_* of blend_w_planes */
    int32_t _pad;
} dvq_mano_model;

/* betas [B,10] (row stride ldb), pose [B,45] (ldp), optional global_orient [B,3] (ldg) and transl
 * [B,3] (ldt) -> verts; layout 0: [B,778,3] (the mano layer's), 1: [B,3,778] (PointNet input).
 * Three launches per 16 384 samples: pose/chain kernel, blendshape GEMM [B,160] x [160,2334], skinning kernel.
 * workspace: dvq_mano_workspace_bytes(B). */
size_t dvq_mano_workspace_bytes(int64_t B);
int dvq_mano_forward(const dvq_mano_model* m_host, const float* betas, int64_t ldb, const float* pose,
                     int64_t ldp, const float* global_orient, int64_t ldg, const float* transl,
                     int64_t ldt, int64_t B, float* verts, int layout, float* joints /* optional [B,16,3] */,
                     void* workspace, size_t workspace_bytes, dvq_stream_t stream);

/* Backward pass of the layer: the vector-Jacobian product of dvq_mano_forward.  The forward call's inputs (same row strides), the
 * upstream gradients grad_verts ([B,778,3], or [B,3,778] with layout 1) and / or grad_joints [B,16,3] (at least one non-null) ->
 * grad_betas [B,10], grad_pose [B,45], grad_global_orient [B,3], grad_transl [B,3], dense; each is optional (null: not wanted).
 * blend_wt [160][2336]: blend_w transposed, rows 145..159 and columns 2334, 2335 zero (16-byte aligned; the model struct is unchanged).
 * Nothing of the forward call is kept: per 16 384 samples the forward's pose kernel and blendshape GEMM run again (X, A, V), then
 *   skin backward   one workgroup per sample: dV[v] = T_r^T g[v] with T = sum_j w[v][j] A[j] as in the forward -> dV [B,2336], pad
 *                   columns zero; dA[j][i][c] = sum_v w[v][j] g[v][i] [V[v];1][c] and sum_v g[v]: every sum by one thread over
 *                   v = 0, 1, .. 777 in this order, term (w g) x, with a compensated (Kahan) accumulator;
 *   GEMM            dX [B,160] = dV . blend_wt^T on the matrix cores (operands split exactly into bf16 pieces on the fly, fp32
 *                   accumulation; the fp32 kernel with DVQ_GEMM=fp32), the forward's row tiling;
 *   pose backward   one wave per sample: A = [Gr | Gt - Gr J] and the chain Gr_j = Gr_p R_j, Gt_j = Gr_p (J_j - J_p) + Gt_p backwards
 *                   (j = 15 .. 0), grad_joints entering at Gt; dR_j += dX[10 + 9 (j - 1) ..] for j >= 1; Rodrigues backwards with
 *                   angle = ||r + 1e-8|| and 1 - cos a taken as 2 sin^2(a/2), forwards and backwards (the literal form loses the K^2
 *                   term's coefficient at angles near 1e-4); grad_global_orient = d full_pose[0:3], grad_pose = comps . d full_pose[3:48],
 *                   grad_betas = dX[0:10] + j_shapedirs . dJ, grad_transl = sum_v g[v] + sum_j grad_joints[j].
 * With grad_verts null only the pose backward runs.  No atomics, every sum in a fixed order: a row's gradient does not depend on the
 * batch it is in.  transl is accepted for symmetry with the forward (no gradient depends on its value).
 * Refused without a launch: null / unaligned workspace or blend_wt, bad strides, layout or parents, both upstream gradients null
 * (DVQ_EINVAL); a short workspace (DVQ_EWORKSPACE).  B == 0: DVQ_OK.  workspace: dvq_mano_backward_workspace_bytes(B). */
size_t dvq_mano_backward_workspace_bytes(int64_t B);
int dvq_mano_backward(const dvq_mano_model* m_host, const float* blend_wt, const float* betas, int64_t ldb, const float* pose,
                      int64_t ldp, const float* global_orient, int64_t ldg, const float* transl, int64_t ldt, int64_t B,
                      const float* grad_verts, int layout, const float* grad_joints /* optional [B,16,3] */,
                      float* grad_betas, float* grad_pose, float* grad_global_orient, float* grad_transl,
                      void* workspace, size_t workspace_bytes, dvq_stream_t stream);

/* ------------------------------------------------------------------ small data movement
 * out[m, col0:col0+W] = src[m, 0:W]  (concatenations of gen_net.py:109,121) */
int dvq_copy_cols(const float* src, int64_t lds, int64_t M, int W, float* out, int64_t ldo,
                  dvq_stream_t stream);
/* 61-parameter assembly, gen_diverse_grasp_obman.py:243-247:
 * [betas(10) | global_orient(3)=pos[:, :3] | pca_pose(45) | transl(3)=pos[:, 3:6]] */
int dvq_assemble61(const float* recon /* [B,55] */, const float* recon_pos /* [B,6] */, int64_t B,
                   float* out /* [B,61] */, dvq_stream_t stream);
/* per-grasp random object rotation pre-step, gen_diverse_grasp_ho3d.py:213-230:
 * out[b,:3,:] = R[b] @ pc[:3,:] + t ; extra channels copied */
int dvq_transform_cloud(const float* pc /* [C,N] or [B,C,N] */, int64_t pc_batch_stride, const float* R /* [B,3,3] */,
                        const float* t /* [3] */, int64_t B, int C, int N, float* out /* [B,C,N] */,
                        dvq_stream_t stream);
/* The same pre-step for rows of MANY objects in one call (the batched form of the per-object loops of
 * gen_diverse_grasp_ho3d.py:205-248 / gen_diverse_grasp_obman.py:233-247):
 * out[b,:3,:] = R[b] @ pc[obj_of_row[b],:3,:] + t ; extra channels copied.  The arithmetic per component is
 * dvq_transform_cloud's in the same order, so row b holds the bits that call writes for object obj_of_row[b] and rotation
 * R[b]; the object clouds are not replicated per grasp.  One workgroup per (row, span of points) reads the row's index, matrix
 * and `t` once; loads and stores are 16 bytes wide when N % 4 == 0 and `pc` / `out` are 16-byte aligned, any other N takes a
 * scalar path.  An index outside [0, O) sets bit 0 of *err_flag (device int32, zeroed by the caller) and leaves that row of
 * `out` unwritten. */
int dvq_transform_clouds(const float* pc /* [O,C,N] */, const int64_t* obj_of_row /* device [B] */, int64_t O,
                         const float* R /* [B,3,3] */, const float* t /* [3] or NULL */, int64_t B, int C, int N,
                         float* out /* [B,C,N] */, int32_t* err_flag, dvq_stream_t stream);

/* ------------------------------------------------------------------ sampling noise of the prior
 * GatedPixelCNN.generate draws with probs.multinomial(1) (network/pixelcnn/models.py:190-197), i.e. argmax_k p_k / q_k with
 * q ~ Exp(1).  out[r, c] = -log(u) from Philox4x32-10 keyed by `seed`, counter (c / 4, row0 + r, stream_id): the noise of a
 * grasp depends on its GLOBAL row only, so a batch sharded over ranks (row0 = first row of the shard) draws exactly what the
 * unsharded batch draws.  `stream_id` separates independent uses (objects, calls).  cols % 4 == 0. */
int dvq_exp1_noise(uint64_t seed, uint32_t stream_id, int64_t row0, int64_t rows, int cols, float* out /* [rows,cols] */,
                   dvq_stream_t stream);
/* The same draws in another row order: out[r, :] = the noise of global row row0 + perm[r] (perm: device int64 [rows], values in
 * [0, rows)).  GenNet.gen evaluates the prior in the order of the object codes; drawing the noise in that order replaces a
 * gather of the whole [B, 9 * 512] tensor. */
int dvq_exp1_noise_rows(uint64_t seed, uint32_t stream_id, int64_t row0, const int64_t* perm, int64_t rows, int cols,
                        float* out /* [rows,cols] */, dvq_stream_t stream);
/* Per-row keys: out[r, :] = exactly what dvq_exp1_noise(seed, stream_ids[r], row_ids[r], 1, cols, ...) writes (same counter,
 * key and -logf expression: the two kernels share one device function), so a call that mixes the grasps of many objects draws,
 * for every grasp, the noise of its own (seed, object, grasp index) -- what the per-object loops of
 * gen_diverse_grasp_ho3d.py:205-248 / gen_diverse_grasp_obman.py:233-247 draw one object at a time.  A stream id outside
 * [0, 2^32) or a negative row id sets bit 0 of *err_flag (device int32, zeroed by the caller) and fills that row with NaN.
 * cols % 4 == 0. */
int dvq_exp1_noise_keyed(uint64_t seed, const int64_t* stream_ids /* device [rows] */, const int64_t* row_ids /* device [rows] */,
                         int64_t rows, int cols, float* out /* [rows,cols] */, int32_t* err_flag, dvq_stream_t stream);

/* Self-test: out[0] (device) = an fp16 MFMA product with a SUBNORMAL input, out[1] = its exact value.  The fast VQ kernel's
 * error bound assumes the matrix core keeps fp16 subnormals (measured so on gfx950); tests assert out[0] == out[1]. */
int dvq_probe_f16_subnormal(float* out /* device [2] */, dvq_stream_t stream);

/* ------------------------------------------------------------------ contact / penetration proxies (after the path)
 * utils/utils_loss.py:7-24 get_NN (pytorch3d knn_points, K=1): nearest target point of every source point of the same
 * batch element: squared distance d = fma(dz,dz, fma(dy,dy, dx*dx)) and index (first minimum; NaN first).
 * Strides are in floats, so [B,N,3] tensors and [B,C,N] channel-first clouds are both read in place.  N2 <= 4096. */
int dvq_nn_points(const float* src, int64_t src_batch_stride, int64_t src_point_stride, int64_t src_coord_stride,
                  const float* trg, int64_t trg_batch_stride, int64_t trg_point_stride, int64_t trg_coord_stride,
                  int64_t B, int N1, int N2, float* dist /* [B,N1] */, int64_t* idx /* [B,N1] */, dvq_stream_t stream);
/* Area-weighted vertex normals (utils/loss.py:156-157: Meshes(...).verts_normals_packed()) of B meshes sharing one
 * topology: faces [F,3] int32; vf_off [V+1], vf_face [3F]: the faces incident to each vertex, ascending (CSR). */
int dvq_vertex_normals(const float* verts /* [B,V,3] */, int64_t B, int V, const int32_t* faces, const int32_t* vf_off,
                       const int32_t* vf_face, float* normals /* [B,V,3] */, dvq_stream_t stream);
/* utils/utils_loss.py:27-45 get_interior: interior[b,p] = (hand[b,nn[b,p]] - obj[b,p]) . normals[b,nn[b,p]] > 0 */
int dvq_interior(const float* normals /* [B,V,3] */, const float* hand /* [B,V,3] */, int V, const float* obj,
                 int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                 const int64_t* nn_idx /* [B,N] */, int64_t B, int N, uint8_t* interior /* [B,N] */, dvq_stream_t stream);

/* Per-grasp scores for ranking candidates: the three reductions of the proxies above (utils/utils_loss.py:7-45 get_NN /
 * get_interior, the penetration and contact terms of utils/loss.py:154-160) in ONE kernel, one workgroup of 256 threads per grasp;
 * no [B,N] or [B,V,3] intermediate is written.  hand [B,V,3] contiguous; faces / vf_off / vf_face as in dvq_vertex_normals; obj
 * with strides in floats as in dvq_nn_points (a channel-first cloud is read in place).  B >= 0, N >= 1, 1 <= V <= 2048; anything
 * else is DVQ_EINVAL.
 * Per object point p of grasp b (the bits dvq_vertex_normals, dvq_nn_points and dvq_interior produce):
 *   normals : per vertex the sum over its incident faces, ascending, of cross(v1 - v0, v2 - v0) (products rounded, no fma), divided
 *             by max(|n|, 1e-6) with |n| = sqrt(fma(nz,nz, fma(ny,ny, nx*nx)))
 *   d, j    : d = fma(dz,dz, fma(dy,dy, dx*dx)) with dx = obj.x - hand[v].x ..., minimum over v = 0 .. V-1, first minimum, NaN first
 *   inside  : fma(vz, n[j].z, fma(vy, n[j].y, vx * n[j].x)) > 0 with vx = hand[j].x - obj.x ...
 *   term    : d when inside or d is NaN, else +0.0f
 * Reduction, in this fixed order (a grasp's result does not depend on B or on its row):
 *   thread t (0 .. 255) starts from +0.0f and adds the terms of its points p = t, t + 256, ... in ascending p (fp32 additions);
 *   the 256 partial sums are combined by the tree  for s in 128, 64, ..., 1: part[t] += part[t + s] for every t < s;
 *   penetration[b] = part[0]  (NaN when any distance of the grasp is NaN);
 *   n_interior[b] = #inside, n_contact[b] = #(d < contact_threshold): integer sums. */
int dvq_grasp_scores(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                     const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                     int64_t B, int N, float contact_threshold, float* penetration /* [B] */, int32_t* n_interior /* [B] */,
                     int32_t* n_contact /* [B] */, dvq_stream_t stream);
/* Translation push-out of grasps: at most `steps` steps of descent on the scores above with respect to the hand's rigid translation,
 * in ONE kernel, one workgroup of 256 threads per grasp; the best iterate is reported.  New here: the reference's TTT_loss
 * (utils/loss.py:144-167) is what the scores mirror, but the reference does not descend on it at generation time.  A translation
 * changes no vertex normal and is added to every vertex (dvq_mano_forward), so no MANO backward pass is involved: the caller adds
 * `offset` to the hand's transl.  The effect on real grasps is NOT MEASURED (no real checkpoint was available); the update rule's
 * constants are a prototype's.  Inputs as dvq_grasp_scores (hand [B,V,3] contiguous, the topology, obj with strides in floats: a
 * channel-first cloud is read in place) plus steps, push, pull, min_contact.  The hand copy never moves: the translation is taken
 * from the object points.  Normals are computed once per grasp.
 * Per grasp, with t = (+0, +0, +0), for k = 0 .. steps:
 *   1. o'_p = obj_p - t per component (fp32); at k = 0 this is obj_p bit for bit.
 *   2. normals, d_p, j_p, inside_p, term_p exactly as dvq_grasp_scores defines them, on o'.
 *   3. g_p = o'_p - hand[j_p] per component; near_p = !inside_p && d_p < contact_threshold.
 *   4. eight sums, each in the fixed order of dvq_grasp_scores (256 strided partial sums from +0.0f in ascending p, then the tree
 *      s = 128 .. 1): pen = sum of term_p; S_in[c] = sum of (inside_p ? g_p[c] : +0.0f) and S_nr[c] = sum of (near_p ? g_p[c] : +0.0f)
 *      for c = 0, 1, 2; the integer counts n_in = #inside, n_ct = #(d < contact_threshold), n_nr = #near.
 *   5. key (cls, pen): cls = 2 if pen is NaN, else 1 if n_ct < min_contact, else 0 (the order of the host's select_keys by
 *      penetration).  Iterate 0 starts as the best; iterate k becomes the best iff cls_k < cls_best, or cls_k == cls_best and
 *      pen_k < pen_best (strictly: among equal keys the earliest iterate is kept; an iterate of class 2 never replaces anything).
 *   6. if k == steps, stop.  Otherwise step[c] = +0.0f; if n_in > 0: step[c] = step[c] + push * (S_in[c] / (float)n_in); if n_nr > 0:
 *      step[c] = step[c] + pull * (S_nr[c] / (float)n_nr); t[c] = t[c] + step[c].  Every operation is rounded to fp32 on its own
 *      (nothing fused), the division is IEEE.  The loop also ends when pen is NaN or all three step[c] == 0 (no later iterate
 *      could become the best).
 * Outputs: offset [B,3] = the best iterate's t; iter [B] = its k; penetration / n_interior / n_contact [B] = its pen, n_in, n_ct.
 * With steps = 0: the three scores are the bits of dvq_grasp_scores, offset = 0, iter = 0.  A grasp's result does not depend on B
 * or on its row.  Interior points push the hand along the mean of their g (out of the object), near points pull it along theirs
 * (towards the surface); an object lying deep inside the hand is pulled further in, since its nearest-vertex distances shrink that
 * way: the kept iterate is only "not worse under the proxy".
 * B >= 0, N >= 1, 1 <= V <= 2048, 0 <= steps <= 64, push and pull finite and >= 0, no null pointer; anything else is DVQ_EINVAL,
 * nothing launched. */
int dvq_grasp_refine(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                     const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                     int64_t B, int N, float contact_threshold, int steps, float push, float pull, int min_contact,
                     float* offset /* [B,3] */, int32_t* iter /* [B] */, float* penetration /* [B] */, int32_t* n_interior /* [B] */,
                     int32_t* n_contact /* [B] */, dvq_stream_t stream);
/* Rigid push-out of grasps: dvq_grasp_refine with the other half of a rigid motion -- at most `steps` steps of descent on the same
 * scores with respect to the hand's rigid translation AND a rotation about a pivot (the wrist), in ONE kernel, one workgroup of 256
 * threads per grasp; the best iterate is reported.  A hand whose fingertips sink into the object while its palm stands off cannot be
 * repaired by a shift; it needs a small turn.  No MANO backward pass is involved: a rotation of the hand about a pivot turns its
 * vertex normals with it, so in the hand's own frame neither the hand nor its normals change, only the object points move; and the
 * MANO layer applies global_orient about the root joint and adds transl afterwards, so a turn Q about the root joint's world position
 * is exactly global_orient <- log(Q * exp(global_orient)), and the shift still goes to transl.  The effect on real grasps is NOT
 * MEASURED (no real checkpoint was available); the update rule's constants are a prototype's, untuned.
 * Inputs as dvq_grasp_refine plus pivot [B,3] fp32 contiguous, the pivot c of every grasp (the wrist's world position), and spin.
 * Everything this entry point adds to dvq_grasp_refine is single fp32 operations, each rounded on its own (no fma), IEEE division and
 * square root, no library function; expressions below are evaluated left to right as parenthesised.  The shared per-point part
 * (step 2) keeps the fmas dvq_grasp_scores documents.  "The canonical sum" is that of dvq_grasp_scores: 256 strided partial sums from
 * +0.0f in ascending p, then the tree s = 128 .. 1.
 * State per grasp: t = (+0, +0, +0), q = (w, x, y, z) = (1, 0, 0, 0), turned = false.  R = R(q), row-major R[i][j], from the products
 *   xx = x*x, yy = y*y, zz = z*z, xy = x*y, xz = x*z, yz = y*z, wx = w*x, wy = w*y, wz = w*z:
 *   R[0] = (1 - 2*(yy + zz),  2*(xy - wz),      2*(xz + wy)    )
 *   R[1] = (2*(xy + wz),      1 - 2*(xx + zz),  2*(yz - wx)    )
 *   R[2] = (2*(xz - wy),      2*(yz + wx),      1 - 2*(xx + yy))
 * The world hand of the state is R (v - c) + c + t.  For k = 0 .. steps:
 *   1. u_p = obj_p - t per component.  If !turned: o'_p = u_p (at k = 0, and always with spin = 0: dvq_grasp_refine's step 1 bit for
 *      bit).  Otherwise w = u_p - c per component and o'_p[i] = ((R[0][i]*w.x + R[1][i]*w.y) + R[2][i]*w.z) + c[i]: R^T w + c.
 *   2. normals (once, of the hand as given), d_p, j_p, inside_p, term_p and near_p exactly as dvq_grasp_refine defines them, on o';
 *      g_p = o'_p - hand[j_p] and r_p = hand[j_p] - c per component.
 *   3. 21 canonical sums and three integer counts: pen = sum of term_p; and for each of the two sets (S = inside_p, S = near_p), every
 *      term masked as (S ? x : +0.0f):  G[c] = sum of g[c];  A[c] = sum of r[c];  X = sum of cross(r, g) with components
 *      (r.y*g.z - r.z*g.y, r.z*g.x - r.x*g.z, r.x*g.y - r.y*g.x);  Q = sum of ((r.x*r.x + r.y*r.y) + r.z*r.z);
 *      n_in = #inside, n_ct = #(d < contact_threshold), n_nr = #near.
 *   4. the key (cls, pen) and the rule for the best iterate are dvq_grasp_refine's step 5: the earliest iterate among equal keys.
 *   5. if k == steps or pen is NaN, stop.  Otherwise
 *      st[c] : dvq_grasp_refine's step 6 on G_in, G_nr (the step of the translation, in the hand's frame);
 *      om[c] = +0.0f.  If spin > 0 (with spin = 0 nothing of the turn is evaluated and om stays +0):
 *        if n_in > 0 and Q_in > 0:  m[c] = G_in[c] / (float)n_in (the quotients of st);  tau = X_in - cross(A_in, m), i.e.
 *          tau.x = X_in.x - (A_in.y*m.z - A_in.z*m.y) and cyclic;  om[c] = om[c] + push * (tau[c] / Q_in);
 *        if n_nr > 0 and Q_nr > 0:  the same on the near set with pull;
 *        om[c] = spin * om[c].
 *      If all six of st[c] and om[c] are == 0, stop (no later iterate could become the best).
 *      t[i] = t[i] + (turned ? ((R[i][0]*st.x + R[i][1]*st.y) + R[i][2]*st.z) : st[i]), with R and turned as they stand.
 *      If some om[c] != 0:  h = 0.5f * om;  p = q (x) (1, h), the Hamilton product with the increment on the right (the turn is
 *        expressed in the hand's frame):
 *          p.w = ((q.w - q.x*h.x) - q.y*h.y) - q.z*h.z        p.x = ((q.x + q.w*h.x) + q.y*h.z) - q.z*h.y
 *          p.y = ((q.y + q.w*h.y) - q.x*h.z) + q.z*h.x        p.z = ((q.z + q.w*h.z) + q.x*h.y) - q.y*h.x
 *        n2 = ((p.w*p.w + p.x*p.x) + p.y*p.y) + p.z*p.z;  q = p * (1.0f / sqrtf(n2)) per component;  turned = true;  R = R(q).
 * tau is the torque of the pull field about the pivot after its mean is removed (a field that a shift alone satisfies turns nothing);
 * tau / Q is the least-squares small rotation under an isotropic inertia, which under-turns when the contacts cluster far from the
 * wrist; the normalised (1, h) bounds a step's angle below pi without trigonometry.  The pull term may turn the hand INTO the object,
 * as it may shift it: the kept iterate is only "not worse under the proxy".
 * Outputs: offset [B,3] = the best iterate's t; quat [B,4] = its q (w, x, y, z); iter [B] = its k; penetration / n_interior /
 * n_contact [B] = its pen, n_in, n_ct.  The refined hand is R(quat) (v - c) + c + offset.  With spin = 0 every output but quat is the
 * bits of dvq_grasp_refine and quat = (1, 0, 0, 0); with steps = 0 the three scores are the bits of dvq_grasp_scores.  A grasp's
 * result does not depend on B or on its row.  Coordinates that are not finite behave as in dvq_grasp_refine: a NaN in the hand or the
 * cloud makes iterate 0 of class 2 (NaN pen), the only iterate; an Inf in the cloud, or a pivot that is not finite, where it enters a
 * sum makes the step not finite, the next iterate is of class 2, ends the loop and never replaces the iterate kept.
 * B >= 0, N >= 1, 1 <= V <= 2048, 0 <= steps <= 64, push, pull and spin finite and >= 0, no null pointer; anything else is
 * DVQ_EINVAL, nothing launched. */
int dvq_grasp_refine_rigid(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                           const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                           int64_t B, int N, const float* pivot /* [B,3] */, float contact_threshold, int steps, float push, float pull,
                           float spin, int min_contact, float* offset /* [B,3] */, float* quat /* [B,4] */, int32_t* iter /* [B] */,
                           float* penetration /* [B] */, int32_t* n_interior /* [B] */, int32_t* n_contact /* [B] */,
                           dvq_stream_t stream);
/* Articulated push-out of grasps: dvq_grasp_refine_rigid whose fingers may also curl -- the state gains one unit quaternion q_f per
 * finger, a turn of the finger about its knuckle c_f, in ONE kernel, one workgroup of 256 threads per grasp; the best iterate is
 * reported.  One fingertip buried in the object while the other four sit well cannot be repaired by a rigid motion.  No MANO backward
 * pass is involved: the kernel searches with a BLEND MODEL of the hand (below), the host writes the turns into the pose parameters (the
 * knuckles are children of the root joint, so a turn D_f about a knuckle is R_loc' = R0^T D_f R0 R_loc on its local rotation), MANO is
 * posed again, and the caller compares the re-posed hand's scores with those of iterate 0, which this entry point reports for that
 * purpose.  The blend model differs from the re-posed hand (measured on the real model: up to 0.44 / 1.81 / 3.24 mm at 0.05 / 0.2 /
 * 0.35 rad), so the kept iterate is the best only under the model.  The effect on real grasps is NOT MEASURED; the constants are untuned.
 * Inputs as dvq_grasp_refine_rigid plus: vert_part [V] int32 (-1, or the vertex's finger in [0, P); a label outside [0, P) is read as
 * -1), vert_w [V] fp32 (a weight in [0, 1]), P (1 <= P <= 5), knuckle [B,P,3] fp32 contiguous (c_f, in the frame of the hand as
 * given), curl >= 0, and min_w = cos(max_curl / 2), computed in float64 by the caller and rounded once to fp32.
 * Everything this entry point adds to dvq_grasp_refine_rigid is single fp32 operations, each rounded on its own (no fma), IEEE division
 * and square root; expressions are evaluated left to right as parenthesised.  With curl = 0 nothing of it is evaluated.
 * State per grasp: dvq_grasp_refine_rigid's (t, q, turned) plus, per finger f, q_f = (1, 0, 0, 0) and turned_f = false; base = the hand
 * as given; hand = base; normals = those of hand.  For k = 0 .. steps:
 *   1-3. dvq_grasp_refine_rigid's steps 1 to 3 on `hand` and `normals` as they stand: o', d_p, j_p, inside_p, near_p, g_p, r_p, the 21
 *      canonical sums and the three counts.  If k == 0: penetration0, n_interior0, n_contact0 = pen, n_in, n_ct.
 *      If curl > 0, with f = vert_part[j_p] (if 0 <= f < P) and w = vert_w[j_p]:  a = hand[j_p] - c_f per component;
 *        e = (w * (a.y*g.z - a.z*g.y), w * (a.z*g.x - a.x*g.z), w * (a.x*g.y - a.y*g.x));  s = (w * w) * ((a.x*a.x + a.y*a.y) + a.z*a.z);
 *        for each set S (inside, near) and each finger f, four more canonical sums over all points, a point's term being
 *        ((S_p and vert_part[j_p] == f) ? x : +0.0f):  X_S,f[c] = sum of e[c];  Q_S,f = sum of s.
 *   4. the key and the rule for the best iterate are dvq_grasp_refine's; the best iterate keeps its q_f too.
 *   5. if k == steps or pen is NaN, stop.  st and om as dvq_grasp_refine_rigid's step 5.
 *      If curl > 0, for every finger f:  of[c] = +0.0f;  if Q_in,f > 0: of[c] = of[c] + push * (X_in,f[c] / Q_in,f);  if Q_nr,f > 0:
 *        of[c] = of[c] + pull * (X_nr,f[c] / Q_nr,f);  of[c] = curl * of[c].  (The least-squares small rotation of the finger about its
 *        knuckle; no mean is removed: a finger has no shift of its own.)  If some of[c] != 0:  h = 0.5f * of;  p = (1, h) (x) q_f, the
 *        increment on the LEFT (it is expressed in the hand's fixed frame):
 *          p.w = ((q.w - h.x*q.x) - h.y*q.y) - h.z*q.z        p.x = ((q.x + h.x*q.w) + h.y*q.z) - h.z*q.y
 *          p.y = ((q.y + h.y*q.w) - h.x*q.z) + h.z*q.x        p.z = ((q.z + h.z*q.w) + h.x*q.y) - h.y*q.x
 *        n2 = ((p.w*p.w + p.x*p.x) + p.y*p.y) + p.z*p.z;  cand = p * (1.0f / sqrtf(n2)) per component.  The candidate is accepted iff
 *        cand.w >= min_w (a NaN refuses): then q_f = cand, turned_f = true.  Otherwise q_f stays for this step.
 *      If all six of st[c] and om[c] are == 0 and no finger was accepted in this step, stop.
 *      t and q are updated as in dvq_grasp_refine_rigid.  If a finger was accepted in this step, the hand of the next iterate is, for
 *      every vertex v with f = vert_part[v] in [0, P) and turned_f, with R = R(q_f) and d = base[v] - c_f per component:
 *        rot[i] = ((R[i][0]*d.x + R[i][1]*d.y) + R[i][2]*d.z) + c_f[i];   hand[v][i] = base[v][i] + vert_w[v] * (rot[i] - base[v][i]);
 *      every other vertex is base[v] bit for bit; and normals = the vertex normals of this hand (recomputed, not rotated).
 * Outputs: dvq_grasp_refine_rigid's six, finger_quat [B,P,4] = the best iterate's q_f (w, x, y, z), and penetration0 / n_interior0 /
 * n_contact0 [B], which are the bits of dvq_grasp_scores on the input.  The hand the kernel believed in is R(quat) (hand* - c) + c +
 * offset with hand* the blend above under finger_quat.  With curl = 0 the six are the bits of dvq_grasp_refine_rigid and every q_f is
 * (1, 0, 0, 0); with spin = 0 as well they are those of dvq_grasp_refine; with steps = 0 the scores are those of dvq_grasp_scores.  A
 * grasp's result does not depend on B or on its row.  Coordinates that are not finite behave as in dvq_grasp_refine_rigid; a knuckle
 * that is NaN makes its finger's Q NaN (no turn), one that is Inf makes the candidate NaN (refused): such a finger never turns.
 * Known limits: no joint limits beyond max_curl; no finger-to-finger collision test; the shift, the turn and the curl all answer the
 * same contacts, so a step may overshoot.
 * B >= 0, N >= 1, 1 <= V <= 2048, 1 <= P <= 5, 0 <= steps <= 64, push, pull, spin and curl finite and >= 0, 0 <= min_w <= 1, no null
 * pointer; anything else is DVQ_EINVAL, nothing launched. */
int dvq_grasp_refine_fingers(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                             const int32_t* vert_part /* [V] */, const float* vert_w /* [V] */, int P, const float* obj,
                             int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride, int64_t B, int N,
                             const float* pivot /* [B,3] */, const float* knuckle /* [B,P,3] */, float contact_threshold, int steps,
                             float push, float pull, float spin, float curl, float min_w, int min_contact, float* offset /* [B,3] */,
                             float* quat /* [B,4] */, float* finger_quat /* [B,P,4] */, int32_t* iter /* [B] */,
                             float* penetration /* [B] */, int32_t* n_interior /* [B] */, int32_t* n_contact /* [B] */,
                             float* penetration0 /* [B] */, int32_t* n_interior0 /* [B] */, int32_t* n_contact0 /* [B] */,
                             dvq_stream_t stream);
/* Grasp stability proxy: the contact-wrench sums of a grasp and a ranking key from them, with the three scores of dvq_grasp_scores,
 * in ONE kernel, one workgroup of 256 threads per grasp.  New here: the reference judges whether the object stays in the hand by a
 * physics run (pybullet + V-HACD, out of scope); this is the usual cheap stand-in, a force-closure figure over the contact wrenches:
 * every object point within the contact threshold of the hand is a contact that pushes with a UNIT force along the normal of its
 * nearest hand vertex, frictionless.  27 sums per grasp -- the 6-vector sum of the wrenches and the upper triangle of sum w w^T --
 * give the net wrench of unit contact forces (the force-closure term of differentiable grasp synthesis, |G c|) and, on the host, the
 * smallest singular value of the grasp matrix (Li & Sastry's Q_MSV).  A PROXY: the force model and the torque length are untuned,
 * it replaces no physics run, and its effect on real grasps is NOT MEASURED (no real checkpoint was available).
 * Inputs exactly as dvq_grasp_scores (hand [B,V,3] contiguous, the topology, obj with strides in floats: a channel-first cloud is
 * read in place) plus inv_length, the reciprocal of the length that makes torques commensurate with forces.
 * "The canonical sum" below is the reduction of dvq_grasp_scores: thread t (0 .. 255) starts from +0.0f and adds the terms of its
 * points p = t, t + 256, ... in ascending p (fp32 additions); then the tree  for s in 128, 64, ..., 1: part[t] += part[t + s] for
 * every t < s.  Per grasp:
 *   1. centre.x = (the canonical sum of obj.x over all N points) / (float)N, an fp32 IEEE division; .y and .z likewise.
 *   2. per point p: normals, d, j, inside and term exactly as dvq_grasp_scores defines them; contact = d < contact_threshold, the
 *      set that n_contact counts.
 *   3. per point p: force f = n[j]; arm r = ((obj.x - centre.x) * inv_length, (obj.y - centre.y) * inv_length, (obj.z - centre.z) *
 *      inv_length); torque tau = (r.y*f.z - r.z*f.y, r.z*f.x - r.x*f.z, r.x*f.y - r.y*f.x), every product rounded, no fma; wrench
 *      w = (f.x, f.y, f.z, tau.x, tau.y, tau.z).
 *   4. the 27 terms of point p: w[a] for a = 0 .. 5 (columns 0 .. 5), then w[a] * w[b] for a <= b in row-major order of the upper
 *      triangle (columns 6 .. 26: 00 01 02 03 04 05 11 12 ... 55); each term is its value when contact holds and +0.0f otherwise;
 *      sums[b][c] = the canonical sum of column c.
 *   5. with S = sums[b]: q = fma(S5,S5, fma(S4,S4, fma(S3,S3, fma(S2,S2, fma(S1,S1, S0*S0))))), nf = (float)n_contact;
 *      key = NaN when penetration is NaN, otherwise +inf when n_contact == 0, otherwise q / (nf * nf) (fp32, IEEE division).
 *      A smaller key means the unit contact forces cancel better.
 * Outputs: penetration, n_interior, n_contact [B]: the bits of dvq_grasp_scores on the same inputs; centre [B,3]; sums [B,27];
 * key [B].  A grasp's outputs depend on neither B nor its row.
 * B >= 0, N >= 1, 1 <= V <= 2048, no null pointer; anything else is DVQ_EINVAL, nothing launched. */
int dvq_grasp_wrench(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                     const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                     int64_t B, int N, float contact_threshold, float inv_length, float* penetration /* [B] */,
                     int32_t* n_interior /* [B] */, int32_t* n_contact /* [B] */, float* centre /* [B,3] */, float* sums /* [B,27] */,
                     float* key /* [B] */, dvq_stream_t stream);
/* Force-closure quality of grasps with friction: the support function of the contacts' Coulomb friction cones over a table of D
 * directions in wrench space, its minimum and the direction that attains it, in ONE kernel, one workgroup of 256 threads per grasp.
 * dvq_grasp_wrench above is frictionless and sums unit forces: it cannot tell a hand that could balance any disturbance from one whose
 * contacts merely cancel.  The classical answer (Ferrari & Canny, L1 form): take the convex hull of the wrenches that unit normal
 * forces within every contact's friction cone can exert; the grasp is in force closure iff the origin lies strictly inside, and the
 * quality eps is the origin's distance to the hull's boundary.  The hull is never built: its support function is h(u) = the largest
 * w . u over contacts and cone forces, and eps = the minimum of h over unit u in R^6.  For the exact circular cone the inner maximum
 * has the closed form below, so `quality`, the minimum over the D directions given, is an UPPER BOUND of eps, and quality <= 0
 * CERTIFIES that the grasp is not in force closure; quality > 0 certifies nothing.  No physics run, no soft contact; mu and the torque
 * length are untuned; contacts are the cloud points within the threshold of the hand, penetrating ones included; the effect on real
 * grasps is NOT MEASURED.
 * Inputs exactly as dvq_grasp_wrench (hand [B,V,3] contiguous, the topology, obj with strides in floats, contact_threshold a squared
 * distance, inv_length) plus mu, the friction coefficient, dirs [D,6] fp32 on the device (the callers' table holds unit vectors; the
 * kernel does not look) and D.
 * Everything is fp32, every operation rounded on its own, fma = the only fused ones; dot(a,b) = fma(a.z,b.z, fma(a.y,b.y, a.x*b.x));
 * cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), every product rounded, no fma; sqrtf is IEEE.  Per grasp:
 *   1. centre: step 1 of dvq_grasp_wrench.
 *   2. per point p: normals, d, j exactly as dvq_grasp_scores defines them; contact = d < contact_threshold, the set n_contact counts.
 *   3. per contact p: n = n[j]; r = ((obj.x - centre.x) * inv_length, (obj.y - centre.y) * inv_length, (obj.z - centre.z) * inv_length).
 *   4. per direction k with u = dirs[k], uf = u[0:3], ut = u[3:6], and per contact:
 *        a = uf + cross(ut, r) per component (so that w . u = f . a for the wrench w = (f, cross(r, f)) of a force f at the contact);
 *        s = dot(n, a);  c = cross(n, a);  h = fma(mu, sqrtf(dot(c, c)), s)
 *      -- the largest f . a over the cone f = n + mu t, |t| <= 1, t normal to n (the tangential part of a is taken from the cross
 *      product, not from |a|^2 - s^2, which cancels).  support[k] = (the largest h over the contacts) + 0.0f: the maximum starts from -inf,
 *      h > max replaces, so a NaN never does; the addition makes a zero +0.0f, so that the contacts' order reaches no bit.
 *   5. quality = the smallest support[k]: it starts from +inf and a smaller value replaces; worst_dir = the lowest k with support[k]
 *      == quality.
 *   6. status, the first that applies: 2 = a coordinate of the hand or of the cloud is not finite: quality NaN, worst_dir -1, every
 *      support NaN; 1 = n_contact == 0: quality -inf, worst_dir -1, every support -inf; 0 otherwise.
 * Only maxima, one minimum and an integer count follow the per-point results -- no float sum over contacts -- so nothing depends on a
 * reduction order, and a grasp's outputs depend on neither B nor its row.
 * Outputs: quality fp32 [B]; worst_dir, status int32 [B]; n_contact int32 [B]: the bits of dvq_grasp_scores; centre fp32 [B,3]: the bits
 * of dvq_grasp_wrench; support fp32 [B,D], which may be NULL (not written).
 * B >= 0, N >= 1, 1 <= V <= 2048, 1 <= D <= DVQ_GRASP_CLOSURE_MAX_DIRS, mu finite and >= 0, no null pointer but support; anything else
 * is DVQ_EINVAL, nothing launched. */
#define DVQ_GRASP_CLOSURE_MAX_DIRS 1024
int dvq_grasp_closure(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                      const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                      int64_t B, int N, float contact_threshold, float inv_length, float mu, const float* dirs /* [D,6] */, int D,
                      float* quality /* [B] */, int32_t* worst_dir /* [B] */, int32_t* status /* [B] */, int32_t* n_contact /* [B] */,
                      float* centre /* [B,3] */, float* support /* [B,D] or NULL */, dvq_stream_t stream);
/* Hand-side contact of grasps: for every hand vertex its nearest object point, and from those which PARTS of the hand touch the
 * object -- per part the smallest squared distance and the number of touching vertices, and a bit per vertex -- in ONE kernel, one
 * workgroup of 256 threads per grasp.  The scores above look from the object's side (how many cloud points lie near the hand); this
 * looks from the hand's, as the reference's finger-restricted contact terms do (utils/loss.py: Contact_loss, CMap_loss_hand and
 * CMap_loss4 take get_NN(hand, obj); CMap_consistency_loss thresholds hard contact at 5 mm).  A PROXIMITY figure: no contact-force
 * model, the threshold is the caller's and untuned, and its effect on real grasps is NOT MEASURED (no real checkpoint was available).
 * Inputs: hand [B,V,3] contiguous fp32; part_of_vertex int32 [V]: the part of every vertex, a value outside [0, P) means "no part"
 * (not an error); P, the number of parts; obj with strides in floats as dvq_grasp_scores takes it (a channel-first cloud is read in
 * place); contact_threshold, a squared distance.
 * Per grasp, when all 3 V hand coordinates and all 3 N cloud coordinates are finite (fp32, fma = the only fused operations):
 *   1. per vertex v and point p: dx = hand.x - obj.x, dy, dz likewise; d(v,p) = fma(dz, dz, fma(dy, dy, dx * dx)).
 *   2. d[v] = the minimum of d(v,p) over p; idx[v] = the lowest p that attains it: the bits of dvq_nn_points with the hand as source.
 *   3. touch[v] = d[v] < contact_threshold.
 *   4. part_min[q] = the minimum of d[v] over the vertices labelled q, +inf if there are none; part_count[q] = the number of
 *      vertices labelled q with touch[v].
 *   5. mask: bit (v & 31) of word (v >> 5) is touch[v], for every vertex, labelled or not; the unused high bits of the last word
 *      are 0.  W = (V + 31) / 32 words per grasp.
 *   6. status = 0; vert_dist[v] = d[v], vert_idx[v] = idx[v].
 * A grasp with a non-finite coordinate (hand or cloud) has no figure: status = 1, part_min and vert_dist NaN, part_count and
 * vert_idx -1, mask 0; other grasps are unaffected.
 * Only minima, integer counts and bits are produced -- no float sum -- so nothing depends on a reduction order, and a grasp's outputs
 * depend on neither B nor its row.
 * Outputs: part_min fp32 [B,P]; part_count int32 [B,P]; mask int32 [B,W]; status int32 [B]; vert_dist fp32 [B,V] and vert_idx int32
 * [B,V], each of which may be NULL (not written).
 * B >= 0, N >= 1, 1 <= V <= 2048, 1 <= P <= 32, no null pointer but the two optional ones; anything else is DVQ_EINVAL, nothing
 * launched. */
int dvq_grasp_parts(const float* hand /* [B,V,3] */, const int32_t* part_of_vertex /* [V] */, int V, int P, const float* obj,
                    int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride, int64_t B, int N,
                    float contact_threshold, float* part_min /* [B,P] */, int32_t* part_count /* [B,P] */, int32_t* mask /* [B,W] */,
                    int32_t* status /* [B] */, float* vert_dist /* [B,V] or NULL */, int32_t* vert_idx /* [B,V] or NULL */,
                    dvq_stream_t stream);
/* Self-collision of grasps: the hand against ITSELF -- for every vertex of a part its nearest vertex among the parts it is tested
 * against, the interior test of dvq_grasp_scores against that vertex's tangent plane, and from those, per part, the number of
 * penetrating vertices, the largest depth, the smallest clearance and which parts were hit, and a bit per vertex -- in ONE kernel, one
 * workgroup of 256 threads per grasp.  The decoder builds a hand from separately sampled codes (thumb, four fingers, palm) and the
 * scores above look at hand against object only: two fingers passing through each other show in none of them.  A PROXIMITY figure in
 * the style of the reference's get_interior (utils/utils_loss.py), NOT a mesh-mesh intersection: vertices only, so a thin crossing
 * between vertices is missed; reach, margin and the seam are the caller's, calibrated only against false alarms on 48 posed hands of
 * the real hand model and untuned otherwise; the effect on real grasps is NOT MEASURED (no real checkpoint was available).
 * Inputs: hand [B,V,3] contiguous fp32; faces / vf_off / vf_face: the topology as dvq_grasp_scores takes it; part_of_vertex int32 [V]
 * on the device: the part of every vertex, a value outside [0, P) means "no part" (not an error); source_of_vertex int32 [V] on the
 * device: != 0 where the vertex may count as a SOURCE (the caller clears the vertices next to a join of two parts, where v - u is
 * tangent to the surface and the sign of the test is noise; they remain targets); P, the number of parts; pairs uint32 [P] on the
 * HOST (read before the call returns): bit b of pairs[a] = part a's vertices are tested against part b's; reach2, a squared distance;
 * margin, a distance.
 * Per grasp, when all 3 V coordinates are finite (fp32, fma = the only fused operations):
 *   1. n[u]: the vertex normals exactly as dvq_grasp_scores defines them.
 *   2. a = part_of_vertex[v]; a vertex whose label is outside [0, P) is neither source nor target.  Vertex u is a target of v iff its
 *      label b is in [0, P) and bit b of pairs[a] is set.  dx = hand[v].x - hand[u].x, dy, dz likewise; d(v,u) = fma(dz, dz, fma(dy, dy,
 *      dx * dx)).  d[v] = the minimum of d(v,u) over the targets; idx[v] = the lowest u that attains it.  With no target: d[v] = +inf,
 *      idx[v] = -1.
 *   3. depth[v] = fma(wz, n[idx].z, fma(wy, n[idx].y, wx * n[idx].x)) with w = hand[idx] - hand[v] per component: the expression of
 *      the interior test.
 *   4. pen[v] = source_of_vertex[v] != 0 && idx[v] >= 0 && d[v] < reach2 && depth[v] > margin.
 *   5. per part a, over the vertices labelled a: pen_count[a] = the number with pen[v]; pen_depth[a] = the largest depth[v] over those,
 *      +0.0f if there are none; gap_min[a] = the smallest d[v] over the vertices with source_of_vertex != 0, +inf if there are none;
 *      pair_bits[a] = the OR of 1 << part_of_vertex[idx[v]] over the vertices with pen[v].
 *   6. mask: bit (v & 31) of word (v >> 5) is pen[v]; the unused high bits of the last word are 0.  W = (V + 31) / 32 words per
 *      grasp.  status = 0.
 * A grasp with a non-finite coordinate has no figure: status = 1, pen_depth and gap_min NaN, pen_count -1, pair_bits and mask 0;
 * other grasps are unaffected.
 * Only minima, maxima, integer counts and bits are produced -- no float sum -- so nothing depends on a reduction order, and a grasp's
 * outputs depend on neither B nor its row.
 * Outputs: pen_count int32 [B,P]; pen_depth fp32 [B,P]; gap_min fp32 [B,P]; pair_bits int32 [B,P]; mask int32 [B,W]; status int32 [B].
 * B >= 0, 1 <= V <= 2048, 1 <= P <= 32, no null pointer, reach2 finite and > 0, margin finite and >= 0, no bit a in pairs[a] (a part
 * against itself) and no bit at or above P; anything else is DVQ_EINVAL, nothing launched.  (B = 0 returns DVQ_OK before any pointer
 * is looked at, as in dvq_grasp_parts.) */
int dvq_grasp_self(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                   const int32_t* part_of_vertex /* [V] device */, const int32_t* source_of_vertex /* [V] device, != 0: may count */,
                   int P, const uint32_t* pairs /* [P] HOST: bit b of pairs[a] = test part a's vertices against part b */,
                   int64_t B, float reach2, float margin,
                   int32_t* pen_count /* [B,P] */, float* pen_depth /* [B,P] */, float* gap_min /* [B,P] */,
                   int32_t* pair_bits /* [B,P] */, int32_t* mask /* [B,W] */, int32_t* status /* [B] */, dvq_stream_t stream);
/* The test-time loss of grasps and its gradient: the two terms of the reference's TTT_loss (utils/loss.py: the penetration term and
 * the hand-centric Contact_loss) AND their gradient with respect to the hand's vertices, in ONE kernel, one workgroup of 256 threads
 * per grasp; no [B,N] or [B,N,V] intermediate is written.  What dvq_mano_backward is fed with for gradient refinement
 * (gen_diverse_grasp_obman.py:69-94).
 * Inputs: everything dvq_grasp_scores takes (hand [B,V,3] contiguous, the topology, obj with strides in floats: a channel-first cloud
 * is read in place; contact_threshold, a squared distance); target_of_vertex int32 [V] on the device or NULL: != 0 where the vertex is
 * a CONTACT TARGET (the reference's prior_idx subset), NULL = every vertex; w_pen, w_con fp32 [B] on the device or NULL (= 1 for every
 * row): the weights of the two terms in the gradient; mean_contact 0 or 1; grad_hand fp32 [B,V,3] or NULL (no gradient phase).
 * Per grasp b, when every coordinate of its hand and of its cloud is finite (fp32, fma = the only fused operations):
 *   1. normals, d_p, j_p, inside_p, term_p exactly as dvq_grasp_scores defines them; penetration, n_interior, n_contact are its bits.
 *   2. dc_p = the minimum over the target vertices of the same distance expression, jc_p = the lowest target index that attains it
 *      (with no target vertex: dc_p = +inf and the point names no vertex); contact_p = d_p < contact_threshold -- the mask is taken
 *      from the all-vertex distance, the value from the target distance, as the reference does.
 *   3. contact_sum = the canonical sum of dvq_grasp_scores (256 strided partial sums from +0.0f in ascending p, then the tree
 *      128 .. 1) of  contact_p ? dc_p : +0.0f.
 *   4. with grad_hand: Gp[v][c] = the fp32 sum from +0.0f, in ascending p, of hand[v][c] - obj[p][c] over the points with inside_p and
 *      j_p == v; Gc[v][c] the same sum over the points with contact_p and jc_p == v; a = 2.0f * w_pen[b]; c = 2.0f * w_con[b], with
 *      mean_contact c = (2.0f * w_con[b]) / (float)max(n_contact, 1) (an IEEE fp32 division);
 *      grad_hand[b][v][c] = fma(c, Gc[v][c], a * Gp[v][c]).  This is the gradient of w_pen * penetration + w_con * contact_sum
 *      (/ max(n_contact, 1)) with the masks and the indices held constant: nothing flows through the normals or the threshold.
 * A grasp with a non-finite coordinate of its hand or of its cloud: the three scores are what dvq_grasp_scores reports, contact_sum is
 * NaN and every element of its grad_hand is NaN; other grasps are unaffected.
 * No atomics: every sum has one owner and one order, so the outputs are the same bits on every run and depend on neither B nor the row.
 * Outputs: penetration, contact_sum fp32 [B]; n_interior, n_contact int32 [B]; grad_hand fp32 [B,V,3] if given.
 * B >= 0, 1 <= N <= DVQ_GRASP_TTT_MAX_N (one word per point sits in LDS), 1 <= V <= 2048, mean_contact 0 or 1, no null pointer but
 * the four that may be; anything else is DVQ_EINVAL, nothing launched.  (B = 0 returns DVQ_OK before any pointer is looked at.) */
#define DVQ_GRASP_TTT_MAX_N 16384
int dvq_grasp_ttt(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                  const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride, int64_t B, int N,
                  float contact_threshold, const int32_t* target_of_vertex /* [V] or NULL */, const float* w_pen /* [B] or NULL */,
                  const float* w_con /* [B] or NULL */, int mean_contact, float* penetration /* [B] */, float* contact_sum /* [B] */,
                  int32_t* n_interior /* [B] */, int32_t* n_contact /* [B] */, float* grad_hand /* [B,V,3] or NULL */,
                  dvq_stream_t stream);
/* Penetration volume of grasps: the voxels, on a lattice of spacing h, whose centres lie both inside the (sealed) hand mesh and
 * inside the convex hull of the object -- an INTEGER per grasp, defined to the bit -- and the depth of the deepest hand vertex inside
 * the hull, in ONE kernel, one workgroup of 256 threads per grasp.  The counterpart of the reference's intersection_eval
 * (gen_diverse_grasp_obman.py:75-145, 265-279: igl + trimesh on the host, one grasp at a time, 1 mm voxels); it differs from it in
 * three stated ways: the hull is given as half-spaces (the caller builds it, e.g. from the sampled cloud: a lower bound of the mesh's
 * hull), the lattice is the object's own and not anchored at a bounding-box corner, and no igl / trimesh output pins parity.
 * Inputs: hand [B,V,3] contiguous fp32, posed, in the frame of its row; faces [F,3] int32, the closed ("sealed") triangle list with
 * indices in [0, V+L): vertex V+l is the fan centre of boundary loop l; loop_off [L+1], loop_vert [n_loop] int32: the loops'
 * vertices (CSR, indices in [0, V)), L >= 0; planes [n_planes,4] fp32 rows (nx, ny, nz, d): x is inside the hull of object o iff
 * n.x <= d for every plane of rows plane_off[o] .. plane_off[o+1] of the n_planes (plane_off int32 [O+1], CSR); obj_of_row int64 [B]; R [B,3,3] and
 * t [3]: the arguments dvq_transform_clouds got for these rows (the object was moved by x -> R x + t), or R = NULL (then t = NULL
 * too) for objects in place; h: the lattice spacing.
 * Everything is fp32; every operation is rounded on its own and "fma(a,b,c)" marks the only fused ones; "/" is the IEEE division;
 * comparisons with a NaN are false.  Per grasp b, with o = obj_of_row[b] and the planes of o:
 *   1. Fan centres (row frame): s = +0.0f; s = s + hand[loop_vert[q]] for q = loop_off[l] .. loop_off[l+1]-1 ascending, per component;
 *      vertex V+l = s / (float)len.
 *   2. Object frame, for all V+L vertices: with R, u = v - t per component (u = v when t is NULL) and v_o[i] = fma(R[2][i], u[2],
 *      fma(R[1][i], u[1], R[0][i] * u[0])) (that is R^T u); without R, v_o = v bit for bit.  The lattice below is therefore the
 *      object's own: a grasp's result depends on neither B, nor its row, nor which objects share the call.
 *   3. Lattice and box: c(i) = ((float)i + 0.5f) * h.  Per axis, with mn / mx the smallest / largest v_o component over the V+L
 *      vertices: lo = (int)floorf(mn / h) - 1, hi = (int)floorf(mx / h) + 1; the box is the cells lo .. hi of the three axes.
 *   4. Projected area of triangle (a,b,c) (indices as listed in `faces`): A = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax).
 *   5. Edge value at column (x,y) = (c(i), c(j)): every edge is evaluated in its canonical direction, the lower vertex index P first,
 *      e = (Qx-Px)*(y-Py) - (Qy-Py)*(x-Px), so the two triangles on an edge see the same bits.  A triangle that traverses the edge
 *      P -> Q uses w = e, one that traverses it Q -> P uses w = -e.
 *   6. Cover: the triangle covers the column iff A != 0 (and is no NaN), min(ax,bx,cx) <= x <= max(ax,bx,cx), the same for y, and
 *      every one of its three edges lies on A's side: for A > 0, w > 0, for A < 0, w < 0, where a value e of exactly 0 counts as
 *      positive iff Qy-Py < 0, or Qy-Py == 0 and Qx-Px > 0, and as negative otherwise (the differences as rounded in e).  That is the
 *      sign e takes at the column moved by (eps, eps^2): the tie is broken by the edge's SIDE, the same for every triangle at the
 *      edge whatever its traversal and the sign of its A, so the parity of a closed mesh survives a column through an edge --
 *      silhouette edges included -- or through a vertex.
 *   7. Crossing height of a covering triangle, with wa, wb, wc the values w of the edges b->c, c->a, a->b (opposite a, b, c):
 *      zc = ((wa * az + wb * bz) + wc * cz) / ((wa + wb) + wc).
 *   8. Voxel (i,j,k) is in the hand iff the number of covering triangles of its column with zc > c(k) is odd.
 *   9. Hull, per column: q = nx * x + ny * y, r = d - q; planes with nz < 0: z = r / nz, zlo = z where z > zlo (from -inf); planes
 *      with nz > 0: zhi = z where z < zhi (from +inf); every other plane rejects the whole column unless q <= d.  Voxel (i,j,k) of
 *      a column not rejected is in the hull iff zlo <= c(k) and c(k) <= zhi.
 *  10. count = the number of voxels of the box that are in both: an integer, free of any summation order.
 *  11. depth: per vertex v < V, g = the smallest over the planes of d - fma(nz, v_o.z, fma(ny, v_o.y, nx * v_o.x)) (from +inf, g' < g
 *      replaces); depth = the largest g over the vertices that exceeds +0.0f, else +0.0f: the exact deepest vertex inside a convex
 *      body, in the units of the input.
 *  12. status, the first that applies: 3 = a component of hand[b] is not finite (count = -1, depth = NaN); 1 = the object has no
 *      plane (count = 0, depth = 0); 2 = an axis of the box has more than 1024 cells, or a floorf of step 3 is beyond +-4194302 (NaN
 *      included), where (float)i + 0.5f stops being exact (count = -1, depth as in 11); 1 = no voxel of the box is in the hull
 *      (count = 0, depth = 0); else 0.
 * obj_of_row[b] outside [0, O) sets bit 0 of *err_flag (device int32, zeroed by the caller), as dvq_transform_clouds does; that row
 * reports count = -1, depth = NaN, status = 4.  Bit 1: a face index outside [0, V+L), a loop entry outside [0, V), an empty loop or one
 * whose offsets leave [0, n_loop] -- such a face or entry is skipped, such a loop's centre is +0 -- and an object with more than 8192
 * planes or a range that leaves [0, n_planes], whose rows report status 4 as well (plane_off lives on the device, so the launcher
 * cannot refuse it; the host's contact.pack_planes does).
 * B >= 0, 1 <= V <= 2048, 0 <= F <= 8192, 0 <= L <= 64, O >= 0, n_loop >= 0, n_planes >= 0, h finite and > 0, t only with R, no null
 * pointer otherwise; anything else is DVQ_EINVAL, nothing launched. */
int dvq_grasp_volume(const float* hand /* [B,V,3] */, int V, const int32_t* faces /* [F,3] */, int F, const int32_t* loop_off /* [L+1] */,
                     const int32_t* loop_vert, int L, int n_loop, const float* planes /* [n_planes,4] */, int n_planes,
                     const int32_t* plane_off /* [O+1] */, int64_t O, const int64_t* obj_of_row /* [B] */, const float* R /* [B,3,3] or NULL */,
                     const float* t /* [3] or NULL */, int64_t B, float h, int32_t* count /* [B] */, float* depth /* [B] */,
                     int32_t* status /* [B] */, int32_t* err_flag, dvq_stream_t stream);
/* Penetration depth of grasps against the object's MESH: the hand vertices that lie inside the closed triangle mesh of the row's
 * object (a parity test along +z) and, of those, the largest distance to the mesh's surface -- in ONE kernel, one workgroup of 256
 * threads per grasp.  The counterpart of the reference's metric/penetration.py (metric/contactutils.py: batch_mesh_contains_points,
 * then the largest distance of an inside vertex to the surface); it differs from it in one stated way: the ray runs along +z and a
 * column through a mesh edge or a mesh vertex is decided by the tie rule of dvq_grasp_volume (the reference casts an oblique ray with
 * strict inequalities and loses exactly those columns).  The depth of dvq_grasp_volume is against the convex HULL; this one sees holes
 * and handles.  An open mesh is not refused: its parity is then undefined.
 * Inputs: hand [B,V,3] contiguous fp32, posed, in the frame of its row; mesh_verts [n_mv,3] fp32 and vert_off int32 [O+1] (CSR: the
 * vertices of object o are rows vert_off[o] .. vert_off[o+1]-1); mesh_faces [n_mf,3] int32 and face_off int32 [O+1] (CSR likewise), the
 * indices LOCAL to the object's vertex range; obj_of_row int64 [B]; R [B,3,3] and t [3]: the arguments dvq_transform_clouds got for
 * these rows, or R = NULL (then t = NULL too) for objects in place, exactly as dvq_grasp_volume takes them.
 * Everything is fp32; every operation is rounded on its own and "fma(a,b,c)" marks the only fused ones; "/" is the IEEE division;
 * comparisons with a NaN are false; dot(u,w) = fma(u.z, w.z, fma(u.y, w.y, u.x * w.x)).  Per grasp b, with o = obj_of_row[b]:
 *   1. Object frame: step 2 of dvq_grasp_volume for the V hand vertices, bit for bit (p = R^T (v - t), or p = v without R).
 *   2. Inside: a face (a,b,c) of object o covers the column (x,y) = (p.x, p.y) by rules 4 - 6 of dvq_grasp_volume (the projected
 *      area, the edges in their canonical direction -- the lower LOCAL vertex index first -- with a value of exactly 0 decided by the
 *      edge's side, and the xy bounds), and its crossing height zc is rule 7's.  The vertex is inside iff the number of covering faces
 *      with zc > p.z is odd.
 *   3. Distance, for inside vertices only: per face the squared distance to its closest point q, by the regions of Ericson, Real-Time
 *      Collision Detection 5.1.5, in his order, the first that applies: ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c,
 *      cb = c - b per component; d1 = dot(ab,ap), d2 = dot(ac,ap), d3 = dot(ab,bp), d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp);
 *      vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4; u = d4 - d3, w = d5 - d6;
 *        d1 <= 0 and d2 <= 0:              q = a;
 *        d3 >= 0 and d4 <= d3:             q = b;
 *        vc <= 0, d1 >= 0 and d3 <= 0:     s = d1 / (d1 - d3), q = fma(s, ab, a) per component;
 *        d6 >= 0 and d5 <= d6:             q = c;
 *        vb <= 0, d2 >= 0 and d6 <= 0:     s = d2 / (d2 - d6), q = fma(s, ac, a);
 *        va <= 0, u >= 0 and w >= 0:       s = u / (u + w), q = fma(s, cb, b);
 *        otherwise:                        n = (va + vb) + vc, s = vb / n, r = vc / n, q = fma(r, ac, fma(s, ab, a));
 *      e = p - q per component, dist2 = dot(e,e).  The vertex's dist2 is the smallest over the faces in ascending order (from +inf,
 *      d' < d replaces: a NaN never does) and its face the lowest LOCAL face index that attains it, -1 if none replaced.
 *   4. Per row: n_inside = the number of inside vertices; over them in ascending order the first and then every one with a larger
 *      dist2 replaces: depth = sqrtf of that dist2, deep_vertex its index, deep_face its face; with none +0.0f, -1, -1.
 *   5. inside_mask: bit (v & 31) of word (v >> 5) is "v is inside"; the unused high bits of the last word are 0; W = (V + 31) / 32 words
 *      per grasp, as dvq_grasp_parts lays out its mask.  vert_d2 / vert_face: step 3's two figures per vertex, +inf / -1 for a vertex
 *      outside.
 *   6. status, the first that applies: 4 = obj_of_row[b] is outside [0, O) (bit 0 of *err_flag, a device int32 zeroed by the caller),
 *      or the object's vertex or face range leaves [0, n_mv] / [0, n_mf] or holds more than DVQ_GRASP_MESH_MAX_FACES faces (bit 1; the
 *      offsets live on the device, so the launcher cannot refuse them); 3 = a component of hand[b] is not finite; both report
 *      n_inside = -1, depth = NaN, deep_vertex = deep_face = -1, mask 0, vert_d2 NaN, vert_face -1.  1 = the object has no face:
 *      n_inside = 0, depth = +0.0f, mask 0 and what "no vertex inside" gives the rest (-1, -1, +inf, -1).  0 otherwise.
 * A face with an index outside the object's vertex range sets bit 1 of *err_flag and is skipped in steps 2 and 3.  A face with a NaN
 * coordinate covers nothing and is never nearest: that follows from the comparisons and needs no rule of its own.
 * Only a parity, minima, a maximum and bits are produced -- no float sum -- so nothing depends on a reduction order or a schedule,
 * and a grasp's outputs depend on neither B, nor its row, nor which objects share the call.
 * Outputs: n_inside int32 [B]; depth fp32 [B]; deep_vertex, deep_face int32 [B]; inside_mask int32 [B,W]; status int32 [B]; vert_d2
 * fp32 [B,V] and vert_face int32 [B,V], each of which may be NULL (not written).
 * B >= 0, 1 <= V <= 2048, O >= 0, n_mv >= 0, n_mf >= 0, t only with R, no null pointer but R, t, the two optional outputs and the
 * arrays of an empty pool; anything else is DVQ_EINVAL, nothing launched.  (B = 0 returns DVQ_OK before any pointer is looked at.) */
#define DVQ_GRASP_MESH_MAX_FACES 262144
int dvq_grasp_mesh(const float* hand /* [B,V,3] */, int V, const float* mesh_verts /* [n_mv,3] */, int n_mv,
                   const int32_t* vert_off /* [O+1] */, const int32_t* mesh_faces /* [n_mf,3] local indices */, int n_mf,
                   const int32_t* face_off /* [O+1] */, int64_t O, const int64_t* obj_of_row /* [B] */,
                   const float* R /* [B,3,3] or NULL */, const float* t /* [3] or NULL */, int64_t B, int32_t* n_inside /* [B] */,
                   float* depth /* [B] */, int32_t* deep_vertex /* [B] */, int32_t* deep_face /* [B] */,
                   int32_t* inside_mask /* [B,W] */, int32_t* status /* [B] */, float* vert_d2 /* [B,V] or NULL */,
                   int32_t* vert_face /* [B,V] or NULL */, int32_t* err_flag, dvq_stream_t stream);
/* Penetration volume of grasps against the object's MESH: the voxels, on the lattice of dvq_grasp_volume, whose centres lie both
 * inside the (sealed) hand mesh and inside the closed triangle mesh of the row's object -- an INTEGER per grasp, defined to the bit --
 * in ONE kernel, one workgroup of 256 threads per grasp.  dvq_grasp_volume counts against the object's convex HULL, which swallows the
 * hollow of a cup and the hole of a handle; this one sees them.  It is the solid intersection on the object's own lattice: NOT the
 * reference's metric/intersect.py figure (trimesh's SURFACE voxels of the object inside the hand), and no igl / trimesh output pins
 * parity.  An open mesh is not refused: its parity, and with it the count, is then undefined.
 * Inputs: hand, faces, loop_off, loop_vert, R, t, h exactly as dvq_grasp_volume takes them; mesh_verts, vert_off, mesh_faces (indices
 * LOCAL to the object's vertex range), face_off exactly as dvq_grasp_mesh takes them; obj_of_row int64 [B].
 * Arithmetic as in dvq_grasp_volume.  Per grasp b, with o = obj_of_row[b] and the faces of o:
 *   1 - 8. Steps 1 - 8 of dvq_grasp_volume, verbatim: the fan centres, the object frame, the lattice c(i) and the box from the HAND's
 *      V+L vertices (cells lo .. hi of the three axes), and which voxels of the box are in the hand.
 *   9'. Voxel (i,j,k) of the box is in the object iff the number of object faces that count for it is odd.  A face (a,b,c) counts iff
 *      it covers the column (c(i), c(j)) by rules 4 - 6 -- its edges in canonical direction by the lower LOCAL vertex index, a value
 *      of exactly 0 decided by the edge's side, as dvq_grasp_mesh takes them -- and its crossing height zc of rule 7 exceeds c(k),
 *      unless az <= c(lo_z), bz <= c(lo_z) and cz <= c(lo_z) all hold: a face wholly at or below the lowest cell centre never counts
 *      (no crossing of it exceeds a cell centre but for rounding; the rule takes the rounding out, so that such faces can be dropped
 *      before any column is looked at).  A face wholly above the box still counts: it flips its whole column.
 *  10'. count = the number of voxels of the box that are in both: an integer, free of any summation order.  No depth is produced: the
 *      depth against the mesh is dvq_grasp_mesh's figure.
 *  11'. status, the first that applies: 4 = obj_of_row[b] is outside [0, O) (bit 0 of *err_flag, a device int32 zeroed by the caller),
 *      or the object's vertex or face range leaves [0, n_mv] / [0, n_mf] or holds more than DVQ_GRASP_MESH_MAX_FACES faces (bit 1):
 *      count = -1; 3 = a component of hand[b] is not finite: count = -1; 1 = the object has no face: count = 0; 2 = the box is refused
 *      exactly as dvq_grasp_volume refuses it: count = -1; 1 = no voxel of the box is in the object: count = 0; else 0.
 * In a row that reaches step 9', a face with an index outside the object's vertex range sets bit 1 of *err_flag and is skipped.  A face
 * with a NaN coordinate covers nothing, or has a NaN crossing that exceeds no cell centre: that follows from the comparisons.  Bit 1
 * is also what dvq_grasp_volume sets for the hand's topology (a face index outside [0, V+L), a loop entry outside [0, V), an empty loop).
 * Object coordinates are arbitrary (1e30, infinities): a face's column range is cut to the box before anything is converted to an
 * integer, which changes no result -- the bounds test of rule 6 decides.
 * Only integers and bits are produced, so nothing depends on a reduction order or a schedule, and a grasp's outputs depend on neither B,
 * nor its row, nor which objects share the call.
 * Outputs: count, status int32 [B].
 * B >= 0, 1 <= V <= 2048, 0 <= F <= 8192, 0 <= L <= 64, O >= 0, n_loop >= 0, n_mv >= 0, n_mf >= 0, h finite and > 0, t only with R, no
 * null pointer but R, t and the arrays of an empty pool; anything else is DVQ_EINVAL, nothing launched.  (B = 0 returns DVQ_OK before
 * any pointer is looked at.) */
int dvq_grasp_mesh_volume(const float* hand /* [B,V,3] */, int V, const int32_t* faces /* [F,3] */, int F,
                          const int32_t* loop_off /* [L+1] */, const int32_t* loop_vert, int L, int n_loop,
                          const float* mesh_verts /* [n_mv,3] */, int n_mv, const int32_t* vert_off /* [O+1] */,
                          const int32_t* mesh_faces /* [n_mf,3] local indices */, int n_mf, const int32_t* face_off /* [O+1] */,
                          int64_t O, const int64_t* obj_of_row /* [B] */, const float* R /* [B,3,3] or NULL */,
                          const float* t /* [3] or NULL */, int64_t B, float h, int32_t* count /* [B] */, int32_t* status /* [B] */,
                          int32_t* err_flag, dvq_stream_t stream);
/* Per-object selection: cls, key [O*M] (candidate c of object o at o * M + c) -> sel [O,keep]: the candidate indices (0 .. M-1) of
 * each object's keep best candidates, best first.  Candidate a ranks before b iff (cls, key, index) is smaller: cls as signed
 * integers; within a class a NaN key sorts after every number and -0.0 == +0.0; the index breaks every tie.  One workgroup per
 * object; a candidate's rank is the count of candidates before it (O(M^2), deterministic, no workspace).
 * O >= 0, 1 <= keep <= M <= 4096; anything else is DVQ_EINVAL. */
int dvq_segment_topk(const int32_t* cls /* [O*M] */, const float* key /* [O*M] */, int64_t O, int M, int keep,
                     int64_t* sel /* [O,keep] */, dvq_stream_t stream);
/* Diverse selection inside a quality pool: greedy farthest-point (k-centre) order of each object's P best-ranked candidates, the
 * first `keep` picks written.  One workgroup per object, no workspace; nothing depends on O, on which objects share a call or on
 * scheduling.  New here: the reference only measures diversity (diverse_grasp/diversity.py:7-15), it does not select for it.
 * Inputs, per object o: feature rows x_c = feat[(o * M + c) * ld .. + D) of candidates c = 0 .. M-1 (fp32, row stride ld >= D floats);
 * pool[o, 0 .. P): distinct candidate indices in rank order (dvq_segment_topk with keep = P; duplicates are the caller's business).
 * Distance d(a, b): eight fp32 partial sums acc[0 .. 7] = +0.0f; for j = 0 .. D-1 ascending: t = a[j] - b[j], acc[j mod 8] =
 *   acc[j mod 8] + t * t, every operation rounded to fp32 on its own (nothing fused);
 *   d = ((acc0 + acc1) + (acc2 + acc3)) + ((acc4 + acc5) + (acc6 + acc7)).  d(a, b) == d(b, a) bit for bit.
 * A pool row is invalid when any of its D features is not finite.
 * Selection: pick 0 is pool position 0; then mind[i] = d(x_i, x_pick0) for every pool position i.  For r = 1 .. keep-1:
 *   key(i) = mind[i] for valid, unpicked i whose mind[i] is not NaN, else -1.0f; pick r = the unpicked position of the largest key,
 *   the lowest position among equals; then mind[i] = d < mind[i] ? d : mind[i] with d = d(x_i, x_pick_r) (a NaN lowers nothing).
 *   So exact duplicates (key 0) follow every distinct row, and invalid rows come last, in rank order.
 * Outputs [O,keep]: sel = the candidate index pool[o, pick_r]; rank = the pool position pick_r; gap = the key when picked: the
 *   squared distance to the nearest earlier pick, -1.0f for pick 0 and for picks whose key was -1 (-1 = not a distance).  Over the
 *   valid picks gap[1:] is non-increasing and its minimum is the kept set's smallest pairwise distance, bit for bit.
 * A pool entry outside [0, M) sets bit 0 of *err (device int32, zeroed by the caller) and that object's outputs are all -1; no
 * feature row of the object is read.
 * O >= 0, 1 <= keep <= P <= M <= 4096, 1 <= D <= 4096, ld >= D, no null pointer; anything else is DVQ_EINVAL, nothing launched. */
int dvq_segment_diverse(const float* feat, int64_t ld, int D, const int64_t* pool /* [O*P] */, int64_t O, int M, int P, int keep,
                        int64_t* sel /* [O,keep] */, int32_t* rank /* [O,keep] */, float* gap /* [O,keep] */, int32_t* err,
                        dvq_stream_t stream);
/* Lloyd's k-means inside each segment: the statistic behind the reference's diversity figure (diverse_grasp/diversity.py:7-15:
 * 20 clusters over the [n,61] parameter vectors) as ONE deterministic run from given starting rows -- scipy's kmeans keeps the
 * best of 20 random starts, which no fixed definition can restate.  One workgroup per segment, the whole loop in one launch, no
 * workspace; nothing depends on O, on which segments share a call or on scheduling.
 * Inputs: feature rows x_i = feat[(o * M + i) * ld .. + D) of segment o, i = 0 .. M-1 (fp32, row stride ld >= D floats, read in
 * place); init[o, 0 .. k): row positions inside the segment; iters >= 0.
 * Valid row: a row is valid iff all D features are finite.  An invalid row gets assign = -1 and dist = NaN and takes part in nothing.
 * Distance: d(x, c) is the eight-chain squared distance of dvq_segment_diverse: acc[j mod 8] = acc[j mod 8] + (x[j] - c[j])^2 over
 *   ascending j, every operation rounded to fp32 on its own (nothing fused), d = ((acc0 + acc1) + (acc2 + acc3)) + ((acc4 + acc5)
 *   + (acc6 + acc7)).
 * Assign: best = 0; for j = 1 .. k-1 centre j replaces best iff d_j < d_best, or d_best is NaN and d_j is not: the lowest index wins
 *   ties and a NaN never wins over a number.  assign[i] = best, dist[i] = d_best.
 * Update: for each centre c and feature j four chains: chain g starts at +0.0f and adds x[i][j] over ascending segment positions
 *   i = g (mod 4) with assign[i] == c.  S = (ch0 + ch1) + (ch2 + ch3); centre[c][j] = S / (float)count[c] by IEEE division, count[c]
 *   the number of rows with assign == c.  A centre with count == 0 keeps its value.
 * Loop: 1. the centres start as the init rows.  2. assign every row.  3. for u = 1 .. iters: update, then assign again; stop when
 *   no assignment changed, with iters_used = u.  4. iters_used = iters when the limit ends the loop; iters = 0 gives 0.
 * Outputs: centres [O,k,D]; counts [O,k]; assign, dist [O*M]; iters_used [O].  assign, dist and counts are always those of the
 *   centres returned.
 * Bad init: an entry outside [0, M), a duplicate within a segment or an invalid row sets bit 0 of *err (device int32, zeroed by the
 *   caller); that segment's integer outputs are all -1 and its centres and dist NaN; no row of the segment is read through a bad index.
 * O >= 0, 1 <= k <= 64, 1 <= D <= 64, k <= M <= 262144, ld >= D, iters >= 0, no null pointer; anything else is DVQ_EINVAL, nothing
 * launched.  Vertex space (D = 2334) is out of scope: the accumulators of one workgroup would not fit in LDS. */
int dvq_segment_kmeans(const float* feat, int64_t ld, int D, const int64_t* init /* [O,k] */, int64_t O, int M, int k, int iters,
                       float* centres /* [O,k,D] */, int32_t* counts /* [O,k] */, int32_t* assign /* [O*M] */, float* dist /* [O*M] */,
                       int32_t* iters_used /* [O] */, int32_t* err, dvq_stream_t stream);
/* Object-side contact map: for every point of an object's cloud, over the grasps of that object, how many hands touch it, how many
 * have it inside, the nearest any hand comes and the summed touching distances -- the figure the reference's contact-map code is
 * built around (utils/utils.py get_pseudo_cmap: the object points' nearest-hand distances as a map over the object), reduced over a
 * segment of grasps on the device: no [B,N] intermediate.  ONE kernel that turns the scan of dvq_grasp_scores round: a workgroup
 * holds 1024 object points still and walks the segment's rows.  No workspace; nothing depends on O, on which segments share a call,
 * on B or on scheduling.
 * Inputs: hand [B,V,3] contiguous fp32, the topology and obj with strides in floats exactly as dvq_grasp_scores takes them (a
 * channel-first cloud is read in place); segment o is the K rows r(o,i) = rows[o * K + i], i = 0 .. K-1 (device int64 [O*K]); with
 * rows == NULL r(o,i) = o * K + i and B == O * K is required.  The hand and the cloud of row r are read in place: a row may appear in
 * several segments or several times in one.
 *   1. Row validity: a row is valid iff all 3 V hand coordinates and all 3 N cloud coordinates of that row are finite.
 *      row_status[o * K + i] = 0 for a valid row, 1 otherwise; n_valid[o] = the number of valid rows.  An invalid row takes part in
 *      nothing below.
 *   2. Per valid row and point p: normals, d_p, j_p and inside_p exactly as dvq_grasp_scores defines them (nearest vertex with the
 *      lowest index on ties, the tangent-plane test against it): the same bits.
 *   3. touch[o,p] = the number of valid rows with d_p < contact_threshold; inside[o,p] = the number with inside_p; dmin[o,p] = the
 *      minimum of d_p over the valid rows, +inf with none.
 *   4. near_sum[o,p] = the sum of sqrtf(d_p) (IEEE square root) over the valid rows with d_p < contact_threshold, as four chains:
 *      chain g starts at +0.0f and adds over ascending segment positions i = g (mod 4); S = (c0 + c1) + (c2 + c3); every operation
 *      rounded to fp32 on its own, nothing fused (the chain rule of dvq_segment_kmeans).  The only float sum; its order is fixed by
 *      the segment positions.
 *   5. Bad index: an entry of rows outside [0, B) sets bit 0 of *err (device int32, zeroed by the caller); that segment's touch,
 *      inside, n_valid and row_status are -1, its dmin and near_sum NaN, and nothing is read through the bad index.
 * Outputs: touch, inside int32 [O,N]; dmin, near_sum fp32 [O,N]; n_valid int32 [O]; row_status int32 [O*K].
 * O >= 0, 1 <= K <= 262144, N >= 1, 1 <= V <= 2048, contact_threshold finite and > 0, no null pointer except rows; anything else is
 * DVQ_EINVAL, nothing launched.  O == 0 returns DVQ_OK before any pointer is looked at. */
int dvq_segment_contact(const float* hand /* [B,V,3] */, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_face, int V,
                        const float* obj, int64_t obj_batch_stride, int64_t obj_point_stride, int64_t obj_coord_stride,
                        int64_t B, int N, const int64_t* rows /* device [O*K] or NULL */, int64_t O, int K, float contact_threshold,
                        int32_t* touch /* [O,N] */, int32_t* inside /* [O,N] */, float* dmin /* [O,N] */, float* near_sum /* [O,N] */,
                        int32_t* n_valid /* [O] */, int32_t* row_status /* [O*K] */, int32_t* err, dvq_stream_t stream);

/* ------------------------------------------------------------------ object clouds from meshes
 * Area-weighted random points on the surface of each object's triangle mesh: what the reference's datasets get from trimesh
 * (dataset/utils_HO3D_FPHA.py:61-73, trimesh.sample.sample_surface(obj_mesh, 3000)), defined here to the bit.  It is NOT trimesh's
 * stream: that one comes from numpy's global generator and a float64 cumulative sum, which no other library can restate; this is the
 * same distribution (up to the weight quantisation below) from the library's own keyed Philox generator.  Two launches: one workgroup
 * per object for the weights and their prefix sum, then one thread per (object, sample).
 * Inputs: the four CSR tables exactly as dvq_grasp_mesh takes them (mesh_verts [n_mv,3] fp32, vert_off int32 [O+1], mesh_faces
 * [n_mf,3] int32 LOCAL indices, face_off int32 [O+1]); S samples per object; seed; stream_ids int64 [O]: the object's GLOBAL index,
 * as the prior's noise keys use it (dvq_exp1_noise_keyed); cdf uint64 [n_mf]: the caller's, the only workspace and also an output.
 * Everything is fp32; every operation is rounded on its own, nothing is fused; "/" is the IEEE division and sqrtf the IEEE square
 * root.  Per object o, over its faces f = 0 .. nf-1 (a, b, c = the face's three vertices):
 *   1. Face weight: e1 = b - a, e2 = c - a per component; n = e1 x e2: n.x = e1.y * e2.z - e1.z * e2.y, n.y = e1.z * e2.x - e1.x *
 *      e2.z, n.z = e1.x * e2.y - e1.y * e2.x, each product and each difference rounded alone; w = sqrtf((n.x * n.x + n.y * n.y) +
 *      n.z * n.z) (twice the area); a w that is not finite counts as 0, and so does the w of a face with an index outside the
 *      object's vertices (bit 1 of *err_flag, as in dvq_grasp_mesh; nothing is read through the index).  amax = the object's largest w.
 *      q_f = 0 if w == 0, else 1 + (uint32)truncf((w / amax) * 1048575.0f): an integer in [1, 2^20].
 *      cdf[face_off[o] + f] = q_0 + .. + q_f as uint64 (the inclusive sum in ascending order); T = the last one.
 *      The weights are INTEGERS on purpose: an integer prefix sum is exact and associative, so any parallel scan gives the same bits.
 *      The price is a bias: a face is drawn with probability q_f / T in place of w_f / sum w, and q_f is off from its exact share by
 *      less than one unit, i.e. by less than 2^-20 of the LARGEST face's share, per face.
 *   2. Draw for sample s = 0 .. S-1: X = Philox4x32-10 of counter (0xFFFFFFF0, s, 0, stream_ids[o]) under the key (seed low, seed
 *      high): the generator of dvq_exp1_noise.  The tag word keeps these draws apart from the prior's noise, whose first counter word
 *      is a column quad below 2^31.  t = the high 64 bits of the 128-bit product ((X0 << 32) | X1) * T, so 0 <= t < T; the face is the
 *      smallest f with cdf[f] > t.  A face with q_f = 0 is never drawn.
 *   3. Point: r1 = ((float)(X2 >> 8) + 0.5f) * 2^-24, r2 likewise from X3; if r1 + r2 > 1.0f then r1 = 1.0f - r1 and r2 = 1.0f - r2
 *      (trimesh's fold of the unit square onto the triangle); p = (a + r1 * e1) + r2 * e2 per component.
 *   4. status[o], the first that applies: 4 = the object's vertex or face range leaves [0, n_mv] / [0, n_mf] or holds more than
 *      DVQ_GRASP_MESH_MAX_FACES faces (bit 1 of *err_flag), or stream_ids[o] is outside [0, 2^32) (bit 0): no cdf word of the object is
 *      written; 1 = T == 0 (no face with area); both give points NaN and face -1.  0 otherwise.
 * A sample's bits depend on (seed, stream id, s, the object's mesh) only: not on O, not on which objects share the call, not on S.
 * Outputs: points fp32 [O,S,3]; face int32 [O,S]: the LOCAL face index; status int32 [O]; cdf as above.
 * O >= 0, 1 <= S <= DVQ_MESH_SAMPLE_MAX_S, O * ceil(S / 256) < 2^31, n_mv >= 0, n_mf >= 0, no null pointer but the arrays of an
 * empty pool; anything else is DVQ_EINVAL, nothing launched.  (O = 0 returns DVQ_OK before any pointer is looked at.) */
#define DVQ_MESH_SAMPLE_MAX_S 1048576
int dvq_mesh_sample(const float* mesh_verts /* [n_mv,3] */, int n_mv, const int32_t* vert_off /* [O+1] */,
                    const int32_t* mesh_faces /* [n_mf,3] local indices */, int n_mf, const int32_t* face_off /* [O+1] */, int64_t O,
                    int S, uint64_t seed, const int64_t* stream_ids /* device [O] */, uint64_t* cdf /* [n_mf] */,
                    float* points /* [O,S,3] */, int32_t* face /* [O,S] */, int32_t* status /* [O] */, int32_t* err_flag,
                    dvq_stream_t stream);
/* Farthest-point subsampling of a 3-D pool: the greedy k-centre order of dvq_segment_diverse for point clouds, where that one stops
 * at 4096 rows and walks a generic D.  One workgroup of 1024 threads per object, the pool in registers, no workspace; nothing depends
 * on O, on which objects share a call or on scheduling.  New here: the reference uses its random samples as they come.
 * Inputs: points fp32 [O,P,3] contiguous.  Distance: dx = x_i - x_j (likewise dy, dz), d = ((dx * dx) + (dy * dy)) + (dz * dz), every
 * operation rounded to fp32 on its own, nothing fused.
 * Selection: pick 0 is pool position 0; then mind[i] = d(i, pick 0) for every position i.  For r = 1 .. keep-1: pick r = the unpicked
 *   position of the largest mind, the lowest position among equals; gap[r] = that mind; then mind[i] = d < mind[i] ? d : mind[i] with
 *   d = d(i, pick r).  gap[0] = -1.0f.  So exact duplicates of a pick (mind 0) come last, in position order; gap[1:] is non-increasing
 *   and its minimum is the kept set's smallest pairwise distance, bit for bit.
 * A pool with a coordinate that is not finite: status[o] = 1, sel all -1, gap all -1.0f.  status[o] = 0 otherwise.
 * Outputs: sel int32 [O,keep]: pool positions in pick order; gap fp32 [O,keep]; status int32 [O].
 * O >= 0, 1 <= keep <= P <= DVQ_CLOUD_FPS_MAX_P, no null pointer; anything else is DVQ_EINVAL, nothing launched. */
#define DVQ_CLOUD_FPS_MAX_P 16384
int dvq_cloud_fps(const float* points /* [O,P,3] */, int64_t O, int P, int keep, int32_t* sel /* [O,keep] */,
                  float* gap /* [O,keep] */, int32_t* status /* [O] */, dvq_stream_t stream);

/* ------------------------------------------------------------------ all-gather of the generated MANO parameters (multi-GPU)
 * The batch of objects shards contiguously over R ranks (one process per GPU); the only exchange of the path is
 * the all-gather of the [B/R, 61] parameter rows (61-parameter assembly, gen_diverse_grasp_obman.py:243-247) into [B, 61],
 * rank-major: RCCL over xGMI.  The reference has no distributed code (nothing to replace); the op is new.
 *   dvq_comm_unique_id : rank 0 makes the 128-byte id; the caller hands it to every rank (any side channel)
 *   dvq_comm_init      : every rank, on its own device (hipSetDevice first): the communicator
 *   dvq_allgather_params: out[r * rows_per_rank + i, :] = rank r's local[i, :]; enqueued on `stream`; equal shards only
 *                        (ragged batches: pad the shard, the host mirror does)
 * RCCL is resolved at the first call (dlopen); without it these return DVQ_ENODEVICE and the rest of the library is unaffected. */
/* 1 when librccl and the six entry points used here resolve in this process, else 0: a probe that creates nothing (v8; making a
 * unique id starts RCCL's bootstrap thread and socket, which only rank 0 should do) */
int dvq_comm_available(void);
int dvq_comm_unique_id(void* id_out, size_t id_bytes /* >= 128 */);
int dvq_comm_init(const void* id, size_t id_bytes, int world, int rank, void** comm_out);
int dvq_allgather_params(void* comm, const float* local /* [rows_per_rank, cols] */, int64_t rows_per_rank, int cols /* 61 */,
                         float* out /* [world * rows_per_rank, cols] */, dvq_stream_t stream);
/* ranks of the communicator as RCCL reports them (ncclCommCount; v9): lets a caller show that the collective really spans N processes */
int dvq_comm_count(void* comm, int* ranks_out);
int dvq_comm_destroy(void* comm);

/* ------------------------------------------------------------------ optional per-launch timing
 * When enabled, every kernel launch of the library is bracketed by two HIP events on its stream.
 * dvq_prof_read waits for the recorded events and returns per-kernel-kind totals (bench.py's roofline leg). */
typedef struct {
    char name[32];
    int64_t count;
    double ms;     /* summed launch durations */
    double flops;  /* summed algorithmic FLOPs  */
    double bytes;  /* summed algorithmic bytes  */
} dvq_prof_entry;
int dvq_prof_enable(int on);
int dvq_prof_reset(void);
int dvq_prof_read(dvq_prof_entry* out, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* DVQ_H */
