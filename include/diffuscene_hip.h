/*
 * diffuscene_hip.h -- C ABI of libdiffuscene_hip.so (gfx950 / MI355X).
 *
 * The reference (tangjiapeng/DiffuScene) has no FFI on this path: its DDPM hot path is pure
 * PyTorch (scene_synthesis/networks/denoise_net.py, diffusion_ddpm.py, loss.py).  The drop-in
 * boundary is therefore the Python class surface; this header is the
 * thin C layer underneath it.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless stated; the caller (PyTorch) owns all
 *    memory, the library allocates nothing and keeps no global state;
 *  - activations are token-major: row = b * N + n (scene b, object slot n), channels contiguous.
 *    The reference's (B, C, N) conv layout is never materialised;
 *  - every call enqueues on `stream` and returns immediately (capturable in a hipGraph);
 *  - return value: 0 on success, a negative DSC_E* code for rejected arguments, or a positive
 *    hipError_t from the launch.  Nothing is silently clamped.
 */
#ifndef DIFFUSCENE_HIP_H
#define DIFFUSCENE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dsc_stream_t; /* hipStream_t */

#define DSC_EINVAL   (-1)  /* bad shape / null pointer */
#define DSC_EALIGN   (-2)  /* pointer or leading dimension not 16-byte aligned where required */
#define DSC_ERANGE   (-3)  /* size outside what the kernel supports (e.g. tokens_per_scene > 160) */

#define DSC_ACT_NONE 0
#define DSC_ACT_GELU 1   /* exact erf GELU (nn.GELU default) */
#define DSC_ACT_SILU 2
#define DSC_ACT_LEAKY01 3 /* nn.LeakyReLU(0.1): the condition MLPs of diffusion_scene_layout_ddpm.py:94-125 (elementwise kernels) */

#define DSC_SS_NONE      0
#define DSC_SS_PER_TOKEN 1   /* scale_shift row = token           (context-conditioned ResnetBlock) */
#define DSC_SS_PER_SCENE 2   /* scale_shift row = token / N       (time-conditioned ResnetBlock)    */
#define DSC_SS_PER_SLOT  3   /* scale_shift row = token % N       (instance embedding shared over B)*/
#define DSC_SS_BY_INDEX  4   /* scale_shift row = ss_index[token / N]  (per-timestep table while sampling) */

#define DSC_HEADS    4
#define DSC_DIM_HEAD 32

int dsc_version(void);

/* ---------------------------------------------------------------------------------------------
 * fp32 MFMA GEMM with fused epilogues:  Y = epilogue( [A1 | A2] . W^T + bias )
 *
 * Replaces every 1x1 nn.Conv1d / nn.Linear on the path (denoise_net.py:163,183,188,214,217,244,
 * 245,397,419-421,440,459,487-503) including the torch.cat of skip connections (:562,:566,:573),
 * which becomes the second K segment.  Arithmetic: v_mfma_f32_32x32x2_f32, exact fp32.
 *   k1, k2 multiples of 32; a1/a2/w rows 16-byte aligned.  y/residual may have any alignment.
 *   batch > 1 launches a grouped GEMM: group z uses pointers advanced by the s* element strides.
 * ------------------------------------------------------------------------------------------- */
typedef struct dsc_gemm_args {
    const float* a1; int64_t lda1; int32_t k1;
    const float* a2; int64_t lda2; int32_t k2;   /* k2 = 0 -> single segment */
    const float* w;  int64_t ldw;                /* [n][k1+k2] */
    const float* bias;                           /* [n] or NULL */
    const float* residual; int64_t ldr;          /* added after act_out, or NULL */
    float* y; int64_t ldy;
    int32_t m, n;
    int32_t act_in;                              /* reserved, must be DSC_ACT_NONE (apply dsc_activation_f32 to A first) */
    int32_t act_out;
    int32_t batch; int64_t sa1, sa2, sw, sbias, sres, sy;
    /* ---- GroupNorm epilogue (dsc_gemm_gn_silu_f32 only) ---- */
    const float* gamma; const float* beta; float eps;
    int32_t tokens_per_scene;                    /* N: GroupNorm reduces over 64 channels x N tokens (:164) */
    const float* scale_shift; int64_t ld_ss; int32_t ss_mode; /* row layout [scale(n) | shift(n)] */
    float* preact; int64_t ld_preact;            /* optional: pre-norm conv output z = [A1|A2].W^T + bias, saved for backward */
    const int64_t* ss_index;                     /* DSC_SS_BY_INDEX: device int64 per scene (the timestep vector t) */
    /* ---- optional: W pre-split into three bf16 planes [3][n][k1+k2] by dsc_split_bf16x3_f32 (same values as w) ----
     * (batch > 1: the planes [3][batch n][k] of the stacked weights, sw == n k.)
     * When set (and n % 128 == 0, 16-byte aligned y / bias / residual), dsc_gemm_f32 and dsc_gemm_gn_silu_f32 compute
     * the SAME f32 product on the bf16 matrix cores: both operands split exactly into 3 bf16 pieces, the 6 significant piece
     * products accumulated in f32 (error vs f64 <= the exact-f32 MFMA path's, ~1.5x faster).  NULL, an unsupported shape, or
     * dsc_get_gemm_arithmetic() == 0: the exact-f32 MFMA kernel runs.
     * Operand range of the split arithmetic (tests/test_gpu_split.py holds these): finite operands with |x| <= 3.3895e38 (the largest
     * bf16) give the f32 product at any magnitude and any mix of magnitudes inside a K row; pieces below the bf16 subnormal range
     * (third pieces of |x| < ~1e-33) may be flushed by the matrix cores: an absolute error <= 2^-16 |x w| on such terms, invisible
     * next to any normal-range term.  An operand that is +-inf, NaN or above the largest bf16 makes its first piece inf and its
     * residual pieces NaN, and a product that overflows f32 may meet an oppositely signed piece product: the affected outputs are
     * non-finite in both arithmetics, but NaN where the exact-f32 kernel may give +-inf. */
    const uint16_t* w_planes;
    /* ---- training-step epilogues of dsc_gemm_f32, implemented by the split-bf16 kernel only (a launch that sets them and does not
     * qualify for that kernel -- dsc_gemm_arithmetic() == 0 -- fails with DSC_EINVAL, it is never silently ignored):
     *   preact (above) with act_out != NONE : the pre-activation u = [A1|A2].W^T + bias is ALSO stored there, y = act_out(u)
     *                                         (Linear + GELU / SiLU of the encoder / decoder MLPs in one launch, u kept for backward)
     *   actgrad_x != NULL                   : y = ([A1|A2].W^T) * act_out'(actgrad_x[row][col]) (+ residual): the input-gradient GEMM
     *                                         of the NEXT layer applies the derivative of the activation whose saved pre-activation
     *                                         is actgrad_x (act_out names the activation; it is not applied to y) */
    const float* actgrad_x; int64_t ld_actgrad;
    /* DSC_SS_BY_INDEX: rows of the scale_shift table (>= 1).  Every gathered index is clamped into [0, ss_rows) on the device, so a
     * timestep vector left out of range (e.g. -1 after the last step of a captured reverse loop) cannot read outside the table. */
    int32_t ss_rows;
    /* Layout of w_planes (round 6): DSC_PLANES_ROWMAJOR = [3][n][K] (the block-staged split kernel stages them through LDS);
     * DSC_PLANES_FRAGMENT = [3][n/16][K/32][64 lanes][8]: one 1 KiB piece per (16-channel block, K tile, plane) in MFMA lane order, read
     * straight into registers by the wave-autonomous kernel (csrc/gemm_split_wave.h).  Which one a launch wants is the library's
     * decision -- ask dsc_gemm_planes_layout() BEFORE making the planes; a launch whose planes have the other layout fails with
     * DSC_EINVAL (it is never computed on the wrong bytes, never silently sent to another kernel). */
    int32_t w_planes_layout;
    /* ---- GroupNorm-backward epilogue of dsc_gemm_f32 (round 6; wave-autonomous kernel only: DSC_TILE_WAVE_DENSE with rows = whole scenes of 65..80 tokens) ----
     * The product P = [A1|A2].W^T is the gradient w.r.t. the OUTPUT of a fused Block (dsc_gemm_gn_silu_f32) whose saved pre-norm activation is gnb_z; y receives
     * the gradient w.r.t. that pre-norm activation -- what dsc_gn_silu_bwd_f32 computes from (gnb_z, P) -- and the per-scene partial sums go to gnb_dgamma /
     * gnb_dbeta / gnb_dbias (row b at + b * gnb_pstride) and, with DSC_SS_PER_SCENE, the per-scene d(scale, shift) to gnb_dss ([scenes][2 n] rows of ld_gnb_dss).
     * gamma, beta, eps, tokens_per_scene, scale_shift, ld_ss, ss_mode describe that Block (ss_mode DSC_SS_NONE or DSC_SS_PER_SCENE); bias, act_out, residual,
     * preact and actgrad_x must be unset.  A launch that sets gnb_z and does not qualify fails with DSC_EINVAL (dsc_gemm_split_tile tells beforehand). */
    const float* gnb_z; int64_t ld_gnb_z;
    float* gnb_dgamma; float* gnb_dbeta; float* gnb_dbias; int64_t gnb_pstride;
    float* gnb_dss; int64_t ld_gnb_dss;
    /* DSC_GEMM_ROW_INVARIANT: every output row must come out exactly as in a launch of the same product with any other number of rows --
     * a table built once with m = T rows stands in for per-step launches with m = B rows (the tabulated time MLP of the reverse loops,
     * engine.ss_table), and a captured loop must reproduce the eager loop bit for bit.  Every kernel family whose choice or K association
     * depends on m refuses a flagged launch: the split-bf16 family (its tiles are chosen by m; w_planes is ignored, dsc_gemm_split_tile
     * answers -1, dsc_gemm_arithmetic 0 and dsc_gemm_planes_layout DSC_PLANES_NONE, so callers make no planes for it) and the K-parallel
     * kernel for small launches (it associates the K sum as eight slice sums; dsc_gemm_skinny answers 0).  The launch runs on ONE exact-f32
     * tile kernel whatever m is, the 64 x 64 tile (dsc_gemm_f32_tile answers DSC_F32_TILE_64x64): the five exact-f32 tiles share the K
     * order, but the 64 x 64 kernel adds the bias to the finished K sum while the four larger ones start their accumulators from the
     * bias, so a row with a bias differs between them in the last bit (measured: t_pack rows at m = 80, 330, 390, 420, 720 against the
     * m = 1000 launch, before the pin).  64 x 64 is the tile the m = T table launch and every batch of <= 64 scenes took before, so the pin
     * moves no result at those sizes.  A flagged launch larger than the table's pays for it with the smallest tile; it is meant for
     * products of a few hundred rows.  tests/test_gpu_row_invariant.py holds all of this at one m inside every dispatch class. */
    int32_t flags;
} dsc_gemm_args;
#define DSC_GEMM_ROW_INVARIANT 1
#define DSC_PLANES_ROWMAJOR 0
#define DSC_PLANES_FRAGMENT 1
#define DSC_PLANES_NONE (-100)   /* answer of dsc_gemm_planes_layout only: no planes wanted (never a value of w_planes_layout, never an error code) */

int dsc_gemm_f32(const dsc_gemm_args* args, dsc_stream_t stream);

/* Exact 3-way bf16 split of f32 matrices (x = x1 + x2 + x3, round-to-nearest at each step) for dsc_gemm_args.w_planes:
 *   planes[p][r][c], p = 0..2, each plane [rows][cols] bf16 (or [cols][rows] with transpose != 0: the planes of w^T, the weight
 * operand of the input-gradient GEMM dA = dY . W).  Output columns % 8 == 0.  items: HOST array, at most DSC_WS_MAX per call. */
/* Which arithmetic dsc_gemm_f32 (gn = 0) / dsc_gemm_gn_silu_f32 (gn != 0) would use for this launch: 1 = the split-bf16 kernel (planes
 * supplied, shape / alignment covered, launch large enough to fill the chip, DSC_GEMM != f32), 0 = the exact-f32 MFMA kernel. */
int dsc_gemm_arithmetic(const dsc_gemm_args* args, int32_t gn);

/* Which TILE of the split-bf16 kernel the launch would run on (-1: none, the exact-f32 MFMA kernel takes it).  Tests use it to say
 * which tile class a golden comparison exercised: the headline batch (B = 256, N = 80) runs the eight-wave GroupNorm tile, half of
 * it the four-wave one -- same K order and product order per output element, bit-identical results (tests/test_gpu_split.py). */
#define DSC_TILE_GN_32       0   /* 4 scenes of <= 32 tokens x 128 channels, 8 waves */
#define DSC_TILE_GN_80_W8    1   /* 2 scenes of 65..80 tokens x 256 channels, 8 waves */
#define DSC_TILE_GN_80_W4    2   /* 2 scenes of 65..80 tokens x 128 channels, 4 waves */
#define DSC_TILE_GN_48       3
#define DSC_TILE_GN_64       4
#define DSC_TILE_160x256     5   /* dense rows, 8 waves */
#define DSC_TILE_256x128     6
#define DSC_TILE_128x128     7
#define DSC_TILE_160x128_W4  8   /* dense rows, 4 waves */
#define DSC_TILE_64x256      9
#define DSC_TILE_WAVE_GN     10  /* wave-autonomous kernel: one scene of 17..80 tokens x 128 channels per wave, 4 waves per block */
#define DSC_TILE_WAVE_DENSE  11  /* the same on dense rows (groups of 80) */
#define DSC_TILE_WAVE_GN_64  12  /* half-size GroupNorm launches: one scene of 65..80 tokens x 64 channels per wave */
int dsc_gemm_split_tile(const dsc_gemm_args* args, int32_t gn);

/* Which TILE of the exact-f32 MFMA kernel dsc_gemm_f32 picks for the launch's shape: the kernel that runs when neither the split-bf16
 * family (dsc_gemm_split_tile) nor the K-parallel kernel (dsc_gemm_skinny) takes the launch.  Host only, launches nothing; a negative
 * DSC_E* code for arguments dsc_gemm_f32 would reject.  Tests use it to say which tiles a bit-for-bit comparison went through. */
#define DSC_F32_TILE_160x256 0   /* 8 waves */
#define DSC_F32_TILE_160x128 1
#define DSC_F32_TILE_128x128 2
#define DSC_F32_TILE_96x128  3
#define DSC_F32_TILE_64x64   4
int dsc_gemm_f32_tile(const dsc_gemm_args* args);

/* The planes layout the launch wants: DSC_PLANES_ROWMAJOR / DSC_PLANES_FRAGMENT, or DSC_PLANES_NONE when it stays on the exact-f32 kernel
 * whatever planes it is given (w_planes / w_planes_layout of `args` are not read; a DSC_GEMM_ROW_INVARIANT launch always does).  Invalid
 * arguments (null, m / n / k1 <= 0) answer DSC_EINVAL, which is none of the three. */
int dsc_gemm_planes_layout(const dsc_gemm_args* args, int32_t gn);

/* The wave-autonomous kernel family of the split arithmetic: 1 = used wherever a launch qualifies (default), 0 = never (every split
 * launch on the block-staged kernel: the round-3..5 behaviour).  Initial value from DSC_WAVE ("", "1", "auto" -> 1; "0" -> 0; anything
 * else -> DSC_EINVAL from get and from every GEMM launch).  Both families compute bit-identical results (tests/test_gpu_split.py). */
int dsc_get_split_wave(void);
int dsc_set_split_wave(int32_t mode);

/* The K-parallel exact-f32 kernel for launches too small to fill the chip (csrc/gemm_skinny.h, round 6): a block owns <= 32 token rows
 * (whole scenes) x 64 channels and splits K over its eight waves.  It takes a launch of dsc_gemm_f32 / dsc_gemm_gn_silu_f32 that stays on
 * the exact-f32 arithmetic when (k1 + k2) % 64 == 0, n % 64 == 0, scenes of <= 32 tokens, 16-byte aligned rows and ALL blocks fit one
 * round of the chip (the one-scene generation call of scripts/generate_diffusion.py:314-323, batches of a few scenes) -- same
 * products, the K sum associated as eight slice sums.  dsc_gemm_skinny: 0 = a tile kernel (or the split family) takes the launch,
 * 1 = this kernel with blocks of <= 32 rows, 2 = with blocks of <= 16 rows (v_mfma_f32_16x16x4_f32 tiles: scenes of <= 16 tokens, K % 512 == 0).  Switch: 1 = on (default), 0 = off; initial value from DSC_SKINNY ("0" -> off). */
int dsc_gemm_skinny(const dsc_gemm_args* args, int32_t gn);
int dsc_get_skinny(void);
int dsc_set_skinny(int32_t on);   /* returns the previous setting */

/* The arithmetic switch of dsc_gemm_f32 / dsc_gemm_gn_silu_f32 / the grouped weight-gradient launch chosen by the host code -- the ONE
 * source of truth (the Python engine, the training plan and bench.py ask this function, nothing else parses the environment):
 *   1 = split-bf16 wherever a launch qualifies (default), 0 = exact-f32 MFMA everywhere.
 * Initial value from the environment, strictly: DSC_GEMM unset, "" or "split" -> 1; "f32" -> 0; any other value -> get returns
 * DSC_EINVAL and every GEMM launch fails with DSC_EINVAL.  set(mode) switches it per call, process-wide (0 / 1, else DSC_EINVAL);
 * launches already captured in a hipGraph keep the kernels they were captured with. */
int dsc_get_gemm_arithmetic(void);
int dsc_set_gemm_arithmetic(int32_t mode);

/* transpose: bit 0 = planes of w^T; bit 1 (DSC_SPLIT_FRAGMENT) = fragment-major output (DSC_PLANES_FRAGMENT; output rows % 16 == 0,
 * output columns % 32 == 0) */
#define DSC_SPLIT_TRANSPOSE 1
#define DSC_SPLIT_FRAGMENT  2
typedef struct dsc_split_item { const float* w; int64_t ldw; int32_t rows, cols; uint16_t* planes; int32_t transpose; } dsc_split_item;
int dsc_split_bf16x3_f32(const dsc_split_item* items, int32_t count, dsc_stream_t stream);

/* Block.forward (denoise_net.py:167-176) as ONE kernel:
 *   Y = SiLU( GroupNorm8( [A1|A2].W^T + bias ) * (scale + 1) + shift ) (+ residual)
 * W must already be weight-standardised (dsc_weight_standardize_f32).  n must be a multiple of 128,
 * groups are 64 channels wide (nn.GroupNorm(8, 512)), m a multiple of tokens_per_scene <= 160. */
int dsc_gemm_gn_silu_f32(const dsc_gemm_args* args, dsc_stream_t stream);

/* Split-K form of dsc_gemm_f32 for short, deep products (few rows, K >= 1024): the K range is cut into `splits` equal parts
 * (k1 % (32 * splits) == 0) computed as the batch dimension of one launch into workspace slabs [splits][m][n], then summed in a
 * fixed order with bias / residual applied.  Restrictions: batch == 1, k2 == 0, act_out == DSC_ACT_NONE. */
int dsc_gemm_splitk_f32(const dsc_gemm_args* a, int32_t splits, float* workspace, int64_t workspace_floats, dsc_stream_t stream);

/* y = LayerNorm over the n = 512 output channels of ([a1 | a2] @ w^T + bias), times gamma, plus residual (optional): the
 * out-projection + LayerNorm (+ residual) of LinearAttention (denoise_net.py:216-235 with :93-102; biased variance, eps from the
 * struct, gain only).  Same argument struct as dsc_gemm_f32 (gamma = the LayerNorm gain, beta unused); one K row stride. */
int dsc_gemm_layernorm_f32(const dsc_gemm_args* a, dsc_stream_t stream);

/* Small-K linear for un-aligned inputs (first layer of _encoder_mlp on slices of the (B,N,C)
 * tensor, denoise_net.py:487,513-524; init_conv of the 5-channel re-arrangement model, :397):
 *   y[m][n] = act( sum_k x[m*ldx + k] * w[n*ldw + k] + bias[n] ),  k_in <= 64. */
int dsc_linear_smallk_f32(const float* x, int64_t ldx, int32_t k_in, const float* w, int64_t ldw,
                          const float* bias, float* y, int64_t ldy, int32_t m, int32_t n,
                          int32_t act_out, dsc_stream_t stream);
/* The same for up to DSC_SMALLK_MAX heads in ONE launch (the first layers of the per-attribute encoders, denoise_net.py:513-524:
 * every head reads its own column slice of the scene tensor and writes its own [m][n] block); items: HOST array.  Bit-identical to
 * `count` single launches. */
#define DSC_SMALLK_MAX 4
typedef struct dsc_smallk_item { const float* x; int64_t ldx; int32_t k_in; const float* w; int64_t ldw; const float* bias;
                                 float* y; int64_t ldy; } dsc_smallk_item;
int dsc_linear_smallk_grouped_f32(const dsc_smallk_item* items, int32_t count, int32_t m, int32_t n, int32_t act_out,
                                  dsc_stream_t stream);
/* dst[r][dst_col + c] = src[r][src_col + c] for c < width, over up to DSC_SMALLK_MAX column spans (HOST array): the padded outputs of
 * the stacked decoder output heads -> their columns of the (M, C) scene tensor. */
typedef struct dsc_col_span { int32_t src_col, dst_col, width; } dsc_col_span;
int dsc_gather_columns_f32(float* dst, int64_t ldd, const float* src, int64_t lds, int32_t rows, const dsc_col_span* spans,
                           int32_t count, dsc_stream_t stream);

/* WeightStandardizedConv2d.forward weight path (denoise_net.py:84-89):
 *   out[o][:] = (w[o][:] - mean_o) * rsqrt(var_o + eps), biased variance over the row.
 * Batched: up to DSC_WS_MAX matrices per launch. */
#define DSC_WS_MAX 64
typedef struct dsc_ws_item { const float* w; float* out; int32_t rows; int32_t cols; } dsc_ws_item;
int dsc_weight_standardize_f32(const dsc_ws_item* items, int32_t count, float eps, dsc_stream_t stream);

/* LayerNorm over channels with gain (denoise_net.py:98-102), optionally + residual (Residual, :39-45):
 *   y[r][:] = (x[r][:] - mean_r) * rsqrt(var_r + eps) * g[:] (+ residual[r][:]);  d must be 512. */
int dsc_layernorm_f32(const float* x, int64_t ldx, const float* g, const float* residual, int64_t ldr,
                      float* y, int64_t ldy, int32_t m, int32_t d, float eps, dsc_stream_t stream);

/* LinearAttention / LinearAttentionCross core (denoise_net.py:226-234, :288-296), 4 heads x 32:
 *   q <- softmax over the 32 head channels, * scale; k <- softmax over the nk tokens of the scene;
 *   ctx[d][e] = sum_j k[j][d] v[j][e];  out[i][e] = sum_d ctx[d][e] q[i][d].
 * q rows b*nq+i (ldq), k/v rows b*nk+j (ldk/ldv); head h uses columns [32h, 32h+32). nq, nk <= 160. */
int dsc_linear_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                             const float* v, int64_t ldv, float* out, int64_t ldo,
                             int32_t scenes, int32_t nq, int32_t nk, float scale, dsc_stream_t stream);

/* Attention core (denoise_net.py:252-258): softmax_j( scale * q_i . k_j ) v_j per scene and head; n <= 160. */
int dsc_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                      const float* v, int64_t ldv, float* out, int64_t ldo,
                      int32_t scenes, int32_t n, float scale, dsc_stream_t stream);

/* SinusoidalPosEmb (denoise_net.py:132-139): out[b] = table[t[b]] when 0 <= t[b] < table_rows (the
 * table is computed by the host with the reference's own fp32 expression), else computed in place
 * from freq[dim/2] as [sin(t f) | cos(t f)]. */
int dsc_time_embedding_f32(const int64_t* t, int32_t b, int32_t dim, const float* table, int32_t table_rows,
                           const float* freq, float* out, dsc_stream_t stream);

/* y = act(x) elementwise (SiLU on the conditioning before ResnetBlock.mlp's Linear, :181-184). */
int dsc_activation_f32(const float* x, float* y, int64_t count, int32_t act, dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Diffusion process (diffusion_ddpm.py).  Coefficient tables live on the device (the reference
 * re-uploads them on every call, :220,:232,:284); t is int64 on the device; `inner` = N*C.
 * These kernels are compiled with -ffp-contract=off and reproduce the reference's fp32
 * expression order bit for bit.
 * num_timesteps = rows of the coefficient tables: every kernel clamps the DEVICE value t[b] into [0, num_timesteps) before it
 * indexes a table (reference: the tables are indexed by torch.gather, which raises on such a t; here the launch is asynchronous,
 * so the access is made safe and the event is counted -- dsc_device_error_count).
 * ------------------------------------------------------------------------------------------- */

/* Out-of-range device timesteps the kernels below (and dsc_ddpm_loss_f32) had to clamp since the last reset; 0 in a correct run.
 * Synchronises the device (a test / debugging facility); -1 on a HIP error.  reset != 0 clears the counters. */
int64_t dsc_device_error_count(int32_t reset);

/* q_sample (:276-286) and, if v_out != NULL, _predict_v (:230-234) in one pass:
 *   x_t = sqrt_ac[t] * x0 + sqrt_1mac[t] * noise ;  v = sqrt_ac[t] * noise - sqrt_1mac[t] * x0 */
int dsc_q_sample_f32(const float* x0, const float* noise, const int64_t* t,
                     const float* sqrt_ac, const float* sqrt_1mac,
                     float* x_t, float* v_out, int32_t b, int64_t inner, int32_t num_timesteps, dsc_stream_t stream);

/* p_mean_variance + p_sample for model_var_type 'fixedsmall' (:242-264, :305-352):
 *   x0 = (mean_type v)   ca[t]*x_t - cb[t]*model_out      ca=sqrt_ac,        cb=sqrt_1mac
 *        (mean_type eps) ca[t]*x_t - cb[t]*model_out      ca=sqrt_recip_ac,  cb=sqrt_recipm1_ac
 *        (mean_type x0)  model_out
 *   clamp to [-1,1] if clip; mean = coef1[t]*x0 + coef2[t]*x_t; out = mean + (t != 0) * sigma[t] * noise
 * sigma[t] = exp(0.5 * posterior_log_variance_clipped[t]) is tabulated by the host.  b > 65535: DSC_ERANGE, as for every step. */
#define DSC_MEAN_EPS 0
#define DSC_MEAN_X0  1
#define DSC_MEAN_V   2
int dsc_p_sample_f32(const float* x_t, const float* model_out, const float* noise, const int64_t* t,
                     const float* ca, const float* cb, const float* coef1, const float* coef2,
                     const float* sigma, float* out, float* x0_out /* may be NULL */,
                     int32_t mean_type, int32_t clip, int32_t b, int64_t inner, int32_t num_timesteps,
                     dsc_stream_t stream);

/* In-graph timestep bookkeeping for the captured reverse loop (:365-366): t[i] += delta. */
int dsc_add_scalar_i64(int64_t* t, int32_t count, int64_t delta, dsc_stream_t stream);

/* One step of ddim_sample_loop (:402-444) for all b scenes, with x_start / pred_noise of model_predictions(clip_x_start=True,
 * rederive_pred_noise=False) (:242-264).  k = *step (device counter, clamped to [0, num_steps)); t = times[k], t_next = times_next[k]:
 *   x0 = clamp(ca[t]*x_t - cb[t]*model_out, -1, 1)   (ca, cb as dsc_p_sample_f32; mean_type x0: clamp(model_out))
 *   pred_noise = model_out (eps)  |  (sqrt_recip_ac[t]*x_t - x0) / sqrt_recipm1_ac[t] (x0, v)
 *   t_next <  0: out = x0 (noise is not read)
 *   t_next >= 0: out = ((x0 * sqrt_alpha_next[k]) + (c_noise[k] * pred_noise)) + (sigma[k] * noise)
 * Every product and sum is rounded separately and the division is IEEE: bit-identical to the fp32 CPU expressions.  The three
 * per-step tables (num_steps rows) are tabulated by the host with the reference's expressions.  out may alias x_t; x0_out may be NULL. */
int dsc_ddim_step_f32(const float* x_t, const float* model_out, const float* noise, const int64_t* step,
                      const int64_t* times, const int64_t* times_next, const float* sqrt_alpha_next,
                      const float* c_noise, const float* sigma, const float* ca, const float* cb,
                      const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, float* out, float* x0_out,
                      int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps,
                      dsc_stream_t stream);

/* Step bookkeeping of the captured DDIM loop (:424-425): *step += 1, then t[i] = times[*step] for i < count (the timestep of the
 * next model call).  One launch, no host work between replays. */
int dsc_ddim_advance_i64(int64_t* step, const int64_t* times, int64_t* t, int32_t count, int32_t num_steps,
                         dsc_stream_t stream);

/* Post-filter of generated scenes (delete_empty_from_network_samples, diffusion_scene_layout_ddpm.py:351-406): slot i is
 * dropped when samples[.., i, empty_col] >= 0 (and keep_empty == 0).  mode 0: the decision of batch row 0 is applied to every
 * scene (the reference's loop, :379); mode 1: per scene.  packed (b, n, c): kept rows first, original order, zero tail;
 * counts[b] = rows kept.  n <= 192; samples and packed must not alias. */
int dsc_postfilter_compact_f32(const float* samples, int32_t b, int32_t n, int32_t c, int32_t empty_col, int32_t mode,
                               int32_t keep_empty, float* packed, int32_t* counts, dsc_stream_t stream);

/* Inpainting overwrite of p_sample_loop_complete (:462-466): rows [0,p) of every scene of x
 * (b, n, c) are replaced by q_sample(partial, t, noise) (partial/noise are (b, p, c)).  b > 65535: DSC_ERANGE, as for the ragged form. */
int dsc_complete_overwrite_f32(float* x, const float* partial, const float* noise, const int64_t* t,
                               const float* sqrt_ac, const float* sqrt_1mac,
                               int32_t b, int32_t n, int32_t p, int32_t c, int32_t num_timesteps, dsc_stream_t stream);

/* dsc_complete_overwrite_f32 with a device vector of per-scene row counts (batched completion of scenes that are given
 * different numbers of objects): scene i writes rows [0, counts[i]) of x (b, n, c) from rows of partial / noise (b, pmax, c);
 * rows >= counts[i] of partial / noise are padding and never read, a count of 0 writes nothing.  counts (b,) int64, each in
 * [0, pmax], pmax <= n; an out-of-range count is clamped into that range and counted by dsc_device_error_count. */
int dsc_complete_overwrite_ragged_f32(float* x, const float* partial, const float* noise, const int64_t* counts,
                                      const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac,
                                      int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_timesteps, dsc_stream_t stream);

/* Fused step of the ragged completion loop, one launch after the model call.  Rows >= counts[i] of scene i: dsc_p_sample_f32.
 * Rows < counts[i] (the given objects):
 *   t[i] >  0: out = sqrt_ac[t-1] * partial + sqrt_1mac[t-1] * noise_p   (the overwrite that precedes the next model call)
 *   t[i] == 0: out = partial                                              (the final restore; noise_p is not read)
 * partial / noise_p are (b, pmax, c), x_t / model_out / noise / out (b, n, c); counts as dsc_complete_overwrite_ragged_f32.
 * Bit-identical to dsc_p_sample_f32 followed by dsc_complete_overwrite_ragged_f32 at t - 1 (or by the restore).  out may alias x_t. */
int dsc_p_sample_inpaint_f32(const float* x_t, const float* model_out, const float* noise, const float* partial,
                             const float* noise_p, const int64_t* counts, const int64_t* t, const float* ca, const float* cb,
                             const float* coef1, const float* coef2, const float* sigma, const float* sqrt_ac,
                             const float* sqrt_1mac, float* out, int32_t mean_type, int32_t clip,
                             int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_timesteps, dsc_stream_t stream);

/* Fused step of the strided (DDIM) ragged completion loop, one launch after the model call.  k, t = times[k], t_next = times_next[k]
 * as dsc_ddim_step_f32.  Rows >= counts[i] of scene i: dsc_ddim_step_f32.  Rows < counts[i] (the given objects):
 *   t_next >= 0: out = sqrt_ac[t_next] * partial + sqrt_1mac[t_next] * noise_p   (the overwrite that precedes the next model call)
 *   t_next <  0: out = partial                                                    (the final restore; noise and noise_p are not read)
 * partial / noise_p are (b, pmax, c), x_t / model_out / noise / out (b, n, c); counts as dsc_complete_overwrite_ragged_f32.  The step
 * index, times[k], times_next[k] (where non-negative) and counts[i] are clamped into range and counted by dsc_device_error_count.
 * Bit-identical to dsc_ddim_step_f32 followed by dsc_complete_overwrite_ragged_f32 at t_next (or by the restore).  out may alias x_t. */
int dsc_ddim_inpaint_step_f32(const float* x_t, const float* model_out, const float* noise, const float* partial,
                              const float* noise_p, const int64_t* counts, const int64_t* step, const int64_t* times,
                              const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise, const float* sigma,
                              const float* ca, const float* cb, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                              const float* sqrt_ac, const float* sqrt_1mac, float* out, int32_t mean_type,
                              int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_steps, int32_t num_timesteps,
                              dsc_stream_t stream);

/* Element-wise in-painting: the given elements of a scene are marked by a byte mask (b, n, c) -- any non-zero byte = given -- instead
 * of a row prefix.  known / noise / mask have the shape of x (b scenes of `inner` elements).  Where mask[i] != 0:
 *   x[i] = sqrt_ac[t] * known[i] + sqrt_1mac[t] * noise[i]      (t per scene, clamped and counted as everywhere)
 * the other elements of x are neither read nor written, and known / noise are not read there. */
int dsc_masked_overwrite_f32(float* x, const float* known, const float* noise, const uint8_t* mask, const int64_t* t,
                             const float* sqrt_ac, const float* sqrt_1mac, int32_t b, int64_t inner, int32_t num_timesteps,
                             dsc_stream_t stream);

/* Fused step of the masked T-step loop, one launch after the model call.  Free elements (mask[i] == 0): dsc_p_sample_f32.  Given ones:
 *   t >  0: out = sqrt_ac[t-1] * known + sqrt_1mac[t-1] * noise_k   (the overwrite that precedes the next model call)
 *   t == 0: out = known                                             (the final select; noise_k is not read)
 * A given element reads mask, known and noise_k only; a free one mask, x_t, model_out and noise only.  All operands (b, inner).
 * Bit-identical to dsc_p_sample_f32 followed by dsc_masked_overwrite_f32 at t - 1 (or by the select).  out may alias x_t. */
int dsc_p_sample_masked_f32(const float* x_t, const float* model_out, const float* noise, const float* known,
                            const float* noise_k, const uint8_t* mask, const int64_t* t, const float* ca, const float* cb,
                            const float* coef1, const float* coef2, const float* sigma, const float* sqrt_ac,
                            const float* sqrt_1mac, float* out, int32_t mean_type, int32_t clip, int32_t b, int64_t inner,
                            int32_t num_timesteps, dsc_stream_t stream);

/* Fused step of the strided (DDIM) masked loop.  k, t = times[k], t_next = times_next[k] as dsc_ddim_step_f32.  Free elements:
 * dsc_ddim_step_f32.  Given ones:
 *   t_next >= 0: out = sqrt_ac[t_next] * known + sqrt_1mac[t_next] * noise_k
 *   t_next <  0: out = known                                        (the final select; noise and noise_k are not read)
 * Reads per element as dsc_p_sample_masked_f32; the step index, times[k] and times_next[k] (where non-negative) are clamped into
 * range and counted by dsc_device_error_count, as in dsc_ddim_inpaint_step_f32.  Bit-identical to dsc_ddim_step_f32 followed by
 * dsc_masked_overwrite_f32 at t_next (or by the select).  out may alias x_t. */
int dsc_ddim_masked_step_f32(const float* x_t, const float* model_out, const float* noise, const float* known,
                             const float* noise_k, const uint8_t* mask, const int64_t* step, const int64_t* times,
                             const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise, const float* sigma,
                             const float* ca, const float* cb, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                             const float* sqrt_ac, const float* sqrt_1mac, float* out, int32_t mean_type,
                             int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps, dsc_stream_t stream);

/* Classifier-free guidance on the text path.  model_out is (2 b, inner): scenes [0, b) are the denoiser on the text features (c),
 * scenes [b, 2 b) the denoiser on the null condition (condition_cross == 0) (u), both on the same x_t.  scale is a (b,) f32 DEVICE
 * vector, read through the pointer by every launch (one captured graph serves every per-scene mix of scales):
 *   m = u + scale[i] * (c - u)        difference, product and sum each rounded on its own
 * eps, x0 and v are linear in each other given x_t, so guiding the raw model output is the same guidance under all three mean types.
 * dsc_cfg_combine_f32 writes m to out (b, inner): the unfused form. */
int dsc_cfg_combine_f32(const float* model_out, const float* scale, float* out, int32_t b, int64_t inner, dsc_stream_t stream);

/* dsc_p_sample_f32 with m computed in registers from the two halves of model_out (2 b, inner); x_t / noise / out / x0_out are
 * (b, inner).  x_dup (may be NULL): the new x is written there too, so a captured loop keeps x as one (2 b, inner) buffer with both
 * halves current.  At t == 0 the noise is not read.  Equal to dsc_cfg_combine_f32 followed by dsc_p_sample_f32 on finite noise (same
 * expressions, same rounding; at t == 0 that kernel adds 0 * noise, which can only change the sign of a zero).  out may alias x_t;
 * x_dup must not. */
int dsc_p_sample_cfg_f32(const float* x_t, const float* model_out, const float* scale, const float* noise, const int64_t* t,
                         const float* ca, const float* cb, const float* coef1, const float* coef2, const float* sigma,
                         float* out, float* x_dup /* may be NULL */, float* x0_out /* may be NULL */, int32_t mean_type,
                         int32_t clip, int32_t b, int64_t inner, int32_t num_timesteps, dsc_stream_t stream);

/* dsc_ddim_step_f32 with the same change (tables, step counter and clamping as there; noise is not read on the last pair).
 * Bit-identical to dsc_cfg_combine_f32 followed by dsc_ddim_step_f32.  out may alias x_t; x_dup must not. */
int dsc_ddim_cfg_step_f32(const float* x_t, const float* model_out, const float* scale, const float* noise, const int64_t* step,
                          const int64_t* times, const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise,
                          const float* sigma, const float* ca, const float* cb, const float* sqrt_recip_ac,
                          const float* sqrt_recipm1_ac, float* out, float* x_dup /* may be NULL */, float* x0_out /* may be NULL */,
                          int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps,
                          dsc_stream_t stream);

/* Guided in-painting: dsc_p_sample_masked_f32 with m = u + scale[i] * (c - u) computed in registers from the two halves of model_out
 * (2 b, inner); x_t / noise / known / noise_k / mask / out are (b, inner), scale is (b,).  x_dup (may be NULL): every written element,
 * given or free, is written there too (the null half of a captured loop's (2 b, inner) state).  A given element reads mask, known and
 * noise_k only (no noise_k at t == 0); a free one mask, x_t, both halves of model_out and noise only.  Bit-identical to
 * dsc_cfg_combine_f32 followed by dsc_p_sample_masked_f32.  out may alias x_t; x_dup must not. */
int dsc_p_sample_masked_cfg_f32(const float* x_t, const float* model_out, const float* scale, const float* noise, const float* known,
                                const float* noise_k, const uint8_t* mask, const int64_t* t, const float* ca, const float* cb,
                                const float* coef1, const float* coef2, const float* sigma, const float* sqrt_ac,
                                const float* sqrt_1mac, float* out, float* x_dup /* may be NULL */, int32_t mean_type, int32_t clip,
                                int32_t b, int64_t inner, int32_t num_timesteps, dsc_stream_t stream);

/* dsc_ddim_masked_step_f32 with the same change and the same x_dup (tables, step counter and clamping as there; on the last pair
 * neither noise nor noise_k is read).  Bit-identical to dsc_cfg_combine_f32 followed by dsc_ddim_masked_step_f32.  out may alias x_t;
 * x_dup must not. */
int dsc_ddim_masked_cfg_step_f32(const float* x_t, const float* model_out, const float* scale, const float* noise, const float* known,
                                 const float* noise_k, const uint8_t* mask, const int64_t* step, const int64_t* times,
                                 const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise, const float* sigma,
                                 const float* ca, const float* cb, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                                 const float* sqrt_ac, const float* sqrt_1mac, float* out, float* x_dup /* may be NULL */,
                                 int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps,
                                 dsc_stream_t stream);

/* Collision steering: one launch between the model call and the unchanged step kernel, correcting model_out IN PLACE so that the step's
 * x0 estimate moves down the gradient of the pairwise box-overlap energy (INTEGRATION.md 9 states the definition).  Scene i of b:
 *   x0     = clamp(predict_x0(x_t, m), -1, 1) per element (always clamped); a given element takes its given value.  m = model_out, or
 *            u + cfg_scale[i] * (c - u) from the two halves of a (2 b, n, c) model_out when cfg_scale is set.
 *   boxes  : centre = descale(x0[0:3]), half sizes = descale(x0[3:6]) with bounds[12] = c_lo[3] c_hi[3] s_lo[3] s_hi[3] (HOST, as in
 *            dsc_ddpm_loss_f32), rotated about y by the (cos, sin) channels 6, 7 over their hypot (both zero: angle 0) and bounded
 *            axis-aligned: hx = |c| sx + |s| sz, hy = sy, hz = |s| sx + |c| sz.  Box j is valid iff x0[j, bbox_dim + class_dim - 1] < 0.
 *   energy : E = sum over valid pairs j < k of the axis-aligned 3-D IoU with union floor 1e-6; boxes that only touch do not interact.
 *   g      = dE / d x0[:, 0:3] (through the centres only; it includes span / 2).
 *   store  : only when t < t_below[0] and weight[i] != 0, and only to free translation elements of valid boxes with weight * g != 0:
 *            d = weight[i] * g + (raw - clamp(raw));  mean type x0: m -= d;  eps / v: m += d / cb[t] (cb[t] == 0: no store), so the step
 *            sees x0 = clamp(x0) - weight[i] * g.  With cfg_scale the same delta is added to both halves.
 * Operand groups that may be NULL: the time source is t (b,) or step (1,) / times (num_steps,) (exactly one); ca / cb / x_t for mean
 * type x0; the given part is none, (partial (b, pmax, c), counts (b,)) -- rows [0, counts[i]) -- or (known, mask) of x_t's shape;
 * cfg_scale; energy_out (b,) and grad_out (b, n, 3), written whether or not the step is active.  weight (b,) f32 and t_below (1,) int64
 * are DEVICE buffers read through their pointers: one captured graph serves every weight and every number of steered steps.
 * One 256-thread block per scene, n <= 160 (else DSC_ERANGE); x0 is the float32 value the step forms, the geometry after it is
 * float64 (energy_out / grad_out are the float32 numbers nearest to it); the energy is summed in a fixed order, no atomics, and scene
 * i's result does not depend on b.  bbox_dim != 8: DSC_ERANGE; bbox_dim + class_dim > c, class_dim < 1, two time sources or two given parts:
 * DSC_EINVAL.  t[i], counts[i], step[0] and times[k] are clamped and counted (dsc_device_error_count). */
int dsc_steer_boxes_f32(const float* x_t, float* model_out, const int64_t* t, const int64_t* step, const int64_t* times,
                        const float* ca, const float* cb, const float* partial, const int64_t* counts, const float* known,
                        const uint8_t* mask, const float* cfg_scale, const float* weight, const int64_t* t_below,
                        const float* bounds, float* energy_out, float* grad_out, int32_t mean_type, int32_t b, int32_t n,
                        int32_t pmax, int32_t c, int32_t bbox_dim, int32_t class_dim, int32_t num_steps, int32_t num_timesteps,
                        dsc_stream_t stream);

/* Multistep DPM-Solver++(2M): one launch between the model call (after dsc_steer_boxes_f32, if any) and the unchanged strided step,
 * correcting model_out IN PLACE so that the step's x0 estimate becomes the extrapolated one (INTEGRATION.md 9 states the definition).
 * At pair k = step[0] of num_steps, with e = weights[k] (the (num_steps,) float32 history weights, e_0 = e_{S-1} = 0, computed on the
 * host in float64), for every free element of scene i:
 *   m     = model_out, or u + cfg_scale[i] * (c - u) from the two halves of a (2 b, inner) model_out when cfg_scale is set (float32);
 *   x0raw = predict_x0(x_t, m) in float32 as the step forms it; x0c = clamp(x0raw, -1, 1);
 *   float64 from here, one final rounding: D = x0c + e (x0c - hist); d = x0raw - D; mean type x0: m -= d; eps / v: m += d / cb[t]
 *   (cb[t] == 0: no store); with cfg_scale the same delta is added to both halves;
 *   hist  = x0c.
 * e == 0: hist is not read, model_out is not written.  hist is written on every pair but the last (k == num_steps - 1), where nothing
 * is read or stored.  A given element -- rows [0, counts[i]) of pmax <= inner / c rows of c channels, or mask != 0 (x_t's shape), at most
 * one of the two, both may be NULL -- is neither read nor written in x_t, model_out and hist.  ca / cb / x_t may be NULL for mean type
 * x0; cfg_scale may be NULL.  step[0] and times[k] are clamped and counted once per launch, counts[i] once per scene
 * (dsc_device_error_count).  b <= 65535 (else DSC_ERANGE); two given parts: DSC_EINVAL. */
int dsc_multistep_x0_f32(const float* x_t, float* model_out, float* hist, const float* weights, const int64_t* step,
                         const int64_t* times, const float* ca, const float* cb, const float* cfg_scale, const int64_t* counts,
                         const uint8_t* mask, int32_t mean_type, int32_t b, int64_t inner, int32_t pmax, int32_t c, int32_t num_steps,
                         int32_t num_timesteps, dsc_stream_t stream);

/* The resampling jump of the completion and in-painting loops (RePaint; INTEGRATION.md 9 states the schedule): one forward diffusion of
 * the whole state x (b, inner), IN PLACE, from remaining index s to s + jump:
 *   free element:   x = (ja[pos] * x) + (jb[pos] * noise)
 *   given element:  x = (sqrt_ac[tt] * given) + (sqrt_1mac[tt] * noise_g)   -- what the overwrite in front of the next model call writes
 * the two products and the sum rounded one by one.  One time source: t (b,) -- pos = t[i], tt = t[i] + jump, ja / jb of num_timesteps
 * rows -- or step (1,) and times (num_steps,) -- pos = k = *step, tt = times[k - jump], ja / jb of num_steps rows.  ja[pos] =
 * sqrt(abar[time(s + jump)] / abar[time(s)]) and jb[pos] = sqrt(1 - that ratio) are tabulated by the host in float64 and rounded once.
 * The given part: rows [0, counts[i]) of pmax <= inner / c rows of c channels (given / noise_g are (b, pmax, c)), or mask != 0 (given /
 * noise_g / mask have x's shape), at most one of the two; given == NULL (then noise_g, counts and mask must be NULL too) is the plain jump
 * of every element, dsc_q_sample_f32 on the tables (ja, jb).  A given element reads mask, given and noise_g only, a free one mask, x and
 * noise only.  x_dup (may be NULL) receives a second copy of every element written.  The result is bit-identical to dsc_q_sample_f32
 * with (ja, jb) at t = s followed by the matching dsc_*_overwrite*_f32 at tt.  Indices are clamped and counted (dsc_device_error_count):
 * t[i], t[i] + jump and counts[i] once per scene; *step, k - jump and times[.] once per launch; tt only with a given part.
 * b <= 65535 (else DSC_ERANGE); jump < 1, two time sources or two given parts: DSC_EINVAL. */
int dsc_resample_jump_f32(float* x, const float* noise, const float* ja, const float* jb, const int64_t* t, const int64_t* step,
                          const int64_t* times, const float* given, const float* noise_g, const uint8_t* mask, const int64_t* counts,
                          const float* sqrt_ac, const float* sqrt_1mac, float* x_dup, int32_t jump, int32_t b, int64_t inner,
                          int32_t pmax, int32_t c, int32_t num_steps, int32_t num_timesteps, dsc_stream_t stream);

/* The move after a jump in a strided loop, the seek form of dsc_ddim_advance_i64: *step += delta (clamped to [0, num_steps) and
 * counted), then t[i] = times[*step] for i < count.  One launch of one block. */
int dsc_ddim_seek_i64(int64_t* step, const int64_t* times, int64_t* t, int32_t count, int32_t num_steps, int64_t delta,
                      dsc_stream_t stream);

/* Floor-plan steering, the field: once per call.  mask (b, h, w) f32, pixel (i, j) inside iff > 0.5; the image
 * covers x in [-room_side, room_side] along its columns and z likewise along its rows, dx = 2 room_side / w, dz = 2 room_side / h.
 *   field[i, j] = 1/2 min over inside pixels (i', j') of ((i - i') dz)^2 + ((j - j') dx)^2   (metres^2; 0 at inside pixels),
 * the float32 nearest to the float64 expression (an exact two-pass minimum); a mask without an inside pixel gives field == 0.
 * 2 <= h, w <= 256 and b <= 65535 (else DSC_ERANGE); room_side must be finite and > 0 (else DSC_EINVAL). */
int dsc_floor_field_f32(const float* mask, float* field, int32_t b, int32_t h, int32_t w, float room_side, dsc_stream_t stream);

/* Floor-plan steering, the launch inside the loop: after dsc_steer_boxes_f32 (if any), before dsc_multistep_x0_f32 and the guidance
 * mix, correcting model_out IN PLACE so that the step's x0 estimate moves its boxes into the room (INTEGRATION.md 9 states the
 * definition).  x0, validity, the operand groups (time source, given part, cfg_scale), bounds (HOST), weight / t_below (DEVICE) and the
 * store rule are those of dsc_steer_boxes_f32; the store goes to channels 0 and 2 only.  Scene i of b:
 *   points : the nine points centre_xz + R (a sx, b sz), a, b in {-1, 0, 1}, of every valid box: the oriented footprint, R the rotation
 *            about y by the (cos, sin) channels over their hypot (x' = c lx - s lz, z' = s lx + c lz; both zero: angle 0).
 *   e(p)   : u = (x + s) / dx - 1/2, v = (z + s) / dz - 1/2, s = room_side[0]; uc = clamp(u, 0, w - 1), j0 = min(floor(uc), w - 2),
 *            fu = uc - j0, likewise vc, i0, fv with h;  e = bilinear(field; i0, j0, fv, fu) + 1/2 ((u - uc) dx)^2 + 1/2 ((v - vc) dz)^2.
 *   energy : E = sum over valid boxes of (1/9) sum of e over the nine points;  g = dE / d x0[:, {0, 2}] (it includes span / 2).
 * field is (field_b, h, w) f32 from dsc_floor_field_f32 with field_b == b or 1 (shared by all scenes); room_side (1,) f32 is a DEVICE
 * buffer read through its pointer, like weight and t_below: one captured graph serves every mask and every room side.  Optional
 * outputs, written whether or not the step is active: energy_out (b,), grad_out (b, n, 3) (the y column is 0), outside_out (b,) int32 =
 * the number of valid boxes with a point of e > 0.  An inactive launch without optional outputs reads no scene.  One 256-thread block
 * per scene, n <= 160; float64 after the float32 x0 and field, fixed summation order, scene i's result does not depend on b.  n > 160,
 * bbox_dim != 8, h or w outside [2, 256]: DSC_ERANGE; the DSC_EINVAL cases of dsc_steer_boxes_f32, and field_b not in {1, b}. */
int dsc_steer_walls_f32(const float* x_t, float* model_out, const int64_t* t, const int64_t* step, const int64_t* times,
                        const float* ca, const float* cb, const float* partial, const int64_t* counts, const float* known,
                        const uint8_t* mask, const float* cfg_scale, const float* weight, const int64_t* t_below,
                        const float* bounds, const float* field, const float* room_side, float* energy_out, float* grad_out,
                        int32_t* outside_out, int32_t mean_type, int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t bbox_dim,
                        int32_t class_dim, int32_t num_steps, int32_t num_timesteps, int32_t field_b, int32_t h, int32_t w,
                        dsc_stream_t stream);

/* Per-scene gate of the text-condition dropout (text_drop_prob): y[i, :] = keep[i] ? x[i, :] : 0 for b scenes of `inner` elements;
 * keep holds one byte per scene.  A select: the elements of a dropped scene are not read (NaN there does not propagate).  Used forward
 * on the text features and backward on their incoming gradient.  y may alias x. */
int dsc_scene_gate_f32(const float* x, const uint8_t* keep, float* y, int32_t b, int64_t inner, dsc_stream_t stream);

/* Per-scene noise: out (b, per_scene) contiguous, out[i, e] = scene_normal(seeds[i], stream, *draw, e), a pure function of its four
 * arguments (diffuscene_amd/scene_noise.py evaluates the same definition on the host) -- nothing of b, of the scene's position or of
 * earlier launches enters:
 *   (r0, r1, r2, r3) = Philox4x32-10 on the counter (e >> 2, stream, draw & 0xffffffff, draw >> 32) under the key
 *                      (seed & 0xffffffff, seed >> 32), the seed read as 64 bits; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
 *                      0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped after every round;
 *   u_i = (float)(r_i >> 8) * 2^-24 + 2^-25   in float32 (rounded to nearest even above 1/2: u in (0, 1], and u == 1 gives rho == 0);
 *   lanes e & 3 == 0, 1: rho = sqrtf(-2 * logf(u0)), theta = (float)(2 pi) * u1, z0 = rho * cosf(theta), z1 = rho * sinf(theta);
 *   lanes 2, 3 the same on (u2, u3).  Full-precision logf / sinf / cosf, no fast-math.
 * seeds: (b,) int64 on the device.  draw: ONE int64 on the device, read by the launch and never written, so a captured launch draws
 * what the counter holds at replay time (dsc_add_scalar_i64 advances it inside the graph).  stream: a 32-bit id (0 the main draws of a
 * loop, 1 the draws for the given part of a scene).  per_scene <= 2^32.  Null pointers, a negative count or a stream outside 32 bits:
 * DSC_EINVAL; b == 0 or per_scene == 0: nothing is launched, 0; b * ceil(per_scene / 4) beyond 2^31 - 1 blocks of 256: DSC_ERANGE.
 * One thread per Philox block; the last quad of a scene stores only its per_scene & 3 live lanes; dwordx4 stores when
 * per_scene % 4 == 0 and out is 16-byte aligned, dword stores otherwise (no alignment is required of out). */
int dsc_scene_randn_f32(float* out, const int64_t* seeds, const int64_t* draw, int64_t stream, int64_t b, int64_t per_scene,
                        dsc_stream_t hip_stream);
/* The raw word r_(e & 3) of every element instead of the normal: a probe for tests, so that the integer stream is pinned exactly. */
int dsc_scene_philox_u32(uint32_t* out, const int64_t* seeds, const int64_t* draw, int64_t stream, int64_t b, int64_t per_scene,
                         dsc_stream_t hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Training: hand-written backward of the denoiser (the reference relies on torch autograd through
 * denoise_net.py; train_on_batch, diffusion_scene_layout_ddpm.py:456-473).  Input gradients
 * dA = dY . W reuse dsc_gemm_f32 on transposed weights (dsc_transpose_f32).
 * ------------------------------------------------------------------------------------------- */

/* Weight gradient  out[n][k] = sum_m dy[m][n] * [a1|a2][m][k]  (fp32 MFMA, split over tokens, deterministic
 * two-stage reduction through `workspace`, sized by dsc_gemm_tn_workspace_floats).  Columns >= kvalid of a
 * zero-padded small-K input are not stored; out is dense [n][kvalid] (ldo == kvalid) when split. */
int dsc_gemm_tn_f32(const float* a1, int64_t lda1, int32_t k1, const float* a2, int64_t lda2, int32_t k2,
                    const float* dy, int64_t ldd, float* out, int64_t ldo, float* dbias /* [n] column sums of dy, or NULL */,
                    int32_t m, int32_t n, int32_t kvalid, float* workspace, int64_t workspace_floats, dsc_stream_t stream);
int64_t dsc_gemm_tn_workspace_floats(int32_t m, int32_t n, int32_t k);

/* The same for MANY layers in one launch (static training plan: weight gradients are leaves of the backward pass and every
 * activation stays alive, so they are deferred and computed together -- enough output tiles to fill the chip without cutting
 * the token dimension into 32 slabs per layer).  `groups_dev` is a DEVICE array of `count` descriptors (pointers are device
 * pointers; the constraints of dsc_gemm_tn_f32 apply to each and are validated by the caller that builds the table);
 * tile0 = number of 128 x 128 output tiles of all earlier groups (ceil(n/128) * ceil((k1+k2)/128) each), total_tiles their
 * sum.  splits == 1 writes `out` / `dbias` directly; splits > 1 cuts every group's tokens into `splits` ranges whose partial
 * results go to workspace + ws_offset ([splits][n*kvalid] then [splits][n], per group) and are summed in a fixed order by
 * a second launch.  workspace_needed = end of the last group's area. */
typedef struct dsc_tn_group {
    const float* a1; int64_t lda1; int32_t k1;
    const float* a2; int64_t lda2; int32_t k2;
    const float* dy; int64_t ldd;
    float* out; int64_t ldo;
    float* dbias;
    int32_t m, n, kvalid;
    int32_t tile0;
    int64_t ws_offset;
    int32_t tile0s;   /* reserved (round 3: first tile in the 256 x 128 numbering; the split launch now takes a block map) */
} dsc_tn_group;
int dsc_gemm_tn_grouped_f32(const dsc_tn_group* groups_dev, int32_t count, int32_t total_tiles, int32_t splits,
                            float* workspace, int64_t workspace_floats, int64_t workspace_needed, dsc_stream_t stream);
/* The same launch on the bf16 matrix cores with f32 accuracy (both operands split exactly into three bf16 pieces, six products, f32
 * accumulation; csrc/gemm_tn_split.h).  Output tiles are 256 (n) x 128 (k); the caller supplies the block placement:
 *   block_map_dev  DEVICE array of `blocks` int32 pairs (group index, tile of that group: k tile + ktiles * n tile), 8-byte aligned;
 *                  (-1, -1) = idle block.  Every tile of every group must appear exactly once.  Consecutive workgroup ids are dealt
 *                  round-robin over the 8 XCDs, so entries b, b + 8, b + 16 ... share one L2: put the tiles of one layer there.
 * total_tiles / tile0 stay the 128 x 128 numbering (used by the slab reduction when splits > 1; tile0s is unused).  Every operand must
 * satisfy m * ld * 4 < 2^31.
 * tile_k (round 6): the k width of the tiles the block map numbers -- 128 (256 x 128 tiles: the round-4 / round-5 bodies) or 256 (256 x 256
 * tiles, tile of a group = k tile + ceil(K / 256) * n tile: the round-6 body, which needs k1 % 256 == 0 wherever k2 > 0). */
int dsc_gemm_tn_grouped_split_f32(const dsc_tn_group* groups_dev, int32_t count, int32_t total_tiles, const int32_t* block_map_dev,
                                  int32_t blocks, int32_t splits, float* workspace, int64_t workspace_floats, int64_t workspace_needed,
                                  int32_t tile_k, dsc_stream_t stream);

/* The split-bf16 weight-gradient launch has three block bodies with IDENTICAL results: 2 = 256 x 256 tiles, four waves of 128 x 128 with
 * the 512-register budget (round 6, default: half the staged bytes per MFMA); 1 = 256 x 128 tiles, producer / consumer waves (round 5);
 * 0 = the round-4 body (every wave stages and multiplies).  set returns the previous form (process-wide; launches already captured in a
 * hipGraph keep theirs); DSC_TN_FORM in the environment gives the initial one.  The host asks get() when it builds a block map: form 2
 * -> tile_k 256.  For tests that hold the three to each other bit for bit. */
int dsc_set_tn_split_form(int32_t form);
int dsc_get_tn_split_form(void);

/* out[c] = sum_r x[r][c] (bias / affine gradients); workspace >= 64 * n floats. */
int dsc_colsum_f32(const float* x, int64_t ldx, int32_t m, int32_t n, float* out, float* workspace,
                   int64_t workspace_floats, dsc_stream_t stream);

/* Grouped column sums: out_i[c] = sum_r x_i[r][c] for `count` small matrices in ONE launch (items: a DEVICE array; every m
 * should be a few hundred rows -- the per-scene partials of bias / affine gradients).  Fixed summation order. */
typedef struct dsc_colsum_item { const float* x; int64_t ldx; int32_t m, n; float* out; } dsc_colsum_item;
int dsc_colsum_grouped_f32(const dsc_colsum_item* items_dev, int32_t count, int32_t max_n, dsc_stream_t stream);

/* Backward of the GroupNorm + (scale+1, shift) + SiLU epilogue of dsc_gemm_gn_silu_f32 (Block.forward,
 * denoise_net.py:167-176) from the saved pre-norm output z.  dz feeds the GEMM backward; dgamma_p / dbeta_p /
 * dbias_p are per-scene partials, row b at p + b*partial_stride (reduce with dsc_colsum_f32); dss is [scenes][1024] for
 * DSC_SS_PER_SCENE, [m][1024] for PER_TOKEN / PER_SLOT (caller reduces over the batch for PER_SLOT). */
int dsc_gn_silu_bwd_f32(const float* z, int64_t ldz, const float* dy, int64_t ldy, const float* gamma,
                        const float* beta, const float* scale_shift, int64_t ld_ss, int32_t ss_mode,
                        float* dz, int64_t lddz, float* dgamma_p, float* dbeta_p, float* dbias_p, int64_t partial_stride,
                        float* dss, int64_t ld_dss, int32_t scenes, int32_t tokens_per_scene, int32_t channels,
                        float eps, dsc_stream_t stream);

/* Backward of dsc_weight_standardize_f32: dw = rstd * (dw_std - mean(dw_std) - w_std * mean(dw_std * w_std)). */
typedef struct dsc_ws_bwd_item { const float* w; const float* dw_std; float* dw; int32_t rows; int32_t cols; } dsc_ws_bwd_item;
int dsc_weight_standardize_bwd_f32(const dsc_ws_bwd_item* items, int32_t count, float eps, dsc_stream_t stream);

/* Backward of dsc_layernorm_f32: dx (+ addend when not NULL: the gradient x already holds from another consumer -- dx may be a
 * different buffer than addend, so nothing is modified in place), and per-block partials of the gain gradient [partial_rows][512]. */
int dsc_layernorm_bwd_f32(const float* x, int64_t ldx, const float* g, const float* dy, int64_t ldy, float* dx,
                          int64_t lddx, const float* addend, int64_t ldadd, float* dg_partial, int32_t partial_rows, int32_t m,
                          int32_t d, float eps, dsc_stream_t stream);

int dsc_linear_attention_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk,
                                 float* dv, int64_t lddv, int32_t scenes, int32_t nq, int32_t nk, float scale,
                                 dsc_stream_t stream);

int dsc_attention_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                          const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk,
                          float* dv, int64_t lddv, int32_t scenes, int32_t n, float scale, dsc_stream_t stream);

/* Training loss of p_losses (diffusion_ddpm.py:556-652, loss_type 'mse', full attribute tensor) and its gradient in
 * one kernel, one block per scene: separated MSE terms x loss_weight[t] + the masked pairwise 3-D IoU regulariser
 * (loss.py:7-102) on the clamped, de-normalised x0 estimate  x0 = ca[t]*x_t - cb[t]*out  (mean_type v / eps; out itself
 * for x0).  losses[b] = losses_weight of scene b; parts[b][9] = {bbox, trans, size, angle, class, object, objfeat,
 * liou, bbox_iou}; dout[b] = grad_scale * d losses[b] / d out[b] (grad_scale = 1/B for loss = losses.mean()).  The
 * re-arrangement model (:558-571; size_dim = class_dim = objectness_dim = objfeat_dim = 0, c = bbox_dim = translation +
 * angle channels) uses losses = l_trans + l_angle, no IoU term.  bounds is a HOST array {centroid min[3], max[3], size min[3],
 * max[3]} (dataset_stats.txt, :137-151), required when loss_iou. */
int dsc_ddpm_loss_f32(const float* target, const float* out, const float* x_t, const int64_t* t,
                      const float* loss_weight, const float* ca, const float* cb, const float* alphas_cumprod,
                      const float* bounds, float* losses, float* parts, float* dout, int32_t b, int32_t n, int32_t c,
                      int32_t translation_dim, int32_t size_dim, int32_t bbox_dim, int32_t class_dim,
                      int32_t objectness_dim, int32_t objfeat_dim, int32_t loss_separate, int32_t loss_iou,
                      int32_t mean_type, float grad_scale, int32_t num_timesteps, dsc_stream_t stream);

/* Strided 2-D copy / accumulate (static training plan: staging of un-aligned column slices, gradient accumulation of
 * multi-consumer activations such as skip connections):  dst[r][c] = src[r][c]   /   dst[r][c] += src[r][c]. */
int dsc_copy2d_f32(float* dst, int64_t ldd, const float* src, int64_t lds, int32_t rows, int32_t cols, dsc_stream_t stream);
int dsc_add2d_f32(float* dst, int64_t ldd, const float* src, int64_t lds, int32_t rows, int32_t cols, dsc_stream_t stream);

/* dx = dy * act'(x) */
int dsc_activation_bwd_f32(const float* x, const float* dy, float* dx, int64_t count, int32_t act, dsc_stream_t stream);

/* out[c][r] = in[r][c] */
int dsc_transpose_f32(const float* in, int64_t ldi, float* out, int64_t ldo, int32_t rows, int32_t cols,
                      dsc_stream_t stream);
/* the same for up to DSC_WS_MAX contiguous matrices in one launch: items[i].out[c][r] = items[i].w[r][c] */
int dsc_transpose_batched_f32(const dsc_ws_item* items, int32_t count, dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Shape retrieval: nearest database object of the same class in the 32-d latent shape-code space,
 * ThreedFutureDataset.get_closest_furniture_to_objfeats (datasets/threed_future_dataset.py:49-59); with sizes
 * (float64, [n][3]) the lexicographic (size mse, feature mse) order of ..._and_size (:61-77, np.lexsort).
 * out_index[q] = database row, -1 when no object carries the label; ties -> lowest index.  Index-exact with the numpy
 * reference (same fp32 summation order).
 * ------------------------------------------------------------------------------------------- */
int dsc_retrieve_nearest_f32(const float* query_feats, const int32_t* query_labels, const double* query_sizes,
                             const float* db_feats, const int32_t* db_labels, const double* db_sizes,
                             int32_t n_query, int32_t n_db, int32_t feat_dim, int32_t* out_index, float* out_dist,
                             dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scene statistics after sampling: the box-level numbers of the reference's iou_states.txt (scripts/utils.py:559-747,
 * computer_intersection / computer_symmetry) for `batch` scenes in two launches.  counts[b] (int32) objects of scene b are
 * valid; rows at or beyond it are never read (they may hold NaN).  A count outside [0, nmax] is clamped into that range and
 * counted by dsc_device_error_count.
 * ------------------------------------------------------------------------------------------- */
#define DSC_STATS_MAX_OBJECTS 160
#define DSC_STATS_ONE_WAVE_MAX 32     /* nmax up to here: one-wave blocks; above: four waves */

/* bounds[b][k] = <x1, y1, z1, x2, y2, z2>: min / max over the eight corners (+-sizes).dot(R) + translations with R of
 * scene_synthesis/utils.py:48-53 (rotation about y by angles[b][k]); float64 arithmetic, rounded once to float32.
 * translations, sizes (half extents) [batch][nmax][3], angles [batch][nmax].  Rows at or beyond counts[b] are written as zeros. */
int dsc_box_bounds_f32(const float* translations, const float* sizes, const float* angles, const int32_t* counts,
                       int32_t batch, int32_t nmax, float* bounds, dsc_stream_t stream);

/* Per scene, over the pairs i < j < counts[b] of bounds [batch][nmax][6]: pairs with IoU > 0, pairs passing judge_if_symmetry
 * (float64 on the float32 bounds; equal class id = first arg-max of class_scores [batch][nmax][num_classes], and equal
 * model_ids [batch][nmax] unless NULL), float64 sums of the float32 per-pair IoU and overlap volume (fp32 arithmetic in the
 * order of axis_aligned_bbox_overlaps_3d, scripts/utils.py:607-647) and of the float32 box volumes; class_counts
 * [batch][num_classes]; pair_iou [batch][nmax][nmax] (strict upper triangle, the rest zero) or NULL.
 * nmax <= DSC_STATS_MAX_OBJECTS.  One workgroup per scene; block_threads 0 (one wave up to DSC_STATS_ONE_WAVE_MAX objects, four
 * above), 64 or 256.  The summation order depends on counts[b] alone: a scene's results are the same bits for every nmax and
 * block size, and from run to run. */
int dsc_scene_stats_f32(const float* bounds, const float* class_scores, const int32_t* model_ids, const int32_t* counts,
                        int32_t batch, int32_t nmax, int32_t num_classes, int32_t block_threads,
                        int32_t* num_intersecting, int32_t* num_symmetry, double* iou_sum, double* overlap_sum,
                        double* volume_sum, int32_t* class_counts, float* pair_iou, dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training input pipeline: one launch turns B scenes of the HBM-resident cached dataset into the padded
 * (B, N, C) training batch -- RotationAugmentation (threed_front_dataset.py:313-371), Jitter (:559-567),
 * Scale_CosinAngle_ObjfeatsNorm (:481-513), Permutation (:570-584) and the Diffusion padding wrapper (:888-925) fused.
 * The random draws (rotation angle, jitter offsets, object order) are made on the host in the reference's order and
 * passed in; the arithmetic follows numpy's mixed float32/float64 promotion (see oracle/dataset_ref.py).
 *
 * Store (device): offsets[S+1] first object row of each scene; class_labels[total][n_cls_in] one-hot incl. the start
 * and end columns; translations/sizes [total][3]; angles [total]; objfeats [total][feat_dim] or NULL.
 * Batch (device): scene[B]; order[B][N] (object j of the output comes from object order[b][j] of the scene; NULL =
 * stored order); rot[B] radians or NULL (no rotation wrapper); jitter[B][3] (translation, size, angle offsets) or NULL.
 * bounds (HOST, double): {t_lo[3], t_hi[3], s_lo[3], s_hi[3], angle_min, feat_lo, feat_hi}.
 * out[B*N][ld_out] channel order [translation 3 | size 3 | cos, sin | class n_cls_in-1 | objfeat feat_dim]
 * (diffusion_scene_layout_ddpm.py:148-154); rows >= length are the end symbol (class = [-1..-1,+1], rest 0).
 * length[B] = number of objects.  Scenes longer than N are an error (DSC_EINVAL) detected on the host by the caller.
 * ------------------------------------------------------------------------------------------- */
int dsc_encode_scene_batch_f32(const int64_t* offsets, const float* class_labels, const float* translations,
                               const float* sizes, const float* angles, const float* objfeats, int32_t n_cls_in,
                               int32_t feat_dim, const int64_t* scene, const int32_t* order, const double* rot,
                               const double* jitter, int32_t permute_objfeats, const double* bounds, float* out,
                               int64_t ld_out, int64_t* length, int32_t b, int32_t n, dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 3-D Chamfer distance -- the binding pair of ChamferDistancePytorch/chamfer3D/chamfer_cuda.cpp
 * (chamfer_cuda_forward / chamfer_cuda_backward, kernels chamfer3D.cu:12-171).  xyz1 [b][n][3], xyz2 [b][m][3]
 * contiguous fp32.  dist1[b][n] = squared distance from each point of cloud 1 to its nearest point of cloud 2,
 * idx1 = that point's index (ties -> lowest index); dist2 / idx2 the other way round.  backward writes (does not
 * accumulate into) gradxyz1 / gradxyz2 = d(sum graddist1*dist1 + sum graddist2*dist2)/d xyz; deterministic gather,
 * no atomics.
 * ------------------------------------------------------------------------------------------- */
int dsc_chamfer3d_forward_f32(const float* xyz1, const float* xyz2, float* dist1, float* dist2, int32_t* idx1,
                              int32_t* idx2, int32_t b, int32_t n, int32_t m, dsc_stream_t stream);
int dsc_chamfer3d_backward_f32(const float* xyz1, const float* xyz2, const float* graddist1, const float* graddist2,
                               const int32_t* idx1, const int32_t* idx2, float* gradxyz1, float* gradxyz2, int32_t b,
                               int32_t n, int32_t m, dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step of train_on_batch (diffusion_scene_layout_ddpm.py:456-473): torch.nn.utils.clip_grad_norm_ +
 * torch.optim.Adam (networks/__init__.py:29-30) as three launches over a DEVICE work list of chunks (each <= 32768
 * contiguous elements of one parameter; pointers are device pointers).  Nothing is synchronised with the host: the
 * total norm and the clip coefficient stay in device memory and dsc_adam_step_f32 multiplies every gradient by
 * *grad_scale (NULL = 1) while it reads it.  Arithmetic of torch.optim.Adam (amsgrad=False, maximize=False):
 *   g += weight_decay * p;  m += (g - m)(1 - beta1);  v = v beta2 + (1 - beta2) g g;
 *   p -= step_size * m / (sqrt(v) / bias_correction2_sqrt + eps),   step_size = lr / (1 - beta1^t).
 * ------------------------------------------------------------------------------------------- */
typedef struct dsc_optim_chunk {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;
} dsc_optim_chunk;

int dsc_grad_sumsq_f32(const dsc_optim_chunk* chunks, int32_t nchunks, double* partial, dsc_stream_t stream);
int dsc_clip_coef_f32(const double* partial, int32_t nchunks, float max_norm, float* total_norm, float* clip_coef,
                      dsc_stream_t stream);
int dsc_adam_step_f32(const dsc_optim_chunk* chunks, int32_t nchunks, float step_size, float beta1, float beta2,
                      float bias_correction2_sqrt, float eps, float weight_decay, const float* grad_scale,
                      dsc_stream_t stream);

/* Weight EMA (the exponential moving average of the parameters that DDPM recipes sample from), over the same work list.
 * dsc_optim_chunk is unchanged: the average's addresses travel in a parallel DEVICE array `ema` of nchunks entries,
 * ema[i] = address of the average of the elements chunks[i] covers.  One expression everywhere, three float32
 * statements with one rounding each (1 - ema_decay is formed in float32 from the argument):
 *   d = p - e;  d = d * (1 - ema_decay);  e = e + d.
 * The f32x4 path of a chunk needs ema[i] 16-byte aligned like the chunk's other pointers and count % 4 == 0; any other
 * chunk takes the scalar path, with the same results.  ema == NULL or !(0 <= ema_decay < 1) -> DSC_EINVAL, no launch.
 *
 * dsc_adam_ema_step_f32: the sweep of dsc_adam_step_f32 (same code: param, exp_avg, exp_avg_sq come out bit-identical)
 *   followed per element, in registers, by the EMA expression on the NEW parameter value.  36 B/parameter.
 * dsc_ema_update_f32: the EMA expression alone (reads chunks[i].param and .count only) -- for optimizers other than
 *   the fused Adam; bit-identical to the EMA half of dsc_adam_ema_step_f32.  12 B/parameter.
 * dsc_ema_swap_f32: exchanges param and ema element for element, in place, as bit patterns (NaN payloads and signed
 *   zeros survive); reads chunks[i].param and .count only.  16 B/parameter. */
int dsc_adam_ema_step_f32(const dsc_optim_chunk* chunks, float* const* ema, int32_t nchunks, float step_size, float beta1,
                          float beta2, float bias_correction2_sqrt, float eps, float weight_decay, const float* grad_scale,
                          float ema_decay, dsc_stream_t stream);
int dsc_ema_update_f32(const dsc_optim_chunk* chunks, float* const* ema, int32_t nchunks, float ema_decay,
                       dsc_stream_t stream);
int dsc_ema_swap_f32(const dsc_optim_chunk* chunks, float* const* ema, int32_t nchunks, dsc_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * FoldingNet KL auto-encoder (scene_synthesis/networks/foldingnet_autoencoder.py:56-390), the pieces around its 1x1
 * convolutions (which are dsc_gemm_f32 calls).  Point features are token-major [cloud * n + point][channel].
 * ------------------------------------------------------------------------------------------- */
/* knn() (:59-76): the 16 nearest points of every point inside its own cloud (itself included), nearest first; idx [clouds*n][16]
 * holds point indices inside the cloud.  dim == 3 and gram == NULL: distances from the coordinates; otherwise
 * gram = per-cloud Gram matrices [clouds][n][n] (a batched dsc_gemm_f32 of the features with themselves) and sqnorm[rows] =
 * squared row norms (dsc_rowsq_f32).  16 <= n <= 2048. */
int dsc_knn16_f32(const float* x, int64_t ldx, int32_t dim, const float* gram, const float* sqnorm, int32_t clouds, int32_t n,
                  int32_t* idx, dsc_stream_t stream);
int dsc_rowsq_f32(const float* x, int64_t ldx, int32_t dim, int64_t rows, float* out, dsc_stream_t stream);
/* Encoder input (:197-205): out[q][0:3] = xyz, out[q][3:12] = covariance sums of the 16 neighbours (row-major 3x3). */
int dsc_knn_cov_f32(const float* xyz, int64_t ldx, const int32_t* idx, int32_t clouds, int32_t n, float* out, int64_t ldo,
                    dsc_stream_t stream);
/* GraphLayer local max pooling (:160-165) and its backward (dx must be zero-filled; fp32 atomic adds). */
int dsc_gather_max_f32(const float* x, int64_t ldx, const int32_t* idx, int32_t clouds, int32_t n, int32_t ch, float* out,
                       int64_t ldo, uint8_t* arg, dsc_stream_t stream);
int dsc_gather_max_bwd_f32(const float* dy, int64_t ldy, const int32_t* idx, const uint8_t* arg, int32_t clouds, int32_t n,
                           int32_t ch, float* dx_zeroed, int64_t lddx, dsc_stream_t stream);
/* nn.BatchNorm1d over the rows of x [rows][ch] (+ ReLU when relu != 0).  Training form: batch statistics (biased variance for
 * the normalisation, unbiased for running_var; running_* may be NULL), xhat (may be NULL) and y dense [rows][ch];
 * workspace >= dsc_bn_workspace_floats(rows, ch).  Eval form: mean / rstd given.  Backward: dense dy, xhat, y. */
int64_t dsc_bn_workspace_floats(int64_t rows, int32_t ch);
int dsc_batchnorm_fwd_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, int64_t rows, int32_t ch, float eps,
                          float momentum, int32_t relu, float* mean, float* rstd, float* running_mean, float* running_var,
                          float* xhat, float* y, float* workspace, int64_t workspace_floats, dsc_stream_t stream);
int dsc_batchnorm_eval_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* mean,
                           const float* rstd, int64_t rows, int32_t ch, int32_t relu, float* y, dsc_stream_t stream);
int dsc_batchnorm_bwd_f32(const float* dy, const float* xhat, const float* y, const float* gamma, const float* rstd, int64_t rows,
                          int32_t ch, int32_t relu, float* dx, float* dgamma, float* dbeta, float* workspace,
                          int64_t workspace_floats, dsc_stream_t stream);
/* Global max pooling over the points of a cloud (:219): out [clouds][ch], arg = first point attaining it; backward dense. */
int dsc_rowmax_f32(const float* x, int64_t ldx, int32_t clouds, int32_t n, int32_t ch, float* out, int32_t* arg,
                   dsc_stream_t stream);
int dsc_rowmax_bwd_f32(const float* dy, const int32_t* arg, int32_t clouds, int32_t n, int32_t ch, float* dx, dsc_stream_t stream);
/* First convolution of a FoldingLayer (:247-251) on cat([x | codeword]) without the cat:
 * y[b*n + p][c] = sum_{k<d} wp[c][k] * x[row][k] + t[b][c], row = p (x_per_cloud == 0: the shared 2-D grid) or b*n + p, d <= 4,
 * t = Wc . codeword + bias from the GEMM.  Backward: dx (optional), dwp [ch][d], dt [clouds][ch]. */
int dsc_point_affine_f32(const float* x, int64_t ldx, int32_t x_per_cloud, const float* wp, int64_t ldw, const float* t,
                         int32_t clouds, int32_t n, int32_t ch, int32_t d, float* y, dsc_stream_t stream);
int dsc_point_affine_bwd_f32(const float* dy, const float* x, int64_t ldx, int32_t x_per_cloud, const float* wp, int64_t ldw,
                             int32_t clouds, int32_t n, int32_t ch, int32_t d, float* dx, int64_t lddx, float* dwp, int64_t lddw,
                             float* dt, float* workspace, int64_t workspace_floats, dsc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Floor-plan encoder (scene_synthesis/networks/feature_extractors.py: ResNet18 on the room mask; frozen_batchnorm.py), the pieces
 * around its convolutions' GEMMs (csrc/floorplan.hip).  Images are channel-last, token-major: x [b * h * w][c], row = (b * h + y) * w + x;
 * a (B, 1, H, W) mask is already in that layout.  Every kernel is a gather with a fixed summation order (no atomics): results are
 * deterministic for a shape.  Element offsets are int64; b * h * w and the output row count must fit int32 (else DSC_ERANGE), h, w, c <= 4096.
 * Channel counts that are a multiple of 4 with 16-byte aligned bases move 16 bytes per lane, anything else 4 bytes per lane, same results.
 * ------------------------------------------------------------------------------------------- */
/* Patch gather of a k x k convolution (k in {1, 3, 7}, stride in {1, 2}, 0 <= pad < k, zero padding; anything else DSC_EINVAL):
 *   patches[(b * ho + oy) * wo + ox][(ky * k + kx) * c + ch] = x[b][oy * stride - pad + ky][ox * stride - pad + kx][ch]   (0 outside)
 * ho = (h + 2 pad - k) / stride + 1, wo likewise; patches is dense [b * ho * wo][kpad], kpad = k * k * c rounded up to a multiple of 32
 * (the K granule of dsc_gemm_f32), columns [k * k * c, kpad) are written as zero.  The convolution is then dsc_gemm_f32 with the weight
 * as [out][(ky, kx, ch)] padded to kpad.  The backward sums, for every input element, the at most k * k patch entries that read it, taps
 * in (ky, kx) row-major order. */
int dsc_conv_patches_f32(const float* x, float* patches, int32_t b, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride,
                         int32_t pad, dsc_stream_t stream);
int dsc_conv_patches_bwd_f32(const float* dpatches, float* dx, int32_t b, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride,
                             int32_t pad, dsc_stream_t stream);
/* nn.MaxPool2d(3, stride 2, padding 1): y [b * ho * wo][c], ho = (h - 1) / 2 + 1.  The padding never wins; among equal maxima the first
 * in row-major window order wins and NaN propagates (torch.nn.functional.max_pool2d); arg holds the winner's window slot ky * 3 + kx.
 * The backward is a gather: every input element sums dy of the at most four windows whose winner it is (oy, ox ascending). */
int dsc_maxpool2d_f32(const float* x, float* y, uint8_t* arg, int32_t b, int32_t h, int32_t w, int32_t c, dsc_stream_t stream);
int dsc_maxpool2d_bwd_f32(const float* dy, const uint8_t* arg, float* dx, int32_t b, int32_t h, int32_t w, int32_t c,
                          dsc_stream_t stream);
/* FrozenBatchNorm2d.forward (frozen_batchnorm.py:56-68) with the residual add and ReLU of a BasicBlock behind it:
 *   y = act(x * s[c] + t[c] (+ residual)),  s = weight / sqrt(running_var),  t = bias - running_mean * s,  act = ReLU when relu != 0.
 * The reference's constructor already added eps to running_var; no second eps is added here.  weight == NULL (then bias, running_mean
 * and running_var too): y = act(x (+ residual)), the plain ReLU of the head.  ch a power of two in [4, 1024] (else DSC_ERANGE), dense
 * [rows][ch], 16-byte aligned (else DSC_EALIGN).
 * Backward: g = dy * [y > 0] (relu; y is the forward's output) or dy; dx = g * s; dresidual (optional) = g; dweight[c] = sum over rows
 * of g * ((x - running_mean[c]) / sqrt(running_var[c])), dbias[c] = sum of g: column sums in a fixed order through `workspace`
 * (>= dsc_frozen_bn_workspace_floats(rows, ch) floats, 8-byte aligned: it holds float64 partial sums).  weight == NULL: x, dweight, dbias
 * NULL as well, no workspace.  Forward and backward evaluate their expressions in float64 and round to float32 once, as do the sums of
 * dsc_conv_patches_bwd_f32 and dsc_avgpool_rows_f32. */
int dsc_frozen_bn_act_f32(const float* x, const float* weight, const float* bias, const float* running_mean, const float* running_var,
                          const float* residual, float* y, int64_t rows, int32_t ch, int32_t relu, dsc_stream_t stream);
int64_t dsc_frozen_bn_workspace_floats(int64_t rows, int32_t ch);
int dsc_frozen_bn_act_bwd_f32(const float* dy, const float* y, const float* x, const float* weight, const float* running_mean,
                              const float* running_var, float* dx, float* dresidual, float* dweight, float* dbias, int64_t rows,
                              int32_t ch, int32_t relu, float* workspace, int64_t workspace_floats, dsc_stream_t stream);
/* nn.AdaptiveAvgPool2d((1, 1)): x [b][hw][ch] -> y [b][ch] = (sum over hw, ascending) / hw; backward dx[b][p][ch] = dy[b][ch] / hw. */
int dsc_avgpool_rows_f32(const float* x, float* y, int32_t b, int32_t hw, int32_t ch, dsc_stream_t stream);
int dsc_avgpool_rows_bwd_f32(const float* dy, float* dx, int32_t b, int32_t hw, int32_t ch, dsc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFUSCENE_HIP_H */
