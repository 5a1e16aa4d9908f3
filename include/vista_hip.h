/* libvista_hip.so -- C ABI of the MI355X (gfx950) kernels behind the Vista denoising hot path.
 *
 * Contract: every entry point borrows device pointers, enqueues on the given HIP stream, performs
 * no allocation and no synchronisation, and returns 0 or a negative errno-style code (-22 bad argument, -5 launch
 * failure). The reference has no FFI of its own (it is pure Python); each function below names the reference
 * call site (file:line under the Vista tree) whose third-party ATen / xformers arithmetic it replaces. The Python
 * boundary classes in vista_amd/modules mirror the reference classes and are the only callers.
 *
 * Activation layout everywhere: token-major "NHWC" bf16, tensor[(b*T + t)][y*W + x][c], c contiguous.
 * bf16 is passed as uint16_t bit patterns. "stream" is a hipStream_t passed as void*.
 */
#ifndef VISTA_HIP_H
#define VISTA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ GEMM / implicit-GEMM convolution */
enum { VK_AMODE_DENSE = 0, VK_AMODE_CONV3X3 = 1, VK_AMODE_TEMPORAL3 = 2, VK_AMODE_CONV3D = 3, VK_AMODE_UPCONV2X2 = 4 };
enum { VK_EPI_LINEAR = 0, VK_EPI_GEGLU = 1, VK_EPI_TRANS = 2 };
/* VK_AMODE_UPCONV2X2 (added under ABI v9 without a version step: a new enum value, no field or meaning of VkGemmDesc changes): the Upsample of the UNet,
 * nearest x2 followed by a 3x3 convolution with pad 1 (openaimodel.py:100-102), as FOUR 2x2 convolutions of the source image. Tap ky of output row
 * 2i + a reads source row (2i + a + ky - 1) >> 1 -- i-1, i, i for a = 0 and i, i, i+1 for a = 1 -- and likewise in x, so output pixel (2i + a, 2j + b)
 * is a 2x2 convolution whose window starts at source pixel (i + a - 1, j + b - 1) (zero padding of the SOURCE reproduces the borders exactly) and whose
 * weights are sums of the nine taps: rows {w[0], w[1] + w[2]} for a = 0, {w[0] + w[1], w[2]} for a = 1, columns by the same rule with b. K = 4 Cin
 * instead of 9 Cin at the same output rows; exact in real arithmetic.
 *   A    NHWC source [n_img][H][Wd][Cin], Cin % 64 == 0;  H, Wd the source size, Hout = 2 H, Wout = 2 Wd, ups = 2, stride = 1, asym_pad = 0
 *   Wt   four class packs one after another, class 2a + b at rows [(2a + b) * pad(N), (2a + b + 1) * pad(N)), each [pad(N)][Cin/64][2 dy + dx][64]
 *        (vista_amd/ops.py: pack_upconv2x2 folds them in fp32 and rounds once); bias: one vector
 *   out  [M][ldc], M = n_img * 4 H Wd output rows in the usual order; K = 4 Cin; rowvec with rows_per_vec = 4 H Wd
 * The plain LINEAR epilogue only (bias, rowvec; 16-bit out): res1 / res2 / rowvec2, gnstat_out, rowstat_out, out_f32, mx8_out, ln_stats, act,
 * alt_cols_from, halos and a row range are VK_EINVAL. It exists on the eight-wave pipelined 256x320 kernel alone (tile_cfg 0 or 7; + 8 = walk the
 * tiles class-fastest instead of class-slowest, bitwise the same output): where the nine-tap form of the same layer would NOT run there as one launch
 * without K slices (N % 320 != 0, too few rows to fill the chip, an operand of 4 GiB), every entry point returns VK_EINVAL and the caller runs
 * VK_AMODE_CONV3X3 with ups = 2 on a nine-tap pack, which is unchanged. vk_gemm_tile_choice answers for it without a launch. */

typedef struct VkGemmDesc {
    const void* A;       /* bf16 activations: [M][lda] (DENSE) or NHWC source image stack (conv modes)            */
    const void* Wt;      /* bf16 weights [pad(N)][K] (pad: multiple of 256 and >= ceil320(N)), K contiguous; conv: [Cout][Cin/64][tap][64]                    */
    void* out;           /* bf16 or f32 [M][ldc]; EPI_TRANS: bf16 [M/S][N][S]                                     */
    const float* bias;   /* [ceil256(N)] f32 or NULL (EPI_GEGLU: in packed row order)                             */
    const float* rowvec; /* f32 [M/rows_per_vec][ldv] added per image, or NULL                                    */
    const void* res1;    /* bf16 [M][ld_res1] residual added before alpha, or NULL                                */
    const void* res2;    /* bf16 [M][ld_res2] residual added with beta, or NULL                                   */
    int32_t M, N, K;
    int32_t lda, ldc, ld_res1, ld_res2, ldv, rows_per_vec;
    float alpha, beta;   /* out = alpha*(acc + bias + rowvec + res1) + beta*res2                                  */
    int32_t amode, epi, out_f32;
    int32_t H, Wd, Cin, Hout, Wout, stride, ups; /* CONV3X3: source H x Wd (before the x`ups` nearest upsample)   */
    int32_t T, S;        /* TEMPORAL3: frames per clip, tokens per frame. EPI_TRANS: S = tokens per image.
                            CONV3D (3x3x3, pad 1 over [frames][H][Wd][Cin], K = 27*Cin): T = frames per clip        */
    int32_t tile_cfg;    /* 0 = auto; forced variants (tests / tuning): 1 = 128x128, 2 = 256x128, 3 = 256x256, 4 = 256x320 (sixteen waves),
                            5 = 128x160 (two workgroups per CU; DENSE LINEAR), 6 = the weight-stationary streaming kernel (K = 320, N = 320 / 640 /
                            960), 7 = 256x320 eight-wave pipelined kernel (DENSE / CONV3X3 / TEMPORAL3 without halos x LINEAR, bf16 out,
                            DENSE x GEGLU; bitwise equal to 4). A variant that does not take the problem falls back to the launcher's choice.
                            Weight rows are zero-padded to max(ceil256(N), ceil320(N)) so every variant reads whole tiles.
                            + 64 (with variant 0): apply the tail-split rule of vk_gemm_tail_split (measured without gain; this bit is the only way to ask for it).
                            + 16: the four-wave pipelined 128x320 kernel, two workgroups per CU (DENSE x LINEAR / GEGLU, 16-bit out; bitwise equal
                            to 7; measured slower, this bit is the only way to ask for it) wherever it takes the problem and leaves the row-sum slabs alone.        */
    const void* halo_prev; /* TEMPORAL3, frame-sharded runs: bf16 [clips][S][Cin] frame preceding / following the local frame range   */
    const void* halo_next; /* (from the neighbour rank); NULL = the conv's zero padding at the window ends                               */
    void* splitk_ws;     /* optional fp32 workspace for split-K of small-M, deep-K LINEAR problems (NULL = never split); must not be  */
    int64_t splitk_ws_bytes; /* shared by GEMMs in flight on different streams. A split needs slices * M * N * 4 bytes.              */
    int32_t asym_pad;    /* CONV3X3: 0 = zero padding 1 on all sides; 1 = padding (0,1,0,1) = bottom/right only, the VAE encoder's
                            Downsample (vwm/modules/diffusionmodules/model.py:77-81: F.pad(x, (0,1,0,1)) then conv stride 2 pad 0)  */
    /* ---- DENSE two-source A: the channel concat of the UNet skip (video_model.py:493) folded into the loader ---- */
    int32_t k_split;     /* columns k >= k_split of A come from A2[m][k - k_split]; a multiple of 64; used only when A2 != NULL    */
    const void* A2;      /* bf16 [M][lda2] or NULL                                                                              */
    int32_t lda2;
    /* ---- LayerNorm folded into the consumer GEMM (attention.py:514-524, video_attention.py:119-137: `Linear(LayerNorm(x))`):
     *   LN(x) W^T + b = rstd_m * (x W'^T - mean_m * s_n) + t_n,  W' = gamma (.) W,  s_n = sum_k W'[n][k],  t_n = (W beta)_n + b_n.
     * Wt holds W', bias holds t, ln_colsum holds s (of the bf16-rounded W' so that the mean term cancels exactly); mean_m / rstd_m
     * come from per-row partial sums (sum x, sum x^2) over column blocks of x, summed here in a fixed order. DENSE only, K = LN width. */
    int32_t ln_parts;    /* number of partial-sum slabs                                                                         */
    const float* ln_stats;  /* f32 [ln_parts][M][2] or NULL (= no LayerNorm fold)                                               */
    const float* ln_colsum; /* f32 [pad(N)] (EPI_GEGLU: packed row order)                                                       */
    float ln_eps;
    /* ---- producer side of the same fold: emit the row sums of the bf16-rounded OUTPUT of this GEMM (EPI_LINEAR, bf16 out) ---- */
    float* rowstat_out;  /* f32 [vk_gemm_rowstat_parts(desc)][M][2] or NULL; one slab per (column tile, wave column)               */
    const float* rowvec2; /* f32 [M/rows_per_vec][ldv] or NULL, added with beta: out = alpha*(...) + beta*(res2 + rowvec2[row/rows_per_vec]) */
    int32_t act;         /* EPI_LINEAR: 0 = none; 1 = exact-erf GELU applied to (acc + bias + rowvec) BEFORE res1 / alpha -- the MLP of the
                            conditioner's OpenCLIP image tower: c_fc -> nn.GELU -> c_proj (vwm/modules/encoders/modules.py:273-279)           */
    /* ---- BASELINE config 5: MX-fp8 output of the LEADING columns of a LINEAR GEMM (no quantisation pass): output columns [0, mx8_cols) are
     *   written as e4m3 bytes to mx8_out[m][n] with one E8M0 scale per row and 32 columns in mx8_scales[m][n / 32] (2^e >= max|v| / 448,
     *   chosen in the epilogue); columns n >= mx8_cols go to out[m][n - mx8_cols] (ldc counts `out`'s own columns). The q | k blocks of the fused
     *   q|k|v projection feeding the fp8 QK^T of vk_attn_spatial_fp8qk (attention.py:344-346,391-407), and the FeedForward output feeding an
     *   fp8 proj_out. N % 320 == 0, mx8_cols % 320 == 0, ld_mx8 % 16 == 0; bf16 out, no rowstat_out on those columns.                       */
    void* mx8_out;
    void* mx8_scales;
    int32_t mx8_cols, ld_mx8, ld_mx8s;
    /* ---- row range (ABI v5): this call computes output rows [m_begin, m_end) of the M-row problem only; 0 / 0 = all rows. Everything else
     *   (M as the extent of the operands, of the row-sum slabs and of the conv / temporal sources) is unchanged, so a problem may be covered by
     *   several calls with bitwise the same result as one call. vk_gemm_bf16 uses it itself: when the last round of a one-tile-per-workgroup
     *   launch would leave most of the chip idle (tiles mod 256 small), the whole rounds run on the 256x320 pipelined kernel and the remaining
     *   rows as a second launch of 128x160 tiles. EPI_LINEAR / EPI_GEGLU, no split-K. ---- */
    int32_t m_begin, m_end;
    /* ---- GroupNorm statistics of the OUTPUT from the epilogue (ABI v6): the GroupNorm32 that follows a ResBlock convolution (openaimodel.py:195-199,
     *   227-234; video_model.py:38-52) needs (sum, sum of squares) per image and group of N/32 channels; instead of a read pass of its own over the
     *   tensor this GEMM is writing, the epilogue emits the stage-1 partials of vk_groupnorm_stats_bf16 -- one slot of 64 floats [32 sums | 32 sums of
     *   squares] per 64 consecutive output rows, taken from the bf16-rounded values it stores, in a fixed order (bitwise reproducible) --
     *   and vk_groupnorm_finalize_partials folds them per image group (nchunks = gn_rows / 64). Only launches for which vk_gemm_gnstat_fit() > 0
     *   may set gnstat_out (vk_gemm_bf16 returns an error otherwise): EPI_LINEAR, bf16 out, CONV3X3 / TEMPORAL3 without halos, N = 320 / 640 / 1280,
     *   gn_rows % 64 == 0, the whole row range, on the 256x320 pipelined kernel in one launch (no split-K). ---- */
    float* gnstat_out;   /* f32 [M / 64][64] or NULL */
    int32_t gn_rows;     /* output rows per image (H*W of the output) */
    /* ---- fp16 storage build only (ABI v7; libvista_hip_f16.so, vk_act_dtype() == 1; the bf16 build ignores it): output columns n >= alt_cols_from
     *   of an EPI_LINEAR 16-bit-out launch are written as bf16 instead of fp16. 0 = none; a multiple of 32. The V column block of the fused q|k|v
     *   projections (attention.py:344-346): the attention kernels keep the P.V product in bf16 in both builds (their zero-base softmax needs bf16's
     *   exponent range for the numerators), so V must arrive as bf16 while q and k are fp16. No row sums / GroupNorm statistics on such a launch. ---- */
    int32_t alt_cols_from;
} VkGemmDesc;

/* nn.Linear / nn.Conv2d / nn.Conv3d call sites of the UNet:
 *   vwm/modules/attention.py:85-92,117-121 (GEGLU FF), :344-346,421 (q,k,v,out), :579,602 (proj_in/out)
 *   vwm/modules/diffusionmodules/openaimodel.py:136 (Downsample), :84,100-102 (Upsample), :195-199,227-234 (ResBlock convs), :241 (skip)
 *   vwm/modules/diffusionmodules/video_model.py:38-52 (3x1x1 temporal conv), :148-157,176-182 (embedding MLPs), :189,438 (in/out conv) */
/* Operand contract of vk_gemm_bf16 and its four plan queries (which hold every operand to this table alike: a query answers VK_EINVAL for an operand
 * the launch would refuse. The shape rules of an epilogue -- ldc % 4, N % 32 for EPI_GEGLU, S % 4 for EPI_TRANS, which is what keeps that epilogue's
 * 8-byte stores aligned -- are checked by vk_gemm_bf16 alone, as before: the queries answer for the shape as given):
 * base alignment in bytes and leading-dimension multiple in elements, from the widest access any kernel the plan may pick makes to the operand.
 * An operand outside its row is VK_EINVAL before any launch; what only a faster path needs is that path's to check, and it declines.
 *   operand                              base   leading dimension        widest access
 *   A, A2, halo_prev, halo_next, Wt      16     lda % 8, lda2 % 8        16-byte LDS-DMA / uint4 pieces (conv modes: rows of Cin % 64 elements)
 *   out, 16-bit                          8      ldc % 4                  uint2 stores of the general epilogue (EPI_TRANS: rows of S % 4 keys, ldc unused)
 *     ... 16 and ldc % 8 select the 16-byte stores and the LDS-staged epilogue; the pipelined (7, + 16) and streaming (6) kernels need them and
 *     decline otherwise, as they do for a residual that is not 16-byte aligned with ld % 8
 *   out, fp32 (out_f32)                  16     ldc % 4                  float4 stores
 *   res1, res2                           8      ld_res1 % 4, ld_res2 % 4 uint2 loads
 *   bias, ln_colsum                      16     -                        float4 loads (EPI_TRANS: 4, one float per lane)
 *   rowvec, rowvec2                      16     ldv % 4                  float4 loads
 *   ln_stats, rowstat_out                8      -                        float2 (sum, sum of squares)
 *   gnstat_out                           4      -                        floats
 *   splitk_ws                            16     -                        float4 partials
 * The L2-prefetch variant of the pipelined kernel additionally wants A 128-byte aligned with lda % 64 == 0 and is bitwise the plain variant.
 * vk_ff_fused_bf16: geglu->A 16 / lda % 8, both Wt 16, geglu->bias / ln_colsum 16, ln_stats 8; out_proj's out / res* / bias / rowvec* / rowstat_out as above. */
int vk_gemm_bf16(const VkGemmDesc* d, void* stream);

/* Number of partial-sum slabs vk_gemm_bf16 would write to d->rowstat_out for this problem (depends on the block tile the launcher
 * picks: column tiles x wave columns); > 0, or a negative error code. Pure host function, no launch. */
int vk_gemm_rowstat_parts(const VkGemmDesc* d);
/* The launcher's decision for `desc` without launching anything (host arithmetic only): block-tile variant (1 = 128x128, 2 = 256x128,
 * 3 = 256x256, 4 = 256x320, 5 = 128x160) * 16 + number of K slices; negative = the error vk_gemm_bf16 would return. */
int vk_gemm_tile_choice(const VkGemmDesc* d);
/* The output row at which vk_gemm_bf16 would split this problem into two launches (whole rounds of 256x320 tiles on the pipelined kernel +
 * the remaining rows as 128x160 tiles; VkGemmDesc.m_begin / m_end), 0 = a single launch; negative = the error vk_gemm_bf16 would return.
 * Pure host function, no launch. */
int vk_gemm_tail_split(const VkGemmDesc* d);
/* ABI v6: > 0 (= M / 64, the number of 64-float slots gnstat_out needs) when vk_gemm_bf16 would take `d` with gnstat_out set, 0 when this
 * problem cannot emit GroupNorm statistics (the caller then runs vk_groupnorm_stats_bf16 as before); negative = the error vk_gemm_bf16 would
 * return. Evaluated with d->gnstat_out ignored (the launcher's kernel choice does not depend on it). Pure host function, no launch. */
int vk_gemm_gnstat_fit(const VkGemmDesc* d);

/* fp8 (OCP e4m3) variant of the DENSE GEMM for the UNet's Linear / 1x1 projections (BASELINE.json config 5: "fp8 1x1
 * conv-as-GEMM path"; same reference call sites as vk_gemm_bf16's DENSE mode: attention.py:268-285,97-128, video_attention.py).
 *   out = epilogue( a_scale[m] * w_scale[n] * sum_k Aq[m][k] * Wq[n][k] )
 * d->A = fp8 activations [M][lda] (bytes), d->Wt = fp8 weights [ceil-tile(N)][d->K] with d->K = row stride, a multiple of 128,
 * zero-filled past k_real; a_scale [M] per-row, w_scale [ceil-tile(N)] per-output-channel (GEGLU: packed row order);
 * amode must be DENSE, epi LINEAR or GEGLU; the epilogue fields (bias, rowvec, res1/res2, alpha/beta, out_f32) as for bf16. */
int vk_gemm_fp8(const VkGemmDesc* desc, const float* a_scale, const float* w_scale, int32_t k_real, void* stream);

/* The same GEMM with the round-2 options (all optional; vk_gemm_fp8(d, a_scale, w_scale, k_real) == {a_scale, w_scale, k_real, 0...}):
 *   a_mx / ld_mx     : MX block scales of the activations INSTEAD of a_scale: E8M0 bytes (2^(e-127)) [M][ld_mx], one per 32 consecutive
 *                      K-elements, applied inside v_mfma_scale_f32_32x32x64_f8f6f4; ld_mx % 4 == 0 and ld_mx * 32 >= d->K. The kernel reads
 *                      all d->K / 32 scale bytes of a row: the pad bytes past k_real / 32 multiply zero-filled activation chunks, so they
 *                      must hold a finite E8M0 value (producers write 127 = 2^0), never 0xFF, the E8M0 NaN.
 *   mx_out / ld_mx_out: EPI_GEGLU only: write the gated output as MX fp8 -- d->out = e4m3 bytes [M][d->ldc], mx_out = E8M0 [M][ld_mx_out],
 *                      one scale per 32 output columns, chosen in the epilogue (2^e >= max|h| / 448) -- so that the FeedForward's second
 *                      GEMM (a_mx = this mx_out) needs no quantisation pass (attention.py:85-128). (N/2) % 32 == 0, ldc % 16 == 0.
 * d->rowstat_out is honoured (vk_gemm_fp8_rowstat_parts sizes it).
 * Implicit-GEMM convolutions (d->amode = CONV3X3 / TEMPORAL3, the ResBlock convolutions of openaimodel.py:300-318 / video_model.py:38-52 on
 * the e4m3 output of vk_groupnorm_silu_fp8): stride 1, pad 1, no upsample / halo, weights [Cout][Cin/64][tap][64] bytes padded to a multiple
 * of 128 per row (d->K), k_real = taps * Cin, Cin % 64 == 0, bf16 output, a_scale + a_scale_rows. */
typedef struct VkFp8Args {
    const float* a_scale;
    const float* w_scale;
    int32_t k_real;
    const void* a_mx;
    int32_t ld_mx;
    void* mx_out;
    int32_t ld_mx_out;
    int32_t a_scale_rows; /* 0 / 1: a_scale is per row; n > 1: one scale per n consecutive rows (the per-image scales of
                             vk_groupnorm_silu_fp8: n = H*W, or T*H*W for the temporal norm) */
} VkFp8Args;
int vk_gemm_fp8_mx(const VkGemmDesc* desc, const VkFp8Args* args, void* stream);
int vk_gemm_fp8_rowstat_parts(const VkGemmDesc* d);

/* Fused FeedForward of the level-0 (width 320) transformers: net = [GEGLU, Dropout, Linear] (vwm/modules/attention.py:85-128) applied as
 * `x = ff(norm3(x)) + x` (attention.py:524) and as ff_in / ff of the temporal block with its AlphaBlender mix (video_attention.py:119-121,
 * 137-141) -- ONE kernel, the hidden activation (M x 1280 bf16, 1.18 GB per call at the BASELINE shape) never goes to HBM.
 *   geglu    : the in-projection exactly as vk_gemm_bf16 would take it (amode DENSE, epi GEGLU: A = x [M][lda], Wt = packed GEGLU weight
 *              [2 Hd][320], bias, optional folded LayerNorm ln_*); K must be 320. `out` / `ldc` are ignored.
 *   out_proj : the out-projection as vk_gemm_bf16 would take it (amode DENSE, epi LINEAR, bf16 out: bias, rowvec / rowvec2, res1 / res2,
 *              alpha / beta, rowstat_out), N = 320, K = Hd (a multiple of 64, 128 <= Hd <= 1280), with ONE difference: Wt's K axis is
 *              permuted inside every group of 16 hidden units to [0-3, 8-11, 4-7, 12-15] (the order in which a lane of the
 *              in-projection's MFMA accumulator holds them, so the hidden values feed the second MFMA straight from registers) and the
 *              matrix is stored chunk-major, bf16 [Hd / 32][320][32] (a 32-wide hidden chunk of all rows = one contiguous 20 KB block;
 *              bias f32 [320]). `A` / `lda` are ignored.
 * The hidden activation is rounded to bf16 exactly where the two-kernel form rounds it; rowstat_out gets vk_ff_fused_rowstat_parts()
 * slabs ([parts][M][2]). Same return codes as vk_gemm_bf16. */
int vk_ff_fused_bf16(const VkGemmDesc* geglu, const VkGemmDesc* out_proj, void* stream);
int vk_ff_fused_rowstat_parts(void);

/* GroupNorm(32)[+SiLU] with e4m3 output and ONE scale per image group (of frames_per_group images): y8 = e4m3(y / scale[g]), scale[g] =
 * (max_c |a_c| max|x| + |b_c|) / 448 with y = a_c x + b_c the folded affine form -- an upper bound from the statistics pass (which also
 * tracks max|x|), so no extra pass over the data; a conv output pixel sums taps of its own image only, so the scale factors out of the
 * fp8 convolution (VkFp8Args.a_scale_rows). x2 != NULL: the input is the channel concat [x1 | x2] (C1 + C2 channels), as
 * vk_groupnorm_silu_cat_bf16. stats_ws: floats, groups * 64 + n_img * ceil(S / 32) * 65.
 * Reference: GroupNorm32 + SiLU of openaimodel.py:281-298, video_model.py:38-52. */
int vk_groupnorm_silu_fp8(const void* x1, const void* x2, void* y8, float* scale_out, const float* gamma, const float* beta, float* stats_ws,
                          int32_t n_img, int32_t S, int32_t C1, int32_t C2, int32_t frames_per_group, float eps, int32_t silu, void* stream);

/* LayerNorm fused with per-row dynamic fp8 quantisation: y = LN(x)*gamma + beta (as vk_layernorm_bf16), scale[r] = max|y[r]| / 448,
 * q[r] = e4m3(y[r] / scale[r]) -- one pass, the normalised tensor is never written in bf16 (FeedForward input of the fp8 configuration:
 * attention.py:524, video_attention.py:119-137). C % 8 == 0, C <= 1536. */
int vk_layernorm_quant_fp8(const void* x, void* q, float* scale, const float* gamma, const float* beta, int32_t rows, int32_t C, float eps,
                           void* stream);

/* Per-row dynamic quantisation bf16 -> fp8 e4m3: scale[m] = max|x[m][:]| / 448, q = e4m3(x / scale). K % 8 == 0, K <= 5120. */
int vk_quantize_rows_fp8(const void* x, void* q, float* scale, int32_t M, int32_t K, int64_t ldx, int64_t ldq, void* stream);

/* ------------------------------------------------------------------ attention */
/* Spatial self-attention, softmax(q k^T * scale) v per (image, head), head dim 64, no mask.
 * Replaces xformers.ops.memory_efficient_attention at vwm/modules/attention.py:400-407 for attn1 of
 * BasicTransformerBlock (attention.py:514-518).
 *   q, k : bf16, row (image*S + token) at q + row*ldq + head*64 (same for k / ldk)
 *   vt   : bf16 [n_img][heads][64][S]   (V transposed, produced by vk_gemm_bf16 EPI_TRANS)
 *   o    : bf16, row at o + row*ldo + head*64
 * S must be a multiple of 8.
 * Operands (all three spatial entries): q, k, vt / v 16-byte aligned with ldq % 8, ldk % 8, ldv % 8 (16-byte pieces); o 8-byte aligned with ldo % 4
 * (8-byte stores; the pipelined kernel of the pre-scaled form is taken only where o is 16-byte aligned with ldo % 8). Anything else: VK_EINVAL. */
int vk_attn_spatial_bf16(const void* q, const void* k, const void* vt, void* o, int32_t n_img, int32_t heads,
                         int32_t S, int32_t ldq, int32_t ldk, int32_t ldo, float scale, void* stream);

/* The same attention with V as a token-major column block [row][ldv] of the fused q|k|v projection (vwm/modules/attention.py:344-346 as ONE
 * GEMM): no V^T tensor and no second pass over x -- the kernel transposes the V tile on its way out of LDS (ds_read_b64_tr_b16).
 *   v : bf16, row (image*S + token) at v + row*ldv + head*64;  ldv % 8 == 0. Everything else as vk_attn_spatial_bf16. */
int vk_attn_spatial_qkv_bf16(const void* q, const void* k, const void* v, void* o, int32_t n_img, int32_t heads,
                             int32_t S, int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo, float scale, void* stream);

/* The same attention for a query that ALREADY carries softmax_scale * log2(e) -- folded into the to_q weight rows when they are packed
 * (vwm/modules/attention.py:344,400-407: q = to_q(x), scale = dim_head ** -0.5; one bf16 rounding of the scaled projection instead of one of the
 * unscaled one: no extra error). q . k is then the base-2 exponent itself; rows whose running maximum lies within +-60 octaves use the base 0
 * (P = exp2(q . k), no per-score scale / base arithmetic), others re-base on their true maximum exactly like vk_attn_spatial_qkv_bf16. */
int vk_attn_spatial_qkv_log2_bf16(const void* q, const void* k, const void* v, void* o, int32_t n_img, int32_t heads,
                                  int32_t S, int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo, void* stream);

/* Small dense attention, any head dim D in {64, 80, 128}: softmax(q k^T * scale) v per (image, head); q / k / v are column blocks of one
 * row-major buffer (q at qkv + row*ld + head*D, k at + k_off, v at + v_off; row = image*S + token). The nn.MultiheadAttention of the
 * conditioner's OpenCLIP ViT-H/14 image tower (FrozenOpenCLIPImageEmbedder, vwm/modules/encoders/modules.py:251-399: 257 tokens, 16 heads
 * of dim 80). 4*S*D bytes of LDS (<= 160 KiB).
 * Operands: qkv and o 16-byte aligned, ld % 8, k_off % 8, v_off % 8, ldo % 8 (16-byte loads and stores); else VK_EINVAL. */
int vk_attn_small_bf16(const void* qkv, void* o, int32_t n_img, int32_t heads, int32_t S, int32_t D, int32_t ld, int32_t k_off,
                       int32_t v_off, int32_t ldo, float scale, void* stream);

/* OpenCLIP image preprocessing + patchify (FrozenOpenCLIPImageEmbedder.preprocess, modules.py:304-315, and the im2col of the tower's
 * patch convolution): kornia-0.6.9 antialiased bicubic resize of img f32 [n][3][H][W] in [-1, 1] to out_hw x out_hw (Gaussian blur with
 * (sigma_y, sigma_x) / odd kernel sizes (ks_y, ks_x) <= 63, reflect border, then bicubic align_corners=True), (x + 1) / 2, CLIP mean / std
 * (HOST arrays of 3 floats), written as the bf16 A operand of the patch-embedding GEMM:
 *   out[(img * (1 + g*g) + 1 + py*g + px) * ldo + c*patch*patch + ky*patch + kx],  g = out_hw / patch.
 * Only those columns are written: the caller zero-fills `out` (class-token row of every image, K padding) once. */
int vk_clip_preprocess_patches(const float* img, void* out, int32_t n_img, int32_t H, int32_t W, int32_t out_hw, int32_t patch, int32_t ldo,
                               float sigma_y, float sigma_x, int32_t ks_y, int32_t ks_x, const float* mean3, const float* std3, void* stream);

/* BASELINE config 5: the same attention with the score product in fp8. q8 / k8: e4m3 bytes, row (image*S + token) at q8 + row*ldq8 + head*64;
 * q_scales / k_scales: E8M0 bytes, one per row and 32 head-dim elements, at + row*ldqs + 2*head + block -- the MX-fp8 q | k blocks written by the
 * fused q|k|v projection's epilogue (VkGemmDesc.mx8_out). S^T = K . Q^T runs as v_mfma_scale_f32_32x32x64_f8f6f4 with both block scales applied
 * inside the instruction; softmax, bf16 P and P.V on the bf16 V rows (v / ldv as in vk_attn_spatial_qkv_bf16) are unchanged.
 * Output: bf16 `o` (ldo), or -- o8 != NULL -- MX fp8: e4m3 bytes at o8 + row*ldo8 + head*64 and E8M0 scales at o_scales + row*ldos + 2*head + block,
 * which an fp8 attention-out projection consumes through VkFp8Args.a_mx (attention.py:391-421).
 * scale == 0: q already carries softmax_scale * log2(e) (the pre-scaled query of vk_attn_spatial_qkv_log2_bf16; zero-base softmax). */
int vk_attn_spatial_fp8qk(const void* q8, const void* k8, const void* q_scales, const void* k_scales, const void* v, void* o, void* o8,
                          void* o_scales, int32_t n_img, int32_t heads, int32_t S, int32_t ldq8, int32_t ldk8, int32_t ldqs, int32_t ldks,
                          int32_t ldv, int32_t ldo, int32_t ldo8, int32_t ldos, float scale, void* stream);

/* Temporal (cross-frame) self-attention over the T frames of every pixel: sequence length T <= 32, head dim 64.
 * Replaces the batchified xformers call at vwm/modules/attention.py:384-399 for VideoTransformerBlock.attn1
 * (vwm/modules/video_attention.py:116-127). Token rows are (b*T + t)*S + s; q,k,v are column blocks of one
 * row-major buffer: q at qkv + row*ld + head*64, k at + k_off, v at + v_off.
 * Operands: qkv 16-byte aligned, ld % 8, k_off % 8, v_off % 8 (16-byte loads); o 8-byte aligned, ldo % 4 (16-byte stores where o is 16-byte
 * aligned with ldo % 8, else 8-byte ones); else VK_EINVAL. */
int vk_attn_temporal_bf16(const void* qkv, void* o, int32_t B, int32_t T, int32_t S, int32_t heads, int32_t ld,
                          int32_t k_off, int32_t v_off, int32_t ldo, float scale, void* stream);

/* Row softmax, fp32 scores -> bf16 probabilities: y[r][c] = softmax_c(x[r][:cols]). cols % 4 == 0, cols <= 16384.
 * Replaces `torch.nn.functional.softmax(w_, dim=2)` of the VAE decoder's single-head AttnBlock
 * (vwm/modules/diffusionmodules/model.py:160-166); q.k^T (scaled) and P.v run as vk_gemm_bf16 calls either side.
 * Operands: x 16-byte aligned, ldx % 4 (float4 loads); y 8-byte aligned, ldy % 4 (uint2 stores); else VK_EINVAL. */
int vk_softmax_rows_f32_bf16(const float* x, void* y, int64_t rows, int32_t cols, int64_t ldx, int64_t ldy, void* stream);

/* ------------------------------------------------------------------ normalisation */
/* GroupNorm(32 groups) [+ SiLU] over token-major x[n_img][S][C]; statistics span `frames_per_group` consecutive
 * images (1 = per-image GroupNorm32 of the 2-D ResBlock / transformer entry norm; T = the 5-D norm of the
 * temporal ResBlock whose statistics cover (C/32, T, H, W)).
 * Replaces GroupNorm32/Normalize + nn.SiLU: vwm/modules/diffusionmodules/util.py:196-216, attention.py:141-142,
 * openaimodel.py:195-199,227-230, video_model.py:434-436.
 * stats_ws: f32 workspace of 64*(n_img/frames_per_group) + 64*n_img*ceil(S/32) floats (fixed-order partial sums:
 * results are bitwise reproducible, no atomics). In the fp16-storage build this call and vk_groupnorm_silu_cat_bf16 take their sums about each
 * group's first element, so that E[x^2] - mean^2 does not cancel at a large |mean| / std, and refuse y == x (VK_EINVAL: every workgroup of a
 * group reads that element while the first one would overwrite it); the sums that cross the ABI below stay raw, so a norm fed by a GEMM
 * epilogue's partials or by sharded statistics -- most of the UNet's ResBlock norms -- is computed as before in both builds.
 * Operands of the whole GroupNorm family (this call, _stats, _apply, _apply_partials, _finalize_partials, _cat): x / x1 / x2 / y 16-byte aligned
 * and dense, C (C1, C2) % 8 == 0 (16-byte loads and stores of 8-channel chunks); gamma, beta, sums, partial(_ws), stats_ws 4-byte aligned
 * (floats); else VK_EINVAL. */
int vk_groupnorm_silu_bf16(const void* x, void* y, const float* gamma, const float* beta, float* stats_ws,
                           int32_t n_img, int32_t S, int32_t C, int32_t frames_per_group, float eps, int32_t silu,
                           void* stream);

/* The two halves of vk_groupnorm_silu_bf16, for pixel-sharded multi-GPU runs of the temporal ResBlock: `sums` is
 * [n_img/frames_per_group][64] = raw [32 sums | 32 sums of squares] over the LOCAL elements (all-reduce them across ranks),
 * `partial_ws` needs 64*n_img*ceil(S/32) floats, `count` is the GLOBAL element count per (image-group, channel-group). */
int vk_groupnorm_stats_bf16(const void* x, float* sums, float* partial_ws, int32_t n_img, int32_t S, int32_t C,
                            int32_t frames_per_group, void* stream);
int vk_groupnorm_apply_bf16(const void* x, void* y, const float* gamma, const float* beta, const float* sums, int32_t n_img,
                            int32_t S, int32_t C, int32_t frames_per_group, float count, float eps, int32_t silu, void* stream);
/* ABI v6: the second stage of vk_groupnorm_stats_bf16 on partials somebody else produced (VkGemmDesc.gnstat_out): `partial` is
 * [n_img][nchunks][64] stage-1 slots (consumed: the fold of large groups works in place), `sums` [n_img/frames_per_group][64] as above.
 * Followed by vk_groupnorm_apply_bf16 (after the all-reduce of `sums` in a pixel-sharded run) it replaces vk_groupnorm_silu_bf16 without the
 * statistics pass over x. */
int vk_groupnorm_finalize_partials(float* partial, float* sums, int32_t n_img, int32_t nchunks, int32_t frames_per_group, void* stream);
/* ABI v7: the apply pass straight on stage-1 slots (`partial` as above, NOT consumed): every workgroup folds its image group's
 * frames_per_group * nchunks slots itself, in gn_finalize's summation order, so the output is bitwise that of vk_groupnorm_finalize_partials +
 * vk_groupnorm_apply_bf16 with one launch less (GroupNorm32 of openaimodel.py:195-199,227-234 = producer epilogue + ONE pass). Taken when
 * frames_per_group * nchunks <= vk_groupnorm_fold_max() (256), else VK_EINVAL. Not for pixel-sharded norms (their raw
 * sums are all-reduced between the two stages). vk_groupnorm_silu_bf16 / _cat_bf16 apply the same rule to their own statistics pass. */
int vk_groupnorm_fold_max(void);
int vk_groupnorm_apply_partials_bf16(const void* x, void* y, const float* gamma, const float* beta, const float* partial, int32_t n_img,
                                     int32_t S, int32_t C, int32_t nchunks, int32_t frames_per_group, float count, float eps, int32_t silu,
                                     void* stream);

/* LayerNorm over C of x[rows][C] (+ optional per-image pre-add vector):  u = x + addvec[row / rows_per_vec];
 * if sum_out: sum_out = u (bf16);  y = LN(u)*gamma + beta.
 * Replaces nn.LayerNorm at attention.py:514-524 (norm1-3) and video_attention.py:119-137 (norm_in, norm1-3),
 * fused with the `x_mix = x + emb` add of video_attention.py:283-284.
 * Operands: x, y, sum_out 16-byte aligned and dense, C % 8 == 0 (16-byte accesses); gamma, beta, addvec 4-byte aligned (floats); else VK_EINVAL. */
int vk_layernorm_bf16(const void* x, void* y, void* sum_out, const float* gamma, const float* beta,
                      const float* addvec, int32_t rows, int32_t C, int32_t rows_per_vec, int32_t ldv, float eps,
                      void* stream);

/* Row sums for a LayerNorm folded into the consumer GEMM (VkGemmDesc.ln_stats with ln_parts = 1) when the tensor was not produced
 * by a GEMM epilogue on this rank (pixel-sharded temporal block after the all-to-all): stats[row] = (sum_c x, sum_c x^2) of
 * x[rows][ldx] (first C columns), fixed order. Read-only pass: half the traffic of vk_layernorm_bf16. C % 8 == 0, C <= 1536.
 * Operands: x 16-byte aligned, ldx % 8 (16-byte loads); stats 8-byte aligned (float2 stores); else VK_EINVAL. */
int vk_rowstats_bf16(const void* x, float* stats, int32_t rows, int32_t C, int64_t ldx, void* stream);

/* vk_groupnorm_silu_bf16 over the channel concat [x1 | x2] (C1 + C2 channels, both token-major, C1 % 8 == C2 % 8 == 0) without
 * materialising it: the `torch.cat([h, hs.pop()], dim=1)` of the UNet's output blocks (video_model.py:493) feeding the ResBlock's
 * first GroupNorm32 (openaimodel.py:195-199). y is [n_img][S][C1+C2]. stats_ws as for vk_groupnorm_silu_bf16. */
int vk_groupnorm_silu_cat_bf16(const void* x1, const void* x2, void* y, const float* gamma, const float* beta, float* stats_ws,
                               int32_t n_img, int32_t S, int32_t C1, int32_t C2, int32_t frames_per_group, float eps, int32_t silu,
                               void* stream);

/* ------------------------------------------------------------------ elementwise / layout */
/* out[m][0:C1] = a[m][:], out[m][C1:C1+C2] = b[m][:]  (channel concat of the UNet skip: video_model.py:493)
 * Operands: a, b, out 16-byte aligned and dense, C1 % 8 == C2 % 8 == 0 (16-byte chunks); else VK_EINVAL. */
int vk_concat_channels_bf16(const void* a, const void* b, void* out, int64_t rows, int32_t C1, int32_t C2, void* stream);

/* NCHW float (f32) -> token-major bf16 with the channel dim zero-padded to Cpad (UNet entry; video_model.py:473)
 * Operands: x 4-byte aligned (floats); out 16-byte aligned, Cpad % 8 == 0 (16-byte stores); else VK_EINVAL. */
int vk_nchw_to_tokens_bf16(const float* x, void* out, int32_t n_img, int32_t C, int32_t HW, int32_t Cpad, void* stream);
/* token-major f32 [n_img][HW][ldx] (first C columns) -> NCHW f32 (UNet exit; video_model.py:502-503). Operands: x, out 4-byte aligned (floats). */
int vk_tokens_to_nchw_f32(const float* x, float* out, int32_t n_img, int32_t C, int32_t HW, int32_t ldx, void* stream);

/* sinusoidal timestep embedding: out[n][0:half]=cos(t[n]*f_j), out[n][half:]=sin(t[n]*f_j), f_j=exp(-ln(max_period)*j/half)
 * (vwm/modules/diffusionmodules/util.py:141-165); bf16 output feeds the embedding MLPs.
 * Operands (both forms, and vk_emb_combine below): every pointer aligned to its element (fp32: 4 bytes, 16-bit: 2); else VK_EINVAL. */
int vk_timestep_embedding_bf16(const float* t, void* out, int32_t n, int32_t dim, float max_period, void* stream);
/* The same sinusoid in fp32: ConcatTimestepEmbedderND of the conditioner (vwm/modules/encoders/modules.py:402-425 over openaimodel.py Timestep). */
int vk_timestep_embedding_f32(const float* t, float* out, int32_t n, int32_t dim, float max_period, void* stream);

/* emb = a*mask[n] + b*(1-mask[n]) + c  (video_model.py:457-471); writes emb (f32) and silu(emb) (bf16, the input
 * of every ResBlock emb_layers: openaimodel.py:222-225). a may be NULL (no cond-frame mask: emb = b + c). */
int vk_emb_combine(const float* a, const float* b, const float* c, const float* mask, float* emb, void* silu_out,
                   int32_t n, int32_t dim, void* stream);

/* y = silu(x) f32 -> bf16 (time_pos_embed MLP hidden: video_attention.py:227-231) */
int vk_silu_f32_to_bf16(const float* x, void* y, int64_t count, void* stream);
/* y = bf16(x) */
int vk_cast_f32_to_bf16(const float* x, void* y, int64_t count, void* stream);

/* ---- sampler-side fused elementwise (EulerEDMSampler step; sampling.py:78-89,104-122, guiders.py:23-36,
 *      denoiser.py:30-35, denoiser_scaling.py:51-59, wrappers.py:28-31) ----
 * x, cond_frame: f32 NCHW [T][4][HW]; mask: f32 [T].
 * vk_sampler_prepare: xr = x*(1-mask) + cond_frame*mask (written back to x when replace != 0) and builds the
 *   CFG-doubled UNet input in token-major bf16 [2T][HW][Cpad]: ch 0-3 = xr * c_in, ch 4-7 = concat latent
 *   (uncond half: concat_uc, cond half: concat_c; f32 NCHW [T][4][HW]), remaining channels 0.
 * Operands: the fp32 tensors 4-byte aligned; net_in 16-byte aligned, Cpad % 8 == 0 (16-byte stores); vk_sampler_update: x, net_out, scale 4-byte
 * aligned (floats). Else VK_EINVAL. */
int vk_sampler_prepare(float* x, const float* cond_frame, const float* mask, const float* concat_uc,
                       const float* concat_c, void* net_in, int32_t T, int32_t HW, int32_t Cpad, float c_in,
                       int32_t replace, void* stream);
/* vk_sampler_update: net_out f32 token-major [2T][HW][ld] (first 4 cols). den = net*c_out + x*c_skip for both
 *   halves; g = den_u + scale[t]*(den_c - den_u); d = (x - g)/sigma; x += d*(sigma_next - sigma). */
int vk_sampler_update(float* x, const float* net_out, const float* scale, int32_t T, int32_t HW, int32_t ld,
                      float c_out, float c_skip, float sigma, float sigma_next, void* stream);
/* vk_sampler_update_2m: the same step for DPM-Solver++(2M) (Lu et al. 2022; k-diffusion's sample_dpmpp_2m). x, hist f32 [T][4][HW];
 *   net_out, scale as for vk_sampler_update; g is formed by the same expression. Then x = fmaf(c, hist, fmaf(b, g, a*x)) and hist = g:
 *   hist carries the guided denoised value to the next step. first != 0: x = fmaf(b, g, a*x); hist is written but never read (it may hold
 *   anything). The coefficients a, b, c are made on the host in float64 (sampling.dpmpp2m_coefficients): the kernel sees no log, exp or
 *   division. With (a, b, c) = (0, 1, 0) x becomes g exactly. No atomics; bitwise repeatable.
 * Operands: x, net_out, scale, hist non-NULL and 4-byte aligned (floats); T, HW > 0; ld >= 4; hist != x. Else VK_EINVAL, before any HIP call. */
int vk_sampler_update_2m(float* x, const float* net_out, const float* scale, float* hist, int32_t T, int32_t HW, int32_t ld,
                         float c_out, float c_skip, float a, float b, float c, int32_t first, void* stream);
/* vk_dpmpp2m_step: the update alone, for a denoiser that is any callable: out = fmaf(c, den_old, fmaf(b, den, a*x)) over n f32 elements;
 *   den_old NULL: out = fmaf(b, den, a*x). out may be x. Operands: x, den, out non-NULL, every pointer 4-byte aligned, n > 0. Else VK_EINVAL. */
int vk_dpmpp2m_step(const float* x, const float* den, const float* den_old, float* out, float a, float b, float c, int64_t n,
                    void* stream);

/* generic pieces of the same maths for callers that use the reference's Denoiser / guider API directly */
/* out = net*c_out[n] + x*c_skip[n]  (NCHW f32, per-image coefficients; denoiser.py:35) */
int vk_denoiser_combine(const float* net, const float* x, const float* c_out, const float* c_skip, float* out,
                        int32_t n_img, int32_t chw, void* stream);
/* out[t] = u[t] + scale[t]*(c[t]-u[t]) with u = x[0:T], c = x[T:2T]  (guiders.py:23-26,54-61) */
int vk_cfg_combine(const float* x2, const float* scale, float* out, int32_t T, int32_t chw, void* stream);
/* x_next = x + (x - den)/sigma[n] * (sigma_next[n]-sigma[n])  (sampling_utils.py:46-47; sampling.py:66-67,85-88) */
int vk_euler_step(const float* x, const float* den, const float* sigma, const float* sigma_next, float* out,
                  int32_t n_img, int32_t chw, void* stream);
/* out = x*(1-mask[n]) + cond*mask[n]  (sampling.py:106,122) */
int vk_mask_replace(const float* x, const float* cond, const float* mask, float* out, int32_t n_img, int32_t chw,
                    void* stream);
/* out = x * s[n]  (per-image scale, NCHW f32; denoiser.py:35 `noised_input * c_in`) */
int vk_scale_rows(const float* x, const float* s, float* out, int32_t n_img, int32_t chw, void* stream);

/* Diagonal-Gaussian posterior of the first-stage encoder (vwm/modules/distributions/distributions.py:24-37 and
 * regularizers/__init__.py:30-39), fused with encode_first_stage's `z * scale_factor` (vwm/models/diffusion.py:194):
 * moments f32 NCHW [n][2C][hw] = (mean | logvar); out[n][C][hw] = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale;
 * noise NULL = the posterior mode (mean * scale). */
int vk_gaussian_sample(const float* moments, const float* noise, float* out, int32_t n_img, int32_t C, int32_t hw, float scale,
                       void* stream);

/* Reward estimation (reward_utils.py:329-335): out[0] = sum_i sum_e (x[e][i] - mean_e)^2 / (E - 1) over an ensemble x[E][n] of f32
 * latents, reduced in a fixed order (f64 partials; partial_ws: 512 doubles). The caller forms exp(-out/n). */
int vk_ensemble_variance_sum(const float* x, double* out, double* partial_ws, int32_t E, int64_t n, void* stream);

/* ------------------------------------------------------------------ image I/O of the sampling front door (ABI v8; csrc/image_io.hip)
 * Storage-type independent: the same code is linked into both libraries.
 *
 * vk_lanczos_resize_u8: `load_img` (sample.py:174-201) for n_img frames of one size -- crop box, PIL `resize(LANCZOS)`, ToTensor, x * 2 - 1.
 *   src   (n_img, src_h, src_w, 3) uint8 RGB, interleaved; the crop box [top, top + crop_h) x [left, left + crop_w) is read in place
 *   tmp   (n_img, crop_h, out_w, 3) uint8 scratch of the caller: the horizontal pass's 8-bit intermediate, as in Pillow (4-byte aligned)
 *   out   (n_img, 3, out_h, out_w) fp32 (16-byte aligned): lut256[byte], lut256[k] = float(k) / 255 * 2 - 1 as the caller computed it in IEEE fp32
 *   bounds_x (out_w, 2) int32 = (first tap's column inside the crop box, tap count <= ksize_x); coef_x (out_w, ksize_x) int32 fixed-point weights
 *   (2^22 scale); bounds_y / coef_y / ksize_y the same for the rows. The tables are Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc`
 *   (vista_amd/image_io.py: lanczos_tables); a value is clip8((2^21 + sum pixel * weight) >> 22) per pass, in int32 -- every byte equals Pillow's.
 *   The caller guarantees 0 <= first + count <= crop_w (crop_h); the entry point checks the box against the source and returns VK_EINVAL for an
 *   empty or overhanging one. */
int vk_lanczos_resize_u8(const void* src, void* tmp, float* out, const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x,
                         const int32_t* bounds_y, const int32_t* coef_y, int32_t ksize_y, const float* lut256, int32_t n_img,
                         int32_t src_h, int32_t src_w, int32_t left, int32_t top, int32_t crop_h, int32_t crop_w, int32_t out_h,
                         int32_t out_w, void* stream);
/* vk_frames_to_u8: the float -> uint8 conversion of `perform_save_locally` (sample_utils.py:96-137). x (n_img, 3, H, W) fp32 (16-byte aligned).
 *   real = 0: uint8(255 * x)   real = 1: uint8(255 * (x + 1) / 2)   -- numpy's float32 arithmetic (one rounding per operation), truncating cast.
 *   pad = 0: out (n_img, H, W, 3) uint8.   pad > 0: out is ONE (ymaps * (H + pad) + pad, xmaps * (W + pad) + pad, 3) canvas, ymaps =
 *   ceil(n_img / xmaps), tile k at row k / xmaps * (H + pad) + pad, column k % xmaps * (W + pad) + pad; every other pixel is the map of 0
 *   (torchvision.utils.make_grid with pad_value 0, written straight from the NCHW tensor). out 4-byte aligned. */
int vk_frames_to_u8(const float* x, void* out, int32_t n_img, int32_t H, int32_t W, int32_t xmaps, int32_t pad, int32_t real, void* stream);

/* ------------------------------------------------------------------ reward estimation front door (csrc/reward.hip)
 * Added under ABI v9 without a version step: the two entry points are purely additive (no existing signature, struct or meaning changes), so
 * vk_abi_version() stays 9. Storage-type independent: the same code is linked into both libraries.
 *
 * vk_ensemble_frame_stats: where in the window, and where in the picture, the E ensemble members of a reward run disagree.
 *   x          [E][T][C][hw] fp32 (the sampler's own output type), dense. 2 <= E <= 64.
 *   v[t][c][p] = the unbiased ensemble variance of one element, in the arithmetic of vk_ensemble_variance_sum operation for operation: the fp32
 *                mean summed in member order and divided by E, an fmaf chain of squared differences in member order, divided by E - 1.
 *   frame_sum  [T] fp64: sum of v over the frame's C * hw elements. Every frame is reduced by VK_FRAME_STATS_BLOCKS workgroups whose element
 *              assignment is a function of hw alone, then one thread adds the frame's partials in block order: no atomics, bitwise repeatable,
 *              and a frame's sum does not change with T or with the frames around it.
 *   map        [T][hw] fp32 or NULL: mean over C of v, summed in channel order and divided by C.
 *   partial_ws T * VK_FRAME_STATS_BLOCKS doubles of scratch, the caller's.
 *   Where hw % 4 == 0 the kernel moves 16 bytes per lane: x (and map, when given) must then be 16-byte aligned; any other hw takes any alignment.
 *   VK_EINVAL: E < 2, E > 64, T / C / hw <= 0, T > 65535, a NULL x / frame_sum / partial_ws, a misaligned pointer where hw % 4 == 0. */
#define VK_FRAME_STATS_BLOCKS 16
int vk_ensemble_frame_stats(const float* x, double* frame_sum, float* map, double* partial_ws, int32_t E, int32_t T, int32_t C, int32_t hw,
                            void* stream);
/* vk_candidate_frame_stats: vk_ensemble_frame_stats for the ensembles of K candidate actions in one call, plus what a planner asks of them --
 * every candidate's total and which one is smallest. Additive under ABI v9, as the two entries around it.
 *   x          [K][E][T][C][hw] fp32, dense: the E members of each of K candidates. Frames [t0, T) are scored (T' = T - t0); the frames before
 *              t0 -- a window's conditioning frames -- are never read.
 *   frame_sum  [K][T'] fp64: frame_sum[k][t - t0] is bit for bit what vk_ensemble_frame_stats returns for frame t of candidate k alone (the same
 *              element arithmetic, thread-to-element assignment, block reduction and fold of VK_FRAME_STATS_BLOCKS partials).
 *   map        [K][T'][hw] fp32 or NULL: bitwise that entry's map.
 *   total      [K] fp64: the candidate's frame sums added in frame order t0 .. T - 1 by one thread.
 *   best       one int32: the index of the smallest total; ties go to the lowest index, a NaN total is never best, -1 when every total is NaN.
 *   partial_ws K * T' * VK_FRAME_STATS_BLOCKS doubles of scratch, the caller's.
 *   Two launches (statistics on a (VK_FRAME_STATS_BLOCKS, T', K) grid, then one block that folds and selects), no atomics: bitwise repeatable.
 *   The 16-byte path and its alignment rule are vk_ensemble_frame_stats's (a function of hw alone).
 *   VK_EINVAL: a NULL x / frame_sum / total / best / partial_ws, K < 1, E < 2, E > 64, t0 < 0, t0 >= T, C / hw <= 0, K > 65535, T' > 65535,
 *   a misaligned x or map where hw % 4 == 0. */
int vk_candidate_frame_stats(const float* x, double* frame_sum, double* total, int32_t* best, float* map, double* partial_ws, int32_t K,
                             int32_t E, int32_t T, int32_t t0, int32_t C, int32_t hw, void* stream);
/* vk_heat_overlay_u8: the input frames with a per-cell map blended in as a heat colour, ready to be written as 8-bit pictures.
 *   frames (n_img, 3, H, W) fp32 in [-1, 1] (16-byte aligned); map (n_img, H / cell, W / cell) fp32, >= 0; out (n_img, H, W, 3) uint8 (4-byte aligned).
 *   f   = 255 * (x + 1) / 2, the float vk_frames_to_u8(real = 1) forms before its cast
 *   a   = alpha * min(1, map[t][y / cell][x / cell] * inv_vmax)
 *   out = uint8(f + a * (K - f)),  K = (255, 32, 0) per channel; the cast truncates.
 *   Every operation is rounded once in fp32 and nothing is contracted into an FMA: the bytes equal numpy's float32 evaluation of the expression.
 *   VK_EINVAL: a NULL or misaligned pointer, n_img / H / W / cell <= 0, H % cell or W % cell != 0, alpha outside [0, 1], inv_vmax negative or
 *   not finite. */
int vk_heat_overlay_u8(const float* frames, const float* map, void* out, int32_t n_img, int32_t H, int32_t W, int32_t cell, float inv_vmax,
                       float alpha, void* stream);

/* ------------------------------------------------------------------ evaluation front door (csrc/fidelity.hip)
 * Added under ABI v9 without a version step, as the reward entry points were: purely additive. Storage-type independent: the same code is
 * linked into both libraries.
 *
 * vk_frame_fidelity_u8: how close the 8-bit frames `a` are to the 8-bit frames `b` -- the bytes vk_frames_to_u8 writes, so a number about them is
 * a number about the saved pictures. a, b (n, H, W, 3) uint8, dense. Per frame f and channel c:
 *   sse[f][c]      uint64: sum over the frame of (a - b)^2. An exact integer: any order gives it.
 *   ssim_sum[f][c] fp64: sum of the SSIM index (Wang, Bovik, Sheikh, Simoncelli 2004) over the (H - 10) * (W - 10) positions at which the 11 x 11
 *                  window lies inside the frame (no padding); the caller divides. Per window, in fp32: the weighted moments under the separable
 *                  window w (rows, then columns) of x' = a - 128, y' = b - 128 (exact in fp32; the pivot keeps the variances of bright, flat
 *                  regions out of the cancellation of two numbers near 255^2), mx, my, xx, yy, xy, and
 *                      ((2 ux uy + C1) (2 sxy + C2)) / ((ux^2 + uy^2 + C1) (sxx + syy + C2)),   ux = mx + 128, uy = my + 128,
 *                      sxx = xx - mx^2, syy = yy - my^2, sxy = xy - mx my,   C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
 *                  with the index expression kept free of FMA contraction, so that a frame scored against itself gives exactly 1 per window.
 *   window11       VK_FIDELITY_TAPS fp32 weights in HOST memory, read during the call (they reach the kernel by value): the caller's Gaussian
 *                  (sigma 1.5, normalised in float64, rounded once).
 *   ws             n * vk_frame_fidelity_ws_bytes(H, W) bytes of scratch, the caller's, 8-byte aligned: one fp64 and one uint64 partial per
 *                  workgroup and channel. A workgroup owns a VK_FIDELITY_TILE_H x VK_FIDELITY_TILE_W tile of window positions of one frame (and
 *                  the squared differences of its pixels; the last tile of an axis those up to the frame's edge); a fold pass adds a frame's
 *                  partials in a fixed order. Which workgroup owns what is a function of (H, W) alone: no atomics, bitwise repeatable, and a
 *                  frame's values do not change with n or with the frames around it.
 *   Where W % 4 == 0 the halo is loaded 4 bytes per lane: a and b must then be 4-byte aligned; any other W takes any alignment.
 *   The entry point allocates nothing and synchronises nothing.
 *   VK_EINVAL: a NULL pointer, n <= 0, n > 65535, H < 11 or W < 11, ws / sse / ssim_sum not 8-byte aligned, a or b misaligned where W % 4 == 0,
 *   a frame of more tiles than vk_frame_fidelity_ws_bytes can state.
 * vk_frame_fidelity_ws_bytes: the workspace bytes PER FRAME for (H, W) frames, or VK_EINVAL (H < 11, W < 11, more than 2^31 - 1 bytes). */
#define VK_FIDELITY_TAPS 11
#define VK_FIDELITY_TILE_H 16
#define VK_FIDELITY_TILE_W 32
int vk_frame_fidelity_ws_bytes(int32_t H, int32_t W);
int vk_frame_fidelity_u8(const void* a, const void* b, uint64_t* sse, double* ssim_sum, void* ws, const float* window11 /* HOST memory */,
                         int32_t n, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------ CLIP-space scores (csrc/perceptual.hip)
 * Added under ABI v9 without a version step: purely additive, so vk_abi_version() stays 9. No float atomics: two calls on the same input return
 * the same bits. The entry points allocate nothing and synchronise nothing. Only the 16-bit store of the first one sees the storage type.
 *
 * vk_clip_preprocess_patches_u8: vk_clip_preprocess_patches (declared with the conditioner's entries) for `img` (n_img, H, W, 3) uint8, dense: the bytes
 * vk_frames_to_u8 writes and the saved pictures hold. A byte b stands for (float)b / 127.5f - 1.0f (one fp32 division, one fp32 subtraction,
 * not contracted); from there the arithmetic is the fp32 entry's, operation for operation (csrc/clip_resample.h), so `out` equals, bit for bit,
 * what vk_clip_preprocess_patches of the same library writes for the frames converted that way. Every other argument as there; the caller
 * zero-fills `out`. A workgroup stages the source rectangle of a tile of outputs into LDS as fp32; the tile is the largest of 16, 8, 4, 2, 1
 * outputs a side whose rectangle fits 60 KiB. Where W % 4 == 0 and img is 4-byte aligned the rectangle is loaded 4 bytes per lane, else a
 * byte per lane: any W and any base address are taken.
 *   VK_EINVAL: what vk_clip_preprocess_patches refuses; n_img > 65535; out_hw > 4096; H or W > VK_CLIP_U8_MAX_SIDE; a blur radius ks / 2 that
 *   is not smaller than the side it runs along; `out` not 2-byte aligned.
 *
 * vk_embed_row_stats: a, b (n, d) fp32, dense -> out (n, 3) fp64: per row a.b, a.a, b.b. fp32 values multiplied (exactly) and summed in
 * fp64; the order of the three sums is one function of d, so a == b gives three equal bit patterns and a cosine of exactly 1.
 *   VK_EINVAL: a NULL pointer, n or d <= 0, n > VK_EMBED_MAX_ROWS, d > VK_EMBED_MAX_DIM, a / b not 4-byte or out not 8-byte aligned.
 *
 * vk_embed_mmd_sums: x (m, d), y (n, d) fp32, dense -> out3, 3 fp64: with u^ = u times the fp32 inverse of its norm (the norm from the fp64
 * sum of squares) and k(u, v) = exp(-|u - v|^2 / (2 sigma^2)),
 *   out3[0] = sum over i < j of 1 - k(x^_i, x^_j),   out3[1] = likewise over y,   out3[2] = sum over all (i, j) of 1 - k(x^_i, y^_j).
 * Per pair |u - v|^2 is the fp32 sum over the columns, in ascending order, of the squared fp32 differences (an FMA of the difference with
 * itself into the sum; never 2 - 2 u.v), and 1 - k is -expm1f(-gamma * that), gamma = (float)(1 / (2 sigma^2)); the terms are added in fp64:
 * per workgroup (a VK_EMBED_MMD_TILE^2 block of pairs) in a fixed order into the workspace, then folded in a fixed order. Two equal rows
 * contribute exactly 0. m == 1 gives out3[0] == 0. A row whose norm is zero or not finite makes every sum it is in NaN; nothing faults.
 *   ws: vk_embed_mmd_ws_bytes(m, n, d) bytes of scratch, the caller's, 8-byte aligned.
 *   VK_EINVAL: a NULL pointer, m / n / d < 1, m or n > VK_EMBED_MAX_ROWS, d > VK_EMBED_MAX_DIM, sigma not positive and finite, x / y not
 *   4-byte or out3 / ws not 8-byte aligned.
 * vk_embed_mmd_ws_bytes: the workspace bytes, 24 per tile of pairs of the larger set with itself plus 4 per row, or VK_EINVAL: a shape
 * vk_embed_mmd_sums refuses, or more than 2^31 - 1 bytes (sets beyond about 600,000 rows), which vk_embed_mmd_sums then refuses too. */
#define VK_CLIP_U8_MAX_SIDE 65536
#define VK_EMBED_MAX_ROWS (1 << 20)
#define VK_EMBED_MAX_DIM (1 << 16)
#define VK_EMBED_MMD_TILE 64
int vk_clip_preprocess_patches_u8(const void* img, void* out, int32_t n_img, int32_t H, int32_t W, int32_t out_hw, int32_t patch, int32_t ldo,
                                  float sigma_y, float sigma_x, int32_t ks_y, int32_t ks_x, const float* mean3 /* HOST memory */,
                                  const float* std3 /* HOST memory */, void* stream);
int vk_embed_row_stats(const float* a, const float* b, double* out, int32_t n, int32_t d, void* stream);
int vk_embed_mmd_ws_bytes(int32_t m, int32_t n, int32_t d);
int vk_embed_mmd_sums(const float* x, const float* y, double* out3, void* ws, int32_t m, int32_t n, int32_t d, float sigma, void* stream);

/* ------------------------------------------------------------------ motion scores (csrc/flow.hip)
 * Added under ABI v9 without a version step: purely additive, so vk_abi_version() stays 9. Integers only, from the bytes to the sums: two calls
 * on the same input return the same bits, and so does a plain restatement on the host. Storage-type independent: the same code is linked into
 * both libraries. The entry points allocate nothing and synchronise nothing.
 *
 * The flow is hierarchical block matching on 8-bit luma, defined exactly:
 *   luma      Y = (77 R + 150 G + 29 B + 128) >> 8.
 *   pyramid   VK_FLOW_LEVELS levels; level l + 1 is the 2 x 2 mean of level l, (a + b + c + d + 2) >> 2.
 *   blocks    VK_FLOW_BLOCK x VK_FLOW_BLOCK pixels at every level; block (by, bx) of level l has the parent (by >> 1, bx >> 1) at level l + 1.
 *   cost      of a vector (vy, vx) for a block of frame i at one level: the sum of absolute differences (SAD) of the block's 64 luma values
 *             against frame i + 1's values at (y + vy, x + vx), both coordinates clamped to the image.
 *   search    level 2: every (dy, dx) in [-7, 7]^2 around zero. Levels 1 and 0: twice the parent's vector plus an increment in [-2, 2]^2.
 *   choice    the smallest (SAD, |dy| + |dx| of the increment, dy, dx), compared lexicographically.
 * A translation of up to 30 px per frame step is within reach (4 * 7 + 2); beyond it the coarse search saturates.
 *
 * vk_flow_luma_pyramid_u8: frames (n, H, W, 3) uint8, dense -> pyr: level 0 of all frames (n, H, W), then level 1 (n, H/2, W/2), then level 2
 * (n, H/4, W/4), vk_flow_pyramid_bytes(n, H, W) = n * H * W * 21 / 16 bytes in all, the caller's.
 * vk_block_flow_u8: pyr of n >= 2 frames -> for every pair (i, i + 1), i < n - 1, and level-0 block:
 *   flow (n - 1, H/8, W/8, 2) int16: (vy, vx) in pixels: content at (y, x) of frame i is found at (y + vy, x + vx) of frame i + 1; |v| <= 34
 *   sad  (n - 1, H/8, W/8, 2) uint16: the block's SAD at that vector, and its SAD at zero displacement (both at most 16320)
 * vk_flow_pair_sums: flow, sad (pairs, blocks, 2) as above, flow_ref likewise or NULL -> out (pairs, 5) int64: per pair the number of blocks
 * with a non-zero vector, sum(vy^2 + vx^2), sum SAD, sum SAD at zero, and sum((vy - vy_ref)^2 + (vx - vx_ref)^2) (0 where flow_ref is NULL).
 *   VK_EINVAL, before any launch: a NULL pointer (but flow_ref); frames / pyr / flow / sad / flow_ref not 4-byte or out not 8-byte aligned; H or
 *   W not a positive multiple of 32 or above VK_FLOW_MAX_SIDE (checked before any product is formed: no extent can wrap); n < 1
 *   (vk_block_flow_u8: n < 2), n > VK_FLOW_MAX_FRAMES; a pyramid of more than 2^31 - 1 bytes; pairs or
 *   blocks < 1, pairs * blocks > 2^31 - 1. */
#define VK_FLOW_BLOCK 8
#define VK_FLOW_LEVELS 3
#define VK_FLOW_COARSE_RANGE 7
#define VK_FLOW_REFINE_RANGE 2
#define VK_FLOW_MAX_FRAMES 65535
#define VK_FLOW_MAX_SIDE 65536
int vk_flow_pyramid_bytes(int32_t n, int32_t H, int32_t W);
int vk_flow_luma_pyramid_u8(const void* frames, void* pyr, int32_t n, int32_t H, int32_t W, void* stream);
int vk_block_flow_u8(const void* pyr, int16_t* flow, uint16_t* sad, int32_t n, int32_t H, int32_t W, void* stream);
int vk_flow_pair_sums(const int16_t* flow, const uint16_t* sad, const int16_t* flow_ref /* or NULL */, int64_t* out, int32_t pairs,
                      int32_t blocks, void* stream);

/* ------------------------------------------------------------------ exchange packing of the frame-sharded step (ABI v9; csrc/reshard.hip)
 * Storage-type independent: the same code is linked into both libraries.
 *
 * vk_copy_row_boxes: every row gather / scatter around an all-to-all of vista_amd/parallel.py (frames <-> pixels re-shards and their chunked
 * form, the halo frames of the temporal convolutions, a rank's rows of a replicated tensor) as ONE launch. `src` is (src_rows, row_bytes) and
 * `dst` (dst_rows, row_bytes), both dense and 16-byte aligned; row_bytes > 0 and a multiple of 16. A plan is 1 .. VK_RESHARD_MAX_BOXES boxes;
 * box rows (b, t, s), 0 <= b < nb, 0 <= t < nt, 0 <= s < ns, are copied
 *     src row  src_row + b * src_stride_b + t * src_stride_t + s   ->   dst row  dst_row + b * dst_stride_b + t * dst_stride_t + s
 * (strides in rows, any sign), so the ns rows of one (b, t) are contiguous on both sides. `reserved` fields are ignored.
 *   Plan passing: `boxes` is HOST memory, read during the call; the plan reaches the kernel by value in its argument. The entry point
 *   allocates nothing, copies nothing and synchronises nothing: the caller may free or overwrite the plan as soon as the call returns, and the
 *   launch may be captured into a graph and replayed.
 *   Validation (VK_EINVAL before any launch, dst untouched): a null or misaligned pointer, row_bytes <= 0 or not a multiple of 16, n outside
 *   [1, VK_RESHARD_MAX_BOXES], a negative extent or row count, a non-empty box that leaves [0, src_rows) on the source or [0, dst_rows) on
 *   the destination (checked on the host in int64).
 *   A box with a zero extent is legal and skipped; a plan of empty boxes only returns VK_OK without a launch.
 *   Overlap: the caller guarantees that the destination rows of the boxes of one plan are pairwise distinct and that dst does not alias the
 *   source rows read; source boxes may overlap (a stride of 0 repeats rows). Overlapping destinations are a data race: undefined contents. */
#define VK_RESHARD_MAX_BOXES 32            /* T <= 32 frames bounds the ranks of a frame-shard group */
typedef struct VkRowBox {
    int64_t src_row, dst_row, src_stride_b, src_stride_t, dst_stride_b, dst_stride_t;
    int32_t nb, nt, ns, reserved;
} VkRowBox;
typedef struct VkRowBoxes {
    int32_t n, reserved;
    VkRowBox box[VK_RESHARD_MAX_BOXES];
} VkRowBoxes;
int vk_copy_row_boxes(const void* src, void* dst, const VkRowBoxes* boxes /* HOST memory */, int64_t src_rows, int64_t dst_rows,
                      int32_t row_bytes, void* stream);

/* ------------------------------------------------------------------ drive front door (csrc/overlay.hip)
 * Added under ABI v9 without a version step, as the reward and evaluation entry points were: purely additive. Storage-type independent: the
 * same code is linked into both libraries.
 *
 * vk_stroke_overlay_u8: anti-aliased strokes (round-capped line segments and discs) drawn over 8-bit frames -- the head-up display of a steered
 * rollout. in, out (n, H, W, 3) uint8, dense; out may be in (every byte is read and written by the same thread).
 *   A plan is up to VK_OVERLAY_MAX_SETS stroke sets over up to VK_OVERLAY_MAX_STROKES strokes over up to VK_OVERLAY_MAX_SEGMENTS segments. A set
 *   is the run [stroke_begin, stroke_begin + stroke_count) of strokes, a stroke a colour K (per channel, in [0, 255]), an alpha in [0, 1], a
 *   half-width r >= 0 and the run [seg_begin, seg_begin + seg_count) of segments; a segment is a = (ax, ay), b = (bx, by) in pixel coordinates
 *   (x to the right, y down, the first pixel's centre at (0.5, 0.5)) and inv_len2 = 1 / |b - a|^2, formed by the caller in fp32. A disc is a
 *   segment with a == b and inv_len2 = 0. Runs may overlap and may be empty.
 *   set_of_frame [n] int32 in DEVICE memory: frame i is drawn with set set_of_frame[i]; a value outside [0, n_sets) (-1 by convention) copies
 *   the frame. One launch draws a whole video whose rounds carry different commands.
 *   Per pixel centre p = (x + 0.5, y + 0.5), in fp32, every operation rounded once and nothing contracted into an FMA:
 *     d    = b - a
 *     t    = clamp(((p.x - a.x) * d.x + (p.y - a.y) * d.y) * inv_len2, 0, 1)          (no division on the device)
 *     q    = a + t * d,   e = p - q,   dist = sqrt(e.x * e.x + e.y * e.y)             (correctly rounded square root)
 *     cov  = clamp((r + 0.5) - dist, 0, 1)
 *   A stroke's coverage is the MAXIMUM of cov over its segments: exact and order-free, so the joints of a polyline are not blended twice.
 *   The strokes of a set composite in list order, per channel:  f <- f + (alpha * cov) * (K - f), starting from f = float(byte); the final
 *   cast truncates. The bytes equal a numpy float32 evaluation of this text (tests/_overlay_ref.py).
 *   A pixel with cov = 0 keeps f exactly, so what lies outside a stroke's bounding box (its segments' extent grown by r + 0.5 and a margin of
 *   two pixels for the rounding of q and dist) is skipped: a workgroup owns a VK_OVERLAY_TILE_H x VK_OVERLAY_TILE_W tile of one frame and tests
 *   the boxes of its frame's set and strokes with wave-uniform (scalar) comparisons; a tile no box touches is a plain copy, or nothing at all
 *   where out == in.
 *   Plan passing: `plan` is HOST memory, read during the call; it reaches the kernel by value in its argument, where every field is fetched by
 *   scalar loads. The maxima keep that argument under 3 KiB of the 4 KiB a kernel argument may take (8 sets x 24 + 32 strokes x 44 + 64
 *   segments x 20 bytes in the kernel's own layout); a caller with more splits the frames over several calls. The entry point allocates
 *   nothing and synchronises nothing.
 *   Rows are 3 W bytes: where W % 4 == 0 a lane moves its four pixels as three dwords (in and out must then be 4-byte aligned), any other W is
 *   moved byte by byte and takes any alignment. The path is a function of W alone.
 *   VK_EINVAL (before any launch): a NULL in / out / set_of_frame / plan, set_of_frame not 4-byte aligned, in or out misaligned where
 *   W % 4 == 0, n / H / W <= 0, n > 65535, a count below 0 or above its maximum, a run that leaves its table, an alpha outside [0, 1], a
 *   colour outside [0, 255], a negative or non-finite r or inv_len2, a coordinate or r that is not finite or beyond 2^20 in magnitude. */
#define VK_OVERLAY_MAX_SETS 8
#define VK_OVERLAY_MAX_STROKES 32
#define VK_OVERLAY_MAX_SEGMENTS 64
#define VK_OVERLAY_TILE_H 16
#define VK_OVERLAY_TILE_W 64
typedef struct VkStrokeSegment {
    float ax, ay, bx, by, inv_len2;
} VkStrokeSegment;
typedef struct VkStroke {
    float color[3];
    float alpha, r;
    int32_t seg_begin, seg_count;
} VkStroke;
typedef struct VkStrokeSet {
    int32_t stroke_begin, stroke_count;
} VkStrokeSet;
typedef struct VkStrokePlan {
    int32_t n_sets, n_strokes, n_segments, reserved;
    VkStrokeSet set[VK_OVERLAY_MAX_SETS];
    VkStroke stroke[VK_OVERLAY_MAX_STROKES];
    VkStrokeSegment seg[VK_OVERLAY_MAX_SEGMENTS];
} VkStrokePlan;
int vk_stroke_overlay_u8(const void* in, void* out, const int32_t* set_of_frame, const VkStrokePlan* plan /* HOST memory */, int32_t n,
                         int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------ denoising-loss front door (csrc/loss.hip)
 * Added under ABI v9 without a version step, as the reward, evaluation and planning entry points were: purely additive (no existing signature,
 * struct or meaning changes), so vk_abi_version() stays 9. fp32 in and out, storage-type independent: the same code is linked into both libraries.
 * Forward only: these are the pieces of the reference's StandardDiffusionLoss (vwm/modules/diffusionmodules/loss.py); no gradient is built.
 *
 * vk_loss_noise_input: out = x + (noise + level * offset[n][c]) * ((1 - mask[n]) * sigma[n]) in one pass.
 *   x, noise, out [n][C][hw] fp32, dense; sigma [n] fp32; mask [n] fp32 or NULL (then the factor is sigma[n]); offset [n][C] fp32 or NULL (then
 *   the noise is taken as it is and `level` is not read).
 *   Evaluated operation by operation as the reference does -- multiply (level * offset), add, subtract and multiply ((1 - mask) * sigma),
 *   multiply, add -- each rounded once in fp32, nothing contracted into an FMA: the result is bit for bit torch's fp32 expression on the CPU.
 *   16 bytes per lane where hw % 4 == 0 and x, noise and out are 16-byte aligned, one element per lane otherwise (the bits are the same).
 *   VK_EINVAL: a NULL x / noise / sigma / out, n / C / hw <= 0, n * C > 2^31 - 1, a pointer not 4-byte aligned. */
int vk_loss_noise_input(const float* x, const float* noise, const float* sigma, const float* mask, const float* offset, float level, float* out,
                        int32_t n, int32_t C, int32_t hw, void* stream);
/* vk_fourier_highpass: the reference's fourier_filter (vwm/modules/diffusionmodules/util.py) of `planes` H x W fp32 planes: the 2-D DFT, every
 * frequency multiplied by 1 where its byte of `keep` is set and by `scale` where it is not, the inverse DFT, the real part.
 *   keep  [H][W] bytes on the GPU, indexed by the UNSHIFTED frequency (kh, kw) (the caller evaluates the reference's disc in double precision and
 *         undoes its fftshift: ties on the disc's edge, and the unsymmetric mask of an odd H or W, are then the reference's own).
 *   input d = a (b == NULL), a - b (cond_mask == NULL), or (a * (1 - m) + b * m) - b with m = cond_mask[plane / planes_per_image]: formed on load,
 *         fp32, one rounding per operation, nothing contracted. The filter is linear, so HF(predict) - HF(target) is HF of this difference.
 *   y     [planes][H][W] fp32; must not alias a or b.
 *   One workgroup per plane, the plane resident in LDS: two complex fp32 buffers of H * W and the fp64 twiddles (cos, sin)(2 pi j / W), j < W, and
 *   (2 pi j / H), j < H, computed in the kernel. Four dense passes (rows, columns, inverse columns, inverse rows); every output is a sum accumulated
 *   in fp64 in index order and rounded to fp32 once. No atomics: bitwise repeatable, and a plane's result does not depend on `planes`.
 *   The plane it can hold: 16 * H * W + 16 * (H + W) <= VK_HIGHPASS_LDS_BYTES (160 KiB, the CU's LDS); 72 x 128, the BASELINE latent, takes 150656.
 *   Any H, W >= 1 within that rule, odd ones included. vk_fourier_highpass_lds_bytes answers the bytes a plane takes, or VK_EINVAL.
 *   VK_EINVAL, before any HIP call: a NULL a / keep / y, cond_mask without b, y == a or y == b, planes / planes_per_image / H / W <= 0, a float pointer
 *   not 4-byte aligned, a plane beyond the rule above. */
#define VK_HIGHPASS_LDS_BYTES (160 * 1024)
int vk_fourier_highpass_lds_bytes(int32_t H, int32_t W);
int vk_fourier_highpass(const float* a, const float* b, const float* cond_mask, const void* keep, float scale, float* y, int32_t planes,
                        int32_t planes_per_image, int32_t H, int32_t W, void* stream);
/* vk_loss_stats: the sums the loss of B clips of T frames is assembled from. out (the denoiser's output), target [B * T][C][hw] fp32, dense;
 * cond_mask [B * T] fp32 or NULL; hf [B * T][C][hw] fp32 (vk_fourier_highpass's output) or NULL; l1 = 0 (squares) or 1 (absolute values).
 *   predict = out * (1 - m) + target * m per frame (out where cond_mask is NULL), fp32, one rounding per operation, nothing contracted.
 *   dd      = (target_t - target_{t-1}) - (predict_t - predict_{t-1}),  a = dd^2 (l2) or |dd| (l1), for t >= 1.
 *   Launch 1, per (clip b, channel c): the sum over (t >= 1, h, w) of a^2 (l2) or of a (l1), in fp64, by VK_LOSS_STATS_BLOCKS workgroups whose
 *   element assignment is a function of T and hw alone -> partial_ws [B][C][VK_LOSS_STATS_BLOCKS] doubles, the caller's.
 *   Launch 2, one workgroup per frame: the clip's partials added in block order; norm = sqrt of that sum (l2) or the sum (l1), rounded to fp32
 *   once; aux_w = 1 at t == 0, else 1 + a / max(norm, 1e-12) in fp32 (F.normalize's clamp: a norm of 0 gives aux_w = 1). Then, in fp64,
 *     sums[f] = (S0, S1, S2) = (sum e, sum e * aux_w, sum |hf|^p),  e = (predict - target)^2 or |predict - target|, p = 2 or 1; S2 = 0 without hf.
 *   Thread i adds the frame's groups i, i + 256, ... (a group = 4 neighbouring elements where hw % 4 == 0, else 1) and the block adds the threads
 *   in a fixed tree: no atomics, bitwise repeatable, and a frame's sums do not depend on B or on the frames of other clips. T == 1 (no frame
 *   differences; also how a caller asks for S0 alone): S1 == S0, launch 1 is skipped, partial_ws may be NULL and B is not limited to 65535.
 *   A frame with m == 1 gives (0, 0, S2) exactly, and S2 == 0 exactly when hf came from vk_fourier_highpass with the same cond_mask.
 *   The loss weight w(sigma) is not applied here: the caller weighs the sums in float64.
 *   16-byte loads where hw % 4 == 0 and out, target and hf are 16-byte aligned; the order of every sum is a function of hw alone either way.
 *   VK_EINVAL: a NULL out / target / sums, B / T / C / hw <= 0, C > VK_LOSS_MAX_CHANNELS, with T > 1 a NULL partial_ws or B > 65535, B * T or C * hw > 2^31 - 1, l1
 *   not 0 or 1, a float pointer not 4-byte aligned, sums or partial_ws not 8-byte aligned. */
#define VK_LOSS_STATS_BLOCKS 16
#define VK_LOSS_MAX_CHANNELS 64
int vk_loss_stats(const float* out, const float* target, const float* cond_mask, const float* hf, double* sums, double* partial_ws, int32_t B,
                  int32_t T, int32_t C, int32_t hw, int32_t l1, void* stream);

/* ------------------------------------------------------------------ Motion-JPEG video output (csrc/jpeg.hip)
 * Added under ABI v9 without a version step, as the reward, evaluation, planning and loss entry points were: purely additive. uint8 in, int16 and
 * bytes out, storage-type independent: the same code is linked into both libraries.
 * A baseline sequential JPEG (ITU-T T.81): 8 bit, three components, 4:2:0 (MCU = 16 x 16 pixels = blocks Y00 Y01 Y10 Y11 Cb Cr), the Annex K
 * "typical" Huffman tables, one restart interval per MCU row. mcu_h = ceil(H / 16), mcu_w = ceil(W / 16). The headers are the host's.
 *
 * vk_jpeg_dct_quant_u8: frames (n, H, W, 3) uint8 -> coef (n, 6 * mcu_h * mcu_w, 64) int16: per block the quantised coefficients in zigzag order,
 * blocks in scan order (MCUs row-major). In fp32: Y = 0.299 R + 0.587 G + 0.114 B, Cb = -0.168736 R - 0.331264 G + 0.5 B + 128,
 * Cr = 0.5 R - 0.418688 G - 0.081312 B + 128, nothing rounded to 8 bit; frames padded to whole MCUs by edge replication; a chroma sample is the
 * mean of its 2 x 2 unrounded samples; level shift by -128; the orthonormal 8 x 8 DCT-II of A.3.3 (rows, then columns); division by the
 * quantiser, rounded half away from zero; DC clamped to [-1024, 1023], AC to [-1023, 1023].
 *   quant  HOST memory, read during the call, handed to the kernel by value: `quality` (1 .. 100, the libjpeg rule the tables were scaled by; the
 *          kernel does not read it) and the two tables in ZIGZAG order, every entry 1 .. 255.
 *   Operands: frames dense, any alignment -- the copy into LDS moves 16 bytes per lane where 3 W % 16 == 0 and frames is 16-byte aligned, 4 where
 *   3 W % 4 == 0 and it is 4-byte aligned, else bytes; the coefficients are the same on every path. coef dense, 16-byte aligned (16-byte stores).
 *   1 <= H, W <= 65535, n >= 1, 6 n mcu_h mcu_w (the block count) and 3 n H W (the frames' bytes) at most 2^31 - 1.
 *   VK_EINVAL, before any HIP call: a NULL pointer, an extent outside those limits, coef misaligned, quality outside 1 .. 100, a table entry
 *   outside 1 .. 255.
 *
 * vk_jpeg_interval_sizes: sizes[n * mcu_h] int32 = the bytes of every restart interval's entropy-coded data: byte stuffing (0xFF -> 0xFF 0x00)
 * included, the last partial byte padded with 1-bits, plus 2 for the RSTm marker that follows every interval but a frame's last.
 * vk_jpeg_entropy_write: writes interval i at out + offsets[i] (int64, DEVICE memory; the caller's exclusive sum of the sizes, so that one frame's
 * scan is one contiguous slice), followed by RSTm (0xFF, 0xD0 + MCU row % 8) where it has one. Every byte of [offsets[i], offsets[i] + sizes[i])
 * is stored exactly once by a plain store and no other byte is touched: out need not be zeroed. A byte that would fall outside [0, out_bytes) is
 * not stored. Both run the same code, one workgroup per interval; integer operations only, bitwise repeatable.
 *   The DC difference of a block is taken against the previous block of its component in scan order, the predictor is 0 at each interval's
 *   start. A coefficient outside the ranges above is replaced by the nearest value inside them before anything else (as a DC value, as a
 *   predictor and as an AC value alike): the stream is that of the clamped array.
 *   blocks  the block count of coef, stated by the caller: it must equal 6 n mcu_h mcu_w.
 *   Operands: coef dense, 16-byte aligned (16-byte loads); sizes 4-byte, offsets 8-byte aligned; out any alignment.
 *   n >= 1, 1 <= mcu_h, mcu_w <= 4096, blocks <= 2^31 - 1, 1 <= out_bytes <= 2^31 - 1.
 *   VK_EINVAL, before any HIP call: a NULL pointer, an extent outside those limits, blocks != 6 n mcu_h mcu_w, a misaligned coef / sizes / offsets. */
typedef struct VkJpegQuant {
    int32_t quality, reserved;
    uint16_t luma[64];
    uint16_t chroma[64];
} VkJpegQuant;
int vk_jpeg_dct_quant_u8(const void* frames, void* coef, const VkJpegQuant* quant /* HOST memory */, int32_t n, int32_t H, int32_t W, void* stream);
int vk_jpeg_interval_sizes(const void* coef, int32_t* sizes, int32_t n, int32_t mcu_h, int32_t mcu_w, int32_t blocks, void* stream);
int vk_jpeg_entropy_write(const void* coef, const int64_t* offsets, void* out, int64_t out_bytes, int32_t n, int32_t mcu_h, int32_t mcu_w,
                          int32_t blocks, void* stream);

/* ------------------------------------------------------------------ PNG output (csrc/png.hip)
 * Added under ABI v9 without a version step, as the Motion-JPEG entry points were: purely additive. uint8 in, bytes out, integer arithmetic only,
 * storage-type independent: the same code is linked into both libraries. The PNG signature and chunks, the two-byte zlib header, the combination
 * of the segments' Adler-32 pairs into a frame's checksum and the chunk CRCs are the host's (vista_amd/png.py).
 *
 * vk_png_filter_u8: frames (n, H, W, 3) uint8 -> rows (n, H, 1 + 3 W) uint8: per row the filter type and the filtered bytes. All five types are
 * coded (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; bpp = 3; the row above a frame's first row is zero: each frame is independent) and the type
 * with the smallest sum of the bytes' absolute values, read as signed, is kept (libpng's heuristic); on a tie the lowest type.
 *   Operands: frames and rows dense, any alignment (byte accesses). n >= 1, 1 <= H, W <= VK_PNG_MAX_EXTENT, n H (1 + 3 W) at most 2^31 - 1.
 *   VK_EINVAL, before any HIP call: a NULL pointer, an extent outside those limits.
 *
 * vk_png_deflate_plan / vk_png_deflate_write: rows (n, H, row_bytes) uint8 -- any row_bytes, not only 1 + 3 W -- are cut into segments of seg_rows
 * rows (a frame's last may be shorter); segment i of the call is segment i % segs of frame i / segs, segs = ceil(H / seg_rows). A segment is coded
 * as exactly ONE dynamic-Huffman deflate block (BTYPE 10), BFINAL set only on a frame's last segment; every other segment is followed by an
 * empty stored block (BFINAL 0, BTYPE 00, zero bits to the byte, 00 00 FF FF), so every segment starts on a byte boundary and a frame's
 * segments, back to back, are one raw deflate stream.
 *   Tokens (zlib's Z_RLE, restated): at position i >= 1 of the segment, if bytes i, i + 1 and i + 2 equal byte i - 1, a match of distance 1 and
 *   length min(rest of the run inside the segment, 258); otherwise a literal. Nothing refers behind the segment's start; runs cross rows.
 *   Codes: a pure function of the segment's histogram. Fewer than two used symbols: symbols 0, then 1, are counted once until two are. The used
 *   symbols sorted by (count, symbol) ascending are the leaves of a two-queue Huffman construction (leaves in that order, internal nodes in order
 *   of creation; the lighter front is taken, the leaf on a tie); a length is a leaf's depth. While the longest length exceeds the limit (15 for
 *   literal/length, 7 for the code-length alphabet) every used count becomes (count + 1) >> 1 and the construction is repeated. The distance
 *   alphabet is distance 1 alone: one code of length 1 where the segment holds a match, a single zero length where it holds none. Canonical codes
 *   (RFC 1951 3.2.2). Tree description: the literal/length lengths up to the last used symbol (at least 257), then the one distance length
 *   (HDIST 0); a run of r zeros is 18 (11 .. 138) while r >= 11, then 17 if r >= 3, else r times 0; a run of r equal lengths v > 0 is v, then 16
 *   (3 .. 6) while at least 3 remain, then v for each left; runs end with the literal/length lengths.
 * vk_png_deflate_plan writes, per segment: sizes[i] int32, its bytes (stored block included); adler[2 i], adler[2 i + 1], the Adler-32 sums
 * (s1, s2) of the segment's bytes alone, started from 1; plan[i * VK_PNG_PLAN_WORDS ...] uint32: word 0 the bits of the block header and tree
 * description, word 1 the distance code's length, words 4 .. 289 per literal/length symbol (bit-reversed code | length << 16), words 290 .. 419
 * the header's bits, LSB first. The trees are built on the GPU: between the two calls only the sizes travel.
 * vk_png_deflate_write writes segment i at out + offsets[i] (int64, DEVICE memory; the caller's exclusive sum of the sizes). Every byte of
 * [offsets[i], offsets[i] + sizes[i]) is stored exactly once by a plain store and no other byte is touched: out need not be zeroed. A byte that
 * would fall outside [0, out_bytes) is not stored. A workgroup per segment streams through it 256 bytes at a time: a segment need not fit LDS.
 *   segments  the segment count, stated by the caller: it must equal n * ceil(H / seg_rows).
 *   Operands: rows dense, any alignment; sizes, adler and plan 4-byte, offsets 8-byte aligned; out any alignment.
 *   n, H, row_bytes, seg_rows >= 1; n H row_bytes at most 2^31 - 1; a segment, min(seg_rows, H) * row_bytes, at most VK_PNG_MAX_SEGMENT_BYTES
 *   (2^24: the grid of 91 frames of 576 x 1024, 6360 rows of 27709 bytes, has segments of 443344); 1 <= out_bytes <= 2^31 - 1.
 *   VK_EINVAL, before any HIP call: a NULL pointer, an extent outside those limits, segments != n * ceil(H / seg_rows), a misaligned sizes /
 *   adler / plan / offsets. */
#define VK_PNG_MAX_EXTENT 65535
#define VK_PNG_MAX_SEGMENT_BYTES (1 << 24)
#define VK_PNG_PLAN_WORDS 420
int vk_png_filter_u8(const void* frames, void* rows, int32_t n, int32_t H, int32_t W, void* stream);
int vk_png_deflate_plan(const void* rows, int32_t* sizes, uint32_t* adler, uint32_t* plan, int32_t n, int32_t H, int32_t row_bytes, int32_t seg_rows,
                        int32_t segments, void* stream);
int vk_png_deflate_write(const void* rows, const uint32_t* plan, const int64_t* offsets, void* out, int64_t out_bytes, int32_t n, int32_t H,
                         int32_t row_bytes, int32_t seg_rows, int32_t segments, void* stream);

/* library info */
int vk_abi_version(void);
/* ABI v7: the 16-bit storage type this library was built for: 0 = bf16 (libvista_hip.so, the default and the BASELINE config's dtype), 1 = IEEE fp16
 * (libvista_hip_f16.so, -DVK_F16=1: the reference's autocast width, sample_utils.py:301-303). Every "bf16" in the entry-point names and comments of
 * this header reads "the storage type" for the fp16 build; fp32 interfaces are unchanged. The fp8 entry points (BASELINE config 5) exist in the bf16
 * build only and return VK_EINVAL in the other. */
int vk_act_dtype(void);

#ifdef __cplusplus
}
#endif
#endif
