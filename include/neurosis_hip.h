/*
 * neurosis_hip.h -- C-ABI of libneurosis_hip.so: the MI355X (gfx950) kernels behind the SDXL
 * training-step hot path of neggles/neurosis.
 *
 * Conventions
 *   - every entry point returns 0 on success, non-zero on error; nk_last_error() gives the message.
 *     Nothing falls back to a CPU path: a bad argument or a failed launch is an error.
 *   - all pointers are DEVICE pointers unless the name says host; `stream` is a hipStream_t passed as void*.
 *   - activations are bf16 (raw uint16 bits), physically channels-last: an image batch is [N][H][W][C],
 *     a token matrix is [rows][C].  Parameters are fp32 masters with bf16 shadows; conv weights are
 *     [Cout][KH][KW][Cin] (= an OIHW tensor in torch.channels_last memory format), Linear weights [out][in].
 *   - gradients of parameters are fp32 and are written ("accumulate=0") or added ("accumulate=1") in place.
 *   - kernels are asynchronous on `stream`; no entry point synchronises, allocates or frees device memory
 *     (so every one of them can be captured into a hipGraph).
 *
 * Each declaration cites the reference call site it replaces (paths relative to
 * /root/reference/src/neurosis/).
 */
#ifndef NEUROSIS_HIP_H
#define NEUROSIS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

const char* nk_last_error(void);
int nk_abi_version(void);     /* 5 (round 6: + the four *_geglu*_s entry points; bumped whenever an entry point changes; purely additive
                                 entry points -- the CAME and AdamW8bit blocks below -- leave it as it is) */

/* ------------------------------------------------------------------------------------------------
 * nn.Linear  (modules/attention.py:53,65,70,204-209,283-290,618,639; modules/diffusion/openaimodel.py:273-279,
 * 586-590,612-618).  1x1 Conv2d on channels-last data is the same contraction (openaimodel.py:301 skip_connection,
 * modules/diffusion/model.py:150-153 q/k/v/proj_out, :108 nin_shortcut).
 * ---------------------------------------------------------------------------------------------- */
/* y[M,N] = alpha * x[M,K] @ w[N,K]^T + bias[N] + residual[M,N]      (bias, residual optional = NULL) */
int nk_linear_fwd(const void* x, const void* w, const float* bias, const void* residual, void* y,
                  int M, int N, int K, long ldx, long ldw, long ldr, long ldy, float alpha, void* stream);
/* dx[M,K] = dy[M,N] @ w[N,K] + dx_add[M,K]                          (dx_add optional) */
int nk_linear_dgrad(const void* dy, const void* w, const void* dx_add, void* dx, int M, int N, int K,
                    long lddy, long ldw, long ldadd, long lddx, void* stream);
/* dw[N,K] (+)= dy[M,N]^T @ x[M,K]   fp32.  accumulate: 0 overwrite, 1 add, 2 destination is known to be all zero */
/* nk_linear_dgrad of FeedForward.net[2] with the GEGLU backward in its epilogue (modules/attention.py:50-74): du[M][2I] =
 * [d * gelu(g) | d * a * gelu'(g)], d = dy[M][N] @ w[N][I], u = [a | g] [M][2I] saved by the forward */
/* FeedForward.net[0] = GEGLU (modules/attention.py:50-57) in one launch: u[M, 2I] = x @ w^T + bias (kept for the backward) and
 * h[M, I] = u[:, :I] * gelu_erf(u[:, I:]).  Only for shapes nk_linear_fwd_geglu_ok() accepts (whole 256-column tiles on the 256 x 256
 * two-group kernel); otherwise NK_ERR_ARG: call nk_linear_fwd then nk_geglu_fwd. */
long nk_linear_fwd_geglu_ok(int M, int I, int K);
int nk_linear_fwd_geglu(const void* x, const void* w, const float* bias, void* u, void* h, int M, int I, int K, long ldx, long ldw, long ldu,
                        long ldh, void* stream);
int nk_linear_dgrad_geglu(const void* dy, const void* w, const void* u, void* du, int M, int N, int I, long lddy, long ldw, long ldu,
                          long lddu, void* stream);
/* The same pair on the SAVED-DERIVATIVE form of the projection output (round 6).  torch autograd, which is what backs FeedForward in the
 * reference (modules/attention.py:50-74; no backward source), saves a and g and evaluates gelu'(g) in the backward; here the forward -- which
 * has the normal cdf and its exponential in registers already -- writes s[M, 2I] = [gelu(g) | a * gelu'(g)] INSTEAD of u = [a | g] (u itself is
 * never written), and the input gradient of net[2] becomes du[M, 2I] = [d * s[:, :I] | d * s[:, I:]]: two products per element where the
 * erf-GELU derivative took ~22 vector instructions beside an idle matrix pipe.  s is rounded to bf16 like every stored activation.
 * nk_linear_fwd_geglu_s takes the shapes nk_linear_fwd_geglu_ok() accepts; elsewhere: nk_linear_fwd then nk_geglu_fwd_s. */
int nk_linear_fwd_geglu_s(const void* x, const void* w, const float* bias, void* s, void* h, int M, int I, int K, long ldx, long ldw, long lds,
                          long ldh, void* stream);
int nk_linear_dgrad_geglu_s(const void* dy, const void* w, const void* s, void* du, int M, int N, int I, long lddy, long ldw, long lds,
                            long lddu, void* stream);
int nk_linear_wgrad(const void* dy, const void* x, float* dw, int M, int N, int K, long lddy, long ldx,
                    long lddw, int accumulate, void* stream);
/* ... with the bias gradient dbias[N] (+)= column sums of dy from the same launch: the weight-gradient kernel already stages the dy panel;
 * the first column tile of each row block sums it with one extra MFMA per k sub-step against ones (no separate reduction launches) */
int nk_linear_wgrad_bias(const void* dy, const void* x, float* dw, float* dbias, int M, int N, int K, long lddy, long ldx, long lddw,
                         int accumulate, void* stream);

/* Health of the persistent stream-K tile kernel (gemm.hip): a workgroup that finishes a K-split tile waits -- bounded --
 * for the partial tiles of lower-indexed workgroups.  Returns 0 if no launch ever gave up that wait, 1 otherwise
 * (that launch's output is wrong), -1 on a device error.  Synchronises the device; meant for tests and end-of-run checks. */
int nk_gemm_sk_status(void);

/* Backward-health word: fail-closed handling of such a give-up on the TRAINING path (no reference counterpart; the
 * reference's cuBLAS / cuDNN calls cannot produce a partial tile).  The workgroup that gives up poisons its output tile
 * with NaN and raises one device word; nk_adafactor_chunk / nk_adamw_flat gate every kernel of the update on that word
 * (masters, optimizer state and bf16 shadows stay untouched) and return NK_ERR_HEALTH (3) from the NEXT call on, without
 * synchronising (a stream-ordered snapshot of the word to pinned memory).
 *   nk_health_status(): 0 healthy / 1 raised / -1 device error; synchronises.
 *   nk_health_clear():  synchronises, lowers the word and every stream-K flag, so a caller that has decided to go on can.
 *   nk_debug_raise_health(stream): test hook, raises the word the way a kernel would. */
int nk_health_status(void);
int nk_health_clear(void);
/* Data parallelism: nk_health_export writes this rank's word (0 / 1) to a device int32 the caller owns; the caller reduces it over the ranks
 * (MAX) and hands the result to nk_health_import, which raises the local word if any rank's was raised.  Both stream-ordered. */
int nk_health_export(int* dst, void* stream);
int nk_health_import(const int* src, void* stream);
int nk_debug_raise_health(void* stream);
/* Diagnostic: writes the device's 100 MHz constant clock (s_memrealtime) to *dst, stream-ordered and capturable into a hipGraph
 * (tools/step_timeline.py: where the replayed backward segments of the two streams lie in time, untraced). */
int nk_debug_stamp(unsigned long long* dst, void* stream);
/* Test hooks: which kernels did a call launch?  Every launch site reports its kernel's name -- with the template arguments where several
 * instantiations share one (nk_gemm_g2p_kernel<160>, nk_conv3x3_halo_kernel<128,2,1>) -- into a per-thread log while the log is on.
 * nk_debug_launch_log(mode): 1 = on and cleared, 2 = cleared, 0 = off.  nk_debug_launch_names(buf, cap) copies the lines logged by the calling
 * thread since the last clear into the HOST buffer and returns their number (the log keeps the first 64): one line per launch, the name, and
 * behind a launch of the GEMM / convolution tile engine one more, its plan: `name grid=x,y,z block smem splitk ksplit_len acc zero krot gm
 * chunk`.  Host-only: nothing is launched, so both may be called while a stream is capturing.
 * mode 3 = on, cleared and PLAN-ONLY: the tile engine logs the launch it plans for a call and returns NK_OK before it touches the GPU (no
 * zero-fill, no workspace, no launch; outputs stay unwritten) -- which kernel a problem gets can be asked without a device. */
int nk_debug_launch_log(int mode);
long nk_debug_launch_names(char* buf, long cap);

/* `count` (<= 8) weight gradients of identical shape in ONE launch: the three 1280x1280 projections of a transformer
 * block are 100 tiles each, far below one workgroup per CU on their own.  dy / x / dw are HOST arrays of device pointers. */
/* `count` (<= 8) bias-free nn.Linear forwards of identical shape in ONE launch: y[i] = x[i] @ w[i]^T.  Serves the key / value
 * projections of cross-attention (reference modules/attention.py:383-385, `k = self.to_k(context); v = self.to_v(context)`): the
 * context is the same for all 70 transformer blocks of a step and does not depend on the UNet's activations, so UNetModel.fwd
 * projects it for every block up front, eight blocks per launch (308 x 2560 x 2048 each: 60 tiles alone, 480 together). */
/* column sums of `nbatch` consecutive row blocks of M rows each: out[b][N] (+)= sum_rows dy[b*M + r][:].  The per-image gradient of
 * the ResBlock embedding projection (h += emb_out[:, :, None, None], reference openaimodel.py:331-333 -> d emb_out[n] = sum over
 * image n's pixels) in one pair of launches instead of one per image.  ws: nbatch * nk_colsum_ws_floats(M, N) floats. */
int nk_colsum_batched(const void* dy, float* out, float* ws, long M, int N, long ld, int nbatch, int accumulate, void* stream);

int nk_linear_fwd_batched(const void* const* x, const void* const* w, void* const* y, int count, int M, int N, int K,
                          long ldx, long ldw, long ldy, void* stream);

/* dbias: NULL, or `count` pointers (NULL entries allowed) to the layers' bias gradients [N], summed in the same launch */
int nk_linear_wgrad_batched(const void* const* dy, const void* const* x, float* const* dw, float* const* dbias, int count, int M, int N,
                            int K, long lddy, long ldx, long lddw, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * nn.Conv2d as implicit GEMM  (openaimodel.py:124 Upsample.conv, :183-190 Downsample.op, :247-301 ResBlock convs,
 * :622-624 input conv, :797-801 out conv; model.py:71-79 asymmetric-pad stride-2 conv, :98-102, :519, :540 VAE convs).
 * upsample=1 fuses F.interpolate(scale_factor=2, mode="nearest") (openaimodel.py:140) into the gather.
 * ---------------------------------------------------------------------------------------------- */
typedef struct NkConvDesc {
  int N, H, W, Cin;   /* input  x [N][H][W][Cin] (before the optional virtual 2x upsample) */
  int Cout, KH, KW;   /* weight w [Cout][KH][KW][Cin] */
  int stride;         /* 1 or 2 */
  int pad_t, pad_l;   /* zero padding on top / left; bottom / right are implied by Ho, Wo */
  int Ho, Wo;         /* output y [N][Ho][Wo][Cout] */
  int upsample;       /* 1: x is read as its 2x nearest-neighbour upsampling */
} NkConvDesc;
/* y = conv(x, w) + bias[Cout] + rowvec[n][Cout] + residual[N][Ho][Wo][Cout]   (all three optional) */
int nk_conv2d_fwd(const NkConvDesc* d, const void* x, const void* w, const float* bias, const void* rowvec,
                  const void* residual, void* y, void* stream);
/* nk_conv2d_fwd that also emits, from its epilogue, the GroupNorm sums of its OUTPUT as per-tile partials [N][tiles][2 * stats_groups]
 * (entry 2g = sum, 2g+1 = sum of squares of the bf16-rounded values; tiles = nk_conv2d_stats_tiles): the GroupNorm that reads y then needs no
 * statistics pass (openaimodel.py:247-283 in_layers conv -> out_layers GroupNorm; model.py:116-124 conv1 -> norm2).  3 x 3 / stride 1 /
 * padding 1 convolutions the halo-tile kernel takes (conv_halo.h); nk_conv2d_stats_tiles returns 0 where it is not available (run
 * nk_conv2d_fwd and nk_groupnorm_fwd then); with stats_groups = 0 it tells whether the halo-tile kernel takes the shape at all. */
long nk_conv2d_stats_tiles(const NkConvDesc* d, int stats_groups);
int nk_conv2d_fwd_stats(const NkConvDesc* d, const void* x, const void* w, const float* bias, const void* rowvec, const void* residual,
                        void* y, float* stats_part, int stats_groups, void* stream);
/* 3 x 3 / stride 1 / padding 1 forward for images with 3 or 4 real channels stored padded to 8 (x [N][H][W][8], w [Cout][3][3][8]): the
 * first convolutions of the VAE encoder (model.py:519) and of the UNet (openaimodel.py:622-624) as a register-resident FMA kernel --
 * K = 27 / 36 gives the MFMA engine nothing to do, and its gather spent milliseconds on a 1 GB output. */
int nk_conv3x3_few_channels_fwd(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Cout, int cin_real,
                                void* stream);
/* wt[Cin][KH*KW][Cout], taps mirrored (tap t of w lands at tap KH*KW-1-t): the weights with which a stride-1 "same" convolution's
 * INPUT GRADIENT is itself such a convolution, dx = nk_conv2d_fwd(dy, wt) with the channel roles swapped -- how the 3 x 3 input
 * gradients of the ResBlocks (autograd of openaimodel.py:247-301) reach the halo-tile forward kernel. */
int nk_conv_weight_flip(const void* w, void* wt, int Cout, int Cin, int taps, void* stream);
/* nk_conv2d_dgrad with those weights, on the halo-tile forward kernel; _ok = 1 where it applies (3 x 3, stride 1, padding 1, whole
 * 64-channel slabs, images the 32-pixel-wide tiles cover), else use nk_conv2d_dgrad */
long nk_conv2d_dgrad_flipped_ok(const NkConvDesc* d);
int nk_conv2d_dgrad_flipped(const NkConvDesc* d, const void* dy, const void* wt, void* dx, void* stream);
/* dx over the conv input grid ([N][2H][2W][Cin] when upsample=1: follow with nk_upsample2x_bwd) */
int nk_conv2d_dgrad(const NkConvDesc* d, const void* dy, const void* w, void* dx, void* stream);
/* dw[Cout][KH][KW][Cin] (+)= ...  fp32 */
int nk_conv2d_wgrad(const NkConvDesc* d, const void* dy, const void* x, float* dw, int accumulate, void* stream);
/* ... with the bias gradient dbias[Cout] (+)= sum over pixels of dy from the same launch */
int nk_conv2d_wgrad_bias(const NkConvDesc* d, const void* dy, const void* x, float* dw, float* dbias, int accumulate, void* stream);

/* conv3x3(nearest_upsample_2x(x)) (Upsample.conv, openaimodel.py:124-143) as four 2 x 2 phase convolutions of x: 16 products per input pixel
 * and channel pair where the fused-upsample gather of nk_conv2d_fwd(upsample = 1) computes 36.  d is that call's descriptor (3 x 3, stride 1,
 * padding 1, upsample = 1, Ho = 2H, Wo = 2W; anything else is refused); no rowvec, residual or statistics epilogue.
 *   nk_up2_phase_weights   w bf16 [Cout][9][Cin] -> wp bf16 [4][Cout][4][Cin] (phase a*2+b, tap u*2+v: the taps of w that output pixel
 *                          (2i+a, 2j+b) applies to x[i+a-1+u][j+b-1+v], summed in fp32 and rounded once) and, unless NULL, wd bf16
 *                          [Cin][16][Cout], the same sums as the 4 x 4 / stride 2 / padding 1 convolution of dy that is the input gradient
 *   nk_conv2d_up2_fwd      y [N][2H][2W][Cout] = the four phase convolutions (+ bias), pixel-shuffled
 *   nk_conv2d_up2_dgrad    dx [N][H][W][Cin] from dy [N][2H][2W][Cout] and wd, one launch (no nk_upsample2x_bwd behind it)
 *   nk_conv2d_up2_wgrad    dw fp32 [Cout][9][Cin] (+)= the four phase weight gradients folded onto the nine taps; _bias: and dbias[Cout]
 * ws: nk_conv2d_up2_ws_bytes(d, direction) bytes, 16-byte aligned; direction 0 = fwd, 1 = dgrad (none), 2 = wgrad; -1: refused descriptor.
 * accumulate as in nk_conv2d_wgrad. */
int nk_up2_phase_weights(const void* w, void* wp, void* wd, int Cout, int Cin, void* stream);
long nk_conv2d_up2_ws_bytes(const NkConvDesc* d, int direction);
int nk_conv2d_up2_fwd(const NkConvDesc* d, const void* x, const void* wp, const float* bias, void* y, void* ws, void* stream);
int nk_conv2d_up2_dgrad(const NkConvDesc* d, const void* dy, const void* wd, void* dx, void* stream);
int nk_conv2d_up2_wgrad(const NkConvDesc* d, const void* dy, const void* x, float* dw, int accumulate, void* ws, void* stream);
int nk_conv2d_up2_wgrad_bias(const NkConvDesc* d, const void* dy, const void* x, float* dw, float* dbias, int accumulate, void* ws, void* stream);
/* the four phase images [4][N][H][W][C] (phase a*2+b = the pixels (2h+a, 2w+b)) -> y [N][2H][2W][C], and back */
int nk_pixel_shuffle2x(const void* phases, void* y, int N, int H, int W, int C, void* stream);
int nk_pixel_unshuffle2x(const void* y, void* phases, int N, int H, int W, int C, void* stream);
/* dw[co][kh][kw][ci] (+)= sum over the phases, in the order 0..3, of dwp fp32 [4][Cout][4][Cin] at tap (kh > a)*2 + (kw > b); dbias[Cout] (+)= the
 * sum of dbias_p [4][Cout] (both NULL: no bias).  accumulate: 1 = add, 0 / 2 = store */
int nk_up2_fold_wgrad(const float* dwp, const float* dbias_p, float* dw, float* dbias, int Cout, int Cin, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused attention  softmax(q k^T * scale) v, no dropout; no mask
 * (modules/attention.py:410-412 TorchSDPCrossAttention, :337-352 MemoryEfficientCrossAttention) or, forward only, the causal
 * mask of the CLIP text transformers (models/text_encoder/clip.py:311-343 attn_mask; HF CLIPTextModel's causal mask).
 * q/k/v/o are token-major [B][L][H*D] views with explicit row and batch strides (elements), so they can be
 * column slices of a fused projection buffer.  lse is [B][H][Lq] fp32 (saved for the backward).
 * ---------------------------------------------------------------------------------------------- */
typedef struct NkAttnDesc {
  int B, H, Lq, Lk, D;          /* D % 8 == 0, D <= 160; or D == 512 (the VAE mid block's single head, model.py:224-243: forward attn512.h -- lse may be NULL when no backward follows --, backward attn512_bwd.h) */
  long sq, sk, sv, so;          /* row strides of q, k, v, o */
  long bq, bk, bv, bo;          /* batch strides */
  long sdq, sdk, sdv, sdo;      /* backward only: row strides of dq, dk, dv, do */
  long bdq, bdk, bdv, bdo;      /* backward only: batch strides */
  float scale;                  /* D^-0.5 */
  int causal;                   /* key j contributes to query i iff j <= i (Lq == Lk); backward: nk_attention_bwd_causal only */
} NkAttnDesc;
int nk_attention_fwd(const NkAttnDesc* d, const void* q, const void* k, const void* v, void* o, float* lse,
                     void* stream);
/* delta_ws: uninitialised fp32 workspace of nk_attention_bwd_ws_floats(d) elements (row dots + cross-attention partials) */
long nk_attention_bwd_ws_floats(const NkAttnDesc* d);
int nk_attention_bwd(const NkAttnDesc* d, const void* q, const void* k, const void* v, const void* o,
                     const float* lse, const void* d_o, void* dq, void* dk, void* dv, float* delta_ws, void* stream);
/* Backward of the CAUSAL forward (d->causal, head dim 64, Lq == Lk <= 96: the trainable text towers' self-attention).  Same arguments as
 * nk_attention_bwd without the workspace; dq / dk / dv 16-byte aligned.  (nk_attention_bwd refuses causal descriptors.) */
int nk_attention_bwd_causal(const NkAttnDesc* d, const void* q, const void* k, const void* v, const void* o,
                            const float* lse, const void* d_o, void* dq, void* dk, void* dv, void* stream);
/* softmax(scale q k^T + rel[h][j - i + Lq - 1]) v, forward only and without lse: the bidirectional self-attention of the T5 encoders with
 * its additive relative position bias (models/text_encoder/t5.py:38-53: input_ids only, so no padding mask; T5 passes scale = 1).  rel is
 * fp32 [H][Lq + Lk - 1], one row per head, indexed by key minus query position; added in fp32 before the running max.  Lq == Lk <= 1024,
 * D % 8 == 0, D <= 160, !causal; q / k / v / o as for nk_attention_fwd. */
int nk_attention_relbias_fwd(const NkAttnDesc* d, const void* q, const void* k, const void* v, void* o, const float* rel, void* stream);
/* The same under training (the T5 / ByT5 towers trained with the UNet).  _fwd_lse: the same kernel, same launch shape and the same bits in o,
 * also writing lse fp32 [B][H][L], the natural-log sum-exp of the BIASED scores.  _bwd: dq, dk, dv (bf16, strides in d; dq / dk carry
 * d->scale, the bias does not) and d_rel fp32 [H][2 L - 1], d_rel[h][key - query + L - 1] = sum over batch and queries of the fp32
 * dS = P (dP - delta); accumulate 1 adds to d_rel (one tower sums every layer into one buffer), 0 overwrites.  No atomics: every sum has
 * a fixed order, so all four outputs are bitwise reproducible.  ws: nk_attention_relbias_bwd_ws_floats(d) uninitialised floats.  Limits of
 * the forward: Lq == Lk <= 1024, D % 8 == 0, D <= 160, !causal. */
int nk_attention_relbias_fwd_lse(const NkAttnDesc* d, const void* q, const void* k, const void* v, void* o, float* lse, const float* rel, void* stream);
long nk_attention_relbias_bwd_ws_floats(const NkAttnDesc* d);
int nk_attention_relbias_bwd(const NkAttnDesc* d, const void* q, const void* k, const void* v, const void* o, const float* lse, const void* d_o, void* dq,
                             void* dk, void* dv, const float* rel, float* d_rel, float* ws, int accumulate, void* stream);
/* relative_attention_bias.weight's gradient [num_buckets][H] from d_rel [H][2 L - 1]: d_weight[bucket][h] (+)= sum of d_rel[h][i] over the
 * entries i with buckets[i] == bucket (int32 [2 L - 1]), i ascending.  accumulate 0: overwritten (unused buckets exactly 0); 1: added to;
 * 2: written, the caller guarantees zeros. */
int nk_relbias_bucket_sum(const float* d_rel, const int* buckets, float* d_weight, int H, int L, int num_buckets, int accumulate, void* stream);
/* in-place row softmax on bf16 [M][L]: unfused single-head attention = nk_linear_fwd (q k^T) -> nk_softmax_rows -> nk_linear_dgrad (p v).
 * Serves head dims the flash kernels do not take, and the chunked recomputing backward of the VAE mid block (d = 512) beyond 2 048 tokens per
 * sample (ops.attention512_fwd; up to there nk_attention_bwd's flash kernels run); d = 512 forward and backward are nk_attention_fwd / _bwd. */
int nk_softmax_rows(void* s, long M, int L, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm(32, C) (+ fused SiLU) on channels-last x [N][HW][C]
 * (openaimodel.py:247-250,281-283,797-799; attention.py:612 with eps 1e-6, no SiLU; layers.py:5-7 Normalize).
 * mean/rstd: [N][G] fp32 (saved for backward).  ws: uninitialised fp32 workspace of nk_groupnorm_ws_floats elements
 * (statistics are reduced through per-block partials, not atomics: deterministic, no memset).
 * Backward adds into dgamma/dbeta (fp32) and optionally adds dx_add into dx.
 * Sizes, the workspace layout (part [N][nsplit][nz][2G] | gsum [N][2G] | chan [N][nsplit][2][C]) and the launches of every entry point of
 * this family, of LayerNorm / RMSNorm and of the column sums come from one host-only planner, csrc/norm_plan.h: the *_ws_floats queries
 * answer from the plan the entry points run (0 for a shape they refuse), and in plan-only mode (nk_debug_launch_log(3)) the entry points
 * log `name grid=x,y,z block smem [region=offset+extent ...] ws=ws_floats` per launch and return before touching a pointer or the device.
 * ---------------------------------------------------------------------------------------------- */
long nk_groupnorm_ws_floats(int N, int HW, int C, int G); /* fp32 elements of `ws`: the same for the forward, the sums and the backward */
int nk_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                     float* ws, int N, int HW, int C, int G, float eps, int silu, void* stream);
/* The forward in separable passes (what nk_groupnorm_fwd runs back to back): sums [N][2G] (entry 2g = sum, 2g+1 = sum of squares over
 * HW * C/G elements) from x, or from a convolution's per-tile partials; and the normalisation given the sums. */
int nk_groupnorm_sums(const void* x, float* sums, float* ws, int N, int HW, int C, int G, void* stream);
long nk_groupnorm_sums_ws_floats(int N, int nparts, int G); /* level 1's [N][64][2G] partial rows (used beyond 128 rows per image); the same for every nparts */
int nk_groupnorm_sums_from_parts(const float* part, float* sums, float* ws, int N, int nparts, int G, void* stream);
int nk_groupnorm_apply(const void* x, const float* sums, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                       int N, int HW, int C, int G, float eps, int silu, void* stream);
int nk_groupnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                     const float* rstd, const void* dx_add, void* dx, float* dgamma, float* dbeta, float* ws,
                     int N, int HW, int C, int G, int silu, int accumulate, void* stream);
/* Scale-shift modulated GroupNorm (ResBlock use_scale_shift_norm): y = silu?(GN(x) * (1 + scale) + shift) with mod = bf16 [N][2C], per
 * image scale in the first C columns and shift in the last C; 1 + scale and the whole affine in fp32.  _mod_fwd is the one-call form,
 * _mod_apply consumes sums like nk_groupnorm_apply; ws as for nk_groupnorm_fwd / _bwd.  The backward also writes dmod = bf16 [N][2C],
 * d_scale | d_shift; every reduction goes through fixed-order partials (no atomics, no memset).  With mod == 0 all three compute what the
 * unmodulated entry points do, bit for bit. */
int nk_groupnorm_mod_fwd(const void* x, const float* gamma, const float* beta, const void* mod, void* y, float* mean, float* rstd,
                         float* ws, int N, int HW, int C, int G, float eps, int silu, void* stream);
int nk_groupnorm_mod_apply(const void* x, const float* sums, const float* gamma, const float* beta, const void* mod, void* y, float* mean,
                           float* rstd, int N, int HW, int C, int G, float eps, int silu, void* stream);
int nk_groupnorm_mod_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const void* mod, const float* mean,
                         const float* rstd, const void* dx_add, void* dx, float* dgamma, float* dbeta, void* dmod, float* ws,
                         int N, int HW, int C, int G, int silu, int accumulate, void* stream);

/* nn.LayerNorm(C) over rows of [M][C] (attention.py:468-470).  mean/rstd: [M] fp32. */
int nk_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                     int M, int C, float eps, void* stream);
long nk_layernorm_ws_floats(int M, int C); /* `ws` of nk_layernorm_bwd and _bwd_params: partial rows [rows][2][C], room for the larger of their two splits; for every C % 8 == 0 (_bwd_params takes widths beyond 2048) */
/* T5LayerNorm (RMS norm: no mean subtraction, no bias), forward only: y[m][c] = x[m][c] * rsqrt(mean_c(x[m]^2) + eps) * gamma[c] on bf16
 * [M][C], fp32 gamma, C % 8 == 0, C <= 4096.  The fp32 reduction has a fixed order: a row's bits do not depend on M. */
int nk_rmsnorm_fwd(const void* x, const float* gamma, void* y, int M, int C, float eps, void* stream);
/* ... under training: _fwd_rstd also keeps rstd [M] fp32 (y has nk_rmsnorm_fwd's bits).  _bwd: dx = rstd (g o dy - xhat mean_c(g o dy o xhat))
 * (+ dx_add, added in fp32 before the single rounding to bf16), xhat = x rstd, and dgamma[c] (+)= sum_m dy xhat through partial rows and the
 * fixed-order column reducer (accumulate 0 / 1).  ws: nk_rmsnorm_bwd_ws_floats(M, C) floats.  C % 8 == 0, C <= 4096, any M; a row's dx does
 * not depend on M. */
int nk_rmsnorm_fwd_rstd(const void* x, const float* gamma, void* y, float* rstd, int M, int C, float eps, void* stream);
long nk_rmsnorm_bwd_ws_floats(int M, int C);
int nk_rmsnorm_bwd(const void* dy, const void* x, const float* gamma, const float* rstd, const void* dx_add, void* dx, float* dgamma, float* ws, int M, int C,
                   int accumulate, void* stream);
int nk_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                     const void* dx_add, void* dx, float* dgamma, float* dbeta, float* ws, int M, int C, int accumulate, void* stream);
/* The one-pass form in its two halves (round 5: what the transformer blocks use): _rows writes dx and nk_layernorm_part_rows(M) partial rows
 * [rows][2][C] (sum dy * xhat | sum dy over the rows each workgroup walked) into `part`; nk_colpart_reduce_batch sums the partial rows of up to
 * NK_COLPART_MAX such launches into their dgamma / dbeta in ONE launch, on any stream, any time later (the three LayerNorms of a
 * BasicTransformerBlock, attention.py:487-511, are reduced behind the block's batched weight gradients). */
#define NK_COLPART_MAX 32
typedef struct NkColpartBatch {
  const float* part[NK_COLPART_MAX];
  float* dgamma[NK_COLPART_MAX];
  float* dbeta[NK_COLPART_MAX];
  int nrows[NK_COLPART_MAX];
  int C[NK_COLPART_MAX];
  int accumulate[NK_COLPART_MAX];     /* 0: overwrite dgamma / dbeta, 1: add to them */
  int n;
} NkColpartBatch;
long nk_layernorm_part_rows(int M);
int nk_layernorm_bwd_rows(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                          const void* dx_add, void* dx, float* part, int M, int C, void* stream);
int nk_colpart_reduce_batch(const NkColpartBatch* b, void* stream);
/* The same in two parts, so the caller can run the parameter gradients (off the critical path of backward) on another
 * stream: _dx needs no workspace; _params reads dy, x and the saved statistics only. */
int nk_layernorm_bwd_dx(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                        const void* dx_add, void* dx, int M, int C, void* stream);
int nk_layernorm_bwd_params(const void* dy, const void* x, const float* mean, const float* rstd, float* dgamma,
                            float* dbeta, float* ws, int M, int C, int accumulate, void* stream);

/* GEGLU (attention.py:55-57): y[M][I] = u[:, :I] * gelu_erf(u[:, I:]) */
int nk_geglu_fwd(const void* u, void* y, long M, int I, void* stream);
int nk_geglu_bwd(const void* dy, const void* u, void* du, long M, int I, void* stream);
/* ... and in the saved-derivative form: y = a * gelu(g), s[M][2I] = [gelu(g) | a * gelu'(g)] from u = [a | g] (s may alias u); du = [dy * s1 | dy * s2] */
int nk_geglu_fwd_s(const void* u, void* y, void* s, long M, int I, void* stream);
int nk_geglu_bwd_s(const void* dy, const void* s, void* du, long M, int I, void* stream);

/* nn.SiLU on a flat bf16 array (openaimodel.py:274,588,615) */
int nk_silu_fwd(const void* x, void* y, long n, void* stream);
int nk_silu_bwd(const void* dy, const void* x, void* dx, long n, void* stream);

/* nn.Dropout of the training path (openaimodel.py:284 ResBlock.out_layers; modules/attention.py:69 FeedForward.net[1], :210 to_out[1];
 * modules/diffusion/model.py:106,125 ResnetBlock.dropout): y = x * mask * scale (+ residual) on bf16 rows, in place allowed (y == x).  The mask
 * is never stored: Philox4x32-10, one call per 8 consecutive LOGICAL elements e = row * cols + col (the row strides play no part, so one
 * mask over [rows, cols] can be laid over a column half of a wider buffer), counter (e / 8 low, e / 8 high, site, step low word), key
 * (seed low, seed high); element j = e % 8 takes the 16-bit half (word[j >> 1] >> 16 (j & 1)) & 0xffff and is kept iff half >= thr.
 * thr = round(p * 65536) and scale = 1 / (1 - p) come from the host.  kept: y = bf16(fmul_rn(x, scale)), dropped: +0; with a residual
 * y = bf16(fadd_rn(residual, that fp32 value)).  {seed, step} are two 64-bit words READ FROM DEVICE MEMORY at `token` (a captured launch
 * sees a new mask on every replay).  The backward is the same call on dy.  cols % 8 == 0, 16-byte-aligned rows. */
int nk_dropout(const void* x, const void* residual, void* y, long rows, int cols, long ld_x, long ld_res, long ld_y, const void* token,
               int site, int thr, float scale, void* stream);
/* one draw: state = {seed, step} (two 64-bit words, one persistent allocation per device): step += 1; token = {seed, step} */
int nk_dropout_draw(void* state, void* token, void* stream);

/* out = a + b on flat bf16 arrays: gradient join where one tensor feeds two consumers (skip connections,
 * openaimodel.py:832-836) */
int nk_add(const void* a, const void* b, void* out, long n, void* stream);

/* torch.cat([h, skip], dim=1) on channels-last rows and its backward (openaimodel.py:836) */
int nk_cat_channels(const void* a, const void* b, void* out, long rows, int Ca, int Cb, void* stream);
int nk_split_channels(const void* src, void* a, void* b, long rows, int Ca, int Cb, void* stream);

/* backward of F.interpolate(scale_factor=2, mode="nearest") (openaimodel.py:140): 2x2 sum-pool */
int nk_upsample2x_bwd(const void* dup, void* dx, int N, int H, int W, int C, void* stream);
/* nearest 2x as a materialised copy, x [N][H][W][C] -> up [N][2H][2W][C] (its backward is nk_upsample2x_bwd); and avg_pool2d(2, 2) in
 * floor mode, x [N][H][W][C] -> y [N][H/2][W/2][C] (fp32 sum, one rounding), whose backward writes dy / 4 to the four inputs of each
 * window and zeros into an odd last row or column.  C % 8 == 0. */
int nk_upsample2x_fwd(const void* x, void* up, int N, int H, int W, int C, void* stream);
int nk_avgpool2x_fwd(const void* x, void* y, int N, int H, int W, int C, void* stream);
int nk_avgpool2x_bwd(const void* dy, void* dx, int N, int H, int W, int C, void* stream);

/* boundary layout/dtype conversion: NCHW (fp32 or bf16) <-> channels-last bf16 with channels padded to Cpad */
int nk_nchw_to_nhwc(const void* src, int src_is_f32, void* dst, int N, int C, int HW, int Cpad, float scale,
                    void* stream);
int nk_nhwc_to_nchw(const void* src, void* dst, int dst_is_f32, int N, int C, int HW, int Cpad, void* stream);
int nk_cast_f32_to_bf16(const float* src, void* dst, long n, void* stream);
int nk_cast_bf16_to_f32(const void* src, float* dst, long n, void* stream);

/* bias gradient: out[N] (+)= sum over rows of dy[M][N] (row stride ld) */
long nk_colsum_ws_floats(long M, int N);
int nk_colsum(const void* dy, float* out, float* ws, long M, int N, long ld, int accumulate, void* stream);

/* backward of nk_softmax_rows, in place on dp [M][L] bf16 given the probabilities p: ds = p * (dp - sum_j dp*p) * scale
 * (AttnBlock of the VAE, modules/diffusion/model.py:144-222, when the autoencoder itself is trained: SURVEY 8(f) N2) */
int nk_softmax_rows_bwd(const void* p, void* dp, long M, int L, float scale, void* stream);

/* PatchGAN discriminator pieces (modules/losses/patchgan/model.py:21-95).  Tokens x[M][C] bf16, M = N*H*W.
 * LeakyReLU: y = x >= 0 ? x : slope*x; the backward takes the OUTPUT y (same sign as x).
 * BatchNorm2d in training mode with the following LeakyReLU fused (slope = 1: none): batch mean / biased variance per
 * channel over all M rows, y = act((x - mean) * rstd * gamma + beta); running_mean / running_var (optional) updated with
 * `momentum` and the unbiased variance, as nn.BatchNorm2d does.  backward: dgamma, dbeta (+= when accumulate) and dx.
 * ws: nk_batchnorm_ws_floats(M, C) fp32 elements of scratch. */
int nk_leaky_relu_fwd(const void* x, void* y, long n, float slope, void* stream);
int nk_leaky_relu_bwd(const void* dy, const void* y, void* dx, long n, float slope, void* stream);
long nk_batchnorm_ws_floats(long M, int C);
int nk_batchnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, float* running_mean,
                     float* running_var, float* ws, long M, int C, float eps, float momentum, float slope, void* stream);
int nk_batchnorm_bwd(const void* dy, const void* x, const void* y, const float* gamma, const float* mean, const float* rstd, void* dx,
                     float* dgamma, float* dbeta, float* ws, long M, int C, float slope, int accumulate, void* stream);
/* BatchNorm2d in evaluation mode (+ LeakyReLU): y = act((x - running_mean) * rsqrt(running_var + eps) * gamma + beta); the discriminator
 * as log_images / validation see it (nn.BatchNorm2d.eval() inside NLayerDiscriminator, patchgan/model.py:53-83).  ws: C fp32 elements. */
int nk_batchnorm_eval(const void* x, const float* gamma, const float* beta, const float* running_mean, const float* running_var, void* y,
                      float* ws, long M, int C, float eps, float slope, void* stream);

/* LPIPS pieces (modules/losses/perceptual.py:64-228 over the AlexNet or VGG16 trunk of extractors.py:11-30).
 * ReLU = nk_leaky_relu_* with slope 0.
 * maxpool2x2: tokens [N][H][W][C] -> [N][H/2][W/2][C]; the backward routes each window's gradient to its first maximum.
 * maxpool: k x k windows at stride s, no padding, floor mode (nn.MaxPool2d(k, s); AlexNet's 3 x 3 / 2): [N][H][W][C] ->
 * [N][(H-k)/s+1][(W-k)/s+1][C]; overlapping windows' gradients add up in the backward.
 * lpips_layer: out[n] (+)= mean_p sum_c w[c] (f0/(|f0|+eps) - f1/(|f1|+eps))^2 over a layer's features [N][HW][C] (normalize_tensor,
 * NetLinLayer, spatial_average: perceptual.py:215-224,198-212); the backward returns upstream[n] * d out[n] / d f1. */
int nk_maxpool2x2_fwd(const void* x, void* y, int N, int H, int W, int C, void* stream);
int nk_maxpool2x2_bwd(const void* dy, const void* x, void* dx, int N, int H, int W, int C, void* stream);
int nk_maxpool_fwd(const void* x, void* y, int N, int H, int W, int C, int k, int s, void* stream);
int nk_maxpool_bwd(const void* dy, const void* x, void* dx, int N, int H, int W, int C, int k, int s, void* stream);
long nk_lpips_layer_ws_floats(int N, int HW);
int nk_lpips_layer_fwd(const void* f0, const void* f1, const float* w, float* out, float* ws, int N, int HW, int C, float eps,
                       int accumulate, void* stream);
int nk_lpips_layer_bwd(const void* f0, const void* f1, const float* w, const float* upstream, void* df1, int N, int HW, int C,
                       float eps, void* stream);

/* y = gelu(x) elementwise over n bf16 values (n % 8 == 0).  mode 0: exact, 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU in open_clip's
 * text tower, models/text_encoder/clip.py:333-343); mode 1: "quick_gelu" x * sigmoid(1.702 x) (HF CLIPTextModel of
 * openai/clip-vit-large-patch14, models/text_encoder/clip.py:49-56). */
int nk_gelu_fwd(const void* x, void* y, long n, int mode, void* stream);
/* ... forward only: mode 2, "gelu_new" 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))); mode 3, ReLU (the ungated FeedForwards of the T5
 * encoders, models/text_encoder/t5.py:38-53 over transformers' T5DenseActDense).  y = gelu_new(u[:, :I]) * u[:, I:] for u [M][2 I] bf16, the
 * stacked projection [wi_0; wi_1] of T5 v1.1 / ByT5 (T5DenseGatedActDense); fp32 arithmetic, I % 8 == 0, y [M][I] dense. */
int nk_gated_gelu_tanh_fwd(const void* u, void* y, long M, int I, void* stream);
/* dx = dy * gelu'(x), same modes as nk_gelu_fwd; bf16 in and out, fp32 arithmetic (trainable text towers) */
int nk_gelu_bwd(const void* dy, const void* x, void* dx, long n, int mode, void* stream);
/* ... in all four modes of nk_gelu_fwd (2: gelu_new; 3: ReLU, dx = dy where x > 0, exactly): the T5 FeedForwards under training.
 * nk_gated_gelu_tanh_bwd: du [M][2 I] = [dy b gelu_new'(a) | dy gelu_new(a)] from dy [M][I] and u = [a | b] (nk_gated_gelu_tanh_fwd's input). */
int nk_act_bwd(const void* dy, const void* x, void* dx, long n, int mode, void* stream);
int nk_gated_gelu_tanh_bwd(const void* dy, const void* u, void* du, long M, int I, void* stream);
/* Token + position embedding backward of the text towers (x[b * L + l] = table[ids[b][l]] + pos[l]): dx [B * L][C] bf16 (row stride ldx);
 * dtable [V][C] and dpos [P][C] fp32 gradients.  accumulate 0: both are overwritten and rows no token (position) hit come out zero;
 * 1: added to; 2: written, the caller guarantees both are zero already (no clearing pass).  Deterministic: every row is a sum in token
 * order, no atomics.  ids int64 [B * L], 0 <= id < V; B * L <= NK_EMBEDDING_BWD_MAX_TOKENS (the duplicate-id scans are quadratic).
 * dpos == NULL with P == 0: no position table (the T5 encoders). */
#define NK_EMBEDDING_BWD_MAX_TOKENS 8192
int nk_embedding_bwd(const long long* ids, const void* dx, long ldx, float* dtable, float* dpos, int B, int L, int V, int P, int C,
                     int accumulate, void* stream);
/* Label embeddings of a class-conditional UNet (modules/diffusion/openaimodel.py:574-590: num_classes an int or "continuous") and
 * ClassEmbedder (modules/encoders/classed.py:9-32).
 * label_rows_fwd: out[b][:] = table[ids[b]][:] (+ add[b][:]); table fp32 [V][D] dense, ids int64 [B], add bf16 [B][D] dense or NULL, out
 *                 [B][D] dense, fp32 (out_is_f32) or bf16 (fp32 sum, one round-to-nearest-even).  An id outside [0, V) is never used as an
 *                 address: its output row is NaN.  D % 8 == 0.
 * label_rows_bwd: dtable[v][:] = sum of d[b][:] over the b with ids[b] = v, in ascending b, fp32; d [B][D] bf16 or fp32 (d_is_f32), row stride
 *                 ldd.  nk_embedding_bwd's kernel with L = 1 and no position table: the same accumulate modes (0: the whole table is
 *                 overwritten, rows no sample hit are zero; 1: the new sum is formed first and added once; 2: written, the caller's
 *                 table is zero already), the same bits on every run, the same cap B <= NK_EMBEDDING_BWD_MAX_TOKENS.
 * linear1_fwd:    nn.Linear(1, D): out[b][j] = bf16(y[b] w[j] + bias[j] (+ add[b][j])); y fp32 [B], w / bias fp32 [D], add / out bf16 [B][D].
 * linear1_bwd:    dw[j] = sum_b y[b] d[b][j], db[j] = sum_b d[b][j] in ascending b, fp32 (accumulate 0 / 2: written, 1: added to);
 *                 dy[b] = sum_j d[b][j] w[j] (fixed order) unless dy is NULL.  d bf16 [B][D] dense. */
int nk_label_rows_fwd(const float* table, const long long* ids, const void* add, void* out, int out_is_f32, int B, int V, int D, void* stream);
int nk_label_rows_bwd(const long long* ids, const void* d, long ldd, int d_is_f32, float* dtable, int B, int V, int D, int accumulate, void* stream);
int nk_linear1_fwd(const float* y, const float* w, const float* bias, const void* add, void* out, int B, int D, void* stream);
int nk_linear1_bwd(const void* d, const float* y, const float* w, float* dw, float* db, float* dy, int B, int D, int accumulate, void* stream);
/* backward of a row gather sel[b] = x[b * L + idx[b]]: dx [B * L][C] bf16 (dense) = 0 except those rows = dsel[b] (row stride ldsel) */
int nk_gather_rows_bwd(const void* dsel, long ldsel, const long long* idx, void* dx, int B, int L, int C, void* stream);
/* dw [K][N] fp32 (row stride lddw) (+)= x^T dy over M <= 256 rows (x [M][K], dy [M][N] bf16): weight gradients the tile engine does not take
 * (bigG's text_projection sees only the B end-of-text rows); fixed-order sums */
int nk_wgrad_few_rows(const void* x, long ldx, const void* dy, long lddy, float* dw, long lddw, int M, int K, int N, int accumulate, void* stream);

/* Vector-quantizer bottleneck (modules/autoencoding/regularizers/quantize.py: VectorQuantizer.forward :222-272, EMAVectorQuantizer.forward
 * :362-409), csrc/vq.hip.  All fp32, no float atomics: every result is bit-reproducible.  1 <= D <= NK_VQ_MAX_D, 1 <= n_e <=
 * NK_VQ_MAX_CODES, N < 2^31, refused with a message otherwise.  z [N][D] with row stride ldz (elements), codebook [n_e][D] dense.
 * search:     idx[i] = argmin_j d_j, d_j = fma(-2, z_i . e_j, n_j): n_j = sum_k e_jk^2 and the dot product are fp32 fma chains in k order from
 *             0 (the dot product on v_mfma_f32_16x16x4_f32, whose result is that chain); |z_i|^2 is left out (constant along a row).  Among
 *             bitwise-equal scores the lowest j wins; a NaN score is never chosen unless the whole row is NaN (then 0).  The [N][n_e] matrix is
 *             never written.  ws: nk_vq_search_ws_floats(N, n_e) floats (the norms; with few rows the code tiles are also cut across workgroups
 *             and each cut's (min, index) per row is merged from there in cut order -- the same index whatever the cut).
 * code_stats: count[j] = #{i : idx[i] = j} (int64), sum[j][:] = the rows z_i of code j added in rising i (a chain of count[j] additions);
 *             codes nobody chose give exact zeros.  Feeds the codebook gradient, the EMA update, perplexity and cluster usage.
 * quantize:   zq = codebook[idx] as fp32 [N / HW][D][HW] (row i = b * HW + p; HW = 1: the [N][D] matrix) and sumsq[0] = sum (zq - z)^2 by a
 *             fixed-order reduction (longest chain D + ceil(ceil(N / 256) / 256) + 16).  ws: nk_vq_quantize_ws_floats(N) floats. */
#define NK_VQ_MAX_D 256
#define NK_VQ_MAX_CODES 65536
long nk_vq_search_ws_floats(long N, int n_e);
int nk_vq_search(const float* z, long ldz, const float* codebook, float* ws, long long* idx, long N, int D, int n_e, void* stream);
int nk_vq_code_stats(const long long* idx, const float* z, long ldz, long long* count, float* sum, long N, int D, int n_e, void* stream);
long nk_vq_quantize_ws_floats(long N);
int nk_vq_quantize(const long long* idx, const float* codebook, const float* z, long ldz, float* zq, float* sumsq, float* ws, long N, int D,
                   int n_e, int HW, void* stream);

/* Gumbel-softmax quantizer bottleneck (modules/autoencoding/regularizers/quantize.py:59-160, GumbelQuantizer.forward :114-148),
 * csrc/gumbel.hip.  No float atomics: every result is bit-identical from run to run.  z [N][h] fp32 with row stride ldz, 1 <= h <=
 * NK_VQ_MAX_D, 1 <= n <= NK_VQ_MAX_CODES, N < 2^31, refused with a message otherwise.
 * logits:      logits[i][j] = fadd_rn(sum_k z_ik w_jk, bias_j) into fp32 [N][n] with row stride ldl; w [n][h] dense (the 1x1 conv's weight).  The
 *              dot product is the fp32 fma chain in rising k from 0 (on v_mfma_f32_16x16x4_f32, as nk_vq_search): the forward decides an index.
 * noise:       g[rows][cols] dense fp32, a pure function of (token, site, e = i * cols + j): Philox4x32-10, one call per 4 consecutive e,
 *              counter (e / 4 low, e / 4 high, site, step low word), key (seed low, seed high ^ 0x47554D42); element e % 4 takes word w,
 *              u = (2 (w >> 9) + 1) 2^-24, g = -logf(-logf(u)).  {seed, step} are read from device memory at `token` (nk_dropout_draw).
 * softmax_fwd: a_j = fmul_rn(fadd_rn(l_j, g_j), inv_tau), g from `noise` [N][n] dense or (noise NULL) from the generator above with `token`,
 *              `site` -- bitwise the same either way; y = softmax(a) as bf16 [N][n] dense; idx[i] = argmax_j a_j (lowest index among equal
 *              scores, a NaN never taken); kl[0] = (1 / N) sum_i sum_j q_j log(q_j n + 1e-10), q = softmax(l), summed in a fixed order.
 *              ws: nk_gumbel_softmax_ws_floats(N) floats (the rows' KL terms).
 * softmax_bwd: in place on bf16 G [N][n] dense (the gradient with respect to the soft one-hot): G_j <- inv_tau y_j (G_j - sum_k G_k y_k) +
 *              (w_kl / N) q_j (h_j - sum_k q_k h_k), h_j = log(q_j n + 1e-10) + q_j n / (q_j n + 1e-10), q recomputed from the logits, fp32
 *              sums in a fixed order: the gradient of <G, y> + w_kl * kl with respect to the logits.
 * inv_tau and w_kl are launch arguments (a captured graph would freeze them). */
int nk_gumbel_logits(const float* z, long ldz, const float* w, const float* bias, float* logits, long ldl, long N, int h, int n, void* stream);
int nk_gumbel_noise(float* g, long rows, int cols, const void* token, int site, void* stream);
long nk_gumbel_softmax_ws_floats(long N);
int nk_gumbel_softmax_fwd(const float* logits, long ldl, const float* noise, const void* token, int site, float inv_tau, void* y,
                          long long* idx, float* kl, float* ws, long N, int n, void* stream);
int nk_gumbel_softmax_bwd(const float* logits, long ldl, const void* y, void* G, float inv_tau, float w_kl, long N, int n, void* stream);

/* Separable banded resampler on dense fp32 planes, csrc/resample.hip: y[p] = Wv . x[p] . Wh^T for p < P, x [P][H][W] -> y [P][OH][OW].
 * With the tables of F.interpolate(mode="bicubic", antialias=True) it is the resize_input / resize_target step of the autoencoder losses
 * (modules/autoencoding/losses/vae_lpips_discr.py:104-107, :326-329); called with the transposed tables ([H x OH], [W x OW]) and the sizes
 * swapped it is that step's adjoint -- one kernel pair for both directions, no atomics, bit-identical from run to run.
 * A banded matrix with n_out rows is three device arrays: start[n_out] and count[n_out] (int32: row i has its non-zeros in columns
 * start[i] .. start[i] + count[i] - 1, inside the input) and weights[n_out][taps] fp32, each row padded with zeros; v_* is Wv [OH x H],
 * h_* is Wh [OW x W].  ws: nk_resample_ws_floats(P, H, W, OH, OW) floats, the intermediate of the two passes (the smaller of
 * [P][OH][W] and [P][H][OW]); x, y and ws must not overlap.  No size has a divisibility requirement; P * max(H, OH) * max(W, OW) <= 2^38.
 * The launch allocates nothing, synchronises nothing and reads nothing on the host: it can be captured into a graph. */
long nk_resample_ws_floats(long P, int H, int W, int OH, int OW);
int nk_resample_planes(const float* x, float* y, float* ws, const int* v_start, const int* v_count, const float* v_weights, int v_taps,
                       const int* h_start, const int* h_count, const float* h_weights, int h_taps, long P, int H, int W, int OH, int OW,
                       void* stream);

/* timestep_embedding (modules/diffusion/util.py:152-177): out[B][dim] bf16 = [cos | sin](t * freq) */
int nk_timestep_embedding(const float* t, void* out, int B, int dim, float max_period, void* stream);

/* StandardDiffusionLoss "edm" branch + Denoiser scaling (modules/diffusion/loss.py:117-157,
 * modules/diffusion/denoiser.py:41-53, modules/losses/functions.py:91-94).
 * prepare: z_t = x + sigma*eps (fp32 NCHW); net_in = bf16 channels-last z_t*c_in, channels padded to Cpad.
 * loss:    D = net_out*c_out + z_t*c_skip; loss[b] = w[b]*mean((D-target)^2);
 *          dnet (optional) = upstream * dloss[b]/dnet_out, bf16 channels-last padded.
 * prepare_cat: prepare for a concat-conditioned UNet (OpenAIWrapper.forward, modules/diffusion/wrappers.py:33: inpainting / edit /
 *          upscale models).  extra: fp32 NCHW [B][Ce][HW]; net_in[b][p][c] = bf16(z_t*c_in) for c < C, bf16(extra[b][c-C][p]) for
 *          C <= c < C+Ce (NOT scaled by c_in: the denoiser scales the latents, the wrapper concatenates afterwards), 0 up to Cpad.
 *          Cpad % 8 == 0, 0 <= Cpad - (C+Ce) < 8; extra may be NULL when Ce == 0.  z_t and the latent channels are bit-equal to prepare's. */
int nk_edm_prepare(const float* x, const float* eps, const float* sigma, const float* c_in, float* zt, void* net_in,
                   int B, int C, int HW, int Cpad, void* stream);
int nk_edm_prepare_cat(const float* x, const float* eps, const float* sigma, const float* c_in, const float* extra, float* zt,
                       void* net_in, int B, int C, int Ce, int HW, int Cpad, void* stream);
int nk_edm_loss(const void* net_out, const float* zt, const float* target, const float* c_out, const float* c_skip,
                const float* w, float* loss, void* dnet, int B, int C, int HW, int Cpad, float upstream, void* stream);

/* Sampler-side latent kernels.  x / denoised / x_next: fp32 NCHW [B][C][HW]; net_in / net_out: bf16
 * channels-last tokens [rep*B][HW][Cpad], rep = 2 for classifier-free guidance laid out [uncond | cond]
 * (VanillaCFG.prepare_inputs, modules/guidance.py:26-37).
 * prepare:    net_in[r*B+b] = bf16(c_in[b] * x[b]) for r < rep        (Denoiser.forward input scaling, denoiser.py:41-49,
 *             + the guider's torch.cat([x] * 2))
 * prepare_cat: the same for a concat-conditioned UNet: channels C..C+Ce-1 of replica 0 = bf16(extra_u[b]), of replica 1 =
 *             bf16(extra_c[b]) (fp32 NCHW [B][Ce][HW], unscaled; rep == 1 reads extra_c only), 0 up to Cpad;
 *             Cpad % 8 == 0, 0 <= Cpad - (C+Ce) < 8
 * denoise:    D = c_skip[b]*x + c_out[b]*(F_u + scale*(F_c - F_u))    (denoiser.py:49-53 + VanillaCFG.__call__ guidance.py:21-24;
 *             rep == 1: F = net_out, scale ignored)
 * euler_step: d = (x - D)/sigma_hat[b]; x_next = x + (sigma_next[b] - sigma_hat[b])*d   (EDMSampler.sampler_step with the
 *             Euler correction, sampling/sampling.py:166-181,313-316, to_d sampling/utils.py:49-51).  x_next may alias x;
 *             `denoised` is optional (NULL to skip). */
int nk_sample_prepare(const float* x, const float* c_in, void* net_in, int B, int C, int HW, int Cpad, int rep, void* stream);
int nk_sample_prepare_cat(const float* x, const float* c_in, const float* extra_u, const float* extra_c, void* net_in, int B, int C,
                          int Ce, int HW, int Cpad, int rep, void* stream);
int nk_sample_denoise(const void* net_out, const float* x, const float* c_skip, const float* c_out, float scale,
                      float* denoised, int B, int C, int HW, int Cpad, int rep, void* stream);
int nk_sample_euler_step(const void* net_out, const float* x, const float* c_skip, const float* c_out, const float* sigma_hat,
                         const float* sigma_next, float scale, float* x_next, float* denoised, int B, int C, int HW, int Cpad,
                         int rep, void* stream);

/* Fused AdamW over the flat fp32 parameter buffer; also rewrites the bf16 shadow the kernels read.
 * (The optimizer itself is outside SURVEY section 8(a); bench.py needs a real parameter update in the timed step.) */
int nk_adamw_flat(float* p, const float* g, float* m, float* v, void* shadow, long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused multi-tensor Adafactor on the flat buffers.  Replaces Adafactor.step,
 * reference optimizers/adafactor.py:162-255 (_get_lr :133-147, _rms :150-151, _approx_sq_grad :154-159): the per-tensor
 * Python loop becomes three launches per chunk of consecutive tensors (statistics, update RMS of the matrices, apply; the per-strip and
 * per-tensor finalisations ride in the last block of each pass to finish).  `tensors` / `items` are device tables built by the
 * host (layout: neurosis_amd/csrc/optim.hip NkAfTensor / NkAfItem; nk_adafactor_tensor_bytes() guards the mirror).
 * nk_adafactor_init fills the per-item partial sums of p^2 once; nk_adafactor_chunk performs one step for tensors
 * [tensor_lo, tensor_hi) = items [item_lo, item_hi).  beta2t = 1 - step^decay_rate and rel_step are host scalars. */
typedef struct NkAdafactorArgs {
  float* master; const float* grad; void* shadow; float* state; float* ws;
  const void* tensors; const void* items;
  float* u2_part; float* p2_part; float* mean_row; float* scale; float* lr_t;
  int item_lo, item_hi, tensor_lo, tensor_hi;
  float beta2t, eps1, eps2, clip_threshold, rel_step, weight_decay, grad_scale;
  int scale_parameter;
  unsigned* counters;   /* "blocks done" counters, one range per tensor (NkAfTensor.cnt0); all zero before a step, all zero after it */
  int has_matrix;       /* the chunk holds at least one 2-D tensor (the update-RMS pass of the matrices is launched) */
  int reserved;
} NkAdafactorArgs;
long nk_adafactor_tensor_bytes(void);
int nk_adafactor_init(const NkAdafactorArgs* args, void* stream);
int nk_adafactor_chunk(const NkAdafactorArgs* args, void* stream);
/* The same step with the reference's first moment (beta1, adafactor.py:194-196, 242-245): the apply pass keeps
 * exp_avg = beta1 * exp_avg + (1 - beta1) * scale * u and subtracts that instead of scale * u.  `exp_avg` is one flat fp32 buffer with the
 * masters' physical layout and element offsets (NkAfTensor.off), zero before the first step; no bias correction.  0 <= beta1 < 1. */
int nk_adafactor_chunk_momentum(const NkAdafactorArgs* args, float* exp_avg, float beta1, void* stream);

/* Fused multi-tensor CAME on the flat buffers.  Replaces CAME.step, reference optimizers/came.py:115-224: per tensor, Adafactor's
 * factored second moment of g^2+eps1 (R, C; vectors: v), the update u clipped by its RMS (u_hat), a first moment m, and for factored
 * tensors a second factored statistic of (u_hat - m)^2 + eps2 (Rr, Cr) that preconditions m.  Up to four launches per chunk of
 * consecutive tensors: statistics, update RMS of the matrices, momentum (+ residual statistics; conv weights and vectors finish
 * here), apply of the matrices.  `tensors` / `items` are device tables built by the host (layout: neurosis_amd/csrc/came.hip
 * NkCameTensor, items as NkAfItem; nk_came_tensor_bytes() guards the mirror).  `state` holds, per tensor, m (the parameter's physical
 * layout) and R, C, Rr, Cr (matrices: [d0], [d1]; conv OIHW weights: [O][KH][I], [O][KW][I]) or v (vectors).  `decay` is the
 * decoupled weight-decay factor 1 - wd * (fixed_decay ? 1 : lr); `lr` the group's current learning rate. */
typedef struct NkCameArgs {
  float* master; const float* grad; void* shadow; float* state; float* ws;
  const void* tensors; const void* items;
  float* u2_part;       /* [nitems] partial sums of u^2 */
  float* mean_row;      /* per matrix: partial sums of R, then of Rr, one per 256-row strip */
  float* denom;         /* [ntensors] clip denominator max(1, rms(u) / clip_threshold) */
  unsigned* counters;   /* "blocks done" counters, one range per tensor; all zero before a step, all zero after it */
  int item_lo, item_hi, tensor_lo, tensor_hi;
  float beta1, beta2, beta3;
  float one_minus_beta1, one_minus_beta2, one_minus_beta3;   /* 1 - beta computed in double on the host, as the reference's `alpha=1.0 - beta` */
  float eps1, eps2, clip_threshold, lr, decay, grad_scale;
  int has_matrix;       /* the chunk holds at least one 2-D tensor (the two matrix-only passes are launched) */
} NkCameArgs;
long nk_came_tensor_bytes(void);
int nk_came_chunk(const NkCameArgs* args, void* stream);

/* Fused 8-bit blockwise AdamW (bitsandbytes' AdamW8bit algorithm; no reference counterpart) on the flat buffers, ONE launch per step.
 * Every parameter is cut into blocks of 256 consecutive elements (physical order; a parameter's last block may be short, blocks never
 * straddle parameters).  Block b keeps m and v as one byte each -- codes into the 256-entry dynamic maps qmap1 (signed, m) and qmap2
 * (unsigned, v) -- and one fp32 absmax each: m = qmap1[code1] * absmax1[b], v = qmap2[code2] * absmax2[b].  The step dequantizes, updates
 * m, v and p with the unquantized new moments, and requantizes to the nearest map entry (lowest index on a tie) of m / max|m| over the block.
 * Tensors with is8 == 0 (below min_8bit_size) keep fp32 m / v in m32 / v32 and take the plain AdamW step.  Layout of `tensors`:
 * neurosis_amd/csrc/adamw8bit.hip NkA8Tensor (nk_adamw8bit_tensor_bytes() guards the mirror); `blk_start` [ntensors + 1] holds each
 * tensor's first block (prefix sums of ceil(numel / 256)); codes of block b are bytes [256 b, 256 b + 256) of code1 / code2.
 * decay = 1 - lr * wd, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t and 1 - beta are computed in double on the host. */
typedef struct NkAdamW8bitArgs {
  float* master; const float* grad; void* shadow;
  unsigned char* code1; unsigned char* code2; float* absmax1; float* absmax2;
  float* m32; float* v32;
  const float* qmap1; const float* qmap2;
  const void* tensors; const int* blk_start;
  int ntensors, nblocks;
  float beta1, beta2, one_minus_beta1, one_minus_beta2, eps, lr, decay, bc1, bc2, grad_scale;
} NkAdamW8bitArgs;
long nk_adamw8bit_tensor_bytes(void);
int nk_adamw8bit_step(const NkAdamW8bitArgs* args, void* stream);

/* Frozen DreamSim ViT towers (neurosis_amd/csrc/vit.hip): what is not a transformer layer.
 * nk_vit_patchify: x fp32 NCHW [N, 3, H, W] (H, W multiples of p, p % 8 == 0) -> rows bf16 [N * (H/p) * (W/p), 3 p p], row = (n, py, px),
 * column = (c, ky, kx) -- nn.Conv2d's weight order, so the patch embedding is rows @ proj.weight.view(E, 3 p p)^T.  `affine` is a HOST array of
 * 8 floats {a_0, a_1, a_2, b_0, b_1, b_2, lo, hi}: each value is a_c * clamp(x, lo, hi) + b_c, product and sum rounded separately.
 * nk_vit_patchify_bwd is its adjoint: dx fp32 NCHW (+)= a_c * drows where lo <= x <= hi, zero where the forward clamped; accumulate = 1 adds to
 * dx.  One writer per pixel, no atomics.
 * nk_vit_tokens: tokens FP32 [N (Np + 1), E] (the towers' residual stream is fp32); row 0 of a sample = cls + pos[0], row 1 + i = patches row i + pos[1 + i] (cls [E], pos [Np + 1, E]
 * fp32, E % 8 == 0).  nk_vit_tokens_bwd: dpatches bf16 [N Np, E] = dtokens (bf16) without the cls rows.
 * nk_vit_add_ln, the seam between the fp32 stream x [M, E] and the bf16 GEMMs: x += branch (bf16 [M, E], or NULL) in place; then, unless gamma
 * is NULL, y = LayerNorm(x) gamma + beta as bf16 (y_f32 = 0) or fp32 (1) with mean / rstd [M] written; xb (or NULL) receives x rounded to bf16,
 * what nk_layernorm_bwd_dx reads in the backward.  E <= 2048.
 * nk_dreamsim_head_fwd: f fp32 [2, B, Dz] -> d [B] = 1 - cosine_similarity(z_0, z_1, eps), z_j = f_j / |f_j| - mean(f_j / |f_j|).
 * nk_dreamsim_head_bwd: df1 [B, Dz] = upstream_b * d d_b / d f[1] (f[0] gets no gradient).  fp32, fixed-order sums (nk_reduce.h). */
int nk_vit_patchify(const float* x, void* rows, const float* affine, int N, int H, int W, int p, void* stream);
int nk_vit_patchify_bwd(const void* drows, const float* x, float* dx, const float* affine, int N, int H, int W, int p, int accumulate, void* stream);
int nk_vit_tokens(const void* patches, const float* cls, const float* pos, void* tokens, int N, int Np, int E, void* stream);
int nk_vit_tokens_bwd(const void* dtokens, void* dpatches, int N, int Np, int E, void* stream);
int nk_vit_add_ln(float* x, const void* branch, const float* gamma, const float* beta, void* y, int y_f32, void* xb, float* mean, float* rstd, int M,
                  int E, float eps, void* stream);
 /* nk_vit_cls_head_fwd: the cls row of each sample (row n * sample_stride / E of the fp32 token matrix; sample_stride in elements) through the
 * final LayerNorm (gamma / beta fp32, or both NULL) and the head (W fp32 [nc, E] and bias, or W NULL and nc == E), all in fp32 -> out fp32
 * [N, nc]; mean / rstd [N] are written when there is a norm.  nk_vit_cls_head_bwd: dcls bf16 [N, E], the gradient w.r.t. the cls rows. E <= 2048. */
int nk_vit_cls_head_fwd(const void* tokens, long sample_stride, const float* gamma, const float* beta, const float* W, const float* bias, float* out,
                        float* mean, float* rstd, int N, int E, int nc, float eps, void* stream);
int nk_vit_cls_head_bwd(const float* dout, const void* tokens, long sample_stride, const float* gamma, const float* W, const float* mean,
                        const float* rstd, void* dcls, int N, int E, int nc, void* stream);
int nk_dreamsim_head_fwd(const float* f, float* d, int B, int Dz, float eps, void* stream);
int nk_dreamsim_head_bwd(const float* f, const float* upstream, float* df1, int B, int Dz, float eps, void* stream);

/* LitEma.forward (reference modules/ema.py:40-59) as one pass over the flat fp32 buffers (n % 4 == 0):
 * ema[i] -= one_minus_decay * (ema[i] - p[i]).  The decay schedule min(decay, (1+n)/(10+n)) is the host's. */
int nk_ema_flat(float* ema, const float* p, long n, float one_minus_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif
