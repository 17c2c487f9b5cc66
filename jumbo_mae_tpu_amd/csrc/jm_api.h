// The host interface of the kernel translation units: every jm_* entry point that bindings.cpp (or
// another translation unit) calls, and the argument structs that cross that boundary.  This header
// is the only place where they are declared -- default arguments included -- and every *.hip file
// and bindings.cpp include it (hipcc and g++), so a definition that drifts from its declaration
// fails to link and a struct has one layout everywhere.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "gemm_plan.h"  // GemmPlan and the EPI_* epilogue names (HIP-free, so that it compiles alone)

// Dense-output dropout applied by the residual kernels that consume the branch output y (ops/blocks.py
// Drops): the element at y + o (y's own element offset o) is kept with common.h drop_keep(seed, ioff + o),
// kept values scaled by 1 / keep.  seed null: no dropout.
struct JmDrop {
  const int64_t* seed;
  uint32_t thr;
  float scale;
  long ioff;
};

// Fused residual backward riding on the LayerNorm backward (layernorm.hip, LnResIO):
// for rows t >= T0, dy(b, t) = bf16(mask[b] * scale * dx(b, t)) at y/dy + b * yB + (t - T0) * yT,
// dscale += colsum(mask * dx * y), dbias += colsum(dy).  scale / mask / dscale / dbias may be null.
struct JmLnRes {
  const uint16_t* y;
  uint16_t* dy;
  long yB, yT;
  const float* scale;
  const float* mask;
  int T0;
  float* dscale;
  float* dbias;
  JmDrop drop;  // y's dropout (dy and dscale use the masked y)
};

// A weight-gradient launch (gemm_tn.hip jm_gemm_tn): n <= 4 independent TN problems
// G_p[N_p][K_p] (+)= A_p[M][N_p]^T . B_p[M][K_p] over the SAME M rows in one grid; tile0 = prefix
// sums of the problems' 256 x 256 output tiles (filled by jm_gemm_tn); out[p] = G_p (one split)
// or its [S][N_p K_p] fp32 partial slices.  With segmented rows a / b stay null (see TnSegs).
struct TnGroup {
  const uint16_t* a[4];
  const uint16_t* b[4];
  long lda[4], ldb[4];
  int N[4], K[4];
  float* out[4];
  int tile0[5];
  int n;
};

// Segmented M (the batched shared-jumbo-MLP weight gradient): the reduction rows are the
// concatenation of ``n`` separately allocated [rows, lda] / [rows, ldb] blocks (one per layer),
// read in place instead of being copied into one tensor first.  Problem p of a launch keeps its
// blocks at entries 32 p + i (so a segmented launch has at most 2 problems).
struct TnSegs {
  const uint16_t* a[64];
  const uint16_t* b[64];
  int rows;  // rows per block, multiple of the 32-row step
  int n;
};

// The 8-bit code of gelu'(h): q = round(GD_Q gelu') + GD_Z (common.h gd_code, where the choice is explained;
// ops/prims.py GD_Q / GD_Z mirror)
constexpr float GD_Q = 195.f;
constexpr int GD_Z = 34;

// Epilogue / output description of an NT GEMM launch (gemm.hip, bindings.cpp).
struct GemmEpi {
  const float* bias;     // [N] fp32 or null
  uint16_t* out;         // bf16 [M, ldo] (EPI_GELU_D: unused, see dq)
  long ldo;
  uint16_t* out2;        // EPI_GELU: gelu(out) bf16 [M, ldo]
  const uint16_t* aux;   // EPI_DGELU: pre-activation h bf16 [M, ldo]
  float* colpart;        // EPI_DGELU: per-row-tile column sums of out, [GemmPlan::colpart_rows][N] fp32
  float* part;           // EPI_PARTIAL: [splits][M][N] fp32 split-K partial products
  int splits;            // K splits (1 = none)
  // tail split (GemmPlan): the last, partly filled wave of output tiles is computed split-K into
  // the compact workspace tail[tail_S][tail_r][256][256] and finished by a reduce kernel that
  // applies the epilogue; t_begin / t_count restrict a launch to a tile range.  The caller gives
  // tail (GemmPlan::tail_floats floats); jm_gemm_nt fills splits, tail_S, t_begin and t_count
  float* tail;
  int tail_S;
  int t_begin;
  int t_count;
  // EPI_GELU_D: FF hidden dropout (ops/blocks.py Drops) -- gelu(h) times keep(seed, m * ldo + n) / keep
  // (common.h drop_keep), gelu'(h) times the keep bit alone (its 1 / keep travels as dqs); dseed null: none
  const int64_t* dseed;
  uint32_t dthr;
  float dscale;
  // gelu'(h) as 8-bit codes (common.h gd_code): EPI_GELU_D writes dq [M, ldo] u8, EPI_DMUL reads dqa and
  // decodes code q as (q - GD_Z) * dqs (dqs = keep scale / GD_Q)
  uint8_t* dq;
  const uint8_t* dqa;
  float dqs;
};

// ------------------------------------------------------------------------------ entry points
// int results: 0 (or a count, where the comment says so), < 0 for an unsupported shape or argument.
// jm_debug_line_<tu> (common.h JM_DEBUG_EXPORT, one per translation unit): the first failing soft
// device check's source line in the debug build (0 = none; reading clears it), always 0 in release.

// ---- layernorm.hip
// y (fp32 or bf16 [B T, D]), mean, rstd of the rows of a strided [B, T, D] x; y2: optional bf16 copy of y
int jm_layernorm_fwd(const float* x, long sB, long sT, int B, int T, int D, const float* gamma, const float* beta,
                     float eps, void* y, int out_bf16, float* mean, float* rstd, hipStream_t st, uint16_t* y2 = nullptr);
// dx (+ dres), dgamma, dbeta; res: the fused residual backward (JmLnRes); hx + beta: x rebuilt from the bf16 output
int jm_layernorm_bwd(const void* dy, int dy_bf16, const float* x, long sB, long sT, int B, int T, int D,
                     const float* mean, const float* rstd, const float* gamma, float* dx_ptr, long oB, long oT,
                     const float* dres, long rB, long rT, float* dgamma, float* dbeta, int accum_params, float* ws,
                     const JmLnRes* res, hipStream_t st, const uint16_t* hx = nullptr,
                     const float* beta = nullptr);
// workgroups of jm_layernorm_bwd (= rows of its partial workspace ws)
int jm_layernorm_bwd_blocks(int rows, int D);
// x1 = x + mask scale drop(y) on rows t >= R0, and h / mean / rstd = LayerNorm of x1's rows t >= T0
int jm_residual_ln_fwd(const float* x, long sB, long sT, const uint16_t* y, const float* scale, const float* mask,
                       float* x1, long oB, long oT, uint16_t* h, float* mean, float* rstd, int B, int T, int T0,
                       int D, const float* gamma, const float* beta, float eps, hipStream_t st, int R0 = 0,
                       JmDrop drop = JmDrop{nullptr, 0u, 1.f, 0});
int jm_debug_line_layernorm();

// ---- elementwise.hip
// a = gelu(h), bf16, n % 8 == 0
int jm_gelu_fwd(const uint16_t* h, uint16_t* a, long n, hipStream_t st);
// floats of the ws argument of the row-column kernels below (nacc column accumulators)
long jm_rowcol_ws_floats(int M, int N, int nacc);
// dh = da gelu'(h) (deriv: h already holds gelu'), bias_grad += colsum(dh)
int jm_gelu_bwd(const uint16_t* h, const uint16_t* da, uint16_t* dh, float* bias_grad, int M, int N, hipStream_t st,
                int deriv, float* ws);
// acc += colsum(x), x bf16 [M, N]
int jm_colsum_bf16(const uint16_t* x, float* acc, int M, int N, hipStream_t st, float* ws);
// out = x + mask scale drop(y)
int jm_residual_fwd(const float* x, long sB, long sT, int B, int T, int D, const uint16_t* y, const float* scale,
                    const float* mask, float* out, long oB, long oT, hipStream_t st, JmDrop drop);
// dy = bf16(mask scale dout) under y's dropout, dscale += colsum(mask dout y), dbias += colsum(dy)
int jm_residual_bwd(const float* dout, long dB, long dT, const uint16_t* y, const float* scale, const float* mask,
                    float* dscale, uint16_t* dy, int B, int T, int D, float* dbias, long yB, long yT, hipStream_t st,
                    JmDrop drop, float* ws);
// p[0, n) = 0
void jm_zero_f32(float* p, long n, hipStream_t st);
// g (+)= the sum of the S fp32 slices part[s][n]; store: g's old contents are ignored
int jm_splitk_reduce_add(const float* part, float* g, long n, int S, hipStream_t st, int store = 0);
// g += the column sums of the row-strided fp32 [rows, n] view x
int jm_colsum_add_f32(const float* x, long ld, int rows, long n, float* g, hipStream_t st);
// zero the n (offset, count) float ranges of base listed in the device array desc
int jm_zero_ranges(float* base, const long long* desc, int n, long long blocks, hipStream_t st);
// dst [C, R] = src [R, C]^T, bf16
int jm_transpose_bf16(const uint16_t* src, uint16_t* dst, int R, int C, hipStream_t st);
// the n transposes {src, dst, R, C, first tile, tiles along C} of the device array desc in one launch
int jm_transpose_bf16_batch(const long long* desc, int n, int tiles, hipStream_t st);
// out (bf16 [n / N, N]) = the sum of the S split-K slices + bias
int jm_splitk_reduce_bf16(const float* part, int S, long n, int N, const float* bias, uint16_t* out, hipStream_t st);
// out (fp32 [M, N]) = the sum of the S split-K slices + bias + add
int jm_splitk_reduce_f32(const float* part, int S, int M, int N, const float* bias, const float* add, long add_ld,
                         float* out, hipStream_t st);
int jm_debug_line_elementwise();
// debug build: one wave fails a soft check iff v != 0 (the test of the debug_lines() plumbing)
void jm_debug_selftest(int v, hipStream_t st);

// ---- attention.hip
// o, lse = softmax(q k^T / sqrt(hd)) v per head of the packed bf16 qkv [B, S, 3 H hd]; dseed: probability dropout
int jm_attn_fwd(const uint16_t* qkv, uint16_t* o, float* lse, int B, int S, int H, int hd, const int64_t* dseed,
                uint32_t dthr, float dscale, hipStream_t st);
// whole-sequence backward (-2 where jm_attn_tiled); dbias_part: optional per-sample column sums of dqkv
int jm_attn_bwd(const uint16_t* qkv, const uint16_t* o, const uint16_t* dO, const float* lse, uint16_t* dqkv, int B,
                int S, int H, int hd, float* dbias_part, const int64_t* dseed, uint32_t dthr, float dscale,
                hipStream_t st);
// tile-streamed backward (jm_attn_tiled shapes); delta: fp32 [B][H][S] workspace
int jm_attn_bwd_long(const uint16_t* qkv, const uint16_t* o, const uint16_t* dO, const float* lse, uint16_t* dqkv,
                     float* delta, int B, int S, int H, int hd, const int64_t* dseed, uint32_t dthr, float dscale,
                     hipStream_t st);
// longest sequence of the whole-sequence kernels
int jm_attn_max_seq();
// the head dims that have kernels (returns their count)
int jm_attn_head_dims(const int** dims);
// 1: (S, hd) runs on the tile-streamed kernels
int jm_attn_tiled(int S, int hd);
// 1: jm_attn_bwd can add the QKV bias gradient (dbias_part)
int jm_attn_fused_bias(int S, int hd);
// rows of jm_attn_bwd's dbias_part workspace
int jm_attn_bwd_part_rows(int B, int S, int hd);
// 1: the kernels of (S, hd) take a dropout seed
int jm_attn_dropout(int S, int hd);
int jm_debug_line_attention();

// ---- optim.hip (chunks: the device chunk table of the flat parameter buffer)
// out = the sum of squares of x
void jm_opt_sumsq(const float* x, const int* chunks, int nchunks, float* out, float* cpart, hipStream_t st);
// one AdamW step on the flat buffers (+ the bf16 shadow copy of p)
void jm_opt_adamw(float* p, const float* g, float* mu, float* nu, uint16_t* shadow, const int* chunks, int nchunks,
                  const float* meta, const float* hyper, const float* gnorm_sq, hipStream_t st);
// LAMB: moments, the update u and the per-tensor norms of p and u
void jm_opt_lamb_phase1(const float* p, const float* g, float* mu, float* nu, float* u, const int* chunks, int nchunks,
                        const float* meta, const float* hyper, const float* gnorm_sq, float* norms, float* cpart,
                        hipStream_t st);
// LARS: the per-tensor norms of p and g
void jm_opt_lars_norms(const float* p, const float* g, const int* chunks, int nchunks, const float* hyper,
                       const float* gnorm_sq, float* norms, float* cpart, hipStream_t st);
// LAMB / LARS: apply the update scaled by the per-tensor trust ratio
void jm_opt_apply_trust(float* p, const float* u_or_g, float* trace, uint16_t* shadow, const int* chunks, int nchunks,
                        const float* meta, const float* hyper, const float* norms, const float* gnorm_sq, int mode,
                        float momentum, float trust_coef, hipStream_t st);
// one SGD (momentum) step
void jm_opt_sgd(float* p, const float* g, float* trace, uint16_t* shadow, const int* chunks, int nchunks,
                const float* meta, const float* hyper, const float* gnorm_sq, float momentum, hipStream_t st);
// weight EMA on the rows of trainable segments: ema += ema_hyper[0] * (p - ema); n = elements of p and
// ema, nseg = rows of meta (ema_kernel)
void jm_opt_ema(const float* p, float* ema, const int* chunks, int nchunks, const float* meta, int nseg,
                const float* ema_hyper, long n, hipStream_t st);
// exchange p and ema on every row, bit for bit (+ the bf16 shadow copy of the new p) (ema_swap_kernel)
void jm_ema_swap(float* p, float* ema, uint16_t* shadow, const int* chunks, int nchunks, long n, hipStream_t st);
// norm monitor (optim/monitor.py): out[seg] = [sum g^2, sum p^2, sum (p - p_old)^2, max |g|, non-finite g,
// non-finite p, covered elements] over the rows of each segment, in fp64; non-finite values are counted and
// left out of the sums, frozen segments (meta[seg][3] == 0) report p only, p_old may be null (column 2 = 0).
// part: fp64 [nchunks, 7] chunk partials; out: fp64 [nseg, 7], every row written (no rows: zeros); n =
// elements of p, g and p_old (seg_stats_kernel, seg_stats_finish_kernel)
constexpr int JM_SEG_STATS_COLS = 7;
void jm_opt_seg_stats(const float* p, const float* g, const float* p_old, const int* chunks, int nchunks,
                      const float* meta, int nseg, long n, double* part, double* out, hipStream_t st);
int jm_debug_line_optim();

// ---- mae.hip
// out = the normalized p x p patches of the uint8 images, fp32
int jm_patchify_normalize(const uint8_t* img, float* out, int B, int H, int W, int p, hipStream_t st);
// out = the normalized patches ids[b, k] of each image, bf16
int jm_gather_patches(const uint8_t* img, const int* ids, long idsB, uint16_t* out, int B, int K, int H, int W, int p,
                      hipStream_t st);
// out = [class tokens; patch embeddings e + their position embeddings], fp32
int jm_embed_finish(const uint16_t* e, const float* pos, const int* ids, long idsB, const float* cls, float* out,
                    int B, int C, int K, int D, hipStream_t st);
// random-masking ids and mask from noise [R, N]: stable argsort, its inverse, their int32 copies
int jm_mask_ids(const float* noise, int R, int N, int keep, int64_t* shuffle, int64_t* restore, int* keep32,
                int* restore32, float* mask, hipStream_t st);
// decoder input: kept tokens / mask tokens back in image order + position embeddings
int jm_unshuffle_fwd(const uint16_t* y, const float* tok, const int* restore, long rsB, const float* pos, float* out,
                     int B, int C, int K, int N, int d, hipStream_t st);
// partial rows that jm_unshuffle_bwd writes to part
int jm_unshuffle_bwd_blocks(int B, int C, int N, int rows_per_block);
// its backward: dy for the kept tokens, per-block fp64 partial sums of the mask-token gradient
int jm_unshuffle_bwd(const float* dout, const int* restore, long rsB, uint16_t* dy, double* part, int B, int C, int K,
                     int N, int d, int rows_per_block, hipStream_t st);
// the patches of the mixup / cutmix of each image with image perm[b], bf16
int jm_mix_patches(const uint8_t* img, const int* perm, const float* prm, const int* box, uint16_t* out, int B, int H,
                   int W, int p, hipStream_t st);
// per-patch MSE of pred against the (norm_pix: per-patch normalized) image patches
int jm_patch_mse_fwd(const uint16_t* pred, long ldp, const uint8_t* img, float* mse, long rows, int N, int H, int W,
                     int p, int norm_pix, hipStream_t st);
int jm_patch_mse_bwd(const uint16_t* pred, long ldp, const uint8_t* img, const float* dmse, uint16_t* dpred, long rows,
                     int N, int H, int W, int p, int norm_pix, hipStream_t st);
int jm_debug_line_mae();

// ---- recon.hip
// reconstruction panels of pred [B*N, 3p^2] (bf16 or fp32, contiguous, (ph, pw, c) order) against the uint8
// images [B, 3, H, W]: recon = every patch painted from pred, paste / masked = the original bytes on visible
// patches and the recon bytes / the fill byte on masked ones (mask fp32, 1 = masked, image b's row at
// b * maskB: 0 = one shared [N] mask, N = per-sample), err fp32 [B, N] = per-patch mean of
// (x_clamped / 255 - orig / 255)^2 before rounding.  p = 16 on 4-byte aligned images with W % 4 == 0 moves
// words, any other even p bytes; -1 bad argument (odd p, H % p, W % p, maskB), -2 failed launch
int jm_recon(const void* pred, int pred_bf16, const uint8_t* img, const float* mask, long maskB, uint8_t* recon,
             uint8_t* paste, uint8_t* masked, float* err, int B, int H, int W, int p, int norm_pix, int fill,
             hipStream_t st);
int jm_debug_line_recon();

// ---- gemm.hip
// the plan of the launch C = A[M, K] . B[N, K]^T with epilogue epi (EPI_*) on this device, under
// jm_gemm_test_force: kernel family, tiles, grid, tail split, sizes of the tail and colpart buffers
GemmPlan jm_gemm_nt_plan(int M, int N, int K, int epi, long lda, int splits);
// that launch on the MFMA kernels, exactly as planned; ep: operands of the epilogue (GemmEpi)
int jm_gemm_nt(const GemmPlan& plan, const uint16_t* A, const uint16_t* B, long ldb, const GemmEpi& ep, hipStream_t st);
// numerics tests only: force a kernel path (0 = by shape)
void jm_gemm_test_force(int path, int rows);
int jm_debug_line_gemm();

// ---- gemm_tn.hip
// dynamic LDS bytes of the weight-gradient kernels
size_t jm_gemm_tn_smem();
// M split of a launch over grp's problems (N, K, n read): returns the 32-row steps per split (a
// multiple of 4), *S_out = the number of splits
int jm_gemm_tn_plan(const TnGroup& grp, int M, int* S_out);
// the launch: contiguous rows a / b (segs null) or the blocks of segs (M = segs->rows segs->n);
// S > 1: out[p] = the [S][N_p K_p] partial slices (the caller reduces them), S == 1: out[p] = G_p,
// accumulated, or stored with store != 0.  -1 shape, -2 operand rows of 4 GiB or more, -3 null output
int jm_gemm_tn(const TnGroup& grp, const TnSegs* segs, int M, int sps, int S, hipStream_t st, int store);
int jm_debug_line_gemm_tn();

// ---- dropout.hip (seed: int64 [1] on the device, thr = round(keep 65536), scale = 1 / keep)
// y = dropout(x), n % 8 == 0, bf16 or fp32
int jm_dropout_apply(const void* x, void* y, long n, int bf16, const int64_t* seed, uint32_t thr, float scale,
                     hipStream_t st);
// h null: g, gp masked in place; else g = gelu(h) m, gp = gelu'(h) m
int jm_gelu_drop(const uint16_t* h, uint16_t* g, uint16_t* gp, long n, const int64_t* seed, uint32_t thr, float scale,
                 hipStream_t st);
// p = softmax(z) over rows of S, pd = dropout(p)
int jm_softmax_dropout_fwd(const float* z, float* p, float* pd, long rows, int S, const int64_t* seed, uint32_t thr,
                           float scale, hipStream_t st);
int jm_softmax_dropout_bwd(const float* dpd, const float* p, float* dz, long rows, int S, const int64_t* seed,
                           uint32_t thr, float scale, hipStream_t st);
int jm_debug_line_dropout();

// ---- augment.hip
// random-resized-crop: the crop windows of src (table tab) resized to out [B, 3, S, S] uint8
int jm_rrc_resize(const uint8_t* src, const int64_t* tab, int B, int S, uint8_t* tmp, int tmp_rows_max, uint8_t* out,
                  hipStream_t st);
// window resize (the validation transform Resize -> CenterCrop): out [B, 3, S, S] uint8 = per image
// the S x S window of a larger resize, or 255 for a pad row.  tab: int64 [B, jm_window_tab()] --
// columns 0 .. 12 as jm_rrc_resize's (src offset, window rows / cols, window origin y0 / x0, image
// H / W, box i / j / h / w, flip, tmp offset), 13 / 14 the full resize's output rows / columns,
// 15 / 16 the window's origin (row, column) in that output, 17 the pad flag (augment.hip, top).
// tmp_rows_max 0: a batch of pad rows only (src and tmp are not read)
int jm_window_resize(const uint8_t* src, const int64_t* tab, int B, int S, uint8_t* tmp, int tmp_rows_max,
                     uint8_t* out, hipStream_t st);
// columns of its table
int jm_window_tab();
// the most filter taps per output pixel that the resize kernels take
int jm_rrc_kmax();
int jm_debug_line_augment();

// ---- augment_chain.hip
// uint32 words per image of jm_aug_chain's stats
int jm_aug_stat_words();
// doubles per slot of its chain records
int jm_aug_record_len();
// the RandAugment op chain of every image on the ping-pong buffers; returns the buffer with the result (0 / 1)
int jm_aug_chain(uint8_t* images, uint8_t* scratch, const double* chain, int B, int slots, int S, uint32_t* stats,
                 hipStream_t st);
// AugMix: out [B, 3, S, S] = the composite of orig with its W chain results (chains [B * W, 3, S, S],
// chain k of image b at b * W + k) by table float [B, W + 1]: weights and m, or (blended) the alphas
int jm_augmix_mix(const uint8_t* orig, const uint8_t* chains, const float* table, uint8_t* out, int B, int W, int S,
                  int blended, hipStream_t st);
// RandomErasing in place: table int64 [B, 5] = box i, j, eh, ew (eh 0: none) and the offset of its
// [3, eh, ew] bytes in fill; box_bytes_max: the batch's largest 3 eh ew (0: unknown, the largest possible)
int jm_erase_paste(uint8_t* images, const int64_t* table, const uint8_t* fill, long fill_len, int B, int S,
                   long box_bytes_max, hipStream_t st);
int jm_debug_line_augment_chain();

// ---- loss.hip (logits: bf16 or fp32 [B, L] rows ld elements apart; labels int64 [B]; perm int32 [B] and
// w, the device label weight, both or neither; smoothing in [0, 1); mode 0 = softmax CE, 1 = sigmoid BCE; -1 bad argument, -2 failed launch)
// loss fp32 [B], hit bytes [B, 2] (top-1, top-5 membership of the arg-max label set), lse fp32 [B, 2] (hi, lo)
int jm_cls_loss_fwd(const void* logits, int bf16, long ld, const int64_t* labels, const int* perm, const float* w,
                    double smoothing, int mode, int B, int L, float* loss, uint8_t* hit, float* lse, hipStream_t st);
// dlogits [B, L] (rows ldo apart, the dtype of logits) = dloss[b] times the gradient of row b's loss
int jm_cls_loss_bwd(const void* logits, int bf16, long ld, const int64_t* labels, const int* perm, const float* w,
                    double smoothing, int mode, int B, int L, const float* lse, const float* dloss, void* dlogits,
                    long ldo, hipStream_t st);
int jm_debug_line_loss();

// ---- distill.hip (z student / u teacher logits: both bf16 or both fp32, [B, L], rows ldz / ldu elements apart;
// temp > 0; mode 0 = soft (temperature-scaled KL), 1 = hard (CE against the teacher's arg-max, temp unused);
// -1 bad argument, -2 failed launch)
// kd fp32 [B], agree bytes [B] (arg-max z == arg-max u, lowest index on ties), lse fp32 [B, 4] = (hi, lo) pairs of
// lse(z / temp), lse(u / temp) (hard: lse(z), zeros), targ int32 [B] = arg-max u
int jm_kd_loss_fwd(const void* z, long ldz, const void* u, long ldu, int bf16, double temp, int mode, int B, int L,
                   float* kd, uint8_t* agree, float* lse, int* targ, hipStream_t st);
// dz [B, L] (rows ldo apart, the dtype of z) = dloss[b] times the gradient of row b's kd; u is read in soft mode
// only (may be null in hard mode), targ in hard mode only (may be null in soft mode)
int jm_kd_loss_bwd(const void* z, long ldz, const void* u, long ldu, int bf16, double temp, int mode, int B, int L,
                   const float* lse, const int* targ, const float* dloss, void* dz, long ldo, hipStream_t st);
int jm_debug_line_distill();

// ---- eval_report.hip (logits bf16 or fp32 [B, L], rows ld elements apart; labels int64 [B], -1 = padded row, other
// out-of-range labels clamped; mode 0 = ce (softmax confidence), 1 = bce (sigmoid); -1 bad argument, -2 failed launch)
// The int64 state, jm_eval_state_words(L, n_bins) words (-1: bad L / n_bins):
//   [0] rows (neither padded nor non-finite)  [1] non-finite rows  [2] padded rows
//   bins [n_bins, 3]: count, top-1 hits, sum of q = llrint(conf * 2^32)
//   count [L], hit1 [L], hit5 [L] per true class, predicted [L] per predicted class
//   confusion [L, L] (true x predicted), only while L <= JM_EVAL_MATRIX_MAX_L
#define JM_EVAL_SCALARS 3
#define JM_EVAL_MAX_BINS 64
#define JM_EVAL_MATRIX_MAX_L 4096
long jm_eval_state_words(int L, int n_bins);
// pred int32 [B] = arg-max (lowest index on ties), rank int32 [B] = classes ahead of the label (strictly larger,
// or equal at a lower index), conf fp32 [B] = probability of pred; padded and non-finite rows: -1, -1, 0
int jm_eval_rows(const void* logits, int bf16, long ld, const int64_t* labels, int mode, int B, int L, int* pred,
                 int* rank, float* conf, hipStream_t st);
// state += this batch; no atomics, one writer per state word (L + n_bins + 1 workgroups)
int jm_eval_accumulate(const int64_t* labels, const int* pred, const int* rank, const float* conf, int B, int L,
                       int n_bins, int64_t* state, hipStream_t st);
int jm_debug_line_eval_report();

// ---- batchnorm.hip (x: fp32 [B, J], rows ld >= J elements apart, any 4-byte-aligned base; gamma / beta / running
// statistics fp32 [J]; part: fp64 [jm_bn_chunks(B), 2, J] workspace; -1 bad argument, -2 failed launch)
// row chunks of a batch (= rows of part), rows per chunk, columns per workgroup
int jm_bn_chunks(int B);
int jm_bn_chunk_rows();
int jm_bn_block_cols();
// packed fp32 [2 J] = [mean, mean of squares] over the B rows
int jm_bn_stats(const float* x, long ld, int B, int J, double* part, float* packed, hipStream_t st);
// y (bf16 or fp32, rows ldy apart) = (x - mean) rstd gamma + beta with var = max(0, mean2 - mean^2) from packed;
// stats fp32 [2 J] = [mean, rstd]; running = momentum running + (1 - momentum) (mean, var), in place
int jm_bn_apply(const float* x, long ld, int B, int J, const float* packed, const float* gamma, const float* beta,
                double eps, double momentum, void* y, int y_bf16, long ldy, float* stats, float* running_mean,
                float* running_var, hipStream_t st);
// the same from the running statistics; writes y only
int jm_bn_apply_eval(const float* x, long ld, int B, int J, const float* running_mean, const float* running_var,
                     const float* gamma, const float* beta, double eps, void* y, int y_bf16, long ldy,
                     hipStream_t st);
// dbeta = colsum(dy), dgamma = colsum(dy xhat) (accum: added to them), packed_g fp32 [2 J] = gamma times both;
// dy bf16 or fp32, rows lddy apart
int jm_bn_bwd_reduce(const void* dy, int dy_bf16, long lddy, const float* x, long ld, int B, int J,
                     const float* stats, const float* gamma, double* part, float* dgamma, float* dbeta, int accum,
                     float* packed_g, hipStream_t st);
// dx (fp32, rows lddx apart) = rstd (gamma dy - packed_g[0] / n - xhat packed_g[1] / n), n = the global batch
int jm_bn_bwd_dx(const void* dy, int dy_bf16, long lddy, const float* x, long ld, int B, int J, const float* stats,
                 const float* gamma, const float* packed_g, double n, float* dx, long lddx, hipStream_t st);
int jm_debug_line_batchnorm();

// ---- knn.hip (q [Nq, D] / bank [Nb, D] bf16, 16-byte aligned rows ldq / ldb elements apart, D % 32 == 0,
// 1 <= k <= 64; self_idx int32 [Nq] or null: the bank row a query skips, -1 = none)
// idx int32 / sim fp32 [Nq, k]: per query the k largest dot products, sorted by (sim descending, bank index
// ascending); missing entries idx = -1, sim = -inf.  splits 0 = chosen from the shape, > 0 = that many
// contiguous bank slices; with more than one slice (jm_knn_splits) sidx / ssim [slices, Nq, k] are the scratch.
// The result does not depend on splits.
int jm_knn_splits(int Nq, int Nb, int splits);
int jm_knn_topk(const void* q, long ldq, const void* bank, long ldb, const int* self_idx, int Nq, int Nb, int D, int k,
                int splits, int* idx, float* sim, int* sidx, float* ssim, hipStream_t st);
// weighted vote over the lists: w_j = exp((sim_j - sim_0) / T) in fp64 (idx -1 ignored), class scores added in
// ascending j, ranked by (score descending, class id ascending).  pred int32 [Nq, 5] (-1 beyond the voted
// classes), hit1 / hit5 bytes [Nq] (a label of -1 never hits)
int jm_knn_vote(const int* idx, const float* sim, const int* bank_labels, const int* labels, double T, int Nq, int Nb,
                int k, int* pred, uint8_t* hit1, uint8_t* hit5, hipStream_t st);
int jm_debug_line_knn();

// ---- attn_stats.hip (qkv: bf16 [B, S, 3, H, hd] contiguous, 16-byte aligned, hd one of jm_attn_head_dims;
// 0 <= n_cls <= S; -1 bad argument or a batch element of 2 GiB or more, -2 failed launch)
// columns of the per-head table: sums of the rows' entropy / largest probability / CLS mass over the good rows
// (finite entropy), the largest logit of the good rows (-inf: none), the rows that are not good, B S
constexpr int JM_ATTN_STATS_COLS = 6;
// doubles of the workspace part
long jm_attn_stats_part(int B, int S, int H);
// part = per workgroup partials; rows_out (fp32 [B, H, S, 4] or null) = (entropy, largest probability, CLS mass,
// largest logit) of every row
int jm_attn_stats(const void* qkv, int B, int S, int H, int hd, int n_cls, double* part, float* rows_out,
                  hipStream_t st);
// out (fp64 [H, 6]) = the partials added per head in (b, tile) order with a fixed tree
int jm_attn_stats_finish(const double* part, int B, int S, int H, double* out, hipStream_t st);
int jm_debug_line_attn_stats();

// ---- attn_rollout.hip (qkv as for attn_stats.hip; r_in, r_out: fp32 [B, C, S] contiguous and distinct, 1 <= C <= 8;
// 0 <= alpha <= 1; -1 bad argument or a batch element of 2 GiB or more, -2 failed launch)
// floats of the workspace ws (16-byte aligned): (max, 1 / sum e) per attention row [B, H, S, 2], then the per-head
// partials [B, H, C, S]
long jm_attn_rollout_ws(int B, int S, int H, int C);
// r_out[b, c, k] = alpha r_in[b, c, k] + (1 - alpha) / H sum_h sum_q r_in[b, c, q] softmax_k(q k^T / sqrt(hd))[b, h, q, k]
int jm_attn_rollout_step(const void* qkv, int B, int S, int H, int hd, const float* r_in, int C, double alpha,
                         float* r_out, float* ws, hipStream_t st);
int jm_debug_line_attn_rollout();

// ---- feat_stats.hip (representation monitor; -1 bad argument, -2 failed launch; no atomics, reruns bit-identical)
// G fp64 [D, D] += sum over valid rows of x x^T, s fp64 [D] += sum over valid rows of x, in place.  x fp32 [n, D],
// rows ldx >= D elements apart, any D in 1..2^20; valid bytes [n] or null (a row with valid == 0 is selected out
// and may hold NaN).  Every product is the exact fp64 product of two fp32 values; an element is one chain in
// ascending row order that starts from the state: two calls equal one call on the concatenated rows bit for bit
// when the first call holds a multiple of 4 rows (the same MFMA steps run) or every partial sum is exact.  Only
// tiles with i <= j are computed, the mirror is written: G stays symmetric bit for bit.
int jm_feat_gram(const float* x, long ldx, const uint8_t* valid, int n, int D, double* G, double* s, hipStream_t st);
// e fp64 [Nq]: e_i = sum over bank rows j with bank_valid[j] != 0 (null: all) and j != self_idx[i] (null or -1:
// none) of exp(-2 t (1 - q_i . bank_j)); q / bank as for knn.hip (bf16, 16-byte aligned rows, D % 32 == 0), t > 0.
// part: fp64 [jm_feat_uniformity_segments(Nb), Nq] workspace, one sum per bank segment of fixed size, added in
// ascending order; splits (0 = one workgroup row per segment, else 1..1024) deals the segments to workgroups and
// never shows in e.
int jm_feat_uniformity_segments(int Nb);
int jm_feat_uniformity(const void* q, long ldq, const void* bank, long ldb, const int* self_idx,
                       const uint8_t* bank_valid, int Nq, int Nb, int D, double t, int splits, double* part, double* e,
                       hipStream_t st);
int jm_debug_line_feat_stats();

// ---- rope.hip (axial 2-D rotary position embedding, ops/rope.py; -1 bad argument, -2 failed launch; no atomics,
// reruns bit-identical)
// rotates, in place, the q and k thirds of the patch rows t >= n_cls of the contiguous bf16 or fp32 qkv
// [B, S, 3, heads, hd], hd % 16 == 0; the v third and the first n_cls rows of every sequence are neither read nor
// written.  Row t has patch index p = t - n_cls (pos null) or pos[b * posB + t - n_cls] (int32; posB 0 = one shared
// list) at coordinates (p / gw, p % gw); table fp32 [G, hd / 4, 2] = (cos, sin) of coord * theta^(-i / (hd / 4)),
// 0 <= p < G gw (the debug build soft-checks it; p is clamped into the table).  inverse: the transpose (sin negated)
int jm_rope_apply(void* qkv, int bf16, int B, int S, int heads, int hd, int n_cls, int gw, const float* table, int G,
                  const int* pos, long posB, int inverse, hipStream_t st);
int jm_debug_line_rope();

// ---- qknorm.hip (QK-norm: per-head RMSNorm of q and k, rope fused behind it, ops/qknorm.py; -1 bad argument,
// -2 failed launch; no atomics, no host sync, reruns bit-identical)
// qkv / dqkv: contiguous bf16 or fp32 [B, S, 3, heads, hd], hd in {32, 64, 80, 96, 128}; saved: [B, S, 2, heads, hd]
// of the same dtype; g_q, g_k: fp32 [hd], 16-byte aligned.  The v third is neither read nor written.  table / G /
// pos / posB / gw / n_cls: as in jm_rope_apply; table null = no rotation (the other rope arguments are then ignored).
// fwd: saved = the q|k bits of qkv; q|k of qkv = rotate(x r g), r = 1 / sqrt(mean(x^2) + 1e-6), rounded once
int jm_qknorm_fwd(void* qkv, void* saved, int bf16, int B, int S, int heads, int hd, const float* g_q,
                  const float* g_k, int n_cls, int gw, const float* table, int G, const int* pos, long posB,
                  hipStream_t st);
// bwd: the q|k thirds of dqkv (gradient of the normalised, rotated tensor) become the gradient of the pre-norm one,
// r recomputed from saved, fp64 arithmetic; dg fp32 [2, hd] = (dg_q, dg_k) is WRITTEN from the per-workgroup partials
// part fp64 [jm_qknorm_bwd_blocks(..), 2, hd] in workgroup order (a fixed tree; the grid depends on the shape only)
int jm_qknorm_bwd(void* dqkv, const void* saved, int bf16, int B, int S, int heads, int hd, const float* g_q,
                  const float* g_k, int n_cls, int gw, const float* table, int G, const int* pos, long posB,
                  double* part, float* dg, hipStream_t st);
int jm_qknorm_bwd_blocks(int B, int S, int heads, int hd);  // 0: unsupported shape
int jm_debug_line_qknorm();

// ---- swiglu.hip (the gate of the gated feed-forward, ops/swiglu.py; bf16; pre: contiguous [M, 2 Hs] = [gate | up],
// a / da: contiguous [M, Hs], every pointer 16-byte aligned, Hs % 8 == 0; seed null = no hidden dropout, else the
// keep bits of common.h drop_keep(seed, m Hs + c, thr), kept values times scale; -1 bad argument (Hs % 8, M <= 0, a
// null or unaligned pointer), -2 an operand of 4 GiB or more, -3 failed launch; no atomics, reruns bit-identical)
// a[m, c] = bf16(silu(pre[m, c]) pre[m, Hs + c] drop), fp32 arithmetic, one rounding
int jm_swiglu_fwd(const uint16_t* pre, uint16_t* a, int M, int Hs, const int64_t* seed, uint32_t thr, float scale,
                  hipStream_t st);
// dpre[m, c] = bf16(da drop u sigma (1 + g (1 - sigma))), dpre[m, Hs + c] = bf16(da drop silu(g)); bias_grad (fp32
// [2 Hs], may be null) += the column sums of the rounded dpre, through the partial rows ws (jm_swiglu_ws_floats
// floats; may be null with bias_grad null)
int jm_swiglu_bwd(const uint16_t* pre, const uint16_t* da, uint16_t* dpre, float* bias_grad, int M, int Hs,
                  const int64_t* seed, uint32_t thr, float scale, hipStream_t st, float* ws);
long jm_swiglu_ws_floats(int M, int Hs);  // 0: unsupported shape
int jm_debug_line_swiglu();
