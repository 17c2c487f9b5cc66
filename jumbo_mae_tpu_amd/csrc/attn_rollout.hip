// Attention maps (gfx950): one step of the CLS attention rollout, straight from the fused QKV tensor
// [B, S, 3, H, hd] (bf16).
//
// jm_attn_rollout_step: with p[b, h, q, k] = softmax_k((q . k) / sqrt(hd)) (no dropout),
//
//   r_out[b, c, k] = alpha r_in[b, c, k] + (1 - alpha) / H  sum_h sum_q r_in[b, c, q] p[b, h, q, k]
//
// for C <= 8 rows r_in[b, c, :] (fp32): a row vector times alpha I + (1 - alpha) mean_h P.  The [S, S]
// probabilities never reach memory; the workspace is B H S (C + 4) floats.
//
// Pass 1 (rollout_lse_kernel), per (b, h, 64-query tile): one workgroup of 4 waves, each wave 16 queries
// whose operand stays in registers, streams the keys through LDS in 64-row tiles (the next tile's loads
// are in flight during the MFMAs of the current one; LDS rows padded by 16 bytes) and keeps a running
// (max, sum e) per query in fp64.  The row's log-sum-exp is written as its two terms, (m, 1 / l) per row in
// fp64: pass 2 then forms p = exp(z - m) (1 / l), which is exact where the softmax is (uniform rows with S a
// power of two, one-hot rows) and does not round m + log l at the size of the largest logit.
//
// Pass 2 (rollout_acc_kernel), per (b, h, 64-key tile): each wave holds its 16 keys in registers and
// sweeps the query tiles through LDS.  Scores are recomputed with v_mfma_f32_16x16x32_bf16 as
// S = Q K^T, so a lane holds 4 queries of ONE key per accumulator; p is formed in fp64 and rounded to fp32
// once, and acc[c] += r_in[c][q] p runs on the VALU in fp32 (p is never rounded to bf16), with the tile's
// r_in rows and (m, 1 / l) in LDS.  The 4 lanes that share a key are added in a symmetric fixed order and write the
// fp32 partials part[b, h, c, k].
//
// Finish (rollout_finish_kernel): per output element the heads added in ascending h into 4 interleaved
// sums joined by a fixed tree, times (1 - alpha) / H, plus alpha r_in.
//
// The head loop is NOT folded into pass 2: with one workgroup per (b, h, key tile) the evaluation shapes
// (B 8, H 16, S 199 or 259: 512 and 640 workgroups) fill the 256 CUs, which a (b, key tile) grid (32 / 40)
// would not, and the partials are only B H C S floats.
//
// Numerics.  Every 32-column step of the contraction is one MFMA from a zero accumulator (the products
// of bf16 values are exact, the step's sum is rounded to fp32 once); the steps are added and scaled by
// 1 / sqrt(hd) in fp64, the same way in both passes, and max, exp, sum and 1 / l are fp64: what remains is
// the step roundings of the MFMA, one rounding of p and the fp32 accumulation over the queries (an all-fp32
// chain misses the bound of tests/test_attn_maps_gpu.py on short rows, profiles/attn_maps.txt).  The fp64
// exp, one per score, is the dominant VALU cost of pass 2 (a software sequence of some tens of fp64
// instructions against the 3 MFMAs and 8 fp32 fmas a score otherwise takes); a compensated fp32 exp -- the
// argument split into a high and a low part -- has not been built or measured against it and is the first
// thing to try when this kernel is tuned.  At
// hd = 80 the contraction runs over 96 columns; the 16 pad columns are zero on both operands (never
// loaded into the register fragments, zero-filled once in the LDS tile), as in attention.hip.
//
// Rows and keys beyond S are never loaded: the bf16 loads go through a buffer resource that ends at
// the batch element's last row and return zeros there, the fp32 loads are predicated.  Padded keys are
// masked to -inf in pass 1, padded queries have p = 0 in pass 2.  A logit of -inf has p = 0; a NaN or +inf
// logit makes its row's 1 / l NaN, and with it every partial of its (b, h) -- 0 * NaN is not filtered --
// so every r_out[b, :, :] is NaN and other images are untouched.  No atomics, every element has one
// writer, reruns are bit-identical.
#include "common.h"

#include <math.h>

namespace {

constexpr int LT = 64;           // queries / keys per tile
constexpr int CP = 8;            // rows of r_in the accumulation is built for (rows beyond C are zeros)
constexpr int OOB = 0x7ffffff0;  // a byte offset beyond every buffer resource: the load returns zeros

JM_DEVICE f32x4_t mfma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// range-checked loads (attn_stats.hip): zeros past the end of [base, base + bytes)
JM_DEVICE __amdgpu_buffer_rsrc_t rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
JM_DEVICE uint4 bld16(__amdgpu_buffer_rsrc_t r, int byte_off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// columns of the d contraction (hd rounded up to the MFMA depth) and the LDS row stride
template <int HD>
constexpr int lkp() {
  return (HD + 31) / 32 * 32;
}
template <int HD>
constexpr int lks() {
  return lkp<HD>() + 8;
}

// the 16 rows of a wave as MFMA fragments: row `row`, columns 32 kk + 8 g .. + 7 (zeros beyond S and in
// the pad columns of hd 80)
template <int HD>
JM_DEVICE void row_frags(bf16x8_t* f, __amdgpu_buffer_rsrc_t r, int row, int ts, int g) {
#pragma unroll
  for (int kk = 0; kk < lkp<HD>() / 32; ++kk) {
    const bool in = HD % 32 == 0 || 32 * kk + 8 * g < HD;
    f[kk] = __builtin_bit_cast(bf16x8_t, bld16(r, in ? (row * ts + 32 * kk + 8 * g) * 2 : OOB));
  }
}

// a 64 x HD tile: its 16-byte chunks dealt over the 256 threads (hd 80: the third pass is half empty)
template <int HD>
struct Tile {
  static constexpr int NJ = lkp<HD>() / 32, CPR = HD / 8, KS = lks<HD>();
  uint4 v[NJ];
  JM_DEVICE void fetch(__amdgpu_buffer_rsrc_t r, int r0, int ts) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = threadIdx.x + 256 * j, row = i / CPR, c = (i % CPR) * 8;
      const bool in = HD % 32 == 0 || i < LT * CPR;
      v[j] = bld16(r, in ? ((r0 + row) * ts + c) * 2 : OOB);
    }
  }
  JM_DEVICE void store(uint16_t* dst) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = threadIdx.x + 256 * j, row = i / CPR, c = (i % CPR) * 8;
      if (HD % 32 == 0 || i < LT * CPR) *reinterpret_cast<uint4*>(dst + row * KS + c) = v[j];
    }
  }
  // zero columns [HD, lkp) once, before the tile loop (its first barrier orders these stores)
  static JM_DEVICE void zero_pad(uint16_t* dst) {
    if constexpr (HD % 32 != 0) {
      constexpr int PCH = (lkp<HD>() - HD) / 8;
      for (int i = threadIdx.x; i < LT * PCH; i += 256)
        *reinterpret_cast<uint4*>(dst + (i / PCH) * KS + HD + (i % PCH) * 8) = make_uint4(0, 0, 0, 0);
    }
  }
};

JM_DEVICE bf16x8_t lds8(const uint16_t* p) { return *reinterpret_cast<const bf16x8_t*>(p); }

// a logit from the MFMA results of its 32-column steps, each accumulated from zero (one rounding per step):
// the steps are added and scaled in fp64
template <int KK>
JM_DEVICE double logit(const f32x4_t* acc, int i, double scale) {
  double s = (double)acc[0][i];
#pragma unroll
  for (int kk = 1; kk < KK; ++kk) s += (double)acc[kk][i];
  return s * scale;
}

// ---------------------------------------------------------------------------------------------- pass 1
template <int HD>
__global__ __launch_bounds__(256, 2) void rollout_lse_kernel(const uint16_t* __restrict__ qkv, int B, int S, int H,
                                                             double scale, double2* __restrict__ ml) {
  constexpr int KS = lks<HD>(), KK = lkp<HD>() / 32;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[LT * KS];
  const int nq = (S + LT - 1) / LT;
  JM_DGUARD(S >= 1 && B >= 1 && H >= 1 && blockDim.x == 256 && gridDim.x == (unsigned)(B * H * nq));
  const int bh = blockIdx.x / nq, qb = blockIdx.x - bh * nq;
  const int b = bh / H, h = bh - b * H;
  const int ts = 3 * H * HD;  // elements per token row; (S + 64) ts 2 < 2^31 is checked by the host
  const uint16_t* base = qkv + (long)b * S * ts;
  const long span = ((long)(S - 1) * ts + HD) * 2;  // up to the end of the head's columns in the last row
  const __amdgpu_buffer_rsrc_t rq = rsrc(base + h * HD, span), rk = rsrc(base + (H + h) * HD, span);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
  const int q = qb * LT + wave * 16 + l16;

  bf16x8_t qf[KK];
  row_frags<HD>(qf, rq, q, ts, g);

  double m = -INFINITY;  // running max of the row (the same in the 4 lanes of a query)
  double l = 0.0;        // this lane's share (keys 4 g .. 4 g + 3 of every 16) of sum e at max m
  Tile<HD>::zero_pad(Ks);
  Tile<HD> kr;
  kr.fetch(rk, 0, ts);
  for (int k0 = 0; k0 < S; k0 += LT) {
    __syncthreads();  // the previous tile's operand reads are done
    kr.store(Ks);
    __syncthreads();
    if (k0 + LT < S) kr.fetch(rk, k0 + LT, ts);  // workgroup-uniform

    // S^T = K Q^T: register i of block kt is key k0 + 16 kt + 4 g + i, query l16
    double z[4][4];
    double mt = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4_t acc[KK];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        acc[kk] = mfma(lds8(Ks + (kt * 16 + l16) * KS + 32 * kk + 8 * g), qf[kk], f32x4_t{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double v = k0 + kt * 16 + 4 * g + i < S ? logit<KK>(acc, i, scale) : -INFINITY;
        z[kt][i] = v;
        mt = fmax(mt, v);  // a NaN is passed over here and caught by l below
      }
    }
    mt = fmax(mt, __shfl_xor(mt, 16, WAVE));
    mt = fmax(mt, __shfl_xor(mt, 32, WAVE));
    const double mn = fmax(m, mt);
    if (mn != m) {  // the max moved: rescale what is held (from -inf: l = 0 stays 0)
      l *= exp(m - mn);
      m = mn;
    }
    const double mr = m == -INFINITY ? 0.0 : m;  // nothing but -inf so far: e = exp(-inf) = 0, not exp(NaN)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) l += exp(z[kt][i] - mr);
    }
  }
  // the 4 lanes of a query added in a symmetric order, so all 4 hold the same bits
  l += __shfl_xor(l, 16, WAVE);
  l += __shfl_xor(l, 32, WAVE);
  if (g == 0 && q < S) ml[((long)b * H + h) * S + q] = make_double2(m, 1.0 / l);
}

// ---------------------------------------------------------------------------------------------- pass 2
template <int HD>
__global__ __launch_bounds__(256, 2) void rollout_acc_kernel(const uint16_t* __restrict__ qkv, int B, int S, int H,
                                                             int C, double scale, const double2* __restrict__ ml,
                                                             const float* __restrict__ r_in,
                                                             float* __restrict__ part) {
  constexpr int KS = lks<HD>(), KK = lkp<HD>() / 32;
  __shared__ __attribute__((aligned(16))) uint16_t Qs[LT * KS];
  __shared__ __attribute__((aligned(16))) float Rs[CP][LT];  // r_in[c][q] of the query tile (zeros beyond C, S)
  __shared__ __attribute__((aligned(16))) double2 MLs[LT];  // m and 1 / l of its rows
  const int nk = (S + LT - 1) / LT;
  JM_DGUARD(S >= 1 && B >= 1 && H >= 1 && C >= 1 && C <= CP && blockDim.x == 256 &&
            gridDim.x == (unsigned)(B * H * nk));
  const int bh = blockIdx.x / nk, kb = blockIdx.x - bh * nk;
  const int b = bh / H, h = bh - b * H;
  const int ts = 3 * H * HD;
  const uint16_t* base = qkv + (long)b * S * ts;
  const long span = ((long)(S - 1) * ts + HD) * 2;
  const __amdgpu_buffer_rsrc_t rq = rsrc(base + h * HD, span), rk = rsrc(base + (H + h) * HD, span);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
  const int key = kb * LT + wave * 16 + l16;
  const double2* mlr = ml + ((long)b * H + h) * S;
  const float* rr = r_in + (long)b * C * S;

  bf16x8_t kf[KK];
  row_frags<HD>(kf, rk, key, ts, g);

  // the tile's fp32 rows: thread t holds r_in[c = t >> 6 and 4 + (t >> 6)][q0 + (t & 63)], threads 0..63 (m, 1 / l)
  const int tq = threadIdx.x & 63, tc = threadIdx.x >> 6;
  float r0v, r1v;
  double2 mlv;
  auto fetch_rows = [&](int q0) __attribute__((always_inline)) {
    const int qq = q0 + tq;
    r0v = qq < S && tc < C ? rr[(long)tc * S + qq] : 0.f;
    r1v = qq < S && tc + 4 < C ? rr[(long)(tc + 4) * S + qq] : 0.f;
    if (tc == 0) mlv = qq < S ? mlr[qq] : make_double2(0.0, 0.0);
  };

  float acc[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  Tile<HD>::zero_pad(Qs);
  Tile<HD> qr;
  qr.fetch(rq, 0, ts);
  fetch_rows(0);
  for (int q0 = 0; q0 < S; q0 += LT) {
    __syncthreads();  // the previous tile's reads are done
    qr.store(Qs);
    Rs[tc][tq] = r0v;
    Rs[tc + 4][tq] = r1v;
    if (tc == 0) MLs[tq] = mlv;
    __syncthreads();
    if (q0 + LT < S) {  // workgroup-uniform
      qr.fetch(rq, q0 + LT, ts);
      fetch_rows(q0 + LT);
    }
    // S = Q K^T: register i of block qt is query q0 + 16 qt + 4 g + i, key l16
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      f32x4_t s[KK];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        s[kk] = mfma(lds8(Qs + (qt * 16 + l16) * KS + 32 * kk + 8 * g), kf[kk], f32x4_t{0.f, 0.f, 0.f, 0.f});
      const int qo = qt * 16 + 4 * g;
      float p[4];  // fp64 up to here, rounded to fp32 once
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double2 mi = MLs[qo + i];
        const float e = (float)(exp(logit<KK>(s, i, scale) - mi.x) * mi.y);
        p[i] = q0 + qo + i < S ? e : 0.f;  // a padded query adds nothing, whatever its key holds
      }
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float4 rv = *reinterpret_cast<const float4*>(&Rs[c][qo]);
        acc[c] = __builtin_fmaf(rv.x, p[0], acc[c]);
        acc[c] = __builtin_fmaf(rv.y, p[1], acc[c]);
        acc[c] = __builtin_fmaf(rv.z, p[2], acc[c]);
        acc[c] = __builtin_fmaf(rv.w, p[3], acc[c]);
      }
    }
  }
  // the 4 lanes of a key added in a symmetric order (all 4 hold the same bits); lane group g writes rows g, g + 4
  float mine0 = 0.f, mine1 = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    float v = acc[c];
    v += __shfl_xor(v, 16, WAVE);
    v += __shfl_xor(v, 32, WAVE);
    if ((c & 3) == g) (c < 4 ? mine0 : mine1) = v;
  }
  if (key < S) {
    float* pr = part + ((long)b * H + h) * C * S + key;
    if (g < C) pr[(long)g * S] = mine0;
    if (g + 4 < C) pr[(long)(g + 4) * S] = mine1;
  }
}

// ---------------------------------------------------------------------------------------------- finish
// one thread per output element: heads h = j, j + 4, ... added in order into sum j, then a fixed tree
__global__ __launch_bounds__(256) void rollout_finish_kernel(const float* __restrict__ part,
                                                              const float* __restrict__ r_in, long n, int H, long CS,
                                                              float alpha, float w, float* __restrict__ r_out) {
  JM_DGUARD(n >= 1 && H >= 1 && CS >= 1 && blockDim.x == 256 && (long)gridDim.x * 256 >= n);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long b = i / CS, cs = i - b * CS;
  const float* p = part + b * H * CS + cs;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int h0 = 0; h0 < H; h0 += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (h0 + j < H) a[j] += p[(long)(h0 + j) * CS];
  }
  r_out[i] = alpha * r_in[i] + w * ((a[0] + a[1]) + (a[2] + a[3]));
}

template <int HD>
void launch(const uint16_t* qkv, int B, int S, int H, int C, const float* r_in, float* ws, hipStream_t st) {
  const int nt = (S + LT - 1) / LT;
  double2* ml = reinterpret_cast<double2*>(ws);
  float* part = ws + 4L * B * H * S;
  const double scale = 1.0 / sqrt((double)HD);
  hipLaunchKernelGGL(rollout_lse_kernel<HD>, dim3(B * H * nt), dim3(256), 0, st, qkv, B, S, H, scale, ml);
  hipLaunchKernelGGL(rollout_acc_kernel<HD>, dim3(B * H * nt), dim3(256), 0, st, qkv, B, S, H, C, scale, ml, r_in,
                     part);
}

}  // namespace

long jm_attn_rollout_ws(int B, int S, int H, int C) {
  if (B < 1 || S < 1 || H < 1 || C < 1) return 0;
  return (long)B * H * S * (C + 4);
}

int jm_attn_rollout_step(const void* qkv, int B, int S, int H, int hd, const float* r_in, int C, double alpha,
                         float* r_out, float* ws, hipStream_t st) {
  if (!qkv || !r_in || !r_out || !ws || r_in == r_out || B < 1 || S < 1 || H < 1 || C < 1 || C > CP) return -1;
  if (!(alpha >= 0.0 && alpha <= 1.0)) return -1;
  if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(ws) & 15)) return -1;
  const long ts = 3L * H * hd;
  if (((long)S + LT) * ts * 2 >= OOB) return -1;  // byte offsets of a batch element are ints
  if ((long)B * H * ((S + LT - 1) / LT) > 0x7fffffffL) return -1;
  const long n = (long)B * C * S;
  if ((n + 255) / 256 > 0x7fffffffL) return -1;
  const uint16_t* p = static_cast<const uint16_t*>(qkv);
  switch (hd) {
    case 32: launch<32>(p, B, S, H, C, r_in, ws, st); break;
    case 64: launch<64>(p, B, S, H, C, r_in, ws, st); break;
    case 80: launch<80>(p, B, S, H, C, r_in, ws, st); break;
    case 96: launch<96>(p, B, S, H, C, r_in, ws, st); break;
    case 128: launch<128>(p, B, S, H, C, r_in, ws, st); break;
    default: return -1;
  }
  if (hipGetLastError() != hipSuccess) return -2;
  hipLaunchKernelGGL(rollout_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     ws + 4L * B * H * S, r_in, n, H, (long)C * S, (float)alpha, (float)((1.0 - alpha) / H), r_out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(attn_rollout)
