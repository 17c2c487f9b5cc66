// Attention monitor (gfx950): per-head statistics of the softmax of q k^T / sqrt(hd), straight from
// the fused QKV tensor [B, S, 3, H, hd] (bf16).
//
// jm_attn_stats: per attention row (b, h, q) the entropy of its softmax (nats), its largest
// probability, the probability mass on the first n_cls keys (the CLS tokens) and its largest logit;
// per head the fp64 sums of the first three over the good rows, the largest logit of the good rows and
// the number of rows that are not good (a row is good when its entropy is finite).  The [S, S] scores
// never reach HBM: one workgroup of 4 waves owns a (b, h, 64-query tile), each wave 16 queries whose
// operands stay in registers, and streams the keys through LDS in 64-row tiles (the next tile's
// loads are in flight during the MFMAs of the current one; LDS rows are padded by 16 bytes like the
// tile-streamed attention kernels').
//
// The logits are EXACT: bf16 values widened to fp64 (exactly), multiplied and added by
// v_mfma_f64_16x16x4_f64 (a product of two bf16 values has 16 significant bits, so a sum of hd <= 128
// of them fits the 53 of an fp64 accumulator for any inputs whose exponents span less than 2^30), as
// S^T = K Q^T, so a lane holds 4 keys of ONE query per accumulator and the row reductions are two lane
// exchanges.  The bf16 MFMA with fp32 accumulation of the attention kernels was built and measured
// first (profiles/attn_stats.txt): it rounds the accumulator once per 32 products, which leaves a logit
// of N(0, 1) inputs off by several fp32 ulp and, through exp, the row's largest probability and CLS
// mass by up to 16 -- as far off as the fp32 torch composition, and outside the per-row bounds of
// tests/test_attn_stats_gpu.py, which only an exact logit meets.  The monitor runs once per layer at an
// evaluation, so it pays for fp64 (3 .. 4 x the time of that first kernel) and is still 4.6 .. 6.1 x faster than the composition.  The contraction index
// is dealt to the 4 lane groups in contiguous quarters of the head (group g: columns g hd / 4 ..), the
// same on both operands, so a lane reads its operands in 8-byte pieces; every head dim of
// jm_attn_head_dims is a multiple of 16, so no step is padded.  The scale 1 / sqrt(hd) is applied in
// fp64 to the finished dot product.
//
// Per row a running (m, l, t, c) = (max z, sum e, sum e (z - m), sum of e over the CLS keys) in fp64,
// with e = exp(z - m), rescaled when m moves: alpha = exp(m_old - m_new), l' = alpha l,
// t' = alpha (t + (m_old - m_new) l), c' = alpha c.  t is kept relative to m -- it equals
// sum e z - m l -- so that ENT = log l - t / l is a sum of two non-negative terms (l >= 1: the
// maximum's own e is exactly 1) instead of the difference m + log l - (sum e z) / l of two terms of
// the size of the largest logit.  PMAX = 1 / l, CLS = c / l, ZMAX = m; each is rounded to fp32 once.
// A logit of -inf (and a key beyond S) has e = 0 and adds nothing; a NaN or +inf logit makes l, and
// with it the row's ENT, NaN: the row is not good.
//
// Rows and keys beyond S are never branched around: their loads go through a buffer resource that
// ends at the batch element's last row and return zeros, padded keys are masked to -inf by a select,
// padded queries compute on zeros and are dropped where the row values are used.  No atomics: every
// workgroup writes its 5 fp64 partials to part[h][b][tile]; attn_stats_finish_kernel adds a head's
// partials in (b, tile) order with a fixed tree, so reruns are bit-identical.
#include "common.h"

#include <math.h>

namespace {

constexpr int LT = 64;  // queries per workgroup, keys per tile
constexpr int PC = 5;   // partials per workgroup: ENT_SUM, PMAX_SUM, CLS_SUM, ZMAX, BAD
constexpr int OOB = 0x7ffffff0;  // a byte offset beyond every buffer resource: the load returns zeros

typedef __attribute__((ext_vector_type(4))) double f64x4_t;
JM_DEVICE f64x4_t mfma(double a, double b, f64x4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// 4 bf16 values (two dwords) widened to fp64, exactly
JM_DEVICE void bf4_to_d(uint32_t lo, uint32_t hi, double* d) {
  d[0] = (double)__uint_as_float(lo << 16);
  d[1] = (double)__uint_as_float(lo & 0xffff0000u);
  d[2] = (double)__uint_as_float(hi << 16);
  d[3] = (double)__uint_as_float(hi & 0xffff0000u);
}

// range-checked loads (attention.hip): zeros past the end of [base, base + bytes)
JM_DEVICE __amdgpu_buffer_rsrc_t rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
JM_DEVICE uint4 bld16(__amdgpu_buffer_rsrc_t r, int byte_off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
JM_DEVICE uint2 bld8(__amdgpu_buffer_rsrc_t r, int byte_off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0);
  return make_uint2(v[0], v[1]);
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

JM_DEVICE double lane_xor_d(double v, int m) { return __shfl_xor(v, m, WAVE); }

template <int HD>
__global__ __launch_bounds__(256, 2) void attn_stats_kernel(const uint16_t* __restrict__ qkv, int B, int S, int H,
                                                            int n_cls, double scale, double* __restrict__ part,
                                                            float* __restrict__ rows_out) {
  constexpr int KS = lks<HD>(), KQ = HD / 4, NC = KQ / 4, CPR = HD / 8, NJ = lkp<HD>() / 32;
  static_assert(HD % 16 == 0, "a lane group's quarter of the head is read in 8-byte pieces");
  __shared__ __attribute__((aligned(16))) uint16_t Ks[LT * KS];
  __shared__ double red[4][PC];
  const int nq = (S + LT - 1) / LT;
  JM_DGUARD(S >= 1 && B >= 1 && H >= 1 && n_cls >= 0 && n_cls <= S && blockDim.x == 256 &&
            gridDim.x == (unsigned)(B * H * nq));
  const int bh = blockIdx.x / nq, qb = blockIdx.x - bh * nq;
  const int b = bh / H, h = bh - b * H;
  const int ts = 3 * H * HD;  // elements per token row; (S + 64) ts 2 < 2^31 is checked by the host
  const uint16_t* base = qkv + (long)b * S * ts;
  const __amdgpu_buffer_rsrc_t rq = rsrc(base + h * HD, (long)S * ts * 2),
                               rk = rsrc(base + (H + h) * HD, (long)S * ts * 2);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
  const int q = qb * LT + wave * 16 + l16;

  // the wave's 16 queries: B operand, query l16, this lane group's quarter of the head (zeros beyond S)
  double qd[KQ];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const uint2 v = bld8(rq, (q * ts + g * KQ + 4 * c) * 2);
    bf4_to_d(v.x, v.y, qd + 4 * c);
  }

  // key tile: 64 x HD / 8 16-byte chunks dealt over the 256 threads (hd 80: the third pass is half empty)
  uint4 kr[NJ];
  auto fetch = [&](int r0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = threadIdx.x + 256 * j, r = i / CPR, c = (i % CPR) * 8;
      const bool in = HD % 32 == 0 || i < LT * CPR;
      kr[j] = bld16(rk, in ? ((r0 + r) * ts + c) * 2 : OOB);
    }
  };

  double m = -INFINITY;              // running max of the row (the same in the 4 lanes of a query)
  double l = 0.0, t = 0.0, c = 0.0;  // this lane's share (keys g, g + 4, g + 8, g + 12 of every 16) at max m
  fetch(0);
  for (int k0 = 0; k0 < S; k0 += LT) {
    __syncthreads();  // the previous tile's operand reads are done
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = threadIdx.x + 256 * j, r = i / CPR, cc = (i % CPR) * 8;
      if (HD % 32 == 0 || i < LT * CPR) *reinterpret_cast<uint4*>(Ks + r * KS + cc) = kr[j];
    }
    __syncthreads();
    if (k0 + LT < S) fetch(k0 + LT);  // workgroup-uniform

    // accumulator layout of the f64 MFMA: register i of block kt is key k0 + 16 kt + g + 4 i, query l16
    double z[4][4];
    double mt = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f64x4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) {
        const uint2 v = *reinterpret_cast<const uint2*>(Ks + (kt * 16 + l16) * KS + g * KQ + 4 * cc);
        double kd[4];
        bf4_to_d(v.x, v.y, kd);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma(kd[j], qd[4 * cc + j], acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double v = k0 + kt * 16 + g + 4 * i < S ? acc[i] * scale : -INFINITY;
        z[kt][i] = v;
        mt = fmax(mt, v);  // a NaN is passed over here and caught by l below
      }
    }
    mt = fmax(mt, lane_xor_d(mt, 16));
    mt = fmax(mt, lane_xor_d(mt, 32));
    const double mn = fmax(m, mt);
    if (mn != m) {  // the max moved (always in the first tile): rescale what is held
      const double dm = m - mn;
      const double alpha = exp(dm);
      t = m > -INFINITY ? alpha * (t + dm * l) : 0.0;
      l *= alpha;
      c *= alpha;
      m = mn;
    }
    const bool cls_tile = k0 < n_cls;  // workgroup-uniform
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double d = z[kt][i] - m;
        const double e = exp(d);
        l += e;
        t += e > 0.0 ? e * d : 0.0;  // e = 0 (d = -inf, or exp underflow) adds 0, not 0 * inf
        if (cls_tile) c += k0 + kt * 16 + g + 4 * i < n_cls ? e : 0.0;
      }
    }
  }

  // the row: the 4 lanes of a query added in a symmetric order, so all 4 hold the same bits
  l += lane_xor_d(l, 16);
  l += lane_xor_d(l, 32);
  t += lane_xor_d(t, 16);
  t += lane_xor_d(t, 32);
  c += lane_xor_d(c, 16);
  c += lane_xor_d(c, 32);
  const float ent = (float)(log(l) - t / l);
  const float pmax = (float)(1.0 / l);
  const float cls = (float)(c / l);
  const bool real = q < S;
  const bool good = real && ent - ent == 0.f;  // finite
  if (rows_out && real) {
    const float v = g == 0 ? ent : g == 1 ? pmax : g == 2 ? cls : (float)m;
    rows_out[(((long)b * H + h) * S + q) * 4 + g] = v;
  }

  // workgroup partials: lanes 0..15 of each wave hold one row each; a fixed butterfly over them
  const bool mine = g == 0;
  double s0 = mine && good ? (double)ent : 0.0, s1 = mine && good ? (double)pmax : 0.0,
         s2 = mine && good ? (double)cls : 0.0, s3 = mine && good ? (double)(float)m : -INFINITY,
         s4 = mine && real && !good ? 1.0 : 0.0;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    s0 += lane_xor_d(s0, o);
    s1 += lane_xor_d(s1, o);
    s2 += lane_xor_d(s2, o);
    s3 = fmax(s3, lane_xor_d(s3, o));
    s4 += lane_xor_d(s4, o);
  }
  if (lane == 0) {
    red[wave][0] = s0;
    red[wave][1] = s1;
    red[wave][2] = s2;
    red[wave][3] = s3;
    red[wave][4] = s4;
  }
  __syncthreads();
  if (threadIdx.x < PC) {
    const int j = threadIdx.x;
    const double a0 = red[0][j], a1 = red[1][j], a2 = red[2][j], a3 = red[3][j];
    part[(((long)h * B + b) * nq + qb) * PC + j] = j == 3 ? fmax(fmax(a0, a1), fmax(a2, a3)) : (a0 + a1) + (a2 + a3);
  }
}

// one workgroup per head: thread i adds partials i, i + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void attn_stats_finish_kernel(const double* __restrict__ part, int n, double rows,
                                                                double* __restrict__ out) {
  __shared__ double red[256][PC];
  JM_DGUARD(n >= 1 && blockDim.x == 256);
  const int h = blockIdx.x, i0 = threadIdx.x;
  double a[PC] = {0.0, 0.0, 0.0, -INFINITY, 0.0};
  for (int i = i0; i < n; i += 256) {
    const double* p = part + ((long)h * n + i) * PC;
#pragma unroll
    for (int j = 0; j < PC; ++j) a[j] = j == 3 ? fmax(a[j], p[j]) : a[j] + p[j];
  }
#pragma unroll
  for (int j = 0; j < PC; ++j) red[i0][j] = a[j];
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (i0 < s) {
#pragma unroll
      for (int j = 0; j < PC; ++j) red[i0][j] = j == 3 ? fmax(red[i0][j], red[i0 + s][j]) : red[i0][j] + red[i0 + s][j];
    }
    __syncthreads();
  }
  if (i0 < PC) out[(long)h * JM_ATTN_STATS_COLS + i0] = red[0][i0];
  if (i0 == PC) out[(long)h * JM_ATTN_STATS_COLS + PC] = rows;
}

template <int HD>
void launch(const uint16_t* qkv, int B, int S, int H, int n_cls, double* part, float* rows_out, hipStream_t st) {
  const int nq = (S + LT - 1) / LT;
  hipLaunchKernelGGL(attn_stats_kernel<HD>, dim3(B * H * nq), dim3(256), 0, st, qkv, B, S, H, n_cls,
                     1.0 / sqrt((double)HD), part, rows_out);
}

}  // namespace

long jm_attn_stats_part(int B, int S, int H) {
  if (B < 1 || S < 1 || H < 1) return 0;
  return (long)B * H * ((S + LT - 1) / LT) * PC;
}

int jm_attn_stats(const void* qkv, int B, int S, int H, int hd, int n_cls, double* part, float* rows_out,
                  hipStream_t st) {
  if (!qkv || !part || B < 1 || S < 1 || H < 1 || n_cls < 0 || n_cls > S) return -1;
  if (reinterpret_cast<uintptr_t>(qkv) & 15) return -1;
  const long ts = 3L * H * hd;
  if (((long)S + LT) * ts * 2 >= OOB) return -1;  // byte offsets of a batch element are ints
  if ((long)B * H * ((S + LT - 1) / LT) > 0x7fffffffL) return -1;
  const uint16_t* p = static_cast<const uint16_t*>(qkv);
  switch (hd) {
    case 32: launch<32>(p, B, S, H, n_cls, part, rows_out, st); break;
    case 64: launch<64>(p, B, S, H, n_cls, part, rows_out, st); break;
    case 80: launch<80>(p, B, S, H, n_cls, part, rows_out, st); break;
    case 96: launch<96>(p, B, S, H, n_cls, part, rows_out, st); break;
    case 128: launch<128>(p, B, S, H, n_cls, part, rows_out, st); break;
    default: return -1;
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_attn_stats_finish(const double* part, int B, int S, int H, double* out, hipStream_t st) {
  if (!part || !out || B < 1 || S < 1 || H < 1) return -1;
  const long n = (long)B * ((S + LT - 1) / LT);
  if (n > 0x7fffffffL) return -1;
  hipLaunchKernelGGL(attn_stats_finish_kernel, dim3(H), dim3(256), 0, st, part, (int)n, (double)B * (double)S, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(attn_stats)
