// Representation monitor (gfx950): the fp64 Gram matrix of fp32 feature rows, and the uniformity
// sums of normalised bf16 rows.  No atomics anywhere; every output is a pure function of the inputs,
// so reruns are bit-identical.
//
// jm_feat_gram: G [D, D] += sum over valid rows of x x^T, s [D] += sum over valid rows of x, both
// fp64 and updated in place.  The rows are the contraction: x^T x = sum_r (row r)^T (row r), so both
// MFMA operands of a 4-row step are read the same way (lane l: row l >> 4, column l & 15 of its
// 16-column block), widened fp32 -> fp64 (exact) and multiplied and added by v_mfma_f64_16x16x4_f64;
// the product of two fp32 values has 48 significant bits, so nothing is rounded before the fp64
// accumulator.  One workgroup of 4 waves owns one 64 x 64 tile (i-block ti <= j-block tj) of G: wave w
// the 16 rows ti 64 + 16 w .. of it (4 accumulators, f64 C/D layout: column l & 15, row (l >> 4) +
// 4 reg).  The accumulators START from the tile of G and the rows are walked in ascending order in
// 32-row stages through LDS (the next stage's global loads are in flight during the MFMAs of the
// current one), so every element has one writer and one fixed chain, and two calls on two batches
// run the chain of one call on their concatenation: the very same MFMA steps when the first batch
// holds a multiple of 4 rows (bit-equal for any values); at another cut the 4 products of a step are
// grouped differently, which shows only if the partial sums round (how the f64 MFMA orders the
// 4 additions of one step is not documented and not relied on).  ti < tj also writes the mirror
// tile; a diagonal tile computes all of its 64 x 64 elements -- (i, j) and (j, i) run the same chain on commuted
// (exact) products, so G stays symmetric bit for bit -- and adds its 64 columns of s (wave 0, one
// column per lane, row by row).  Rows beyond n, columns beyond D and rows with valid == 0 are
// SELECTED to zero after the load (a masked row may hold NaN); their addresses are clamped into x.
// LDS rows are 80 floats apart: the 4 lane groups of an operand read (rows r .. r + 3) then fall
// into 4 different quarters of the 64 banks.
//
// jm_feat_uniformity: e[i] = sum over valid bank rows j != self_idx[i] of exp(-2 t (1 - s_ij)),
// s_ij = q_i . bank_j.  The scores are those of knn.hip -- the same staging (64-deep chunks of D,
// XOR-swizzled 128-B LDS rows), the same v_mfma_f32_16x16x32_bf16 chain per (query, bank row) pair --
// and are never stored: a workgroup of 4 waves owns 128 queries and walks bank SEGMENTS of 1024 rows
// (16 tiles of 64).  exp and the sums are fp64.  Inside a segment a lane adds its 4 columns of each
// tile in ascending order, tile after tile, and the 16 lanes of a query row are added by a fixed
// butterfly; the segment's sum goes to part[segment][query].  feat_unif_finish_kernel adds a
// query's segments in ascending order.  The segment size is a constant, so the summation tree
// depends on (Nq, Nb) alone: `splits` only deals the segments to blockIdx.y and never shows in e.
#include "common.h"

#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;
JM_DEVICE f64x4_t mfma64(double a, double b, f64x4_t c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------------------ Gram
constexpr int GT = 64;       // tile of G
constexpr int GR = 32;       // rows per stage
constexpr int GS = GT + 16;  // LDS row stride in floats
constexpr int GE = GR / 4;   // rows per thread per stage
constexpr int GD_MAX = 1 << 20;

__global__ __launch_bounds__(256, 2) void feat_gram_kernel(const float* __restrict__ x, long ldx,
                                                           const uint8_t* __restrict__ valid, int n, int D,
                                                           double* __restrict__ G, double* __restrict__ s) {
  __shared__ float sA[GR * GS];  // columns of the i-block
  __shared__ float sB[GR * GS];  // columns of the j-block
  const int T = (D + GT - 1) / GT;
  JM_DGUARD(n >= 1 && D >= 1 && ldx >= D && blockDim.x == 256 && (long)gridDim.x == (long)T * (T + 1) / 2);
  // blockIdx.x -> (ti, tj), ti <= tj: row ti of the triangle holds T - ti tiles
  int ti = 0, rest = blockIdx.x;
  while (rest >= T - ti) {
    rest -= T - ti;
    ++ti;
  }
  const int tj = ti + rest;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l16 = lane & 15, g = lane >> 4;
  const bool diag = ti == tj;

  // accumulators from G: block nb, register i is G[ti 64 + 16 w + g + 4 i][tj 64 + 16 nb + l16]
  const int gi0 = ti * GT + w * 16 + g, gj0 = tj * GT + l16;
  f64x4_t acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gi = gi0 + 4 * i, gj = gj0 + 16 * nb;
      acc[nb][i] = (gi < D && gj < D) ? G[(long)gi * D + gj] : 0.0;
    }
  const int sc = ti * GT + lane;  // the column of s of this lane (diagonal tile, wave 0)
  double ssum = (diag && w == 0 && sc < D) ? s[sc] : 0.0;

  // staging: thread t loads column t & 63 of rows (t >> 6) + 4 e of both blocks
  const int ca = ti * GT + lane, cb = tj * GT + lane;
  const bool ina = ca < D, inb = cb < D;
  const int cca = ina ? ca : D - 1, ccb = inb ? cb : D - 1;
  float ra[GE], rb[GE];
  bool rv[GE];
  auto gload = [&](int r0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < GE; ++e) {
      const int row = r0 + w + 4 * e;
      const int rc = row < n ? row : n - 1;
      rv[e] = row < n && (!valid || valid[rc] != 0);
      ra[e] = x[(long)rc * ldx + cca];
      rb[e] = x[(long)rc * ldx + ccb];
    }
  };

  gload(0);
  for (int r0 = 0; r0 < n; r0 += GR) {
    __syncthreads();  // the previous stage's operand reads are done
#pragma unroll
    for (int e = 0; e < GE; ++e) {
      sA[(w + 4 * e) * GS + lane] = (rv[e] && ina) ? ra[e] : 0.f;  // selected, not multiplied
      sB[(w + 4 * e) * GS + lane] = (rv[e] && inb) ? rb[e] : 0.f;
    }
    __syncthreads();
    if (r0 + GR < n) gload(r0 + GR);  // workgroup-uniform
#pragma unroll
    for (int kk = 0; kk < GR / 4; ++kk) {
      const int r = kk * 4 + g;
      const double a = (double)sA[r * GS + w * 16 + l16];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a, (double)sB[r * GS + nb * 16 + l16], acc[nb]);
    }
    if (diag && w == 0) {  // wave-uniform
#pragma unroll
      for (int r = 0; r < GR; ++r) ssum += (double)sA[r * GS + lane];
    }
  }

#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gi = gi0 + 4 * i, gj = gj0 + 16 * nb;
      if (gi < D && gj < D) {
        G[(long)gi * D + gj] = acc[nb][i];
        if (!diag) G[(long)gj * D + gi] = acc[nb][i];
      }
    }
  if (diag && w == 0 && sc < D) s[sc] = ssum;
}

// ------------------------------------------------------------------------------ uniformity
constexpr int QT = 128;   // queries per workgroup
constexpr int QW = 32;    // queries per wave
constexpr int BT = 64;    // bank rows per tile
constexpr int DK = 64;    // depth of a staged chunk
constexpr int SEG = 1024;  // bank rows per segment: the unit of the summation tree
constexpr int SPLITS_MAX = 1024;

JM_DEVICE f32x4_t mfma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// knn.hip's XOR swizzle of the 16-byte chunks of a 128-B row
JM_DEVICE int kswz(int row) {
  return ((row >> 2) & 1) | ((((row >> 2) ^ (row >> 3)) & 1) << 1) | (((row >> 1) & 1) << 2);
}
JM_DEVICE int kso(int row, int ch) { return row * DK + (((ch ^ kswz(row)) & 7) << 3); }

JM_DEVICE double lane_xor_d(double v, int m) { return __shfl_xor(v, m, WAVE); }

__global__ __launch_bounds__(256, 2) void feat_unif_kernel(const uint16_t* __restrict__ q, long ldq,
                                                           const uint16_t* __restrict__ bank, long ldb,
                                                           const int* __restrict__ self_idx,
                                                           const uint8_t* __restrict__ bank_valid, int Nq, int Nb,
                                                           int D, double c2t, int nseg, int per,
                                                           double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint16_t sQ[QT * DK];  // 16 KB
  __shared__ __attribute__((aligned(16))) uint16_t sB[BT * DK];  // 8 KB
  JM_DGUARD((D & 31) == 0 && D >= 32 && per >= 1 && nseg == (Nb + SEG - 1) / SEG && blockDim.x == 256 &&
            (long)gridDim.y * per >= nseg);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = blockIdx.x * QT;
  const int nch = (D + DK - 1) / DK;
  const int seg_begin = blockIdx.y * per;
  const int seg_end = seg_begin + per < nseg ? seg_begin + per : nseg;

  // accumulator layout: register j of block (m, n) is query w 32 + m 16 + fq 4 + j, bank column n 16 + fr
  int selfL[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = q0 + w * QW + m * 16 + fq * 4 + j;
      selfL[m][j] = (self_idx && row < Nq) ? self_idx[row] : -1;
      JM_DASSERT(selfL[m][j] >= -1 && selfL[m][j] < Nb);  // out of range: matches no bank row, recorded in the debug build
    }

  // staging as in knn_topk_kernel: rows past the end are clamped (their scores are masked / never
  // written), chunks past D are zero; every load is issued unconditionally from a valid address
  const int sch = t & 7, srow = t >> 3;  // + 32 e
  const uint16_t* qp[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = q0 + srow + 32 * e;
    qp[e] = q + (long)(row < Nq ? row : Nq - 1) * ldq;
  }
  uint4 rq[4], rb[2];
  bool rin = true;
  auto gload = [&](int tile0, int c) __attribute__((always_inline)) {
    rin = c * DK + sch * 8 < D;
    const int co = rin ? c * DK + sch * 8 : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) rq[e] = *reinterpret_cast<const uint4*>(qp[e] + co);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int row = tile0 + srow + 32 * e;
      rb[e] = *reinterpret_cast<const uint4*>(bank + (long)(row < Nb ? row : Nb - 1) * ldb + co);
    }
  };

  const int b_first = seg_begin * SEG;
  const int b_last = (long)seg_end * SEG < Nb ? seg_end * SEG : Nb;  // end of this workgroup's bank rows
  if (b_first < b_last) gload(b_first, 0);
  for (int seg = seg_begin; seg < seg_end; ++seg) {
    const int b_begin = seg * SEG;
    const int b_end = b_begin + SEG < Nb ? b_begin + SEG : Nb;
    double es[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) es[m][j] = 0.0;

    for (int tile0 = b_begin; tile0 < b_end; tile0 += BT) {
      bool bv[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = tile0 + n * 16 + fr;
        bv[n] = col < b_end && (!bank_valid || bank_valid[col] != 0);
      }
      f32x4_t acc[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

      for (int c = 0; c < nch; ++c) {
        __syncthreads();  // the previous chunk's fragment reads are done
        const uint32_t km = rin ? 0xffffffffu : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          *reinterpret_cast<uint4*>(&sQ[kso(srow + 32 * e, sch)]) =
              make_uint4(rq[e].x & km, rq[e].y & km, rq[e].z & km, rq[e].w & km);
#pragma unroll
        for (int e = 0; e < 2; ++e)
          *reinterpret_cast<uint4*>(&sB[kso(srow + 32 * e, sch)]) =
              make_uint4(rb[e].x & km, rb[e].y & km, rb[e].z & km, rb[e].w & km);
        __syncthreads();
        if (c + 1 < nch)
          gload(tile0, c + 1);
        else if (tile0 + BT < b_last)
          gload(tile0 + BT, 0);
        const int nk = (c * DK + 32 < D) ? 2 : 1;  // D % 64 == 32: the last chunk is half full
        for (int kk = 0; kk < nk; ++kk) {
          bf16x8_t a[2], b[4];
#pragma unroll
          for (int m = 0; m < 2; ++m)
            a[m] = *reinterpret_cast<const bf16x8_t*>(&sQ[kso(w * QW + m * 16 + fr, kk * 4 + fq)]);
#pragma unroll
          for (int n = 0; n < 4; ++n) b[n] = *reinterpret_cast<const bf16x8_t*>(&sB[kso(n * 16 + fr, kk * 4 + fq)]);
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = mfma(a[m], b[n], acc[m][n]);
        }
      }

      // this lane's 4 columns of each of its 8 query rows, in ascending column order
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const int col = tile0 + n * 16 + fr;
            const double ev = exp(c2t * (1.0 - (double)acc[m][n][j]));
            es[m][j] += (bv[n] && col != selfL[m][j]) ? ev : 0.0;  // selected: a masked score may be NaN
          }
    }

    // the 16 lanes of a query row: a fixed butterfly (every lane ends with the same bits)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double v = es[m][j];
        v += lane_xor_d(v, 1);
        v += lane_xor_d(v, 2);
        v += lane_xor_d(v, 4);
        v += lane_xor_d(v, 8);
        const int row = q0 + w * QW + m * 16 + fq * 4 + j;
        if (fr == 0 && row < Nq) part[(long)seg * Nq + row] = v;
      }
  }
}

// one thread per query: its segments in ascending order
__global__ __launch_bounds__(256) void feat_unif_finish_kernel(const double* __restrict__ part, int Nq, int nseg,
                                                               double* __restrict__ e) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= Nq) return;
  double v = 0.0;
  for (int sg = 0; sg < nseg; ++sg) v += part[(long)sg * Nq + row];
  e[row] = v;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int jm_feat_gram(const float* x, long ldx, const uint8_t* valid, int n, int D, double* G, double* s, hipStream_t st) {
  if (n == 0 && D >= 1 && G && s) return 0;
  if (!x || !G || !s || n < 0 || D < 1 || D > GD_MAX || ldx < D) return -1;
  const long T = (D + GT - 1) / GT;
  hipLaunchKernelGGL(feat_gram_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st, x, ldx, valid, n, D, G, s);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_feat_uniformity_segments(int Nb) { return Nb < 1 ? 0 : (Nb + SEG - 1) / SEG; }

int jm_feat_uniformity(const void* q, long ldq, const void* bank, long ldb, const int* self_idx,
                       const uint8_t* bank_valid, int Nq, int Nb, int D, double t, int splits, double* part, double* e,
                       hipStream_t st) {
  if (Nq == 0) return 0;
  if (!q || !bank || !part || !e || Nq < 0 || Nb < 1 || D < 32 || (D & 31) || !(t > 0.0) || splits < 0 ||
      splits > SPLITS_MAX)
    return -1;
  if (ldq < D || ldb < D || (ldq & 7) || (ldb & 7) || !aligned16(q) || !aligned16(bank)) return -1;
  const int nseg = jm_feat_uniformity_segments(Nb);
  int S = splits > 0 ? splits : SPLITS_MAX;
  S = S < nseg ? S : nseg;
  const int per = (nseg + S - 1) / S;
  const dim3 grid((Nq + QT - 1) / QT, (nseg + per - 1) / per);
  hipLaunchKernelGGL(feat_unif_kernel, grid, dim3(256), 0, st, static_cast<const uint16_t*>(q), ldq,
                     static_cast<const uint16_t*>(bank), ldb, self_idx, bank_valid, Nq, Nb, D, -2.0 * t, nseg, per,
                     part);
  hipLaunchKernelGGL(feat_unif_finish_kernel, dim3((Nq + 255) / 256), dim3(256), 0, st, part, Nq, nseg, e);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(feat_stats)
