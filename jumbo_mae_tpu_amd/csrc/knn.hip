// k-NN monitor (gfx950): fused similarity + running top-k, and the weighted vote.
//
// jm_knn_topk: for every query row the k bank rows with the largest dot product, as idx int32 /
// sim fp32 [Nq, k] sorted by (sim descending, bank index ascending); fewer than k eligible rows:
// the tail is idx = -1, sim = -inf.  The [Nq, Nb] scores are never stored: a workgroup of 4 waves
// owns 128 queries (32 per wave) and walks its bank slice in 64-row tiles; both operands stream
// through LDS in 64-deep chunks of D (rows of 128 B, 16-byte chunks XOR-swizzled as in the attention
// kernels; the next chunk's global loads are in flight during the MFMAs of the current one), the
// 32 x 64 scores of a wave come out of v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
//
// Each query's sorted list lives in REGISTERS: k <= 64 = one wave, so lane j of the owning wave holds
// entry j of each of its 32 queries (64 VGPRs).  Per tile every lane compares its 32 scores with the
// current k-th score of their rows (8 thresholds per lane, in the accumulator's layout); 8 ballots
// tell which rows have a candidate at all.  Only those rows are looked at again: the wave's scores go
// through a wave-private LDS tile so that lane c sees column c, and the candidates are inserted
// one by one in ascending bank index (a ballot gives the position, one lane shift makes room).
// A candidate displaces the k-th entry only if it is strictly greater, or equal with a smaller index.
//
// splits > 1: slice s of the bank (contiguous, a multiple of 64 rows) writes its lists to the
// scratch [splits][Nq][k]; knn_merge_kernel (one wave per query) inserts them in slice order with
// the same rule.  No atomics anywhere; the score of a (query, bank row) pair is the same MFMA chain
// whatever the slice, so the output is a pure function of the inputs and independent of splits.
//
// jm_knn_vote: one wave per query, lane j = neighbour j.  w_j = exp((sim_j - sim_0) / T) in fp64,
// class scores added in ascending j, classes ranked by (score descending, class id ascending) by
// a k x k comparison in registers; no [Nq, classes] tensor.
#include "common.h"

namespace {

constexpr int QT = 128;   // queries per workgroup
constexpr int QW = 32;    // queries per wave
constexpr int BT = 64;    // bank rows per tile
constexpr int DK = 64;    // depth of a staged chunk
constexpr int KMAX = 64;  // one list entry per lane
constexpr int SPLITS_MAX = 1024;

JM_DEVICE f32x4_t mfma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// the attention kernels' XOR swizzle of the 16-byte chunks of a 128-B row
JM_DEVICE int kswz(int row) {
  return ((row >> 2) & 1) | ((((row >> 2) ^ (row >> 3)) & 1) << 1) | (((row >> 1) & 1) << 2);
}
// element offset of 16-byte chunk ch of a row
JM_DEVICE int kso(int row, int ch) { return row * DK + (((ch ^ kswz(row)) & 7) << 3); }

JM_DEVICE float lane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// Insert candidate (v, ci) into the sorted list held one entry per lane (lanes >= k are not part of
// it).  False when it does not make the list.  All 64 lanes active; v, ci, k wave-uniform.
JM_DEVICE bool list_insert(float& ls, int& li, float v, int ci, int k, int lane) {
  const bool ahead = ls > v || (ls == v && li < ci);  // a prefix of the list: it is sorted
  const unsigned long long kmask = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
  const int p = __popcll(__ballot(ahead) & kmask);
  if (p >= k) return false;
  const float us = __shfl_up(ls, 1, WAVE);
  const int ui = __shfl_up(li, 1, WAVE);
  if (lane > p) {
    ls = us;
    li = ui;
  } else if (lane == p) {
    ls = v;
    li = ci;
  }
  return true;
}

__global__ __launch_bounds__(256, 2) void knn_topk_kernel(const uint16_t* __restrict__ q, long ldq,
                                                          const uint16_t* __restrict__ bank, long ldb,
                                                          const int* __restrict__ self_idx, int Nq, int Nb, int D,
                                                          int k, int per, int* __restrict__ oidx,
                                                          float* __restrict__ osim) {
  __shared__ __attribute__((aligned(16))) uint16_t sQ[QT * DK];  // 16 KB
  __shared__ __attribute__((aligned(16))) uint16_t sB[BT * DK];  // 8 KB
  __shared__ float sS[4][QW * BT];                               // 32 KB, one score tile per wave
  JM_DGUARD(k >= 1 && k <= KMAX && (D & 31) == 0 && per > 0 && per % BT == 0 && blockDim.x == 256);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = blockIdx.x * QT;
  const long sb = (long)blockIdx.y * per;
  const int b_begin = (int)(sb < Nb ? sb : Nb);
  const int b_end = (int)(sb + per < Nb ? sb + per : Nb);
  const int nch = (D + DK - 1) / DK;

  float ls[QW];
  int li[QW];
#pragma unroll
  for (int r = 0; r < QW; ++r) {
    ls[r] = -INFINITY;
    li[r] = -1;
  }
  // accumulator layout: register j of block (m, n) is query w 32 + m 16 + fq 4 + j, bank column n 16 + fr
  float thr[2][4];
  int selfL[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      thr[m][j] = -INFINITY;
      const int row = q0 + w * QW + m * 16 + fq * 4 + j;
      selfL[m][j] = (self_idx && row < Nq) ? self_idx[row] : -1;
    }

  // staging: Q tile 128 rows x 8 chunks = 4 per thread, bank tile 64 x 8 = 2 per thread; rows past
  // the end are clamped (their scores are masked / never written), chunks past D are zero
  const int sch = t & 7, srow = t >> 3;  // + 32 e
  const uint16_t* qp[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = q0 + srow + 32 * e;
    qp[e] = q + (long)(row < Nq ? row : Nq - 1) * ldq;
  }
  // every load is issued unconditionally from a valid address (a chunk past D re-reads the row's first
  // chunk and is zeroed at the LDS write): a select around the load would put a branch and a full wait at each
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

  if (b_begin < b_end) gload(b_begin, 0);
  for (int tile0 = b_begin; tile0 < b_end; tile0 += BT) {
    f32x4_t acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nch; ++c) {
      __syncthreads();  // the previous chunk's fragment reads are done
      const uint32_t km = rin ? 0xffffffffu : 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) *reinterpret_cast<uint4*>(&sQ[kso(srow + 32 * e, sch)]) = make_uint4(rq[e].x & km, rq[e].y & km, rq[e].z & km, rq[e].w & km);
#pragma unroll
      for (int e = 0; e < 2; ++e) *reinterpret_cast<uint4*>(&sB[kso(srow + 32 * e, sch)]) = make_uint4(rb[e].x & km, rb[e].y & km, rb[e].z & km, rb[e].w & km);
      __syncthreads();
      if (c + 1 < nch)
        gload(tile0, c + 1);
      else if (tile0 + BT < b_end)
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

    // mask what is not eligible, then the common path: compares and 8 ballots
    unsigned long long bal[2][4];
    unsigned long long any = 0ull;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bool pass = false;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const int col = tile0 + n * 16 + fr;
          const float v = (col < b_end && col != selfL[m][j]) ? acc[m][n][j] : -INFINITY;
          acc[m][n][j] = v;
          pass = pass || v > thr[m][j];
        }
        bal[m][j] = __ballot(pass);
        any |= bal[m][j];
      }
    if (any == 0ull) continue;  // wave-uniform

    // some row of this wave has a candidate: lane c gets column c of those rows
    float* S = sS[w];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[(m * 16 + fq * 4 + j) * BT + n * 16 + fr] = acc[m][n][j];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < QW; ++r) {
      const int m = r >> 4, g = (r & 15) >> 2, j = r & 3;
      if (((bal[m][j] >> (16 * g)) & 0xffffull) == 0ull) continue;  // wave-uniform
      const float sc = S[r * BT + lane];
      float th = lane_f(ls[r], k - 1);
      unsigned long long mm = __ballot(sc > th);
      while (mm) {  // ascending bank index
        const int c = __builtin_ctzll(mm);
        mm &= mm - 1ull;
        const float v = lane_f(sc, c);
        if (v > th && list_insert(ls[r], li[r], v, tile0 + c, k, lane)) th = lane_f(ls[r], k - 1);
      }
      if (fq == g) thr[m][j] = th;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  if (lane < k) {
#pragma unroll
    for (int r = 0; r < QW; ++r) {
      const int row = q0 + w * QW + r;
      if (row < Nq) {
        const long o = ((long)blockIdx.y * Nq + row) * k + lane;
        oidx[o] = li[r];
        osim[o] = ls[r];
      }
    }
  }
}

// one wave per query: the slices' lists, each sorted, inserted in slice order
__global__ __launch_bounds__(256) void knn_merge_kernel(const int* __restrict__ sidx, const float* __restrict__ ssim,
                                                        int Nq, int k, int splits, int* __restrict__ oidx,
                                                        float* __restrict__ osim) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Nq) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  float ls = -INFINITY;
  int li = -1;
  for (int s = 0; s < splits; ++s) {
    const long base = ((long)s * Nq + row) * k;
    const float cs = lane < k ? ssim[base + lane] : -INFINITY;
    const int ci = lane < k ? sidx[base + lane] : -1;
    for (int j = 0; j < k; ++j) {
      const int c = __builtin_amdgcn_readlane(ci, j);
      // the slice's list is sorted: after the first entry that fails, all fail
      if (c < 0 || !list_insert(ls, li, lane_f(cs, j), c, k, lane)) break;
    }
  }
  if (lane < k) {
    oidx[(long)row * k + lane] = li;
    osim[(long)row * k + lane] = ls;
  }
}

JM_DEVICE double lane_d(double v, int l) { return __shfl(v, l, WAVE); }

__global__ __launch_bounds__(256) void knn_vote_kernel(const int* __restrict__ idx, const float* __restrict__ sim,
                                                       const int* __restrict__ bank_labels,
                                                       const int* __restrict__ labels, double T, int Nq, int Nb,
                                                       int k, int* __restrict__ pred, uint8_t* __restrict__ hit1,
                                                       uint8_t* __restrict__ hit5) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Nq) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  int id = lane < k ? idx[(long)row * k + lane] : -1;
  JM_DASSERT(id >= -1 && id < Nb);
  if (id >= Nb) id = -1;  // out of range: ignored like an empty slot, recorded in the debug build
  const bool valid = id >= 0;
  const float s = lane < k ? sim[(long)row * k + lane] : 0.f;
  const float s0 = lane_f(s, 0);
  const int lab = valid ? bank_labels[id] : -1;
  const double wj = valid ? exp(((double)s - (double)s0) / T) : 0.0;
  // this neighbour's class score (added in ascending j) and whether it is the class's first neighbour
  double score = 0.0;
  bool rep = valid;
  for (int i = 0; i < k; ++i) {
    const double wi = lane_d(wj, i);
    const int labi = __shfl(lab, i, WAVE);
    const bool vi = __shfl((int)valid, i, WAVE) != 0;
    const bool same = vi && valid && labi == lab;
    if (same) score += wi;
    if (same && i < lane) rep = false;
  }
  int rank = 0;
  for (int i = 0; i < k; ++i) {
    const double si = lane_d(score, i);
    const int labi = __shfl(lab, i, WAVE);
    const bool ri = __shfl((int)rep, i, WAVE) != 0;
    if (ri && (si > score || (si == score && labi < lab))) ++rank;
  }
  const int nd = __popcll(__ballot(rep));
  if (rep && rank < 5) pred[(long)row * 5 + rank] = lab;
  if (lane < 5 && lane >= nd) pred[(long)row * 5 + lane] = -1;
  const int y = labels[row];
  const bool mine = rep && y >= 0 && lab == y;
  const bool h1 = __ballot(mine && rank == 0) != 0ull;
  const bool h5 = __ballot(mine && rank < 5) != 0ull;
  if (lane == 0) {
    hit1[row] = h1 ? 1 : 0;
    hit5[row] = h5 ? 1 : 0;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int jm_knn_splits(int Nq, int Nb, int splits) {
  if (Nq < 1 || Nb < 1 || splits < 0 || splits > SPLITS_MAX) return -1;
  if (splits > 0) return splits;
  // enough workgroups for two per CU, slices of at least 4 tiles
  const int qt = (Nq + QT - 1) / QT;
  int s = 512 / qt;
  const int cap = Nb / (4 * BT);
  s = s < cap ? s : cap;
  s = s < 64 ? s : 64;
  return s < 1 ? 1 : s;
}

int jm_knn_topk(const void* q, long ldq, const void* bank, long ldb, const int* self_idx, int Nq, int Nb, int D, int k,
                int splits, int* idx, float* sim, int* sidx, float* ssim, hipStream_t st) {
  if (Nq == 0) return 0;
  if (!q || !bank || !idx || !sim || Nq < 0 || Nb < 1 || D < 32 || (D & 31) || k < 1 || k > KMAX) return -1;
  if (ldq < D || ldb < D || (ldq & 7) || (ldb & 7) || !aligned16(q) || !aligned16(bank)) return -1;
  const int S = jm_knn_splits(Nq, Nb, splits);
  if (S < 1 || (S > 1 && (!sidx || !ssim))) return -1;
  const int per = (((Nb + S - 1) / S + BT - 1) / BT) * BT;
  const dim3 grid((Nq + QT - 1) / QT, S);
  hipLaunchKernelGGL(knn_topk_kernel, grid, dim3(256), 0, st, static_cast<const uint16_t*>(q), ldq,
                     static_cast<const uint16_t*>(bank), ldb, self_idx, Nq, Nb, D, k, per, S > 1 ? sidx : idx,
                     S > 1 ? ssim : sim);
  if (S > 1)
    hipLaunchKernelGGL(knn_merge_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, sidx, ssim, Nq, k, S, idx, sim);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_knn_vote(const int* idx, const float* sim, const int* bank_labels, const int* labels, double T, int Nq, int Nb,
                int k, int* pred, uint8_t* hit1, uint8_t* hit5, hipStream_t st) {
  if (Nq == 0) return 0;
  if (!idx || !sim || !bank_labels || !labels || !pred || !hit1 || !hit5 || Nq < 0 || Nb < 1 || k < 1 || k > KMAX ||
      !(T > 0.0))
    return -1;
  hipLaunchKernelGGL(knn_vote_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, idx, sim, bank_labels, labels, T, Nq, Nb, k,
                     pred, hit1, hit5);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(knn)
