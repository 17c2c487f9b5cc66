// Evaluation report (--eval-report): what the validation pass knows about the classifier's output
// beyond the loss and the two accuracies -- per-class accuracy, calibration bins and the confusion
// matrix -- accumulated on the GPU from the logits csrc/loss.hip reads.
//
// eval_rows_kernel: per row the arg-max class (lowest index on a tie), the label's rank under
// loss.hip's rule (strictly larger logits plus equal ones at a lower index) and the confidence, the
// probability of the arg-max class in fp64 rounded once to fp32 (ce: 1 / sum exp(z - max), bce:
// sigmoid(max)).  A padded row (label -1) and a non-finite row (a NaN, or a row maximum that is not
// finite) give pred = rank = -1, conf = 0.  Layout as in loss.hip: L <= WAVE_ROW_MAX: one wave per row,
// the row loaded once into 16 registers per lane (any alignment, any row stride); larger L: one
// 256-thread workgroup per row, each pass re-reading the row.  Wave butterflies + a fixed-order
// combine of the 4 wave results.
//
// eval_accumulate_kernel: adds a batch of such rows into the int64 state (jm_api.h has the layout).
// No atomics: every state word has ONE writer -- workgroup c owns true class c (its count / hit
// words, row c of the matrix, thread t the columns p % 256 == t) and predicted[c]; n_bins more
// workgroups own one bin each, the last one the three scalars.  Every workgroup scans the whole batch
// (an evaluation batch: a few hundred rows, L2 resident).  All sums are integers, so the order of the
// reductions, of the batches and of the ranks does not show in the result.
#include <limits.h>

#include "common.h"

namespace {

#define JM_INLINE __attribute__((always_inline))

constexpr int WAVE_ROW_MAX = 1024;  // 16 cached elements per lane
constexpr int ROW_CACHE = WAVE_ROW_MAX / WAVE;
constexpr int NT = 256;

// One row seen by its wave (cached) or its workgroup (re-read per pass), as in loss.hip
template <bool WG>
struct RowCache {
  float v[ROW_CACHE];
};
template <>
struct RowCache<true> {};

template <typename T, bool WG>
struct Row : RowCache<WG> {
  const T* p;
  int L, t;

  JM_DEVICE Row(const T* p_, int L_, int t_) : p(p_), L(L_), t(t_) {
    if constexpr (!WG) {
#pragma unroll
      for (int i = 0; i < ROW_CACHE; ++i) {
        const int c = t + WAVE * i;
        this->v[i] = c < L ? to_f<T>(p[c]) : 0.f;
      }
    }
  }
  template <typename F>
  JM_DEVICE void each(F f) const {
    if constexpr (WG) {
      for (int c = t; c < L; c += NT) f(c, to_f<T>(p[c]));
    } else {
#pragma unroll
      for (int i = 0; i < ROW_CACHE; ++i) {
        const int c = t + WAVE * i;
        if (c < L) f(c, this->v[i]);
      }
    }
  }
};

// Reductions over the row's threads (a wave, or the 4 waves of the workgroup), every thread gets the
// result.  All 64 lanes of each wave are active at every call.
template <typename V>
JM_DEVICE V wave_all_sum(V v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}

template <bool WG, typename V>
JM_DEVICE V row_sum(V v, double* sh) {
  v = wave_all_sum(v);
  if (WG) {
    V* s = reinterpret_cast<V*>(sh);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
  }
  return v;
}

// (value, index) pairs: the larger value, the lower index among equal values
JM_DEVICE void best_of(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

template <bool WG>
JM_DEVICE void row_argmax(float& v, int& i, double* sh) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m, WAVE);
    const int oi = __shfl_xor(i, m, WAVE);
    best_of(v, i, ov, oi);
  }
  if (WG) {
    float* sv = reinterpret_cast<float*>(sh);  // 4 values, then 4 indices
    int* si = reinterpret_cast<int*>(sh) + 4;
    if ((threadIdx.x & 63) == 0) {
      sv[threadIdx.x >> 6] = v;
      si[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = sv[0];
    i = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best_of(v, i, sv[w], si[w]);
    __syncthreads();
  }
}

// sigmoid without overflow
JM_DEVICE double sigmoid_d(float x) {
  const double e = exp(-fabs((double)x));
  const double r = 1.0 / (1.0 + e);
  return x >= 0.f ? r : e * r;
}

template <typename T, bool WG>
__global__ __launch_bounds__(256) void eval_rows_kernel(const T* __restrict__ z, long ld,
                                                        const int64_t* __restrict__ labels, int mode, int B, int L,
                                                        int* __restrict__ pred, int* __restrict__ rank,
                                                        float* __restrict__ conf) {
  __shared__ double sh[4];
  const int r = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (r >= B) return;  // wave-uniform (WG: workgroup-uniform), before the first reduction
  const int t = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const long y = (long)labels[r];
  int o_pred = -1, o_rank = -1;
  float o_conf = 0.f;
  if (y != -1) {  // uniform over the row's threads
    JM_DASSERT(y >= 0 && y < L);
    const int a = (int)(y < 0 ? 0 : (y >= L ? L - 1 : y));
    const T* zr = z + (long)r * ld;
    const Row<T, WG> row(zr, L, t);
    const float za = to_f<T>(zr[a]);

    // pass 1: NaNs, the arg-max pair, the label's rank (lower index wins a tie)
    float bv = -INFINITY;
    int bi = INT_MAX, nan = 0, ra = 0;
    row.each([&](int c, float x) JM_INLINE {
      nan |= (x != x) ? 1 : 0;
      if (x > bv) {  // ascending c: the first of equal values stays
        bv = x;
        bi = c;
      }
      ra += (x > za || (x == za && c < a)) ? 1 : 0;
    });
    row_argmax<WG>(bv, bi, sh);
    nan = row_sum<WG>(nan, sh);
    ra = row_sum<WG>(ra, sh);
    const bool finite = nan == 0 && bv > -INFINITY && bv < INFINITY;
    if (finite) {  // uniform
      double p;
      if (mode == 0) {
        double S = 0.0;
        row.each([&](int, float x) JM_INLINE { S += exp((double)x - (double)bv); });
        S = row_sum<WG>(S, sh);
        p = 1.0 / S;
      } else {
        p = sigmoid_d(bv);
      }
      o_pred = bi;
      o_rank = ra;
      o_conf = (float)p;
    }
  }
  if (t == 0) {
    pred[r] = o_pred;
    rank[r] = o_rank;
    conf[r] = o_conf;
  }
}

// ------------------------------------------------------------------------------ accumulation
struct RowIn {
  bool padded, finite;
  int a, p, rk, bin;
  long long q;
};

// row i as the accumulation sees it: labels clamped as in the row kernel; a row whose pred is outside
// [0, L) is a non-finite row; a confidence outside [0, 1] (never from the row kernel) counts as 0
JM_DEVICE RowIn row_in(const int64_t* labels, const int* pred, const int* rank, const float* conf, int i, int L,
                       int n_bins) {
  RowIn w;
  const long y = (long)labels[i];
  w.padded = y == -1;
  w.a = (int)(y < 0 ? 0 : (y >= L ? L - 1 : y));
  w.p = pred[i];
  w.finite = !w.padded && w.p >= 0 && w.p < L;
  w.rk = rank[i];
  const float cf = conf[i];
  const double c = (cf >= 0.f && cf <= 1.f) ? (double)cf : 0.0;
  w.q = __double2ll_rn(c * 4294967296.0);  // exact: conf is fp32
  const int b = (int)(c * (double)n_bins);   // exact product, c >= 0: truncation is floor
  w.bin = b < n_bins - 1 ? b : n_bins - 1;
  return w;
}

// sum over the workgroup, every thread gets the result; sh: 4 words
JM_DEVICE long long wg_sum(long long v, long long* sh) {
  v = wave_all_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(256) void eval_accumulate_kernel(const int64_t* __restrict__ labels,
                                                              const int* __restrict__ pred,
                                                              const int* __restrict__ rank,
                                                              const float* __restrict__ conf, int B, int L, int n_bins,
                                                              long long* __restrict__ state) {
  __shared__ long long sh[4];
  __shared__ int list[NT];  // the pred values of this class's rows in one chunk of 256 rows
  __shared__ int wcnt[4];
  const int t = (int)threadIdx.x;
  const int blk = (int)blockIdx.x;
  long long* bins = state + JM_EVAL_SCALARS;
  long long* cls = bins + 3L * n_bins;  // count, hit1, hit5, predicted: [L] each
  const int k5 = L < 5 ? L : 5;

  if (blk < L) {  // true class blk and predicted class blk
    const int c = blk;
    const bool matrix = L <= JM_EVAL_MATRIX_MAX_L;
    long long* mrow = cls + 4L * L + (long)c * L;
    long long n = 0, h1 = 0, h5 = 0, np = 0;
    for (int base = 0; base < B; base += NT) {  // uniform trip count: barriers inside
      const int i = base + t;
      bool mine = false;
      int p = 0;
      if (i < B) {
        const RowIn w = row_in(labels, pred, rank, conf, i, L, n_bins);
        mine = w.finite && w.a == c;
        p = w.p;
        if (mine) {
          n += 1;
          h1 += w.rk == 0 ? 1 : 0;
          h5 += (w.rk >= 0 && w.rk < k5) ? 1 : 0;
        }
        np += (w.finite && w.p == c) ? 1 : 0;
      }
      if (matrix) {
        // compact this chunk's pred values: ballot + prefix over the 4 waves
        const unsigned long long m = __ballot(mine);
        const int lane = t & 63, wv = t >> 6;
        if (lane == 0) wcnt[wv] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          off += w < wv ? wcnt[w] : 0;
          total += wcnt[w];
        }
        if (mine) list[off + __popcll(m & ((1ull << lane) - 1ull))] = p;
        __syncthreads();
        // thread t owns the columns p % 256 == t of row c: its own read-modify-writes, in program order
        for (int j = 0; j < total; ++j) {
          const int pj = list[j];
          if ((pj & (NT - 1)) == t) mrow[pj] += 1;
        }
        __syncthreads();  // list and wcnt are rewritten by the next chunk
      }
    }
    n = wg_sum(n, sh);
    h1 = wg_sum(h1, sh);
    h5 = wg_sum(h5, sh);
    np = wg_sum(np, sh);
    if (t == 0) {
      cls[c] += n;
      cls[(long)L + c] += h1;
      cls[2L * L + c] += h5;
      cls[3L * L + c] += np;
    }
  } else if (blk < L + n_bins) {  // one calibration bin
    const int b = blk - L;
    long long n = 0, h1 = 0, sq = 0;
    for (int i = t; i < B; i += NT) {
      const RowIn w = row_in(labels, pred, rank, conf, i, L, n_bins);
      if (w.finite && w.bin == b) {
        n += 1;
        h1 += w.rk == 0 ? 1 : 0;
        sq += w.q;
      }
    }
    n = wg_sum(n, sh);
    h1 = wg_sum(h1, sh);
    sq = wg_sum(sq, sh);
    if (t == 0) {
      bins[3 * b] += n;
      bins[3 * b + 1] += h1;
      bins[3 * b + 2] += sq;
    }
  } else {  // the scalars
    long long rows = 0, nonf = 0, pad = 0;
    for (int i = t; i < B; i += NT) {
      const RowIn w = row_in(labels, pred, rank, conf, i, L, n_bins);
      rows += w.finite ? 1 : 0;
      pad += w.padded ? 1 : 0;
      nonf += (!w.finite && !w.padded) ? 1 : 0;
    }
    rows = wg_sum(rows, sh);
    nonf = wg_sum(nonf, sh);
    pad = wg_sum(pad, sh);
    if (t == 0) {
      state[0] += rows;
      state[1] += nonf;
      state[2] += pad;
    }
  }
}

}  // namespace

long jm_eval_state_words(int L, int n_bins) {
  if (L < 1 || n_bins < 1 || n_bins > JM_EVAL_MAX_BINS) return -1;
  return JM_EVAL_SCALARS + 3L * n_bins + 4L * L + (L <= JM_EVAL_MATRIX_MAX_L ? (long)L * L : 0L);
}

int jm_eval_rows(const void* logits, int bf16, long ld, const int64_t* labels, int mode, int B, int L, int* pred,
                 int* rank, float* conf, hipStream_t st) {
  if (!logits || !labels || !pred || !rank || !conf || B < 1 || L < 1 || ld < L || (mode != 0 && mode != 1)) return -1;
  const bool wg = L > WAVE_ROW_MAX;
  const dim3 grid(wg ? B : (B + 3) / 4), block(256);
#define JM_LAUNCH(T, WG)                                                                                       \
  hipLaunchKernelGGL((eval_rows_kernel<T, WG>), grid, block, 0, st, static_cast<const T*>(logits), ld, labels, \
                     mode, B, L, pred, rank, conf)
  if (bf16) {
    if (wg) JM_LAUNCH(uint16_t, true); else JM_LAUNCH(uint16_t, false);
  } else {
    if (wg) JM_LAUNCH(float, true); else JM_LAUNCH(float, false);
  }
#undef JM_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_eval_accumulate(const int64_t* labels, const int* pred, const int* rank, const float* conf, int B, int L,
                       int n_bins, int64_t* state, hipStream_t st) {
  if (!labels || !pred || !rank || !conf || !state || B < 1 || jm_eval_state_words(L, n_bins) < 0) return -1;
  if ((long)L + n_bins + 1 > 0x7fffffffL) return -1;
  const dim3 grid((unsigned)(L + n_bins + 1)), block(NT);
  hipLaunchKernelGGL(eval_accumulate_kernel, grid, block, 0, st, labels, pred, rank, conf, B, L, n_bins,
                     reinterpret_cast<long long*>(state));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(eval_report)
