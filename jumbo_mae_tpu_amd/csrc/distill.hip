// Fused knowledge-distillation loss (ops/functional.py kd_loss): per row of student logits z and
// teacher logits u,
//   soft:  kd = T^2 sum_c q_c (log q_c - log p_c), q = softmax(u / T), p = softmax(z / T),
//          d kd / d z_c = T (p_c - q_c);
//   hard:  kd = -log softmax(z)_t, t = argmax_c u (lowest index among ties; T unused),
//          d kd / d z_c = softmax(z)_c - [c == t];
//   agree = (argmax z == argmax u), lowest index on ties in both.
// u takes no gradient.  The row math is fp64 as in loss.hip, for the reason given there (the rows are
// L2 / register resident: the wider arithmetic is not what the kernel waits for), and the
// log-sum-exps travel to the backward as fp32 (hi, lo) pairs.  Both operands go through the same
// operations in the same order, so u == z gives kd == 0 and dz == 0 exactly.
//
// Layout as in loss.hip (its row machinery is repeated here for two operands; loss.hip itself is
// left alone so that its kernels stay what they were): L <= WAVE_ROW_MAX: one wave per row (4 rows
// per workgroup), BOTH rows loaded once into 16 + 16 registers per lane (element lane + 64 i: every
// wave load is one contiguous run, any alignment, any row stride); larger L: one 256-thread
// workgroup per row, each pass re-reading both rows.  Wave butterflies + a fixed-order combination of
// the 4 wave results: no atomics, reruns are bit-identical.
#include "common.h"

namespace {

// on the per-element lambdas: the closure stays in registers
#define JM_INLINE __attribute__((always_inline))

constexpr int WAVE_ROW_MAX = 1024;  // 16 cached elements per lane and operand
constexpr int ROW_CACHE = WAVE_ROW_MAX / WAVE;

// One row pair seen by its wave (cached) or its workgroup (re-read per pass); a null u reads as z
template <bool WG>
struct PairCache {
  float vz[ROW_CACHE], vu[ROW_CACHE];
};
template <>
struct PairCache<true> {};

template <typename T, bool WG>
struct RowPair : PairCache<WG> {
  static constexpr int NT = WG ? 256 : WAVE;
  const T *pz, *pu;
  int L, t;

  JM_DEVICE RowPair(const T* pz_, const T* pu_, int L_, int t_) : pz(pz_), pu(pu_ ? pu_ : pz_), L(L_), t(t_) {
    if constexpr (!WG) {
#pragma unroll
      for (int i = 0; i < ROW_CACHE; ++i) {
        const int c = t + WAVE * i;
        this->vz[i] = c < L ? to_f<T>(pz[c]) : 0.f;
        this->vu[i] = c < L ? to_f<T>(pu[c]) : 0.f;
      }
    }
  }
  // f(class, student logit, teacher logit) for every element of this thread, ascending class
  template <typename F>
  JM_DEVICE void each(F f) const {
    if constexpr (WG) {
      for (int c = t; c < L; c += NT) f(c, to_f<T>(pz[c]), to_f<T>(pu[c]));
    } else {
#pragma unroll
      for (int i = 0; i < ROW_CACHE; ++i) {
        const int c = t + WAVE * i;
        if (c < L) f(c, this->vz[i], this->vu[i]);
      }
    }
  }
};

// Reductions over the row's threads, every thread gets the result.  All 64 lanes of each wave are
// active at every call (a wave leaves only as a whole, before the first one).
JM_DEVICE double wave_all_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}

template <bool WG>
JM_DEVICE double row_sum(double v, double* sh) {
  v = wave_all_sum(v);
  if (WG) {
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
  }
  return v;
}

// (largest value, its lowest index): a total order on NaN-free rows, so the result does not depend
// on the order of the combination.  A thread without elements holds (-inf, NO_CLASS) and loses to
// every thread with one, NaN rows included: the index that comes out is always a class of the row.
constexpr int NO_CLASS = 0x7fffffff;
struct ArgMax {
  float v;
  int i;
};
JM_DEVICE ArgMax arg_better(ArgMax a, ArgMax b) {
  return (b.i != NO_CLASS && (a.i == NO_CLASS || b.v > a.v || (b.v == a.v && b.i < a.i))) ? b : a;
}

template <bool WG>
JM_DEVICE ArgMax row_argmax(ArgMax a, double* sh) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    ArgMax o;
    o.v = __shfl_xor(a.v, m, WAVE);
    o.i = __shfl_xor(a.i, m, WAVE);
    a = arg_better(a, o);
  }
  if (WG) {
    ArgMax* s = reinterpret_cast<ArgMax*>(sh);  // 4 x 8 bytes
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
    __syncthreads();
    a = arg_better(arg_better(s[0], s[1]), arg_better(s[2], s[3]));
    __syncthreads();
  }
  return a;
}

// the row of this wave / workgroup, -1 past the batch (wave-uniform)
template <bool WG>
JM_DEVICE int row_index(int B) {
  const int r = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  return r < B ? r : -1;
}

// (x - m) / T, the argument of every exponential: one subtraction and one division, the same for
// both operands
JM_DEVICE double scaled(float x, float m, double T) {
#pragma clang fp contract(off)
  return ((double)x - (double)m) / T;
}

JM_DEVICE void put_pair(float* p, double v) {
  const float hi = (float)v;
  p[0] = hi;
  p[1] = (float)(v - (double)hi);
}

// One rounding from fp64 to the output type.  bf16: through an fp32 rounded to odd (the truncated
// value with the sticky bit in its last place), whose 24 bits make the final round-to-nearest-even
// the correctly rounded one; NaN and infinities pass through.
template <typename T> JM_DEVICE T from_d(double v);
template <> JM_DEVICE float from_d<float>(double v) { return (float)v; }
template <> JM_DEVICE uint16_t from_d<uint16_t>(double v) {
  float f = (float)v;
  const double back = (double)f;
  if (back != v && back - back == 0.0 && v == v) {  // inexact, finite
    uint32_t b = __float_as_uint(f);
    if (fabs(back) > fabs(v)) b -= 1;  // towards zero (f != 0: |f| > |v| >= 0)
    f = __uint_as_float(b | 1u);
  }
  return f2bf(f);
}

// mode 0 soft, 1 hard.  lse4 [B, 4]: soft (lse(z / T) hi, lo, lse(u / T) hi, lo), hard (lse(z) hi, lo, 0, 0)
template <typename T, bool WG>
__global__ __launch_bounds__(256) void kd_loss_fwd_kernel(const T* __restrict__ z, long ldz, const T* __restrict__ u,
                                                          long ldu, double temp, int mode, int B, int L,
                                                          float* __restrict__ kd, uint8_t* __restrict__ agree,
                                                          float* __restrict__ lse4, int* __restrict__ targ) {
  __shared__ double sh[4];
  const int r = row_index<WG>(B);
  if (r < 0) return;
  const int t = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const T* zr = z + (long)r * ldz;
  const RowPair<T, WG> row(zr, u + (long)r * ldu, L, t);

  // pass 1: both arg-maxima (ascending classes per thread: a strict > keeps the lowest index)
  ArgMax az = {-INFINITY, NO_CLASS}, au = {-INFINITY, NO_CLASS};
  row.each([&](int c, float x, float y) JM_INLINE {
    if (x > az.v || az.i == NO_CLASS) az = ArgMax{x, c};
    if (y > au.v || au.i == NO_CLASS) au = ArgMax{y, c};
  });
  az = row_argmax<WG>(az, sh);
  au = row_argmax<WG>(au, sh);

  double l, lz, lu = 0.0;
  if (mode == 0) {
    // pass 2: S_z = sum exp(a), S_u = sum exp(b), W = sum exp(b) (b - a) with a = (z - max z) / T,
    // b = (u - max u) / T; then sum_c q_c (log q_c - log p_c) = W / S_u - (log S_u - log S_z)
    double Sz = 0.0, Su = 0.0, W = 0.0;
    row.each([&](int, float x, float y) JM_INLINE {
      const double a = scaled(x, az.v, temp), b = scaled(y, au.v, temp);
      const double eb = exp(b);
      Sz += exp(a);
      Su += eb;
      W += eb * (b - a);
    });
    Sz = row_sum<WG>(Sz, sh);
    Su = row_sum<WG>(Su, sh);
    W = row_sum<WG>(W, sh);
    const double logSz = log(Sz), logSu = log(Su);
    l = temp * temp * (W / Su - (logSu - logSz));
    lz = (double)az.v / temp + logSz;
    lu = (double)au.v / temp + logSu;
  } else {
    double S = 0.0;
    row.each([&](int, float x, float) JM_INLINE { S += exp((double)x - (double)az.v); });
    S = row_sum<WG>(S, sh);
    const double logS = log(S);
    // lse - z_t = log S + (m - z_t), as log_softmax has it (thread 0 holds a class of the row: it
    // owns class 0)
    l = t == 0 ? logS + ((double)az.v - (double)to_f<T>(zr[au.i])) : 0.0;
    lz = (double)az.v + logS;
  }
  if (t == 0) {
    kd[r] = (float)l;
    agree[r] = az.i == au.i ? 1 : 0;
    targ[r] = au.i;
    put_pair(lse4 + 4 * (long)r, lz);
    put_pair(lse4 + 4 * (long)r + 2, lu);
  }
}

// u is null in hard mode (the row pair then reads z twice; the teacher enters through targ)
template <typename T, bool WG>
__global__ __launch_bounds__(256) void kd_loss_bwd_kernel(const T* __restrict__ z, long ldz, const T* __restrict__ u,
                                                          long ldu, double temp, int mode, int B, int L,
                                                          const float* __restrict__ lse4, const int* __restrict__ targ,
                                                          const float* __restrict__ dloss, T* __restrict__ dz,
                                                          long ldo) {
  const int r = row_index<WG>(B);
  if (r < 0) return;
  const int t = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const RowPair<T, WG> row(z + (long)r * ldz, u ? u + (long)r * ldu : nullptr, L, t);
  T* d = dz + (long)r * ldo;
  const double gl = (double)dloss[r];
  const float* ls = lse4 + 4 * (long)r;
  const double lz = (double)ls[0] + (double)ls[1];
  if (mode == 0) {
    const double lu = (double)ls[2] + (double)ls[3];
    const double s = gl * temp;
    row.each([&](int c, float x, float y) JM_INLINE {
      d[c] = from_d<T>(s * (exp((double)x / temp - lz) - exp((double)y / temp - lu)));
    });
  } else {
    const int tc = targ[r];
    row.each([&](int c, float x, float) JM_INLINE {
      d[c] = from_d<T>(gl * (exp((double)x - lz) - (c == tc ? 1.0 : 0.0)));
    });
  }
}

bool bad_args(const void* z, long ldz, const void* u, long ldu, double temp, int mode, int B, int L) {
  return !z || B < 1 || L < 1 || ldz < L || (u && ldu < L) || (mode != 0 && mode != 1) || !(temp > 0.0) ||
         !(temp <= 1.7976931348623157e308);
}

}  // namespace

int jm_kd_loss_fwd(const void* z, long ldz, const void* u, long ldu, int bf16, double temp, int mode, int B, int L,
                   float* kd, uint8_t* agree, float* lse, int* targ, hipStream_t st) {
  if (bad_args(z, ldz, u, ldu, temp, mode, B, L) || !u || !kd || !agree || !lse || !targ) return -1;
  const bool wg = L > WAVE_ROW_MAX;
  const dim3 grid(wg ? B : (B + 3) / 4), block(256);
#define JM_LAUNCH(T, WG)                                                                                      \
  hipLaunchKernelGGL((kd_loss_fwd_kernel<T, WG>), grid, block, 0, st, static_cast<const T*>(z), ldz,          \
                     static_cast<const T*>(u), ldu, temp, mode, B, L, kd, agree, lse, targ)
  if (bf16) {
    if (wg) JM_LAUNCH(uint16_t, true); else JM_LAUNCH(uint16_t, false);
  } else {
    if (wg) JM_LAUNCH(float, true); else JM_LAUNCH(float, false);
  }
#undef JM_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_kd_loss_bwd(const void* z, long ldz, const void* u, long ldu, int bf16, double temp, int mode, int B, int L,
                   const float* lse, const int* targ, const float* dloss, void* dz, long ldo, hipStream_t st) {
  if (bad_args(z, ldz, u, ldu, temp, mode, B, L) || !lse || !dloss || !dz || ldo < L) return -1;
  if (mode == 0 ? !u : !targ) return -1;
  if (mode == 1) u = nullptr;
  const bool wg = L > WAVE_ROW_MAX;
  const dim3 grid(wg ? B : (B + 3) / 4), block(256);
#define JM_LAUNCH(T, WG)                                                                                      \
  hipLaunchKernelGGL((kd_loss_bwd_kernel<T, WG>), grid, block, 0, st, static_cast<const T*>(z), ldz,          \
                     static_cast<const T*>(u), ldu, temp, mode, B, L, lse, targ, dloss, static_cast<T*>(dz), ldo)
  if (bf16) {
    if (wg) JM_LAUNCH(uint16_t, true); else JM_LAUNCH(uint16_t, false);
  } else {
    if (wg) JM_LAUNCH(float, true); else JM_LAUNCH(float, false);
  }
#undef JM_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(distill)
