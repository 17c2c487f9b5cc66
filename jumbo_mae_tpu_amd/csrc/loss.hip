// Fused classification loss: softmax cross-entropy or sigmoid BCE against the
// smoothed, Mixup / CutMix-mixed one-hot targets, the top-1 / top-5 hits and the logit gradient,
// straight from the integer labels -- the dense [B, L] targets of models/classifier.py are never
// built.  Per row the targets take at most three distinct values (own class a, the permuted row's
// class b, every other class); they are evaluated with the fp32 operations of the torch
// composition (smooth_labels, then Mixup.mix_labels), unfused and in its order, so that t_a == t_b
// holds here exactly when it holds there (the arg-max label set depends on it).
//
// Everything after the targets runs in fp64: the row is L2 / register resident and a row of 1000
// classes is 16 elements per lane, so the wider arithmetic is not what the kernel waits for, and
// loss and gradient come out correctly rounded for practical purposes -- lse travels to the backward
// as an fp32 (hi, lo) pair for the same reason (one fp32 alone is off by up to 2^-21 at lse ~ 10,
// several fp32 ulps of every softmax value).
//
// Layout: L <= WAVE_ROW_MAX: one wave per row (4 rows per workgroup), the row loaded once into 16
// registers per lane (element lane + 64 i: every wave load is one contiguous run, any alignment, any
// row stride); larger L: one 256-thread workgroup per row, each pass re-reading the row.  Wave
// butterflies + a fixed-order sum of the 4 wave results: no atomics, reruns are bit-identical.
#include "common.h"

namespace {

// on the per-element lambdas: the closure stays in registers
#define JM_INLINE __attribute__((always_inline))

constexpr int WAVE_ROW_MAX = 1024;  // 16 cached elements per lane
constexpr int ROW_CACHE = WAVE_ROW_MAX / WAVE;

struct ClsTargets {
  int a, b;          // own class, the permuted row's class (== a without mixing)
  float ta, tb, t0;  // their targets and every other class's
};

// labels / perm out of range: clamped (the composition clamps the labels), recorded in the debug build
JM_DEVICE ClsTargets cls_targets(const int64_t* labels, const int* perm, const float* wp, float s1, float s0, int r,
                                 int B, int L) {
#pragma clang fp contract(off)
  ClsTargets g;
  const long la = (long)labels[r];
  JM_DASSERT(la >= 0 && la < L);
  g.a = (int)(la < 0 ? 0 : (la >= L ? L - 1 : la));
  g.b = g.a;
  g.ta = g.tb = s1;
  g.t0 = s0;
  if (perm) {
    int pr = perm[r];
    JM_DASSERT(pr >= 0 && pr < B);
    pr = pr < 0 ? 0 : (pr >= B ? B - 1 : pr);
    const long lb = (long)labels[pr];
    JM_DASSERT(lb >= 0 && lb < L);
    g.b = (int)(lb < 0 ? 0 : (lb >= L ? L - 1 : lb));
    // w * labels + (1 - w) * labels[perm], one rounding per operation
    const float w = wp[0];
    const float omw = 1.f - w;
    const float x1 = w * s1, x0 = w * s0, y1 = omw * s1, y0 = omw * s0;
    g.t0 = x0 + y0;
    if (g.a == g.b) {
      g.ta = g.tb = x1 + y1;
    } else {
      g.ta = x1 + y0;
      g.tb = x0 + y1;
    }
  }
  return g;
}

// One row seen by its wave (cached) or its workgroup (re-read per pass)
template <bool WG>
struct RowCache {
  float v[ROW_CACHE];
};
template <>
struct RowCache<true> {};

template <typename T, bool WG>
struct Row : RowCache<WG> {
  static constexpr int NT = WG ? 256 : WAVE;
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
  // f(class, logit) for every element of this thread
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

// Reductions over the row's threads, every thread gets the result.  All 64 lanes of each wave
// are active at every call (a wave leaves only as a whole, before the first one).
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

template <bool WG>
JM_DEVICE float row_max(float v, double* sh) {
  v = wave_max(v);
  if (WG) {
    float* s = reinterpret_cast<float*>(sh);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    __syncthreads();
  }
  return v;
}

// log(1 + exp(x)) in its stable form
JM_DEVICE double softplus_d(float x) { return fmax((double)x, 0.0) + log1p(exp(-fabs((double)x))); }

// sigmoid without overflow
JM_DEVICE double sigmoid_d(float x) {
  const double e = exp(-fabs((double)x));
  const double r = 1.0 / (1.0 + e);
  return x >= 0.f ? r : e * r;
}

// the row of this wave / workgroup, -1 past the batch (wave-uniform)
template <bool WG>
JM_DEVICE int row_index(int B) {
  const int r = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  return r < B ? r : -1;
}

template <typename T, bool WG>
__global__ __launch_bounds__(256) void cls_loss_fwd_kernel(const T* __restrict__ z, long ld,
                                                           const int64_t* __restrict__ labels,
                                                           const int* __restrict__ perm, const float* __restrict__ wp,
                                                           float s1, float s0, int mode, int B, int L,
                                                           float* __restrict__ loss, uint8_t* __restrict__ hit,
                                                           float* __restrict__ lse2) {
  __shared__ double sh[4];
  const int r = row_index<WG>(B);
  if (r < 0) return;
  const int t = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const ClsTargets g = cls_targets(labels, perm, wp, s1, s0, r, B, L);
  const T* zr = z + (long)r * ld;
  const Row<T, WG> row(zr, L, t);
  const float za = to_f<T>(zr[g.a]), zb = to_f<T>(zr[g.b]);
  const bool two = g.a != g.b;

  // pass 1: row maximum, sum of the logits, ranks of the two candidate classes (lower index wins a tie)
  float m = -INFINITY;
  double sz = 0.0;
  int ra = 0, rb = 0;
  row.each([&](int c, float x) JM_INLINE {
    m = fmaxf(m, x);
    sz += (double)x;
    ra += (x > za || (x == za && c < g.a)) ? 1 : 0;
    rb += (x > zb || (x == zb && c < g.b)) ? 1 : 0;
  });
  m = row_max<WG>(m, sh);
  sz = row_sum<WG>(sz, sh);
  ra = row_sum<WG>(ra, sh);
  rb = row_sum<WG>(rb, sh);

  // arg-max label set: labels == labels.max(-1) of the dense targets (alpha < 1: never a third class)
  const float tm = two ? fmaxf(g.ta, g.tb) : g.ta;
  const bool ina = g.ta == tm, inb = two && g.tb == tm;
  const int k = L < 5 ? L : 5;
  const bool h1 = (ina && ra == 0) || (inb && rb == 0);
  const bool h5 = (ina && ra < k) || (inb && rb < k);

  double l, lse = 0.0;
  if (mode == 0) {
    double S = 0.0;
    row.each([&](int, float x) JM_INLINE { S += exp((double)x - (double)m); });
    S = row_sum<WG>(S, sh);
    const double logS = log(S);
    lse = (double)m + logS;
    // sum_c t_c (lse - z_c) with lse - z_c = log S + (m - z_c), as log_softmax has it (a label far
    // above the rest keeps its tiny loss); the L - 1 or L - 2 other classes through the logit sum
    const double da = logS + ((double)m - (double)za), db = logS + ((double)m - (double)zb);
    l = (double)g.t0 * ((double)L * logS + ((double)L * (double)m - sz)) + ((double)g.ta - (double)g.t0) * da;
    if (two) l += ((double)g.tb - (double)g.t0) * db;
  } else {
    // softplus(z) - t z = softplus(z) for t = 0 and softplus(-z) for t = 1: no cancellation; the
    // candidates' terms are added apart from the other classes' sum
    const float sg0 = g.t0 > 0.f ? -1.f : 1.f;
    const int ca = g.a, cb = g.b;
    double sp = 0.0;
    row.each([&](int c, float x) JM_INLINE {
      const double v = softplus_d(sg0 * x);
      sp += (c == ca || c == cb) ? 0.0 : v;
    });
    sp = row_sum<WG>(sp, sh);
    l = sp + softplus_d(g.ta > 0.f ? -za : za);
    if (two) l += softplus_d(g.tb > 0.f ? -zb : zb);
    l /= (double)L;
  }
  if (t == 0) {
    loss[r] = (float)l;
    hit[2 * (long)r] = h1 ? 1 : 0;
    hit[2 * (long)r + 1] = h5 ? 1 : 0;
    const float hi = (float)lse;
    lse2[2 * (long)r] = hi;
    lse2[2 * (long)r + 1] = (float)(lse - (double)hi);
  }
}

template <typename T, bool WG>
__global__ __launch_bounds__(256) void cls_loss_bwd_kernel(const T* __restrict__ z, long ld,
                                                           const int64_t* __restrict__ labels,
                                                           const int* __restrict__ perm, const float* __restrict__ wp,
                                                           float s1, float s0, int mode, int B, int L,
                                                           const float* __restrict__ lse2,
                                                           const float* __restrict__ dloss, T* __restrict__ dz,
                                                           long ldo) {
  const int r = row_index<WG>(B);
  if (r < 0) return;
  const int t = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const ClsTargets g = cls_targets(labels, perm, wp, s1, s0, r, B, L);
  const T* zr = z + (long)r * ld;
  const Row<T, WG> row(zr, L, t);
  T* d = dz + (long)r * ldo;
  const bool two = g.a != g.b;
  const double gl = (double)dloss[r];
  // every class as an "other" class first; the thread that owns a candidate class then rewrites
  // that element with its own target (same thread, program order)
  const bool own_a = g.a % (Row<T, WG>::NT) == t, own_b = two && g.b % (Row<T, WG>::NT) == t;
  if (mode == 0) {
    const double lse = (double)lse2[2 * (long)r] + (double)lse2[2 * (long)r + 1];
    const double Tsum = (double)(L - (two ? 2 : 1)) * (double)g.t0 + (double)g.ta + (two ? (double)g.tb : 0.0);
    const double t0 = (double)g.t0;
    row.each([&](int c, float x) JM_INLINE { d[c] = from_f<T>((float)(gl * (Tsum * exp((double)x - lse) - t0))); });
    if (own_a) d[g.a] = from_f<T>((float)(gl * (Tsum * exp((double)to_f<T>(zr[g.a]) - lse) - (double)g.ta)));
    if (own_b) d[g.b] = from_f<T>((float)(gl * (Tsum * exp((double)to_f<T>(zr[g.b]) - lse) - (double)g.tb)));
  } else {
    const double s = gl / (double)L;
    const double b0 = g.t0 > 0.f ? 1.0 : 0.0;
    row.each([&](int c, float x) JM_INLINE { d[c] = from_f<T>((float)(s * (sigmoid_d(x) - b0))); });
    if (own_a) d[g.a] = from_f<T>((float)(s * (sigmoid_d(to_f<T>(zr[g.a])) - (g.ta > 0.f ? 1.0 : 0.0))));
    if (own_b) d[g.b] = from_f<T>((float)(s * (sigmoid_d(to_f<T>(zr[g.b])) - (g.tb > 0.f ? 1.0 : 0.0))));
  }
}

// the fp32 values of the smoothed one-hot, as smooth_labels computes them: (1 - alpha) * {1, 0} + alpha / L
void smooth_values(double alpha, int L, float* s1, float* s0) {
  const float om = (float)(1.0 - alpha);
  *s0 = (float)(alpha / (double)L);
  *s1 = om + *s0;  // alpha 0: exactly 1 and 0, the unsmoothed one-hot
}

bool bad_args(const void* logits, long ld, const int64_t* labels, const int* perm, const float* w, double alpha,
              int mode, int B, int L) {
  return !logits || !labels || B < 1 || L < 1 || ld < L || (mode != 0 && mode != 1) || ((perm == nullptr) != (w == nullptr)) ||
         !(alpha >= 0.0 && alpha < 1.0);
}

}  // namespace

int jm_cls_loss_fwd(const void* logits, int bf16, long ld, const int64_t* labels, const int* perm, const float* w,
                    double smoothing, int mode, int B, int L, float* loss, uint8_t* hit, float* lse, hipStream_t st) {
  if (bad_args(logits, ld, labels, perm, w, smoothing, mode, B, L) || !loss || !hit || !lse) return -1;
  float s1, s0;
  smooth_values(smoothing, L, &s1, &s0);
  const bool wg = L > WAVE_ROW_MAX;
  const dim3 grid(wg ? B : (B + 3) / 4), block(256);
#define JM_LAUNCH(T, WG)                                                                                          \
  hipLaunchKernelGGL((cls_loss_fwd_kernel<T, WG>), grid, block, 0, st, static_cast<const T*>(logits), ld, labels, \
                     perm, w, s1, s0, mode, B, L, loss, hit, lse)
  if (bf16) {
    if (wg) JM_LAUNCH(uint16_t, true); else JM_LAUNCH(uint16_t, false);
  } else {
    if (wg) JM_LAUNCH(float, true); else JM_LAUNCH(float, false);
  }
#undef JM_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_cls_loss_bwd(const void* logits, int bf16, long ld, const int64_t* labels, const int* perm, const float* w,
                    double smoothing, int mode, int B, int L, const float* lse, const float* dloss, void* dlogits,
                    long ldo, hipStream_t st) {
  if (bad_args(logits, ld, labels, perm, w, smoothing, mode, B, L) || !lse || !dloss || !dlogits || ldo < L) return -1;
  float s1, s0;
  smooth_values(smoothing, L, &s1, &s0);
  const bool wg = L > WAVE_ROW_MAX;
  const dim3 grid(wg ? B : (B + 3) / 4), block(256);
#define JM_LAUNCH(T, WG)                                                                                          \
  hipLaunchKernelGGL((cls_loss_bwd_kernel<T, WG>), grid, block, 0, st, static_cast<const T*>(logits), ld, labels, \
                     perm, w, s1, s0, mode, B, L, lse, dloss, static_cast<T*>(dlogits), ldo)
  if (bf16) {
    if (wg) JM_LAUNCH(uint16_t, true); else JM_LAUNCH(uint16_t, false);
  } else {
    if (wg) JM_LAUNCH(float, true); else JM_LAUNCH(float, false);
  }
#undef JM_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(loss)
