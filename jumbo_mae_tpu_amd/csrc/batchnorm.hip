// Fused BatchNorm of the linear-probe head (parallel/syncbn.py): batch statistics, the
// normalisation in training and inference form, and the backward, on fp32 [B, J] features whose rows
// may be any distance >= J apart and start at any 4-byte address (a column slice).
//
// Layout, the same for every pass: a workgroup owns BN_COLS columns x BN_ROWS rows, one column per
// lane -- each wave load or store is one contiguous run of 64 elements, whatever the alignment -- and
// BN_ROWS / 4 rows per wave, all of them loaded before the first is used.  Reductions over the rows:
// every thread accumulates its rows in fp64, the four waves are added in a fixed order through LDS,
// the workgroup writes one fp64 partial per column, and a second kernel adds the partials of the row
// chunks in their order.  No atomics and no arrival counters, so reruns are bit-identical; and the
// fp64 sums of fp32 values and of their (exact) squares are exact whenever the true sum has 53 bits.
//
// Everything a thread computes between its loads and its stores is fp64: these passes wait for
// memory, and each fp32 tensor that leaves a kernel (packed, mean / rstd, y, dgamma, dbeta,
// packed_g, dx, the running statistics) is the fp64 value of its inputs rounded once.
#include "common.h"

namespace {

constexpr int BN_COLS = 64;               // columns per workgroup: one per lane
constexpr int BN_WAVES = 4;
constexpr int BN_ROWS = 64;               // rows per workgroup
constexpr int BN_RPT = BN_ROWS / BN_WAVES;  // rows per thread, all in flight at once
constexpr int BN_MAX_CHUNKS = 65535;      // gridDim.y

struct BnPos {
  int c, r0, w, lane;
  bool full;  // every row of this chunk lies inside the batch
};

JM_DEVICE BnPos bn_pos(int B) {
  BnPos p;
  p.lane = (int)(threadIdx.x & 63);
  p.w = (int)(threadIdx.x >> 6);
  p.c = (int)blockIdx.x * BN_COLS + p.lane;
  p.r0 = (int)blockIdx.y * BN_ROWS;
  p.full = p.r0 + BN_ROWS <= B;
  return p;
}

// row i of this thread: the waves interleave, so a chunk's rows are read in address order
JM_DEVICE int bn_row(const BnPos& p, int i) { return p.r0 + p.w + BN_WAVES * i; }

// the thread's BN_RPT elements of column p.c (rows past the batch: 0, never read).  The bounds test is
// hoisted out of the unrolled loads, so that a full chunk issues them back to back.
template <typename T>
JM_DEVICE void bn_load(const T* __restrict__ src, long ld, const BnPos& p, int B, float* v) {
  const T* q = src + p.c;
  if (p.full) {
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) v[i] = to_f<T>(q[(long)bn_row(p, i) * ld]);
  } else {
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const int r = bn_row(p, i);
      v[i] = 0.f;
      if (r < B) v[i] = to_f<T>(q[(long)r * ld]);
    }
  }
}

template <typename T>
JM_DEVICE void bn_store(T* __restrict__ dst, long ld, const BnPos& p, int B, const float* v) {
  T* q = dst + p.c;
#pragma unroll
  for (int i = 0; i < BN_RPT; ++i) {
    const int r = bn_row(p, i);
    if (p.full || r < B) q[(long)r * ld] = from_f<T>(v[i]);
  }
}

// the two column sums (a, b) of the workgroup's rows -> part[chunk][0 / 1][J]; called by every thread
JM_DEVICE void bn_block_partials(double a, double b, const BnPos& p, int J, double* __restrict__ part) {
  __shared__ double sh[2][BN_WAVES][BN_COLS];
  sh[0][p.w][p.lane] = a;
  sh[1][p.w][p.lane] = b;
  __syncthreads();
  if (p.w == 0 && p.c < J) {
    const int l = p.lane;
    a = (sh[0][0][l] + sh[0][1][l]) + (sh[0][2][l] + sh[0][3][l]);
    b = (sh[1][0][l] + sh[1][1][l]) + (sh[1][2][l] + sh[1][3][l]);
    double* o = part + (long)blockIdx.y * 2 * J;
    o[p.c] = a;
    o[(long)J + p.c] = b;
  }
}

// the partials of column c added over the chunks, in their order
JM_DEVICE void bn_finish_sums(const double* __restrict__ part, int chunks, int J, int c, double* a, double* b) {
  double s = 0.0, q = 0.0;
  for (int k = 0; k < chunks; ++k) {
    const double* o = part + (long)k * 2 * J;
    s += o[c];
    q += o[(long)J + c];
  }
  *a = s;
  *b = q;
}

JM_DEVICE double bn_rstd(double var, double eps) { return 1.0 / sqrt(var + eps); }

// ---------------------------------------------------------------------------------- statistics
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, long ld, int B, int J,
                                                       double* __restrict__ part) {
  JM_DGUARD(blockDim.x == 256 && (long)gridDim.x * BN_COLS >= J && (long)gridDim.y * BN_ROWS >= B && ld >= J);
  const BnPos p = bn_pos(B);
  double s = 0.0, q = 0.0;
  if (p.c < J) {
    float v[BN_RPT];
    bn_load(x, ld, p, B, v);
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const double d = (double)v[i];
      s += d;
      q += d * d;
    }
  }
  bn_block_partials(s, q, p, J, part);
}

// packed = [mean (J), mean of squares (J)]
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ part, int chunks, int B, int J,
                                                              float* __restrict__ packed) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= J) return;
  double s, q;
  bn_finish_sums(part, chunks, J, c, &s, &q);
  packed[c] = (float)(s / (double)B);
  packed[(long)J + c] = (float)(q / (double)B);
}

// ---------------------------------------------------------------------------------- normalisation
// TRAIN: (a0, a1) = packed's (mean, mean of squares), var = max(0, mean2 - mean^2); the workgroups of the
// first row chunk also write stats = [mean (J), rstd (J)] and move the running statistics.
// Inference: (a0, a1) = (running mean, running variance); nothing but y is written.
template <typename T, bool TRAIN>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, long ld, int B, int J,
                                                       const float* __restrict__ a0, const float* __restrict__ a1,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       double eps, double mom, double omm, T* __restrict__ y, long ldy,
                                                       float* __restrict__ stats, float* __restrict__ rm,
                                                       float* __restrict__ rv) {
  JM_DGUARD(blockDim.x == 256 && (long)gridDim.x * BN_COLS >= J && (long)gridDim.y * BN_ROWS >= B && ld >= J &&
            ldy >= J);
  const BnPos p = bn_pos(B);
  if (p.c >= J) return;
  float v[BN_RPT];
  bn_load(x, ld, p, B, v);
  const float m32 = a0[p.c], s32 = a1[p.c];
  const double mean = (double)m32;
  double var = (double)s32;
  if (TRAIN) {
    // mean2 - mean^2 without a rounding of its own.  Where mean2 IS the fp32 square of the mean, the
    // difference is only mean2's rounding: fp32 statistics cannot tell the column from a constant one
    // (B = 1, a constant column), and the variance is 0 as in the fp32 composition.
    const float sq32 = m32 * m32;
    var = s32 == sq32 ? 0.0 : fmax(var - mean * mean, 0.0);
  }
  const double rstd = bn_rstd(var, eps);
  const double g = (double)gamma[p.c], b = (double)beta[p.c];
#pragma unroll
  for (int i = 0; i < BN_RPT; ++i) v[i] = (float)((((double)v[i] - mean) * rstd) * g + b);
  bn_store(y, ldy, p, B, v);
  if (TRAIN && blockIdx.y == 0 && p.w == 0) {
    stats[p.c] = (float)mean;
    stats[(long)J + p.c] = (float)rstd;
    rm[p.c] = (float)(mom * (double)rm[p.c] + omm * mean);
    rv[p.c] = (float)(mom * (double)rv[p.c] + omm * var);
  }
}

// ---------------------------------------------------------------------------------- backward
// per column: sum dy and sum dy xhat, xhat = (x - mean) rstd rebuilt from x
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dy, long lddy,
                                                            const float* __restrict__ x, long ld, int B, int J,
                                                            const float* __restrict__ stats,
                                                            double* __restrict__ part) {
  JM_DGUARD(blockDim.x == 256 && (long)gridDim.x * BN_COLS >= J && (long)gridDim.y * BN_ROWS >= B && ld >= J &&
            lddy >= J);
  const BnPos p = bn_pos(B);
  double s = 0.0, q = 0.0;
  if (p.c < J) {
    float v[BN_RPT], d[BN_RPT];
    bn_load(x, ld, p, B, v);
    bn_load(dy, lddy, p, B, d);
    const double mean = (double)stats[p.c], rstd = (double)stats[(long)J + p.c];
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      // rows past the batch hold dy = 0 and add nothing
      const double g = (double)d[i];
      s += g;
      q += g * (((double)v[i] - mean) * rstd);
    }
  }
  bn_block_partials(s, q, p, J, part);
}

// dbeta = sum dy, dgamma = sum dy xhat (stored, or added with accum), packed_g = gamma times both
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ part, int chunks, int J,
                                                            const float* __restrict__ gamma,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            int accum, float* __restrict__ packed_g) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= J) return;
  double s, q;
  bn_finish_sums(part, chunks, J, c, &s, &q);
  const float db = (float)s, dg = (float)q;
  dbeta[c] = accum ? dbeta[c] + db : db;
  dgamma[c] = accum ? dgamma[c] + dg : dg;
  const double g = (double)gamma[c];
  packed_g[c] = (float)(g * s);
  packed_g[(long)J + c] = (float)(g * q);
}

// dx = rstd (gamma dy - sg / n - xhat sgx / n), (sg, sgx) = packed_g summed over the replicas
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const T* __restrict__ dy, long lddy,
                                                        const float* __restrict__ x, long ld, int B, int J,
                                                        const float* __restrict__ stats,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ packed_g, double inv_n,
                                                        float* __restrict__ dx, long lddx) {
  JM_DGUARD(blockDim.x == 256 && (long)gridDim.x * BN_COLS >= J && (long)gridDim.y * BN_ROWS >= B && ld >= J &&
            lddy >= J && lddx >= J);
  const BnPos p = bn_pos(B);
  if (p.c >= J) return;
  float v[BN_RPT], d[BN_RPT];
  bn_load(x, ld, p, B, v);
  bn_load(dy, lddy, p, B, d);
  const double mean = (double)stats[p.c], rstd = (double)stats[(long)J + p.c];
  const double g = (double)gamma[p.c];
  const double sg = (double)packed_g[p.c] * inv_n, sgx = (double)packed_g[(long)J + p.c] * inv_n;
#pragma unroll
  for (int i = 0; i < BN_RPT; ++i) {
    const double xhat = ((double)v[i] - mean) * rstd;
    v[i] = (float)(rstd * (g * (double)d[i] - sg - xhat * sgx));
  }
  bn_store(dx, lddx, p, B, v);
}

bool bad_shape(int B, int J, long ld) { return B < 1 || J < 1 || ld < J || jm_bn_chunks(B) > BN_MAX_CHUNKS; }

dim3 bn_grid(int B, int J) { return dim3((J + BN_COLS - 1) / BN_COLS, jm_bn_chunks(B)); }

int launched() { return hipGetLastError() == hipSuccess ? 0 : -2; }

}  // namespace

int jm_bn_chunks(int B) { return (B + BN_ROWS - 1) / BN_ROWS; }
int jm_bn_chunk_rows() { return BN_ROWS; }
int jm_bn_block_cols() { return BN_COLS; }

int jm_bn_stats(const float* x, long ld, int B, int J, double* part, float* packed, hipStream_t st) {
  if (bad_shape(B, J, ld) || !x || !part || !packed) return -1;
  hipLaunchKernelGGL(bn_stats_kernel, bn_grid(B, J), dim3(256), 0, st, x, ld, B, J, part);
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((J + 255) / 256), dim3(256), 0, st, part, jm_bn_chunks(B), B, J,
                     packed);
  return launched();
}

int jm_bn_apply(const float* x, long ld, int B, int J, const float* packed, const float* gamma, const float* beta,
                double eps, double momentum, void* y, int y_bf16, long ldy, float* stats, float* running_mean,
                float* running_var, hipStream_t st) {
  if (bad_shape(B, J, ld) || ldy < J || !x || !packed || !gamma || !beta || !y || !stats || !running_mean ||
      !running_var || !(eps > 0.0))
    return -1;
  const double omm = 1.0 - momentum;
  if (y_bf16)
    hipLaunchKernelGGL((bn_apply_kernel<uint16_t, true>), bn_grid(B, J), dim3(256), 0, st, x, ld, B, J, packed,
                       packed + J, gamma, beta, eps, momentum, omm, static_cast<uint16_t*>(y), ldy, stats,
                       running_mean, running_var);
  else
    hipLaunchKernelGGL((bn_apply_kernel<float, true>), bn_grid(B, J), dim3(256), 0, st, x, ld, B, J, packed,
                       packed + J, gamma, beta, eps, momentum, omm, static_cast<float*>(y), ldy, stats, running_mean,
                       running_var);
  return launched();
}

int jm_bn_apply_eval(const float* x, long ld, int B, int J, const float* running_mean, const float* running_var,
                     const float* gamma, const float* beta, double eps, void* y, int y_bf16, long ldy,
                     hipStream_t st) {
  if (bad_shape(B, J, ld) || ldy < J || !x || !running_mean || !running_var || !gamma || !beta || !y || !(eps > 0.0))
    return -1;
  float* none = nullptr;
  if (y_bf16)
    hipLaunchKernelGGL((bn_apply_kernel<uint16_t, false>), bn_grid(B, J), dim3(256), 0, st, x, ld, B, J, running_mean,
                       running_var, gamma, beta, eps, 0.0, 0.0, static_cast<uint16_t*>(y), ldy, none, none, none);
  else
    hipLaunchKernelGGL((bn_apply_kernel<float, false>), bn_grid(B, J), dim3(256), 0, st, x, ld, B, J, running_mean,
                       running_var, gamma, beta, eps, 0.0, 0.0, static_cast<float*>(y), ldy, none, none, none);
  return launched();
}

int jm_bn_bwd_reduce(const void* dy, int dy_bf16, long lddy, const float* x, long ld, int B, int J,
                     const float* stats, const float* gamma, double* part, float* dgamma, float* dbeta, int accum,
                     float* packed_g, hipStream_t st) {
  if (bad_shape(B, J, ld) || lddy < J || !dy || !x || !stats || !gamma || !part || !dgamma || !dbeta || !packed_g)
    return -1;
  if (dy_bf16)
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<uint16_t>, bn_grid(B, J), dim3(256), 0, st,
                       static_cast<const uint16_t*>(dy), lddy, x, ld, B, J, stats, part);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<float>, bn_grid(B, J), dim3(256), 0, st, static_cast<const float*>(dy),
                       lddy, x, ld, B, J, stats, part);
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((J + 255) / 256), dim3(256), 0, st, part, jm_bn_chunks(B), J, gamma,
                     dgamma, dbeta, accum, packed_g);
  return launched();
}

int jm_bn_bwd_dx(const void* dy, int dy_bf16, long lddy, const float* x, long ld, int B, int J, const float* stats,
                 const float* gamma, const float* packed_g, double n, float* dx, long lddx, hipStream_t st) {
  if (bad_shape(B, J, ld) || lddy < J || lddx < J || !dy || !x || !stats || !gamma || !packed_g || !dx || !(n >= 1.0))
    return -1;
  const double inv_n = 1.0 / n;
  if (dy_bf16)
    hipLaunchKernelGGL(bn_bwd_dx_kernel<uint16_t>, bn_grid(B, J), dim3(256), 0, st, static_cast<const uint16_t*>(dy),
                       lddy, x, ld, B, J, stats, gamma, packed_g, inv_n, dx, lddx);
  else
    hipLaunchKernelGGL(bn_bwd_dx_kernel<float>, bn_grid(B, J), dim3(256), 0, st, static_cast<const float*>(dy), lddy,
                       x, ld, B, J, stats, gamma, packed_g, inv_n, dx, lddx);
  return launched();
}

JM_DEBUG_EXPORT(batchnorm)
