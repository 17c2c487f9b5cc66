// QK-norm: per-head RMSNorm of q and k on the fused QKV tensor, with the axial rotary embedding of
// rope.hip fused behind it (ops/qknorm.py holds the definition).
//
// qkv is [B, S, 3, H, hd] contiguous.  Every (b, t, q|k, h) row x[hd] becomes y = x r g with
// r = 1 / sqrt(mean(x^2) + 1e-6) and the layer's fp32 scale g_q or g_k [hd]; with a rope table the
// rows t >= n_cls are then rotated exactly as rope.hip rotates them (same table, same pair
// expression), and the result is rounded once to the tensor's dtype.  v is neither read nor written.
//
// Lane mapping.  One lane owns 8 consecutive channels of one head row -- one 16-byte vector of a
// bf16 tensor, two of an fp32 tensor -- so a row is hd / 8 = 4, 8, 10, 12 or 16 lanes.  A row lives
// in an aligned group of GS = 4, 8 or 16 lanes (the next power of two, one DPP row at most); the
// surplus lanes of hd 80 and 96 load nothing and add zeros.  With hd % 16 == 0 a lane never
// straddles a head or the rotary y / x boundary at hd / 2.  Consecutive groups take consecutive
// rows of the 2 H hd contiguous q|k elements of a token, so a wave reads whole runs.
// Row sums: 8 fused multiply-adds in channel order inside the lane, then the xor butterfly of
// common.h row16_sum cut off at the group size; each stage adds the same two operands in every
// lane of a pair, so all lanes of a group hold the same bits and the order is fixed.
//
// Backward (dy = gradient of what the attention kernels consumed, in dqkv; x = the forward's saved
// pre-norm q|k bits): u = inverse-rotate(dy) on the rotated rows, r recomputed from x, xh = x r,
// t = u g, dx = r (t - xh mean(t xh)) over dy in place -- exact at g == 0, nothing is divided by g.
// dg = sum over rows of u xh: every lane keeps its 8 channels' sums for q and for k over the
// grid-stride loop, the workgroup adds its lanes' sums in lane-group order through LDS and writes one
// partial [2, hd]; qknorm_finish adds the partials in workgroup order (16 interleaved chains, then a
// fixed tree).  The grid depends on the shape alone, so every sum has one order: no atomics, reruns
// are bit-identical, nothing syncs with the host.
// The backward's arithmetic is fp64 from the loaded values to the one rounding of dx and of dg: dx
// cancels (t - xh m) and dg sums B S H products per channel, and in fp32 both miss the fp64 gradient
// by several fp32 ulps (measured: dg 4.4 x the tests' bound); the kernel is bound by its 6 bytes
// per element of HBM traffic, not by the vector ALU, at either width.
#include <climits>

#include "common.h"

namespace {

constexpr int QKN_THREADS = 256;
constexpr int QKN_MAX_BLOCKS = 1024;  // grid-stride beyond: 4 workgroups per CU
constexpr int QKN_E = 8;              // channels per lane
constexpr float QKN_EPS = 1e-6f;      // prims.LN_EPS

// 8 elements moved as raw bits (saved must hold the input's exact bits) and read as floats
template <typename T>
struct Vec8;
template <>
struct Vec8<uint16_t> {
  bf16x8_u v;
  JM_DEVICE void load(const uint16_t* p) { v.u = *reinterpret_cast<const uint4*>(p); }
  JM_DEVICE void store(uint16_t* p) const { *reinterpret_cast<uint4*>(p) = v.u; }
  JM_DEVICE void get(float* f) const {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = bf2f(v.h[i]);
  }
};
template <>
struct Vec8<float> {
  float4 a, b;
  JM_DEVICE void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  JM_DEVICE void store(float* p) const {
    *reinterpret_cast<float4*>(p) = a;
    *reinterpret_cast<float4*>(p + 4) = b;
  }
  JM_DEVICE void get(float* f) const {
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
};

// sum over the aligned group of GS lanes; every lane of the group gets the same bits.  Requires the
// whole DPP row active.
template <int GS>
JM_DEVICE float group_sum(float v) {
  v += dpp_mov<0xB1>(v);                // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);                // quad_perm [2,3,0,1]
  if (GS >= 8) v += dpp_mov<0x141>(v);  // row_half_mirror
  if (GS >= 16) v += dpp_mov<0x140>(v); // row_mirror
  return v;
}

template <int CTRL>
JM_DEVICE double dpp_mov_d(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = dpp_mov_u32<CTRL>((uint32_t)b), hi = dpp_mov_u32<CTRL>((uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <int GS>
JM_DEVICE double group_sum_d(double v) {
  v += dpp_mov_d<0xB1>(v);
  v += dpp_mov_d<0x4E>(v);
  if (GS >= 8) v += dpp_mov_d<0x141>(v);
  if (GS >= 16) v += dpp_mov_d<0x140>(v);
  return v;
}

struct QknGeo {
  int S, n_cls, H, hd, gw, G;
  const float* table;  // null: no rotation
  const int* pos;
  long posB;
  long groups;  // B S 2 H head rows
};

// what one lane works on: the head row of its group and its 8 channels in it
struct QknLane {
  bool valid;      // the row exists and the lane's channels lie inside hd
  bool rot;        // valid, and the row is rotated
  int s;           // 0 = q, 1 = k
  int d;           // first channel within the head
  long qkv_off;    // element offset in qkv / dqkv
  long saved_off;  // element offset in saved [B, S, 2, H, hd]
  const float* cs; // (cos, sin) of the lane's 4 pairs
};

template <int GS>
JM_DEVICE QknLane qkn_lane(const QknGeo& g, long i) {
  QknLane L;
  const long gi = i / GS;
  const int j = (int)(i - gi * GS);
  const int HD = g.H * g.hd;
  L.d = j * QKN_E;
  L.valid = gi < g.groups && L.d < g.hd;
  const long row = L.valid ? gi : 0;
  const long bt = row / (2 * g.H);
  const int rem = (int)(row - bt * (2 * g.H));  // s * H + h
  L.s = rem >= g.H ? 1 : 0;
  const long co = (long)rem * g.hd + (L.valid ? L.d : 0);
  L.qkv_off = bt * (3L * HD) + co;
  L.saved_off = bt * (2L * HD) + co;
  const int b = (int)(bt / g.S), t = (int)(bt - (long)b * g.S);
  L.rot = L.valid && g.table != nullptr && t >= g.n_cls;
  L.cs = nullptr;
  if (L.rot) {  // as rope.hip: patch index -> (y, x), channels [0, hd/2) turn by y, the rest by x
    const int tp = t - g.n_cls;
    int p = g.pos ? g.pos[b * g.posB + tp] : tp;
    JM_DASSERT(p >= 0 && p < g.G * g.gw);
    p = min(max(p, 0), g.G * g.gw - 1);  // the table read stays inside [G, hd/4, 2] whatever pos holds
    const int y = p / g.gw, x = p - y * g.gw;
    const int half = g.hd >> 1;
    const int coord = L.d >= half ? x : y;
    const int pair0 = (L.d >= half ? L.d - half : L.d) >> 1;
    L.cs = g.table + ((long)coord * (g.hd >> 2) + pair0) * 2;
  }
  return L;
}

// the pair expression of rope.hip; inverse: sin negated
JM_DEVICE void qkn_rotate(const float* f, const float* cs, bool inverse, float* o) {
  float t[QKN_E];
  load8(cs, t);
#pragma unroll
  for (int j = 0; j < QKN_E; j += 2) {
    const float co = t[j], si = inverse ? -t[j + 1] : t[j + 1];
    o[j] = __fsub_rn(__fmul_rn(f[j], co), __fmul_rn(f[j + 1], si));
    o[j + 1] = __fadd_rn(__fmul_rn(f[j + 1], co), __fmul_rn(f[j], si));
  }
}

template <int GS>
JM_DEVICE float qkn_rstd(const float* x, int hd) {
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < QKN_E; ++e) ss = __builtin_fmaf(x[e], x[e], ss);
  ss = group_sum<GS>(ss);
  return 1.f / sqrtf(ss / (float)hd + QKN_EPS);
}

template <typename T, int GS>
__global__ __launch_bounds__(QKN_THREADS) void qknorm_fwd_kernel(T* __restrict__ qkv, T* __restrict__ saved,
                                                                 const float* __restrict__ gq,
                                                                 const float* __restrict__ gk, QknGeo g) {
  JM_DGUARD(blockDim.x == QKN_THREADS);
  const long total = g.groups * GS;
  // the loop bound is workgroup-uniform: every lane stays in for the DPP sums
  for (long base = (long)blockIdx.x * QKN_THREADS; base < total; base += (long)gridDim.x * QKN_THREADS) {
    const QknLane L = qkn_lane<GS>(g, base + threadIdx.x);
    float x[QKN_E] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (L.valid) {
      Vec8<T> raw;
      raw.load(qkv + L.qkv_off);
      raw.store(saved + L.saved_off);
      raw.get(x);
    }
    const float r = qkn_rstd<GS>(x, g.hd);
    if (L.valid) {
      float sc[QKN_E], y[QKN_E], o[QKN_E];
      load8((L.s ? gk : gq) + L.d, sc);
#pragma unroll
      for (int e = 0; e < QKN_E; ++e) y[e] = __fmul_rn(__fmul_rn(x[e], r), sc[e]);
      if (L.rot) {
        qkn_rotate(y, L.cs, false, o);
        store8(qkv + L.qkv_off, o);
      } else {
        store8(qkv + L.qkv_off, y);
      }
    }
  }
}

template <typename T, int GS>
__global__ __launch_bounds__(QKN_THREADS) void qknorm_bwd_kernel(T* __restrict__ dqkv, const T* __restrict__ saved,
                                                                 const float* __restrict__ gq,
                                                                 const float* __restrict__ gk,
                                                                 double* __restrict__ part, QknGeo g) {
  JM_DGUARD(blockDim.x == QKN_THREADS);
  __shared__ double red[QKN_THREADS][2 * QKN_E + 1];
  const long total = g.groups * GS;
  const double inv_hd = 1.0 / (double)g.hd;
  double aq[QKN_E] = {0., 0., 0., 0., 0., 0., 0., 0.};
  double ak[QKN_E] = {0., 0., 0., 0., 0., 0., 0., 0.};
  for (long base = (long)blockIdx.x * QKN_THREADS; base < total; base += (long)gridDim.x * QKN_THREADS) {
    const QknLane L = qkn_lane<GS>(g, base + threadIdx.x);
    float x[QKN_E] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dy[QKN_E] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float sc[QKN_E] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float cs[QKN_E] = {1.f, 0.f, 1.f, 0.f, 1.f, 0.f, 1.f, 0.f};  // (cos, sin) of the 4 pairs; the identity
    if (L.valid) {
      Vec8<T> raw;
      raw.load(saved + L.saved_off);
      raw.get(x);
      load8(dqkv + L.qkv_off, dy);
      load8((L.s ? gk : gq) + L.d, sc);
      if (L.rot) load8(L.cs, cs);
    }
    double u[QKN_E];
#pragma unroll
    for (int e = 0; e < QKN_E; e += 2) {  // the transpose of the forward's rotation: sin negated
      const double co = (double)cs[e], si = -(double)cs[e + 1];
      u[e] = (double)dy[e] * co - (double)dy[e + 1] * si;
      u[e + 1] = (double)dy[e + 1] * co + (double)dy[e] * si;
    }
    double ss = 0.;
#pragma unroll
    for (int e = 0; e < QKN_E; ++e) ss = __builtin_fma((double)x[e], (double)x[e], ss);
    ss = group_sum_d<GS>(ss);
    const double r = 1.0 / sqrt(ss * inv_hd + 1e-6);
    double xh[QKN_E], t[QKN_E];
    double dot = 0.;
#pragma unroll
    for (int e = 0; e < QKN_E; ++e) {
      xh[e] = (double)x[e] * r;
      t[e] = u[e] * (double)sc[e];
      dot = __builtin_fma(t[e], xh[e], dot);
    }
    const double m = group_sum_d<GS>(dot) * inv_hd;
#pragma unroll
    for (int e = 0; e < QKN_E; ++e) {
      const double p = u[e] * xh[e];  // 0 on the lanes that hold nothing
      aq[e] += L.s ? 0. : p;
      ak[e] += L.s ? p : 0.;
    }
    if (L.valid) {
      float dx[QKN_E];
#pragma unroll
      for (int e = 0; e < QKN_E; ++e) dx[e] = (float)(r * (t[e] - xh[e] * m));
      store8(dqkv + L.qkv_off, dx);
    }
  }
  // the workgroup's [2, hd] partial: lane j of every group holds channels [8 j, 8 j + 8)
#pragma unroll
  for (int e = 0; e < QKN_E; ++e) {
    red[threadIdx.x][e] = aq[e];
    red[threadIdx.x][QKN_E + e] = ak[e];
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < 2 * g.hd) {
    const int s = c / g.hd, d = c - s * g.hd;
    const int j = d / QKN_E, e = d - j * QKN_E;
    double acc = 0.;
    for (int grp = 0; grp < QKN_THREADS / GS; ++grp) acc += red[grp * GS + j][s * QKN_E + e];
    part[(long)blockIdx.x * (2 * g.hd) + c] = acc;
  }
}

// dg[c] = sum of part[b][c] over the nb workgroups: 16 chains b = r, r + 16, .. per channel in workgroup
// order, then a fixed tree over the chains, rounded once to fp32.  One workgroup per 16 channels
// (2 hd % 16 == 0).
__global__ __launch_bounds__(QKN_THREADS) void qknorm_finish_kernel(const double* __restrict__ part,
                                                                    float* __restrict__ dg, int nb, int C) {
  JM_DGUARD(blockDim.x == QKN_THREADS);
  __shared__ double red[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + c;
  double acc = 0.;
  for (int b = r; b < nb; b += 16) acc += part[(long)b * C + ch];
  red[r][c] = acc;
  __syncthreads();
  if (r == 0) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = red[k][c];
#pragma unroll
    for (int w = 1; w < 16; w <<= 1)
#pragma unroll
      for (int k = 0; k < 16; k += 2 * w) v[k] += v[k + w];
    dg[ch] = (float)v[0];
  }
}

int qkn_group(int hd) { return hd == 32 ? 4 : hd == 64 ? 8 : (hd == 80 || hd == 96 || hd == 128) ? 16 : 0; }

bool qkn_geo(int B, int S, int heads, int hd, int n_cls, int gw, const float* table, int G, const int* pos,
             long posB, QknGeo& g) {
  if (B <= 0 || S <= 0 || heads <= 0 || qkn_group(hd) == 0 || posB < 0) return false;
  if ((long)heads * hd > INT_MAX / 4 || (long)B * S > INT_MAX) return false;
  if (table != nullptr) {
    if (n_cls < 0 || n_cls > S || gw <= 0 || G <= 0 || (long)G * gw > INT_MAX) return false;
    if (!pos && (long)(S - n_cls) > (long)G * gw) return false;  // t - n_cls must be a table position
  }
  g.S = S;
  g.n_cls = n_cls;
  g.H = heads;
  g.hd = hd;
  g.gw = gw;
  g.G = G;
  g.table = table;
  g.pos = pos;
  g.posB = posB;
  g.groups = (long)B * S * 2 * heads;
  return true;
}

int qkn_blocks(long groups, int GS) {
  const long want = (groups * GS + QKN_THREADS - 1) / QKN_THREADS;
  return (int)(want < QKN_MAX_BLOCKS ? want : QKN_MAX_BLOCKS);
}

}  // namespace

int jm_qknorm_bwd_blocks(int B, int S, int heads, int hd) {
  const int GS = qkn_group(hd);
  if (B <= 0 || S <= 0 || heads <= 0 || GS == 0) return 0;
  return qkn_blocks((long)B * S * 2 * heads, GS);
}

#define QKN_DISPATCH(KERNEL, T, ...)                                                  \
  do {                                                                                \
    if (GS == 4) KERNEL<T, 4><<<grid, QKN_THREADS, 0, st>>>(__VA_ARGS__);             \
    else if (GS == 8) KERNEL<T, 8><<<grid, QKN_THREADS, 0, st>>>(__VA_ARGS__);        \
    else KERNEL<T, 16><<<grid, QKN_THREADS, 0, st>>>(__VA_ARGS__);                    \
  } while (0)

int jm_qknorm_fwd(void* qkv, void* saved, int bf16, int B, int S, int heads, int hd, const float* g_q,
                  const float* g_k, int n_cls, int gw, const float* table, int G, const int* pos, long posB,
                  hipStream_t st) {
  QknGeo g;
  if (qkv == nullptr || saved == nullptr || g_q == nullptr || g_k == nullptr ||
      !qkn_geo(B, S, heads, hd, n_cls, gw, table, G, pos, posB, g))
    return -1;
  const int GS = qkn_group(hd);
  const int grid = qkn_blocks(g.groups, GS);
  if (bf16) QKN_DISPATCH(qknorm_fwd_kernel, uint16_t, (uint16_t*)qkv, (uint16_t*)saved, g_q, g_k, g);
  else QKN_DISPATCH(qknorm_fwd_kernel, float, (float*)qkv, (float*)saved, g_q, g_k, g);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int jm_qknorm_bwd(void* dqkv, const void* saved, int bf16, int B, int S, int heads, int hd, const float* g_q,
                  const float* g_k, int n_cls, int gw, const float* table, int G, const int* pos, long posB,
                  double* part, float* dg, hipStream_t st) {
  QknGeo g;
  if (dqkv == nullptr || saved == nullptr || g_q == nullptr || g_k == nullptr || part == nullptr || dg == nullptr ||
      !qkn_geo(B, S, heads, hd, n_cls, gw, table, G, pos, posB, g))
    return -1;
  const int GS = qkn_group(hd);
  const int grid = qkn_blocks(g.groups, GS);
  if (bf16) QKN_DISPATCH(qknorm_bwd_kernel, uint16_t, (uint16_t*)dqkv, (const uint16_t*)saved, g_q, g_k, part, g);
  else QKN_DISPATCH(qknorm_bwd_kernel, float, (float*)dqkv, (const float*)saved, g_q, g_k, part, g);
  if (hipGetLastError() != hipSuccess) return -2;
  qknorm_finish_kernel<<<2 * hd / 16, QKN_THREADS, 0, st>>>(part, dg, grid, 2 * hd);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(qknorm)
