// SwiGLU gate of the gated feed-forward (gfx950), ops/swiglu.py holds the definition.
//
//  swiglu_fwd   a[m, c]         = bf16( silu(g) u drop )                g = pre[m, c], u = pre[m, Hs + c]
//  swiglu_bwd   dpre[m, c]      = bf16( da drop u sigma (1 + g (1 - sigma)) )
//               dpre[m, Hs + c] = bf16( da drop silu(g) )
//               bias_grad      += colsum(dpre) over all 2 Hs columns     (the gradients of b1 | b3)
//
// pre = [gate | up] is the contiguous [M, 2 Hs] output of ONE FF1 GEMM over the adjacent w1 | w3 segments.
// Both kernels are pure streaming (forward 6 B per element of a, backward 10 B + the partial rows): every
// access is 16 B per lane, a thread owns 8 adjacent columns and walks the rows of its slab U at a time with
// all loads of a trip issued before the first use (32 KiB / 48 KiB in flight per workgroup), and the grid
// strides over (row slab, column chunk of <= 2048 columns) items.  The hidden dropout's keep bits are
// common.h drop_keep on the element index of a (m Hs + c); the backward regenerates them, no mask is stored.
//
// Arithmetic, fp32, in this order (ops/swiglu.py mirrors it operation by operation):
//   e = exp(-g)   sigma = rcp(1 + e)   s = g sigma   a = (s u) drop
//   t = 1 - sigma where g < 0, e sigma elsewhere  (= 1 - sigma without the cancellation at large g; e <= 1 there, so
//                                                   an overflowed e = inf at g < -88 never meets sigma = 0)
//   f = 1 + g t   dam = da drop   dgate = ((dam u) sigma) f   dup = dam s
// expf is the library's (<= 1 ulp: its argument reduction is exact, unlike exp2(g log2 e)), the reciprocal
// the hardware's (v_rcp_f32, 1 ulp).  sigma saturates cleanly: e = inf -> 0, e = 0 -> 1; no NaN from finite g.
//
// The bias gradient follows jm_gelu_bwd: the column sums are taken over the bf16 values the GEMMs consume,
// each (slab, chunk) item merges its row slots through LDS in slot order into one partial row of ws, and a
// column-sum pass adds the partial rows into bias_grad in a fixed order -- no atomics, the same bits on every run.
#include "common.h"
#include "jm_api.h"

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_CW = 2048;        // columns per chunk: 256 lanes x 8
constexpr int SW_U = 4;            // rows per trip and slot
constexpr int SW_MAX_ITEMS = 512;  // (slab, chunk) items aimed at: <= 512 partial rows of 2 Hs floats
constexpr int SW_MAX_GRID = 2048;

struct SwGeom {
  int ncol;   // column chunks
  int rows;   // rows per slab
  int nb;     // row slabs (= partial rows of the backward)
  long items;
};

bool sw_geom(int M, int Hs, SwGeom& g) {
  if (M <= 0 || Hs <= 0 || Hs % 8) return false;
  g.ncol = (Hs + SW_CW - 1) / SW_CW;
  const int cap = SW_MAX_ITEMS / g.ncol > 1 ? SW_MAX_ITEMS / g.ncol : 1;
  int rows = 16;
  if ((M + rows - 1) / rows > cap) rows = (M + cap - 1) / cap;
  // few rows (the jumbo MLP: 512 x 8192): one item per CU before 16 rows per slab
  const int want = (256 + g.ncol - 1) / g.ncol;
  if ((M + rows - 1) / rows < want) rows = (M + want - 1) / want;
  if (rows < 1) rows = 1;
  g.rows = rows;
  g.nb = (M + rows - 1) / rows;
  g.items = (long)g.nb * g.ncol;
  return true;
}

// the thread's place in one (slab, chunk) item
struct SwItem {
  int col, nc, rps, slot, r_begin, r_end, slab, c0;
  bool active;
};

JM_DEVICE SwItem sw_item(long item, int ncol, int rows, int M, int Hs) {
  SwItem it;
  it.slab = (int)(item / ncol);
  it.c0 = (int)(item % ncol) * SW_CW;
  it.nc = (Hs - it.c0) < SW_CW ? (Hs - it.c0) : SW_CW;
  const int tpr = it.nc / 8;  // <= 256 threads per row, one 16-byte vector each
  it.rps = SW_THREADS / tpr;
  it.slot = threadIdx.x / tpr;
  it.col = it.c0 + (threadIdx.x % tpr) * 8;
  it.active = it.slot < it.rps;
  it.r_begin = it.slab * rows;
  it.r_end = it.r_begin + rows < M ? it.r_begin + rows : M;
  return it;
}

JM_DEVICE void unpack8(const uint4& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

JM_DEVICE uint4 pack8(const float* f) {
  return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}

// sigma(g) and e = exp(-g)
JM_DEVICE float sw_sigmoid(float g, float& e) {
  e = expf(-g);
  return __builtin_amdgcn_rcpf(1.f + e);
}

template <bool DROP>
__global__ __launch_bounds__(SW_THREADS) void swiglu_fwd_kernel(const uint16_t* __restrict__ pre,
                                                                uint16_t* __restrict__ a, int M, int Hs, int ncol,
                                                                int rows, long items, DropIO drop) {
  JM_DGUARD(Hs % 8 == 0 && M > 0 && rows > 0);
  const long ldp = 2L * Hs;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const SwItem it = sw_item(item, ncol, rows, M, Hs);
    if (!it.active) continue;
    JM_DASSERT(it.col + 8 <= Hs);
    for (int r0 = it.r_begin + it.slot; r0 < it.r_end; r0 += SW_U * it.rps) {
      uint4 vg[SW_U], vu[SW_U];
#pragma unroll
      for (int u = 0; u < SW_U; ++u) {
        const int r = r0 + u * it.rps;
        if (r < it.r_end) {
          const uint16_t* p = pre + (long)r * ldp + it.col;
          vg[u] = *reinterpret_cast<const uint4*>(p);
          vu[u] = *reinterpret_cast<const uint4*>(p + Hs);
        }
      }
#pragma unroll
      for (int u = 0; u < SW_U; ++u) {
        const int r = r0 + u * it.rps;
        if (r >= it.r_end) break;
        float g[8], x[8], o[8];
        unpack8(vg[u], g);
        unpack8(vu[u], x);
        const long idx = (long)r * Hs + it.col;  // element index of a: the dropout mask's
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float e;
          const float s = g[j] * sw_sigmoid(g[j], e);
          o[j] = s * x[j];
        }
        if (DROP) {
          float f[8];
          drop_factors<8>(drop, idx, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] *= f[j];
        }
        *reinterpret_cast<uint4*>(a + idx) = pack8(o);
      }
    }
  }
}

template <bool DROP, bool BIAS>
__global__ __launch_bounds__(SW_THREADS) void swiglu_bwd_kernel(const uint16_t* __restrict__ pre,
                                                                const uint16_t* __restrict__ da,
                                                                uint16_t* __restrict__ dpre, int M, int Hs, int ncol,
                                                                int rows, long items, DropIO drop,
                                                                float* __restrict__ ws) {
  // slot partials of the item's gate and up columns: rps * nc <= 2048 floats each
  __shared__ __attribute__((aligned(16))) float red[2][SW_CW];
  JM_DGUARD(Hs % 8 == 0 && M > 0 && rows > 0);
  const long ldp = 2L * Hs;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {  // (the bounds are workgroup-uniform)
    const SwItem it = sw_item(item, ncol, rows, M, Hs);
    if (it.active) {
      JM_DASSERT(it.col + 8 <= Hs);
      float sg[8], su[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) sg[j] = su[j] = 0.f;
      for (int r0 = it.r_begin + it.slot; r0 < it.r_end; r0 += SW_U * it.rps) {
        uint4 vg[SW_U], vu[SW_U], vd[SW_U];
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
          const int r = r0 + u * it.rps;
          if (r < it.r_end) {
            const uint16_t* p = pre + (long)r * ldp + it.col;
            vg[u] = *reinterpret_cast<const uint4*>(p);
            vu[u] = *reinterpret_cast<const uint4*>(p + Hs);
            vd[u] = *reinterpret_cast<const uint4*>(da + (long)r * Hs + it.col);
          }
        }
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
          const int r = r0 + u * it.rps;
          if (r >= it.r_end) break;
          float g[8], x[8], d[8], og[8], ou[8];
          unpack8(vg[u], g);
          unpack8(vu[u], x);
          unpack8(vd[u], d);
          if (DROP) {
            float f[8];
            drop_factors<8>(drop, (long)r * Hs + it.col, f);
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] *= f[j];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float e;
            const float sig = sw_sigmoid(g[j], e);
            const float t = g[j] < 0.f ? 1.f - sig : e * sig;
            const float f = 1.f + g[j] * t;
            og[j] = ((d[j] * x[j]) * sig) * f;
            ou[j] = d[j] * (g[j] * sig);
          }
          const uint4 pg = pack8(og), pu = pack8(ou);
          uint16_t* q = dpre + (long)r * ldp + it.col;
          *reinterpret_cast<uint4*>(q) = pg;
          *reinterpret_cast<uint4*>(q + Hs) = pu;
          if (BIAS) {  // the column sums of the rounded values, the ones the GEMMs consume
            unpack8(pg, og);
            unpack8(pu, ou);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              sg[j] += og[j];
              su[j] += ou[j];
            }
          }
        }
      }
      if (BIAS) {
        float* rg = &red[0][it.slot * it.nc + (it.col - it.c0)];
        float* ru = &red[1][it.slot * it.nc + (it.col - it.c0)];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          rg[j] = sg[j];
          ru[j] = su[j];
        }
      }
    }
    if (BIAS) {
      __syncthreads();
      // the item's partial row (slots summed in order) -> ws[slab][c0 ..) and ws[slab][Hs + c0 ..)
      float* wr = ws + (long)it.slab * ldp + it.c0;
      for (int i = threadIdx.x; i < it.nc; i += SW_THREADS) {
        float pg = 0.f, pu = 0.f;
        for (int k = 0; k < it.rps; ++k) {
          pg += red[0][k * it.nc + i];
          pu += red[1][k * it.nc + i];
        }
        wr[i] = pg;
        wr[Hs + i] = pu;
      }
      __syncthreads();  // red is the next item's
    }
  }
}

int sw_grid(long items) { return (int)(items < SW_MAX_GRID ? items : SW_MAX_GRID); }

// -1 bad argument, -2 an operand of 4 GiB or more
int sw_check(const void* pre, const void* x, int M, int Hs, SwGeom& g) {
  if (pre == nullptr || x == nullptr || !sw_geom(M, Hs, g)) return -1;
  if (((uintptr_t)pre | (uintptr_t)x) & 15) return -1;
  if ((long)M * Hs * 4 >= (1L << 32)) return -2;  // pre / dpre: M * 2 Hs bf16
  return 0;
}

}  // namespace

long jm_swiglu_ws_floats(int M, int Hs) {
  SwGeom g;
  if (!sw_geom(M, Hs, g)) return 0;
  return (long)g.nb * 2 * Hs;
}

int jm_swiglu_fwd(const uint16_t* pre, uint16_t* a, int M, int Hs, const int64_t* seed, uint32_t thr, float scale,
                  hipStream_t st) {
  SwGeom g;
  const int rc = sw_check(pre, a, M, Hs, g);
  if (rc) return rc;
  const DropIO drop{seed, thr, scale, 0};
  if (seed)
    swiglu_fwd_kernel<true><<<sw_grid(g.items), SW_THREADS, 0, st>>>(pre, a, M, Hs, g.ncol, g.rows, g.items, drop);
  else
    swiglu_fwd_kernel<false><<<sw_grid(g.items), SW_THREADS, 0, st>>>(pre, a, M, Hs, g.ncol, g.rows, g.items, drop);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int jm_swiglu_bwd(const uint16_t* pre, const uint16_t* da, uint16_t* dpre, float* bias_grad, int M, int Hs,
                  const int64_t* seed, uint32_t thr, float scale, hipStream_t st, float* ws) {
  SwGeom g;
  int rc = sw_check(pre, da, M, Hs, g);
  if (rc) return rc;
  if (dpre == nullptr || ((uintptr_t)dpre & 15)) return -1;
  if (bias_grad && (ws == nullptr || (((uintptr_t)bias_grad | (uintptr_t)ws) & 15))) return -1;
  const DropIO drop{seed, thr, scale, 0};
  const int grid = sw_grid(g.items);
#define SW_BWD(D, B) \
  swiglu_bwd_kernel<D, B><<<grid, SW_THREADS, 0, st>>>(pre, da, dpre, M, Hs, g.ncol, g.rows, g.items, drop, ws)
  if (seed) {
    if (bias_grad) SW_BWD(true, true);
    else SW_BWD(true, false);
  } else {
    if (bias_grad) SW_BWD(false, true);
    else SW_BWD(false, false);
  }
#undef SW_BWD
  if (hipGetLastError() != hipSuccess) return -3;
  if (bias_grad) {
    rc = jm_colsum_add_f32(ws, 2L * Hs, g.nb, 2L * Hs, bias_grad, st);
    if (rc) return rc;
  }
  return 0;
}

JM_DEBUG_EXPORT(swiglu)
