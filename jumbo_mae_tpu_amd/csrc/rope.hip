// Axial 2-D rotary position embedding on the fused QKV tensor (ops/rope.py holds the definition).
//
// qkv is [B, S, 3, H, hd] contiguous; the q and k thirds of every patch row t >= n_cls are rotated in
// place, the v third and the CLS rows are neither read nor written.  Patch index p (t - n_cls, or
// pos[b, t - n_cls]) has coordinates y = p / gw, x = p % gw; channels [0, hd/2) of a head rotate by y,
// [hd/2, hd) by x; adjacent channels (2i, 2i + 1) are pair i with angle coord * theta^(-i / (hd/4)).
// (cos, sin) come from the host's fp32 table [G, hd/4, 2]; per pair o0 = x0 c - x1 s, o1 = x1 c + x0 s
// in fp32, each rounded once to the tensor's dtype (no fma: two products and one add, so that the
// result does not depend on contraction).  inverse: s -> -s, the transpose.
//
// One lane moves 16 bytes -- 8 bf16 = 4 pairs or 4 fp32 = 2 pairs -- and with hd % 16 == 0 a vector
// never straddles a head or the y / x boundary at hd/2.  Consecutive lanes take consecutive vectors
// of the 2 H hd contiguous q|k elements of a row, so a wave reads and writes whole 1 KiB runs.  The
// table (G hd / 2 floats, a few KiB) stays in cache.  No LDS, no atomics; every element has one
// writer and a fixed expression, so reruns are bit-identical.
#include <climits>

#include "common.h"

namespace {

constexpr int ROPE_THREADS = 256;
constexpr int ROPE_MAX_BLOCKS = 2048;  // grid-stride beyond: 8 workgroups per CU

template <typename T>
__global__ __launch_bounds__(ROPE_THREADS) void rope_kernel(T* __restrict__ qkv, const float* __restrict__ table,
                                                            const int* __restrict__ pos, long posB, int S, int n_cls,
                                                            int HD, int hd, int gw, int G, int inverse, long total) {
  constexpr int V = 16 / (int)sizeof(T);  // elements per lane
  const int vpr = 2 * HD / V;             // vectors per row (q and k)
  const int Sp = S - n_cls;
  const int half = hd >> 1;
  for (long i = (long)blockIdx.x * ROPE_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * ROPE_THREADS) {
    const long row = i / vpr;  // patch row over (b, t - n_cls)
    const int c = (int)(i - row * vpr) * V;
    const int b = (int)(row / Sp), tp = (int)(row - (long)b * Sp);
    int p = pos ? pos[b * posB + tp] : tp;
    JM_DASSERT(p >= 0 && p < G * gw);
    p = min(max(p, 0), G * gw - 1);  // the table read stays inside [G, hd/4, 2] whatever pos holds
    const int y = p / gw, x = p - y * gw;
    const int d = c % hd;  // channel within the head; d and hd/2 are multiples of V
    const int coord = d >= half ? x : y;
    const int pair0 = (d >= half ? d - half : d) >> 1;
    const float* cs = table + ((long)coord * (hd >> 2) + pair0) * 2;
    T* ptr = qkv + ((long)b * S + n_cls + tp) * (3L * HD) + c;
    float f[V], t[V], o[V];
    if (V == 8) {
      load8(ptr, f);
      load8(cs, t);
    } else {
      load4(ptr, f);
      load4(cs, t);
    }
#pragma unroll
    for (int j = 0; j < V; j += 2) {
      const float co = t[j], si = inverse ? -t[j + 1] : t[j + 1];
      o[j] = __fsub_rn(__fmul_rn(f[j], co), __fmul_rn(f[j + 1], si));
      o[j + 1] = __fadd_rn(__fmul_rn(f[j + 1], co), __fmul_rn(f[j], si));
    }
    if (V == 8) store8(ptr, o);
    else store4(ptr, o);
  }
}

}  // namespace

int jm_rope_apply(void* qkv, int bf16, int B, int S, int heads, int hd, int n_cls, int gw, const float* table, int G,
                  const int* pos, long posB, int inverse, hipStream_t st) {
  if (B <= 0 || S <= 0 || heads <= 0 || hd <= 0 || hd % 16 != 0 || n_cls < 0 || n_cls > S || gw <= 0 || G <= 0 ||
      table == nullptr || posB < 0)
    return -1;
  if ((long)G * gw > INT_MAX || (long)heads * hd > INT_MAX / 4) return -1;
  const int HD = heads * hd;
  const long rows = (long)B * (S - n_cls);
  if (rows == 0) return 0;
  if (!pos && (long)(S - n_cls) > (long)G * gw) return -1;  // t - n_cls must be a table position
  const int V = bf16 ? 8 : 4;
  const long total = rows * (2 * HD / V);
  const long want = (total + ROPE_THREADS - 1) / ROPE_THREADS;
  const int grid = (int)(want < ROPE_MAX_BLOCKS ? want : ROPE_MAX_BLOCKS);
  if (bf16)
    rope_kernel<uint16_t><<<grid, ROPE_THREADS, 0, st>>>((uint16_t*)qkv, table, pos, posB, S, n_cls, HD, hd, gw, G,
                                                         inverse, total);
  else
    rope_kernel<float><<<grid, ROPE_THREADS, 0, st>>>((float*)qkv, table, pos, posB, S, n_cls, HD, hd, gw, G, inverse,
                                                      total);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

JM_DEBUG_EXPORT(rope)
