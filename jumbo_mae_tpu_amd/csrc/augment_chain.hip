// Device-side RandAugment / AutoAugment / AugMix / ColorJitter / RandomErasing on the uint8
// [B, 3, S, S] output of rrc_resize (csrc/augment.hip), BIT-EXACT to the PIL calls of
// data/autoaugment.py and data/transforms.py (gfx950).
//
// The loader worker makes the transform's random draws and ships, per image, a chain of op records
// (data/autoaugment.py op_record; data/loader.py DeviceTrainParams).  The chain is applied slot by
// slot between two ping-pong buffers: every image is written in every slot, an identity record is a
// copy.  Per slot:
//
//   aug_stats_kernel  one workgroup per image, working only where the slot's op is autocontrast,
//                     equalize or contrast: the per-channel 256-bin histograms (integer LDS atomics)
//                     -> the band lookup tables of ImageOps.autocontrast / equalize, or the luma sum
//                     -> ImageEnhance.Contrast's mean.  All integer, so exact and run-to-run identical.
//   aug_apply_kernel  block (image, tile of AUG_TILE pixels), thread = pixel (all three channels):
//                     lookup table staged in LDS (from the statistics or the static arguments), the
//                     blend against a degenerate image, the 3x3 smooth + blend, or the affine gather.
//                     Nothing assumes an image fits in LDS.
//
// Arithmetic as Pillow's (data/augment_ref.py is the NumPy mirror and documents it): blends in
// float32, t = d + f (i - d), truncated for 0 <= f <= 1, else clipped and truncated; SMOOTH taps
// k / 13 in float32 summed onto 0.5 row by row; affine source coordinates, bilinear and bicubic in
// double; floating-point contraction off, since one fused multiply-add changes the last bit.
//
// Record (double x AUG_P): kind, argument (bits / threshold / add / blend factor), affine
// coefficients m0..m5, resample (2 bilinear, 3 bicubic), fill r, g, b.  A kind the device does not
// know (the host rejects it in collate) is an identity copy, never an out-of-range access.
//
// AugMix runs its W chains as one op chain over a [B * W] batch of replicas and composites them with
// augmix_mix_kernel; RandomErasing's noise is drawn by the worker (np.random, so the PIL path's
// bytes) and pasted by erase_paste_kernel.  Both are documented at the kernels below.
#include "common.h"
#include "jm_api.h"

namespace {

constexpr int AUG_P = 12;
constexpr int AUG_TILE = 2048;
constexpr int AUG_STAT_WORDS = 193;  // per image: 3 x 256 table bytes (192 words), then the contrast mean
enum AugKind {
  K_IDENTITY = 0, K_INVERT, K_POSTERIZE, K_SOLARIZE, K_SOLARIZE_ADD, K_AUTOCONTRAST, K_EQUALIZE, K_COLOR,
  K_BRIGHTNESS, K_CONTRAST, K_SHARPNESS, K_AFFINE, AUG_KINDS
};

#pragma clang fp contract(off)

JM_DEVICE int aug_kind(const double* rec) {
  const double k = rec[0];
  const bool ok = k >= 0.0 && k < (double)AUG_KINDS && k == floor(k);  // false for NaN
  JM_DASSERT(ok);
  return ok ? (int)k : K_IDENTITY;
}

// integer argument of a record clamped to [lo, hi] (NaN -> lo)
JM_DEVICE int aug_iarg(double v, int lo, int hi) {
  if (!(v >= (double)lo)) return lo;
  if (v >= (double)hi) return hi;
  return (int)v;
}

JM_DEVICE int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__global__ __launch_bounds__(512) void aug_stats_kernel(const uint8_t* __restrict__ in,
                                                        const double* __restrict__ chain, int slots, int slot,
                                                        uint32_t* __restrict__ stats, int S) {
  __shared__ uint32_t hist[768];
  __shared__ uint32_t lsum;
  __shared__ int lo[3], hi[3];
  JM_DGUARD(slot >= 0 && slot < slots && blockDim.x == 512);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int kind = aug_kind(chain + ((long)b * slots + slot) * AUG_P);
  if (kind != K_AUTOCONTRAST && kind != K_EQUALIZE && kind != K_CONTRAST) return;  // workgroup-uniform
  const int n = S * S;
  const uint8_t* ib = in + (long)b * 3 * n;
  uint32_t* sb = stats + (long)b * AUG_STAT_WORDS;
  uint8_t* table = reinterpret_cast<uint8_t*>(sb);

  if (kind == K_CONTRAST) {
    if (tid == 0) lsum = 0;
    __syncthreads();
    uint32_t s = 0;  // 255 x 4096^2 < 2^32
    for (int p = tid; p < n; p += 512) s += (uint32_t)luma(ib[p], ib[n + p], ib[2 * n + p]);
    atomicAdd(&lsum, s);
    __syncthreads();
    if (tid == 0) sb[AUG_STAT_WORDS - 1] = (uint32_t)(int)((double)lsum / (double)n + 0.5);
    return;
  }

  for (int i = tid; i < 768; i += 512) hist[i] = 0;
  if (tid < 3) {
    lo[tid] = 256;
    hi[tid] = -1;
  }
  __syncthreads();
  for (int c = 0; c < 3; ++c)
    for (int p = tid; p < n; p += 512) atomicAdd(&hist[c * 256 + ib[(long)c * n + p]], 1u);
  __syncthreads();

  if (kind == K_AUTOCONTRAST) {
    for (int i = tid; i < 768; i += 512)
      if (hist[i]) {
        atomicMin(&lo[i >> 8], i & 255);
        atomicMax(&hi[i >> 8], i & 255);
      }
    __syncthreads();
    for (int i = tid; i < 768; i += 512) {
      const int c = i >> 8, v = i & 255;
      int o = v;
      if (hi[c] > lo[c]) {
        const double scale = 255.0 / (double)(hi[c] - lo[c]);
        const double offset = (double)(-lo[c]) * scale;
        const double t = (double)v * scale + offset;
        o = t <= 0.0 ? 0 : (t >= 255.0 ? 255 : (int)t);  // int() truncates toward zero: (-1, 0) -> 0
      }
      table[i] = (uint8_t)o;
    }
    return;
  }

  // equalize: one thread per band walks its histogram (256 steps, once per image)
  if (tid < 3) {
    const uint32_t* h = hist + tid * 256;
    uint32_t nonzero = 0, last = 0;
    for (int i = 0; i < 256; ++i)
      if (h[i]) {
        ++nonzero;
        last = h[i];
      }
    const uint32_t step = nonzero > 1 ? ((uint32_t)n - last) / 255u : 0u;
    uint32_t acc = step / 2;
    for (int i = 0; i < 256; ++i) {
      uint32_t o = (uint32_t)i;
      if (step) {
        o = acc / step;
        if (o > 255u) o = 255u;
        acc += h[i];
      }
      table[tid * 256 + i] = (uint8_t)o;
    }
  }
}

// Image.blend(degenerate, image, f) of one byte
JM_DEVICE uint8_t blend8(int d, int i, float f, bool trunc_only) {
  const float t = (float)d + f * (float)(i - d);
  if (!trunc_only) {
    if (t <= 0.f) return 0;
    if (t >= 255.f) return 255;
  }
  return (uint8_t)(int)t;
}

JM_DEVICE double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

JM_DEVICE int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void aug_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                        const double* __restrict__ chain, int slots, int slot,
                                                        const uint32_t* __restrict__ stats, int S) {
  __shared__ uint8_t lut[768];
  JM_DGUARD(slot >= 0 && slot < slots && blockDim.x == 256);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = S * S;
  const int p0 = blockIdx.y * AUG_TILE;
  const int p1 = min(n, p0 + AUG_TILE);
  JM_DASSERT(p0 < n);
  const double* rec = chain + ((long)b * slots + slot) * AUG_P;
  const int kind = aug_kind(rec);  // workgroup-uniform
  const uint8_t* ib = in + (long)b * 3 * n;
  uint8_t* ob = out + (long)b * 3 * n;
  const uint32_t* sb = stats + (long)b * AUG_STAT_WORDS;

  if (kind >= K_INVERT && kind <= K_EQUALIZE) {
    if (kind == K_AUTOCONTRAST || kind == K_EQUALIZE) {
      const uint8_t* table = reinterpret_cast<const uint8_t*>(sb);
      for (int i = tid; i < 768; i += 256) lut[i] = table[i];
    } else {
      int o = tid;
      if (kind == K_INVERT) {
        o = 255 - tid;
      } else if (kind == K_POSTERIZE) {
        o = tid & ~((1 << (8 - aug_iarg(rec[1], 0, 8))) - 1);
      } else if (kind == K_SOLARIZE) {
        o = tid < aug_iarg(rec[1], 0, 256) ? tid : 255 - tid;
      } else {  // K_SOLARIZE_ADD, threshold 128
        o = tid < 128 ? min(tid + aug_iarg(rec[1], 0, 255), 255) : tid;
      }
      lut[tid] = lut[256 + tid] = lut[512 + tid] = (uint8_t)o;
    }
    __syncthreads();
    for (int p = p0 + tid; p < p1; p += 256) {
      ob[p] = lut[ib[p]];
      ob[n + p] = lut[256 + ib[n + p]];
      ob[2 * n + p] = lut[512 + ib[2 * n + p]];
    }
    return;
  }

  if (kind >= K_COLOR && kind <= K_SHARPNESS) {
    const float f = (float)rec[1];
    const bool trunc_only = f >= 0.f && f <= 1.f;
    const int mean = kind == K_CONTRAST ? clampi((int)sb[AUG_STAT_WORDS - 1], 255) : 0;
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    for (int p = p0 + tid; p < p1; p += 256) {
      int v[3] = {ib[p], ib[n + p], ib[2 * n + p]};
      int d[3] = {mean, mean, mean};  // brightness: black; contrast: the mean luma
      if (kind == K_COLOR) {
        d[0] = d[1] = d[2] = luma(v[0], v[1], v[2]);
      } else if (kind == K_SHARPNESS) {
        const int y = p / S, x = p - y * S;
        if (x == 0 || y == 0 || x == S - 1 || y == S - 1) {
          d[0] = v[0], d[1] = v[1], d[2] = v[2];  // ImageFilter copies the one-pixel border
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const uint8_t* q = ib + (long)c * n + p;
            float ss = 0.5f;
            ss = ss + (((float)q[-S - 1] * k1 + (float)q[-S] * k1) + (float)q[-S + 1] * k1);
            ss = ss + (((float)q[-1] * k1 + (float)q[0] * k5) + (float)q[1] * k1);
            ss = ss + (((float)q[S - 1] * k1 + (float)q[S] * k1) + (float)q[S + 1] * k1);
            d[c] = ss <= 0.f ? 0 : (ss >= 255.f ? 255 : (int)ss);
          }
        }
      }
      ob[p] = blend8(d[0], v[0], f, trunc_only);
      ob[n + p] = blend8(d[1], v[1], f, trunc_only);
      ob[2 * n + p] = blend8(d[2], v[2], f, trunc_only);
    }
    return;
  }

  const int resample = kind == K_AFFINE ? aug_iarg(rec[8], 0, 4) : 0;
  if (kind == K_AFFINE) JM_DASSERT(resample == 2 || resample == 3);
  if (kind == K_AFFINE && (resample == 2 || resample == 3)) {
    const double m0 = rec[2], m1 = rec[3], m2 = rec[4], m3 = rec[5], m4 = rec[6], m5 = rec[7];
    const uint8_t fill[3] = {(uint8_t)aug_iarg(rec[9], 0, 255), (uint8_t)aug_iarg(rec[10], 0, 255),
                             (uint8_t)aug_iarg(rec[11], 0, 255)};
    for (int p = p0 + tid; p < p1; p += 256) {
      const int y = p / S, x = p - y * S;
      double xin = (m0 * (x + 0.5) + m1 * (y + 0.5)) + m2;
      double yin = (m3 * (x + 0.5) + m4 * (y + 0.5)) + m5;
      const bool inside = xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S;  // false for NaN
      if (!inside) {
        ob[p] = fill[0];
        ob[n + p] = fill[1];
        ob[2 * n + p] = fill[2];
        continue;
      }
      xin -= 0.5;
      yin -= 0.5;
      const int xf = (int)floor(xin), yf = (int)floor(yin);  // in [-1, S - 1]
      const double dx = xin - xf, dy = yin - yf;
      JM_DASSERT(xf >= -1 && xf < S && yf >= -1 && yf < S);
      if (resample == 2) {
        const int xa = clampi(xf, S - 1), xb = clampi(xf + 1, S - 1);
        const int ya = clampi(yf, S - 1) * S, yb = clampi(yf + 1, S - 1) * S;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint8_t* q = ib + (long)c * n;
          const double l0 = q[ya + xa], r0 = q[ya + xb], l1 = q[yb + xa], r1 = q[yb + xb];
          const double v1 = l0 + (r0 - l0) * dx;
          const double v2 = l1 + (r1 - l1) * dx;
          ob[(long)c * n + p] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
        }
      } else {
        int xs[4], ys[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xs[k] = clampi(xf - 1 + k, S - 1);
          ys[k] = clampi(yf - 1 + k, S - 1) * S;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint8_t* q = ib + (long)c * n;
          double r[4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            r[k] = cubic(q[ys[k] + xs[0]], q[ys[k] + xs[1]], q[ys[k] + xs[2]], q[ys[k] + xs[3]], dx);
          const double v = cubic(r[0], r[1], r[2], r[3], dy);
          ob[(long)c * n + p] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (uint8_t)(int)v);
        }
      }
    }
    return;
  }

  // identity (and anything unknown): copy
  for (int p = p0 + tid; p < p1; p += 256) {
    ob[p] = ib[p];
    ob[n + p] = ib[n + p];
    ob[2 * n + p] = ib[2 * n + p];
  }
}

// ---- AugMix mixing and random erasing (data/autoaugment.py AugMix, data/transforms.py RandomErasing)
constexpr int MIX_WMAX = 8;
constexpr int ERASE_TILE = 2048;

template <int NB> struct ByteVec;
template <> struct ByteVec<1> { using T = uint8_t; };
template <> struct ByteVec<4> { using T = uint32_t; };
template <> struct ByteVec<16> { using T = uint4; };

template <int NB> JM_DEVICE void load_bytes(const uint8_t* p, uint8_t* v) {
  const typename ByteVec<NB>::T t = *reinterpret_cast<const typename ByteVec<NB>::T*>(p);
  __builtin_memcpy(v, &t, NB);
}

template <int NB> JM_DEVICE void store_bytes(uint8_t* p, const uint8_t* v) {
  typename ByteVec<NB>::T t;
  __builtin_memcpy(&t, v, NB);
  *reinterpret_cast<typename ByteVec<NB>::T*>(p) = t;
}

// AugMix's composite of an image with its W augmented chains.  block (tile of 256 x NB bytes, image),
// thread = NB consecutive bytes of the image's 3 S S (n3): one NB-byte load from the original and
// from each chain, one NB-byte store.  NB is the widest of 16 / 4 / 1 that divides n3 and every base
// pointer (the launcher picks it), so every image's and chain's offset is aligned and no thread
// straddles the end of an image: NB = 1 is the scalar path of an odd S.
//   table float [B, W + 1].  Not blended: the weights w_k and m --
//     mixed = 0; mixed = mixed + w_k * x_k (float32, multiply and add rounded separately, chain
//     order); clip to [0, 255], truncate; Image.blend(original, mixed, m).
//   Blended: the alphas a_k in application order -- img = Image.blend(img, x_k, a_k), rounded to a
//     byte after every step.
template <int NB>
__global__ __launch_bounds__(256) void augmix_mix_kernel(const uint8_t* __restrict__ orig,
                                                         const uint8_t* __restrict__ chains,
                                                         const float* __restrict__ table, uint8_t* __restrict__ out,
                                                         int W, int blended, long n3) {
  JM_DGUARD(blockDim.x == 256 && W >= 1 && W <= MIX_WMAX && n3 % NB == 0);
  const int b = blockIdx.y;
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * NB;
  if (e >= n3) return;
  const float* tb = table + (long)b * (W + 1);
  const uint8_t* xb = chains + (long)b * W * n3 + e;
  uint8_t o[NB], x[NB], r[NB];
  load_bytes<NB>(orig + (long)b * n3 + e, o);
  if (blended) {
#pragma unroll
    for (int q = 0; q < NB; ++q) r[q] = o[q];
    for (int k = 0; k < W; ++k) {
      const float a = tb[k];
      const bool trunc_only = a >= 0.f && a <= 1.f;
      load_bytes<NB>(xb + (long)k * n3, x);
#pragma unroll
      for (int q = 0; q < NB; ++q) r[q] = blend8(r[q], x[q], a, trunc_only);
    }
  } else {
    float acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = 0.f;
    for (int k = 0; k < W; ++k) {
      const float w = tb[k];
      load_bytes<NB>(xb + (long)k * n3, x);
#pragma unroll
      for (int q = 0; q < NB; ++q) acc[q] = acc[q] + w * (float)x[q];
    }
    const float m = tb[W];
    const bool trunc_only = m >= 0.f && m <= 1.f;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int mixed = acc[q] >= 255.f ? 255 : (acc[q] > 0.f ? (int)acc[q] : 0);  // NaN -> 0
      r[q] = blend8(o[q], mixed, m, trunc_only);
    }
  }
  store_bytes<NB>(out + (long)b * n3 + e, r);
}

// RandomErasing's paste, in place.  block (tile of ERASE_TILE bytes of the box, image); table int64
// [B, 5]: box row i, column j, rows eh, columns ew, offset of its [3, eh, ew] fill bytes in ``fill``.
// eh == 0: the image is not erased.  A record that does not describe a box inside the image with its
// bytes inside ``fill`` (the host rejects it in collate) erases nothing, so no record can make this
// kernel read or write out of bounds.
__global__ __launch_bounds__(256) void erase_paste_kernel(uint8_t* __restrict__ images,
                                                          const int64_t* __restrict__ table,
                                                          const uint8_t* __restrict__ fill, long fill_len, int S) {
  JM_DGUARD(blockDim.x == 256);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t* t = table + (long)b * 5;
  const int64_t i = t[0], j = t[1], eh = t[2], ew = t[3], off = t[4];
  if (eh == 0) return;  // workgroup-uniform
  const bool ok = eh > 0 && eh < S && ew > 0 && ew < S && i >= 0 && i <= S - eh && j >= 0 && j <= S - ew && off >= 0 &&
                  off <= fill_len - 3 * eh * ew;
  JM_DASSERT(ok);
  if (!ok) return;  // workgroup-uniform
  const int w = (int)ew, area = (int)eh * w, nb = 3 * area;
  const int p0 = blockIdx.x * ERASE_TILE;
  if (p0 >= nb) return;  // the grid covers the largest box of the batch
  const int p1 = min(nb, p0 + ERASE_TILE);
  const long n = (long)S * S;
  const uint8_t* fb = fill + off;
  uint8_t* ob = images + (long)b * 3 * n + (long)i * S + j;
  for (int p = p0 + tid; p < p1; p += 256) {
    const int c = p / area, q = p - c * area;
    const int y = q / w, x = q - y * w;
    ob[(long)c * n + (long)y * S + x] = fb[p];
  }
}

}  // namespace

int jm_aug_stat_words() { return AUG_STAT_WORDS; }
int jm_aug_record_len() { return AUG_P; }

// images / scratch: uint8 [B, 3, S, S] ping-pong buffers (images holds the input, both are
// overwritten); chain: double [B, slots, AUG_P]; stats: uint32 [B, AUG_STAT_WORDS].  Returns the
// buffer that holds the result (0: images, 1: scratch), or <0 on bad arguments.  Stream-ordered.
int jm_aug_chain(uint8_t* images, uint8_t* scratch, const double* chain, int B, int slots, int S, uint32_t* stats,
                 hipStream_t st) {
  if (B <= 0 || slots < 0 || S <= 0 || S > 4096) return -1;
  uint8_t* src = images;
  uint8_t* dst = scratch;
  const int tiles = (S * S + AUG_TILE - 1) / AUG_TILE;
  for (int s = 0; s < slots; ++s) {
    aug_stats_kernel<<<B, 512, 0, st>>>(src, chain, slots, s, stats, S);
    aug_apply_kernel<<<dim3(B, tiles), 256, 0, st>>>(src, dst, chain, slots, s, stats, S);
    uint8_t* t = src;
    src = dst;
    dst = t;
  }
  return src == images ? 0 : 1;
}

// orig / out: uint8 [B, 3, S, S]; chains: uint8 [B * W, 3, S, S], chain k of image b at b * W + k;
// table: float [B, W + 1] (augmix_mix_kernel).  out must not alias an input.  Stream-ordered.
int jm_augmix_mix(const uint8_t* orig, const uint8_t* chains, const float* table, uint8_t* out, int B, int W, int S,
                  int blended, hipStream_t st) {
  if (B <= 0 || B > 65535 || W < 1 || W > MIX_WMAX || S <= 0 || S > 4096) return -1;
  const long n3 = 3L * S * S;
  const uintptr_t al = (uintptr_t)orig | (uintptr_t)chains | (uintptr_t)out | (uintptr_t)n3;
  if ((al & 15) == 0) {
    augmix_mix_kernel<16><<<dim3((unsigned)((n3 / 16 + 255) / 256), B), 256, 0, st>>>(orig, chains, table, out, W,
                                                                                      blended, n3);
  } else if ((al & 3) == 0) {
    augmix_mix_kernel<4><<<dim3((unsigned)((n3 / 4 + 255) / 256), B), 256, 0, st>>>(orig, chains, table, out, W,
                                                                                    blended, n3);
  } else {
    augmix_mix_kernel<1><<<dim3((unsigned)((n3 + 255) / 256), B), 256, 0, st>>>(orig, chains, table, out, W, blended,
                                                                                n3);
  }
  return 0;
}

// images: uint8 [B, 3, S, S], erased in place; table: int64 [B, 5]; fill: fill_len bytes
// (erase_paste_kernel).  box_bytes_max: the largest 3 eh ew of the batch's boxes, which sizes the
// grid (0: the largest box there can be, 3 (S - 1)^2).  Stream-ordered.
int jm_erase_paste(uint8_t* images, const int64_t* table, const uint8_t* fill, long fill_len, int B, int S,
                   long box_bytes_max, hipStream_t st) {
  if (B <= 0 || B > 65535 || S <= 0 || S > 4096 || fill_len < 0 || box_bytes_max < 0) return -1;
  const long limit = 3L * (S - 1) * (S - 1);
  const long bytes = box_bytes_max == 0 || box_bytes_max > limit ? limit : box_bytes_max;
  if (bytes == 0) return 0;  // S == 1: no box fits
  erase_paste_kernel<<<dim3((unsigned)((bytes + ERASE_TILE - 1) / ERASE_TILE), B), 256, 0, st>>>(images, table, fill,
                                                                                                fill_len, S);
  return 0;
}

JM_DEBUG_EXPORT(augment_chain)
