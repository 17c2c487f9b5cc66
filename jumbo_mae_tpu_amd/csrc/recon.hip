// MAE reconstruction panels (gfx950): un-patchify the decoder's prediction straight into uint8
// images and score it in pixel space, one 64-lane wave per (image, patch) like the patch kernels
// of mae.hip.
//
//   pred   [B*N, 3p^2] bf16 / fp32, element order (ph, pw, c) (patchify_kernel / patch_pixel)
//   recon  every patch painted from pred;  paste / masked: the original bytes on visible patches,
//          the recon bytes / the fill byte on masked ones;  err [B, N] fp32 = per-patch mean of
//          (x_clamped / 255 - orig / 255)^2 on the clamped, UNROUNDED pixel value x_clamped.
//
// Per element: v = pred (norm_pix: pred sqrt(var + 1e-6) + mean, the inverse of ops/mae.py
// norm_pix, with the biased statistics of the patch's normalized pixels taken from the uint8
// image in two passes: the mean, then the mean squared deviation), x = (v std_c + mean_c) 255,
// clamped to [0, 255] (a NaN becomes 0), byte = round half to even.
//
// The arithmetic is fp64 on the fp32 constants and the stored pred: err is compared per patch to an
// fp64 oracle within one fp32 ulp wherever the fp32 torch composition happens to be that close,
// which fp32 statistics (a patch-wide shift of every x) do not deliver.  The kernel moves ~5 bytes
// and ~25 flops per element and stays bound by its loads and stores.  The wave sums are butterflies
// over fixed lane pairs after a fixed per-lane order: reruns are bit-identical.  Every output
// element is written exactly once; no atomics.
#include "common.h"
#include "jm_api.h"

namespace {

__constant__ float c_mean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float c_std[3] = {0.229f, 0.224f, 0.225f};

// full-wave fp64 sum (the same value in every lane); requires all 64 lanes active
JM_DEVICE double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}

// normalized pixel ((u / 255) - mean_c) / std_c
JM_DEVICE double norm_px(uint32_t u, int c) {
  return ((double)u * (1.0 / 255.0) - (double)c_mean[c]) / (double)c_std[c];
}

// clamped, unrounded pixel value of prediction v (already un-normalized per patch); NaN -> 0
JM_DEVICE double pixel_value(double v, int c) {
  double x = (v * (double)c_std[c] + (double)c_mean[c]) * 255.0;
  x = x > 0.0 ? x : 0.0;
  return x < 255.0 ? x : 255.0;
}

JM_DEVICE void load_pred12(const uint16_t* __restrict__ pr, float* f) {  // 8-byte aligned
#pragma unroll
  for (int q = 0; q < 3; ++q) load4(pr + 4 * q, f + 4 * q);
}
JM_DEVICE void load_pred12(const float* __restrict__ pr, float* f) {  // 16-byte aligned
#pragma unroll
  for (int q = 0; q < 3; ++q) load4(pr + 4 * q, f + 4 * q);
}

// p = 16, 4-byte aligned images with W % 4 == 0 (host checks): the p16_raw lane layout of mae.hip.
// Lane l holds patch row l / 4, pixels 4 (l % 4) .. + 3 of the three channels = the 12 consecutive
// pred elements 12 l + 3 k + c: one 4-byte load and one 4-byte store per channel and output.
template <typename T>
__global__ __launch_bounds__(256) void recon16_kernel(const T* __restrict__ pred, const uint8_t* __restrict__ img,
                                                      const float* __restrict__ mask, long maskB,
                                                      uint8_t* __restrict__ recon, uint8_t* __restrict__ paste,
                                                      uint8_t* __restrict__ masked, float* __restrict__ err,
                                                      long rows, int N, int H, int W, int norm_pix, uint32_t fill4) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int g = W / 16;
  const int b = (int)(row / N), n = (int)(row - (long)b * N);
  const int gy = n / g, gx = n - (n / g) * g;
  float f[12];
  load_pred12(pred + row * 768 + 12 * lane, f);
  const int ph = lane >> 2, pw0 = (lane & 3) * 4;
  long off[3];
  uint32_t px[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    off[c] = (((long)b * 3 + c) * H + gy * 16 + ph) * W + gx * 16 + pw0;
    px[c] = *reinterpret_cast<const uint32_t*>(img + off[c]);
  }
  const bool m = mask[b * maskB + n] > 0.f;
  double mu = 0.0, sd = 1.0;
  if (norm_pix) {
    double t[12], s = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        t[4 * c + k] = norm_px((px[c] >> (8 * k)) & 0xffu, c);
        s += t[4 * c + k];
      }
    mu = wave_sum_f64(s) * (1.0 / 768.0);
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < 12; ++j) q += (t[j] - mu) * (t[j] - mu);
    sd = sqrt(wave_sum_f64(q) * (1.0 / 768.0) + 1e-6);
  }
  double e = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v = (double)f[3 * k + c];
      const double x = pixel_value(norm_pix ? v * sd + mu : v, c);
      const double d = x - (double)((px[c] >> (8 * k)) & 0xffu);
      e += d * d;
      w |= (uint32_t)rint(x) << (8 * k);
    }
    *reinterpret_cast<uint32_t*>(recon + off[c]) = w;
    *reinterpret_cast<uint32_t*>(paste + off[c]) = m ? w : px[c];
    *reinterpret_cast<uint32_t*>(masked + off[c]) = m ? fill4 : px[c];
  }
  e = wave_sum_f64(e);
  if (lane == 0) err[row] = (float)(e * (1.0 / (768.0 * 255.0 * 255.0)));
}

// any even p: lane l takes the elements o = l + 64 j of the patch, byte loads and byte stores
template <typename T>
__global__ __launch_bounds__(256) void recon_kernel(const T* __restrict__ pred, const uint8_t* __restrict__ img,
                                                    const float* __restrict__ mask, long maskB,
                                                    uint8_t* __restrict__ recon, uint8_t* __restrict__ paste,
                                                    uint8_t* __restrict__ masked, float* __restrict__ err, long rows,
                                                    int N, int H, int W, int p, int norm_pix, uint32_t fill) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int P3 = 3 * p * p, g = W / p;
  const int b = (int)(row / N), n = (int)(row - (long)b * N);
  const int gy = n / g, gx = n - (n / g) * g;
  const long base = ((long)b * 3 * H + gy * p) * W + gx * p;  // channel 0, first row of the patch
  const long plane = (long)H * W;
  const bool m = mask[b * maskB + n] > 0.f;
  double mu = 0.0, sd = 1.0;
  if (norm_pix) {
    double s = 0.0;
    for (int o = lane; o < P3; o += 64) {
      const int ph = o / (3 * p), r = o - ph * 3 * p;
      const int pw = r / 3, c = r - (r / 3) * 3;
      s += norm_px(img[base + c * plane + (long)ph * W + pw], c);
    }
    mu = wave_sum_f64(s) / P3;
    double q = 0.0;
    for (int o = lane; o < P3; o += 64) {
      const int ph = o / (3 * p), r = o - ph * 3 * p;
      const int pw = r / 3, c = r - (r / 3) * 3;
      const double dlt = norm_px(img[base + c * plane + (long)ph * W + pw], c) - mu;
      q += dlt * dlt;
    }
    sd = sqrt(wave_sum_f64(q) / P3 + 1e-6);
  }
  double e = 0.0;
  for (int o = lane; o < P3; o += 64) {
    const int ph = o / (3 * p), r = o - ph * 3 * p;
    const int pw = r / 3, c = r - (r / 3) * 3;
    const long a = base + c * plane + (long)ph * W + pw;
    const uint32_t u = img[a];
    const double v = (double)to_f<T>(pred[row * P3 + o]);
    const double x = pixel_value(norm_pix ? v * sd + mu : v, c);
    const double d = x - (double)u;
    e += d * d;
    const uint32_t w = (uint32_t)rint(x);
    recon[a] = (uint8_t)w;
    paste[a] = (uint8_t)(m ? w : u);
    masked[a] = (uint8_t)(m ? fill : u);
  }
  e = wave_sum_f64(e);
  if (lane == 0) err[row] = (float)(e / ((double)P3 * 255.0 * 255.0));
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename T>
int launch(const T* pred, const uint8_t* img, const float* mask, long maskB, uint8_t* recon, uint8_t* paste,
           uint8_t* masked, float* err, int B, int H, int W, int p, int norm_pix, uint32_t fill, hipStream_t st) {
  const int N = (H / p) * (W / p);
  const long rows = (long)B * N;
  const int nb = (int)((rows + 3) / 4);
  if (p == 16 && W % 4 == 0 && aligned(img, 4) && aligned(recon, 4) && aligned(paste, 4) && aligned(masked, 4) &&
      aligned(pred, 4 * sizeof(T)))
    recon16_kernel<T><<<nb, 256, 0, st>>>(pred, img, mask, maskB, recon, paste, masked, err, rows, N, H, W, norm_pix,
                                          fill * 0x01010101u);
  else
    recon_kernel<T><<<nb, 256, 0, st>>>(pred, img, mask, maskB, recon, paste, masked, err, rows, N, H, W, p, norm_pix,
                                        fill);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int jm_recon(const void* pred, int pred_bf16, const uint8_t* img, const float* mask, long maskB, uint8_t* recon,
             uint8_t* paste, uint8_t* masked, float* err, int B, int H, int W, int p, int norm_pix, int fill,
             hipStream_t st) {
  if (p <= 0 || (p & 1) || H <= 0 || W <= 0 || H % p || W % p || B < 0 || fill < 0 || fill > 255) return -1;
  const int N = (H / p) * (W / p);
  if (maskB != 0 && maskB != N) return -1;
  if ((long)B * N > (long)INT32_MAX) return -1;
  if (B == 0) return 0;
  if (pred_bf16)
    return launch(static_cast<const uint16_t*>(pred), img, mask, maskB, recon, paste, masked, err, B, H, W, p, norm_pix,
                  (uint32_t)fill, st);
  return launch(static_cast<const float*>(pred), img, mask, maskB, recon, paste, masked, err, B, H, W, p, norm_pix,
                (uint32_t)fill, st);
}

JM_DEBUG_EXPORT(recon)
