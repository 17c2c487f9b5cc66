// PyTorch bindings of the jumbo_mae_tpu_amd HIP kernels.
// Kernels live in *.hip translation units with a plain pointer + hipStream_t interface; this file
// only validates tensors, allocates outputs with the caching allocator and launches on the
// current HIP stream (so everything is HIP-graph capturable).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <array>
#include <climits>

#include "jm_api.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_DT(x, d) TORCH_CHECK((x).scalar_type() == (d), #x " has wrong dtype")

const uint16_t* bf(const torch::Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* bfm(torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }
uint16_t* bfp(const torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }
const float* fopt(const c10::optional<torch::Tensor>& t) {
  return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr;
}
float* fopt_m(c10::optional<torch::Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr; }

void check_rc(int rc, const char* what) { TORCH_CHECK(rc == 0, what, ": unsupported shape (rc=", rc, ")"); }

// dropout: keep threshold on 16 hash bits (common.h drop_keep) and the 1/keep scale of a drop
// rate in [0, 1)
static std::pair<uint32_t, float> keep_params(double rate) {
  TORCH_CHECK(rate >= 0.0 && rate < 1.0, "dropout rate must be in [0, 1)");
  const double keep = 1.0 - rate;
  return {(uint32_t)std::llround(keep * 65536.0), (float)(1.0 / keep)};
}

static void check_seed(const torch::Tensor& seed, const torch::Tensor& like) {
  TORCH_CHECK(seed.scalar_type() == torch::kInt64 && seed.numel() == 1 && seed.device() == like.device(),
              "dropout seed: int64 [1] on the data's device");
}

// Dense-output dropout descriptor for the residual kernels: seed null / rate 0 = none; ioff = the
// element offset of y's view within the branch tensor the mask indexes
JmDrop make_drop(const c10::optional<torch::Tensor>& seed, double rate, const torch::Tensor& like, int64_t ioff) {
  if (!seed.has_value() || !seed->defined() || rate <= 0.0) return JmDrop{nullptr, 0u, 1.f, 0};
  check_seed(*seed, like);
  const auto kp = keep_params(rate);
  return JmDrop{seed->data_ptr<int64_t>(), kp.first, kp.second, (long)ioff};
}

// ------------------------------------------------------------------------------ layernorm
// also_bf16 (fp32 output only): a bf16 copy of y written by the same pass, returned 4th
std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor gamma, torch::Tensor beta, double eps,
                                         py::object out_dtype, bool also_bf16) {
  CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 3 && x.stride(2) == 1, "x must be [B,T,D] with contiguous last dim");
  CHECK_DT(x, torch::kFloat32);
  CHECK_CONTIG(gamma);
  CHECK_CONTIG(beta);
  const auto odt = torch::python::detail::py_object_to_dtype(out_dtype);
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  auto y = torch::empty({(long)B * T, D}, x.options().dtype(odt));
  auto mean = torch::empty({(long)B * T}, x.options());
  auto rstd = torch::empty({(long)B * T}, x.options());
  TORCH_CHECK(odt == torch::kBFloat16 || odt == torch::kFloat32, "out dtype must be bf16/fp32");
  TORCH_CHECK(!also_bf16 || odt == torch::kFloat32, "also_bf16 needs an fp32 output");
  torch::Tensor y2;
  if (also_bf16) y2 = torch::empty({(long)B * T, D}, x.options().dtype(torch::kBFloat16));
  check_rc(jm_layernorm_fwd(x.data_ptr<float>(), x.stride(0), x.stride(1), B, T, D, gamma.data_ptr<float>(),
                            beta.data_ptr<float>(), (float)eps, y.data_ptr(), odt == torch::kBFloat16,
                            mean.data_ptr<float>(), rstd.data_ptr<float>(), stream(), also_bf16 ? bfm(y2) : nullptr),
           "layernorm_fwd");
  if (also_bf16) return {y, mean, rstd, y2};
  return {y, mean, rstd};
}

// res_*: optional fused residual backward of the consumer of dx (see JmLnRes); returns [dx] or
// [dx, dy_res] (dy_res written into res_out, a [B, T - T0, D] view, or a new [B*(T-T0), D] tensor)
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor mean, torch::Tensor rstd,
                                         torch::Tensor gamma, torch::Tensor dgamma, torch::Tensor dbeta, bool accum,
                                         c10::optional<torch::Tensor> dres, c10::optional<torch::Tensor> out,
                                         c10::optional<torch::Tensor> res_y, c10::optional<torch::Tensor> res_scale,
                                         c10::optional<torch::Tensor> res_mask, c10::optional<torch::Tensor> res_dscale,
                                         c10::optional<torch::Tensor> res_dbias, int64_t res_T0,
                                         c10::optional<torch::Tensor> res_out, c10::optional<torch::Tensor> res_seed,
                                         double res_rate, int64_t res_ioff, c10::optional<torch::Tensor> hx,
                                         c10::optional<torch::Tensor> beta) {
  CHECK_CONTIG(dy);
  TORCH_CHECK(x.dim() == 3 && x.stride(2) == 1, "x must be [B,T,D]");
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  TORCH_CHECK(dy.numel() == (long)B * T * D, "dy shape");
  torch::Tensor dx;
  if (out.has_value() && out->defined()) {
    dx = *out;
    TORCH_CHECK(dx.dim() == 3 && dx.size(0) == B && dx.size(1) == T && dx.size(2) == D && dx.stride(2) == 1, "out view");
  } else {
    dx = torch::empty({B, T, D}, x.options());
  }
  const float* rp = nullptr;
  long rB = 0, rT = 0;
  if (dres.has_value() && dres->defined()) {
    TORCH_CHECK(dres->dim() == 3 && dres->size(0) == B && dres->size(1) == T && dres->stride(2) == 1, "dres view");
    rp = dres->data_ptr<float>();
    rB = dres->stride(0);
    rT = dres->stride(1);
  }
  const bool dyb = dy.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(dyb || dy.scalar_type() == torch::kFloat32, "dy dtype");
  const bool has_res = res_y.has_value() && res_y->defined();
  JmLnRes res{};
  torch::Tensor dyr;
  if (has_res) {
    const int Tr = T - (int)res_T0;
    TORCH_CHECK(res_T0 >= 0 && Tr > 0, "res_T0");
    const auto& y = *res_y;
    CHECK_DT(y, torch::kBFloat16);
    long yB, yT;
    if (y.dim() == 3) {  // [B, Tr, D] view
      TORCH_CHECK(y.size(0) == B && y.size(1) == Tr && y.size(2) == D && y.stride(2) == 1, "res_y view");
      yB = y.stride(0);
      yT = y.stride(1);
    } else {
      TORCH_CHECK(y.is_contiguous() && y.numel() == (long)B * Tr * D, "res_y shape");
      yB = (long)Tr * D;
      yT = D;
    }
    if (res_out.has_value() && res_out->defined()) {  // same view layout as y (e.g. rows of a shared buffer)
      dyr = *res_out;
      CHECK_DT(dyr, torch::kBFloat16);
      TORCH_CHECK(dyr.sizes() == y.sizes() && dyr.strides() == y.strides(), "res_out must match res_y's view");
    } else {
      TORCH_CHECK(y.is_contiguous(), "res_y view needs res_out");
      dyr = torch::empty_like(y);
    }
    res = JmLnRes{bf(y), bfm(dyr), yB, yT, fopt(res_scale), fopt(res_mask), (int)res_T0, fopt_m(res_dscale),
                  fopt_m(res_dbias), make_drop(res_seed, res_rate, y, res_ioff)};
  }
  const uint16_t* hxp = nullptr;
  const float* betap = nullptr;
  if (hx.has_value() && hx->defined()) {  // the forward's bf16 LN output, rows like dy
    CHECK_DT((*hx), torch::kBFloat16);
    CHECK_CONTIG((*hx));
    TORCH_CHECK(hx->numel() == (long)B * T * D, "hx shape");
    TORCH_CHECK(beta.has_value() && beta->defined() && beta->numel() == D, "hx needs beta [D]");
    CHECK_DT((*beta), torch::kFloat32);
    hxp = bf(*hx);
    betap = beta->data_ptr<float>();
  }
  const int NP = has_res ? 4 : 2;
  auto ws = torch::empty({(accum || has_res) ? (long)jm_layernorm_bwd_blocks(B * T, D) * NP * D : 1}, x.options());
  check_rc(jm_layernorm_bwd(dy.data_ptr(), dyb, x.data_ptr<float>(), x.stride(0), x.stride(1), B, T, D,
                            mean.data_ptr<float>(), rstd.data_ptr<float>(), gamma.data_ptr<float>(),
                            dx.data_ptr<float>(), dx.stride(0), dx.stride(1), rp, rB, rT, dgamma.data_ptr<float>(),
                            dbeta.data_ptr<float>(), accum, ws.data_ptr<float>(), has_res ? &res : nullptr,
                            stream(), hxp, betap),
           "layernorm_bwd");
  if (has_res) return {dx, dyr};
  return {dx};
}

// ------------------------------------------------------------------------------ elementwise
torch::Tensor gelu_fwd(torch::Tensor h) {
  CHECK_CONTIG(h);
  CHECK_DT(h, torch::kBFloat16);
  auto a = torch::empty_like(h);
  check_rc(jm_gelu_fwd(bf(h), bfm(a), h.numel(), stream()), "gelu_fwd");
  return a;
}

// deriv: h holds the saved gelu'(pre-activation) (EPI_GELU_D forward) -> dh = da * h
// partial-row workspace of the column-reducing elementwise kernels (their fixed-order bias /
// scale gradient sums); a caching-allocator temporary on the current stream
static torch::Tensor rowcol_ws(const torch::Tensor& like, int M, int N, int nacc) {
  const long n = jm_rowcol_ws_floats(M, N, nacc);
  return torch::empty({n > 0 ? n : 1}, like.options().dtype(torch::kFloat32));
}

torch::Tensor gelu_bwd(torch::Tensor h, torch::Tensor da, c10::optional<torch::Tensor> bias_grad, bool deriv) {
  CHECK_CONTIG(h);
  CHECK_CONTIG(da);
  CHECK_DT(h, torch::kBFloat16);
  CHECK_DT(da, torch::kBFloat16);
  const int N = h.size(-1);
  const int M = h.numel() / N;
  auto dh = torch::empty_like(h);
  float* bg = fopt_m(bias_grad);
  torch::Tensor ws;
  if (bg) ws = rowcol_ws(h, M, N, 1);
  check_rc(jm_gelu_bwd(bf(h), bf(da), bfm(dh), bg, M, N, stream(), deriv ? 1 : 0, bg ? ws.data_ptr<float>() : nullptr),
           "gelu_bwd");
  return dh;
}

void colsum(torch::Tensor x, torch::Tensor acc) {
  CHECK_CONTIG(x);
  CHECK_DT(x, torch::kBFloat16);
  const int N = x.size(-1);
  const int M = x.numel() / N;
  auto ws = rowcol_ws(x, M, N, 1);
  check_rc(jm_colsum_bf16(bf(x), acc.data_ptr<float>(), M, N, stream(), ws.data_ptr<float>()), "colsum");
}

void splitk_reduce_add(torch::Tensor part, torch::Tensor g) {
  CHECK_CONTIG(part);
  TORCH_CHECK(g.is_contiguous() && g.numel() * part.size(0) == part.numel(), "splitk_reduce_add shapes");
  check_rc(jm_splitk_reduce_add(part.data_ptr<float>(), g.data_ptr<float>(), g.numel(), part.size(0), stream()),
           "splitk_reduce_add");
}

// g += x.sum(0) for a 2-D fp32 view with unit column stride (any row stride), no torch reduce
void colsum_add_f32(torch::Tensor x, torch::Tensor g) {
  CHECK_CUDA(x);
  CHECK_DT(x, torch::kFloat32);
  CHECK_DT(g, torch::kFloat32);
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1 && g.is_contiguous() && g.numel() == x.size(1),
              "colsum_add_f32: x [rows, n] with unit column stride, g [n]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0,
              "colsum_add_f32: 16-byte aligned operands");
  check_rc(jm_colsum_add_f32(x.data_ptr<float>(), x.stride(0), x.size(0), x.size(1), g.data_ptr<float>(), stream()),
           "colsum_add_f32");
}

torch::Tensor residual_fwd(torch::Tensor x, torch::Tensor y, c10::optional<torch::Tensor> scale,
                           c10::optional<torch::Tensor> mask, c10::optional<torch::Tensor> out_opt,
                           c10::optional<torch::Tensor> seed, double rate, int64_t ioff) {
  TORCH_CHECK(x.dim() == 3 && x.stride(2) == 1, "x must be [B,T,D]");
  CHECK_DT(x, torch::kFloat32);
  CHECK_CONTIG(y);
  CHECK_DT(y, torch::kBFloat16);
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  torch::Tensor out;
  if (out_opt.has_value() && out_opt->defined()) {
    out = *out_opt;
    TORCH_CHECK(out.dim() == 3 && out.size(0) == B && out.size(1) == T && out.size(2) == D && out.stride(2) == 1,
                "out view");
  } else {
    out = torch::empty({B, T, D}, x.options());
  }
  check_rc(jm_residual_fwd(x.data_ptr<float>(), x.stride(0), x.stride(1), B, T, D, bf(y), fopt(scale), fopt(mask),
                           out.data_ptr<float>(), out.stride(0), out.stride(1), stream(),
                           make_drop(seed, rate, y, ioff)),
           "residual_fwd");
  return out;
}

// y / out: contiguous [B*T, D] or [B, T, D] views (out must then share y's strides; out given
// with y absent: its own strides)
torch::Tensor residual_bwd(torch::Tensor dout, c10::optional<torch::Tensor> y, c10::optional<torch::Tensor> scale,
                           c10::optional<torch::Tensor> mask, c10::optional<torch::Tensor> dscale, py::object ydtype,
                           c10::optional<torch::Tensor> dbias, c10::optional<torch::Tensor> out,
                           c10::optional<torch::Tensor> seed, double rate, int64_t ioff) {
  TORCH_CHECK(dout.dim() == 3 && dout.stride(2) == 1, "dout must be a [B,T,D] view");
  CHECK_DT(dout, torch::kFloat32);
  const int B = dout.size(0), T = dout.size(1), D = dout.size(2);
  const auto odt = torch::python::detail::py_object_to_dtype(ydtype);
  TORCH_CHECK(odt == torch::kBFloat16, "residual_bwd: y must be bf16");
  const bool has_y = y.has_value() && y->defined();
  auto strides_of = [&](const torch::Tensor& t, long& sb, long& st_) {
    if (t.dim() == 3) {
      TORCH_CHECK(t.size(0) == B && t.size(1) == T && t.size(2) == D && t.stride(2) == 1, "residual_bwd view");
      sb = t.stride(0);
      st_ = t.stride(1);
    } else {
      TORCH_CHECK(t.is_contiguous() && t.numel() == (long)B * T * D, "residual_bwd shape");
      sb = (long)T * D;
      st_ = D;
    }
  };
  long yB = (long)T * D, yT = D;
  if (has_y) strides_of(*y, yB, yT);
  torch::Tensor dy;
  if (out.has_value() && out->defined()) {
    dy = *out;
    CHECK_DT(dy, odt);
    long oB, oT;
    strides_of(dy, oB, oT);
    if (has_y) {
      TORCH_CHECK(oB == yB && oT == yT, "residual_bwd: out must share y's strides");
    } else {
      yB = oB;
      yT = oT;
    }
  } else {
    TORCH_CHECK(yB == (long)T * D && yT == D, "residual_bwd: a strided y needs out");
    dy = torch::empty({(long)B * T, D}, dout.options().dtype(odt));
  }
  torch::Tensor ws;
  const bool sums = (dscale && dscale->defined()) || (dbias && dbias->defined());
  if (sums) ws = rowcol_ws(dout, B * T, D, 2);
  check_rc(jm_residual_bwd(dout.data_ptr<float>(), dout.stride(0), dout.stride(1), has_y ? bf(*y) : nullptr,
                           fopt(scale), fopt(mask), fopt_m(dscale), bfm(dy), B, T, D, fopt_m(dbias), yB, yT,
                           stream(), make_drop(seed, rate, dout, ioff), sums ? ws.data_ptr<float>() : nullptr),
           "residual_bwd");
  return dy;
}

// ------------------------------------------------------------------------------ attention
// seed (int64 [1] on the device) with rate > 0: dropout on the attention probabilities (mask:
// common.h drop_keep at ((b H + h) S + q) SE + k, the backward regenerates it from the same seed)
static std::tuple<const int64_t*, uint32_t, float> attn_drop(const c10::optional<torch::Tensor>& seed, double rate,
                                                             const torch::Tensor& like) {
  if (!seed.has_value() || !seed->defined() || rate <= 0.0) return {nullptr, 0u, 1.f};
  check_seed(*seed, like);
  const auto kp = keep_params(rate);
  return {seed->data_ptr<int64_t>(), kp.first, kp.second};
}

// head dims with HIP attention kernels
py::tuple attn_head_dims() {
  const int* d = nullptr;
  const int n = jm_attn_head_dims(&d);
  py::tuple t(n);
  for (int i = 0; i < n; ++i) t[i] = py::int_(d[i]);
  return t;
}

// whether attn_bwd accepts dbias at (S, hd): the whole-sequence kernels fuse the QKV bias gradient,
// the tile-streamed ones (S > attn_max_seq(), head dims 80 / 96 / 128 at any S) leave it to the caller
bool attn_fused_bias(int64_t S, int64_t hd) { return jm_attn_fused_bias((int)S, (int)hd) != 0; }

// whether attn_fwd / attn_bwd take a dropout seed at (S, hd): wherever there is a kernel
bool attn_dropout(int64_t S, int64_t hd) { return jm_attn_dropout((int)S, (int)hd) != 0; }

static void check_attn_shape(const torch::Tensor& qkv, int64_t heads, const char* what) {
  TORCH_CHECK(qkv.dim() == 3 && heads > 0 && qkv.size(2) % (3 * heads) == 0, what,
              ": qkv must be [B, S, 3 * heads * hd]");
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t heads, c10::optional<torch::Tensor> seed, double rate) {
  CHECK_CONTIG(qkv);
  CHECK_DT(qkv, torch::kBFloat16);
  check_attn_shape(qkv, heads, "attn_fwd");
  const int B = qkv.size(0), S = qkv.size(1), D3 = qkv.size(2);
  const int D = D3 / 3, hd = D / heads;
  auto o = torch::empty({B, S, D}, qkv.options());
  auto lse = torch::empty({B, (long)heads, S}, qkv.options().dtype(torch::kFloat32));
  const auto dr = attn_drop(seed, rate, qkv);
  check_rc(jm_attn_fwd(bf(qkv), bfm(o), lse.data_ptr<float>(), B, S, heads, hd, std::get<0>(dr), std::get<1>(dr),
                       std::get<2>(dr), stream()),
           "attn_fwd");
  return {o, lse};
}

// dbias (optional, fp32 [3D]) += column sums of dqkv (the QKV Dense bias gradient), taken from
// the kernel's fp32 accumulators as per-sample partials and reduced here.
torch::Tensor attn_bwd(torch::Tensor dO, torch::Tensor qkv, torch::Tensor o, torch::Tensor lse, int64_t heads,
                       c10::optional<torch::Tensor> dbias, c10::optional<torch::Tensor> seed, double rate) {
  CHECK_CONTIG(dO);
  CHECK_CONTIG(qkv);
  CHECK_CONTIG(o);
  CHECK_DT(dO, torch::kBFloat16);
  check_attn_shape(qkv, heads, "attn_bwd");
  const int B = qkv.size(0), S = qkv.size(1), D3 = qkv.size(2);
  const int D = D3 / 3, hd = D / heads;
  TORCH_CHECK(dO.numel() == (long)B * S * D && o.numel() == (long)B * S * D && lse.numel() == (long)B * heads * S,
              "attn_bwd: dO / o must hold [B, S, D] and lse [B, H, S]");
  auto dqkv = torch::empty_like(qkv);
  const auto dr = attn_drop(seed, rate, qkv);
  if (jm_attn_tiled(S, hd)) {  // tile-streamed kernels; the caller reduces the bias gradient
    TORCH_CHECK(!dbias, "attn_bwd: no fused bias gradient at S = ", S, ", head dim ", hd,
                " (tile-streamed kernels; see attn_fused_bias)");
    auto delta = torch::empty({B, (long)heads, S}, qkv.options().dtype(torch::kFloat32));
    check_rc(jm_attn_bwd_long(bf(qkv), bf(o), bf(dO), lse.data_ptr<float>(), bfm(dqkv), delta.data_ptr<float>(), B,
                              S, heads, hd, std::get<0>(dr), std::get<1>(dr), std::get<2>(dr), stream()),
             "attn_bwd (long)");
    return dqkv;
  }
  torch::Tensor part;
  const int rows = jm_attn_bwd_part_rows(B, S, hd);
  if (dbias) {
    TORCH_CHECK(dbias->is_contiguous() && dbias->scalar_type() == torch::kFloat32 && dbias->numel() == D3,
                "attn_bwd: dbias must be contiguous fp32 [3D]");
    part = torch::empty({rows, D3}, qkv.options().dtype(torch::kFloat32));
  }
  float* pp = dbias ? part.data_ptr<float>() : nullptr;
  check_rc(jm_attn_bwd(bf(qkv), bf(o), bf(dO), lse.data_ptr<float>(), bfm(dqkv), B, S, heads, hd, pp, std::get<0>(dr),
                       std::get<1>(dr), std::get<2>(dr), stream()),
           "attn_bwd");
  if (dbias) check_rc(jm_splitk_reduce_add(pp, dbias->data_ptr<float>(), D3, rows, stream()), "attn_bwd dbias");
  return dqkv;
}

// ------------------------------------------------------------------------------ optimizer
int nch(const torch::Tensor& chunks) { return chunks.size(0); }
const int* chp(const torch::Tensor& chunks) { return chunks.data_ptr<int>(); }
uint16_t* shadow_ptr(c10::optional<torch::Tensor>& s) {
  return (s.has_value() && s->defined()) ? reinterpret_cast<uint16_t*>(s->data_ptr()) : nullptr;
}

// per-chunk partial sums of the norm kernels (summed per segment in chunk order: deterministic)
torch::Tensor chunk_part(const torch::Tensor& like, const torch::Tensor& chunks, int nc) {
  return torch::empty({(long)nch(chunks) * nc + 1}, like.options().dtype(torch::kFloat32));
}

void opt_sumsq(torch::Tensor x, torch::Tensor chunks, torch::Tensor out) {
  auto cp = chunk_part(x, chunks, 1);
  jm_opt_sumsq(x.data_ptr<float>(), chp(chunks), nch(chunks), out.data_ptr<float>(), cp.data_ptr<float>(), stream());
}

void opt_adamw(torch::Tensor p, torch::Tensor g, torch::Tensor mu, torch::Tensor nu, c10::optional<torch::Tensor> shadow,
               torch::Tensor chunks, torch::Tensor meta, torch::Tensor hyper, torch::Tensor gnorm_sq) {
  jm_opt_adamw(p.data_ptr<float>(), g.data_ptr<float>(), mu.data_ptr<float>(), nu.data_ptr<float>(),
               shadow_ptr(shadow), chp(chunks), nch(chunks), meta.data_ptr<float>(), hyper.data_ptr<float>(),
               gnorm_sq.data_ptr<float>(), stream());
}

void opt_lamb_phase1(torch::Tensor p, torch::Tensor g, torch::Tensor mu, torch::Tensor nu, torch::Tensor u,
                     torch::Tensor chunks, torch::Tensor meta, torch::Tensor hyper, torch::Tensor gnorm_sq,
                     torch::Tensor norms) {
  auto cp = chunk_part(p, chunks, 2);
  jm_opt_lamb_phase1(p.data_ptr<float>(), g.data_ptr<float>(), mu.data_ptr<float>(), nu.data_ptr<float>(),
                     u.data_ptr<float>(), chp(chunks), nch(chunks), meta.data_ptr<float>(), hyper.data_ptr<float>(),
                     gnorm_sq.data_ptr<float>(), norms.data_ptr<float>(), cp.data_ptr<float>(), stream());
}

void opt_lars_norms(torch::Tensor p, torch::Tensor g, torch::Tensor chunks, torch::Tensor hyper,
                    torch::Tensor gnorm_sq, torch::Tensor norms) {
  auto cp = chunk_part(p, chunks, 2);
  jm_opt_lars_norms(p.data_ptr<float>(), g.data_ptr<float>(), chp(chunks), nch(chunks), hyper.data_ptr<float>(),
                    gnorm_sq.data_ptr<float>(), norms.data_ptr<float>(), cp.data_ptr<float>(), stream());
}

void opt_apply_trust(torch::Tensor p, torch::Tensor u_or_g, c10::optional<torch::Tensor> trace,
                     c10::optional<torch::Tensor> shadow, torch::Tensor chunks, torch::Tensor meta, torch::Tensor hyper,
                     torch::Tensor norms, torch::Tensor gnorm_sq, int64_t mode, double momentum, double trust_coef) {
  jm_opt_apply_trust(p.data_ptr<float>(), u_or_g.data_ptr<float>(), fopt_m(trace), shadow_ptr(shadow), chp(chunks),
                     nch(chunks), meta.data_ptr<float>(), hyper.data_ptr<float>(), norms.data_ptr<float>(),
                     gnorm_sq.data_ptr<float>(), (int)mode, (float)momentum, (float)trust_coef, stream());
}

void opt_sgd(torch::Tensor p, torch::Tensor g, torch::Tensor trace, c10::optional<torch::Tensor> shadow,
             torch::Tensor chunks, torch::Tensor meta, torch::Tensor hyper, torch::Tensor gnorm_sq, double momentum) {
  jm_opt_sgd(p.data_ptr<float>(), g.data_ptr<float>(), trace.data_ptr<float>(), shadow_ptr(shadow), chp(chunks),
             nch(chunks), meta.data_ptr<float>(), hyper.data_ptr<float>(), gnorm_sq.data_ptr<float>(),
             (float)momentum, stream());
}

// weight EMA: flat fp32 master / ema of one length on one GPU, an int32 [nchunks, 3] chunk table
// (what: the second buffer's name in the messages -- the norm monitor checks grad and p_old with it)
void check_ema_pair(const torch::Tensor& master, const torch::Tensor& ema, const torch::Tensor& rows,
                    const char* fn, const char* what = "ema") {
  TORCH_CHECK(master.is_cuda() && ema.is_cuda() && rows.is_cuda() && ema.device() == master.device() &&
                  rows.device() == master.device(),
              fn, ": master, ", what, " and rows must be tensors on one GPU");
  TORCH_CHECK(master.scalar_type() == torch::kFloat32 && ema.scalar_type() == torch::kFloat32, fn,
              ": master and ", what, " must be fp32");
  TORCH_CHECK(master.dim() == 1 && ema.dim() == 1 && master.is_contiguous() && ema.is_contiguous(), fn,
              ": master and ", what, " must be flat contiguous buffers");
  TORCH_CHECK(ema.numel() == master.numel(), fn, ": ", what, " has ", ema.numel(),
              " elements, the rows reach into master's ", master.numel());
  TORCH_CHECK(rows.scalar_type() == torch::kInt32 && rows.dim() == 2 && rows.size(1) == 3 && rows.is_contiguous(), fn,
              ": rows must be a contiguous int32 [nchunks, 3] chunk table");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(master.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(ema.data_ptr()) % 16 == 0,
              fn, ": master and ", what, " must be 16-byte aligned");
}

void opt_ema(torch::Tensor master, torch::Tensor ema, torch::Tensor rows, torch::Tensor meta, torch::Tensor ema_hyper) {
  check_ema_pair(master, ema, rows, "opt_ema");
  TORCH_CHECK(meta.is_cuda() && meta.device() == master.device() && meta.scalar_type() == torch::kFloat32 &&
                  meta.is_contiguous() && meta.dim() == 2 && meta.size(1) == 4,
              "opt_ema: meta must be a contiguous fp32 [segments, 4] GPU tensor");
  TORCH_CHECK(ema_hyper.is_cuda() && ema_hyper.device() == master.device() &&
                  ema_hyper.scalar_type() == torch::kFloat32 && ema_hyper.numel() >= 1 && ema_hyper.is_contiguous(),
              "opt_ema: ema_hyper must be an fp32 GPU tensor holding 1 - decay");
  jm_opt_ema(master.data_ptr<float>(), ema.data_ptr<float>(), chp(rows), nch(rows), meta.data_ptr<float>(),
             (int)meta.size(0), ema_hyper.data_ptr<float>(), (long)master.numel(), stream());
}

void ema_swap(torch::Tensor master, torch::Tensor ema, c10::optional<torch::Tensor> shadow, torch::Tensor rows) {
  check_ema_pair(master, ema, rows, "ema_swap");
  if (shadow.has_value() && shadow->defined()) {
    TORCH_CHECK(shadow->is_cuda() && shadow->device() == master.device() &&
                    shadow->scalar_type() == torch::kBFloat16 && shadow->is_contiguous(),
                "ema_swap: shadow must be a contiguous bf16 tensor on master's GPU");
    TORCH_CHECK(shadow->numel() == master.numel(), "ema_swap: shadow has ", shadow->numel(), " elements, master ",
                master.numel());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(shadow->data_ptr()) % 8 == 0, "ema_swap: shadow must be 8-byte aligned");
  }
  jm_ema_swap(master.data_ptr<float>(), ema.data_ptr<float>(), shadow_ptr(shadow), chp(rows), nch(rows),
              (long)master.numel(), stream());
}

// norm monitor: out[seg] = [sum g^2, sum p^2, sum (p - p_old)^2, max |g|, non-finite g, non-finite p,
// elements] over the rows, fp64 [segments, 7]; every row of out is written, whatever it held
torch::Tensor opt_seg_stats(torch::Tensor master, torch::Tensor grad, c10::optional<torch::Tensor> p_old,
                            torch::Tensor rows, torch::Tensor meta, c10::optional<torch::Tensor> out) {
  check_ema_pair(master, grad, rows, "opt_seg_stats", "grad");
  const bool old = p_old.has_value() && p_old->defined();
  if (old) check_ema_pair(master, *p_old, rows, "opt_seg_stats", "p_old");
  TORCH_CHECK(meta.is_cuda() && meta.device() == master.device() && meta.scalar_type() == torch::kFloat32 &&
                  meta.is_contiguous() && meta.dim() == 2 && meta.size(1) == 4 && meta.size(0) >= 1,
              "opt_seg_stats: meta must be a contiguous fp32 [segments, 4] GPU tensor");
  const long nseg = meta.size(0);
  const auto f64 = master.options().dtype(torch::kFloat64);
  torch::Tensor o;
  if (out.has_value() && out->defined()) {
    o = *out;
    TORCH_CHECK(o.is_cuda() && o.device() == master.device() && o.scalar_type() == torch::kFloat64 &&
                    o.is_contiguous() && o.dim() == 2 && o.size(0) == nseg && o.size(1) == JM_SEG_STATS_COLS,
                "opt_seg_stats: out must be a contiguous fp64 [segments, ", JM_SEG_STATS_COLS,
                "] tensor on master's GPU");
  } else {
    o = torch::empty({nseg, (long)JM_SEG_STATS_COLS}, f64);
  }
#ifdef JM_DEBUG
  auto part = torch::zeros({(long)nch(rows) + 1, (long)JM_SEG_STATS_COLS}, f64);  // a skipped row adds nothing
#else
  auto part = torch::empty({(long)nch(rows) + 1, (long)JM_SEG_STATS_COLS}, f64);
#endif
  jm_opt_seg_stats(master.data_ptr<float>(), grad.data_ptr<float>(), old ? p_old->data_ptr<float>() : nullptr,
                   chp(rows), nch(rows), meta.data_ptr<float>(), (int)nseg, (long)master.numel(),
                   part.data_ptr<double>(), o.data_ptr<double>(), stream());
  return o;
}

// ------------------------------------------------------------------------------ MAE
torch::Tensor patchify_normalize(torch::Tensor img, int64_t p) {
  CHECK_CONTIG(img);
  CHECK_DT(img, torch::kUInt8);
  const int B = img.size(0), H = img.size(2), W = img.size(3);
  TORCH_CHECK(img.size(1) == 3, "expects 3 channels");
  const int n = (H / p) * (W / p);
  auto out = torch::empty({B, n, (long)p * p * 3}, img.options().dtype(torch::kFloat32));
  check_rc(jm_patchify_normalize(img.data_ptr<uint8_t>(), out.data_ptr<float>(), B, H, W, p, stream()),
           "patchify_normalize");
  return out;
}

// Index tensors: int32, 1-D (shared permutation, batch stride 0) or 2-D [B, n] (per sample).
long ids_bstride(const torch::Tensor& ids) {
  CHECK_DT(ids, torch::kInt32);
  CHECK_CONTIG(ids);
  TORCH_CHECK(ids.dim() == 1 || ids.dim() == 2, "ids must be 1-D or 2-D");
  return ids.dim() == 1 ? 0 : ids.size(1);
}

torch::Tensor gather_patches(torch::Tensor img, torch::Tensor ids_keep, int64_t p) {
  CHECK_CONTIG(img);
  CHECK_DT(img, torch::kUInt8);
  TORCH_CHECK(img.size(1) == 3, "expects 3 channels");
  const long sb = ids_bstride(ids_keep);
  const int B = img.size(0), H = img.size(2), W = img.size(3);
  const int K = ids_keep.size(-1);
  TORCH_CHECK(ids_keep.dim() == 1 || ids_keep.size(0) == B, "ids_keep batch mismatch");
  auto out = torch::empty({(long)B * K, 3 * p * p}, img.options().dtype(torch::kBFloat16));
  check_rc(jm_gather_patches(img.data_ptr<uint8_t>(), ids_keep.data_ptr<int>(), sb, bfp(out), B, K, H, W, p, stream()),
           "gather_patches");
  return out;
}

torch::Tensor embed_finish(torch::Tensor e, c10::optional<torch::Tensor> pos, torch::Tensor ids_keep, torch::Tensor cls,
                           int64_t B) {
  CHECK_CONTIG(e);
  CHECK_DT(e, torch::kBFloat16);
  CHECK_CONTIG(cls);
  CHECK_DT(cls, torch::kFloat32);
  const long sb = ids_bstride(ids_keep);
  const int K = ids_keep.size(-1), D = e.size(1), C = cls.numel() / D;
  TORCH_CHECK(e.size(0) == B * K, "embed_finish: e rows");
  const float* pp = nullptr;
  if (pos) {
    CHECK_CONTIG((*pos));
    CHECK_DT((*pos), torch::kFloat32);
    TORCH_CHECK(pos->size(-1) == D, "pos dim");
    pp = pos->data_ptr<float>();
  }
  auto out = torch::empty({B, C + K, D}, e.options().dtype(torch::kFloat32));
  check_rc(jm_embed_finish(bfp(e), pp, ids_keep.data_ptr<int>(), sb, cls.data_ptr<float>(), out.data_ptr<float>(), B, C,
                           K, D, stream()),
           "embed_finish");
  return out;
}

torch::Tensor unshuffle_fwd(torch::Tensor y, torch::Tensor tok, torch::Tensor ids_restore, torch::Tensor pos,
                            int64_t C) {
  CHECK_CONTIG(y);
  CHECK_DT(y, torch::kBFloat16);
  CHECK_CONTIG(tok);
  CHECK_CONTIG(pos);
  CHECK_DT(tok, torch::kFloat32);
  CHECK_DT(pos, torch::kFloat32);
  const long sb = ids_bstride(ids_restore);
  const int B = y.size(0), d = y.size(2), K = y.size(1) - C, N = pos.size(0);
  TORCH_CHECK(ids_restore.size(-1) == N && tok.numel() == d && pos.size(1) == d, "unshuffle_fwd shapes");
  auto out = torch::empty({B, C + N, d}, y.options().dtype(torch::kFloat32));
  check_rc(jm_unshuffle_fwd(bfp(y), tok.data_ptr<float>(), ids_restore.data_ptr<int>(), sb, pos.data_ptr<float>(),
                            out.data_ptr<float>(), B, C, K, N, d, stream()),
           "unshuffle_fwd");
  return out;
}

// t[:] = 0 by the kernel the store-mode gradients use in front of an accumulating reduce (graph tests)
void zero_f32(torch::Tensor t) {
  CHECK_CUDA(t);
  CHECK_CONTIG(t);
  CHECK_DT(t, torch::kFloat32);
  jm_zero_f32(t.data_ptr<float>(), t.numel(), stream());
}

// random-masking ids from noise [N] or [R, N] fp32 -> (ids_shuffle i64, ids_restore i64, keep32 i32
// [.., keep], restore32 i32, mask f32), each shaped like the noise (keep32: last dim keep)
std::vector<torch::Tensor> mask_ids(torch::Tensor noise, int64_t keep) {
  CHECK_CUDA(noise);
  CHECK_CONTIG(noise);
  CHECK_DT(noise, torch::kFloat32);
  TORCH_CHECK(noise.dim() == 1 || noise.dim() == 2, "mask_ids: noise [N] or [R, N]");
  const int N = noise.size(-1), R = noise.dim() == 1 ? 1 : noise.size(0);
  TORCH_CHECK(N <= 1024 && keep >= 0 && keep <= N, "mask_ids: N <= 1024, 0 <= keep <= N");
  auto i64 = noise.options().dtype(torch::kInt64), i32 = noise.options().dtype(torch::kInt32);
  auto shuffle = torch::empty(noise.sizes(), i64), restore = torch::empty(noise.sizes(), i64);
  auto restore32 = torch::empty(noise.sizes(), i32), mask = torch::empty(noise.sizes(), noise.options());
  auto ks = noise.sizes().vec();
  ks.back() = keep;
  auto keep32 = torch::empty(ks, i32);
  check_rc(jm_mask_ids(noise.data_ptr<float>(), R, N, (int)keep, shuffle.data_ptr<int64_t>(),
                       restore.data_ptr<int64_t>(), keep32.data_ptr<int>(), restore32.data_ptr<int>(),
                       mask.data_ptr<float>(), stream()),
           "mask_ids");
  return {shuffle, restore, keep32, restore32, mask};
}

// -> (dy bf16 [B, C+K, d], d mask_token fp32 [d])
std::vector<torch::Tensor> unshuffle_bwd(torch::Tensor dout, torch::Tensor ids_restore, int64_t C, int64_t K) {
  CHECK_CONTIG(dout);
  CHECK_DT(dout, torch::kFloat32);
  const long sb = ids_bstride(ids_restore);
  const int B = dout.size(0), N = dout.size(1) - C, d = dout.size(2);
  TORCH_CHECK(ids_restore.size(-1) == N, "unshuffle_bwd shapes");
  const int rpb = 64;
  const int nb = jm_unshuffle_bwd_blocks(B, C, N, rpb);
  auto dy = torch::empty({B, C + K, d}, dout.options().dtype(torch::kBFloat16));
  auto part = torch::empty({nb, d}, dout.options().dtype(torch::kFloat64));
  check_rc(jm_unshuffle_bwd(dout.data_ptr<float>(), ids_restore.data_ptr<int>(), sb, bfp(dy), part.data_ptr<double>(), B,
                            C, K, N, d, rpb, stream()),
           "unshuffle_bwd");
  // the kernel's per-block fp64 partials summed in fp64 and rounded once -> [1, d] fp32: cancelling
  // columns keep one fp32 ulp; the caller adds it to the gradient (colsum_add_f32)
  return {dy, part.sum(0, true).to(torch::kFloat32)};
}

// finetune input: [B*N, 3p^2] bf16 normalized patches of the (Mixup / CutMix) blended batch
torch::Tensor mix_patches(torch::Tensor img, c10::optional<torch::Tensor> perm, c10::optional<torch::Tensor> prm,
                          c10::optional<torch::Tensor> box, int64_t p) {
  CHECK_CONTIG(img);
  CHECK_DT(img, torch::kUInt8);
  TORCH_CHECK(img.size(1) == 3, "mix_patches: 3 channels");
  const int B = img.size(0), H = img.size(2), W = img.size(3);
  const int* pp = nullptr;
  const float* pr = nullptr;
  const int* bx = nullptr;
  if (prm) {
    TORCH_CHECK(perm && box, "mix_patches: prm needs perm and box");
    CHECK_DT((*perm), torch::kInt32);
    CHECK_DT((*prm), torch::kFloat32);
    CHECK_DT((*box), torch::kInt32);
    TORCH_CHECK(perm->numel() == B && prm->numel() >= 2 && box->numel() == 4, "mix_patches: param sizes");
    pp = perm->data_ptr<int>();
    pr = prm->data_ptr<float>();
    bx = box->data_ptr<int>();
  }
  auto out = torch::empty({(long)B * (H / p) * (W / p), 3 * p * p}, img.options().dtype(torch::kBFloat16));
  check_rc(jm_mix_patches(img.data_ptr<uint8_t>(), pp, pr, bx, bfp(out), B, H, W, p, stream()), "mix_patches");
  return out;
}

// pred: bf16 [B*N, P3] (row stride may exceed P3); -> per-patch MSE fp32 [B*N]
torch::Tensor patch_mse_fwd(torch::Tensor pred, torch::Tensor img, int64_t p, bool norm_pix) {
  CHECK_DT(pred, torch::kBFloat16);
  TORCH_CHECK(pred.stride(1) == 1, "pred rows must be contiguous");
  CHECK_CONTIG(img);
  CHECK_DT(img, torch::kUInt8);
  const int H = img.size(2), W = img.size(3), N = (H / p) * (W / p);
  TORCH_CHECK(pred.size(0) == img.size(0) * N && pred.size(1) == 3 * p * p, "patch_mse_fwd shapes");
  auto mse = torch::empty({pred.size(0)}, pred.options().dtype(torch::kFloat32));
  check_rc(jm_patch_mse_fwd(bfp(pred), pred.stride(0), img.data_ptr<uint8_t>(), mse.data_ptr<float>(), pred.size(0), N,
                            H, W, p, norm_pix, stream()),
           "patch_mse_fwd");
  return mse;
}

torch::Tensor patch_mse_bwd(torch::Tensor pred, torch::Tensor img, torch::Tensor dmse, int64_t p, bool norm_pix) {
  CHECK_DT(pred, torch::kBFloat16);
  TORCH_CHECK(pred.stride(1) == 1, "pred rows must be contiguous");
  CHECK_CONTIG(img);
  CHECK_CONTIG(dmse);
  CHECK_DT(dmse, torch::kFloat32);
  const int H = img.size(2), W = img.size(3), N = (H / p) * (W / p);
  TORCH_CHECK(dmse.numel() == pred.size(0) && pred.size(0) == img.size(0) * N && pred.size(1) == 3 * p * p,
              "patch_mse_bwd shapes");
  auto dpred = torch::empty({pred.size(0), pred.size(1)}, pred.options());
  check_rc(jm_patch_mse_bwd(bfp(pred), pred.stride(0), img.data_ptr<uint8_t>(), dmse.data_ptr<float>(), bfp(dpred),
                            pred.size(0), N, H, W, p, norm_pix, stream()),
           "patch_mse_bwd");
  return dpred;
}

// reconstruction panels (recon.hip) -> (recon, paste, masked uint8 [B, 3, H, W], err fp32 [B, N]).
// pred: bf16 or fp32 [B*N, 3p^2]; mask: fp32 [N] (shared) or [B, N], 1 = masked; out: the four outputs to
// write into instead of new tensors.  Everything is checked before any pointer reaches the kernel.
std::vector<torch::Tensor> recon(torch::Tensor pred, torch::Tensor images, torch::Tensor mask, int64_t p, bool norm_pix,
                                 int64_t fill, c10::optional<std::vector<torch::Tensor>> out) {
  CHECK_CUDA(pred);
  CHECK_CUDA(images);
  CHECK_CUDA(mask);
  TORCH_CHECK(images.device() == pred.device() && mask.device() == pred.device(), "recon: tensors on one device");
  TORCH_CHECK(pred.scalar_type() == torch::kBFloat16 || pred.scalar_type() == torch::kFloat32,
              "recon: pred must be bf16 or fp32");
  CHECK_DT(images, torch::kUInt8);
  CHECK_DT(mask, torch::kFloat32);
  CHECK_CONTIG(pred);
  CHECK_CONTIG(images);
  CHECK_CONTIG(mask);
  TORCH_CHECK(pred.dim() == 2, "recon: pred [B*N, 3p^2]");
  TORCH_CHECK(images.dim() == 4 && images.size(1) == 3, "recon: images [B, 3, H, W]");
  TORCH_CHECK(fill >= 0 && fill <= 255, "recon: fill is a byte");
  const int64_t B = images.size(0), H = images.size(2), W = images.size(3);
  TORCH_CHECK(p > 0 && p % 2 == 0, "recon: patch size must be positive and even, got ", p);
  TORCH_CHECK(H > 0 && W > 0 && H % p == 0 && W % p == 0, "recon: image ", H, " x ", W,
              " is not a whole number of ", p, " x ", p, " patches");
  TORCH_CHECK(H <= INT_MAX && W <= INT_MAX && B <= INT_MAX, "recon: image batch too large");
  const int64_t N = (H / p) * (W / p);
  TORCH_CHECK(B * N <= INT_MAX, "recon: too many patches");
  TORCH_CHECK(pred.size(0) == B * N && pred.size(1) == 3 * p * p, "recon: pred must be [", B * N, ", ", 3 * p * p,
              "], got [", pred.size(0), ", ", pred.size(1), "]");
  TORCH_CHECK((mask.dim() == 1 && mask.size(0) == N) || (mask.dim() == 2 && mask.size(0) == B && mask.size(1) == N),
              "recon: mask must be [", N, "] or [", B, ", ", N, "]");
  const long maskB = mask.dim() == 1 ? 0 : (long)N;
  torch::Tensor rec, paste, masked, err;
  if (out.has_value()) {
    TORCH_CHECK(out->size() == 4, "recon: out = (recon, paste, masked, err)");
    for (int i = 0; i < 3; ++i) {
      const auto& t = (*out)[i];
      TORCH_CHECK(t.is_cuda() && t.device() == pred.device() && t.scalar_type() == torch::kUInt8 &&
                      t.is_contiguous() && t.sizes() == images.sizes(),
                  "recon: out[", i, "] must be a contiguous uint8 tensor shaped like images");
    }
    const auto& e = (*out)[3];
    TORCH_CHECK(e.is_cuda() && e.device() == pred.device() && e.scalar_type() == torch::kFloat32 &&
                    e.is_contiguous() && e.dim() == 2 && e.size(0) == B && e.size(1) == N,
                "recon: out[3] must be a contiguous fp32 [B, N] tensor");
    rec = (*out)[0], paste = (*out)[1], masked = (*out)[2], err = e;
  } else {
    rec = torch::empty_like(images);
    paste = torch::empty_like(images);
    masked = torch::empty_like(images);
    err = torch::empty({B, N}, images.options().dtype(torch::kFloat32));
  }
  check_rc(jm_recon(pred.data_ptr(), pred.scalar_type() == torch::kBFloat16, images.data_ptr<uint8_t>(),
                    mask.data_ptr<float>(), maskB, rec.data_ptr<uint8_t>(), paste.data_ptr<uint8_t>(),
                    masked.data_ptr<uint8_t>(), err.data_ptr<float>(), (int)B, (int)H, (int)W, (int)p, norm_pix,
                    (int)fill, stream()),
           "recon");
  return {rec, paste, masked, err};
}

}  // namespace

// ------------------------------------------------------------------------------ GEMM
// Every NT launch: one plan (gemm_plan.h GemmPlan, jm_gemm_nt_plan) that sizes the buffers here and
// that jm_gemm_nt obeys.
// the bf16 operands A [M, K] and B [N, K], K contiguous (rows may be strided) -> {M, N, K}
std::array<int, 3> check_nt_operands(const char* fn, const torch::Tensor& A, const torch::Tensor& B) {
  CHECK_DT(A, torch::kBFloat16);
  CHECK_DT(B, torch::kBFloat16);
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(1) == B.size(1), fn, ": A [M,K], B [N,K]");
  TORCH_CHECK(A.stride(1) == 1 && B.stride(1) == 1, fn, ": K must be contiguous");
  return {(int)A.size(0), (int)B.size(0), (int)A.size(1)};
}

// the data of an optional contiguous fp32 [N] bias (or bias gradient); null without one
float* bias_ptr(const char* what, const c10::optional<torch::Tensor>& bias, int N) {
  if (!bias) return nullptr;
  TORCH_CHECK(bias->is_contiguous() && bias->scalar_type() == torch::kFloat32 && bias->numel() == N, what);
  return bias->data_ptr<float>();
}

// the planned launch, with the workspace of its tail split (GemmPlan::tail_floats)
void run_nt(const char* fn, const GemmPlan& plan, const torch::Tensor& A, const torch::Tensor& B, GemmEpi ep) {
  torch::Tensor ws;
  if (plan.tail_floats) {
    ws = torch::empty({plan.tail_floats}, A.options().dtype(torch::kFloat32));
    ep.tail = ws.data_ptr<float>();
  }
  check_rc(jm_gemm_nt(plan, bf(A), bf(B), B.stride(0), ep, stream()), fn);
}

// C[M, N] = A[M, K] . B[N, K]^T (+ bias) in bf16 (fp32 accumulate); gelu=true also returns
// gelu(C) (the pre-activation C is what the backward needs).  A / B rows may be strided.
// gelu_deriv (with gelu): returns {gelu'(h) as uint8 codes (common.h gd_code), gelu(h)} instead of
// {h, gelu(h)} (EPI_GELU_D); with dropout the codes are those of the kept gelu'(h) unscaled (0 where
// dropped) and gemm_nt_dgelu applies 1 / keep when it decodes them
std::vector<torch::Tensor> gemm_nt(torch::Tensor A, torch::Tensor B, c10::optional<torch::Tensor> bias, bool gelu,
                                   bool gelu_only, bool gelu_deriv, c10::optional<torch::Tensor> seed, double rate) {
  const auto [M, N, K] = check_nt_operands("gemm_nt", A, B);
  TORCH_CHECK(!gelu_deriv || N % 8 == 0, "gemm_nt: gelu_deriv needs N % 8 == 0");
  auto out = torch::empty({M, N}, gelu_deriv ? A.options().dtype(torch::kUInt8) : A.options());
  torch::Tensor out2;
  GemmEpi ep{bias_ptr("gemm_nt bias", bias, N), gelu_deriv ? nullptr : bfm(out), N};
  if (gelu_deriv) ep.dq = out.data_ptr<uint8_t>();
  if (gelu && !gelu_only) {
    out2 = torch::empty({M, N}, A.options());
    ep.out2 = bfm(out2);
  }
  TORCH_CHECK(!gelu_deriv || (gelu && !gelu_only), "gemm_nt: gelu_deriv needs gelu and not gelu_only");
  const int epi = gelu_only ? EPI_GELU_ONLY : (gelu_deriv ? EPI_GELU_D : (gelu ? EPI_GELU : EPI_STORE));
  if (seed.has_value() && seed->defined() && rate > 0.0) {  // FF hidden dropout in the GELU_D epilogue
    TORCH_CHECK(epi == EPI_GELU_D, "gemm_nt: dropout only with gelu_deriv");
    check_seed(*seed, A);
    const auto kp = keep_params(rate);
    ep.dseed = seed->data_ptr<int64_t>();
    ep.dthr = kp.first;
    ep.dscale = kp.second;
  }
  run_nt("gemm_nt", jm_gemm_nt_plan(M, N, K, epi, A.stride(0), 1), A, B, ep);
  if (gelu && !gelu_only) return {out, out2};
  return {out};
}

// split-K: C[M, N] = A[M, K] . B[N, K]^T (+ bias) in bf16 via S fp32 partial products
// add (optional fp32 [M, N] view, unit column stride): the result is returned in fp32 as
// A.B^T (+ bias) + add, summed in the split-K reduction
torch::Tensor gemm_nt_splitk(torch::Tensor A, torch::Tensor B, c10::optional<torch::Tensor> bias, int64_t splits,
                             c10::optional<torch::Tensor> add) {
  const auto [M, N, K] = check_nt_operands("gemm_nt_splitk", A, B);
  auto out = torch::empty({M, N}, A.options());
  auto part = torch::empty({splits, (long)M * N}, A.options().dtype(torch::kFloat32));
  GemmEpi ep{nullptr, bfm(out), N};
  ep.part = part.data_ptr<float>();
  run_nt("gemm_nt_splitk", jm_gemm_nt_plan(M, N, K, EPI_PARTIAL, A.stride(0), (int)splits), A, B, ep);
  const float* bp = bias_ptr("bias", bias, N);
  if (add) {
    CHECK_CUDA(*add);
    CHECK_DT(*add, torch::kFloat32);
    TORCH_CHECK(add->dim() == 2 && add->size(0) == M && add->size(1) == N && add->stride(1) == 1,
                "gemm_nt_splitk: add must be fp32 [M, N] with unit column stride");
    auto out32 = torch::empty({M, N}, A.options().dtype(torch::kFloat32));
    check_rc(jm_splitk_reduce_f32(part.data_ptr<float>(), (int)splits, M, N, bp, add->data_ptr<float>(),
                                  add->stride(0), out32.data_ptr<float>(), stream()),
             "gemm_nt_splitk reduce f32");
    return out32;
  }
  check_rc(jm_splitk_reduce_bf16(part.data_ptr<float>(), (int)splits, (long)M * N, N, bp, bfm(out), stream()),
           "gemm_nt_splitk reduce");
  return out;
}

// C[M, N] = A[M, K] . B[N, K]^T in fp32 (EPI_PARTIAL with one split: the accumulators stored as
// they are) -- short-reduction weight gradients in NT form (ops/prims.py wgrad)
torch::Tensor gemm_nt_f32(torch::Tensor A, torch::Tensor B) {
  const auto [M, N, K] = check_nt_operands("gemm_nt_f32", A, B);
  auto out = torch::empty({M, N}, A.options().dtype(torch::kFloat32));
  GemmEpi ep{nullptr, nullptr, N};
  ep.part = out.data_ptr<float>();
  run_nt("gemm_nt_f32", jm_gemm_nt_plan(M, N, K, EPI_PARTIAL, A.stride(0), 1), A, B, ep);
  return out;
}

// dh[M, N] = (A[M, K] . B[N, K]^T) * gelu'(pre[M, N]) -- FF2 data gradient through the GELU,
// B = W2^T; dbias (fp32 [N], optional) += column sums of dh (the FF1 bias gradient).
// deriv: ``pre`` holds the saved gelu'(h) as uint8 codes (EPI_GELU_D forward): the epilogue decodes
// and multiplies (EPI_DMUL); ``rate`` > 0: the forward's FF hidden dropout rate (codes of the unscaled
// kept derivative), 1 / keep applied with the decode
torch::Tensor gemm_nt_dgelu(torch::Tensor A, torch::Tensor B, torch::Tensor pre, c10::optional<torch::Tensor> dbias,
                            bool deriv, double rate) {
  CHECK_DT(pre, deriv ? torch::kUInt8 : torch::kBFloat16);
  const auto [M, N, K] = check_nt_operands("gemm_nt_dgelu", A, B);
  TORCH_CHECK(pre.is_contiguous() && pre.size(0) == M && pre.size(1) == N, "gemm_nt_dgelu: pre [M,N]");
  auto out = torch::empty({M, N}, A.options());
  GemmEpi ep{nullptr, bfm(out), N};
  if (deriv) {
    ep.dqa = pre.data_ptr<uint8_t>();
    ep.dqs = (rate > 0.0 ? keep_params(rate).second : 1.f) / GD_Q;
  } else {
    ep.aux = bf(pre);
  }
  GemmPlan plan = jm_gemm_nt_plan(M, N, K, deriv ? EPI_DMUL : EPI_DGELU, A.stride(0), 1);
  float* db = bias_ptr("gemm_nt_dgelu dbias", dbias, N);
  torch::Tensor part;  // the launch's column sums (GemmPlan::colpart_rows), added to dbias below
  if (db) {
    const auto f32 = A.options().dtype(torch::kFloat32);
    part = plan.colpart_zero ? torch::zeros({plan.colpart_rows, N}, f32) : torch::empty({plan.colpart_rows, N}, f32);
    ep.colpart = part.data_ptr<float>();
  } else {
    plan.colpart = false;  // no bias gradient asked for: the kernels skip the column sums
  }
  run_nt("gemm_nt_dgelu", plan, A, B, ep);
  if (db) check_rc(jm_splitk_reduce_add(part.data_ptr<float>(), db, N, plan.colpart_rows, stream()),
                   "gemm_nt_dgelu dbias");
  return out;
}

// the plan's fields by name (tests, tools)
py::dict gemm_nt_plan_dict(int M, int N, int K, int epi, long lda, int splits) {
  const GemmPlan p = jm_gemm_nt_plan(M, N, K, epi, lda, splits);
  using namespace py::literals;
  return py::dict("status"_a = p.status, "family"_a = p.family, "tile_rows"_a = p.tile_rows,
                  "tile_cols"_a = p.tile_cols, "row_tiles"_a = p.row_tiles, "col_tiles"_a = p.col_tiles,
                  "tiles"_a = p.tiles, "grid"_a = p.grid, "tail_S"_a = p.tail_S, "tail_r"_a = p.tail_r,
                  "tail_floats"_a = p.tail_floats, "colpart"_a = p.colpart, "colpart_rows"_a = p.colpart_rows,
                  "colpart_zero"_a = p.colpart_zero);
}

// ---------------------------------------------------------------- augment (csrc/augment.hip)
// Pillow-exact RandomResizedCrop (bicubic) + flip of a batch of decoded crop windows on the device
// (data/loader.py DeviceAugment): src = concatenated HWC uint8 windows, tab = [B, 13] int64
// descriptors (csrc/augment.hip); tmp_bytes / tmp_rows_max from the host copy of the table.
torch::Tensor rrc_resize(torch::Tensor src, torch::Tensor tab, int64_t size, int64_t tmp_bytes, int64_t tmp_rows_max) {
  CHECK_CUDA(src);
  CHECK_CUDA(tab);
  CHECK_DT(src, torch::kUInt8);
  CHECK_DT(tab, torch::kInt64);
  TORCH_CHECK(src.dim() == 1 && src.is_contiguous(), "rrc_resize: src must be a flat uint8 buffer");
  TORCH_CHECK(tab.dim() == 2 && tab.size(1) == 13 && tab.is_contiguous(), "rrc_resize: tab [B, 13] int64");
  TORCH_CHECK(size > 0 && size <= 4096 && tmp_bytes > 0 && tmp_rows_max > 0, "rrc_resize: bad sizes");
  const int B = tab.size(0);
  auto out = torch::empty({B, 3, size, size}, src.options());
  auto tmp = torch::empty({tmp_bytes}, src.options());
  check_rc(jm_rrc_resize(src.data_ptr<uint8_t>(), tab.data_ptr<int64_t>(), B, (int)size, tmp.data_ptr<uint8_t>(),
                         (int)tmp_rows_max, out.data_ptr<uint8_t>(), stream()),
           "rrc_resize");
  return out;
}

// Pillow-exact validation transform (Resize bicubic -> CenterCrop) of a padded batch on the device
// (data/loader.py DeviceValidParams / collate_valid_packed): tab = [B, 18] int64 descriptors
// (csrc/augment.hip: the 13 columns above + the full output size, the window origin and the pad
// flag); pad rows come out as 255.  tmp_bytes / tmp_rows_max are 0 for a batch of pad rows only.
torch::Tensor window_resize(torch::Tensor src, torch::Tensor tab, int64_t size, int64_t tmp_bytes,
                            int64_t tmp_rows_max) {
  CHECK_CUDA(src);
  CHECK_CUDA(tab);
  CHECK_DT(src, torch::kUInt8);
  CHECK_DT(tab, torch::kInt64);
  TORCH_CHECK(src.dim() == 1 && src.is_contiguous(), "window_resize: src must be a flat uint8 buffer");
  TORCH_CHECK(tab.dim() == 2 && tab.size(1) == jm_window_tab() && tab.is_contiguous() && tab.size(0) > 0,
              "window_resize: tab [B, ", jm_window_tab(), "] int64");
  TORCH_CHECK(size > 0 && size <= 4096 && tmp_bytes >= 0 && tmp_rows_max >= 0 && (tmp_bytes > 0) == (tmp_rows_max > 0),
              "window_resize: bad sizes");
  const int B = tab.size(0);
  auto out = torch::empty({B, 3, size, size}, src.options());
  auto tmp = torch::empty({tmp_bytes > 0 ? tmp_bytes : 1}, src.options());
  check_rc(jm_window_resize(src.data_ptr<uint8_t>(), tab.data_ptr<int64_t>(), B, (int)size, tmp.data_ptr<uint8_t>(),
                            (int)tmp_rows_max, out.data_ptr<uint8_t>(), stream()),
           "window_resize");
  return out;
}

// RandAugment / AutoAugment / ColorJitter op chains on the resized batch (csrc/augment_chain.hip):
// images uint8 [B, 3, S, S] (rrc_resize's result; CONSUMED -- it is one of the two ping-pong
// buffers), chain float64 [B, slots, P] records (data/autoaugment.py), scratch the other buffer.
// Returns whichever of the two holds the result.  Stream-ordered, no host sync.
torch::Tensor aug_chain(torch::Tensor images, torch::Tensor chain, torch::Tensor scratch) {
  CHECK_CUDA(images);
  CHECK_CUDA(chain);
  CHECK_CUDA(scratch);
  CHECK_DT(images, torch::kUInt8);
  CHECK_DT(scratch, torch::kUInt8);
  CHECK_DT(chain, torch::kFloat64);
  TORCH_CHECK(images.dim() == 4 && images.size(1) == 3 && images.size(2) == images.size(3) && images.is_contiguous(),
              "aug_chain: images must be contiguous uint8 [B, 3, S, S]");
  TORCH_CHECK(scratch.sizes() == images.sizes() && scratch.is_contiguous() && scratch.data_ptr() != images.data_ptr(),
              "aug_chain: scratch must be a second contiguous buffer of the images' shape");
  TORCH_CHECK(chain.dim() == 3 && chain.size(0) == images.size(0) && chain.size(2) == jm_aug_record_len() &&
                  chain.is_contiguous(),
              "aug_chain: chain must be contiguous float64 [B, slots, ", jm_aug_record_len(), "]");
  TORCH_CHECK(images.size(0) > 0 && images.size(2) <= 4096, "aug_chain: bad sizes");
  const int B = images.size(0);
  auto stats = torch::empty({B, jm_aug_stat_words()}, images.options().dtype(torch::kInt32));
  const int rc = jm_aug_chain(images.data_ptr<uint8_t>(), scratch.data_ptr<uint8_t>(), chain.data_ptr<double>(), B,
                              (int)chain.size(1), (int)images.size(2),
                              reinterpret_cast<uint32_t*>(stats.data_ptr<int32_t>()), stream());
  check_rc(rc < 0 ? rc : 0, "aug_chain");
  return rc == 1 ? scratch : images;
}

// AugMix's composite (csrc/augment_chain.hip augmix_mix_kernel): orig uint8 [B, 3, S, S] (the resized
// batch), chains uint8 [B * W, 3, S, S] (aug_chain's result on the W replicas of every image, chain
// k of image b at b * W + k), table float32 [B, W + 1] (data/autoaugment.py AugMix.describe).
// Returns a new [B, 3, S, S]; the inputs are left as they are.  Stream-ordered, no host sync.
torch::Tensor augmix_mix(torch::Tensor orig, torch::Tensor chains, torch::Tensor table, bool blended) {
  CHECK_CUDA(orig);
  CHECK_CUDA(chains);
  CHECK_CUDA(table);
  CHECK_DT(orig, torch::kUInt8);
  CHECK_DT(chains, torch::kUInt8);
  CHECK_DT(table, torch::kFloat32);
  TORCH_CHECK(orig.dim() == 4 && orig.size(1) == 3 && orig.size(2) == orig.size(3) && orig.is_contiguous(),
              "augmix_mix: orig must be contiguous uint8 [B, 3, S, S]");
  TORCH_CHECK(orig.size(0) > 0 && orig.size(0) <= 65535 && orig.size(2) > 0 && orig.size(2) <= 4096,
              "augmix_mix: bad sizes");
  TORCH_CHECK(table.dim() == 2 && table.size(0) == orig.size(0) && table.size(1) >= 2 && table.size(1) <= 9 &&
                  table.is_contiguous(),
              "augmix_mix: table must be contiguous float32 [B, W + 1] with 1 <= W <= 8");
  const int64_t B = orig.size(0), W = table.size(1) - 1, S = orig.size(2);
  TORCH_CHECK(chains.dim() == 4 && chains.size(0) == B * W && chains.size(1) == 3 && chains.size(2) == S &&
                  chains.size(3) == S && chains.is_contiguous(),
              "augmix_mix: chains must be contiguous uint8 [B * W, 3, S, S]");
  auto out = torch::empty_like(orig);
  check_rc(jm_augmix_mix(orig.data_ptr<uint8_t>(), chains.data_ptr<uint8_t>(), table.data_ptr<float>(),
                         out.data_ptr<uint8_t>(), (int)B, (int)W, (int)S, blended ? 1 : 0, stream()),
           "augmix_mix");
  return out;
}

// RandomErasing's paste (csrc/augment_chain.hip erase_paste_kernel), in place on images uint8
// [B, 3, S, S]: table int64 [B, 5] = box row, column, rows, columns (rows 0: not erased) and the
// offset of the box's [3, rows, columns] bytes in the flat uint8 fill (data/loader.py
// collate_packed).  box_bytes_max: the largest 3 * rows * columns of the table, from its host copy
// (0: unknown).  Returns images.  Stream-ordered, no host sync.
torch::Tensor erase_paste(torch::Tensor images, torch::Tensor table, torch::Tensor fill, int64_t box_bytes_max) {
  CHECK_CUDA(images);
  CHECK_CUDA(table);
  CHECK_CUDA(fill);
  CHECK_DT(images, torch::kUInt8);
  CHECK_DT(table, torch::kInt64);
  CHECK_DT(fill, torch::kUInt8);
  TORCH_CHECK(images.dim() == 4 && images.size(1) == 3 && images.size(2) == images.size(3) && images.is_contiguous(),
              "erase_paste: images must be contiguous uint8 [B, 3, S, S]");
  TORCH_CHECK(images.size(0) > 0 && images.size(0) <= 65535 && images.size(2) > 0 && images.size(2) <= 4096,
              "erase_paste: bad sizes");
  TORCH_CHECK(table.dim() == 2 && table.size(0) == images.size(0) && table.size(1) == 5 && table.is_contiguous(),
              "erase_paste: table must be contiguous int64 [B, 5]");
  TORCH_CHECK(fill.dim() == 1 && fill.is_contiguous(), "erase_paste: fill must be a flat uint8 buffer");
  TORCH_CHECK(box_bytes_max >= 0, "erase_paste: box_bytes_max < 0");
  check_rc(jm_erase_paste(images.data_ptr<uint8_t>(), table.data_ptr<int64_t>(),
                          fill.numel() ? fill.data_ptr<uint8_t>() : nullptr, (long)fill.numel(), (int)images.size(0),
                          (int)images.size(2), (long)box_bytes_max, stream()),
           "erase_paste");
  return images;
}

// ---------------------------------------------------------------- dropout (csrc/dropout.hip)

// y = x * keep(seed, i) / keep  (bf16 or fp32, contiguous, numel % 8 == 0); also its own backward
torch::Tensor dropout_apply(torch::Tensor x, torch::Tensor seed, double rate) {
  CHECK_CONTIG(x);
  check_seed(seed, x);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 || x.scalar_type() == torch::kFloat32, "dropout: bf16 / fp32");
  TORCH_CHECK(x.numel() % 8 == 0, "dropout: numel % 8");
  auto [thr, scale] = keep_params(rate);
  auto y = torch::empty_like(x);
  check_rc(jm_dropout_apply(x.data_ptr(), y.data_ptr(), x.numel(), x.scalar_type() == torch::kBFloat16,
                            seed.data_ptr<int64_t>(), thr, scale, stream()),
           "dropout_apply");
  return y;
}

// rows of fp32 logits [..., S] -> (softmax p (saved for the backward), dropped p * mask / keep)
// x *= keep(seed, i) / keep in place (bf16 or fp32, contiguous, numel % 8 == 0): the fused
// blocks' Dense-output dropout (forward on the branch output, backward on its gradient)
void dropout_apply_(torch::Tensor x, torch::Tensor seed, double rate) {
  CHECK_CUDA(x);
  check_seed(seed, x);
  TORCH_CHECK(x.is_contiguous() && x.numel() % 8 == 0, "dropout_apply_: contiguous, numel % 8 == 0");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 || x.scalar_type() == torch::kFloat32, "dropout: bf16 / fp32");
  const auto kp = keep_params(rate);
  check_rc(jm_dropout_apply(x.data_ptr(), x.data_ptr(), x.numel(), x.scalar_type() == torch::kBFloat16,
                            seed.data_ptr<int64_t>(), kp.first, kp.second, stream()),
           "dropout_apply_");
}

// FF hidden dropout: (g, gp) masked in place (pair = the fused epilogue's gelu(h), gelu'(h)), or
// from the pre-activation h: returns (gelu(h) m, gelu'(h) m)
std::vector<torch::Tensor> gelu_drop(torch::Tensor a, c10::optional<torch::Tensor> b, torch::Tensor seed, double rate) {
  CHECK_CONTIG(a);
  CHECK_DT(a, torch::kBFloat16);
  check_seed(seed, a);
  TORCH_CHECK(a.numel() % 8 == 0, "gelu_drop: numel % 8");
  const auto kp = keep_params(rate);
  if (b.has_value() && b->defined()) {
    CHECK_CONTIG((*b));
    TORCH_CHECK(b->sizes() == a.sizes() && b->scalar_type() == torch::kBFloat16, "gelu_drop: (g, gp) pair");
    check_rc(jm_gelu_drop(nullptr, bfm(a), bfm(*b), a.numel(), seed.data_ptr<int64_t>(), kp.first, kp.second,
                          stream()),
             "gelu_drop");
    return {a, *b};
  }
  auto g = torch::empty_like(a), gp = torch::empty_like(a);
  check_rc(jm_gelu_drop(bf(a), bfm(g), bfm(gp), a.numel(), seed.data_ptr<int64_t>(), kp.first, kp.second, stream()),
           "gelu_drop");
  return {g, gp};
}

std::vector<torch::Tensor> softmax_dropout_fwd(torch::Tensor z, torch::Tensor seed, double rate) {
  CHECK_CONTIG(z);
  CHECK_DT(z, torch::kFloat32);
  check_seed(seed, z);
  auto [thr, scale] = keep_params(rate);
  const int S = z.size(-1);
  auto p = torch::empty_like(z);
  auto pd = torch::empty_like(z);
  check_rc(jm_softmax_dropout_fwd(z.data_ptr<float>(), p.data_ptr<float>(), pd.data_ptr<float>(), z.numel() / S, S,
                                  seed.data_ptr<int64_t>(), thr, scale, stream()),
           "softmax_dropout_fwd");
  return {p, pd};
}

torch::Tensor softmax_dropout_bwd(torch::Tensor dpd, torch::Tensor p, torch::Tensor seed, double rate) {
  CHECK_CONTIG(dpd);
  CHECK_CONTIG(p);
  CHECK_DT(dpd, torch::kFloat32);
  CHECK_DT(p, torch::kFloat32);
  TORCH_CHECK(dpd.sizes() == p.sizes(), "softmax_dropout_bwd shapes");
  check_seed(seed, p);
  auto [thr, scale] = keep_params(rate);
  const int S = p.size(-1);
  auto dz = torch::empty_like(p);
  check_rc(jm_softmax_dropout_bwd(dpd.data_ptr<float>(), p.data_ptr<float>(), dz.data_ptr<float>(), p.numel() / S, S,
                                  seed.data_ptr<int64_t>(), thr, scale, stream()),
           "softmax_dropout_bwd");
  return dz;
}

// dst [C, R] = src [R, C]^T (bf16, both contiguous)
void transpose_bf16(torch::Tensor src, torch::Tensor dst) {
  CHECK_CONTIG(src);
  CHECK_CONTIG(dst);
  CHECK_DT(src, torch::kBFloat16);
  CHECK_DT(dst, torch::kBFloat16);
  TORCH_CHECK(src.dim() == 2 && dst.dim() == 2 && dst.size(0) == src.size(1) && dst.size(1) == src.size(0),
              "transpose_bf16 shapes");
  check_rc(jm_transpose_bf16(bf(src), bfm(dst), src.size(0), src.size(1), stream()), "transpose_bf16");
}

// all transposed weight copies of a step in one launch: desc int64 [n, 6] on the device
// ({src, dst, R, C, first tile, tiles along C}, built by ParamStore.refresh_transposes)
void transpose_bf16_batch(torch::Tensor desc, int64_t tiles) {
  CHECK_CONTIG(desc);
  TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == torch::kInt64 && desc.dim() == 2 && desc.size(1) == 6,
              "transpose_bf16_batch: desc int64 [n, 6] on the device");
  check_rc(jm_transpose_bf16_batch(reinterpret_cast<const long long*>(desc.data_ptr<int64_t>()), (int)desc.size(0),
                                   (int)tiles, stream()),
           "transpose_bf16_batch");
}

// ------------------------------------------------------------------------------ weight gradients
using Tensors = std::vector<torch::Tensor>;

// One-split grouped launches store into every G or accumulate into every G (one kernel variant):
// with mixed store flags the store problems' G are zeroed first and all accumulate.  Returns the
// launch's store mode.
int group_stores(const std::vector<bool>& stores, const Tensors& gs, int S, int n) {
  if (S > 1 || stores.empty()) return 0;
  int ns = 0;
  for (int p = 0; p < n; ++p) ns += p < (int)stores.size() && stores[p];
  if (ns == n) return 1;
  for (int p = 0; p < n; ++p)
    if (p < (int)stores.size() && stores[p])
      jm_zero_f32(gs[p].data_ptr<float>(), gs[p].numel(), stream());
  return 0;
}

// gs[p] [N_p, K_p] += sum_i dys[p][i]^T . xs[p][i] on the TN MFMA kernels (csrc/gemm_tn.hip): up to
// 4 problems over the same M rows in ONE grid (fewer M splits per problem than separate launches,
// so fewer fp32 partial slices to write and reduce), the M rows split over S workgroups per tile
// and the partial slices reduced into gs[p]; returns S.  segmented: the M rows of each problem are
// its 1..32 row blocks (same shape and strides), read in place -- no torch.cat copy -- for at most
// 2 problems; else one block per problem.  stores[p]: gs[p] = the product (its old contents
// ignored: the first contribution of a step) instead of +=.
int64_t tn_wgrad(const char* what, const std::vector<Tensors>& dys, const std::vector<Tensors>& xs, const Tensors& gs,
                 const std::vector<bool>& stores, bool segmented) {
  const int np = (int)dys.size(), max_np = segmented ? 2 : 4, max_nb = segmented ? 32 : 1;
  TORCH_CHECK(np >= 1 && np <= max_np && (int)xs.size() == np && (int)gs.size() == np, what, ": 1..", max_np,
              " problems, each with its dy, x and g");
  const int nb = (int)dys[0].size();
  TORCH_CHECK(nb >= 1 && nb <= max_nb, what, ": 1..", max_nb, " row blocks");
  const auto dev = gs[0].device();
  TORCH_CHECK(dev.is_cuda(), what, ": g must be a GPU tensor");
  TnGroup grp{};
  TnSegs segs{};
  grp.n = np;
  int64_t rows = -1, total = 0;
  for (int p = 0; p < np; ++p) {
    TORCH_CHECK((int)dys[p].size() == nb && (int)xs[p].size() == nb, what, ": block counts differ");
    const auto &d0 = dys[p][0], &x0 = xs[p][0];
    for (int i = 0; i < nb; ++i) {
      const auto &d = dys[p][i], &x = xs[p][i];
      TORCH_CHECK(d.scalar_type() == torch::kBFloat16 && x.scalar_type() == torch::kBFloat16, what,
                  ": dy and x must be bf16");
      TORCH_CHECK(d.device() == dev && x.device() == dev, what, ": dy and x must be on g's GPU");
      TORCH_CHECK(d.dim() == 2 && x.dim() == 2 && d.stride(1) == 1 && x.stride(1) == 1, what,
                  ": dy [M,N], x [M,K] with contiguous rows");
      if (rows < 0) rows = d.size(0);
      TORCH_CHECK(d.size(0) == rows && x.size(0) == rows, what, ": dy and x of every problem and block have one M");
      TORCH_CHECK(d.size(1) == d0.size(1) && x.size(1) == x0.size(1) && d.stride(0) == d0.stride(0) &&
                      x.stride(0) == x0.stride(0),
                  what, ": block shapes / strides differ");
      if (segmented) {
        segs.a[32 * p + i] = bf(d);
        segs.b[32 * p + i] = bf(x);
      }
    }
    const int64_t N = d0.size(1), K = x0.size(1);
    TORCH_CHECK(N > 0 && K > 0 && N % 256 == 0 && K % 256 == 0, what, ": N, K multiples of 256");
    const auto& g = gs[p];
    TORCH_CHECK(g.device() == dev && g.scalar_type() == torch::kFloat32 && g.is_contiguous() && g.numel() == N * K,
                what, ": g must be fp32 [N,K], contiguous, on one GPU");
    if (!segmented) {
      grp.a[p] = bf(d0);
      grp.b[p] = bf(x0);
    }
    grp.lda[p] = d0.stride(0);
    grp.ldb[p] = x0.stride(0);
    grp.N[p] = (int)N;
    grp.K[p] = (int)K;
    total += N * K;
  }
  TORCH_CHECK(rows >= 1 && rows * nb <= INT_MAX, what, ": M out of range");
  const int M = (int)(rows * nb);
  segs.rows = (int)rows;
  segs.n = nb;
  int S = 1;
  const int sps = jm_gemm_tn_plan(grp, M, &S);
  torch::Tensor part;  // fp32 partial slices [S][N_p K_p] per problem, reduced into gs[p]
  if (S > 1) part = torch::empty({S * total}, gs[0].options());
  int64_t off = 0;
  for (int p = 0; p < np; ++p) {
    grp.out[p] = S > 1 ? part.data_ptr<float>() + off : gs[p].data_ptr<float>();
    off += (int64_t)S * grp.N[p] * grp.K[p];
  }
  const int all_store = group_stores(stores, gs, S, np);
  check_rc(jm_gemm_tn(grp, segmented ? &segs : nullptr, M, sps, S, stream(), all_store), what);
  if (S > 1)
    for (int p = 0; p < np; ++p)
      check_rc(jm_splitk_reduce_add(grp.out[p], gs[p].data_ptr<float>(), (long)grp.N[p] * grp.K[p], S, stream(),
                                    p < (int)stores.size() && stores[p]),
               what);
  return S;
}

// the Python-visible forms: one problem or several, contiguous rows or row blocks
int64_t gemm_tn_wgrad(torch::Tensor dy, torch::Tensor x, torch::Tensor g, bool store) {
  return tn_wgrad("gemm_tn_wgrad", {Tensors{dy}}, {Tensors{x}}, {g}, {store}, false);
}

int64_t gemm_tn_wgrad_seg(Tensors dys, Tensors xs, torch::Tensor g, bool store) {
  return tn_wgrad("gemm_tn_wgrad_seg", {dys}, {xs}, {g}, {store}, true);
}

int64_t gemm_tn_wgrad_group(Tensors dys, Tensors xs, Tensors gs, std::vector<bool> stores) {
  std::vector<Tensors> d, x;
  for (const auto& t : dys) d.push_back({t});
  for (const auto& t : xs) x.push_back({t});
  return tn_wgrad("gemm_tn_wgrad_group", d, x, gs, stores, false);
}

int64_t gemm_tn_wgrad_seg_group(std::vector<Tensors> dys, std::vector<Tensors> xs, Tensors gs,
                                std::vector<bool> stores) {
  return tn_wgrad("gemm_tn_wgrad_seg_group", dys, xs, gs, stores, true);
}

// zero the (offset, count) float ranges of ``base`` listed in desc (int64 [n, 2] on the device)
void zero_ranges(torch::Tensor base, torch::Tensor desc, int64_t blocks) {
  CHECK_CONTIG(base);
  CHECK_DT(base, torch::kFloat32);
  TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == torch::kInt64 && desc.dim() == 2 && desc.size(1) == 2,
              "zero_ranges: desc int64 [n, 2] on the device");
  check_rc(jm_zero_ranges(base.data_ptr<float>(), reinterpret_cast<const long long*>(desc.data_ptr<int64_t>()),
                          (int)desc.size(0), blocks, stream()),
           "zero_ranges");
}

// x1 = x + mask*scale*y ([B,T,D] fp32, fresh contiguous); h / mean / rstd = LN of rows t >= T0
std::vector<torch::Tensor> residual_ln_fwd(torch::Tensor x, torch::Tensor y, c10::optional<torch::Tensor> scale,
                                           c10::optional<torch::Tensor> mask, torch::Tensor gamma,
                                           torch::Tensor beta, double eps, int64_t T0, int64_t R0,
                                           c10::optional<torch::Tensor> out, c10::optional<torch::Tensor> seed,
                                           double rate) {
  CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 3 && x.stride(2) == 1, "x must be [B,T,D] with contiguous last dim");
  CHECK_DT(x, torch::kFloat32);
  CHECK_DT(y, torch::kBFloat16);
  CHECK_CONTIG(y);
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  TORCH_CHECK(R0 >= 0 && R0 < T, "residual_ln_fwd: R0");
  TORCH_CHECK(y.numel() == (long)B * (T - R0) * D, "residual_ln_fwd: y must be [B*(T-R0), D]");
  TORCH_CHECK(T0 >= 0 && T0 < T, "residual_ln_fwd: T0");
  TORCH_CHECK(R0 == 0 || out.has_value(), "residual_ln_fwd: R0 > 0 needs out (its rows t < R0 are inputs)");
  torch::Tensor x1;
  if (out) {
    CHECK_DT(*out, torch::kFloat32);
    TORCH_CHECK(out->dim() == 3 && out->size(0) == B && out->size(1) == T && out->size(2) == D && out->stride(2) == 1,
                "residual_ln_fwd: out must be [B,T,D] with contiguous last dim");
    x1 = *out;
  } else {
    x1 = torch::empty({B, T, D}, x.options());
  }
  const long R = (long)B * (T - T0);
  auto h = torch::empty({R, D}, y.options());
  auto mean = torch::empty({R}, x.options());
  auto rstd = torch::empty({R}, x.options());
  check_rc(jm_residual_ln_fwd(x.data_ptr<float>(), x.stride(0), x.stride(1), bf(y), fopt(scale), fopt(mask),
                              x1.data_ptr<float>(), x1.stride(0), x1.stride(1), bfm(h), mean.data_ptr<float>(),
                              rstd.data_ptr<float>(), B, T, T0, D, gamma.data_ptr<float>(), beta.data_ptr<float>(),
                              (float)eps, stream(), (int)R0, make_drop(seed, rate, y, 0)),
           "residual_ln_fwd");
  return {x1, h, mean, rstd};
}

// ------------------------------------------------------------------------------ classification loss
// Shared argument checks of cls_loss_fwd / cls_loss_bwd; returns (perm, w) device pointers or nulls
static std::pair<const int*, const float*> check_cls_loss(const torch::Tensor& logits, const torch::Tensor& labels,
                                                          const c10::optional<torch::Tensor>& perm,
                                                          const c10::optional<torch::Tensor>& w, double smoothing,
                                                          int64_t mode) {
  CHECK_CUDA(logits);
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 || logits.scalar_type() == torch::kFloat32,
              "cls_loss: logits must be bf16 or fp32");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1, "cls_loss: logits must be [B, L]");
  TORCH_CHECK(logits.stride(1) == 1, "cls_loss: logits must have a unit column stride");
  TORCH_CHECK(logits.size(0) == 1 || logits.stride(0) >= logits.size(1), "cls_loss: logits rows must not overlap");
  TORCH_CHECK(logits.size(0) < INT_MAX && logits.size(1) < INT_MAX, "cls_loss: logits too large");
  const int64_t B = logits.size(0);
  TORCH_CHECK(labels.device() == logits.device() && labels.scalar_type() == torch::kInt64 && labels.dim() == 1 &&
                  labels.size(0) == B && labels.is_contiguous(),
              "cls_loss: labels must be int64 [B] on the logits' device");
  TORCH_CHECK(mode == 0 || mode == 1, "cls_loss: mode 0 (ce) or 1 (bce)");
  TORCH_CHECK(smoothing >= 0.0 && smoothing < 1.0, "cls_loss: smoothing must be in [0, 1)");
  const bool hp = perm.has_value() && perm->defined(), hw = w.has_value() && w->defined();
  TORCH_CHECK(hp == hw, "cls_loss: perm and w come together");
  if (!hp) return {nullptr, nullptr};
  TORCH_CHECK(perm->device() == logits.device() && perm->scalar_type() == torch::kInt32 && perm->dim() == 1 &&
                  perm->size(0) == B && perm->is_contiguous(),
              "cls_loss: perm must be int32 [B] on the logits' device");
  TORCH_CHECK(w->device() == logits.device() && w->scalar_type() == torch::kFloat32 && w->numel() == 1,
              "cls_loss: w must be one fp32 element on the logits' device");
  return {perm->data_ptr<int>(), w->data_ptr<float>()};
}

// a single row's stride is never used (and may be anything): the row length then
static long row_stride(const torch::Tensor& logits) { return logits.size(0) == 1 ? logits.size(1) : logits.stride(0); }

// [loss fp32 [B], hit bool [B, 2] (top-1, top-5), lse fp32 [B, 2] (hi, lo; zeros for bce)]
std::vector<torch::Tensor> cls_loss_fwd(torch::Tensor logits, torch::Tensor labels, c10::optional<torch::Tensor> perm,
                                        c10::optional<torch::Tensor> w, double smoothing, int64_t mode) {
  const auto pw = check_cls_loss(logits, labels, perm, w, smoothing, mode);
  const int64_t B = logits.size(0);
  auto loss = torch::empty({B}, logits.options().dtype(torch::kFloat32));
  auto hit = torch::empty({B, 2}, logits.options().dtype(torch::kBool));
  auto lse = torch::empty({B, 2}, logits.options().dtype(torch::kFloat32));
  check_rc(jm_cls_loss_fwd(logits.data_ptr(), logits.scalar_type() == torch::kBFloat16, row_stride(logits),
                           labels.data_ptr<int64_t>(), pw.first, pw.second, smoothing, (int)mode, (int)B,
                           (int)logits.size(1), loss.data_ptr<float>(), reinterpret_cast<uint8_t*>(hit.data_ptr()),
                           lse.data_ptr<float>(), stream()),
           "cls_loss_fwd");
  return {loss, hit, lse};
}

// dlogits [B, L] contiguous, in the dtype of logits
torch::Tensor cls_loss_bwd(torch::Tensor dloss, torch::Tensor logits, torch::Tensor labels,
                           c10::optional<torch::Tensor> perm, c10::optional<torch::Tensor> w, double smoothing,
                           int64_t mode, torch::Tensor lse) {
  const auto pw = check_cls_loss(logits, labels, perm, w, smoothing, mode);
  const int64_t B = logits.size(0), L = logits.size(1);
  TORCH_CHECK(lse.device() == logits.device() && lse.scalar_type() == torch::kFloat32 && lse.dim() == 2 &&
                  lse.size(0) == B && lse.size(1) == 2 && lse.is_contiguous(),
              "cls_loss_bwd: lse must be the forward's fp32 [B, 2]");
  TORCH_CHECK(dloss.device() == logits.device() && dloss.scalar_type() == torch::kFloat32 && dloss.dim() == 1 &&
                  dloss.size(0) == B && dloss.is_contiguous(),
              "cls_loss_bwd: dloss must be fp32 [B] on the logits' device");
  auto dlogits = torch::empty({B, L}, logits.options());
  check_rc(jm_cls_loss_bwd(logits.data_ptr(), logits.scalar_type() == torch::kBFloat16, row_stride(logits),
                           labels.data_ptr<int64_t>(), pw.first, pw.second, smoothing, (int)mode, (int)B, (int)L,
                           lse.data_ptr<float>(), dloss.data_ptr<float>(), dlogits.data_ptr(), L, stream()),
           "cls_loss_bwd");
  return dlogits;
}

// ------------------------------------------------------------------------------ distillation loss
// Shared argument checks of kd_loss_fwd / kd_loss_bwd (u may be undefined where the caller allows it)
static void check_kd_logits(const torch::Tensor& t, const char* what) {
  CHECK_CUDA(t);
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, "kd_loss: ", what,
              " must be bf16 or fp32");
  TORCH_CHECK(t.dim() == 2 && t.size(0) >= 1 && t.size(1) >= 1, "kd_loss: ", what, " must be [B, L]");
  TORCH_CHECK(t.stride(1) == 1, "kd_loss: ", what, " must have a unit column stride");
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= t.size(1), "kd_loss: ", what, " rows must not overlap");
  TORCH_CHECK(t.size(0) < INT_MAX && t.size(1) < INT_MAX, "kd_loss: ", what, " too large");
}

static void check_kd(const torch::Tensor& z, const torch::Tensor* u, double temp, int64_t mode) {
  check_kd_logits(z, "z");
  if (u) {
    check_kd_logits(*u, "u");
    TORCH_CHECK(u->device() == z.device() && u->scalar_type() == z.scalar_type() && u->sizes() == z.sizes(),
                "kd_loss: u must have the dtype, shape and device of z");
  }
  TORCH_CHECK(mode == 0 || mode == 1, "kd_loss: mode 0 (soft) or 1 (hard)");
  TORCH_CHECK(temp > 0.0 && std::isfinite(temp), "kd_loss: the temperature must be positive");
}

// [kd fp32 [B], agree bool [B], lse fp32 [B, 4], t int32 [B] (the teacher's arg-max)]
std::vector<torch::Tensor> kd_loss_fwd(torch::Tensor z, torch::Tensor u, double temp, int64_t mode) {
  check_kd(z, &u, temp, mode);
  const int64_t B = z.size(0);
  auto kd = torch::empty({B}, z.options().dtype(torch::kFloat32));
  auto agree = torch::empty({B}, z.options().dtype(torch::kBool));
  auto lse = torch::empty({B, 4}, z.options().dtype(torch::kFloat32));
  auto targ = torch::empty({B}, z.options().dtype(torch::kInt32));
  check_rc(jm_kd_loss_fwd(z.data_ptr(), row_stride(z), u.data_ptr(), row_stride(u),
                          z.scalar_type() == torch::kBFloat16, temp, (int)mode, (int)B, (int)z.size(1),
                          kd.data_ptr<float>(), reinterpret_cast<uint8_t*>(agree.data_ptr()), lse.data_ptr<float>(),
                          targ.data_ptr<int>(), stream()),
           "kd_loss_fwd");
  return {kd, agree, lse, targ};
}

// dz [B, L] contiguous, in the dtype of z; u: soft mode only, t: hard mode only
torch::Tensor kd_loss_bwd(torch::Tensor dloss, torch::Tensor z, c10::optional<torch::Tensor> u, double temp,
                          int64_t mode, torch::Tensor lse, c10::optional<torch::Tensor> t) {
  const bool hu = u.has_value() && u->defined(), ht = t.has_value() && t->defined();
  check_kd(z, hu ? &*u : nullptr, temp, mode);
  const int64_t B = z.size(0), L = z.size(1);
  TORCH_CHECK(mode == 0 ? hu : ht, "kd_loss_bwd: soft mode needs u, hard mode needs t");
  TORCH_CHECK(lse.device() == z.device() && lse.scalar_type() == torch::kFloat32 && lse.dim() == 2 &&
                  lse.size(0) == B && lse.size(1) == 4 && lse.is_contiguous(),
              "kd_loss_bwd: lse must be the forward's fp32 [B, 4]");
  TORCH_CHECK(dloss.device() == z.device() && dloss.scalar_type() == torch::kFloat32 && dloss.dim() == 1 &&
                  dloss.size(0) == B && dloss.is_contiguous(),
              "kd_loss_bwd: dloss must be fp32 [B] on the logits' device");
  if (mode == 1)
    TORCH_CHECK(t->device() == z.device() && t->scalar_type() == torch::kInt32 && t->dim() == 1 && t->size(0) == B &&
                    t->is_contiguous(),
                "kd_loss_bwd: t must be the forward's int32 [B]");
  auto dz = torch::empty({B, L}, z.options());
  const bool soft = mode == 0;
  check_rc(jm_kd_loss_bwd(z.data_ptr(), row_stride(z), soft ? u->data_ptr() : nullptr, soft ? row_stride(*u) : 0,
                          z.scalar_type() == torch::kBFloat16, temp, (int)mode, (int)B, (int)L, lse.data_ptr<float>(),
                          soft ? nullptr : t->data_ptr<int>(), dloss.data_ptr<float>(), dz.data_ptr(), L, stream()),
           "kd_loss_bwd");
  return dz;
}

// ------------------------------------------------------------------------------ evaluation report
static void check_eval_vec(const torch::Tensor& t, const torch::Tensor& like, torch::ScalarType dt, int64_t B,
                           const char* what) {
  TORCH_CHECK(t.device() == like.device() && t.scalar_type() == dt && t.dim() == 1 && t.size(0) == B &&
                  t.is_contiguous(),
              "eval_report: ", what, " must be a contiguous [B] vector of its dtype on the labels' device");
}

// [pred int32 [B], rank int32 [B], conf fp32 [B]]; padded (label -1) and non-finite rows: -1, -1, 0
std::vector<torch::Tensor> eval_rows(torch::Tensor logits, torch::Tensor labels, int64_t mode) {
  CHECK_CUDA(logits);
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 || logits.scalar_type() == torch::kFloat32,
              "eval_rows: logits must be bf16 or fp32");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1, "eval_rows: logits must be [B, L]");
  TORCH_CHECK(logits.stride(1) == 1, "eval_rows: logits must have a unit column stride");
  TORCH_CHECK(logits.size(0) == 1 || logits.stride(0) >= logits.size(1), "eval_rows: logits rows must not overlap");
  TORCH_CHECK(logits.size(0) < INT_MAX && logits.size(1) < INT_MAX, "eval_rows: logits too large");
  TORCH_CHECK(mode == 0 || mode == 1, "eval_rows: mode 0 (ce) or 1 (bce)");
  const int64_t B = logits.size(0);
  check_eval_vec(labels, logits, torch::kInt64, B, "labels");
  auto pred = torch::empty({B}, logits.options().dtype(torch::kInt32));
  auto rank = torch::empty({B}, logits.options().dtype(torch::kInt32));
  auto conf = torch::empty({B}, logits.options().dtype(torch::kFloat32));
  check_rc(jm_eval_rows(logits.data_ptr(), logits.scalar_type() == torch::kBFloat16, row_stride(logits),
                        labels.data_ptr<int64_t>(), (int)mode, (int)B, (int)logits.size(1), pred.data_ptr<int>(),
                        rank.data_ptr<int>(), conf.data_ptr<float>(), stream()),
           "eval_rows");
  return {pred, rank, conf};
}

int64_t eval_state_words(int64_t L, int64_t n_bins) {
  TORCH_CHECK(L >= 1 && L < INT_MAX && n_bins >= 1 && n_bins <= JM_EVAL_MAX_BINS,
              "eval_report: L >= 1 and 1 <= n_bins <= ", JM_EVAL_MAX_BINS);
  return jm_eval_state_words((int)L, (int)n_bins);
}

// state (int64, eval_state_words(L, n_bins) words) += the batch
void eval_accumulate(torch::Tensor labels, torch::Tensor pred, torch::Tensor rank, torch::Tensor conf, int64_t L,
                     int64_t n_bins, torch::Tensor state) {
  CHECK_CUDA(labels);
  const int64_t B = labels.numel();
  TORCH_CHECK(B >= 1 && B < INT_MAX, "eval_accumulate: 1 <= B < 2^31");
  check_eval_vec(labels, labels, torch::kInt64, B, "labels");
  check_eval_vec(pred, labels, torch::kInt32, B, "pred");
  check_eval_vec(rank, labels, torch::kInt32, B, "rank");
  check_eval_vec(conf, labels, torch::kFloat32, B, "conf");
  const int64_t words = eval_state_words(L, n_bins);
  TORCH_CHECK(state.device() == labels.device() && state.scalar_type() == torch::kInt64 && state.dim() == 1 &&
                  state.is_contiguous() && state.size(0) == words,
              "eval_accumulate: state must be int64 [", words, "] on the labels' device");
  check_rc(jm_eval_accumulate(labels.data_ptr<int64_t>(), pred.data_ptr<int>(), rank.data_ptr<int>(),
                              conf.data_ptr<float>(), (int)B, (int)L, (int)n_bins, state.data_ptr<int64_t>(),
                              stream()),
           "eval_accumulate");
}

// ------------------------------------------------------------------------------ batch norm
// Argument checks of the bn_* entry points.  Dtypes, shapes and strides are checked before the
// devices, and everything before any launch, so each message can be reached with CPU tensors.
// A [B, J] operand `what` (x, dy, out): dtype (bf16 allowed or fp32 only), 2-D, unit column stride, rows apart
static void check_bn_mat(const torch::Tensor& t, const char* fn, const char* what, bool bf16_ok) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 || (bf16_ok && t.scalar_type() == torch::kBFloat16), fn, ": ", what,
              bf16_ok ? " must be bf16 or fp32" : " must be fp32");
  TORCH_CHECK(t.dim() == 2 && t.size(0) >= 1 && t.size(1) >= 1, fn, ": ", what, " must be [B, J]");
  TORCH_CHECK(t.stride(1) == 1, fn, ": ", what, " must have a unit column stride");
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= t.size(1), fn, ": ", what, " rows must not overlap");
  TORCH_CHECK(t.size(0) < INT_MAX && t.size(1) < INT_MAX, fn, ": ", what, " too large");
}

// a second [B, J] operand against x
static void check_bn_like(const torch::Tensor& t, const torch::Tensor& x, const char* fn, const char* what,
                          bool bf16_ok) {
  check_bn_mat(t, fn, what, bf16_ok);
  TORCH_CHECK(t.size(0) == x.size(0) && t.size(1) == x.size(1), fn, ": ", what, " must have the shape of x");
}

// a contiguous fp32 vector of n elements
static void check_bn_vec(const torch::Tensor& t, int64_t n, const char* fn, const char* what, const char* shape) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.dim() == 1 && t.size(0) == n && t.is_contiguous(), fn, ": ",
              what, " must be fp32 ", shape);
}

// last: one device, a GPU
static void check_bn_device(const torch::Tensor& x, std::initializer_list<const torch::Tensor*> others,
                            const char* fn) {
  for (const torch::Tensor* t : others)
    TORCH_CHECK(t->device() == x.device(), fn, ": all tensors must be on the device of x");
  TORCH_CHECK(x.is_cuda(), fn, ": x must be a GPU tensor");
}

static bool bn_out_bf16(py::object out_dtype, const char* fn) {
  const auto odt = torch::python::detail::py_object_to_dtype(out_dtype);
  TORCH_CHECK(odt == torch::kBFloat16 || odt == torch::kFloat32, fn, ": out_dtype must be bf16 or fp32");
  return odt == torch::kBFloat16;
}

static torch::Tensor bn_part(const torch::Tensor& x) {
  return torch::empty({(int64_t)jm_bn_chunks((int)x.size(0)), 2, x.size(1)}, x.options().dtype(torch::kFloat64));
}

// packed fp32 [2 J] = [mean, mean of squares] of the rows of x
torch::Tensor bn_stats(torch::Tensor x) {
  check_bn_mat(x, "bn_stats", "x", false);
  check_bn_device(x, {}, "bn_stats");
  const int64_t B = x.size(0), J = x.size(1);
  auto part = bn_part(x);
  auto packed = torch::empty({2 * J}, x.options());
  check_rc(jm_bn_stats(x.data_ptr<float>(), row_stride(x), (int)B, (int)J, part.data_ptr<double>(),
                       packed.data_ptr<float>(), stream()),
           "bn_stats");
  return packed;
}

// [y (out_dtype; written into out when given), stats fp32 [2, J] = (mean, rstd)]; the running statistics move in place
std::vector<torch::Tensor> bn_apply(torch::Tensor x, torch::Tensor packed, torch::Tensor gamma, torch::Tensor beta,
                                    torch::Tensor running_mean, torch::Tensor running_var, double eps, double momentum,
                                    py::object out_dtype, c10::optional<torch::Tensor> out) {
  const char* fn = "bn_apply";
  check_bn_mat(x, fn, "x", false);
  const int64_t B = x.size(0), J = x.size(1);
  check_bn_vec(packed, 2 * J, fn, "packed", "[2 J]");
  check_bn_vec(gamma, J, fn, "gamma", "[J]");
  check_bn_vec(beta, J, fn, "beta", "[J]");
  check_bn_vec(running_mean, J, fn, "running_mean", "[J]");
  check_bn_vec(running_var, J, fn, "running_var", "[J]");
  const bool bf16 = bn_out_bf16(out_dtype, fn);
  TORCH_CHECK(eps > 0.0 && momentum >= 0.0 && momentum <= 1.0, fn, ": eps > 0 and momentum in [0, 1]");
  const bool has_out = out.has_value() && out->defined();
  if (has_out) {
    check_bn_like(*out, x, fn, "out", true);
    TORCH_CHECK((out->scalar_type() == torch::kBFloat16) == bf16, fn, ": out must have out_dtype");
    check_bn_device(x, {&packed, &gamma, &beta, &running_mean, &running_var, &*out}, fn);
  } else {
    check_bn_device(x, {&packed, &gamma, &beta, &running_mean, &running_var}, fn);
  }
  auto y = has_out ? *out : torch::empty({B, J}, x.options().dtype(bf16 ? torch::kBFloat16 : torch::kFloat32));
  auto stats = torch::empty({2, J}, x.options());
  check_rc(jm_bn_apply(x.data_ptr<float>(), row_stride(x), (int)B, (int)J, packed.data_ptr<float>(),
                       gamma.data_ptr<float>(), beta.data_ptr<float>(), eps, momentum, y.data_ptr(), bf16,
                       row_stride(y), stats.data_ptr<float>(), running_mean.data_ptr<float>(),
                       running_var.data_ptr<float>(), stream()),
           fn);
  return {y, stats};
}

// y from the running statistics (inference); nothing else is written
torch::Tensor bn_apply_eval(torch::Tensor x, torch::Tensor running_mean, torch::Tensor running_var, torch::Tensor gamma,
                            torch::Tensor beta, double eps, py::object out_dtype, c10::optional<torch::Tensor> out) {
  const char* fn = "bn_apply_eval";
  check_bn_mat(x, fn, "x", false);
  const int64_t B = x.size(0), J = x.size(1);
  check_bn_vec(running_mean, J, fn, "running_mean", "[J]");
  check_bn_vec(running_var, J, fn, "running_var", "[J]");
  check_bn_vec(gamma, J, fn, "gamma", "[J]");
  check_bn_vec(beta, J, fn, "beta", "[J]");
  const bool bf16 = bn_out_bf16(out_dtype, fn);
  TORCH_CHECK(eps > 0.0, fn, ": eps > 0");
  const bool has_out = out.has_value() && out->defined();
  if (has_out) {
    check_bn_like(*out, x, fn, "out", true);
    TORCH_CHECK((out->scalar_type() == torch::kBFloat16) == bf16, fn, ": out must have out_dtype");
    check_bn_device(x, {&running_mean, &running_var, &gamma, &beta, &*out}, fn);
  } else {
    check_bn_device(x, {&running_mean, &running_var, &gamma, &beta}, fn);
  }
  auto y = has_out ? *out : torch::empty({B, J}, x.options().dtype(bf16 ? torch::kBFloat16 : torch::kFloat32));
  check_rc(jm_bn_apply_eval(x.data_ptr<float>(), row_stride(x), (int)B, (int)J, running_mean.data_ptr<float>(),
                            running_var.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(), eps,
                            y.data_ptr(), bf16, row_stride(y), stream()),
           fn);
  return y;
}

// shared by the two backward entry points
static void check_bn_bwd(const torch::Tensor& dy, const torch::Tensor& x, const torch::Tensor& stats,
                         const torch::Tensor& gamma, const char* fn) {
  check_bn_mat(x, fn, "x", false);
  check_bn_like(dy, x, fn, "dy", true);
  const int64_t J = x.size(1);
  TORCH_CHECK(stats.scalar_type() == torch::kFloat32 && stats.dim() == 2 && stats.size(0) == 2 && stats.size(1) == J &&
                  stats.is_contiguous(),
              fn, ": stats must be the forward's fp32 [2, J]");
  check_bn_vec(gamma, J, fn, "gamma", "[J]");
}

// [dgamma, dbeta, packed_g fp32 [2 J] = gamma (sum dy, sum dy xhat)]; dgamma / dbeta given: added to in place
std::vector<torch::Tensor> bn_bwd_reduce(torch::Tensor dy, torch::Tensor x, torch::Tensor stats, torch::Tensor gamma,
                                         c10::optional<torch::Tensor> dgamma, c10::optional<torch::Tensor> dbeta) {
  const char* fn = "bn_bwd_reduce";
  check_bn_bwd(dy, x, stats, gamma, fn);
  const int64_t B = x.size(0), J = x.size(1);
  const bool acc = dgamma.has_value() && dgamma->defined();
  TORCH_CHECK(acc == (dbeta.has_value() && dbeta->defined()), fn, ": dgamma and dbeta come together");
  if (acc) {
    check_bn_vec(*dgamma, J, fn, "dgamma", "[J]");
    check_bn_vec(*dbeta, J, fn, "dbeta", "[J]");
    check_bn_device(x, {&dy, &stats, &gamma, &*dgamma, &*dbeta}, fn);
  } else {
    check_bn_device(x, {&dy, &stats, &gamma}, fn);
  }
  auto dg = acc ? *dgamma : torch::empty({J}, x.options());
  auto db = acc ? *dbeta : torch::empty({J}, x.options());
  auto part = bn_part(x);
  auto packed_g = torch::empty({2 * J}, x.options());
  check_rc(jm_bn_bwd_reduce(dy.data_ptr(), dy.scalar_type() == torch::kBFloat16, row_stride(dy), x.data_ptr<float>(),
                            row_stride(x), (int)B, (int)J, stats.data_ptr<float>(), gamma.data_ptr<float>(),
                            part.data_ptr<double>(), dg.data_ptr<float>(), db.data_ptr<float>(), acc,
                            packed_g.data_ptr<float>(), stream()),
           fn);
  return {dg, db, packed_g};
}

// dx fp32 [B, J] (written into out when given); n = rows of the global batch
torch::Tensor bn_bwd_dx(torch::Tensor dy, torch::Tensor x, torch::Tensor stats, torch::Tensor gamma,
                        torch::Tensor packed_g, double n, c10::optional<torch::Tensor> out) {
  const char* fn = "bn_bwd_dx";
  check_bn_bwd(dy, x, stats, gamma, fn);
  const int64_t B = x.size(0), J = x.size(1);
  check_bn_vec(packed_g, 2 * J, fn, "packed_g", "[2 J]");
  TORCH_CHECK(n >= (double)B, fn, ": n counts at least the local rows");
  const bool has_out = out.has_value() && out->defined();
  if (has_out) {
    check_bn_like(*out, x, fn, "out", false);
    check_bn_device(x, {&dy, &stats, &gamma, &packed_g, &*out}, fn);
  } else {
    check_bn_device(x, {&dy, &stats, &gamma, &packed_g}, fn);
  }
  auto dx = has_out ? *out : torch::empty({B, J}, x.options());
  check_rc(jm_bn_bwd_dx(dy.data_ptr(), dy.scalar_type() == torch::kBFloat16, row_stride(dy), x.data_ptr<float>(),
                        row_stride(x), (int)B, (int)J, stats.data_ptr<float>(), gamma.data_ptr<float>(),
                        packed_g.data_ptr<float>(), n, dx.data_ptr<float>(), row_stride(dx), stream()),
           fn);
  return dx;
}

// ------------------------------------------------------------------------------ k-NN monitor
static void check_knn_rows(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 && t.dim() == 2, "knn_topk: ", what, " must be bf16 [N, D]");
  TORCH_CHECK(t.size(1) >= 1 && t.stride(1) == 1, "knn_topk: ", what, " must have a unit column stride");
  TORCH_CHECK(t.size(0) <= 1 || t.stride(0) >= t.size(1), "knn_topk: ", what, " rows must not overlap");
  TORCH_CHECK(t.size(0) < INT_MAX && t.size(1) < INT_MAX, "knn_topk: ", what, " too large");
}

// a caller's [Nq, cols] output: contiguous, on the device of q
static void check_knn_out(const torch::Tensor& t, const torch::Tensor& q, int64_t rows, int64_t cols,
                          torch::ScalarType dt, const char* fn, const char* what) {
  TORCH_CHECK(t.scalar_type() == dt && t.dim() == 2 && t.size(0) == rows && t.size(1) == cols && t.is_contiguous() &&
                  t.device() == q.device(),
              fn, ": ", what, " must be a contiguous [Nq, ", cols, "] tensor of the right dtype on the inputs' device");
}

// (idx int32 [Nq, k], sim fp32 [Nq, k]); out_idx / out_sim given: written in place
std::vector<torch::Tensor> knn_topk(torch::Tensor q, torch::Tensor bank, int64_t k,
                                    c10::optional<torch::Tensor> self_idx, int64_t splits,
                                    c10::optional<torch::Tensor> out_idx, c10::optional<torch::Tensor> out_sim) {
  check_knn_rows(q, "q");
  check_knn_rows(bank, "bank");
  TORCH_CHECK(q.size(1) == bank.size(1), "knn_topk: q and bank must have the same D");
  TORCH_CHECK(q.size(1) % 32 == 0, "knn_topk: D must be a multiple of 32");
  TORCH_CHECK(k >= 1 && k <= 64, "knn_topk: k must be in 1..64");
  TORCH_CHECK(splits >= 0 && splits <= 1024, "knn_topk: splits must be in 0..1024");
  TORCH_CHECK(bank.size(0) >= 1, "knn_topk: the bank is empty");
  TORCH_CHECK(bank.device() == q.device(), "knn_topk: q and bank must be on one device");
  const int64_t Nq = q.size(0), Nb = bank.size(0);
  const int* sp = nullptr;
  if (self_idx.has_value() && self_idx->defined()) {
    TORCH_CHECK(self_idx->scalar_type() == torch::kInt32 && self_idx->dim() == 1 && self_idx->size(0) == Nq &&
                    self_idx->is_contiguous() && self_idx->device() == q.device(),
                "knn_topk: self_idx must be int32 [Nq] on the inputs' device");
    sp = self_idx->data_ptr<int>();
  }
  const bool has_out = out_idx.has_value() && out_idx->defined();
  TORCH_CHECK(has_out == (out_sim.has_value() && out_sim->defined()), "knn_topk: out_idx and out_sim come together");
  if (has_out) {
    check_knn_out(*out_idx, q, Nq, k, torch::kInt32, "knn_topk", "out_idx");
    check_knn_out(*out_sim, q, Nq, k, torch::kFloat32, "knn_topk", "out_sim");
  }
  TORCH_CHECK(q.is_cuda(), "knn_topk: q must be a GPU tensor");
  auto idx = has_out ? *out_idx : torch::empty({Nq, k}, q.options().dtype(torch::kInt32));
  auto sim = has_out ? *out_sim : torch::empty({Nq, k}, q.options().dtype(torch::kFloat32));
  if (Nq == 0) return {idx, sim};
  const int S = jm_knn_splits((int)Nq, (int)Nb, (int)splits);
  TORCH_CHECK(S >= 1, "knn_topk: unsupported shape");
  torch::Tensor sidx, ssim;
  if (S > 1) {
    sidx = torch::empty({S, Nq, k}, idx.options());
    ssim = torch::empty({S, Nq, k}, sim.options());
  }
  check_rc(jm_knn_topk(q.data_ptr(), row_stride(q), bank.data_ptr(), row_stride(bank), sp, (int)Nq, (int)Nb,
                       (int)q.size(1), (int)k, (int)splits, idx.data_ptr<int>(), sim.data_ptr<float>(),
                       S > 1 ? sidx.data_ptr<int>() : nullptr, S > 1 ? ssim.data_ptr<float>() : nullptr, stream()),
           "knn_topk");
  return {idx, sim};
}

// (pred int32 [Nq, 5], hit1 bool [Nq], hit5 bool [Nq])
std::vector<torch::Tensor> knn_vote(torch::Tensor idx, torch::Tensor sim, torch::Tensor bank_labels,
                                    torch::Tensor labels, double T) {
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.dim() == 2 && idx.is_contiguous(),
              "knn_vote: idx must be a contiguous int32 [Nq, k]");
  TORCH_CHECK(sim.scalar_type() == torch::kFloat32 && sim.dim() == 2 && sim.is_contiguous() &&
                  sim.size(0) == idx.size(0) && sim.size(1) == idx.size(1),
              "knn_vote: sim must be a contiguous fp32 [Nq, k]");
  const int64_t Nq = idx.size(0), k = idx.size(1);
  TORCH_CHECK(k >= 1 && k <= 64, "knn_vote: k must be in 1..64");
  TORCH_CHECK(bank_labels.scalar_type() == torch::kInt32 && bank_labels.dim() == 1 && bank_labels.is_contiguous() &&
                  bank_labels.size(0) >= 1 && bank_labels.size(0) < INT_MAX,
              "knn_vote: bank_labels must be a contiguous int32 [Nb]");
  TORCH_CHECK(labels.scalar_type() == torch::kInt32 && labels.dim() == 1 && labels.is_contiguous() &&
                  labels.size(0) == Nq && Nq < INT_MAX,
              "knn_vote: labels must be a contiguous int32 [Nq]");
  TORCH_CHECK(T > 0.0, "knn_vote: the temperature must be positive");
  TORCH_CHECK(sim.device() == idx.device() && bank_labels.device() == idx.device() && labels.device() == idx.device(),
              "knn_vote: all tensors must be on one device");
  TORCH_CHECK(idx.is_cuda(), "knn_vote: idx must be a GPU tensor");
  auto pred = torch::empty({Nq, 5}, idx.options());
  auto hit1 = torch::empty({Nq}, idx.options().dtype(torch::kBool));
  auto hit5 = torch::empty({Nq}, idx.options().dtype(torch::kBool));
  check_rc(jm_knn_vote(idx.data_ptr<int>(), sim.data_ptr<float>(), bank_labels.data_ptr<int>(), labels.data_ptr<int>(),
                       T, (int)Nq, (int)bank_labels.size(0), (int)k, pred.data_ptr<int>(),
                       reinterpret_cast<uint8_t*>(hit1.data_ptr()), reinterpret_cast<uint8_t*>(hit5.data_ptr()),
                       stream()),
           "knn_vote");
  return {pred, hit1, hit5};
}

// attention monitor: fp64 [H, 6] = per head [sum entropy, sum max prob, sum CLS mass, max logit, bad rows, B S]
// of softmax(q k^T / sqrt(hd)); rows_out (fp32 [B, H, S, 4], optional) receives every row's four values
torch::Tensor attn_stats(torch::Tensor qkv, int64_t heads, int64_t n_cls, c10::optional<torch::Tensor> rows_out) {
  TORCH_CHECK(qkv.is_cuda(), "attn_stats: qkv must be a GPU tensor");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 && qkv.is_contiguous(), "attn_stats: qkv must be contiguous bf16");
  check_attn_shape(qkv, heads, "attn_stats");
  const int64_t B = qkv.size(0), S = qkv.size(1), hd = qkv.size(2) / 3 / heads;
  TORCH_CHECK(B >= 1 && S >= 1 && B < INT_MAX && S < INT_MAX && heads < INT_MAX, "attn_stats: empty or oversized qkv");
  TORCH_CHECK(n_cls >= 0 && n_cls <= S, "attn_stats: n_cls must be in 0..S (got ", n_cls, ", S = ", S, ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "attn_stats: qkv must be 16-byte aligned");
  float* rp = nullptr;
  if (rows_out.has_value() && rows_out->defined()) {
    const auto& r = *rows_out;
    TORCH_CHECK(r.is_cuda() && r.device() == qkv.device() && r.scalar_type() == torch::kFloat32 && r.is_contiguous() &&
                    r.dim() == 4 && r.size(0) == B && r.size(1) == heads && r.size(2) == S && r.size(3) == 4,
                "attn_stats: rows_out must be a contiguous fp32 [B, H, S, 4] tensor on qkv's GPU");
    rp = r.data_ptr<float>();
  }
  const auto f64 = qkv.options().dtype(torch::kFloat64);
  const long np = jm_attn_stats_part((int)B, (int)S, (int)heads);
#ifdef JM_DEBUG
  auto part = torch::zeros({np}, f64);  // a workgroup stopped by its guard adds nothing
#else
  auto part = torch::empty({np}, f64);
#endif
  auto out = torch::empty({heads, (long)JM_ATTN_STATS_COLS}, f64);
  check_rc(jm_attn_stats(qkv.data_ptr(), (int)B, (int)S, (int)heads, (int)hd, (int)n_cls, part.data_ptr<double>(), rp,
                         stream()),
           "attn_stats");
  check_rc(jm_attn_stats_finish(part.data_ptr<double>(), (int)B, (int)S, (int)heads, out.data_ptr<double>(), stream()),
           "attn_stats (finish)");
  return out;
}

// attention maps: one rollout step, r_out = alpha r_in + (1 - alpha) / H sum_h r_in softmax(q k^T / sqrt(hd))
// (r_in fp32 [B, C, S], C <= 8); the [S, S] probabilities are never stored
torch::Tensor attn_rollout_step(torch::Tensor qkv, int64_t heads, torch::Tensor r_in, double alpha,
                                c10::optional<torch::Tensor> out_opt) {
  TORCH_CHECK(qkv.is_cuda(), "attn_rollout_step: qkv must be a GPU tensor");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 && qkv.is_contiguous(),
              "attn_rollout_step: qkv must be contiguous bf16");
  check_attn_shape(qkv, heads, "attn_rollout_step");
  const int64_t B = qkv.size(0), S = qkv.size(1), hd = qkv.size(2) / 3 / heads;
  TORCH_CHECK(B >= 1 && S >= 1 && B < INT_MAX && S < INT_MAX && heads < INT_MAX,
              "attn_rollout_step: empty or oversized qkv");
  TORCH_CHECK(r_in.is_cuda() && r_in.device() == qkv.device() && r_in.scalar_type() == torch::kFloat32 &&
                  r_in.is_contiguous() && r_in.dim() == 3 && r_in.size(0) == B && r_in.size(2) == S,
              "attn_rollout_step: r_in must be a contiguous fp32 [B, C, S] tensor on qkv's GPU");
  const int64_t C = r_in.size(1);
  TORCH_CHECK(C >= 1 && C <= 8, "attn_rollout_step: C must be in 1..8 (got ", C, ")");
  TORCH_CHECK(alpha >= 0.0 && alpha <= 1.0, "attn_rollout_step: alpha must be in [0, 1] (got ", alpha, ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "attn_rollout_step: qkv must be 16-byte aligned");
  const long nw = jm_attn_rollout_ws((int)B, (int)S, (int)heads, (int)C);
#ifdef JM_DEBUG
  auto ws = torch::zeros({nw}, r_in.options());  // a workgroup stopped by its guard adds nothing
#else
  auto ws = torch::empty({nw}, r_in.options());
#endif
  torch::Tensor out;
  if (out_opt.has_value() && out_opt->defined()) {
    out = *out_opt;
    TORCH_CHECK(out.is_cuda() && out.device() == qkv.device() && out.scalar_type() == torch::kFloat32 &&
                    out.is_contiguous() && out.sizes() == r_in.sizes() && out.data_ptr() != r_in.data_ptr(),
                "attn_rollout_step: out must be a contiguous fp32 [B, C, S] tensor on qkv's GPU, distinct from r_in");
  } else {
    out = torch::empty_like(r_in);
  }
  check_rc(jm_attn_rollout_step(qkv.data_ptr(), (int)B, (int)S, (int)heads, (int)hd, r_in.data_ptr<float>(), (int)C,
                                alpha, out.data_ptr<float>(), ws.data_ptr<float>(), stream()),
           "attn_rollout_step");
  return out;
}

// ------------------------------------------------------------------------------ representation monitor
// G fp64 [D, D] += x^T x, s fp64 [D] += column sums, over the rows with valid != 0 (all without valid); in place
void feat_gram(torch::Tensor x, c10::optional<torch::Tensor> valid, torch::Tensor G, torch::Tensor s) {
  TORCH_CHECK(x.is_cuda(), "feat_gram: x must be a GPU tensor");
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && x.dim() == 2, "feat_gram: x must be fp32 [n, D]");
  const int64_t n = x.size(0), D = x.size(1);
  TORCH_CHECK(D >= 1 && D <= (1 << 20) && n < INT_MAX, "feat_gram: D must be in 1..2^20 and n below 2^31");
  TORCH_CHECK(x.stride(1) == 1 || D == 1, "feat_gram: x must have a unit column stride");
  TORCH_CHECK(n <= 1 || x.stride(0) >= D, "feat_gram: rows of x must not overlap");
  TORCH_CHECK(G.scalar_type() == torch::kFloat64 && G.dim() == 2 && G.size(0) == D && G.size(1) == D &&
                  G.is_contiguous() && G.device() == x.device(),
              "feat_gram: G must be a contiguous fp64 [D, D] tensor on x's GPU");
  TORCH_CHECK(s.scalar_type() == torch::kFloat64 && s.dim() == 1 && s.size(0) == D && s.is_contiguous() &&
                  s.device() == x.device(),
              "feat_gram: s must be a contiguous fp64 [D] tensor on x's GPU");
  const uint8_t* vp = nullptr;
  if (valid.has_value() && valid->defined()) {
    const auto& v = *valid;
    TORCH_CHECK((v.scalar_type() == torch::kUInt8 || v.scalar_type() == torch::kBool) && v.dim() == 1 &&
                    v.size(0) == n && v.is_contiguous() && v.device() == x.device(),
                "feat_gram: valid must be a contiguous uint8 or bool [n] tensor on x's GPU");
    vp = reinterpret_cast<const uint8_t*>(v.data_ptr());
  }
  if (n == 0) return;
  check_rc(jm_feat_gram(x.data_ptr<float>(), n > 1 ? x.stride(0) : D, vp, (int)n, (int)D, G.data_ptr<double>(),
                        s.data_ptr<double>(), stream()),
           "feat_gram");
}

// e fp64 [Nq] = per query the sum over valid bank rows j != self_idx of exp(-2 t (1 - q . bank_j))
torch::Tensor feat_uniformity(torch::Tensor q, torch::Tensor bank, c10::optional<torch::Tensor> self_idx,
                              c10::optional<torch::Tensor> bank_valid, double t, int64_t splits,
                              c10::optional<torch::Tensor> out) {
  const char* fn = "feat_uniformity";
  for (const auto* p : {&q, &bank}) {
    TORCH_CHECK(p->scalar_type() == torch::kBFloat16 && p->dim() == 2, fn, ": q and bank must be bf16 [N, D]");
    TORCH_CHECK(p->size(1) >= 1 && p->stride(1) == 1, fn, ": q and bank must have a unit column stride");
    TORCH_CHECK(p->size(0) <= 1 || p->stride(0) >= p->size(1), fn, ": rows must not overlap");
    TORCH_CHECK(p->size(0) < INT_MAX && p->size(1) < INT_MAX, fn, ": q or bank too large");
  }
  TORCH_CHECK(q.size(1) == bank.size(1), fn, ": q and bank must have the same D");
  TORCH_CHECK(q.size(1) % 32 == 0, fn, ": D must be a multiple of 32");
  TORCH_CHECK(t > 0.0, fn, ": t must be positive");
  TORCH_CHECK(splits >= 0 && splits <= 1024, fn, ": splits must be in 0..1024");
  TORCH_CHECK(bank.size(0) >= 1, fn, ": the bank is empty");
  TORCH_CHECK(bank.device() == q.device(), fn, ": q and bank must be on one device");
  TORCH_CHECK(q.is_cuda(), fn, ": q must be a GPU tensor");
  const int64_t Nq = q.size(0), Nb = bank.size(0);
  const int* sp = nullptr;
  if (self_idx.has_value() && self_idx->defined()) {
    TORCH_CHECK(self_idx->scalar_type() == torch::kInt32 && self_idx->dim() == 1 && self_idx->size(0) == Nq &&
                    self_idx->is_contiguous() && self_idx->device() == q.device(),
                fn, ": self_idx must be int32 [Nq] on the inputs' device");
    sp = self_idx->data_ptr<int>();
  }
  const uint8_t* vp = nullptr;
  if (bank_valid.has_value() && bank_valid->defined()) {
    const auto& v = *bank_valid;
    TORCH_CHECK((v.scalar_type() == torch::kUInt8 || v.scalar_type() == torch::kBool) && v.dim() == 1 &&
                    v.size(0) == Nb && v.is_contiguous() && v.device() == q.device(),
                fn, ": bank_valid must be a contiguous uint8 or bool [Nb] tensor on the inputs' device");
    vp = reinterpret_cast<const uint8_t*>(v.data_ptr());
  }
  const auto f64 = q.options().dtype(torch::kFloat64);
  torch::Tensor e;
  if (out.has_value() && out->defined()) {
    e = *out;
    TORCH_CHECK(e.scalar_type() == torch::kFloat64 && e.dim() == 1 && e.size(0) == Nq && e.is_contiguous() &&
                    e.device() == q.device(),
                fn, ": out must be a contiguous fp64 [Nq] tensor on the inputs' device");
  } else {
    e = torch::empty({Nq}, f64);
  }
  if (Nq == 0) return e;
  const int64_t nseg = jm_feat_uniformity_segments((int)Nb);
#ifdef JM_DEBUG
  auto part = torch::zeros({nseg, Nq}, f64);  // a workgroup stopped by its guard adds nothing
#else
  auto part = torch::empty({nseg, Nq}, f64);
#endif
  check_rc(jm_feat_uniformity(q.data_ptr(), row_stride(q), bank.data_ptr(), row_stride(bank), sp, vp, (int)Nq, (int)Nb,
                              (int)q.size(1), t, (int)splits, part.data_ptr<double>(), e.data_ptr<double>(), stream()),
           fn);
  return e;
}

// ------------------------------------------------------------------------------ rotary position embedding
// rotates q and k of the patch rows of qkv [B, S, 3 heads hd] in place (rope.hip); returns qkv
torch::Tensor rope_apply(torch::Tensor qkv, int64_t heads, int64_t n_cls, int64_t gw, torch::Tensor table,
                         c10::optional<torch::Tensor> pos, bool inverse) {
  const char* fn = "rope_apply";
  TORCH_CHECK(qkv.is_cuda(), fn, ": qkv must be a GPU tensor");
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous(), fn, ": qkv must be a contiguous [B, S, 3 heads hd] tensor");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 || qkv.scalar_type() == torch::kFloat32, fn,
              ": qkv must be bf16 or fp32");
  const int64_t B = qkv.size(0), S = qkv.size(1), W = qkv.size(2);
  TORCH_CHECK(heads >= 1 && W % (3 * heads) == 0, fn, ": the last dim must be 3 heads hd");
  const int64_t hd = W / (3 * heads);
  TORCH_CHECK(hd % 16 == 0, fn, ": hd must be a multiple of 16");
  TORCH_CHECK(n_cls >= 0 && n_cls <= S && gw >= 1, fn, ": n_cls must be in 0..S and gw positive");
  TORCH_CHECK(B * S < INT_MAX && W < INT_MAX, fn, ": qkv too large");
  TORCH_CHECK(table.scalar_type() == torch::kFloat32 && table.dim() == 3 && table.size(0) >= 1 &&
                  table.size(1) == hd / 4 && table.size(2) == 2 && table.is_contiguous() &&
                  table.device() == qkv.device(),
              fn, ": table must be a contiguous fp32 [G, hd / 4, 2] tensor on qkv's device");
  const int64_t G = table.size(0), Sp = S - n_cls;
  TORCH_CHECK(G * gw < INT_MAX, fn, ": table too large");
  const int* pp = nullptr;
  long pb = 0;
  if (pos.has_value() && pos->defined()) {
    const auto& p = *pos;
    TORCH_CHECK(p.scalar_type() == torch::kInt32 && p.is_contiguous() && p.device() == qkv.device() &&
                    ((p.dim() == 1 && p.size(0) == Sp) || (p.dim() == 2 && p.size(0) == B && p.size(1) == Sp)),
                fn, ": pos must be a contiguous int32 [S - n_cls] or [B, S - n_cls] tensor on qkv's device");
    pp = p.data_ptr<int>();
    pb = p.dim() == 2 ? (long)Sp : 0;
  } else {
    TORCH_CHECK(Sp <= G * gw, fn, ": the table covers fewer positions than the sequence has patch rows");
  }
  if (B == 0 || Sp == 0) return qkv;
  check_rc(jm_rope_apply(qkv.data_ptr(), qkv.scalar_type() == torch::kBFloat16, (int)B, (int)S, (int)heads, (int)hd,
                         (int)n_cls, (int)gw, table.data_ptr<float>(), (int)G, pp, pb, inverse ? 1 : 0, stream()),
           fn);
  return qkv;
}

// ------------------------------------------------------------------------------ QK-norm
// the rope arguments of qknorm_fwd / qknorm_bwd, checked as rope_apply checks them; table absent = no rotation
struct QknRope {
  const float* table = nullptr;
  int G = 0;
  const int* pos = nullptr;
  long posB = 0;
};

QknRope qkn_rope(const char* fn, const torch::Tensor& qkv, int64_t hd, int64_t n_cls, int64_t gw,
                 const c10::optional<torch::Tensor>& table, const c10::optional<torch::Tensor>& pos) {
  QknRope r;
  if (!(table.has_value() && table->defined())) {
    TORCH_CHECK(!(pos.has_value() && pos->defined()), fn, ": pos without a table");
    return r;
  }
  const auto& t = *table;
  const int64_t B = qkv.size(0), S = qkv.size(1);
  TORCH_CHECK(n_cls >= 0 && n_cls <= S && gw >= 1, fn, ": n_cls must be in 0..S and gw positive");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.dim() == 3 && t.size(0) >= 1 && t.size(1) == hd / 4 &&
                  t.size(2) == 2 && t.is_contiguous() && t.device() == qkv.device(),
              fn, ": table must be a contiguous fp32 [G, hd / 4, 2] tensor on qkv's device");
  const int64_t G = t.size(0), Sp = S - n_cls;
  TORCH_CHECK(G * gw < INT_MAX, fn, ": table too large");
  if (pos.has_value() && pos->defined()) {
    const auto& p = *pos;
    TORCH_CHECK(p.scalar_type() == torch::kInt32 && p.is_contiguous() && p.device() == qkv.device() &&
                    ((p.dim() == 1 && p.size(0) == Sp) || (p.dim() == 2 && p.size(0) == B && p.size(1) == Sp)),
                fn, ": pos must be a contiguous int32 [S - n_cls] or [B, S - n_cls] tensor on qkv's device");
    r.pos = p.data_ptr<int>();
    r.posB = p.dim() == 2 ? (long)Sp : 0;
  } else {
    TORCH_CHECK(Sp <= G * gw, fn, ": the table covers fewer positions than the sequence has patch rows");
  }
  r.table = t.data_ptr<float>();
  r.G = (int)G;
  return r;
}

int64_t qkn_check(const char* fn, const torch::Tensor& qkv, int64_t heads, const torch::Tensor& g_q,
                  const torch::Tensor& g_k) {
  TORCH_CHECK(qkv.is_cuda(), fn, ": qkv must be a GPU tensor");
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous(), fn, ": qkv must be a contiguous [B, S, 3 heads hd] tensor");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 || qkv.scalar_type() == torch::kFloat32, fn,
              ": qkv must be bf16 or fp32");
  const int64_t B = qkv.size(0), S = qkv.size(1), W = qkv.size(2);
  TORCH_CHECK(heads >= 1 && W % (3 * heads) == 0, fn, ": the last dim must be 3 heads hd");
  const int64_t hd = W / (3 * heads);
  TORCH_CHECK(B * S < INT_MAX && W < INT_MAX, fn, ": qkv too large");
  TORCH_CHECK(B == 0 || S == 0 || jm_qknorm_bwd_blocks((int)B, (int)S, (int)heads, (int)hd) > 0, fn,
              ": hd must be one of 32, 64, 80, 96, 128");
  for (const auto* g : {&g_q, &g_k})
    TORCH_CHECK(g->scalar_type() == torch::kFloat32 && g->dim() == 1 && g->size(0) == hd && g->is_contiguous() &&
                    g->device() == qkv.device() && reinterpret_cast<uintptr_t>(g->data_ptr()) % 16 == 0,
                fn, ": g_q and g_k must be contiguous 16-byte aligned fp32 [hd] tensors on qkv's device");
  return hd;
}

// normalises (and, with a table, rotates) q and k of qkv in place; returns saved [B, S, 2 heads hd], their input bits
torch::Tensor qknorm_fwd(torch::Tensor qkv, int64_t heads, torch::Tensor g_q, torch::Tensor g_k, int64_t n_cls,
                         int64_t gw, c10::optional<torch::Tensor> table, c10::optional<torch::Tensor> pos) {
  const char* fn = "qknorm_fwd";
  const int64_t hd = qkn_check(fn, qkv, heads, g_q, g_k);
  const QknRope r = qkn_rope(fn, qkv, hd, n_cls, gw, table, pos);
  const int64_t B = qkv.size(0), S = qkv.size(1);
  auto saved = torch::empty({B, S, 2 * heads * hd}, qkv.options());
  if (B == 0 || S == 0) return saved;
  check_rc(jm_qknorm_fwd(qkv.data_ptr(), saved.data_ptr(), qkv.scalar_type() == torch::kBFloat16, (int)B, (int)S,
                         (int)heads, (int)hd, g_q.data_ptr<float>(), g_k.data_ptr<float>(), (int)n_cls, (int)gw,
                         r.table, r.G, r.pos, r.posB, stream()),
           fn);
  return saved;
}

// dx over the q and k thirds of dqkv in place; returns dg fp32 [2, hd] = (dg_q, dg_k)
torch::Tensor qknorm_bwd(torch::Tensor dqkv, torch::Tensor saved, int64_t heads, torch::Tensor g_q, torch::Tensor g_k,
                         int64_t n_cls, int64_t gw, c10::optional<torch::Tensor> table,
                         c10::optional<torch::Tensor> pos) {
  const char* fn = "qknorm_bwd";
  const int64_t hd = qkn_check(fn, dqkv, heads, g_q, g_k);
  const QknRope r = qkn_rope(fn, dqkv, hd, n_cls, gw, table, pos);
  const int64_t B = dqkv.size(0), S = dqkv.size(1);
  TORCH_CHECK(saved.scalar_type() == dqkv.scalar_type() && saved.is_contiguous() && saved.device() == dqkv.device() &&
                  saved.numel() == B * S * 2 * heads * hd,
              fn, ": saved must be a contiguous [B, S, 2 heads hd] tensor of dqkv's dtype and device");
  auto fopt = dqkv.options().dtype(torch::kFloat32);
  if (B == 0 || S == 0) return torch::zeros({2, hd}, fopt);
  const int nb = jm_qknorm_bwd_blocks((int)B, (int)S, (int)heads, (int)hd);
  auto part = torch::empty({nb, 2, hd}, fopt.dtype(torch::kFloat64));
  auto dg = torch::empty({2, hd}, fopt);
  check_rc(jm_qknorm_bwd(dqkv.data_ptr(), saved.data_ptr(), dqkv.scalar_type() == torch::kBFloat16, (int)B, (int)S,
                         (int)heads, (int)hd, g_q.data_ptr<float>(), g_k.data_ptr<float>(), (int)n_cls, (int)gw,
                         r.table, r.G, r.pos, r.posB, part.data_ptr<double>(), dg.data_ptr<float>(), stream()),
           fn);
  return dg;
}

// ------------------------------------------------------------------------------ SwiGLU gate (csrc/swiglu.hip)
// Both return (status, result): a negative status (jm_api.h) is a shape the kernels do not take -- the result is then
// an empty tensor and the caller (ops/prims.py) takes the torch composition.  rate <= 0: no dropout, seed ignored.
struct SwDrop {
  const int64_t* seed = nullptr;
  uint32_t thr = 0;
  float scale = 1.f;
};

static SwDrop sw_drop(const char* fn, const torch::Tensor& pre, const c10::optional<torch::Tensor>& seed, double rate) {
  SwDrop d;
  if (rate <= 0.0) return d;
  TORCH_CHECK(seed.has_value() && seed->defined(), fn, ": a dropout rate needs a seed");
  check_seed(*seed, pre);
  const auto kp = keep_params(rate);
  d.seed = seed->data_ptr<int64_t>();
  d.thr = kp.first;
  d.scale = kp.second;
  return d;
}

static void sw_check(const char* fn, const torch::Tensor& pre) {
  CHECK_CUDA(pre);
  TORCH_CHECK(pre.scalar_type() == torch::kBFloat16 && pre.dim() == 2 && pre.is_contiguous() && pre.size(1) % 2 == 0,
              fn, ": pre must be a contiguous bf16 [M, 2 Hs] tensor");
  TORCH_CHECK(pre.size(0) < INT_MAX && pre.size(1) < INT_MAX, fn, ": pre too large");
}

std::tuple<int64_t, torch::Tensor> swiglu_fwd(torch::Tensor pre, c10::optional<torch::Tensor> seed, double rate) {
  const char* fn = "swiglu_fwd";
  sw_check(fn, pre);
  const SwDrop d = sw_drop(fn, pre, seed, rate);
  const int64_t M = pre.size(0), Hs = pre.size(1) / 2;
  if (M == 0) return {-1, torch::empty({0}, pre.options())};
  auto a = torch::empty({M, Hs}, pre.options());
  const int rc = jm_swiglu_fwd(bf(pre), bfm(a), (int)M, (int)Hs, d.seed, d.thr, d.scale, stream());
  if (rc < 0) return {rc, torch::empty({0}, pre.options())};
  return {0, a};
}

std::tuple<int64_t, torch::Tensor> swiglu_bwd(torch::Tensor pre, torch::Tensor da, c10::optional<torch::Tensor> bias_grad,
                                              c10::optional<torch::Tensor> seed, double rate) {
  const char* fn = "swiglu_bwd";
  sw_check(fn, pre);
  const SwDrop d = sw_drop(fn, pre, seed, rate);
  const int64_t M = pre.size(0), Hs = pre.size(1) / 2;
  TORCH_CHECK(da.scalar_type() == torch::kBFloat16 && da.is_contiguous() && da.device() == pre.device() &&
                  da.dim() == 2 && da.size(0) == M && da.size(1) == Hs,
              fn, ": da must be a contiguous bf16 [M, Hs] tensor on pre's device");
  float* bg = nullptr;
  if (bias_grad.has_value() && bias_grad->defined()) {
    TORCH_CHECK(bias_grad->scalar_type() == torch::kFloat32 && bias_grad->is_contiguous() &&
                    bias_grad->numel() == 2 * Hs && bias_grad->device() == pre.device(),
                fn, ": bias_grad must be a contiguous fp32 [2 Hs] tensor on pre's device");
    bg = bias_grad->data_ptr<float>();
  }
  if (M == 0) return {-1, torch::empty({0}, pre.options())};
  auto dpre = torch::empty_like(pre);
  torch::Tensor ws;
  if (bg) ws = torch::empty({jm_swiglu_ws_floats((int)M, (int)Hs)}, pre.options().dtype(torch::kFloat32));
  const int rc = jm_swiglu_bwd(bf(pre), bf(da), bfm(dpre), bg, (int)M, (int)Hs, d.seed, d.thr, d.scale, stream(),
                               bg ? ws.data_ptr<float>() : nullptr);
  if (rc < 0) return {rc, torch::empty({0}, pre.options())};
  return {0, dpre};
}

py::dict debug_lines() {
  py::dict d;
  const std::pair<const char*, int (*)()> tus[] = {
      {"attention", jm_debug_line_attention}, {"dropout", jm_debug_line_dropout},
      {"batchnorm", jm_debug_line_batchnorm},
      {"augment", jm_debug_line_augment},     {"augment_chain", jm_debug_line_augment_chain},
      {"elementwise", jm_debug_line_elementwise},
      {"gemm", jm_debug_line_gemm},           {"gemm_tn", jm_debug_line_gemm_tn},
      {"layernorm", jm_debug_line_layernorm}, {"loss", jm_debug_line_loss},
      {"mae", jm_debug_line_mae},             {"optim", jm_debug_line_optim},
      {"recon", jm_debug_line_recon},         {"knn", jm_debug_line_knn},
      {"attn_stats", jm_debug_line_attn_stats}, {"attn_rollout", jm_debug_line_attn_rollout},
      {"distill", jm_debug_line_distill},     {"eval_report", jm_debug_line_eval_report},
      {"feat_stats", jm_debug_line_feat_stats}, {"rope", jm_debug_line_rope},
      {"qknorm", jm_debug_line_qknorm},       {"swiglu", jm_debug_line_swiglu}};
  for (const auto& t : tus) {
    const int line = t.second();
    if (line) d[t.first] = line;
  }
  return d;
}

void debug_selftest(int v) { jm_debug_selftest(v, stream()); }

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "jumbo_mae_tpu_amd CDNA4 (gfx950) HIP kernels";
  m.def("layernorm_fwd", &layernorm_fwd, py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("eps"),
        py::arg("out_dtype"), py::arg("also_bf16") = false);
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("x"), py::arg("mean"), py::arg("rstd"),
        py::arg("gamma"), py::arg("dgamma"), py::arg("dbeta"), py::arg("accum"), py::arg("dres") = py::none(),
        py::arg("out") = py::none(), py::arg("res_y") = py::none(), py::arg("res_scale") = py::none(),
        py::arg("res_mask") = py::none(), py::arg("res_dscale") = py::none(), py::arg("res_dbias") = py::none(),
        py::arg("res_T0") = 0, py::arg("res_out") = py::none(), py::arg("res_seed") = py::none(),
        py::arg("res_rate") = 0.0, py::arg("res_ioff") = 0, py::arg("hx") = py::none(), py::arg("beta") = py::none());
  m.def("gelu_fwd", &gelu_fwd);
  m.def("dropout_apply", &dropout_apply);
  m.def("dropout_apply_", &dropout_apply_);
  m.def("rrc_resize", &rrc_resize, py::arg("src"), py::arg("tab"), py::arg("size"), py::arg("tmp_bytes"),
        py::arg("tmp_rows_max"));
  m.def("rrc_kmax", &jm_rrc_kmax);
  m.def("window_resize", &window_resize, py::arg("src"), py::arg("tab"), py::arg("size"), py::arg("tmp_bytes"),
        py::arg("tmp_rows_max"));
  m.def("window_tab", &jm_window_tab);
  m.def("aug_chain", &aug_chain, py::arg("images"), py::arg("chain"), py::arg("scratch"));
  m.def("augmix_mix", &augmix_mix, py::arg("orig"), py::arg("chains"), py::arg("table"), py::arg("blended"));
  m.def("erase_paste", &erase_paste, py::arg("images"), py::arg("table"), py::arg("fill"),
        py::arg("box_bytes_max") = 0);
  m.def("gelu_drop", &gelu_drop, py::arg("a"), py::arg("b") = py::none(), py::arg("seed"), py::arg("rate"));
  m.def("softmax_dropout_fwd", &softmax_dropout_fwd);
  m.def("softmax_dropout_bwd", &softmax_dropout_bwd);
  m.def("gelu_bwd", &gelu_bwd, py::arg("h"), py::arg("da"), py::arg("bias_grad") = py::none(),
        py::arg("deriv") = false);
  m.def("colsum", &colsum);
  m.def("splitk_reduce_add", &splitk_reduce_add);
  m.def("residual_ln_fwd", &residual_ln_fwd, py::arg("x"), py::arg("y"), py::arg("scale"), py::arg("mask"),
        py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("T0"), py::arg("R0") = 0,
        py::arg("out") = py::none(), py::arg("seed") = py::none(), py::arg("rate") = 0.0);
  m.def("transpose_bf16", &transpose_bf16);
  m.def("residual_fwd", &residual_fwd, py::arg("x"), py::arg("y"), py::arg("scale"), py::arg("mask"),
        py::arg("out") = py::none(), py::arg("seed") = py::none(), py::arg("rate") = 0.0, py::arg("ioff") = 0);
  m.def("residual_bwd", &residual_bwd, py::arg("dout"), py::arg("y"), py::arg("scale"), py::arg("mask"),
        py::arg("dscale"), py::arg("ydtype"), py::arg("dbias") = py::none(), py::arg("out") = py::none(),
        py::arg("seed") = py::none(), py::arg("rate") = 0.0, py::arg("ioff") = 0);
  m.def("attn_fwd", &attn_fwd, py::arg("qkv"), py::arg("heads"), py::arg("seed") = py::none(), py::arg("rate") = 0.0);
  m.def("attn_bwd", &attn_bwd, py::arg("dO"), py::arg("qkv"), py::arg("o"), py::arg("lse"), py::arg("heads"),
        py::arg("dbias") = py::none(), py::arg("seed") = py::none(), py::arg("rate") = 0.0);
  m.def("attn_max_seq", &jm_attn_max_seq);
  m.def("attn_head_dims", &attn_head_dims);
  m.def("attn_fused_bias", &attn_fused_bias, py::arg("S"), py::arg("hd"));
  m.def("attn_dropout", &attn_dropout, py::arg("S"), py::arg("hd"));
  m.def("gemm_tn_wgrad", &gemm_tn_wgrad, py::arg("dy"), py::arg("x"), py::arg("g"), py::arg("store") = false);
  m.def("gemm_tn_wgrad_seg", &gemm_tn_wgrad_seg, py::arg("dys"), py::arg("xs"), py::arg("g"), py::arg("store") = false);
  m.def("zero_ranges", &zero_ranges, "zero float ranges of a flat buffer (one launch)");
  m.def("colsum_add_f32", &colsum_add_f32, "g += x.sum(0) for a row-strided fp32 [rows, n] view");
  m.def("gemm_tn_wgrad_seg_group", &gemm_tn_wgrad_seg_group, py::arg("dys"), py::arg("xs"), py::arg("gs"),
        py::arg("stores") = std::vector<bool>{}, "grouped segmented weight gradients (<= 2 problems)");
  m.def("gemm_tn_wgrad_group", &gemm_tn_wgrad_group, py::arg("dys"), py::arg("xs"), py::arg("gs"),
        py::arg("stores") = std::vector<bool>{}, "grouped weight gradients over one M (<= 4 problems)");
  m.def("gemm_test_force", &jm_gemm_test_force, py::arg("path"), py::arg("rows") = 0,
        "numerics tests only: NT GEMM kernel path 0 = by shape, 1 = 64-deep main loop everywhere, "
        "2 = 4-phase kernels at every M without tail split (rows = forced tile height)");
  m.def("gemm_nt_plan", &gemm_nt_plan_dict, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("epi") = 0,
        py::arg("lda") = 0, py::arg("splits") = 1,
        "the launch plan of an NT GEMM (csrc/gemm_plan.h GemmPlan) as a dict; read-only");
  m.def(
      "gemm_nt_tiles", [](int M, int N, int K, int epi, long lda) { return jm_gemm_nt_plan(M, N, K, epi, lda, 1).tiles; },
      py::arg("M"), py::arg("N"), py::arg("K") = 1024, py::arg("epi") = 0, py::arg("lda") = 0,
      "output tiles (workgroups before split-K) of an NT launch");
  m.def(
      "gemm_nt_tail_plan",
      [](int M, int N, int K, int epi, long lda) {
        const GemmPlan p = jm_gemm_nt_plan(M, N, K, epi, lda, 1);
        return std::make_pair(p.tail_S, p.tail_r);
      },
      py::arg("M"), py::arg("N"), py::arg("K"), py::arg("epi") = 0, py::arg("lda") = 0,
      "(S, tail tiles) of the tail split of an NT launch (S = 0: none); read-only");
  m.def("transpose_bf16_batch", &transpose_bf16_batch);
  m.def("gemm_nt_splitk", &gemm_nt_splitk, py::arg("A"), py::arg("B"), py::arg("bias") = py::none(),
        py::arg("splits") = 8, py::arg("add") = py::none());
  m.def("gemm_nt_dgelu", &gemm_nt_dgelu, py::arg("A"), py::arg("B"), py::arg("pre"), py::arg("dbias") = py::none(),
        py::arg("deriv") = false, py::arg("rate") = 0.0);
  m.def("gemm_nt_f32", &gemm_nt_f32, py::arg("A"), py::arg("B"));
  m.def("gemm_nt", &gemm_nt, py::arg("A"), py::arg("B"), py::arg("bias") = py::none(), py::arg("gelu") = false,
        py::arg("gelu_only") = false, py::arg("gelu_deriv") = false, py::arg("seed") = py::none(),
        py::arg("rate") = 0.0);
  m.def("opt_sumsq", &opt_sumsq);
  m.def("opt_adamw", &opt_adamw);
  m.def("opt_lamb_phase1", &opt_lamb_phase1);
  m.def("opt_lars_norms", &opt_lars_norms);
  m.def("opt_apply_trust", &opt_apply_trust);
  m.def("opt_sgd", &opt_sgd);
  m.def("opt_ema", &opt_ema, py::arg("master"), py::arg("ema"), py::arg("rows"), py::arg("meta"),
        py::arg("ema_hyper"));
  m.def("ema_swap", &ema_swap, py::arg("master"), py::arg("ema"), py::arg("shadow"), py::arg("rows"));
  m.def("opt_seg_stats", &opt_seg_stats, py::arg("master"), py::arg("grad"), py::arg("p_old"), py::arg("rows"),
        py::arg("meta"), py::arg("out") = py::none());
  m.def("patchify_normalize", &patchify_normalize);
  m.def("gather_patches", &gather_patches);
  m.def("embed_finish", &embed_finish);
  m.def("zero_f32", &zero_f32, "fp32 zero fill kernel (the store-mode gradients' pre-reduce fill)");
  m.def("mask_ids", &mask_ids, "random-masking permutation ids + mask from noise (one workgroup per row)");
  m.def("unshuffle_fwd", &unshuffle_fwd);
  m.def("unshuffle_bwd", &unshuffle_bwd);
  m.def("patch_mse_fwd", &patch_mse_fwd);
  m.def("mix_patches", &mix_patches);
  m.def("patch_mse_bwd", &patch_mse_bwd);
  m.def("recon", &recon, py::arg("pred"), py::arg("images"), py::arg("mask"), py::arg("p"), py::arg("norm_pix"),
        py::arg("fill") = 127, py::arg("out") = py::none(),
        "MAE reconstruction panels -> (recon, paste, masked uint8 [B, 3, H, W], err fp32 [B, N])");
  m.def("cls_loss_fwd", &cls_loss_fwd, py::arg("logits"), py::arg("labels"), py::arg("perm") = py::none(),
        py::arg("w") = py::none(), py::arg("smoothing") = 0.0, py::arg("mode") = 0);
  m.def("cls_loss_bwd", &cls_loss_bwd, py::arg("dloss"), py::arg("logits"), py::arg("labels"),
        py::arg("perm"), py::arg("w"), py::arg("smoothing"), py::arg("mode"), py::arg("lse"));
  m.def("kd_loss_fwd", &kd_loss_fwd, py::arg("z"), py::arg("u"), py::arg("temperature") = 1.0, py::arg("mode") = 0,
        "distillation loss -> (kd fp32 [B], agree bool [B], lse fp32 [B, 4], t int32 [B])");
  m.def("kd_loss_bwd", &kd_loss_bwd, py::arg("dloss"), py::arg("z"), py::arg("u"), py::arg("temperature"),
        py::arg("mode"), py::arg("lse"), py::arg("t") = py::none());
  m.def("eval_rows", &eval_rows, py::arg("logits"), py::arg("labels"), py::arg("mode") = 0,
        "evaluation report, per row -> (pred int32 [B], rank int32 [B], conf fp32 [B])");
  m.def("eval_state_words", &eval_state_words, py::arg("L"), py::arg("n_bins"));
  m.def("eval_accumulate", &eval_accumulate, py::arg("labels"), py::arg("pred"), py::arg("rank"), py::arg("conf"),
        py::arg("L"), py::arg("n_bins"), py::arg("state"), "evaluation report: int64 state += the batch");
  m.def("knn_topk", &knn_topk, py::arg("q"), py::arg("bank"), py::arg("k"), py::arg("self_idx") = py::none(),
        py::arg("splits") = 0, py::arg("out_idx") = py::none(), py::arg("out_sim") = py::none(),
        "fused similarity + top-k -> (idx int32, sim fp32) [Nq, k], ties by ascending bank index");
  m.def("knn_splits", &jm_knn_splits, py::arg("Nq"), py::arg("Nb"), py::arg("splits") = 0,
        "bank slices of a knn_topk launch");
  m.def("knn_vote", &knn_vote, py::arg("idx"), py::arg("sim"), py::arg("bank_labels"), py::arg("labels"), py::arg("T"),
        "weighted k-NN vote -> (pred int32 [Nq, 5], hit1, hit5 bool [Nq])");
  m.def("bn_stats", &bn_stats, py::arg("x"));
  m.def("bn_apply", &bn_apply, py::arg("x"), py::arg("packed"), py::arg("gamma"), py::arg("beta"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("eps"), py::arg("momentum"), py::arg("out_dtype"),
        py::arg("out") = py::none());
  m.def("bn_apply_eval", &bn_apply_eval, py::arg("x"), py::arg("running_mean"), py::arg("running_var"),
        py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("out_dtype"), py::arg("out") = py::none());
  m.def("bn_bwd_reduce", &bn_bwd_reduce, py::arg("dy"), py::arg("x"), py::arg("stats"), py::arg("gamma"),
        py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none());
  m.def("bn_bwd_dx", &bn_bwd_dx, py::arg("dy"), py::arg("x"), py::arg("stats"), py::arg("gamma"), py::arg("packed_g"),
        py::arg("n"), py::arg("out") = py::none());
  m.def("bn_chunk_rows", &jm_bn_chunk_rows, "rows per workgroup of the BatchNorm kernels");
  m.def("bn_block_cols", &jm_bn_block_cols, "columns per workgroup of the BatchNorm kernels");
  m.def("attn_stats", &attn_stats, py::arg("qkv"), py::arg("heads"), py::arg("n_cls"),
        py::arg("rows_out") = py::none(), "per-head attention statistics, fp64 [H, 6]");
  m.def("attn_rollout_step", &attn_rollout_step, py::arg("qkv"), py::arg("heads"), py::arg("r_in"), py::arg("alpha"),
        py::arg("out") = py::none(), "one attention-rollout step on fp32 rows [B, C, S] (C <= 8) -> fp32 [B, C, S]");
  m.def("feat_gram", &feat_gram, py::arg("x"), py::arg("valid"), py::arg("G"), py::arg("s"),
        "representation monitor: fp64 G [D, D] += x^T x, s [D] += column sums over the valid rows, in place");
  m.def("feat_uniformity", &feat_uniformity, py::arg("q"), py::arg("bank"), py::arg("self_idx") = py::none(),
        py::arg("bank_valid") = py::none(), py::arg("t") = 2.0, py::arg("splits") = 0, py::arg("out") = py::none(),
        "representation monitor: fp64 [Nq] sums of exp(-2 t (1 - q . bank_j)) over the valid bank rows");
  m.def("feat_uniformity_segments", &jm_feat_uniformity_segments, py::arg("Nb"),
        "bank segments (rows of the workspace) of a feat_uniformity launch");
  m.def("rope_apply", &rope_apply, py::arg("qkv"), py::arg("heads"), py::arg("n_cls"), py::arg("gw"), py::arg("table"),
        py::arg("pos") = py::none(), py::arg("inverse") = false,
        "axial 2-D rotary embedding of q and k of the patch rows of qkv [B, S, 3 heads hd], in place");
  m.def("qknorm_fwd", &qknorm_fwd, py::arg("qkv"), py::arg("heads"), py::arg("g_q"), py::arg("g_k"),
        py::arg("n_cls") = 0, py::arg("gw") = 1, py::arg("table") = py::none(), py::arg("pos") = py::none(),
        "QK-norm: RMSNorm of q and k per head (then the rotary embedding, with a table) of qkv in place; returns the "
        "saved pre-norm q|k");
  m.def("qknorm_bwd", &qknorm_bwd, py::arg("dqkv"), py::arg("saved"), py::arg("heads"), py::arg("g_q"), py::arg("g_k"),
        py::arg("n_cls") = 0, py::arg("gw") = 1, py::arg("table") = py::none(), py::arg("pos") = py::none(),
        "QK-norm backward: dx over the q and k thirds of dqkv in place; returns fp32 [2, hd] = (dg_q, dg_k)");
  m.def("qknorm_bwd_blocks", &jm_qknorm_bwd_blocks, py::arg("B"), py::arg("S"), py::arg("heads"), py::arg("hd"),
        "workgroups (rows of the partial workspace) of a qknorm_bwd launch");
  m.def("swiglu_fwd", &swiglu_fwd, py::arg("pre"), py::arg("seed") = py::none(), py::arg("rate") = 0.0,
        "SwiGLU gate: (status, a [M, Hs]) of pre [M, 2 Hs] = [gate | up]; a negative status: shape not taken");
  m.def("swiglu_bwd", &swiglu_bwd, py::arg("pre"), py::arg("da"), py::arg("bias_grad") = py::none(),
        py::arg("seed") = py::none(), py::arg("rate") = 0.0,
        "SwiGLU gate backward: (status, dpre [M, 2 Hs]); bias_grad fp32 [2 Hs] += colsum(dpre)");
  m.def("swiglu_ws_floats", &jm_swiglu_ws_floats, py::arg("M"), py::arg("Hs"),
        "floats of a swiglu_bwd launch's partial-row workspace (0: shape not taken)");
  m.def("debug_lines", &debug_lines);
  m.def("debug_selftest", &debug_selftest);
#ifdef JM_DEBUG
  m.attr("debug_build") = true;
#else
  m.attr("debug_build") = false;
#endif
}
