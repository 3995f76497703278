// Torch bindings for the mine_amd HIP kernels (gfx950 only).
//
// Tensor-level contracts are documented in mine_amd/ops/renderer.py and
// mine_amd/ops/ssim.py; the launchers and their pointer contracts are
// declared in launchers.h. Everything here is thin glue: every tensor is
// checked before its pointer is handed on, outputs are allocated, and the
// launch status is read after every launcher call. Sections follow the
// kernel files in build order.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <string>
#include <vector>

#include "launchers.h"

namespace {

hipStream_t stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// --------------------------------------------------------------------------
// helpers

// accepted dtypes of one argument: a set over the element codes plus the
// two index types
constexpr unsigned kF32 = 1u << kElemF32;
constexpr unsigned kBF16 = 1u << kElemBF16;
constexpr unsigned kF16 = 1u << kElemF16;
constexpr unsigned k16 = kBF16 | kF16;    // the MFMA / stream kernels' pair
constexpr unsigned kFloat = kF32 | k16;
constexpr unsigned kI32 = 1u << 3;
constexpr unsigned kI64 = 1u << 4;

unsigned dtype_bit(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return kF32;
    case at::kBFloat16: return kBF16;
    case at::kHalf: return kF16;
    case at::kInt: return kI32;
    case at::kLong: return kI64;
    default: return 0;
  }
}

std::string dtype_names(unsigned accept) {
  static const char* const names[] = {"f32", "bf16", "fp16", "int32", "int64"};
  std::string s;
  for (int i = 0; i < 5; ++i)
    if (accept & (1u << i)) s += (s.empty() ? "" : " or ") + std::string(names[i]);
  return s;
}

// element code of a launcher's `elem` argument
int elem_of(at::ScalarType t, const char* who) {
  switch (t) {
    case at::kFloat: return kElemF32;
    case at::kBFloat16: return kElemBF16;
    case at::kHalf: return kElemF16;
    default:
      TORCH_CHECK(false, who, ": dtype must be f32, bf16 or fp16, got ", t);
  }
}

// The one argument check, in this order: on the GPU and on the device of
// the binding's first tensor, contiguous, dtype in `accept`, and `numel`
// elements as the geometry implies (numel < 0: the size is the geometry).
void check_arg(const char* who, const char* name, const at::Tensor& t,
               const at::Tensor& first, unsigned accept, int64_t numel) {
  TORCH_CHECK(t.is_cuda(), who, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.device() == first.device(), who, ": ", name,
              " must be on the device of the first tensor");
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " must be contiguous");
  TORCH_CHECK(dtype_bit(t.scalar_type()) & accept, who, ": ", name,
              " must be ", dtype_names(accept), ", got ", t.scalar_type());
  TORCH_CHECK(numel < 0 || t.numel() == numel, who, ": ", name, " must have ",
              numel, " elements, got ", t.numel());
}

// The absent-tensor convention: numel() == 0 stands for "not given" and
// becomes a null pointer; anything else gets the full check.
template <typename T>
T* opt_arg(const char* who, const char* name, const at::Tensor& t,
           const at::Tensor& first, unsigned accept, int64_t numel) {
  if (t.numel() == 0) return nullptr;
  check_arg(who, name, t, first, accept, numel);
  return static_cast<T*>(t.data_ptr());
}

// sizes that the launchers take as int
void check_ints(const char* who, std::initializer_list<int64_t> positive) {
  for (const int64_t v : positive)
    TORCH_CHECK(v > 0 && v <= INT_MAX, who, ": size ", v, " out of range");
}

// After every launcher call: the dispatch code of the launchers that take
// an element code, then the launch status.
void launched(const char* who, int rc = kLaunched) {
  TORCH_CHECK(rc == kLaunched, who, ": no kernel for this dtype and shape");
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Output of a reduction. Default mode: `out` is zero-filled and the kernel
// adds into it atomically. Deterministic mode: `out` is unfilled, the kernel
// stores per-block partials into the unfilled `ws` and a finishing launch
// sums them in index order.
struct Reduction {
  at::Tensor out, ws;
  float* out_ptr() const { return out.data_ptr<float>(); }
  float* ws_ptr() const { return ws.defined() ? ws.data_ptr<float>() : nullptr; }
  // where the reduction kernel writes
  float* target() const { return ws.defined() ? ws_ptr() : out_ptr(); }
};

Reduction reduction_out(bool det, at::IntArrayRef out_shape,
                        at::IntArrayRef ws_shape, const at::Tensor& like) {
  const auto fopt = like.options().dtype(at::kFloat);
  if (det) return {at::empty(out_shape, fopt), at::empty(ws_shape, fopt)};
  return {at::zeros(out_shape, fopt), at::Tensor()};
}

// pack output dtype from the optional Python-side argument (default bf16)
at::ScalarType pack_dtype(const c10::optional<at::ScalarType>& dtype,
                          const char* who) {
  const at::ScalarType t = dtype.value_or(at::kBFloat16);
  TORCH_CHECK(dtype_bit(t) & k16, who, ": output dtype must be bf16 or fp16");
  return t;
}

// --------------------------------------------------------------------------
// renderer (render_kernels.hip) — all f32

struct MpiGeom {
  int64_t B, S, H, W;
};

// first-tensor check of the renderer bindings: mpi (B,S,H,W,4)
MpiGeom check_mpi(const char* who, const char* name, const at::Tensor& mpi,
                  int64_t max_S) {
  check_arg(who, name, mpi, mpi, kF32, -1);
  TORCH_CHECK(mpi.dim() == 5 && mpi.size(4) == 4, who, ": ", name,
              " must be (B,S,H,W,4)");
  const MpiGeom g{mpi.size(0), mpi.size(1), mpi.size(2), mpi.size(3)};
  check_ints(who, {g.B, g.S, g.H, g.W, g.H * g.W});
  TORCH_CHECK(g.B <= 65535, who, ": B too large for the grid");
  TORCH_CHECK(g.S <= max_S, who, ": S too large (at most ", max_S, ")");
  return g;
}

constexpr int64_t kMaxPlanes = 192;  // LDS geometry stage of the composites

std::vector<at::Tensor> src_composite_fwd(at::Tensor mpi, at::Tensor depths,
                                          at::Tensor kinv, at::Tensor img,
                                          bool bg_inf, bool alpha) {
  const char* who = "src_composite_fwd";
  const auto [B, S, H, W] = check_mpi(who, "mpi", mpi, kMaxPlanes);
  check_arg(who, "depths", depths, mpi, kF32, B * S);
  check_arg(who, "kinv", kinv, mpi, kF32, B * 9);
  const float* img_p =
      opt_arg<const float>(who, "img", img, mpi, kF32, B * H * W * 3);
  const bool blend = img_p != nullptr;
  auto rgb = at::empty({B, 3, H, W}, mpi.options());
  auto depth = at::empty({B, 1, H, W}, mpi.options());
  auto mpi_blend = blend ? at::empty_like(mpi) : at::empty({0}, mpi.options());
  mine_src_composite_fwd(mpi.data_ptr<float>(), depths.data_ptr<float>(),
                         kinv.data_ptr<float>(), img_p, rgb.data_ptr<float>(),
                         depth.data_ptr<float>(),
                         blend ? mpi_blend.data_ptr<float>() : nullptr, (int)B,
                         (int)S, (int)H, (int)W, bg_inf ? 1 : 0, alpha ? 1 : 0,
                         stream());
  launched(who);
  return {rgb, depth, mpi_blend};
}

at::Tensor src_composite_bwd(at::Tensor mpi, at::Tensor depths,
                             at::Tensor kinv, at::Tensor img, bool bg_inf,
                             bool alpha, at::Tensor g_rgb,
                             at::Tensor g_depth, at::Tensor g_blend) {
  const char* who = "src_composite_bwd";
  const auto [B, S, H, W] = check_mpi(who, "mpi", mpi, kMaxPlanes);
  check_arg(who, "depths", depths, mpi, kF32, B * S);
  check_arg(who, "kinv", kinv, mpi, kF32, B * 9);
  const float* img_p =
      opt_arg<const float>(who, "img", img, mpi, kF32, B * H * W * 3);
  const float* g_rgb_p =
      opt_arg<const float>(who, "g_rgb", g_rgb, mpi, kF32, B * 3 * H * W);
  const float* g_depth_p =
      opt_arg<const float>(who, "g_depth", g_depth, mpi, kF32, B * H * W);
  const float* g_blend_p =
      opt_arg<const float>(who, "g_blend", g_blend, mpi, kF32, mpi.numel());
  auto grad_mpi = at::empty_like(mpi);
  mine_src_composite_bwd(mpi.data_ptr<float>(), depths.data_ptr<float>(),
                         kinv.data_ptr<float>(), img_p, g_rgb_p, g_depth_p,
                         g_blend_p, grad_mpi.data_ptr<float>(), (int)B, (int)S,
                         (int)H, (int)W, bg_inf ? 1 : 0, alpha ? 1 : 0,
                         stream());
  launched(who);
  return grad_mpi;
}

std::vector<at::Tensor> tgt_composite_fwd(at::Tensor mpi, at::Tensor hinv,
                                          at::Tensor m, at::Tensor tvec,
                                          at::Tensor depths, bool bg_inf,
                                          bool alpha) {
  const char* who = "tgt_composite_fwd";
  const auto [B, S, H, W] = check_mpi(who, "mpi", mpi, kMaxPlanes);
  TORCH_CHECK(H * W * 4 < (int64_t(1) << 31), who,
              ": one plane must stay below 2^31 floats (32-bit tap offsets)");
  check_arg(who, "hinv", hinv, mpi, kF32, B * S * 9);
  check_arg(who, "m", m, mpi, kF32, B * 9);
  check_arg(who, "tvec", tvec, mpi, kF32, B * 3);
  check_arg(who, "depths", depths, mpi, kF32, B * S);
  auto rgb = at::empty({B, 3, H, W}, mpi.options());
  auto depth = at::empty({B, 1, H, W}, mpi.options());
  auto mask = at::empty({B, 1, H, W}, mpi.options());
  mine_tgt_composite_fwd(mpi.data_ptr<float>(), hinv.data_ptr<float>(),
                         m.data_ptr<float>(), tvec.data_ptr<float>(),
                         depths.data_ptr<float>(), rgb.data_ptr<float>(),
                         depth.data_ptr<float>(), mask.data_ptr<float>(),
                         (int)B, (int)S, (int)H, (int)W, bg_inf ? 1 : 0,
                         alpha ? 1 : 0, stream());
  launched(who);
  return {rgb, depth, mask};
}

// mode 1 (default): gather redesign — interior pixels write plain
// per-plane payloads, a per-src-tile gather kernel inverts the map
// (hfwd required). mode 0: the round-1 all-atomic scatter (kept for
// A/B tests and as a fallback; hfwd is not looked at). mode 2:
// order-fixed — every target pixel emits its payload and
// tgt_collect_kernel pulls it into grad_mpi with no float atomic
// (deterministic mode; hfwd required).
// workspace (trailing, default none = allocate here) is the mode-1 / 2
// payload buffer, same shape as mpi. Its contents on entry do not
// matter: the backward kernel writes every entry before the gather
// kernel reads it, so it is at::empty here and a test may hand in a
// NaN-filled one.
at::Tensor tgt_composite_bwd(at::Tensor mpi, at::Tensor hinv, at::Tensor hfwd,
                             at::Tensor m, at::Tensor tvec, at::Tensor depths,
                             bool bg_inf, bool alpha, at::Tensor g_rgb,
                             at::Tensor g_depth, int64_t mode,
                             c10::optional<at::Tensor> workspace) {
  const char* who = "tgt_composite_bwd";
  const auto [B, S, H, W] = check_mpi(who, "mpi", mpi, kMaxPlanes);
  TORCH_CHECK(H * W * 4 < (int64_t(1) << 31), who,
              ": one plane must stay below 2^31 floats (32-bit tap offsets)");
  TORCH_CHECK(mode >= 0 && mode <= 2, who, ": unknown mode");
  check_arg(who, "hinv", hinv, mpi, kF32, B * S * 9);
  check_arg(who, "m", m, mpi, kF32, B * 9);
  check_arg(who, "tvec", tvec, mpi, kF32, B * 3);
  check_arg(who, "depths", depths, mpi, kF32, B * S);
  const float* g_rgb_p =
      opt_arg<const float>(who, "g_rgb", g_rgb, mpi, kF32, B * 3 * H * W);
  const float* g_depth_p =
      opt_arg<const float>(who, "g_depth", g_depth, mpi, kF32, B * H * W);
  at::Tensor payload;
  if (mode >= 1) {
    check_arg(who, "hfwd", hfwd, mpi, kF32, B * S * 9);
    if (workspace.has_value()) {
      payload = *workspace;
      check_arg(who, "workspace", payload, mpi, kF32, mpi.numel());
    } else {
      payload = at::empty_like(mpi);
    }
  }
  // mode 2 (order-fixed): the collect pass stores every grad_mpi entry,
  // so there is no zero fill; the payload is the same workspace
  auto grad_mpi = mode == 2 ? at::empty_like(mpi) : at::zeros_like(mpi);
  mine_tgt_composite_bwd(mpi.data_ptr<float>(), hinv.data_ptr<float>(),
                         mode >= 1 ? hfwd.data_ptr<float>() : nullptr,
                         m.data_ptr<float>(), tvec.data_ptr<float>(),
                         depths.data_ptr<float>(), g_rgb_p, g_depth_p,
                         grad_mpi.data_ptr<float>(),
                         mode >= 1 ? payload.data_ptr<float>() : nullptr,
                         (int)B, (int)S, (int)H, (int)W, bg_inf ? 1 : 0,
                         (int)mode, alpha ? 1 : 0, stream());
  launched(who);
  return grad_mpi;
}

// View-batched novel-view render: V cameras read ONE mpi (B,S,H,W,4).
// Geometry and outputs are view-major, row v*B + b: hinv (V,B,S,3,3),
// m (V,B,3,3), tvec (V,B,3); depths (B,S) belongs to the MPI.

// the checks both view-batched bindings share; returns the MPI geometry
MpiGeom check_views(const char* who, const at::Tensor& mpi,
                    const at::Tensor& hinv, const at::Tensor& m,
                    const at::Tensor& tvec, const at::Tensor& depths,
                    int64_t V) {
  const MpiGeom g = check_mpi(who, "mpi", mpi, kMaxPlanes);
  TORCH_CHECK(g.H * g.W * 4 < (int64_t(1) << 31), who,
              ": one plane must stay below 2^31 floats (32-bit tap offsets)");
  TORCH_CHECK(V >= 1, who, ": views must be at least 1, got ", V);
  TORCH_CHECK(V * g.B <= 65535, who, ": views * B too large for the grid");
  check_arg(who, "hinv", hinv, mpi, kF32, V * g.B * g.S * 9);
  check_arg(who, "m", m, mpi, kF32, V * g.B * 9);
  check_arg(who, "tvec", tvec, mpi, kF32, V * g.B * 3);
  check_arg(who, "depths", depths, mpi, kF32, g.B * g.S);
  return g;
}

std::vector<at::Tensor> tgt_views_fwd(at::Tensor mpi, at::Tensor hinv,
                                      at::Tensor m, at::Tensor tvec,
                                      at::Tensor depths, int64_t views,
                                      bool bg_inf, bool alpha) {
  const char* who = "tgt_views_fwd";
  const int64_t V = views;
  const auto [B, S, H, W] = check_views(who, mpi, hinv, m, tvec, depths, V);
  auto rgb = at::empty({V, B, 3, H, W}, mpi.options());
  auto depth = at::empty({V, B, 1, H, W}, mpi.options());
  auto mask = at::empty({V, B, 1, H, W}, mpi.options());
  mine_tgt_views_fwd(mpi.data_ptr<float>(), hinv.data_ptr<float>(),
                     m.data_ptr<float>(), tvec.data_ptr<float>(),
                     depths.data_ptr<float>(), rgb.data_ptr<float>(),
                     depth.data_ptr<float>(), mask.data_ptr<float>(), (int)V,
                     (int)B, (int)S, (int)H, (int)W, bg_inf ? 1 : 0,
                     alpha ? 1 : 0, stream());
  launched(who);
  return {rgb, depth, mask};
}

// Modes as tgt_composite_bwd. ONE grad_mpi and ONE payload, both the
// size of the MPI, serve all V views: the launcher runs the views in
// stream order. g_rgb (V,B,3,H,W) and g_depth (V,B,1,H,W) may be empty.
// workspace as there: contents on entry do not matter.
at::Tensor tgt_views_bwd(at::Tensor mpi, at::Tensor hinv, at::Tensor hfwd,
                         at::Tensor m, at::Tensor tvec, at::Tensor depths,
                         int64_t views, bool bg_inf, bool alpha,
                         at::Tensor g_rgb, at::Tensor g_depth, int64_t mode,
                         c10::optional<at::Tensor> workspace) {
  const char* who = "tgt_views_bwd";
  const int64_t V = views;
  const auto [B, S, H, W] = check_views(who, mpi, hinv, m, tvec, depths, V);
  TORCH_CHECK(mode >= 0 && mode <= 2, who, ": unknown mode");
  const float* g_rgb_p =
      opt_arg<const float>(who, "g_rgb", g_rgb, mpi, kF32, V * B * 3 * H * W);
  const float* g_depth_p =
      opt_arg<const float>(who, "g_depth", g_depth, mpi, kF32, V * B * H * W);
  at::Tensor payload;
  if (mode >= 1) {
    check_arg(who, "hfwd", hfwd, mpi, kF32, V * B * S * 9);
    if (workspace.has_value()) {
      payload = *workspace;
      check_arg(who, "workspace", payload, mpi, kF32, mpi.numel());
    } else {
      payload = at::empty_like(mpi);
    }
  }
  // mode 2: view 0's collect pass stores every entry, later views add
  auto grad_mpi = mode == 2 ? at::empty_like(mpi) : at::zeros_like(mpi);
  mine_tgt_views_bwd(mpi.data_ptr<float>(), hinv.data_ptr<float>(),
                     mode >= 1 ? hfwd.data_ptr<float>() : nullptr,
                     m.data_ptr<float>(), tvec.data_ptr<float>(),
                     depths.data_ptr<float>(), g_rgb_p, g_depth_p,
                     grad_mpi.data_ptr<float>(),
                     mode >= 1 ? payload.data_ptr<float>() : nullptr, (int)V,
                     (int)B, (int)S, (int)H, (int)W, bg_inf ? 1 : 0, (int)mode,
                     alpha ? 1 : 0, stream());
  launched(who);
  return grad_mpi;
}

// collect pass of the order-fixed warp backward alone, on a caller's
// payload (B,S,H,W,4): grad_mpi[b,s,q] = sum over the target pixels whose
// bilinear taps hit source texel q, in raster order
at::Tensor tgt_collect(at::Tensor payload, at::Tensor hinv, at::Tensor hfwd) {
  const char* who = "tgt_collect";
  const auto [B, S, H, W] = check_mpi(who, "payload", payload, 65535);
  TORCH_CHECK(H * W * 4 < (int64_t(1) << 31), who,
              ": one plane must stay below 2^31 floats (32-bit tap offsets)");
  check_arg(who, "hinv", hinv, payload, kF32, B * S * 9);
  check_arg(who, "hfwd", hfwd, payload, kF32, B * S * 9);
  auto grad_mpi = at::empty_like(payload);
  mine_tgt_collect(payload.data_ptr<float>(), hinv.data_ptr<float>(),
                   hfwd.data_ptr<float>(), grad_mpi.data_ptr<float>(), (int)B,
                   (int)S, (int)H, (int)W, stream());
  launched(who);
  return grad_mpi;
}

// --------------------------------------------------------------------------
// SSIM (ssim_kernels.hip) — f32 (B,C,H,W)

bool g_window_set = false;

void ensure_window() {
  if (g_window_set) return;
  // Gaussian(11, sigma=1.5), normalized (ref network/ssim.py:7-9)
  double w[11], sum = 0.0;
  for (int i = 0; i < 11; ++i) {
    const double d = i - 5;
    w[i] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += w[i];
  }
  float wf[11];
  for (int i = 0; i < 11; ++i) wf[i] = (float)(w[i] / sum);
  mine_ssim_set_window(wf);
  launched("ssim window");
  g_window_set = true;
}

// shared checks of ssim_fwd / ssim_bwd; returns (BC, H, W)
std::array<int64_t, 3> check_ssim(const char* who, const at::Tensor& img1,
                                  const at::Tensor& img2) {
  check_arg(who, "img1", img1, img1, kF32, -1);
  TORCH_CHECK(img1.dim() == 4, who, ": img1 must be (B,C,H,W)");
  check_arg(who, "img2", img2, img1, kF32, img1.numel());
  TORCH_CHECK(img2.sizes() == img1.sizes(), who,
              ": img2 must have the shape of img1");
  const int64_t BC = img1.size(0) * img1.size(1);
  const int64_t H = img1.size(2), W = img1.size(3);
  check_ints(who, {BC, H, W});
  TORCH_CHECK(BC <= 65535, who, ": B*C too large for the grid");
  return {BC, H, W};
}

// det (trailing, default false): per-block partials in an unfilled
// workspace, summed in index order by one block (ssim_kernels.hip)
std::vector<at::Tensor> ssim_fwd(at::Tensor img1, at::Tensor img2, bool det) {
  const char* who = "ssim_fwd";
  const auto [BC, H, W] = check_ssim(who, img1, img2);
  ensure_window();
  const auto sum = reduction_out(
      det, {1}, {BC * mine_ssim_tiles((int)H, (int)W)}, img1);
  mine_ssim_fwd(img1.data_ptr<float>(), img2.data_ptr<float>(), sum.out_ptr(),
                sum.ws_ptr(), (int)BC, (int)H, (int)W, stream());
  launched(who);
  return {(sum.out / (double)(BC * H * W)).squeeze(0)};
}

at::Tensor ssim_bwd(at::Tensor img1, at::Tensor img2, at::Tensor gscale) {
  const char* who = "ssim_bwd";
  const auto [BC, H, W] = check_ssim(who, img1, img2);
  check_arg(who, "gscale", gscale, img1, kF32, 1);
  ensure_window();
  auto F1 = at::empty_like(img1);
  auto F2 = at::empty_like(img1);
  auto F3 = at::empty_like(img1);
  auto grad1 = at::empty_like(img1);
  mine_ssim_bwd(img1.data_ptr<float>(), img2.data_ptr<float>(),
                gscale.data_ptr<float>(), F1.data_ptr<float>(),
                F2.data_ptr<float>(), F3.data_ptr<float>(),
                grad1.data_ptr<float>(), (int)BC, (int)H, (int)W, stream());
  launched(who);
  return grad1;
}

// --------------------------------------------------------------------------
// reflection pad (pad_kernels.hip) — logical (N,H,W,C) layout; f32, bf16
// or fp16. The caller (mine_amd/ops/pad.py) maps channels_last / NCHW
// onto it.

at::Tensor reflect_pad_fwd(at::Tensor in, int64_t N, int64_t H, int64_t W,
                           int64_t C, int64_t pad) {
  const char* who = "reflect_pad_fwd";
  check_arg(who, "in", in, in, kFloat, N * H * W * C);
  check_ints(who, {N, H, W, C, H + 2 * pad, W + 2 * pad});
  TORCH_CHECK(pad >= 0 && H > pad && W > pad, who,
              ": pad must be >= 0 and < spatial size");
  auto out = at::empty({N * (H + 2 * pad) * (W + 2 * pad) * C}, in.options());
  launched(who, mine_reflect_pad_fwd(in.data_ptr(), out.data_ptr(), (int)N,
                                     (int)H, (int)W, (int)C, (int)pad,
                                     elem_of(in.scalar_type(), who),
                                     stream()));
  return out;
}

at::Tensor reflect_pad_bwd(at::Tensor gout, int64_t N, int64_t H, int64_t W,
                           int64_t C, int64_t pad) {
  const char* who = "reflect_pad_bwd";
  check_arg(who, "gout", gout, gout, kFloat,
            N * (H + 2 * pad) * (W + 2 * pad) * C);
  check_ints(who, {N, H, W, C, H + 2 * pad, W + 2 * pad});
  TORCH_CHECK(pad >= 0 && H > pad && W > pad, who,
              ": pad must be >= 0 and < spatial size");
  auto gin = at::empty({N * H * W * C}, gout.options());
  launched(who, mine_reflect_pad_bwd(gout.data_ptr(), gin.data_ptr(), (int)N,
                                     (int)H, (int)W, (int)C, (int)pad,
                                     elem_of(gout.scalar_type(), who),
                                     stream()));
  return gin;
}

// --------------------------------------------------------------------------
// fused BatchNorm + activation (bn_kernels.hip). Tensors arrive as flat
// logical (M, C) channels_last views; f32, bf16 or fp16.
//
// max_blocks (trailing, default 0 = automatic) caps grid.x of the BN
// launches so a test can run the strided row loop and its tail at a
// small shape.
//
// deterministic (trailing, default false): the reduction kernels write
// per-block partials into an unfilled [grid.x][2][C] workspace and
// mine_bn_det_finish adds them in a fixed order (bn_kernels.hip).

// Output of a BN reduction over (M, C) of type `elem`: (2, C) sums, or
// `sums_numel` = 0 where only the finish's mean / invstd are wanted
Reduction bn_reduction_out(const char* who, bool det, const at::Tensor& x,
                           int64_t M, int64_t C, int64_t max_blocks,
                           int64_t sums_numel) {
  int64_t G = 0;
  if (det) {
    G = mine_bn_reduce_grid(M, (int)C, (int)max_blocks,
                            elem_of(x.scalar_type(), who));
    TORCH_CHECK(G > 0, who, ": no reduction grid for this dtype and shape");
  }
  return reduction_out(det, {sums_numel}, {G, 2, C}, x);
}

// The BN "partials, then finish" step: nothing in the default mode; in
// deterministic mode one launch sums r.ws into r.out (where it has
// elements) and finalizes into mean / invstd / running stats (where given).
void bn_det_finish(const char* who, const Reduction& r, int64_t M, int64_t C,
                   float* mean = nullptr, float* invstd = nullptr,
                   float* running_mean = nullptr,
                   float* running_var = nullptr, double eps = 0.0,
                   double momentum = 0.0) {
  if (!r.ws.defined()) return;
  mine_bn_det_finish(r.ws_ptr(), (int)r.ws.size(0), (int)C,
                     r.out.numel() ? r.out_ptr() : nullptr, mean, invstd,
                     running_mean, running_var, M, (float)eps, (float)momentum,
                     stream());
  launched(who);
}

// x of bn_sums / bn_stats
void check_bn_x(const char* who, const at::Tensor& x, int64_t M, int64_t C,
                int64_t max_blocks) {
  check_arg(who, "x", x, x, kFloat, M * C);
  check_ints(who, {M, C});
  TORCH_CHECK(max_blocks >= 0 && max_blocks <= INT_MAX, who,
              ": max_blocks out of range");
}

// stats pass over x into r.target()
void bn_stats_pass(const char* who, const at::Tensor& x, const Reduction& r,
                   int64_t M, int64_t C, int64_t max_blocks) {
  launched(who, mine_bn_stats(x.data_ptr(), r.target(), M, (int)C,
                              (int)max_blocks, r.ws.defined() ? 1 : 0,
                              elem_of(x.scalar_type(), who), stream()));
}

at::Tensor bn_sums(at::Tensor x, int64_t M, int64_t C, int64_t max_blocks,
                   bool deterministic) {
  const char* who = "bn_sums";
  check_bn_x(who, x, M, C, max_blocks);
  const auto r =
      bn_reduction_out(who, deterministic, x, M, C, max_blocks, 2 * C);
  bn_stats_pass(who, x, r, M, C, max_blocks);
  bn_det_finish(who, r, M, C);
  return r.out;
}

// running_mean / running_var (C) f32, both given or both absent
void check_running(const char* who, const at::Tensor& first,
                   const at::Tensor& running_mean,
                   const at::Tensor& running_var, int64_t C, float** rm,
                   float** rv) {
  *rm = opt_arg<float>(who, "running_mean", running_mean, first, kF32, C);
  *rv = opt_arg<float>(who, "running_var", running_var, first, kF32, C);
  TORCH_CHECK((*rm == nullptr) == (*rv == nullptr), who,
              ": running_mean and running_var go together");
}

// (sum, sumsq) -> (mean, invstd) + running-stat update
std::vector<at::Tensor> bn_finalize(at::Tensor sums, int64_t M, int64_t C,
                                    at::Tensor running_mean,
                                    at::Tensor running_var, double eps,
                                    double momentum) {
  const char* who = "bn_finalize";
  check_arg(who, "sums", sums, sums, kF32, 2 * C);
  check_ints(who, {M, C});
  float *rm, *rv;
  check_running(who, sums, running_mean, running_var, C, &rm, &rv);
  auto mean = at::empty({C}, sums.options());
  auto invstd = at::empty({C}, sums.options());
  mine_bn_finalize(sums.data_ptr<float>(), mean.data_ptr<float>(),
                   invstd.data_ptr<float>(), rm, rv, M, (int)C, (float)eps,
                   (float)momentum, stream());
  launched(who);
  return {mean, invstd};
}

std::vector<at::Tensor> bn_stats(at::Tensor x, int64_t M, int64_t C,
                                 at::Tensor running_mean,
                                 at::Tensor running_var, double eps,
                                 double momentum, int64_t max_blocks,
                                 bool deterministic) {
  const char* who = "bn_stats";
  check_bn_x(who, x, M, C, max_blocks);
  float *rm, *rv;
  check_running(who, x, running_mean, running_var, C, &rm, &rv);
  if (!deterministic)
    return bn_finalize(bn_sums(x, M, C, max_blocks, false), M, C, running_mean,
                       running_var, eps, momentum);
  // the finishing kernel also finalizes: two launches, no zero fill
  const auto r = bn_reduction_out(who, true, x, M, C, max_blocks, 0);
  bn_stats_pass(who, x, r, M, C, max_blocks);
  auto mean = at::empty({C}, r.ws.options());
  auto invstd = at::empty({C}, r.ws.options());
  bn_det_finish(who, r, M, C, mean.data_ptr<float>(),
                invstd.data_ptr<float>(), rm, rv, eps, momentum);
  return {mean, invstd};
}

// SplitConvBlock join fused into the stats pass (see bn_kernels.hip):
// y_dec (B*S,HW,C), y_base (B,HW,C), bias (B*S,C), flat NHWC, all of one
// 16-bit type T. Returns x = T(T(y_base + bias) + y_dec) and its
// (sum, sumsq).
std::vector<at::Tensor> bn_join_stats(at::Tensor y_dec, at::Tensor y_base,
                                      at::Tensor bias, int64_t B, int64_t S,
                                      int64_t HW, int64_t C,
                                      int64_t max_blocks,
                                      bool deterministic) {
  const char* who = "bn_join_stats";
  check_arg(who, "y_dec", y_dec, y_dec, k16, B * S * HW * C);
  const unsigned same = dtype_bit(y_dec.scalar_type());
  check_arg(who, "y_base", y_base, y_dec, same, B * HW * C);
  check_arg(who, "bias", bias, y_dec, same, B * S * C);
  check_ints(who, {B, S, HW, C});
  TORCH_CHECK(C % 8 == 0, who, ": C must be a multiple of 8");
  TORCH_CHECK(max_blocks >= 0 && max_blocks <= INT_MAX, who,
              ": max_blocks out of range");
  const int64_t M = B * S * HW;
  auto x = at::empty_like(y_dec);
  const auto r =
      bn_reduction_out(who, deterministic, y_dec, M, C, max_blocks, 2 * C);
  launched(who, mine_bn_join_stats(
                    y_dec.data_ptr(), y_base.data_ptr(), bias.data_ptr(),
                    x.data_ptr(), r.target(), M, (int)HW, (int)S, (int)C,
                    (int)max_blocks, deterministic ? 1 : 0,
                    elem_of(y_dec.scalar_type(), who), stream()));
  // the finish launch takes the place of the zero fill
  bn_det_finish(who, r, M, C);
  return {x, r.out};
}

// The arguments bn_act_fwd, bn_act_bwd_reduce and bn_act_bwd_dx share.
// Returns res, which act 4 (add_relu) requires, or null where absent.
const void* check_bn_act(const char* who, const at::Tensor& x,
                         const at::Tensor& res, const at::Tensor& mean,
                         const at::Tensor& invstd, const at::Tensor& gamma,
                         const at::Tensor& beta, int64_t M, int64_t C,
                         int64_t act, int64_t max_blocks) {
  check_bn_x(who, x, M, C, max_blocks);
  const void* res_p = opt_arg<const void>(
      who, "res", res, x, dtype_bit(x.scalar_type()), M * C);
  check_arg(who, "mean", mean, x, kF32, C);
  check_arg(who, "invstd", invstd, x, kF32, C);
  check_arg(who, "gamma", gamma, x, kF32, C);
  check_arg(who, "beta", beta, x, kF32, C);
  TORCH_CHECK(act >= 0 && act <= 4, who, ": unknown activation");
  TORCH_CHECK(act != 4 || res_p != nullptr, who,
              ": res is required for add_relu");
  return res_p;
}

at::Tensor bn_act_fwd(at::Tensor x, at::Tensor res, at::Tensor mean,
                      at::Tensor invstd, at::Tensor gamma, at::Tensor beta,
                      int64_t M, int64_t C, int64_t act, int64_t max_blocks) {
  const char* who = "bn_act_fwd";
  const void* res_p = check_bn_act(who, x, res, mean, invstd, gamma, beta, M,
                                   C, act, max_blocks);
  auto y = at::empty_like(x);
  launched(who, mine_bn_act_fwd(
                    x.data_ptr(), res_p, mean.data_ptr<float>(),
                    invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                    beta.data_ptr<float>(), y.data_ptr(), M, (int)C, (int)act,
                    (int)max_blocks, elem_of(x.scalar_type(), who), stream()));
  return y;
}

at::Tensor bn_act_bwd_reduce(at::Tensor x, at::Tensor res, at::Tensor gy,
                             at::Tensor mean, at::Tensor invstd,
                             at::Tensor gamma, at::Tensor beta, int64_t M,
                             int64_t C, int64_t act, int64_t max_blocks,
                             bool deterministic) {
  const char* who = "bn_act_bwd_reduce";
  const void* res_p = check_bn_act(who, x, res, mean, invstd, gamma, beta, M,
                                   C, act, max_blocks);
  check_arg(who, "gy", gy, x, dtype_bit(x.scalar_type()), M * C);
  const auto red =
      bn_reduction_out(who, deterministic, x, M, C, max_blocks, 2 * C);
  launched(who, mine_bn_act_bwd_reduce(
                    x.data_ptr(), act == 4 ? res_p : nullptr, gy.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    gamma.data_ptr<float>(), beta.data_ptr<float>(),
                    red.target(), M, (int)C, (int)act, (int)max_blocks,
                    deterministic ? 1 : 0, elem_of(x.scalar_type(), who),
                    stream()));
  bn_det_finish(who, red, M, C);
  return red.out;  // (dbeta, dgamma)
}

// M iterates the LOCAL elements; M_norm is the (possibly cross-rank
// global) batch count in the d(mean)/d(var) terms — they differ only
// under SyncBN, where `red` has been all-reduced in between.
std::vector<at::Tensor> bn_act_bwd_dx(at::Tensor x, at::Tensor res,
                                      at::Tensor gy, at::Tensor mean,
                                      at::Tensor invstd, at::Tensor gamma,
                                      at::Tensor beta, at::Tensor red,
                                      int64_t M, int64_t C, int64_t act,
                                      int64_t M_norm, int64_t max_blocks) {
  const char* who = "bn_act_bwd_dx";
  const void* res_p = check_bn_act(who, x, res, mean, invstd, gamma, beta, M,
                                   C, act, max_blocks);
  check_arg(who, "gy", gy, x, dtype_bit(x.scalar_type()), M * C);
  check_arg(who, "red", red, x, kF32, 2 * C);
  TORCH_CHECK(M_norm > 0, who, ": M_norm must be positive");
  const bool add_relu = act == 4;
  // the dx kernel divides by its M argument; rescale red instead of
  // adding a second kernel parameter
  const auto scaled = M_norm != M ? red * ((double)M / (double)M_norm) : red;
  auto dx = at::empty_like(x);
  auto dres = add_relu ? at::empty_like(x) : at::empty({0}, x.options());
  launched(who, mine_bn_act_bwd_dx(
                    x.data_ptr(), add_relu ? res_p : nullptr, gy.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    gamma.data_ptr<float>(), beta.data_ptr<float>(),
                    scaled.data_ptr<float>(), dx.data_ptr(),
                    add_relu ? dres.data_ptr() : nullptr, M, (int)C, (int)act,
                    (int)max_blocks, elem_of(x.scalar_type(), who), stream()));
  return {dx, dres};
}

std::vector<at::Tensor> bn_act_bwd(at::Tensor x, at::Tensor res,
                                   at::Tensor gy, at::Tensor mean,
                                   at::Tensor invstd, at::Tensor gamma,
                                   at::Tensor beta, int64_t M, int64_t C,
                                   int64_t act, bool deterministic) {
  auto red = bn_act_bwd_reduce(x, res, gy, mean, invstd, gamma, beta,
                               M, C, act, 0, deterministic);
  auto dxr = bn_act_bwd_dx(x, res, gy, mean, invstd, gamma, beta, red,
                           M, C, act, M, 0);
  // dgamma = red[C:], dbeta = red[:C]; nothing writes `red` after the
  // dx launch, so views suffice
  return {dxr[0], dxr[1], red.narrow(0, C, C), red.narrow(0, 0, C)};
}

// Small-layer path (submodule _bn; bn_kernels.hip): a reduction stores G
// partials into a workspace (G,2,C) and the consumer adds them itself, so
// a direction is two launches with no fill, finish or counter launch.
// max_blocks > 0 forces the reduction's G, or the consumer's grid.x, in
// place of the plan's; a consumer names the G of its workspace the same
// way (max_blocks_reduce).
struct BnSmall {
  bool small;
  int G, cgv, grid_x;
};

BnSmall bn_small(const char* who, const at::Tensor& x, int64_t M, int64_t C,
                 int64_t max_blocks_reduce, int64_t max_blocks, int64_t cgv) {
  for (const int64_t v : {max_blocks_reduce, max_blocks})
    TORCH_CHECK(v >= 0 && v <= 4096, who, ": max_blocks out of range");
  BnSmall p{};
  const int rc = mine_bn_small_plan(M, (int)C, elem_of(x.scalar_type(), who),
                                    &p.G, &p.cgv, &p.grid_x);
  TORCH_CHECK(rc >= 0, who, ": no plan for this dtype");
  p.small = rc == 1;
  if (max_blocks_reduce > 0) p.G = (int)max_blocks_reduce;
  if (max_blocks > 0) p.grid_x = (int)max_blocks;
  if (cgv > 0) {
    TORCH_CHECK(cgv <= 64 && (cgv & (cgv - 1)) == 0, who,
                ": cgv must be a power of two up to 64");
    p.cgv = (int)cgv;
  }
  return p;
}

// (small, G, reduction cgv, consumer grid.x) for (M, C) of `dtype`
std::tuple<bool, int64_t, int64_t, int64_t> bn_small_plan(
    int64_t M, int64_t C, at::ScalarType dtype) {
  const char* who = "small_plan";
  check_ints(who, {M, C});
  int G, cgv, grid_x;
  const int rc = mine_bn_small_plan(M, (int)C, elem_of(dtype, who), &G, &cgv,
                                    &grid_x);
  return {rc == 1, G, cgv, grid_x};
}

at::Tensor bn_stats_partials(at::Tensor x, int64_t M, int64_t C,
                             int64_t max_blocks, int64_t cgv) {
  const char* who = "stats_partials";
  check_bn_x(who, x, M, C, max_blocks);
  const BnSmall p = bn_small(who, x, M, C, max_blocks, 0, cgv);
  auto ws = at::empty({p.G, 2, C}, x.options().dtype(at::kFloat));
  launched(who, mine_bn_stats_partials(x.data_ptr(), ws.data_ptr<float>(), M,
                                       (int)C, p.G, p.cgv,
                                       elem_of(x.scalar_type(), who),
                                       stream()));
  return ws;
}

// -> y, mean, invstd; running_mean / running_var / num_batches_tracked are
// updated in place where given
std::vector<at::Tensor> bn_act_fwd_ws(
    at::Tensor x, at::Tensor res, at::Tensor ws, at::Tensor gamma,
    at::Tensor beta, int64_t M, int64_t C, int64_t act,
    at::Tensor running_mean, at::Tensor running_var,
    at::Tensor num_batches_tracked, double eps, double momentum,
    int64_t max_blocks_reduce, int64_t max_blocks) {
  const char* who = "act_fwd_ws";
  check_bn_x(who, x, M, C, max_blocks);
  const void* res_p = opt_arg<const void>(
      who, "res", res, x, dtype_bit(x.scalar_type()), M * C);
  const BnSmall p = bn_small(who, x, M, C, max_blocks_reduce, max_blocks, 0);
  check_arg(who, "ws", ws, x, kF32, (int64_t)p.G * 2 * C);
  check_arg(who, "gamma", gamma, x, kF32, C);
  check_arg(who, "beta", beta, x, kF32, C);
  TORCH_CHECK(act >= 0 && act <= 4, who, ": unknown activation");
  TORCH_CHECK(act != 4 || res_p != nullptr, who,
              ": res is required for add_relu");
  float *rm, *rv;
  check_running(who, x, running_mean, running_var, C, &rm, &rv);
  int64_t* nbt = opt_arg<int64_t>(who, "num_batches_tracked",
                                  num_batches_tracked, x, kI64, 1);
  const auto fopt = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  auto mean = at::empty({C}, fopt);
  auto invstd = at::empty({C}, fopt);
  launched(who, mine_bn_act_fwd_ws(
                    x.data_ptr(), act == 4 ? res_p : nullptr,
                    ws.data_ptr<float>(), p.G, gamma.data_ptr<float>(),
                    beta.data_ptr<float>(), y.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(), rm, rv,
                    nbt, M, (int)C, (int)act, p.grid_x, (float)eps,
                    (float)momentum, elem_of(x.scalar_type(), who), stream()));
  return {y, mean, invstd};
}

at::Tensor bn_bwd_reduce_partials(at::Tensor x, at::Tensor res, at::Tensor gy,
                                  at::Tensor mean, at::Tensor invstd,
                                  at::Tensor gamma, at::Tensor beta, int64_t M,
                                  int64_t C, int64_t act, int64_t max_blocks,
                                  int64_t cgv) {
  const char* who = "bwd_reduce_partials";
  const void* res_p = check_bn_act(who, x, res, mean, invstd, gamma, beta, M,
                                   C, act, max_blocks);
  check_arg(who, "gy", gy, x, dtype_bit(x.scalar_type()), M * C);
  const BnSmall p = bn_small(who, x, M, C, max_blocks, 0, cgv);
  auto ws = at::empty({p.G, 2, C}, x.options().dtype(at::kFloat));
  launched(who, mine_bn_act_bwd_reduce_partials(
                    x.data_ptr(), act == 4 ? res_p : nullptr, gy.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    gamma.data_ptr<float>(), beta.data_ptr<float>(),
                    ws.data_ptr<float>(), M, (int)C, (int)act, p.G, p.cgv,
                    elem_of(x.scalar_type(), who), stream()));
  return ws;
}

// -> dx, dres, red (2,C) = (dbeta, dgamma)
std::vector<at::Tensor> bn_act_bwd_dx_ws(
    at::Tensor x, at::Tensor res, at::Tensor gy, at::Tensor mean,
    at::Tensor invstd, at::Tensor gamma, at::Tensor beta, at::Tensor ws,
    int64_t M, int64_t C, int64_t act, int64_t max_blocks_reduce,
    int64_t max_blocks) {
  const char* who = "act_bwd_dx_ws";
  const void* res_p = check_bn_act(who, x, res, mean, invstd, gamma, beta, M,
                                   C, act, max_blocks);
  check_arg(who, "gy", gy, x, dtype_bit(x.scalar_type()), M * C);
  const BnSmall p = bn_small(who, x, M, C, max_blocks_reduce, max_blocks, 0);
  check_arg(who, "ws", ws, x, kF32, (int64_t)p.G * 2 * C);
  const bool add_relu = act == 4;
  auto dx = at::empty_like(x);
  auto dres = add_relu ? at::empty_like(x) : at::empty({0}, x.options());
  auto red = at::empty({2 * C}, x.options().dtype(at::kFloat));
  launched(who, mine_bn_act_bwd_dx_ws(
                    x.data_ptr(), add_relu ? res_p : nullptr, gy.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    gamma.data_ptr<float>(), beta.data_ptr<float>(),
                    ws.data_ptr<float>(), p.G, red.data_ptr<float>(),
                    dx.data_ptr(), add_relu ? dres.data_ptr() : nullptr, M,
                    (int)C, (int)act, p.grid_x, elem_of(x.scalar_type(), who),
                    stream()));
  return {dx, dres, red};
}

// --------------------------------------------------------------------------
// fused MPI head (head_kernels.hip) over a flat (N,4) view of f32, bf16 or
// fp16; the packed MPI is f32 (N,4)

at::Tensor mpi_head_fwd(at::Tensor z, int64_t N, bool alpha) {
  const char* who = "mpi_head_fwd";
  check_arg(who, "z", z, z, kFloat, N * 4);
  TORCH_CHECK(N > 0, who, ": N must be positive");
  auto out = at::empty({N * 4}, z.options().dtype(at::kFloat));
  launched(who, mine_mpi_head_fwd(z.data_ptr(), out.data_ptr<float>(), N,
                                  alpha ? 1 : 0, elem_of(z.scalar_type(), who),
                                  stream()));
  return out;
}

at::Tensor mpi_head_bwd(at::Tensor z, at::Tensor gout, int64_t N, bool alpha) {
  const char* who = "mpi_head_bwd";
  check_arg(who, "z", z, z, kFloat, N * 4);
  check_arg(who, "gout", gout, z, kF32, N * 4);
  TORCH_CHECK(N > 0, who, ": N must be positive");
  auto gz = at::empty_like(z);
  launched(who, mine_mpi_head_bwd(z.data_ptr(), gout.data_ptr<float>(),
                                  gz.data_ptr(), N, alpha ? 1 : 0,
                                  elem_of(z.scalar_type(), who), stream()));
  return gz;
}

// --------------------------------------------------------------------------
// fused reflect-pad + 3x3 conv (conv_kernels.hip, MFMA); flat NHWC views,
// all bf16 or all fp16.
// (src_h, src_w, off) back a zero-embedded logical image for the
// transposed/data-grad use (pad_mode 1, off 1, logical = src + 2);
// plain forward: src == logical, off == 0.
// c_mem = channels per pixel of x in memory: 0 (= C), or 4 with C == 8
// in zero-embed mode (the 4-channel dispconv gradient, staged into the
// lower half of an 8-channel vector).
void conv3x3_fwd(at::Tensor x_flat, at::Tensor wp, at::Tensor bias,
                 at::Tensor out, int64_t N, int64_t H, int64_t W, int64_t C,
                 int64_t K, int64_t pad_mode, int64_t src_h, int64_t src_w,
                 int64_t off, int64_t c_mem) {
  const char* who = "conv3x3_fwd";
  if (c_mem == 0) c_mem = C;
  check_arg(who, "x_flat", x_flat, x_flat, k16, N * src_h * src_w * c_mem);
  const unsigned same = dtype_bit(x_flat.scalar_type());
  check_arg(who, "wp", wp, x_flat, same,
            ((K + 15) / 16) * ((9 * (C / 8) + 3) / 4) * 64 * 8);
  const float* bias_p = opt_arg<const float>(who, "bias", bias, x_flat, kF32, K);
  check_arg(who, "out", out, x_flat, same, N * H * W * K);
  check_ints(who, {N, H, W, C, K, src_h, src_w, c_mem});
  TORCH_CHECK(C % 8 == 0 && N <= 65535 && (H + 3) / 4 <= 65535 && off >= 0 &&
                  off <= INT_MAX,
              who, ": shape out of range");
  if (pad_mode == 0)
    TORCH_CHECK(src_h == H && src_w == W && off == 0 && H >= 2 && W >= 2, who,
                ": the reflect mode needs src == logical, H, W >= 2");
  launched(who, mine_conv3x3_fwd(
                    x_flat.data_ptr(), wp.data_ptr(), bias_p, out.data_ptr(),
                    (int)N, (int)H, (int)W, (int)C, (int)c_mem, (int)K,
                    (int)pad_mode, (int)src_h, (int)src_w, (int)off,
                    elem_of(x_flat.scalar_type(), who), stream()));
}

// (K,C,3,3) weight (fp32, bf16 or fp16, flat) -> fragment-ordered buffer
// of `dtype` (bf16 by default, or fp16) through an int64 gather LUT; LUT
// entries == w.numel() read as zero.
at::Tensor conv3x3_pack(at::Tensor w_flat, at::Tensor lut,
                        c10::optional<at::ScalarType> dtype) {
  const char* who = "conv3x3_pack";
  check_arg(who, "w_flat", w_flat, w_flat, kFloat, -1);
  check_arg(who, "lut", lut, w_flat, kI64, -1);
  const at::ScalarType ot = pack_dtype(dtype, who);
  auto out = at::empty({lut.numel()}, w_flat.options().dtype(ot));
  if (lut.numel())
    launched(who, mine_conv3x3_pack(
                      w_flat.data_ptr(), elem_of(w_flat.scalar_type(), who),
                      lut.data_ptr<int64_t>(), out.data_ptr(),
                      elem_of(ot, who), lut.numel(), w_flat.numel(),
                      stream()));
  return out;
}

// --------------------------------------------------------------------------
// Weight (and bias) gradient of the fused reflect-pad 3x3 conv
// (wrw_kernels.hip). Flat NHWC inputs, both bf16 or both fp16; returns dW
// fp32 (K, C, 3, 3) and, with want_bias, db fp32 (K). Every workgroup
// writes its partial to a workspace and a second kernel sums them in a
// fixed order, so the result is bitwise reproducible. max_slabs caps the
// number of pixel slabs (0 = automatic).
std::tuple<at::Tensor, at::Tensor> wrw_impl(
    const char* who, at::Tensor x_flat, at::Tensor gy_flat, int64_t N,
    int64_t H, int64_t W, int64_t C, int64_t K, bool want_bias,
    int64_t max_slabs) {
  check_arg(who, "x_flat", x_flat, x_flat, k16, N * H * W * C);
  check_arg(who, "gy_flat", gy_flat, x_flat, dtype_bit(x_flat.scalar_type()),
            N * H * W * K);
  check_ints(who, {N, H, W, C, K});
  TORCH_CHECK(C % 16 == 0 && C >= 16 && C <= 64, who,
              ": C must be 16, 32, 48 or 64, got ", C);
  TORCH_CHECK(W >= 2 && H >= 2 && max_slabs >= 0 && max_slabs <= INT_MAX, who,
              ": shape out of range");
  TORCH_CHECK(N * H < (1 << 30) && W < (1 << 24), who, ": image too large");
  // the kernel stages gy in 8-byte (K = 4) or 16-byte pieces; any other
  // channel count is zero-padded to a multiple of 8 first
  int64_t Kmem = K;
  if (K != 4 && K % 8 != 0) {
    Kmem = (K + 7) / 8 * 8;
    gy_flat = at::constant_pad_nd(gy_flat.view({N * H * W, K}),
                                  {0, Kmem - K}).reshape({-1});
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x_flat.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(gy_flat.data_ptr()) % 16 == 0,
              who, ": inputs must be 16-byte aligned");
  int slabs = 0, nkb = 0;
  int64_t ws_floats = 0;
  mine_conv3x3_wrw_plan((int)C, (int)Kmem, N * H, (int)max_slabs, &slabs,
                        &nkb, &ws_floats);
  auto fopt = x_flat.options().dtype(at::kFloat);
  auto ws = at::empty({ws_floats}, fopt);
  auto dw = at::empty({K, C, 3, 3}, fopt);
  auto db = want_bias ? at::empty({K}, fopt) : at::Tensor();
  launched(who, mine_conv3x3_wrw(
                    x_flat.data_ptr(), gy_flat.data_ptr(),
                    ws.data_ptr<float>(), dw.data_ptr<float>(),
                    want_bias ? db.data_ptr<float>() : nullptr, (int)N, (int)H,
                    (int)W, (int)C, (int)Kmem, (int)K, slabs,
                    elem_of(x_flat.scalar_type(), who), stream()));
  return {dw, db};
}

at::Tensor conv3x3_wrw(at::Tensor x_flat, at::Tensor gy_flat, int64_t N,
                       int64_t H, int64_t W, int64_t C, int64_t K,
                       int64_t max_slabs) {
  return std::get<0>(wrw_impl("conv3x3_wrw", x_flat, gy_flat, N, H, W, C, K,
                              false, max_slabs));
}

std::tuple<at::Tensor, at::Tensor> conv3x3_wrw_bias(
    at::Tensor x_flat, at::Tensor gy_flat, int64_t N, int64_t H, int64_t W,
    int64_t C, int64_t K, int64_t max_slabs) {
  return wrw_impl("conv3x3_wrw_bias", x_flat, gy_flat, N, H, W, C, K, true,
                  max_slabs);
}

// --------------------------------------------------------------------------
// nearest x2 upsample (resample_kernels.hip) — flat logical (N,H,W,C);
// bf16 / fp16 need C%8==0, f32 C%4==0.

// geometry check shared by both directions; `t` holds N*H*W*C * scale
int check_upsample(const char* who, const char* name, const at::Tensor& t,
                   int64_t N, int64_t H, int64_t W, int64_t C,
                   int64_t scale) {
  check_arg(who, name, t, t, kFloat, N * H * W * C * scale);
  check_ints(who, {N, H, W, C});
  const int elem = elem_of(t.scalar_type(), who);
  TORCH_CHECK(C % (elem == kElemF32 ? 4 : 8) == 0, who,
              ": C must be a multiple of 4 (f32) or 8 (bf16, fp16)");
  TORCH_CHECK((N * H * W * (C / 4) + 255) / 256 <= UINT_MAX, who,
              ": tensor too large for the grid");
  return elem;
}

at::Tensor upsample2x_fwd(at::Tensor in, int64_t N, int64_t H, int64_t W,
                          int64_t C) {
  const char* who = "upsample2x_fwd";
  const int elem = check_upsample(who, "in", in, N, H, W, C, 1);
  auto out = at::empty({N * H * W * 4 * C}, in.options());
  launched(who, mine_upsample2x_fwd(in.data_ptr(), out.data_ptr(), N, H, W, C,
                                    elem, stream()));
  return out;
}

at::Tensor upsample2x_bwd(at::Tensor gout, int64_t N, int64_t H, int64_t W,
                          int64_t C) {
  const char* who = "upsample2x_bwd";
  const int elem = check_upsample(who, "gout", gout, N, H, W, C, 4);
  auto gin = at::empty({N * H * W * C}, gout.options());
  launched(who, mine_upsample2x_bwd(gout.data_ptr(), gin.data_ptr(), N, H, W,
                                    C, elem, stream()));
  return gin;
}

// --------------------------------------------------------------------------
// general igemm conv (igemm_kernels.hip; encoder / neck / base shapes),
// bf16 or fp16

// one-launch fragment pack: gather through a device LUT (neg -> 0) into
// bf16 (default) or fp16
at::Tensor pack_gather(at::Tensor w, at::Tensor lut,
                       c10::optional<at::ScalarType> dtype) {
  const char* who = "pack_gather";
  check_arg(who, "w", w, w, kFloat, -1);
  check_arg(who, "lut", lut, w, kI32, -1);
  TORCH_CHECK(w.numel() <= INT_MAX, who, ": w too large for an int32 LUT");
  const at::ScalarType ot = pack_dtype(dtype, who);
  auto out = at::empty({lut.numel()}, w.options().dtype(ot));
  if (lut.numel())
    launched(who, mine_pack_gather(w.data_ptr(), lut.data_ptr<int>(),
                                   out.data_ptr(), lut.numel(),
                                   elem_of(w.scalar_type(), who),
                                   elem_of(ot, who), stream()));
  return out;
}

// checks shared by conv_igemm_fwd / conv_igemm_wrw: x_flat holds the
// (Hs,Ws,C) source images of the M = n*P*Q output pixels
void check_igemm(const char* who, const at::Tensor& x_flat, int64_t M,
                 int64_t P, int64_t Q, int64_t K, int64_t Hs, int64_t Ws,
                 int64_t C, int64_t R, int64_t S,
                 std::initializer_list<int64_t> coord_map) {
  check_arg(who, "x_flat", x_flat, x_flat, k16,
            P > 0 && Q > 0 ? M / (P * Q) * Hs * Ws * C : 0);
  check_ints(who, {M, P, Q, K, Hs, Ws, C});
  TORCH_CHECK(M % (P * Q) == 0, who, ": M must be a multiple of P*Q");
  TORCH_CHECK(R == S && (R == 1 || R == 3 || R == 7), who,
              ": the filter must be 1x1, 3x3 or 7x7");
  for (const int64_t v : coord_map)
    TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, who,
                ": coordinate map out of range");
}

at::Tensor conv_igemm_fwd(at::Tensor x_flat, at::Tensor wp, at::Tensor bias,
                          int64_t M, int64_t P, int64_t Q, int64_t K,
                          int64_t Hs, int64_t Ws, int64_t C, int64_t R,
                          int64_t S, int64_t SA, int64_t SB, int64_t SD,
                          int64_t SE, int64_t pad_mode, bool deterministic) {
  const char* who = "conv_igemm_fwd";
  check_igemm(who, x_flat, M, P, Q, K, Hs, Ws, C, R, S,
              {SA, SB, SD, SE, pad_mode});
  TORCH_CHECK(C % 8 == 0, who, ": C must be a multiple of 8");
  TORCH_CHECK(SE >= 1, who, ": SE must be positive");
  const int64_t nchunks = (R * S * (C / 8) + 3) / 4;
  check_arg(who, "wp", wp, x_flat, dtype_bit(x_flat.scalar_type()),
            (K + 15) / 16 * nchunks * 64 * 8);
  const float* bias_p = opt_arg<const float>(who, "bias", bias, x_flat, kF32, K);
  auto out = at::empty({M * K}, x_flat.options());
  // contraction split-K when the (M, K) grid underfills the 256 CUs
  const int64_t blocks = ((M + 63) / 64) * ((K + 63) / 64);
  int64_t splitz = 1;
  if (blocks < 192 && nchunks >= 16)
    splitz = std::min<int64_t>({256 / blocks + 1, nchunks / 4, 16});
  float* ws_ptr = nullptr;
  Reduction acc;
  if (splitz > 1) {
    // the fp32 accumulator is cast into `out` by the epilogue, so it is a
    // workspace in both modes. deterministic: one unfilled (M,K) slice per
    // z, summed in ascending z; default: one zero-filled (M,K), atomics
    acc = reduction_out(deterministic, {deterministic ? 0 : M * K},
                        {splitz * M * K}, x_flat);
    ws_ptr = acc.target();
  }
  launched(who, mine_conv_igemm_fwd(
                    x_flat.data_ptr(), wp.data_ptr(), bias_p, out.data_ptr(),
                    ws_ptr, M, (int)P, (int)Q, (int)K, (int)Hs, (int)Ws,
                    (int)C, (int)R, (int)S, (int)SA, (int)SB, (int)SD, (int)SE,
                    (int)pad_mode, (int)splitz, deterministic ? 1 : 0,
                    elem_of(x_flat.scalar_type(), who), stream()));
  return out;
}

at::Tensor conv_igemm_wrw(at::Tensor x_flat, at::Tensor gy_flat, int64_t M,
                          int64_t P, int64_t Q, int64_t K, int64_t Hs,
                          int64_t Ws, int64_t C, int64_t R, int64_t S,
                          int64_t SA, int64_t SB, int64_t SD, int64_t SE,
                          int64_t pad_mode, bool deterministic) {
  const char* who = "conv_igemm_wrw";
  check_igemm(who, x_flat, M, P, Q, K, Hs, Ws, C, R, S,
              {SA, SB, SD, SE, pad_mode});
  check_arg(who, "gy_flat", gy_flat, x_flat, dtype_bit(x_flat.scalar_type()),
            M * K);
  // deterministic: per-slab partials, summed in ascending slab order by
  // the finish
  const int64_t slabs =
      mine_conv_igemm_wrw_slabs(M, (int)K, (int)C, (int)R, (int)S);
  const auto dw = reduction_out(deterministic, {K, C, R, S},
                                {slabs, K, C, R, S}, x_flat);
  launched(who, mine_conv_igemm_wrw(
                    x_flat.data_ptr(), gy_flat.data_ptr(), dw.out_ptr(),
                    dw.ws_ptr(), M, (int)P, (int)Q, (int)K, (int)Hs, (int)Ws,
                    (int)C, (int)R, (int)S, (int)SA, (int)SB, (int)SD, (int)SE,
                    (int)pad_mode, elem_of(x_flat.scalar_type(), who),
                    stream()));
  return dw.out;
}

// --------------------------------------------------------------------------
// loss kernels (loss_kernels.hip) — f32

// shared checks of eav2_fwd / eav2_bwd: disp (B,1,H,W) contiguous, img
// (B,3,H,W) through its strides (any layout that stays inside its storage)
std::array<int64_t, 3> check_eav2(const char* who, const at::Tensor& disp,
                                  const at::Tensor& img,
                                  const at::Tensor& mean_d) {
  check_arg(who, "disp", disp, disp, kF32, -1);
  TORCH_CHECK(disp.dim() == 4 && disp.size(1) == 1, who,
              ": disp must be (B,1,H,W)");
  const int64_t B = disp.size(0), H = disp.size(2), W = disp.size(3);
  check_ints(who, {B, H, W, H * W});
  TORCH_CHECK(B <= 65535, who, ": B too large for the grid");
  // img goes by strides, so of the one check only the layout clause differs
  TORCH_CHECK(img.is_cuda() && img.device() == disp.device(), who,
              ": img must be on the device of the first tensor");
  TORCH_CHECK(img.scalar_type() == at::kFloat, who, ": img must be f32, got ",
              img.scalar_type());
  TORCH_CHECK(img.dim() == 4 && img.size(0) == B && img.size(1) == 3 &&
                  img.size(2) == H && img.size(3) == W,
              who, ": img must be (B,3,H,W) matching disp");
  for (int d = 0; d < 4; ++d)
    TORCH_CHECK(img.stride(d) >= 0, who, ": img strides must be non-negative");
  check_arg(who, "mean_d", mean_d, disp, kF32, B);
  return {B, H, W};
}

// fused edge-aware smoothness v2
// det (trailing, default false): every block stores its partial into an
// unfilled workspace row and one block per output sums the rows in index
// order, instead of one atomic per block.
at::Tensor eav2_fwd(at::Tensor disp, at::Tensor img, at::Tensor mean_d,
                    bool det) {
  const char* who = "eav2_fwd";
  const auto [B, H, W] = check_eav2(who, disp, img, mean_d);
  const auto out =
      reduction_out(det, {2}, {2, B, mine_eav2_grid((int)(H * W))}, disp);
  mine_eav2_fwd(disp.data_ptr<float>(), img.data_ptr<float>(),
                mean_d.data_ptr<float>(), out.out_ptr(), out.ws_ptr(), (int)B,
                (int)H, (int)W, img.stride(0), img.stride(1), img.stride(2),
                img.stride(3), stream());
  launched(who);
  return out.out;
}

at::Tensor eav2_bwd(at::Tensor disp, at::Tensor img, at::Tensor mean_d,
                    at::Tensor gl, bool det) {
  const char* who = "eav2_bwd";
  const auto [B, H, W] = check_eav2(who, disp, img, mean_d);
  check_arg(who, "gl", gl, disp, kF32, 1);
  auto g_d = at::empty({B, 1, H, W}, disp.options());
  const auto Tb =
      reduction_out(det, {B}, {B, mine_eav2_grid((int)(H * W))}, disp);
  auto grad = at::empty_like(disp);
  mine_eav2_bwd(disp.data_ptr<float>(), img.data_ptr<float>(),
                mean_d.data_ptr<float>(), g_d.data_ptr<float>(), Tb.out_ptr(),
                Tb.ws_ptr(), gl.data_ptr<float>(), grad.data_ptr<float>(),
                (int)B, (int)H, (int)W, img.stride(0), img.stride(1),
                img.stride(2), img.stride(3), stream());
  launched(who);
  return grad;
}

// Backward of the sparse-point gather without atomics: grad_out (B,C,N),
// idx (B,N) int64 flat pixel indices in [0, HW) -> (B,C,HW). Points that
// share a pixel are summed in point order by the first of them.
at::Tensor gather_pxpy_bwd(at::Tensor grad_out, at::Tensor idx, int64_t HW) {
  const char* who = "gather_pxpy_bwd";
  check_arg(who, "grad_out", grad_out, grad_out, kF32, -1);
  TORCH_CHECK(grad_out.dim() == 3, who, ": grad_out must be (B,C,N)");
  const int64_t B = grad_out.size(0), C = grad_out.size(1),
                N = grad_out.size(2);
  check_arg(who, "idx", idx, grad_out, kI64, B * N);
  TORCH_CHECK(HW > 0 && B * C * N < (int64_t(1) << 31), who,
              ": shape out of range");
  auto grad_img = at::zeros({B, C, HW}, grad_out.options());
  if (B * C * N > 0) {
    mine_gather_pxpy_bwd(grad_out.data_ptr<float>(), idx.data_ptr<int64_t>(),
                         grad_img.data_ptr<float>(), (int)B, (int)C, (int)N,
                         HW, stream());
    launched(who);
  }
  return grad_img;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("src_composite_fwd", &src_composite_fwd,
          "fused src-view MPI composite + RGB blend, forward");
  mod.def("src_composite_bwd", &src_composite_bwd);
  mod.def("tgt_composite_fwd", &tgt_composite_fwd,
          "fused plane-sweep warp + z-cull + composite, forward");
  mod.def("tgt_composite_bwd", &tgt_composite_bwd, pybind11::arg("mpi"),
          pybind11::arg("hinv"), pybind11::arg("hfwd"), pybind11::arg("m"),
          pybind11::arg("tvec"), pybind11::arg("depths"),
          pybind11::arg("bg_inf"), pybind11::arg("alpha"),
          pybind11::arg("g_rgb"), pybind11::arg("g_depth"),
          pybind11::arg("mode"), pybind11::arg("workspace") = pybind11::none());
  mod.def("tgt_collect", &tgt_collect,
          "collect pass of the order-fixed warp backward on a given payload",
          pybind11::arg("payload"), pybind11::arg("hinv"),
          pybind11::arg("hfwd"));
  // The top-level names are the single-view bindings, one row each in
  // the table of tests/test_binding_checks.py. The view-batched renderer
  // (a view count, view-major geometry) sits in a submodule; its refusal
  // table is in tests/test_render_views_gpu.py.
  auto views = mod.def_submodule(
      "_views", "novel-view render of V cameras from one MPI");
  views.def("tgt_views_fwd", &tgt_views_fwd, pybind11::arg("mpi"),
            pybind11::arg("hinv"), pybind11::arg("m"), pybind11::arg("tvec"),
            pybind11::arg("depths"), pybind11::arg("views"),
            pybind11::arg("bg_inf"), pybind11::arg("alpha"));
  views.def("tgt_views_bwd", &tgt_views_bwd, pybind11::arg("mpi"),
            pybind11::arg("hinv"), pybind11::arg("hfwd"), pybind11::arg("m"),
            pybind11::arg("tvec"), pybind11::arg("depths"),
            pybind11::arg("views"), pybind11::arg("bg_inf"),
            pybind11::arg("alpha"), pybind11::arg("g_rgb"),
            pybind11::arg("g_depth"), pybind11::arg("mode"),
            pybind11::arg("workspace") = pybind11::none());
  mod.def("ssim_fwd", &ssim_fwd, pybind11::arg("img1"), pybind11::arg("img2"),
          pybind11::arg("det") = false);
  mod.def("ssim_bwd", &ssim_bwd);
  mod.def("eav2_fwd", &eav2_fwd, "fused edge-aware smoothness v2 fwd",
          pybind11::arg("disp"), pybind11::arg("img"),
          pybind11::arg("mean_d"), pybind11::arg("det") = false);
  mod.def("eav2_bwd", &eav2_bwd, "fused edge-aware smoothness v2 bwd",
          pybind11::arg("disp"), pybind11::arg("img"),
          pybind11::arg("mean_d"), pybind11::arg("gl"),
          pybind11::arg("det") = false);
  mod.def("gather_pxpy_bwd", &gather_pxpy_bwd,
          "atomic-free backward of the sparse-point gather",
          pybind11::arg("grad_out"), pybind11::arg("idx"),
          pybind11::arg("HW"));
  namespace py = pybind11;
  mod.def("pack_gather", &pack_gather,
          "one-launch fragment pack through a device LUT", py::arg("w"),
          py::arg("lut"), py::arg("dtype") = py::none());
  mod.def("conv_igemm_fwd", &conv_igemm_fwd,
          "general igemm conv fwd / data-grad (coordinate-remapped)",
          py::arg("x_flat"), py::arg("wp"), py::arg("bias"), py::arg("M"),
          py::arg("P"), py::arg("Q"), py::arg("K"), py::arg("Hs"),
          py::arg("Ws"), py::arg("C"), py::arg("R"), py::arg("S"),
          py::arg("SA"), py::arg("SB"), py::arg("SD"), py::arg("SE"),
          py::arg("pad_mode"), py::arg("deterministic") = false);
  mod.def("conv_igemm_wrw", &conv_igemm_wrw,
          "general igemm conv weight-grad", py::arg("x_flat"),
          py::arg("gy_flat"), py::arg("M"), py::arg("P"), py::arg("Q"),
          py::arg("K"), py::arg("Hs"), py::arg("Ws"), py::arg("C"),
          py::arg("R"), py::arg("S"), py::arg("SA"), py::arg("SB"),
          py::arg("SD"), py::arg("SE"), py::arg("pad_mode"),
          py::arg("deterministic") = false);
  mod.def("upsample2x_fwd", &upsample2x_fwd,
          "nearest x2 upsample fwd, flat NHWC");
  mod.def("upsample2x_bwd", &upsample2x_bwd,
          "nearest x2 upsample bwd (4-child sum), flat NHWC");
  mod.def("reflect_pad_fwd", &reflect_pad_fwd,
          "gather reflection pad over logical (N,H,W,C)");
  mod.def("reflect_pad_bwd", &reflect_pad_bwd,
          "gather (atomic-free) reflection pad backward");
  mod.def("bn_stats", &bn_stats,
          "per-channel mean/invstd + running-stat update", py::arg("x"),
          py::arg("M"), py::arg("C"), py::arg("running_mean"),
          py::arg("running_var"), py::arg("eps"), py::arg("momentum"),
          py::arg("max_blocks") = 0, py::arg("deterministic") = false);
  mod.def("bn_sums", &bn_sums,
          "per-channel (sum, sumsq) only — for cross-rank SyncBN",
          py::arg("x"), py::arg("M"), py::arg("C"),
          py::arg("max_blocks") = 0, py::arg("deterministic") = false);
  mod.def("bn_finalize", &bn_finalize,
          "(sum, sumsq) -> mean/invstd + running-stat update");
  mod.def("bn_join_stats", &bn_join_stats,
          "x = (y_base + bias) + y_dec with its per-channel (sum, sumsq)",
          py::arg("y_dec"), py::arg("y_base"), py::arg("bias"), py::arg("B"),
          py::arg("S"), py::arg("HW"), py::arg("C"),
          py::arg("max_blocks") = 0, py::arg("deterministic") = false);
  mod.def("bn_act_fwd", &bn_act_fwd, "fused normalize + activation",
          py::arg("x"), py::arg("res"), py::arg("mean"), py::arg("invstd"),
          py::arg("gamma"), py::arg("beta"), py::arg("M"), py::arg("C"),
          py::arg("act"), py::arg("max_blocks") = 0);
  mod.def("bn_act_bwd", &bn_act_bwd,
          "fused BN+act backward -> dx, dres, dgamma, dbeta", py::arg("x"),
          py::arg("res"), py::arg("gy"), py::arg("mean"), py::arg("invstd"),
          py::arg("gamma"), py::arg("beta"), py::arg("M"), py::arg("C"),
          py::arg("act"), py::arg("deterministic") = false);
  mod.def("bn_act_bwd_reduce", &bn_act_bwd_reduce, py::arg("x"),
          py::arg("res"), py::arg("gy"), py::arg("mean"), py::arg("invstd"),
          py::arg("gamma"), py::arg("beta"), py::arg("M"), py::arg("C"),
          py::arg("act"), py::arg("max_blocks") = 0,
          py::arg("deterministic") = false);
  mod.def("bn_act_bwd_dx", &bn_act_bwd_dx, py::arg("x"), py::arg("res"),
          py::arg("gy"), py::arg("mean"), py::arg("invstd"), py::arg("gamma"),
          py::arg("beta"), py::arg("red"), py::arg("M"), py::arg("C"),
          py::arg("act"), py::arg("M_norm"), py::arg("max_blocks") = 0);
  // The small-layer BN path sits in a submodule, as _views does; its
  // refusal table is in tests/test_bn_small_gpu.py.
  auto bn = mod.def_submodule(
      "_bn", "two-launch BatchNorm for small layers: partials + consumer");
  bn.def("small_plan", &bn_small_plan,
         "(small, G, reduction cgv, consumer grid.x) for (M, C) of dtype",
         py::arg("M"), py::arg("C"), py::arg("dtype"));
  bn.def("stats_partials", &bn_stats_partials, py::arg("x"), py::arg("M"),
         py::arg("C"), py::arg("max_blocks") = 0, py::arg("cgv") = 0);
  bn.def("act_fwd_ws", &bn_act_fwd_ws, py::arg("x"), py::arg("res"),
         py::arg("ws"), py::arg("gamma"), py::arg("beta"), py::arg("M"),
         py::arg("C"), py::arg("act"), py::arg("running_mean"),
         py::arg("running_var"), py::arg("num_batches_tracked"),
         py::arg("eps"), py::arg("momentum"),
         py::arg("max_blocks_reduce") = 0, py::arg("max_blocks") = 0);
  bn.def("bwd_reduce_partials", &bn_bwd_reduce_partials, py::arg("x"),
         py::arg("res"), py::arg("gy"), py::arg("mean"), py::arg("invstd"),
         py::arg("gamma"), py::arg("beta"), py::arg("M"), py::arg("C"),
         py::arg("act"), py::arg("max_blocks") = 0, py::arg("cgv") = 0);
  bn.def("act_bwd_dx_ws", &bn_act_bwd_dx_ws, py::arg("x"), py::arg("res"),
         py::arg("gy"), py::arg("mean"), py::arg("invstd"), py::arg("gamma"),
         py::arg("beta"), py::arg("ws"), py::arg("M"), py::arg("C"),
         py::arg("act"), py::arg("max_blocks_reduce") = 0,
         py::arg("max_blocks") = 0);
  mod.def("mpi_head_fwd", &mpi_head_fwd,
          "dispconv out -> packed fp32 MPI (sigmoid rgb, |x|+1e-4 sigma)");
  mod.def("mpi_head_bwd", &mpi_head_bwd);
  mod.def("conv3x3_fwd", &conv3x3_fwd,
          "fused reflect/zero-pad + 3x3 conv on MFMA 16x16x32 tiles",
          py::arg("x_flat"), py::arg("wp"), py::arg("bias"), py::arg("out"),
          py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("K"),
          py::arg("pad_mode"), py::arg("src_h"), py::arg("src_w"),
          py::arg("off"), py::arg("c_mem") = 0);
  mod.def("conv3x3_pack", &conv3x3_pack,
          "gather a conv weight into MFMA fragment order (bf16 or fp16)",
          py::arg("w_flat"), py::arg("lut"), py::arg("dtype") = py::none());
  mod.def("conv3x3_wrw", &conv3x3_wrw,
          "reflect-pad 3x3 conv weight gradient, fp32 (K, C, 3, 3)",
          py::arg("x_flat"), py::arg("gy_flat"), py::arg("N"), py::arg("H"),
          py::arg("W"), py::arg("C"), py::arg("K"), py::arg("max_slabs") = 0);
  mod.def("conv3x3_wrw_bias", &conv3x3_wrw_bias,
          "weight and bias gradient in one pass -> (dw, db)",
          py::arg("x_flat"), py::arg("gy_flat"), py::arg("N"), py::arg("H"),
          py::arg("W"), py::arg("C"), py::arg("K"), py::arg("max_slabs") = 0);
}
