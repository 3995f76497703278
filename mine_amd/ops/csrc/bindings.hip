// Torch bindings for the mine_amd HIP kernels (gfx950 only).
//
// Tensor-level contracts are documented in mine_amd/ops/renderer.py and
// mine_amd/ops/ssim.py. Everything here is thin glue: shape checks,
// output allocation, stream plumbing.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <vector>

extern "C" {
void mine_src_composite_fwd(const float*, const float*, const float*,
                            const float*, float*, float*, float*, int, int,
                            int, int, int, int, hipStream_t);
void mine_src_composite_bwd(const float*, const float*, const float*,
                            const float*, const float*, const float*,
                            const float*, float*, int, int, int, int, int,
                            int, hipStream_t);
void mine_tgt_composite_fwd(const float*, const float*, const float*,
                            const float*, const float*, float*, float*,
                            float*, int, int, int, int, int, int,
                            hipStream_t);
void mine_tgt_composite_bwd(const float*, const float*, const float*,
                            const float*, const float*, const float*,
                            const float*, const float*, float*, float*,
                            int, int, int, int, int, int, int, hipStream_t);
void mine_tgt_collect(const float*, const float*, const float*, float*, int,
                      int, int, int, hipStream_t);
void mine_conv_igemm_fwd(const void*, const void*, const float*, void*,
                         float*, int64_t, int, int, int, int, int, int, int,
                         int, int, int, int, int, int, int, int, int,
                         hipStream_t);
int mine_conv_igemm_wrw_slabs(int64_t, int, int, int, int);
void mine_conv_igemm_wrw(const void*, const void*, float*, float*, int64_t,
                         int, int, int, int, int, int, int, int, int, int,
                         int, int, int, int, hipStream_t);
int mine_eav2_grid(int);
void mine_eav2_fwd(const float*, const float*, const float*, float*, float*,
                   int, int, int, int64_t, int64_t, int64_t, int64_t,
                   hipStream_t);
void mine_eav2_bwd(const float*, const float*, const float*, float*, float*,
                   float*, const float*, float*, int, int, int, int64_t,
                   int64_t, int64_t, int64_t, hipStream_t);
void mine_gather_pxpy_bwd(const float*, const int64_t*, float*, int, int, int,
                          int64_t, hipStream_t);
void mine_pack_gather(const void*, const int*, void*, int64_t, int, int,
                      hipStream_t);
void mine_upsample2x_fwd(const void*, void*, int64_t, int64_t, int64_t,
                         int64_t, int, hipStream_t);
void mine_upsample2x_bwd(const void*, void*, int64_t, int64_t, int64_t,
                         int64_t, int, hipStream_t);
void mine_reflect_pad_fwd_f32(const float*, float*, int, int, int, int, int,
                              hipStream_t);
void mine_reflect_pad_fwd_bf16(const void*, void*, int, int, int, int, int,
                               hipStream_t);
void mine_reflect_pad_fwd_f16(const void*, void*, int, int, int, int, int,
                              hipStream_t);
void mine_reflect_pad_bwd_f16(const void*, void*, int, int, int, int, int,
                              hipStream_t);
void mine_reflect_pad_bwd_f32(const float*, float*, int, int, int, int, int,
                              hipStream_t);
void mine_reflect_pad_bwd_bf16(const void*, void*, int, int, int, int, int,
                               hipStream_t);
int mine_conv3x3_fwd(const void*, const void*, const float*, void*, int, int,
                     int, int, int, int, int, int, int, int, int, hipStream_t);
void mine_conv3x3_pack(const void*, int, const int64_t*, void*, int, int64_t,
                       int64_t, hipStream_t);
void mine_conv3x3_wrw_plan(int, int, int64_t, int, int*, int*, int64_t*);
int mine_conv3x3_wrw(const void*, const void*, float*, float*, float*, int,
                     int, int, int, int, int, int, int, hipStream_t);
void mine_mpi_head_fwd_f32(const void*, float*, int64_t, int, hipStream_t);
void mine_mpi_head_fwd_bf16(const void*, float*, int64_t, int, hipStream_t);
void mine_mpi_head_fwd_f16(const void*, float*, int64_t, int, hipStream_t);
void mine_mpi_head_bwd_f16(const void*, const float*, void*, int64_t, int,
                           hipStream_t);
void mine_mpi_head_bwd_f32(const void*, const float*, void*, int64_t, int,
                           hipStream_t);
void mine_mpi_head_bwd_bf16(const void*, const float*, void*, int64_t, int,
                            hipStream_t);
void mine_bn_stats_f32(const void*, float*, int64_t, int, int, int,
                       hipStream_t);
void mine_bn_stats_bf16(const void*, float*, int64_t, int, int, int,
                        hipStream_t);
void mine_bn_stats_f16(const void*, float*, int64_t, int, int, int,
                       hipStream_t);
int mine_bn_reduce_grid_f16(int64_t, int, int);
int mine_bn_reduce_grid_f32(int64_t, int, int);
int mine_bn_reduce_grid_bf16(int64_t, int, int);
void mine_bn_det_finish(const float*, int, int, float*, float*, float*,
                        float*, float*, int64_t, float, float, hipStream_t);
void mine_bn_join_stats_bf16(const void*, const void*, const void*, void*,
                             float*, int64_t, int, int, int, int, int,
                             hipStream_t);
void mine_bn_join_stats_f16(const void*, const void*, const void*, void*,
                            float*, int64_t, int, int, int, int, int,
                            hipStream_t);
void mine_bn_finalize(const float*, float*, float*, float*, float*, int64_t,
                      int, float, float, hipStream_t);
void mine_bn_act_fwd_f32(const void*, const void*, const float*, const float*,
                         const float*, const float*, void*, int64_t, int, int,
                         int, hipStream_t);
void mine_bn_act_fwd_bf16(const void*, const void*, const float*, const float*,
                          const float*, const float*, void*, int64_t, int, int,
                          int, hipStream_t);
void mine_bn_act_fwd_f16(const void*, const void*, const float*, const float*,
                         const float*, const float*, void*, int64_t, int, int,
                         int, hipStream_t);
void mine_bn_act_bwd_reduce_f16(const void*, const void*, const void*,
                                const float*, const float*, const float*,
                                const float*, float*, int64_t, int, int, int,
                                int, hipStream_t);
void mine_bn_act_bwd_dx_f16(const void*, const void*, const void*,
                            const float*, const float*, const float*,
                            const float*, const float*, void*, void*, int64_t,
                            int, int, int, hipStream_t);
void mine_bn_act_bwd_reduce_f32(const void*, const void*, const void*,
                                const float*, const float*, const float*,
                                const float*, float*, int64_t, int, int, int,
                                int, hipStream_t);
void mine_bn_act_bwd_reduce_bf16(const void*, const void*, const void*,
                                 const float*, const float*, const float*,
                                 const float*, float*, int64_t, int, int, int,
                                 int, hipStream_t);
void mine_bn_act_bwd_dx_f32(const void*, const void*, const void*,
                            const float*, const float*, const float*,
                            const float*, const float*, void*, void*, int64_t,
                            int, int, int, hipStream_t);
void mine_bn_act_bwd_dx_bf16(const void*, const void*, const void*,
                             const float*, const float*, const float*,
                             const float*, const float*, void*, void*, int64_t,
                             int, int, int, hipStream_t);
void mine_ssim_set_window(const float*);
int mine_ssim_tiles(int, int);
void mine_ssim_fwd(const float*, const float*, float*, float*, int, int, int,
                   hipStream_t);
void mine_ssim_bwd(const float*, const float*, const float*, float*, float*,
                   float*, float*, int, int, int, hipStream_t);
}

namespace {

#define CHECK_IN(x)                                               \
  TORCH_CHECK((x).is_cuda(), #x " must be on GPU");               \
  TORCH_CHECK((x).is_contiguous(), #x " must be contiguous");     \
  TORCH_CHECK((x).scalar_type() == at::kFloat, #x " must be f32")

const float* optr(const at::Tensor& t) {
  return t.numel() ? t.data_ptr<float>() : nullptr;
}

hipStream_t stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// the two 16-bit element types of the MFMA / stream kernels
bool is_16bit(at::ScalarType t) {
  return t == at::kBFloat16 || t == at::kHalf;
}

// weight dtype code of the pack kernels: 0 fp32, 1 bf16, 2 fp16
int w_kind(at::ScalarType t) {
  return t == at::kBFloat16 ? 1 : (t == at::kHalf ? 2 : 0);
}

// pack output dtype from the optional Python-side argument (default bf16)
at::ScalarType pack_dtype(const c10::optional<at::ScalarType>& dtype,
                          const char* who) {
  const at::ScalarType t = dtype.value_or(at::kBFloat16);
  TORCH_CHECK(is_16bit(t), who, ": output dtype must be bf16 or fp16");
  return t;
}

std::vector<at::Tensor> src_composite_fwd(at::Tensor mpi, at::Tensor depths,
                                          at::Tensor kinv, at::Tensor img,
                                          bool bg_inf, bool alpha) {
  CHECK_IN(mpi); CHECK_IN(depths); CHECK_IN(kinv);
  TORCH_CHECK(mpi.dim() == 5 && mpi.size(4) == 4, "mpi must be (B,S,H,W,4)");
  const int B = mpi.size(0), S = mpi.size(1), H = mpi.size(2), W = mpi.size(3);
  TORCH_CHECK(S <= 192, "S too large for the LDS geometry stage");
  const bool blend = img.numel() > 0;
  if (blend) {
    CHECK_IN(img);
    TORCH_CHECK(img.sizes() == at::IntArrayRef({B, H, W, 3}),
                "img must be (B,H,W,3)");
  }
  auto rgb = at::empty({B, 3, H, W}, mpi.options());
  auto depth = at::empty({B, 1, H, W}, mpi.options());
  auto mpi_blend = blend ? at::empty_like(mpi) : at::empty({0}, mpi.options());
  mine_src_composite_fwd(mpi.data_ptr<float>(), depths.data_ptr<float>(),
                         kinv.data_ptr<float>(), optr(img),
                         rgb.data_ptr<float>(), depth.data_ptr<float>(),
                         blend ? mpi_blend.data_ptr<float>() : nullptr,
                         B, S, H, W, bg_inf ? 1 : 0, alpha ? 1 : 0,
                         stream());
  return {rgb, depth, mpi_blend};
}

at::Tensor src_composite_bwd(at::Tensor mpi, at::Tensor depths,
                             at::Tensor kinv, at::Tensor img, bool bg_inf,
                             bool alpha, at::Tensor g_rgb,
                             at::Tensor g_depth, at::Tensor g_blend) {
  CHECK_IN(mpi);
  const int B = mpi.size(0), S = mpi.size(1), H = mpi.size(2), W = mpi.size(3);
  auto grad_mpi = at::empty_like(mpi);
  mine_src_composite_bwd(mpi.data_ptr<float>(), depths.data_ptr<float>(),
                         kinv.data_ptr<float>(), optr(img), optr(g_rgb),
                         optr(g_depth), optr(g_blend),
                         grad_mpi.data_ptr<float>(), B, S, H, W,
                         bg_inf ? 1 : 0, alpha ? 1 : 0, stream());
  return grad_mpi;
}

std::vector<at::Tensor> tgt_composite_fwd(at::Tensor mpi, at::Tensor hinv,
                                          at::Tensor m, at::Tensor tvec,
                                          at::Tensor depths, bool bg_inf,
                                          bool alpha) {
  CHECK_IN(mpi); CHECK_IN(hinv); CHECK_IN(m); CHECK_IN(tvec); CHECK_IN(depths);
  TORCH_CHECK(mpi.dim() == 5 && mpi.size(4) == 4, "mpi must be (B,S,H,W,4)");
  const int B = mpi.size(0), S = mpi.size(1), H = mpi.size(2), W = mpi.size(3);
  TORCH_CHECK(S <= 192, "S too large for the LDS geometry stage");
  TORCH_CHECK((int64_t)H * W * 4 < (int64_t(1) << 31),
              "one plane must stay below 2^31 floats (32-bit tap offsets)");
  TORCH_CHECK(hinv.sizes() == at::IntArrayRef({B, S, 3, 3}));
  auto rgb = at::empty({B, 3, H, W}, mpi.options());
  auto depth = at::empty({B, 1, H, W}, mpi.options());
  auto mask = at::empty({B, 1, H, W}, mpi.options());
  mine_tgt_composite_fwd(mpi.data_ptr<float>(), hinv.data_ptr<float>(),
                         m.data_ptr<float>(), tvec.data_ptr<float>(),
                         depths.data_ptr<float>(), rgb.data_ptr<float>(),
                         depth.data_ptr<float>(), mask.data_ptr<float>(),
                         B, S, H, W, bg_inf ? 1 : 0, alpha ? 1 : 0,
                         stream());
  return {rgb, depth, mask};
}

// mode 1 (default): gather redesign — interior pixels write plain
// per-plane payloads, a per-src-tile gather kernel inverts the map
// (hfwd required). mode 0: the round-1 all-atomic scatter (kept for
// A/B tests and as a fallback). mode 2: order-fixed — every target pixel
// emits its payload and tgt_collect_kernel pulls it into grad_mpi with
// no float atomic (deterministic mode; hfwd required).
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
  CHECK_IN(mpi);
  const int B = mpi.size(0), S = mpi.size(1), H = mpi.size(2), W = mpi.size(3);
  TORCH_CHECK((int64_t)H * W * 4 < (int64_t(1) << 31),
              "one plane must stay below 2^31 floats (32-bit tap offsets)");
  TORCH_CHECK(mode >= 0 && mode <= 2, "tgt_composite_bwd: unknown mode");
  // mode 2 (order-fixed): the collect pass stores every grad_mpi entry,
  // so there is no zero fill; the payload is the same workspace
  auto grad_mpi = mode == 2 ? at::empty_like(mpi) : at::zeros_like(mpi);
  at::Tensor payload;
  float* pay_ptr = nullptr;
  if (mode >= 1) {
    CHECK_IN(hfwd);
    TORCH_CHECK(hfwd.numel() == (int64_t)B * S * 9,
                "hfwd required in gather and order-fixed mode");
    if (workspace.has_value()) {
      payload = *workspace;
      CHECK_IN(payload);
      TORCH_CHECK(payload.numel() == mpi.numel() &&
                  payload.device() == mpi.device(),
                  "workspace must match mpi in size and device");
    } else {
      payload = at::empty_like(mpi);
    }
    pay_ptr = payload.data_ptr<float>();
  }
  mine_tgt_composite_bwd(mpi.data_ptr<float>(), hinv.data_ptr<float>(),
                         mode >= 1 ? hfwd.data_ptr<float>() : nullptr,
                         m.data_ptr<float>(), tvec.data_ptr<float>(),
                         depths.data_ptr<float>(), optr(g_rgb), optr(g_depth),
                         grad_mpi.data_ptr<float>(), pay_ptr, B, S, H, W,
                         bg_inf ? 1 : 0, (int)mode, alpha ? 1 : 0, stream());
  return grad_mpi;
}

// collect pass of the order-fixed warp backward alone, on a caller's
// payload (B,S,H,W,4): grad_mpi[b,s,q] = sum over the target pixels whose
// bilinear taps hit source texel q, in raster order
at::Tensor tgt_collect(at::Tensor payload, at::Tensor hinv, at::Tensor hfwd) {
  CHECK_IN(payload); CHECK_IN(hinv); CHECK_IN(hfwd);
  TORCH_CHECK(payload.dim() == 5 && payload.size(4) == 4,
              "payload must be (B,S,H,W,4)");
  const int B = payload.size(0), S = payload.size(1), H = payload.size(2),
            W = payload.size(3);
  TORCH_CHECK(B > 0 && S > 0 && S <= 65535 && B <= 65535 && H > 0 && W > 0);
  TORCH_CHECK((int64_t)H * W * 4 < (int64_t(1) << 31),
              "one plane must stay below 2^31 floats (32-bit tap offsets)");
  TORCH_CHECK(hinv.numel() == (int64_t)B * S * 9 &&
              hfwd.numel() == (int64_t)B * S * 9,
              "hinv and hfwd must be (B,S,3,3)");
  auto grad_mpi = at::empty_like(payload);
  mine_tgt_collect(payload.data_ptr<float>(), hinv.data_ptr<float>(),
                   hfwd.data_ptr<float>(), grad_mpi.data_ptr<float>(), B, S,
                   H, W, stream());
  return grad_mpi;
}

// --------------------------------------------------------------------------
// general igemm conv (encoder/neck/base shapes; igemm_kernels.hip)

// fused edge-aware smoothness v2 (loss_kernels.hip)
// det (trailing, default false): every block stores its partial into an
// unfilled workspace row and one block per output sums the rows in index
// order, instead of one atomic per block (loss_kernels.hip).
at::Tensor eav2_fwd(at::Tensor disp, at::Tensor img, at::Tensor mean_d,
                    bool det) {
  TORCH_CHECK(disp.is_cuda() && disp.is_contiguous() &&
              disp.scalar_type() == at::kFloat &&
              img.scalar_type() == at::kFloat);
  const int B = disp.size(0), H = disp.size(2), W = disp.size(3);
  auto out = det ? at::empty({2}, disp.options())
                 : at::zeros({2}, disp.options());
  at::Tensor ws;
  if (det) ws = at::empty({2, B, mine_eav2_grid(H * W)}, disp.options());
  mine_eav2_fwd(disp.data_ptr<float>(), img.data_ptr<float>(),
                mean_d.data_ptr<float>(), out.data_ptr<float>(),
                det ? ws.data_ptr<float>() : nullptr, B, H, W,
                img.stride(0), img.stride(1), img.stride(2), img.stride(3),
                stream());
  return out;
}

at::Tensor eav2_bwd(at::Tensor disp, at::Tensor img, at::Tensor mean_d,
                    at::Tensor gl, bool det) {
  const int B = disp.size(0), H = disp.size(2), W = disp.size(3);
  auto g_d = at::empty({B, 1, H, W}, disp.options());
  auto Tb = det ? at::empty({B}, disp.options())
                : at::zeros({B}, disp.options());
  at::Tensor ws;
  if (det) ws = at::empty({B, mine_eav2_grid(H * W)}, disp.options());
  auto grad = at::empty_like(disp);
  mine_eav2_bwd(disp.data_ptr<float>(), img.data_ptr<float>(),
                mean_d.data_ptr<float>(), g_d.data_ptr<float>(),
                Tb.data_ptr<float>(), det ? ws.data_ptr<float>() : nullptr,
                gl.data_ptr<float>(), grad.data_ptr<float>(), B, H, W,
                img.stride(0), img.stride(1), img.stride(2), img.stride(3),
                stream());
  return grad;
}

// Backward of the sparse-point gather without atomics: grad_out (B,C,N),
// idx (B,N) int64 flat pixel indices in [0, HW) -> (B,C,HW). Points that
// share a pixel are summed in point order by the first of them.
at::Tensor gather_pxpy_bwd(at::Tensor grad_out, at::Tensor idx, int64_t HW) {
  CHECK_IN(grad_out);
  TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() &&
              idx.scalar_type() == at::kLong, "idx must be int64 on GPU");
  TORCH_CHECK(grad_out.dim() == 3 && idx.dim() == 2 &&
              idx.size(0) == grad_out.size(0) &&
              idx.size(1) == grad_out.size(2), "grad_out (B,C,N), idx (B,N)");
  const int64_t B = grad_out.size(0), C = grad_out.size(1),
                N = grad_out.size(2);
  TORCH_CHECK(HW > 0 && B * C * N < (int64_t(1) << 31));
  auto grad_img = at::zeros({B, C, HW}, grad_out.options());
  if (B * C * N > 0)
    mine_gather_pxpy_bwd(grad_out.data_ptr<float>(), idx.data_ptr<int64_t>(),
                         grad_img.data_ptr<float>(), (int)B, (int)C, (int)N,
                         HW, stream());
  return grad_img;
}

// one-launch fragment pack: gather through a device LUT (neg -> 0) into
// bf16 (default) or fp16
at::Tensor pack_gather(at::Tensor w, at::Tensor lut,
                       c10::optional<at::ScalarType> dtype) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && lut.is_contiguous());
  TORCH_CHECK(lut.scalar_type() == at::kInt);
  TORCH_CHECK(w.scalar_type() == at::kFloat || is_16bit(w.scalar_type()),
              "pack_gather: weight must be f32, bf16 or fp16");
  const at::ScalarType ot = pack_dtype(dtype, "pack_gather");
  auto out = at::empty({lut.numel()}, w.options().dtype(ot));
  mine_pack_gather(w.data_ptr(), lut.data_ptr<int>(), out.data_ptr(),
                   lut.numel(), w_kind(w.scalar_type()),
                   ot == at::kHalf ? 1 : 0, stream());
  return out;
}

at::Tensor conv_igemm_fwd(at::Tensor x_flat, at::Tensor wp, at::Tensor bias,
                          int64_t M, int64_t P, int64_t Q, int64_t K,
                          int64_t Hs, int64_t Ws, int64_t C, int64_t R,
                          int64_t S, int64_t SA, int64_t SB, int64_t SD,
                          int64_t SE, int64_t pad_mode, bool deterministic) {
  TORCH_CHECK(x_flat.is_cuda() && x_flat.is_contiguous() &&
              wp.is_contiguous());
  TORCH_CHECK(is_16bit(x_flat.scalar_type()) &&
              wp.scalar_type() == x_flat.scalar_type(),
              "conv_igemm_fwd: x and the packed weights must both be bf16 or "
              "both fp16");
  TORCH_CHECK(C % 8 == 0);
  auto out = at::empty({M * K}, x_flat.options());
  // contraction split-K when the (M, K) grid underfills the 256 CUs
  const int64_t blocks = ((M + 63) / 64) * ((K + 63) / 64);
  const int nchunks = (int)((R * S * (C / 8) + 3) / 4);
  int splitz = 1;
  at::Tensor ws;
  float* ws_ptr = nullptr;
  if (blocks < 192 && nchunks >= 16) {
    splitz = (int)(256 / blocks + 1);
    if (splitz > nchunks / 4) splitz = (int)(nchunks / 4);
    if (splitz > 16) splitz = 16;
    if (splitz > 1) {
      // deterministic: one unfilled (M,K) slice per z, summed in ascending
      // z by the epilogue; default: one zero-filled (M,K), atomics
      const auto fopt = x_flat.options().dtype(at::kFloat);
      ws = deterministic ? at::empty({splitz * M * K}, fopt)
                         : at::zeros({M * K}, fopt);
      ws_ptr = ws.data_ptr<float>();
    }
  }
  mine_conv_igemm_fwd(x_flat.data_ptr(), wp.data_ptr(),
                      bias.numel() ? bias.data_ptr<float>() : nullptr,
                      out.data_ptr(), ws_ptr, M, (int)P, (int)Q, (int)K,
                      (int)Hs, (int)Ws, (int)C, (int)R, (int)S, (int)SA,
                      (int)SB, (int)SD, (int)SE, (int)pad_mode, splitz,
                      deterministic ? 1 : 0,
                      x_flat.scalar_type() == at::kHalf ? 1 : 0, stream());
  return out;
}

at::Tensor conv_igemm_wrw(at::Tensor x_flat, at::Tensor gy_flat, int64_t M,
                          int64_t P, int64_t Q, int64_t K, int64_t Hs,
                          int64_t Ws, int64_t C, int64_t R, int64_t S,
                          int64_t SA, int64_t SB, int64_t SD, int64_t SE,
                          int64_t pad_mode, bool deterministic) {
  TORCH_CHECK(x_flat.is_cuda() && x_flat.is_contiguous() &&
              gy_flat.is_contiguous());
  TORCH_CHECK(is_16bit(x_flat.scalar_type()) &&
              gy_flat.scalar_type() == x_flat.scalar_type(),
              "conv_igemm_wrw: x and gy must both be bf16 or both fp16");
  const auto fopt = x_flat.options().dtype(at::kFloat);
  at::Tensor dw, ws;
  float* ws_ptr = nullptr;
  if (deterministic) {
    // per-slab partials, summed in ascending slab order by the finish
    const int slabs =
        mine_conv_igemm_wrw_slabs(M, (int)K, (int)C, (int)R, (int)S);
    ws = at::empty({slabs, K, C, R, S}, fopt);
    ws_ptr = ws.data_ptr<float>();
    dw = at::empty({K, C, R, S}, fopt);
  } else {
    dw = at::zeros({K, C, R, S}, fopt);
  }
  mine_conv_igemm_wrw(x_flat.data_ptr(), gy_flat.data_ptr(),
                      dw.data_ptr<float>(), ws_ptr, M, (int)P, (int)Q, (int)K,
                      (int)Hs, (int)Ws, (int)C, (int)R, (int)S, (int)SA,
                      (int)SB, (int)SD, (int)SE, (int)pad_mode,
                      x_flat.scalar_type() == at::kHalf ? 1 : 0, stream());
  return dw;
}

// --------------------------------------------------------------------------
// nearest x2 upsample — flat logical (N,H,W,C); bf16 / fp16 need C%8==0,
// f32 C%4==0 (see resample_kernels.hip).

at::Tensor upsample2x_fwd(at::Tensor in, int64_t N, int64_t H, int64_t W,
                          int64_t C) {
  TORCH_CHECK(in.is_cuda() && in.is_contiguous() &&
              in.numel() == N * H * W * C);
  const at::ScalarType t = in.scalar_type();
  TORCH_CHECK(t == at::kFloat || is_16bit(t),
              "upsample2x: dtype must be f32, bf16 or fp16");
  TORCH_CHECK(is_16bit(t) ? (C % 8 == 0) : (C % 4 == 0));
  auto out = at::empty({N * H * W * 4 * C}, in.options());
  mine_upsample2x_fwd(in.data_ptr(), out.data_ptr(), N, H, W, C, w_kind(t),
                      stream());
  return out;
}

at::Tensor upsample2x_bwd(at::Tensor gout, int64_t N, int64_t H, int64_t W,
                          int64_t C) {
  TORCH_CHECK(gout.is_cuda() && gout.is_contiguous() &&
              gout.numel() == N * H * W * 4 * C);
  const at::ScalarType t = gout.scalar_type();
  TORCH_CHECK(t == at::kFloat || is_16bit(t),
              "upsample2x: dtype must be f32, bf16 or fp16");
  TORCH_CHECK(is_16bit(t) ? (C % 8 == 0) : (C % 4 == 0));
  auto gin = at::empty({N * H * W * C}, gout.options());
  mine_upsample2x_bwd(gout.data_ptr(), gin.data_ptr(), N, H, W, C, w_kind(t),
                      stream());
  return gin;
}

// --------------------------------------------------------------------------
// reflection pad — logical (N,H,W,C) layout (see pad_kernels.hip).
// The caller (mine_amd/ops/pad.py) maps channels_last / NCHW onto it.

at::Tensor reflect_pad_fwd(at::Tensor in, int64_t N, int64_t H, int64_t W,
                           int64_t C, int64_t pad) {
  TORCH_CHECK(in.is_cuda() && in.is_contiguous());
  TORCH_CHECK(in.numel() == N * H * W * C, "bad logical shape");
  TORCH_CHECK(H > pad && W > pad, "pad must be < spatial size");
  auto out = at::empty({N * (H + 2 * pad) * (W + 2 * pad) * C}, in.options());
  if (in.scalar_type() == at::kFloat) {
    mine_reflect_pad_fwd_f32(in.data_ptr<float>(), out.data_ptr<float>(),
                             N, H, W, C, pad, stream());
  } else if (in.scalar_type() == at::kBFloat16) {
    mine_reflect_pad_fwd_bf16(in.data_ptr(), out.data_ptr(),
                              N, H, W, C, pad, stream());
  } else if (in.scalar_type() == at::kHalf) {
    mine_reflect_pad_fwd_f16(in.data_ptr(), out.data_ptr(),
                             N, H, W, C, pad, stream());
  } else {
    TORCH_CHECK(false, "reflect_pad: dtype must be f32, bf16 or fp16");
  }
  return out;
}

at::Tensor reflect_pad_bwd(at::Tensor gout, int64_t N, int64_t H, int64_t W,
                           int64_t C, int64_t pad) {
  TORCH_CHECK(gout.is_cuda() && gout.is_contiguous());
  TORCH_CHECK(gout.numel() == N * (H + 2 * pad) * (W + 2 * pad) * C);
  auto gin = at::empty({N * H * W * C}, gout.options());
  if (gout.scalar_type() == at::kFloat) {
    mine_reflect_pad_bwd_f32(gout.data_ptr<float>(), gin.data_ptr<float>(),
                             N, H, W, C, pad, stream());
  } else if (gout.scalar_type() == at::kBFloat16) {
    mine_reflect_pad_bwd_bf16(gout.data_ptr(), gin.data_ptr(),
                              N, H, W, C, pad, stream());
  } else if (gout.scalar_type() == at::kHalf) {
    mine_reflect_pad_bwd_f16(gout.data_ptr(), gin.data_ptr(),
                             N, H, W, C, pad, stream());
  } else {
    TORCH_CHECK(false, "reflect_pad: dtype must be f32, bf16 or fp16");
  }
  return gin;
}

// --------------------------------------------------------------------------
// fused BatchNorm + activation (see bn_kernels.hip). Tensors arrive as
// flat logical (M, C) channels_last views; f32, bf16 or fp16.

#define BN_DISPATCH(FN, T, ...)                                   \
  do {                                                            \
    if ((T) == at::kFloat) FN##_f32(__VA_ARGS__);                 \
    else if ((T) == at::kBFloat16) FN##_bf16(__VA_ARGS__);        \
    else if ((T) == at::kHalf) FN##_f16(__VA_ARGS__);             \
    else TORCH_CHECK(false, "bn: dtype must be f32, bf16 or fp16"); \
  } while (0)

// fused reflect-pad + 3x3 conv (MFMA); flat NHWC views, all bf16 or all
// fp16.
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
  if (c_mem == 0) c_mem = C;
  TORCH_CHECK(x_flat.is_cuda() && x_flat.is_contiguous() &&
              wp.is_contiguous() && out.is_contiguous());
  TORCH_CHECK(is_16bit(x_flat.scalar_type()) &&
              wp.scalar_type() == x_flat.scalar_type() &&
              out.scalar_type() == x_flat.scalar_type(),
              "conv3x3_fwd: x, the packed weights and out must all be bf16 "
              "or all fp16");
  TORCH_CHECK(C % 8 == 0 && x_flat.numel() == N * src_h * src_w * c_mem);
  TORCH_CHECK(out.numel() == N * H * W * K);
  TORCH_CHECK(N > 0 && N <= 65535 && H > 0 && W > 0 && (H + 3) / 4 <= 65535);
  TORCH_CHECK(wp.numel() ==
              ((K + 15) / 16) * ((9 * (C / 8) + 3) / 4) * 64 * 8,
              "conv3x3_fwd: packed weight size does not match (K, C)");
  TORCH_CHECK(bias.numel() == 0 ||
              (bias.numel() == K && bias.scalar_type() == at::kFloat &&
               bias.is_contiguous()));
  if (pad_mode == 0)
    TORCH_CHECK(src_h == H && src_w == W && off == 0 && H >= 2 && W >= 2);
  const int rc = mine_conv3x3_fwd(
      x_flat.data_ptr(), wp.data_ptr(),
      bias.numel() ? bias.data_ptr<float>() : nullptr, out.data_ptr(), (int)N,
      (int)H, (int)W, (int)C, (int)c_mem, (int)K, (int)pad_mode, (int)src_h,
      (int)src_w, (int)off, x_flat.scalar_type() == at::kHalf ? 1 : 0,
      stream());
  TORCH_CHECK(rc == 0, "conv3x3_fwd: no kernel for C=", C, " c_mem=", c_mem,
              " pad_mode=", pad_mode);
}

// (K,C,3,3) weight (fp32, bf16 or fp16, flat) -> fragment-ordered buffer
// of `dtype` (bf16 by default, or fp16) through an int64 gather LUT; LUT
// entries == w.numel() read as zero.
at::Tensor conv3x3_pack(at::Tensor w_flat, at::Tensor lut,
                        c10::optional<at::ScalarType> dtype) {
  TORCH_CHECK(w_flat.is_cuda() && w_flat.is_contiguous() && lut.is_cuda() &&
              lut.is_contiguous() && lut.scalar_type() == at::kLong);
  TORCH_CHECK(w_flat.scalar_type() == at::kFloat ||
              is_16bit(w_flat.scalar_type()),
              "conv3x3_pack: weight must be f32, bf16 or fp16");
  const at::ScalarType ot = pack_dtype(dtype, "conv3x3_pack");
  auto out = at::empty({lut.numel()}, w_flat.options().dtype(ot));
  if (lut.numel())
    mine_conv3x3_pack(w_flat.data_ptr(), w_kind(w_flat.scalar_type()),
                      lut.data_ptr<int64_t>(), out.data_ptr(),
                      ot == at::kHalf ? 1 : 0, lut.numel(), w_flat.numel(),
                      stream());
  return out;
}

// Weight (and bias) gradient of the fused reflect-pad 3x3 conv (see
// wrw_kernels.hip). Flat NHWC inputs, both bf16 or both fp16; returns dW
// fp32 (K, C, 3, 3)
// and, with want_bias, db fp32 (K). Every workgroup writes its partial
// to a workspace and a second kernel sums them in a fixed order, so the
// result is bitwise reproducible. max_slabs caps the number of pixel
// slabs (0 = automatic).
static std::tuple<at::Tensor, at::Tensor> wrw_impl(
    at::Tensor x_flat, at::Tensor gy_flat, int64_t N, int64_t H, int64_t W,
    int64_t C, int64_t K, bool want_bias, int64_t max_slabs) {
  TORCH_CHECK(x_flat.is_cuda() && gy_flat.is_cuda() &&
              x_flat.is_contiguous() && gy_flat.is_contiguous());
  TORCH_CHECK(is_16bit(x_flat.scalar_type()) &&
              gy_flat.scalar_type() == x_flat.scalar_type(),
              "conv3x3_wrw: x and gy must both be bf16 or both fp16");
  TORCH_CHECK(C % 16 == 0 && C >= 16 && C <= 64,
              "conv3x3_wrw: C must be 16, 32, 48 or 64, got ", C);
  TORCH_CHECK(K >= 1 && W >= 2 && H >= 2 && N >= 1 && max_slabs >= 0);
  TORCH_CHECK(N * H < (1 << 30) && W < (1 << 24));
  TORCH_CHECK(x_flat.numel() == N * H * W * C &&
              gy_flat.numel() == N * H * W * K);
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
              "conv3x3_wrw: inputs must be 16-byte aligned");
  int slabs = 0, nkb = 0;
  int64_t ws_floats = 0;
  mine_conv3x3_wrw_plan((int)C, (int)Kmem, N * H, (int)max_slabs, &slabs,
                        &nkb, &ws_floats);
  auto fopt = x_flat.options().dtype(at::kFloat);
  auto ws = at::empty({ws_floats}, fopt);
  auto dw = at::empty({K, C, 3, 3}, fopt);
  auto db = want_bias ? at::empty({K}, fopt) : at::Tensor();
  const int rc = mine_conv3x3_wrw(
      x_flat.data_ptr(), gy_flat.data_ptr(), ws.data_ptr<float>(),
      dw.data_ptr<float>(), want_bias ? db.data_ptr<float>() : nullptr,
      (int)N, (int)H, (int)W, (int)C, (int)Kmem, (int)K, slabs,
      x_flat.scalar_type() == at::kHalf ? 1 : 0, stream());
  TORCH_CHECK(rc != -2, "conv3x3_wrw: kernel launch failed for C=", C,
              " K=", K);
  TORCH_CHECK(rc == 0, "conv3x3_wrw: no kernel for C=", C, " K=", K);
  return {dw, db};
}

at::Tensor conv3x3_wrw(at::Tensor x_flat, at::Tensor gy_flat, int64_t N,
                       int64_t H, int64_t W, int64_t C, int64_t K,
                       int64_t max_slabs) {
  return std::get<0>(
      wrw_impl(x_flat, gy_flat, N, H, W, C, K, false, max_slabs));
}

std::tuple<at::Tensor, at::Tensor> conv3x3_wrw_bias(
    at::Tensor x_flat, at::Tensor gy_flat, int64_t N, int64_t H, int64_t W,
    int64_t C, int64_t K, int64_t max_slabs) {
  return wrw_impl(x_flat, gy_flat, N, H, W, C, K, true, max_slabs);
}

// fused MPI head over a flat (N,4) view; out is fp32 (N,4)
at::Tensor mpi_head_fwd(at::Tensor z, int64_t N, bool alpha) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.numel() == N * 4);
  auto out = at::empty({N * 4}, z.options().dtype(at::kFloat));
  if (z.scalar_type() == at::kFloat)
    mine_mpi_head_fwd_f32(z.data_ptr(), out.data_ptr<float>(), N,
                          alpha ? 1 : 0, stream());
  else if (z.scalar_type() == at::kBFloat16)
    mine_mpi_head_fwd_bf16(z.data_ptr(), out.data_ptr<float>(), N,
                           alpha ? 1 : 0, stream());
  else if (z.scalar_type() == at::kHalf)
    mine_mpi_head_fwd_f16(z.data_ptr(), out.data_ptr<float>(), N,
                          alpha ? 1 : 0, stream());
  else
    TORCH_CHECK(false, "mpi_head: dtype must be f32, bf16 or fp16");
  return out;
}

at::Tensor mpi_head_bwd(at::Tensor z, at::Tensor gout, int64_t N, bool alpha) {
  TORCH_CHECK(gout.is_contiguous() && gout.scalar_type() == at::kFloat);
  auto gz = at::empty_like(z);
  if (z.scalar_type() == at::kFloat)
    mine_mpi_head_bwd_f32(z.data_ptr(), gout.data_ptr<float>(), gz.data_ptr(),
                          N, alpha ? 1 : 0, stream());
  else if (z.scalar_type() == at::kHalf)
    mine_mpi_head_bwd_f16(z.data_ptr(), gout.data_ptr<float>(),
                          gz.data_ptr(), N, alpha ? 1 : 0, stream());
  else
    mine_mpi_head_bwd_bf16(z.data_ptr(), gout.data_ptr<float>(),
                           gz.data_ptr(), N, alpha ? 1 : 0, stream());
  return gz;
}

// max_blocks (trailing, default 0 = automatic) caps grid.x of the BN
// launches so a test can run the strided row loop and its tail at a
// small shape.
//
// deterministic (trailing, default false): the reduction kernels write
// per-block partials into an unfilled [grid.x][2][C] workspace and
// mine_bn_det_finish adds them in a fixed order (bn_kernels.hip).
int bn_reduce_grid(at::ScalarType t, int64_t M, int64_t C,
                   int64_t max_blocks) {
  TORCH_CHECK(t == at::kFloat || is_16bit(t),
              "bn: dtype must be f32, bf16 or fp16");
  if (t == at::kFloat)
    return mine_bn_reduce_grid_f32(M, (int)C, (int)max_blocks);
  return t == at::kHalf ? mine_bn_reduce_grid_f16(M, (int)C, (int)max_blocks)
                        : mine_bn_reduce_grid_bf16(M, (int)C, (int)max_blocks);
}

// deterministic stats pass over x: returns the workspace and its grid.x
at::Tensor bn_stats_partials(const at::Tensor& x, int64_t M, int64_t C,
                             int64_t max_blocks, int* G) {
  *G = bn_reduce_grid(x.scalar_type(), M, C, max_blocks);
  auto ws = at::empty({*G, 2, C}, x.options().dtype(at::kFloat));
  BN_DISPATCH(mine_bn_stats, x.scalar_type(), x.data_ptr(),
              ws.data_ptr<float>(), M, (int)C, (int)max_blocks, 1, stream());
  return ws;
}

at::Tensor bn_sums(at::Tensor x, int64_t M, int64_t C, int64_t max_blocks,
                   bool deterministic) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.numel() == M * C);
  if (deterministic) {
    int G = 0;
    auto ws = bn_stats_partials(x, M, C, max_blocks, &G);
    auto sums = at::empty({2 * C}, ws.options());
    mine_bn_det_finish(ws.data_ptr<float>(), G, (int)C,
                       sums.data_ptr<float>(), nullptr, nullptr, nullptr,
                       nullptr, M, 0.0f, 0.0f, stream());
    return sums;
  }
  auto sums = at::zeros({2 * C}, x.options().dtype(at::kFloat));
  BN_DISPATCH(mine_bn_stats, x.scalar_type(), x.data_ptr(),
              sums.data_ptr<float>(), M, (int)C, (int)max_blocks, 0,
              stream());
  return sums;
}

// (sum, sumsq) -> (mean, invstd) + running-stat update
std::vector<at::Tensor> bn_finalize(at::Tensor sums, int64_t M, int64_t C,
                                    at::Tensor running_mean,
                                    at::Tensor running_var, double eps,
                                    double momentum) {
  TORCH_CHECK(sums.is_cuda() && sums.is_contiguous() &&
              sums.scalar_type() == at::kFloat && sums.numel() == 2 * C);
  auto mean = at::empty({C}, sums.options());
  auto invstd = at::empty({C}, sums.options());
  const bool track = running_mean.numel() > 0;
  mine_bn_finalize(sums.data_ptr<float>(), mean.data_ptr<float>(),
                   invstd.data_ptr<float>(),
                   track ? running_mean.data_ptr<float>() : nullptr,
                   track ? running_var.data_ptr<float>() : nullptr,
                   M, (int)C, (float)eps, (float)momentum, stream());
  return {mean, invstd};
}

std::vector<at::Tensor> bn_stats(at::Tensor x, int64_t M, int64_t C,
                                 at::Tensor running_mean,
                                 at::Tensor running_var, double eps,
                                 double momentum, int64_t max_blocks,
                                 bool deterministic) {
  if (deterministic) {
    // the finishing kernel also finalizes: two launches, no zero fill
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.numel() == M * C);
    int G = 0;
    auto ws = bn_stats_partials(x, M, C, max_blocks, &G);
    auto mean = at::empty({C}, ws.options());
    auto invstd = at::empty({C}, ws.options());
    const bool track = running_mean.numel() > 0;
    mine_bn_det_finish(ws.data_ptr<float>(), G, (int)C, nullptr,
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       track ? running_mean.data_ptr<float>() : nullptr,
                       track ? running_var.data_ptr<float>() : nullptr, M,
                       (float)eps, (float)momentum, stream());
    return {mean, invstd};
  }
  return bn_finalize(bn_sums(x, M, C, max_blocks, false), M, C, running_mean,
                     running_var, eps, momentum);
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
  TORCH_CHECK(y_dec.is_cuda() && y_dec.is_contiguous() &&
              y_base.is_contiguous() && bias.is_contiguous());
  const at::ScalarType jt = y_dec.scalar_type();
  TORCH_CHECK(is_16bit(jt) && y_base.scalar_type() == jt &&
              bias.scalar_type() == jt,
              "bn_join_stats: operands must all be bf16 or all fp16");
  const auto join = jt == at::kHalf ? mine_bn_join_stats_f16
                                    : mine_bn_join_stats_bf16;
  TORCH_CHECK(C % 8 == 0 && B > 0 && S > 0 && HW > 0 &&
              HW < (int64_t(1) << 31));
  TORCH_CHECK(y_dec.numel() == B * S * HW * C &&
              y_base.numel() == B * HW * C && bias.numel() == B * S * C);
  auto x = at::empty_like(y_dec);
  const auto fopt = y_dec.options().dtype(at::kFloat);
  if (deterministic) {
    // the finish launch takes the place of the zero fill
    const int64_t M = B * S * HW;
    const int G = bn_reduce_grid(jt, M, C, max_blocks);
    auto ws = at::empty({G, 2, C}, fopt);
    auto sums = at::empty({2 * C}, fopt);
    join(y_dec.data_ptr(), y_base.data_ptr(), bias.data_ptr(), x.data_ptr(),
         ws.data_ptr<float>(), M, (int)HW, (int)S, (int)C, (int)max_blocks, 1,
         stream());
    mine_bn_det_finish(ws.data_ptr<float>(), G, (int)C,
                       sums.data_ptr<float>(), nullptr, nullptr, nullptr,
                       nullptr, M, 0.0f, 0.0f, stream());
    return {x, sums};
  }
  auto sums = at::zeros({2 * C}, fopt);
  join(y_dec.data_ptr(), y_base.data_ptr(), bias.data_ptr(), x.data_ptr(),
       sums.data_ptr<float>(), B * S * HW, (int)HW, (int)S, (int)C,
       (int)max_blocks, 0, stream());
  return {x, sums};
}

at::Tensor bn_act_fwd(at::Tensor x, at::Tensor res, at::Tensor mean,
                      at::Tensor invstd, at::Tensor gamma, at::Tensor beta,
                      int64_t M, int64_t C, int64_t act, int64_t max_blocks) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.numel() == M * C);
  TORCH_CHECK(act >= 0 && act <= 4, "bn: unknown activation");
  TORCH_CHECK(act != 4 || res.numel() == x.numel());
  auto y = at::empty_like(x);
  BN_DISPATCH(mine_bn_act_fwd, x.scalar_type(), x.data_ptr(),
              res.numel() ? res.data_ptr() : nullptr,
              mean.data_ptr<float>(), invstd.data_ptr<float>(),
              gamma.data_ptr<float>(), beta.data_ptr<float>(), y.data_ptr(),
              M, (int)C, (int)act, (int)max_blocks, stream());
  return y;
}

at::Tensor bn_act_bwd_reduce(at::Tensor x, at::Tensor res, at::Tensor gy,
                             at::Tensor mean, at::Tensor invstd,
                             at::Tensor gamma, at::Tensor beta, int64_t M,
                             int64_t C, int64_t act, int64_t max_blocks,
                             bool deterministic) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && gy.is_contiguous());
  TORCH_CHECK(act >= 0 && act <= 4, "bn: unknown activation");
  const auto fopt = x.options().dtype(at::kFloat);
  const bool add_relu = act == 4;
  at::Tensor red, ws;
  int G = 0;
  if (deterministic) {
    G = bn_reduce_grid(x.scalar_type(), M, C, max_blocks);
    ws = at::empty({G, 2, C}, fopt);
    red = at::empty({2 * C}, fopt);
  } else {
    red = at::zeros({2 * C}, fopt);
  }
  BN_DISPATCH(mine_bn_act_bwd_reduce, x.scalar_type(), x.data_ptr(),
              add_relu ? res.data_ptr() : nullptr, gy.data_ptr(),
              mean.data_ptr<float>(), invstd.data_ptr<float>(),
              gamma.data_ptr<float>(), beta.data_ptr<float>(),
              deterministic ? ws.data_ptr<float>() : red.data_ptr<float>(), M,
              (int)C, (int)act, (int)max_blocks, deterministic ? 1 : 0,
              stream());
  if (deterministic)
    mine_bn_det_finish(ws.data_ptr<float>(), G, (int)C, red.data_ptr<float>(),
                       nullptr, nullptr, nullptr, nullptr, M, 0.0f, 0.0f,
                       stream());
  return red;  // (dbeta, dgamma)
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
  TORCH_CHECK(act >= 0 && act <= 4, "bn: unknown activation");
  const bool add_relu = act == 4;
  auto scaled = red;
  if (M_norm != M) {
    // the dx kernel divides by its M argument; rescale red instead of
    // adding a second kernel parameter
    scaled = red * ((double)M / (double)M_norm);
  }
  scaled = scaled.contiguous();
  auto dx = at::empty_like(x);
  auto dres = add_relu ? at::empty_like(x) : at::empty({0}, x.options());
  BN_DISPATCH(mine_bn_act_bwd_dx, x.scalar_type(), x.data_ptr(),
              add_relu ? res.data_ptr() : nullptr, gy.data_ptr(),
              mean.data_ptr<float>(), invstd.data_ptr<float>(),
              gamma.data_ptr<float>(), beta.data_ptr<float>(),
              scaled.data_ptr<float>(), dx.data_ptr(),
              add_relu ? dres.data_ptr() : nullptr, M, (int)C, (int)act,
              (int)max_blocks, stream());
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

// --------------------------------------------------------------------------

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
  g_window_set = true;
}

// det (trailing, default false): per-block partials in an unfilled
// workspace, summed in index order by one block (ssim_kernels.hip)
std::vector<at::Tensor> ssim_fwd(at::Tensor img1, at::Tensor img2, bool det) {
  CHECK_IN(img1); CHECK_IN(img2);
  TORCH_CHECK(img1.dim() == 4 && img1.sizes() == img2.sizes());
  ensure_window();
  const int BC = img1.size(0) * img1.size(1);
  const int H = img1.size(2), W = img1.size(3);
  auto sum = det ? at::empty({1}, img1.options())
                 : at::zeros({1}, img1.options());
  at::Tensor ws;
  if (det)
    ws = at::empty({(int64_t)BC * mine_ssim_tiles(H, W)}, img1.options());
  mine_ssim_fwd(img1.data_ptr<float>(), img2.data_ptr<float>(),
                sum.data_ptr<float>(), det ? ws.data_ptr<float>() : nullptr,
                BC, H, W, stream());
  return {(sum / (double)(BC * (int64_t)H * W)).squeeze(0)};
}

at::Tensor ssim_bwd(at::Tensor img1, at::Tensor img2, at::Tensor gscale) {
  CHECK_IN(img1); CHECK_IN(img2);
  ensure_window();
  const int BC = img1.size(0) * img1.size(1);
  const int H = img1.size(2), W = img1.size(3);
  auto F1 = at::empty_like(img1);
  auto F2 = at::empty_like(img1);
  auto F3 = at::empty_like(img1);
  auto grad1 = at::empty_like(img1);
  auto g = gscale.to(img1.options()).contiguous();
  mine_ssim_bwd(img1.data_ptr<float>(), img2.data_ptr<float>(),
                g.data_ptr<float>(), F1.data_ptr<float>(),
                F2.data_ptr<float>(), F3.data_ptr<float>(),
                grad1.data_ptr<float>(), BC, H, W, stream());
  return grad1;
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
