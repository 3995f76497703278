// CDNA4 (gfx950) fused MPI rendering kernels.
//
// Design notes (MI355X-first, see /root/repo/SURVEY.md section 2b):
//  * The MPI is packed (B, S, H, W, 4) = rgb+sigma adjacent per pixel, so
//    every per-plane access is ONE naturally-aligned float4 — a wave's 64
//    lanes walk x-adjacent pixels, giving 16 B/lane coalesced streams.
//  * Per output pixel, ONE thread walks all S planes in registers: the
//    compositing scan (shifted cumprod of transparencies) is a sequential
//    recurrence per pixel but embarrassingly parallel across the B*H*W
//    pixels (>3M at the flagship config — far above the 256-CU fill
//    requirement of ~16k threads).
//  * The novel-view kernel fuses homography projection, border-clamped
//    bilinear sampling, analytic warped plane points (bilinear sampling of
//    a linear field == evaluation at the mapped point), z-culling and the
//    volume composite. The reference materialized nine BxSx{3,7}xHxW
//    tensors per scale for this (ref operations/mpi_rendering.py:181-241 +
//    homography_sampler.py:58-141); here nothing but the output leaves
//    registers.
//  * Backward recomputes the forward chain in three ascending passes per
//    pixel (no per-plane state is saved): pass 1 accumulates the composite
//    totals, pass 2 accumulates the cumprod-suffix total, pass 3 emits
//    gradients. Ascending recomputation keeps the running transmittance
//    product stable (no division by ~1e-6 factors).
//  * Per-plane homographies/depths are staged in LDS per workgroup.
//
// Shapes: mpi (B,S,H,W,4) f32; images packed (B,H,W,3); composited outputs
// (B,3,H,W) / (B,1,H,W) channel-major (what the loss stack consumes).

#include <hip/hip_runtime.h>
#include <cstdint>

#include "launchers.h"

#define DEV __device__ __forceinline__

namespace {

constexpr int kBlock = 256;
constexpr int kMaxS = 192;  // LDS budget: 192 planes * 10 f32 = 7.5 KB

struct float3x3 {
  float m[9];
  DEV float3 mul(float x, float y, float z) const {
    return make_float3(m[0] * x + m[1] * y + m[2] * z,
                       m[3] * x + m[4] * y + m[5] * z,
                       m[6] * x + m[7] * y + m[8] * z);
  }
};

DEV float clampf(float v, float lo, float hi) {
  return fminf(fmaxf(v, lo), hi);
}

// ---------------------------------------------------------------------------
// Source-view composite (+ optional RGB blending)
// ---------------------------------------------------------------------------
//   delta_s = |K^-1 p| * (d_{s+1} - d_s), far plane 1e3
//   t = exp(-sigma*delta); u = t + 1e-6; A_s = prod_{j<s} u_j
//   w = A * (1 - t); blended c = A*I + (1-A)*rgb
//   R = sum w*c ; D = sum(w*z)/(sum w + 1e-5)  (or + 1000*(1-sum w))
// ref operations/mpi_rendering.py:42-82, synthesis_task.py:267-274.

// ALPHA: the 4th MPI channel is an alpha in (0,1) (ref
// operations/mpi_rendering.py:23-39): t = 1-alpha (no exp, no plane
// distance), the running product has NO epsilon, and the depth is the
// PLAIN weighted z sum (no normalization, no background term). BLEND
// is never combined with ALPHA (ref mpi_rendering.py:19).
template <bool BLEND, bool BG_INF, bool ALPHA = false>
__global__ void __launch_bounds__(kBlock)
src_composite_fwd_kernel(const float* __restrict__ mpi,
                         const float* __restrict__ depths,   // (B,S)
                         const float* __restrict__ kinv,     // (B,3,3)
                         const float* __restrict__ img,      // (B,H,W,3)
                         float* __restrict__ rgb_out,        // (B,3,H,W)
                         float* __restrict__ depth_out,      // (B,1,H,W)
                         float* __restrict__ mpi_blend,      // (B,S,H,W,4)
                         int B, int S, int H, int W) {
  __shared__ float s_depth[kMaxS];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < S; i += kBlock) s_depth[i] = depths[b * S + i];
  __syncthreads();

  float3x3 Ki;
#pragma unroll
  for (int i = 0; i < 9; ++i) Ki.m[i] = kinv[b * 9 + i];

  const int HW = H * W;
  const int64_t mpi_b = (int64_t)b * S * HW * 4;
  for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < HW;
       pix += gridDim.x * kBlock) {
    const int y = pix / W;
    const int x = pix - y * W;
    const float3 ray = Ki.mul((float)x, (float)y, 1.0f);
    const float nu = sqrtf(ray.x * ray.x + ray.y * ray.y + ray.z * ray.z);

    float3 I = make_float3(0.f, 0.f, 0.f);
    if (BLEND) {
      const float* ip = img + ((int64_t)b * HW + pix) * 3;
      I = make_float3(ip[0], ip[1], ip[2]);
    }

    float A = 1.0f, Wsum = 0.0f, Nsum = 0.0f;
    float3 R = make_float3(0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 px = *reinterpret_cast<const float4*>(
          mpi + mpi_b + ((int64_t)s * HW + pix) * 4);
      const float d = s_depth[s];
      const float delta = (s + 1 < S) ? nu * (s_depth[s + 1] - d) : 1e3f;
      const float t = ALPHA ? (1.0f - px.w) : __expf(-px.w * delta);
      const float w = A * (1.0f - t);
      float3 c = make_float3(px.x, px.y, px.z);
      if (BLEND) {
        c.x = A * I.x + (1.0f - A) * c.x;
        c.y = A * I.y + (1.0f - A) * c.y;
        c.z = A * I.z + (1.0f - A) * c.z;
        float4 ob = make_float4(c.x, c.y, c.z, px.w);
        *reinterpret_cast<float4*>(mpi_blend + mpi_b + ((int64_t)s * HW + pix) * 4) = ob;
      }
      R.x += w * c.x; R.y += w * c.y; R.z += w * c.z;
      Wsum += w;
      Nsum += w * d;  // src-view z of plane s is its depth
      A *= ALPHA ? t : (t + 1e-6f);
      if (A < 1e-14f) {  // dead transmittance: remaining planes add ~0
        if (BLEND) {
          // the blended tail is c = A*I + (1-A)*rgb ~= rgb: copy through
          for (int s2 = s + 1; s2 < S; ++s2) {
            const int64_t o = mpi_b + ((int64_t)s2 * HW + pix) * 4;
            *reinterpret_cast<float4*>(mpi_blend + o) =
                *reinterpret_cast<const float4*>(mpi + o);
          }
        }
        break;
      }
    }
    const float D = ALPHA ? Nsum
                          : (BG_INF ? (Nsum + 1000.0f * (1.0f - Wsum))
                                    : (Nsum / (Wsum + 1e-5f)));
    rgb_out[((int64_t)b * 3 + 0) * HW + pix] = R.x;
    rgb_out[((int64_t)b * 3 + 1) * HW + pix] = R.y;
    rgb_out[((int64_t)b * 3 + 2) * HW + pix] = R.z;
    depth_out[(int64_t)b * HW + pix] = D;
  }
}

// Per-plane backward term, shared by passes 2 and 3.
//
// noinline is LOAD-BEARING: the two passes telescope fp64 prefix sums of
// dA*A against each other and divide the residue by u ~ 1e-6. If the
// passes inline this computation separately, FMA contraction may fuse
// differently in the two contexts, the terms stop being bitwise equal,
// and the nonzero residue at late planes amplifies into O(0.1) sigma
// gradients. One out-of-line instance -> identical bits -> exact
// cancellation.
struct PlaneTerm {
  float t;      // transparency exp(-sigma*delta)
  float e;      // dL/dw
  float dA;     // dL/dA_s (direct)
  float dcx, dcy, dcz;  // dL/dc_s
};

template <bool BLEND, bool BG_INF, bool ALPHA = false>
__device__ __attribute__((noinline)) PlaneTerm
src_plane_term(float4 px, float Af, float3 I, float3 gR, float gD,
               float d, float delta, float D, float Wp, float3 gC) {
  PlaneTerm r;
  r.t = ALPHA ? (1.0f - px.w) : __expf(-px.w * delta);
  const float w = Af * (1.0f - r.t);
  float3 c = make_float3(px.x, px.y, px.z);
  if (BLEND) {
    c.x = Af * I.x + (1.0f - Af) * c.x;
    c.y = Af * I.y + (1.0f - Af) * c.y;
    c.z = Af * I.z + (1.0f - Af) * c.z;
  }
  r.dcx = w * gR.x + gC.x;
  r.dcy = w * gR.y + gC.y;
  r.dcz = w * gR.z + gC.z;
  r.e = c.x * gR.x + c.y * gR.y + c.z * gR.z +
        gD * (ALPHA ? d : (BG_INF ? (d - 1000.0f) : (d - D) / Wp));
  float dA = (1.0f - r.t) * r.e;
  if (BLEND) {
    dA += (I.x - px.x) * r.dcx + (I.y - px.y) * r.dcy + (I.z - px.z) * r.dcz;
  }
  r.dA = dA;
  return r;
}

template <bool BLEND, bool BG_INF, bool ALPHA = false>
__global__ void __launch_bounds__(kBlock)
src_composite_bwd_kernel(const float* __restrict__ mpi,
                         const float* __restrict__ depths,
                         const float* __restrict__ kinv,
                         const float* __restrict__ img,
                         const float* __restrict__ g_rgb,    // (B,3,H,W) or null
                         const float* __restrict__ g_depth,  // (B,1,H,W) or null
                         const float* __restrict__ g_blend,  // (B,S,H,W,4) or null
                         float* __restrict__ grad_mpi,       // (B,S,H,W,4)
                         int B, int S, int H, int W) {
  __shared__ float s_depth[kMaxS];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < S; i += kBlock) s_depth[i] = depths[b * S + i];
  __syncthreads();

  float3x3 Ki;
#pragma unroll
  for (int i = 0; i < 9; ++i) Ki.m[i] = kinv[b * 9 + i];

  const int HW = H * W;
  const int64_t mpi_b = (int64_t)b * S * HW * 4;
  for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < HW;
       pix += gridDim.x * kBlock) {
    const int y = pix / W;
    const int x = pix - y * W;
    const float3 ray = Ki.mul((float)x, (float)y, 1.0f);
    const float nu = sqrtf(ray.x * ray.x + ray.y * ray.y + ray.z * ray.z);

    float3 I = make_float3(0.f, 0.f, 0.f);
    if (BLEND) {
      const float* ip = img + ((int64_t)b * HW + pix) * 3;
      I = make_float3(ip[0], ip[1], ip[2]);
    }
    float3 gR = make_float3(0.f, 0.f, 0.f);
    if (g_rgb) {
      gR.x = g_rgb[((int64_t)b * 3 + 0) * HW + pix];
      gR.y = g_rgb[((int64_t)b * 3 + 1) * HW + pix];
      gR.z = g_rgb[((int64_t)b * 3 + 2) * HW + pix];
    }
    const float gD = g_depth ? g_depth[(int64_t)b * HW + pix] : 0.0f;

    // ---- pass 1: composite totals ----
    float A = 1.0f, Wsum = 0.0f, Nsum = 0.0f;
    for (int s = 0; s < S; ++s) {
      const float4 px = *reinterpret_cast<const float4*>(
          mpi + mpi_b + ((int64_t)s * HW + pix) * 4);
      const float d = s_depth[s];
      const float delta = (s + 1 < S) ? nu * (s_depth[s + 1] - d) : 1e3f;
      const float t = ALPHA ? (1.0f - px.w) : __expf(-px.w * delta);
      const float w = A * (1.0f - t);
      Wsum += w;
      Nsum += w * d;
      A *= ALPHA ? t : (t + 1e-6f);
    }
    const float Wp = Wsum + 1e-5f;
    const float D = ALPHA ? Nsum
                          : (BG_INF ? (Nsum + 1000.0f * (1.0f - Wsum))
                                    : (Nsum / Wp));

    // ---- pass 2: total cumprod-suffix mass ----
    // fp64 transmittance + accumulators: pass 3 computes
    // (TotalP - prefix) / u with u ~ 1e-6. The shared-prefix terms of
    // the two fp64 sums must cancel EXACTLY, so both passes obtain the
    // per-plane term from the single noinline src_plane_term instance
    // (bitwise-identical values); fp32 term differences would leave
    // O(eps_f32 * |e|) residues which the divide amplifies by up to 1e6
    // (0.1-magnitude sigma-grad errors when the bg-inf depth term makes
    // |e| ~ 1e3).
    double TotalP = 0.0;
    double Ad = 1.0;
    for (int s = 0; s < S; ++s) {
      const float4 px = *reinterpret_cast<const float4*>(
          mpi + mpi_b + ((int64_t)s * HW + pix) * 4);
      const float d = s_depth[s];
      const float delta = (s + 1 < S) ? nu * (s_depth[s + 1] - d) : 1e3f;
      float3 gC = make_float3(0.f, 0.f, 0.f);
      if (BLEND && g_blend) {
        const float4 gb = *reinterpret_cast<const float4*>(
            g_blend + mpi_b + ((int64_t)s * HW + pix) * 4);
        gC = make_float3(gb.x, gb.y, gb.z);
      }
      const PlaneTerm pt = src_plane_term<BLEND, BG_INF, ALPHA>(
          px, (float)Ad, I, gR, gD, d, delta, D, Wp, gC);
      TotalP += (double)pt.dA * Ad;
      Ad *= (double)(ALPHA ? pt.t : (pt.t + 1e-6f));
      if (Ad < 1e-14) break;
    }

    // ---- pass 3: emit gradients ----
    double prefix = 0.0;
    Ad = 1.0;
    for (int s = 0; s < S; ++s) {
      const float4 px = *reinterpret_cast<const float4*>(
          mpi + mpi_b + ((int64_t)s * HW + pix) * 4);
      const float d = s_depth[s];
      const float delta = (s + 1 < S) ? nu * (s_depth[s + 1] - d) : 1e3f;
      float3 gC = make_float3(0.f, 0.f, 0.f);
      float gCs = 0.0f;
      if (BLEND && g_blend) {
        const float4 gb = *reinterpret_cast<const float4*>(
            g_blend + mpi_b + ((int64_t)s * HW + pix) * 4);
        gC = make_float3(gb.x, gb.y, gb.z);
        gCs = gb.w;
      }
      const float Af = (float)Ad;
      const PlaneTerm pt = src_plane_term<BLEND, BG_INF, ALPHA>(
          px, Af, I, gR, gD, d, delta, D, Wp, gC);
      const float u = ALPHA ? pt.t : (pt.t + 1e-6f);
      prefix += (double)pt.dA * Ad;
      const float dt = -Af * pt.e + (float)((TotalP - prefix) / (double)u);
      // alpha mode: d(t)/d(alpha) = -1; sigma mode: d(t)/d(sigma) = -delta*t
      const float dsigma = (ALPHA ? -dt : dt * (-delta * pt.t)) + gCs;
      float4 g;
      if (BLEND) {
        const float oneA = 1.0f - Af;
        g = make_float4(oneA * pt.dcx, oneA * pt.dcy, oneA * pt.dcz, dsigma);
      } else {
        g = make_float4(pt.dcx, pt.dcy, pt.dcz, dsigma);
      }
      *reinterpret_cast<float4*>(grad_mpi + mpi_b + ((int64_t)s * HW + pix) * 4) = g;
      Ad *= (double)u;
      if (Ad < 1e-14) {
        // tail: w ~ 0, A ~ 0 -> drgb = dc ~= gC, dsigma = gCs (blend
        // pass-through); zeros without blend. grad_mpi is at::empty.
        for (int s2 = s + 1; s2 < S; ++s2) {
          const int64_t o = mpi_b + ((int64_t)s2 * HW + pix) * 4;
          float4 gt = make_float4(0.f, 0.f, 0.f, 0.f);
          if (BLEND && g_blend) {
            gt = *reinterpret_cast<const float4*>(g_blend + o);
          }
          *reinterpret_cast<float4*>(grad_mpi + o) = gt;
        }
        break;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Novel-view render: homography warp + z-cull + composite, fully fused
// ---------------------------------------------------------------------------
// Per (b,s) geometry staged in LDS: Hinv (tgt pixel -> src homogeneous,
// 9 f32) and plane depth. M = R_tgt_src * K_src_inv and t give the warped
// plane point analytically: v_s(p) = M * qhat_s(p) * d_s + t, where
// qhat_s = (clamped src pixel, 1). ref operations/homography_sampler.py +
// mpi_rendering.py:181-241.

struct TapRef {
  int x0, x1, y0, y1;
  float wx, wy;  // fractional weights toward x1 / y1
  bool interior; // no border clamping: u in [0, W-1], v in [0, H-1]
};

DEV TapRef make_tap(float u, float v, int W, int H) {
  TapRef t;
  const float uc = clampf(u, 0.0f, (float)(W - 1));
  const float vc = clampf(v, 0.0f, (float)(H - 1));
  const float fx = floorf(uc), fy = floorf(vc);
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  t.x1 = min(t.x0 + 1, W - 1);
  t.y1 = min(t.y0 + 1, H - 1);
  t.wx = uc - fx;
  t.wy = vc - fy;
  t.interior = (u == uc) && (v == vc);
  return t;
}

// CONTRACTION RULE. The per-plane functions below (project_uv,
// bilinear4, sample_plane, plane_delta, tgt_plane_terms) are inlined
// into several contexts that must see BITWISE-identical values:
//  * pass A and pass B of the backward telescope fp64 sums of the same
//    fp32 terms against each other and divide the residue by u ~ 1e-6;
//    a last-bit difference in a term becomes an O(0.1) sigma gradient;
//  * the backward kernel and the gather kernel classify taps from the
//    same (u, v); a different rounding flips a floor()/interior decision
//    at an integer boundary and silently drops one pixel's gradient.
// The compiler decides FMA contraction per inlining context, so each of
// these functions switches it off for its own body and writes every
// fused operation as an explicit fmaf. What is fused is then fixed in
// the source, and no call, scratch or out-parameter is needed to pin
// it. A helper called from them must follow the same rule or hold no
// contractible expression (clampf, make_tap).
DEV float2 project_uv(const float* Hrow, int x, int y) {
#pragma clang fp contract(off)
  const float fx = (float)x, fy = (float)y;
  const float hx = fmaf(Hrow[0], fx, fmaf(Hrow[1], fy, Hrow[2]));
  const float hy = fmaf(Hrow[3], fx, fmaf(Hrow[4], fy, Hrow[5]));
  const float hz = fmaf(Hrow[6], fx, fmaf(Hrow[7], fy, Hrow[8]));
  const float iz = 1.0f / hz;
  return make_float2(hx * iz, hy * iz);
}

// no border clamping: u in [0, W-1], v in [0, H-1] (TapRef::interior)
DEV bool uv_interior(float u, float v, int W, int H) {
  return (u == clampf(u, 0.0f, (float)(W - 1))) &&
         (v == clampf(v, 0.0f, (float)(H - 1)));
}

// `base` is one plane (wave-uniform); the tap offsets are 32-bit (the
// bindings check H*W*4 < 2^31), so the loads address as uniform base +
// per-lane offset and hold no 64-bit pointers in vector registers.
DEV float4 bilinear4(const float* base, const TapRef& t, int W) {
#pragma clang fp contract(off)
  const float4 p00 = *reinterpret_cast<const float4*>(base + (unsigned)(t.y0 * W + t.x0) * 4u);
  const float4 p01 = *reinterpret_cast<const float4*>(base + (unsigned)(t.y0 * W + t.x1) * 4u);
  const float4 p10 = *reinterpret_cast<const float4*>(base + (unsigned)(t.y1 * W + t.x0) * 4u);
  const float4 p11 = *reinterpret_cast<const float4*>(base + (unsigned)(t.y1 * W + t.x1) * 4u);
  const float w00 = (1 - t.wx) * (1 - t.wy), w01 = t.wx * (1 - t.wy);
  const float w10 = (1 - t.wx) * t.wy, w11 = t.wx * t.wy;
#define BL(C) fmaf(w11, p11.C, fmaf(w10, p10.C, fmaf(w01, p01.C, w00 * p00.C)))
  return make_float4(BL(x), BL(y), BL(z), BL(w));
#undef BL
}

// One plane's warped sample: rgb+sigma (z-culled), analytic point,
// validity, and the projected (u, v) the taps were made from (pass B
// rebuilds the TapRef from them where it scatters).
struct PlaneSample {
  float4 rgbs;
  float3 v;
  float inb;
  float pu, pv;
};

DEV PlaneSample sample_plane(const float* mpi_b, int s, int HW,
                             const float* s_geom, float d,
                             const float3x3& M, float3 tv,
                             int x, int y, int W, int H) {
#pragma clang fp contract(off)
  const float2 uv = project_uv(s_geom + s * 9, x, y);
  const float u = uv.x, v = uv.y;

  PlaneSample ps;
  ps.pu = u;
  ps.pv = v;
  ps.inb = (u > -1.0f && u < (float)W && v > -1.0f && v < (float)H) ? 1.0f : 0.0f;

  const TapRef tap = make_tap(u, v, W, H);
  ps.rgbs = bilinear4(mpi_b + (int64_t)s * HW * 4, tap, W);

  const float ucl = clampf(u, 0.0f, (float)(W - 1));
  const float vcl = clampf(v, 0.0f, (float)(H - 1));
  const float rx = fmaf(M.m[0], ucl, fmaf(M.m[1], vcl, M.m[2]));
  const float ry = fmaf(M.m[3], ucl, fmaf(M.m[4], vcl, M.m[5]));
  const float rz = fmaf(M.m[6], ucl, fmaf(M.m[7], vcl, M.m[8]));
  ps.v = make_float3(fmaf(rx, d, tv.x), fmaf(ry, d, tv.y), fmaf(rz, d, tv.z));
  if (ps.v.z < 0.0f) ps.rgbs.w = 0.0f;  // z-cull (ref mpi_rendering.py:233-235)
  return ps;
}

// Inter-plane distance of two warped plane points (contraction rule).
DEV float plane_delta(float3 a, float3 b) {
#pragma clang fp contract(off)
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

template <bool BG_INF, bool ALPHA = false>
__global__ void __launch_bounds__(kBlock)
tgt_composite_fwd_kernel(const float* __restrict__ mpi,     // (Bm,S,H,W,4)
                         const float* __restrict__ hinv,    // (R,S,3,3)
                         const float* __restrict__ m_rki,   // (R,3,3)
                         const float* __restrict__ tvec,    // (R,3)
                         const float* __restrict__ depths,  // (Bm,S)
                         float* __restrict__ rgb_out,       // (R,3,H,W)
                         float* __restrict__ depth_out,     // (R,1,H,W)
                         float* __restrict__ mask_out,      // (R,1,H,W)
                         int Bm, int S, int H, int W) {
  __shared__ float s_geom[kMaxS * 9];
  __shared__ float s_depth[kMaxS];
  // VIEW ROWS. The grid has R = gridDim.y rows. Row b takes its geometry
  // and writes its outputs at index b; it reads the MPI and the plane
  // depths of batch element b % Bm, Bm being the MPI batch count. Single
  // view: R == Bm. View-batched: R = V * Bm rows, view-major, so V
  // cameras read one MPI.
  const int b = blockIdx.y;
  const int bm = b % Bm;
  for (int i = threadIdx.x; i < S * 9; i += kBlock) s_geom[i] = hinv[(int64_t)b * S * 9 + i];
  for (int i = threadIdx.x; i < S; i += kBlock) s_depth[i] = depths[bm * S + i];
  __syncthreads();

  float3x3 M;
#pragma unroll
  for (int i = 0; i < 9; ++i) M.m[i] = m_rki[b * 9 + i];
  const float3 tv = make_float3(tvec[b * 3], tvec[b * 3 + 1], tvec[b * 3 + 2]);

  const int HW = H * W;
  const float* mpi_b = mpi + (int64_t)bm * S * HW * 4;
  for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < HW;
       pix += gridDim.x * kBlock) {
    const int y = pix / W;
    const int x = pix - y * W;

    float A = 1.0f, Wsum = 0.0f, Nsum = 0.0f, mask = 0.0f;
    float3 R = make_float3(0.f, 0.f, 0.f);

    PlaneSample cur = sample_plane(mpi_b, 0, HW, s_geom, s_depth[0], M, tv,
                                   x, y, W, H);
    mask += cur.inb;
    int s = 0;
    for (; s < S; ++s) {
      float delta;
      PlaneSample nxt;
      if (s + 1 < S) {
        nxt = sample_plane(mpi_b, s + 1, HW, s_geom, s_depth[s + 1], M, tv,
                           x, y, W, H);
        mask += nxt.inb;
        delta = plane_delta(cur.v, nxt.v);
      } else {
        delta = 1e3f;
      }
      const float t = ALPHA ? (1.0f - cur.rgbs.w)
                            : __expf(-cur.rgbs.w * delta);
      const float w = A * (1.0f - t);
      R.x += w * cur.rgbs.x; R.y += w * cur.rgbs.y; R.z += w * cur.rgbs.z;
      Wsum += w;
      Nsum += w * cur.v.z;
      A *= ALPHA ? t : (t + 1e-6f);
      cur = nxt;
      if (A < 1e-14f) {  // transmittance dead: remaining planes add ~0
        ++s;
        break;
      }
    }
    // mask still counts EVERY plane's validity (ref mpi_rendering.py:239):
    // projection-only tail, no MPI gathers
    for (int s2 = s + 1; s2 < S; ++s2) {
      const float2 uv = project_uv(s_geom + s2 * 9, x, y);
      const float u = uv.x, v = uv.y;
      mask += (u > -1.0f && u < (float)W && v > -1.0f && v < (float)H)
                  ? 1.0f : 0.0f;
    }
    const float D = ALPHA ? Nsum
                          : (BG_INF ? (Nsum + 1000.0f * (1.0f - Wsum))
                                    : (Nsum / (Wsum + 1e-5f)));
    rgb_out[((int64_t)b * 3 + 0) * HW + pix] = R.x;
    rgb_out[((int64_t)b * 3 + 1) * HW + pix] = R.y;
    rgb_out[((int64_t)b * 3 + 2) * HW + pix] = R.z;
    depth_out[(int64_t)b * HW + pix] = D;
    mask_out[(int64_t)b * HW + pix] = mask;
  }
}

DEV void scatter4(float* base, const TapRef& t, int W, float4 g) {
  const float w00 = (1 - t.wx) * (1 - t.wy), w01 = t.wx * (1 - t.wy);
  const float w10 = (1 - t.wx) * t.wy, w11 = t.wx * t.wy;
  float* p00 = base + (unsigned)(t.y0 * W + t.x0) * 4u;
  float* p01 = base + (unsigned)(t.y0 * W + t.x1) * 4u;
  float* p10 = base + (unsigned)(t.y1 * W + t.x0) * 4u;
  float* p11 = base + (unsigned)(t.y1 * W + t.x1) * 4u;
#define SC(P, WGT)                                  \
  if (WGT != 0.0f) {                                \
    atomicAdd(P + 0, WGT * g.x);                    \
    atomicAdd(P + 1, WGT * g.y);                    \
    atomicAdd(P + 2, WGT * g.z);                    \
    atomicAdd(P + 3, WGT * g.w);                    \
  }
  SC(p00, w00) SC(p01, w01) SC(p10, w10) SC(p11, w11)
#undef SC
}

// Per-plane backward components for the tgt kernel. e depends on the
// composite totals (D, Wsum) which are only known after a full pass, but
// it is LINEAR in them: e = r + qv*vz + qc with pass-independent
// r = rgb.gR. The suffix sums therefore split into three component sums
// (cr, cv, cw) accumulated WITHOUT D, and the /u-amplified telescoping
// stays exact per component because both passes get bitwise-identical
// terms (contraction rule above).
struct TgtTerm {
  float t, r, cr, cv, cw;
};

template <bool ALPHA>
DEV TgtTerm tgt_plane_terms(float4 rgbs, float vz, float delta, float3 gR) {
#pragma clang fp contract(off)
  TgtTerm o;
  o.t = ALPHA ? (1.0f - rgbs.w) : __expf(-rgbs.w * delta);
  o.r = fmaf(rgbs.z, gR.z, fmaf(rgbs.y, gR.y, rgbs.x * gR.x));
  const float omt = 1.0f - o.t;
  o.cr = omt * o.r;
  o.cv = omt * vz;
  o.cw = omt;
  return o;
}

// GATHER mode (the round-2 redesign, docs/NEXT.md 2 / VERDICT item 3):
// interior target pixels write their per-plane gradient as a PLAIN
// coalesced float4 into `payload` (B,S,H,W,4) instead of a 16-atomic
// bilinear scatter; only border-clamped pixels (a thin ring per plane)
// take the atomic path. `payload` needs no zero fill: the kernel writes
// every entry, zeros where a pixel is border-clamped or lies behind the
// dead-transmittance break. tgt_gather_kernel then inverts the
// map per source tile. Decomposition proven against the scatter form
// in tests/test_kernel_sim.py::test_warp_backward_gather_decomposition.
//
// EMIT mode (the order-fixed backward, mode 2 of the launcher): EVERY
// target pixel, border-clamped ones included, writes its per-plane
// gradient into `payload` (zeros behind the dead-transmittance break),
// nothing is scattered and grad_mpi is never touched. tgt_collect_kernel
// then pulls the payload into grad_mpi in a fixed order.
enum TgtBwdMode : int { kTgtScatter = 0, kTgtGather = 1, kTgtEmit = 2 };

template <bool BG_INF, int MODE, bool ALPHA = false>
__global__ void __launch_bounds__(kBlock)
tgt_composite_bwd_kernel(const float* __restrict__ mpi,
                         const float* __restrict__ hinv,
                         const float* __restrict__ m_rki,
                         const float* __restrict__ tvec,
                         const float* __restrict__ depths,
                         const float* __restrict__ g_rgb,
                         const float* __restrict__ g_depth,
                         float* __restrict__ grad_mpi,  // pre-zeroed; unused (EMIT)
                         float* __restrict__ payload,   // fully written (GATHER, EMIT)
                         int B, int S, int H, int W) {
  constexpr bool GATHER = MODE == kTgtGather;
  constexpr bool EMIT = MODE == kTgtEmit;
  constexpr bool PAYLOAD = GATHER || EMIT;
  __shared__ float s_geom[kMaxS * 9];
  __shared__ float s_depth[kMaxS];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < S * 9; i += kBlock) s_geom[i] = hinv[(int64_t)b * S * 9 + i];
  for (int i = threadIdx.x; i < S; i += kBlock) s_depth[i] = depths[b * S + i];
  __syncthreads();

  float3x3 M;
#pragma unroll
  for (int i = 0; i < 9; ++i) M.m[i] = m_rki[b * 9 + i];
  const float3 tv = make_float3(tvec[b * 3], tvec[b * 3 + 1], tvec[b * 3 + 2]);

  const int HW = H * W;
  const float* mpi_b = mpi + (int64_t)b * S * HW * 4;
  float* gm_b = EMIT ? nullptr : grad_mpi + (int64_t)b * S * HW * 4;
  for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < HW;
       pix += gridDim.x * kBlock) {
    const int y = pix / W;
    const int x = pix - y * W;

    float3 gR = make_float3(0.f, 0.f, 0.f);
    if (g_rgb) {
      gR.x = g_rgb[((int64_t)b * 3 + 0) * HW + pix];
      gR.y = g_rgb[((int64_t)b * 3 + 1) * HW + pix];
      gR.z = g_rgb[((int64_t)b * 3 + 2) * HW + pix];
    }
    const float gD = g_depth ? g_depth[(int64_t)b * HW + pix] : 0.0f;

    // ---- pass A: composite totals + D-independent suffix components ----
    float A = 1.0f, Wsum = 0.0f, Nsum = 0.0f;
    double TaR = 0.0, TaV = 0.0, TaW = 0.0;
    double Ad = 1.0;
    PlaneSample cur = sample_plane(mpi_b, 0, HW, s_geom, s_depth[0], M, tv,
                                   x, y, W, H);
    for (int s = 0; s < S; ++s) {
      float delta;
      PlaneSample nxt;
      if (s + 1 < S) {
        nxt = sample_plane(mpi_b, s + 1, HW, s_geom, s_depth[s + 1], M, tv,
                           x, y, W, H);
        delta = plane_delta(cur.v, nxt.v);
      } else {
        delta = 1e3f;
      }
      const TgtTerm tt = tgt_plane_terms<ALPHA>(cur.rgbs, cur.v.z, delta,
                                                gR);
      const float w = A * (1.0f - tt.t);
      Wsum += w;
      Nsum += w * cur.v.z;
      TaR += (double)tt.cr * Ad;
      TaV += (double)tt.cv * Ad;
      TaW += (double)tt.cw * Ad;
      A *= ALPHA ? tt.t : (tt.t + 1e-6f);
      Ad *= (double)(ALPHA ? tt.t : (tt.t + 1e-6f));
      cur = nxt;
      if (Ad < 1e-14) break;  // dead transmittance: tail adds ~0
    }
    const float Wp = Wsum + 1e-5f;
    const float D = BG_INF ? (Nsum + 1000.0f * (1.0f - Wsum)) : (Nsum / Wp);
    // e = r + qv*vz + qc (alpha: plain weighted z sum -> qv = gD, qc = 0)
    const float qv = ALPHA ? gD : (BG_INF ? gD : gD / Wp);
    const float qc = ALPHA ? 0.0f
                           : (BG_INF ? (-1000.0f * gD) : (-gD / Wp * D));

    // ---- pass B: emit gradients, bilinear scatter ----
    double prR = 0.0, prV = 0.0, prW = 0.0;
    Ad = 1.0;
    float* pay_b = PAYLOAD ? payload + (int64_t)b * S * HW * 4 : nullptr;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    cur = sample_plane(mpi_b, 0, HW, s_geom, s_depth[0], M, tv, x, y, W, H);
    int s = 0;
    for (; s < S; ++s) {
      float delta;
      PlaneSample nxt;
      if (s + 1 < S) {
        nxt = sample_plane(mpi_b, s + 1, HW, s_geom, s_depth[s + 1], M, tv,
                           x, y, W, H);
        delta = plane_delta(cur.v, nxt.v);
      } else {
        delta = 1e3f;
      }
      const TgtTerm tt = tgt_plane_terms<ALPHA>(cur.rgbs, cur.v.z, delta,
                                                gR);
      const float t = tt.t;
      const float u = ALPHA ? t : (t + 1e-6f);
      const float Af = (float)Ad;
      const float w = Af * (1.0f - t);
      prR += (double)tt.cr * Ad;
      prV += (double)tt.cv * Ad;
      prW += (double)tt.cw * Ad;
      // per-component exact telescoping, recombined with the (qv, qc)
      // coefficients in fp64
      const double suffix = (TaR - prR) + (double)qv * (TaV - prV) +
                            (double)qc * (TaW - prW);
      const float e = tt.r + qv * cur.v.z + qc;
      // the exactness requirement is on the fp64 subtractions; dividing
      // the converted residue by u in fp32 is well conditioned
      const float dt = -Af * e + (float)suffix / u;
      // culled sigma/alpha contributed nothing -> no gradient through it
      const float dsigma = (cur.v.z < 0.0f)
          ? 0.0f : (ALPHA ? -dt : dt * (-delta * t));
      const float4 g = make_float4(w * gR.x, w * gR.y, w * gR.z, dsigma);
      // payload is NOT pre-zeroed: this thread writes every (s, pix)
      // entry it owns — g where the taps are interior, zeros where the
      // pixel goes through the atomic border path instead (EMIT has no
      // such path: every pixel's g goes into the payload)
      const bool interior =
          EMIT || (GATHER && uv_interior(cur.pu, cur.pv, W, H));
      if (PAYLOAD) {
        // per-component selects: a select between two float4 objects
        // goes through scratch
        *reinterpret_cast<float4*>(pay_b + (int64_t)s * HW * 4 +
                                   (unsigned)pix * 4u) =
            make_float4(interior ? g.x : 0.f, interior ? g.y : 0.f,
                        interior ? g.z : 0.f, interior ? g.w : 0.f);
      }
      if (!EMIT && !interior) {
        scatter4(gm_b + (int64_t)s * HW * 4,
                 make_tap(cur.pu, cur.pv, W, H), W, g);
      }
      Ad *= (double)u;
      cur = nxt;
      // grad_mpi is pre-zeroed; dead-transmittance tail scatters ~0
      if (Ad < 1e-14) break;
    }
    if (PAYLOAD) {  // ... and zeros for the planes behind the break
      for (int s2 = s + 1; s2 < S; ++s2) {
        *reinterpret_cast<float4*>(pay_b + (int64_t)s2 * HW * 4 +
                                   (unsigned)pix * 4u) = zero4;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Gather pass of the tgt backward: per (b, s, 32x32 src tile), invert
// the homography to find the contributing interior tgt pixels, bilinear-
// accumulate their payloads into an LDS tile, flush with PLAIN float4
// adds (each src pixel belongs to exactly one tile, and the scatter
// pass has already completed — no concurrent writers).
// ---------------------------------------------------------------------------

// Plain LDS add of an already rounded addend: with contraction off the
// caller's product cannot fuse into the add, so this path adds the same
// fp32 addends as the atomic one.
DEV void lds_add(float* p, float v) {
#pragma clang fp contract(off)
  *p = *p + v;
}

constexpr int GT = 32;      // gather tile side
constexpr int kGBlock = 64; // ONE wave per tile, see below
constexpr int kGRows = 4;   // payload rows the wave keeps in flight

// The wave takes bbox rows and its lanes take x (no integer division per
// pixel); it issues the loads of kGRows rows before it processes them.
//
// LDS float atomics are what this kernel used to spend its time on
// (profiles/r09_warp_bwd.md: 1.98 ms with them, 0.25 ms with plain adds in
// their place, same loads and arithmetic). So a tile belongs to ONE wave,
// and a row of target pixels adds its taps with plain LDS read-add-write
// wherever no two lanes of one instruction can hit the same address:
//  * one instruction handles one tap kind ((x0,y0), (x1,y0), ...) of the
//    even or of the odd lanes, so two of its lanes collide only if they
//    have the same (x0, y0) and are an even number of lanes apart;
//  * the row qualifies if x0 and y0 are each weakly monotone over the
//    lanes of the chunk and, within every run of neighbouring lanes that
//    share one (x0, y0), at most one even and one odd lane add anything.
//    Two lanes i < j with one (x0, y0) squeeze every lane between them
//    onto the same (x0, y0), so they lie in one run, which the check
//    covers; lanes that add nothing (border-clamped, zero payload) do
//    not disqualify a row. Along an image row a homography moves u and v
//    monotonically, so rows fail only where the map shrinks below half a
//    source pixel per target pixel or where rounding makes y0 flicker;
//    those rows keep the atomics.
//  * instructions of one wave reach the LDS in order, and nobody else
//    touches the tile; a wavefront fence between the tap kinds keeps the
//    compiler from reordering their read-add-writes.
// The tile is channel-planar (four GT*GT planes): x-adjacent lanes map to
// x-adjacent source taps, so a channel's adds fall on consecutive banks.
__global__ void __launch_bounds__(kGBlock)
tgt_gather_kernel(const float* __restrict__ payload,  // (B,S,H,W,4)
                  const float* __restrict__ hinv,     // (B,S,3,3) tgt->src
                  const float* __restrict__ hfwd,     // (B,S,3,3) src->tgt
                  float* __restrict__ grad_mpi,       // += (B,S,H,W,4)
                  int B, int S, int H, int W, int tiles_x) {
  __shared__ float s_acc[4 * GT * GT];  // [channel][qy][qx]
  __shared__ float s_Hi[9];
  __shared__ float s_Hf[9];
  const int tile = blockIdx.x;
  const int s = blockIdx.y;
  const int b = blockIdx.z;
  const int tx0 = (tile % tiles_x) * GT;
  const int ty0 = (tile / tiles_x) * GT;
  const int tid = threadIdx.x;

  for (int i = tid; i < GT * GT * 4; i += kGBlock) s_acc[i] = 0.0f;
  if (tid < 9) {
    s_Hi[tid] = hinv[((int64_t)b * S + s) * 9 + tid];
    s_Hf[tid] = hfwd[((int64_t)b * S + s) * 9 + tid];
  }
  __syncthreads();

  // ---- bbox: preimage of the (tile + 1px tap halo) under the forward
  // homography. The preimage of a convex region is convex, so the bbox
  // of the 4 mapped corners bounds it exactly; a non-positive or
  // non-finite depth at any corner (horizon crossing / degenerate
  // plane) falls back to the whole image — slower, never wrong.
  float bx0 = 0.f, by0 = 0.f, bx1 = (float)(W - 1), by1 = (float)(H - 1);
  {
    const float cx[2] = {(float)tx0 - 1.25f, (float)(tx0 + GT) + 0.25f};
    const float cy[2] = {(float)ty0 - 1.25f, (float)(ty0 + GT) + 0.25f};
    float mnx = 1e30f, mny = 1e30f, mxx = -1e30f, mxy = -1e30f;
    bool ok = true;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const float x = cx[ci & 1], y = cy[ci >> 1];
      const float qz = s_Hf[6] * x + s_Hf[7] * y + s_Hf[8];
      const float qx = (s_Hf[0] * x + s_Hf[1] * y + s_Hf[2]) / qz;
      const float qy = (s_Hf[3] * x + s_Hf[4] * y + s_Hf[5]) / qz;
      ok = ok && (qz > 1e-8f) && isfinite(qx) && isfinite(qy);
      mnx = fminf(mnx, qx); mny = fminf(mny, qy);
      mxx = fmaxf(mxx, qx); mxy = fmaxf(mxy, qy);
    }
    if (ok) {
      bx0 = fmaxf(0.f, floorf(mnx - 1.0f));
      by0 = fmaxf(0.f, floorf(mny - 1.0f));
      bx1 = fminf((float)(W - 1), ceilf(mxx + 1.0f));
      by1 = fminf((float)(H - 1), ceilf(mxy + 1.0f));
    }
  }
  const int px0 = (int)bx0, py0 = (int)by0;
  const int bw = (int)bx1 - px0 + 1, bh = (int)by1 - py0 + 1;
  const int HW = H * W;
  const float* pay_b = payload + ((int64_t)b * S + s) * HW * 4;

  if (bw > 0 && bh > 0) {
    const int lane = tid;
    for (int r0 = 0; r0 < bh; r0 += kGRows) {
      for (int c0 = 0; c0 < bw; c0 += 64) {
        const int cx = c0 + lane;
        const bool in_chunk = cx < bw;
        const int px = px0 + cx;  // <= W - 1 where in_chunk
        float4 g[kGRows];
#pragma unroll
        for (int k = 0; k < kGRows; ++k) {
          g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (in_chunk && r0 + k < bh) {  // py0 + r0 + k <= H - 1
            g[k] = *reinterpret_cast<const float4*>(
                pay_b + (unsigned)((py0 + r0 + k) * W + px) * 4u);
          }
        }
#pragma unroll
        for (int k = 0; k < kGRows; ++k) {
          if (r0 + k >= bh) break;  // wave-uniform
          const float4 gk = g[k];
          const int py = py0 + r0 + k;
          // every lane projects, also where it adds nothing: the row's
          // monotonicity is judged on all lanes of the chunk
          const float2 uv = project_uv(s_Hi, px, py);
          const TapRef t = make_tap(uv.x, uv.y, W, H);
          // the backward kernel writes zeros for non-interior pixels,
          // but re-derive and skip just in case (bitwise-identical
          // classification: contraction rule of project_uv)
          const bool adds = in_chunk &&
              !(gk.x == 0.f && gk.y == 0.f && gk.z == 0.f && gk.w == 0.f) &&
              uv_interior(uv.x, uv.y, W, H);
          if (!__any(adds)) continue;  // wave-uniform

          const int x0l = __shfl_up(t.x0, 1), y0l = __shfl_up(t.y0, 1);
          const bool has_l = in_chunk && lane >= 1;  // left one in_chunk too
          const bool mono_x = __all(!has_l || t.x0 >= x0l) ||
                              __all(!has_l || t.x0 <= x0l);
          const bool mono_y = __all(!has_l || t.y0 >= y0l) ||
                              __all(!has_l || t.y0 <= y0l);
          // runs of lanes with one (x0, y0): a lane collides if an adding
          // lane of its parity sits to its left in its own run
          const unsigned long long starts =
              __ballot(!(has_l && t.x0 == x0l && t.y0 == y0l));
          const unsigned long long addm = __ballot(adds);
          const unsigned long long upto = (2ull << lane) - 1ull;  // 0..lane
          const int start = 63 - __clzll((long long)(starts & upto));
          const unsigned long long left =
              (upto >> 1) & ~((1ull << start) - 1ull);  // start..lane-1
          const unsigned long long par = (lane & 1) ? 0xAAAAAAAAAAAAAAAAull
                                                    : 0x5555555555555555ull;
          const bool no_dup = __all(!(adds && (addm & left & par) != 0ull));
          const bool plain = mono_x && mono_y && no_dup;  // wave-uniform

          const float w00 = (1 - t.wx) * (1 - t.wy), w01 = t.wx * (1 - t.wy);
          const float w10 = (1 - t.wx) * t.wy, w11 = t.wx * t.wy;
#define GSC(ADD, QX, QY, WGT)                                         \
          if (WGT != 0.0f && (QX) >= tx0 && (QX) < tx0 + GT &&        \
              (QY) >= ty0 && (QY) < ty0 + GT) {                       \
            float* a = s_acc + ((QY) - ty0) * GT + ((QX) - tx0);      \
            ADD(a + 0 * GT * GT, WGT * gk.x);                         \
            ADD(a + 1 * GT * GT, WGT * gk.y);                         \
            ADD(a + 2 * GT * GT, WGT * gk.z);                         \
            ADD(a + 3 * GT * GT, WGT * gk.w);                         \
          }
#define GSC4(ADD)                                                     \
          GSC(ADD, t.x0, t.y0, w00) TAP_ORDER                         \
          GSC(ADD, t.x1, t.y0, w01) TAP_ORDER                         \
          GSC(ADD, t.x0, t.y1, w10) TAP_ORDER                         \
          GSC(ADD, t.x1, t.y1, w11)
          // one lane's tap may be the cell of another lane's other tap
          // kind: keep the kinds' read-add-writes in program order
#define TAP_ORDER                                                     \
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      \
          __builtin_amdgcn_wave_barrier();
#define ADD_PLAIN(P, V) lds_add((P), (V))
#define ADD_ATOMIC(P, V) atomicAdd((P), (V))
          if (plain) {
            if (adds && (lane & 1) == 0) { GSC4(ADD_PLAIN) }
            // keeps the two halves two instruction streams: without it
            // merging the identical bodies would be a legal transform
            TAP_ORDER
            if (adds && (lane & 1) == 1) { GSC4(ADD_PLAIN) }
          } else if (adds) {
            GSC4(ADD_ATOMIC)
          }
#undef ADD_ATOMIC
#undef ADD_PLAIN
#undef TAP_ORDER
#undef GSC4
#undef GSC
        }
      }
    }
  }
  __syncthreads();

  // ---- flush: plain read-add-write float4 (no concurrent writers) ----
  float* gm = grad_mpi + ((int64_t)b * S + s) * HW * 4;
  for (int i = tid; i < GT * GT; i += kGBlock) {
    const int qx = tx0 + (i & (GT - 1));
    const int qy = ty0 + i / GT;
    if (qx >= W || qy >= H) continue;
    const float4 a = make_float4(s_acc[i], s_acc[GT * GT + i],
                                 s_acc[2 * GT * GT + i],
                                 s_acc[3 * GT * GT + i]);
    if (a.x == 0.f && a.y == 0.f && a.z == 0.f && a.w == 0.f) continue;
    float4* dst = reinterpret_cast<float4*>(gm + ((int64_t)qy * W + qx) * 4);
    float4 cur = *dst;
    cur.x += a.x; cur.y += a.y; cur.z += a.z; cur.w += a.w;
    *dst = cur;
  }
}


// ---------------------------------------------------------------------------
// Collect pass of the order-fixed tgt backward (mode 2): a pull kernel
// with no float atomic, global or LDS. Each source texel (b, s, qy, qx)
// has ONE owner thread, which sums the contributions of all target
// pixels whose taps hit it — target pixels in raster order (y, then x),
// tap kinds in scatter4's order — and writes grad_mpi with a plain
// store, zeros included (grad_mpi needs no zero fill). The order is a
// function of the shapes and the geometry alone.
//
// ACCUM is the form of the view-batched backward for every view after the
// first: the owner's sum is formed exactly as above and then
// grad_mpi = grad_mpi + sum in one plain read-add-write by the owner, so
// V stream-ordered launches leave ((g_0 + g_1) + g_2) ... bit for bit.
//
// MEMBERSHIP is decided exactly as the scatter decides it: make_tap of
// project_uv on the same hinv row (contraction rule); a tap contributes
// if it equals (qx, qy) and its weight is non-zero. Nothing else
// decides membership.
//
// The search WINDOW is only a bound and errs on the wide side. A pixel
// can reach the texel only if its clamped (u, v) lies in
// (qx-1, qx+1) x (qy-1, qy+1); for a ring texel (qx == 0, qx == W-1,
// qy == 0, qy == H-1) the outward condition is dropped, which is where
// the border-clamped pixels arrive (a strip for an edge texel, up to a
// quadrant for a corner). Where hz keeps one sign s over a target row,
// u > k is s * ((h0 - k h6) x + (h1 - k h7) y + (h2 - k h8)) > 0, linear
// in x, so every condition cuts the row to a half-line and the row
// holds one candidate interval. The fp32 (u, v) of project_uv differ
// from the exact ones by a few ulp of the terms; every condition is
// therefore relaxed by m = 1e-5 * (sum of the term magnitudes), more
// than a hundred times that error, and the interval is widened by one
// pixel on each side. A row on which hz is not safely of one sign, or a
// plane with a non-finite entry, scans the whole row: slower, never
// wrong (the rule of tgt_gather_kernel). Interior texels bound their
// rows with the four hfwd-mapped corners of their tap halo, again as
// the gather kernel does; ring texels visit every row, most of which
// come out empty in closed form.
// ---------------------------------------------------------------------------

// One condition s*(a x + c) > 0 relaxed by m, applied to the inclusive
// candidate interval [lo, hi] of a row (x in [0, W-1]); widened by one
// pixel. Returns false if the row holds no candidate at all.
DEV bool clip_row(float a, float c, float m, int W, int& lo, int& hi) {
  const float tiny = m / (float)W;  // |a| x stays below m over the row
  if (a > tiny) {          // x > xb
    const float xb = (-m - c) / a;
    lo = max(lo, (int)clampf(floorf(xb), -1.0f, (float)W));
  } else if (a < -tiny) {  // x < xb
    const float xb = (-m - c) / a;
    hi = min(hi, (int)clampf(ceilf(xb), -1.0f, (float)W));
  } else if (c <= -2.0f * m) {
    return false;          // a x + c <= -m on the whole row
  }
  return lo <= hi;
}

DEV void collect_tap(float4& acc, float w, float4 g) {
#pragma clang fp contract(off)
  // the addends of scatter4: the product is rounded, then added
  acc.x = acc.x + w * g.x;
  acc.y = acc.y + w * g.y;
  acc.z = acc.z + w * g.z;
  acc.w = acc.w + w * g.w;
}

template <bool ACCUM>
__global__ void __launch_bounds__(kBlock)
tgt_collect_kernel(const float* __restrict__ payload,  // (B,S,H,W,4)
                   const float* __restrict__ hinv,     // (B,S,3,3) tgt->src
                   const float* __restrict__ hfwd,     // (B,S,3,3) src->tgt
                   float* __restrict__ grad_mpi,       // (B,S,H,W,4), stored
                   int B, int S, int H, int W) {
  __shared__ float s_Hi[9];
  __shared__ float s_Hf[9];
  const int s = blockIdx.y;
  const int b = blockIdx.z;
  if (threadIdx.x < 9) {
    s_Hi[threadIdx.x] = hinv[((int64_t)b * S + s) * 9 + threadIdx.x];
    s_Hf[threadIdx.x] = hfwd[((int64_t)b * S + s) * 9 + threadIdx.x];
  }
  __syncthreads();

  const float fW1 = (float)(W - 1), fH1 = (float)(H - 1);
  // term magnitudes of hx, hy, hz over the image (the relaxation scale)
  const float Tx = fabsf(s_Hi[0]) * fW1 + fabsf(s_Hi[1]) * fH1 + fabsf(s_Hi[2]);
  const float Ty = fabsf(s_Hi[3]) * fW1 + fabsf(s_Hi[4]) * fH1 + fabsf(s_Hi[5]);
  const float Tz = fabsf(s_Hi[6]) * fW1 + fabsf(s_Hi[7]) * fH1 + fabsf(s_Hi[8]);
  const bool finite = isfinite(Tx + Ty + Tz);
  const float mz = 1e-5f * Tz;

  const int HW = H * W;
  const float* pay = payload + ((int64_t)b * S + s) * HW * 4;
  float* gm = grad_mpi + ((int64_t)b * S + s) * HW * 4;
  for (int q = blockIdx.x * kBlock + threadIdx.x; q < HW;
       q += gridDim.x * kBlock) {
    const int qy = q / W;
    const int qx = q - qy * W;
    // which of the four conditions hold for this texel (ring: the
    // outward one is dropped)
    const bool c_ul = qx > 0, c_uh = qx < W - 1;
    const bool c_vl = qy > 0, c_vh = qy < H - 1;
    const float kul = (float)(qx - 1), kuh = (float)(qx + 1);
    const float kvl = (float)(qy - 1), kvh = (float)(qy + 1);

    // ---- rows: interior texels from the hfwd image of the tap halo ----
    int ylo = 0, yhi = H - 1;
    if (finite && c_ul && c_uh && c_vl && c_vh) {
      const float cx[2] = {(float)qx - 1.25f, (float)qx + 1.25f};
      const float cy[2] = {(float)qy - 1.25f, (float)qy + 1.25f};
      float mny = 1e30f, mxy = -1e30f;
      bool pos = true, neg = true, fin = true;
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const float x = cx[ci & 1], y = cy[ci >> 1];
        const float pz = s_Hf[6] * x + s_Hf[7] * y + s_Hf[8];
        const float py = (s_Hf[3] * x + s_Hf[4] * y + s_Hf[5]) / pz;
        pos = pos && (pz > 1e-8f);
        neg = neg && (pz < -1e-8f);
        fin = fin && isfinite(py);
        mny = fminf(mny, py);
        mxy = fmaxf(mxy, py);
      }
      // one sign of the depth over the halo: its image is convex and the
      // corners bound it
      if ((pos || neg) && fin) {
        ylo = (int)clampf(floorf(mny - 1.0f), 0.0f, fH1);
        yhi = (int)clampf(ceilf(mxy + 1.0f), 0.0f, fH1);
      }
    }

    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int y = ylo; y <= yhi; ++y) {
      int lo = 0, hi = W - 1;
      const float fy = (float)y;
      const float hz0 = s_Hi[7] * fy + s_Hi[8];
      const float hz1 = s_Hi[6] * fW1 + hz0;
      float sg = 0.0f;  // sign of hz over the row, 0 = not safely one sign
      if (finite) {
        if (hz0 > mz && hz1 > mz) sg = 1.0f;
        else if (hz0 < -mz && hz1 < -mz) sg = -1.0f;
      }
      if (sg != 0.0f) {
        bool any = true;
#define CLIP(COND, K, SGN, R0, R1, R2, T)                                   \
        if (any && (COND)) {                                                \
          const float a_ = (SGN) * sg * (s_Hi[R0] - (K) * s_Hi[6]);         \
          const float c_ = (SGN) * sg * ((s_Hi[R1] - (K) * s_Hi[7]) * fy +  \
                                         (s_Hi[R2] - (K) * s_Hi[8]));       \
          const float m_ = 1e-5f * ((T) + (fabsf(K) + 1.0f) * Tz);          \
          any = clip_row(a_, c_, m_, W, lo, hi);                            \
        }
        CLIP(c_ul, kul, 1.0f, 0, 1, 2, Tx)    // u > qx - 1
        CLIP(c_uh, kuh, -1.0f, 0, 1, 2, Tx)   // u < qx + 1
        CLIP(c_vl, kvl, 1.0f, 3, 4, 5, Ty)    // v > qy - 1
        CLIP(c_vh, kvh, -1.0f, 3, 4, 5, Ty)   // v < qy + 1
#undef CLIP
        if (!any) continue;
        lo = max(lo, 0);
        hi = min(hi, W - 1);
      }
      for (int x = lo; x <= hi; ++x) {
        const float2 uv = project_uv(s_Hi, x, y);
        const TapRef t = make_tap(uv.x, uv.y, W, H);
        if ((t.x0 != qx && t.x1 != qx) || (t.y0 != qy && t.y1 != qy)) continue;
        const float4 g = *reinterpret_cast<const float4*>(
            pay + (unsigned)(y * W + x) * 4u);
        const float w00 = (1 - t.wx) * (1 - t.wy), w01 = t.wx * (1 - t.wy);
        const float w10 = (1 - t.wx) * t.wy, w11 = t.wx * t.wy;
        if (t.x0 == qx && t.y0 == qy && w00 != 0.0f) collect_tap(acc, w00, g);
        if (t.x1 == qx && t.y0 == qy && w01 != 0.0f) collect_tap(acc, w01, g);
        if (t.x0 == qx && t.y1 == qy && w10 != 0.0f) collect_tap(acc, w10, g);
        if (t.x1 == qx && t.y1 == qy && w11 != 0.0f) collect_tap(acc, w11, g);
      }
    }
    float4* dst = reinterpret_cast<float4*>(gm + (unsigned)q * 4u);
    if (ACCUM) {
      const float4 cur = *dst;
      acc = make_float4(cur.x + acc.x, cur.y + acc.y, cur.z + acc.z,
                        cur.w + acc.w);
    }
    *dst = acc;
  }
}

inline int grid_x(int HW) {
  int g = (HW + kBlock - 1) / kBlock;
  return g < 4096 ? g : 4096;
}

// accum false: grad_mpi = pull of `payload` (no fill needed); accum true:
// grad_mpi, holding the earlier views, += pull
void launch_collect(bool accum, const float* payload, const float* hinv,
                    const float* hfwd, float* grad_mpi, int B, int S, int H,
                    int W, hipStream_t stream) {
  dim3 grid(grid_x(H * W), S, B);
  if (accum) {
    hipLaunchKernelGGL(tgt_collect_kernel<true>, grid, dim3(kBlock), 0, stream,
                       payload, hinv, hfwd, grad_mpi, B, S, H, W);
  } else {
    hipLaunchKernelGGL(tgt_collect_kernel<false>, grid, dim3(kBlock), 0,
                       stream, payload, hinv, hfwd, grad_mpi, B, S, H, W);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

#define DISPATCH_BOOL(VAL, NAME, ...)          \
  if (VAL) {                                   \
    constexpr bool NAME = true;                \
    __VA_ARGS__;                               \
  } else {                                     \
    constexpr bool NAME = false;               \
    __VA_ARGS__;                               \
  }

extern "C" {

void mine_src_composite_fwd(const float* mpi, const float* depths,
                            const float* kinv, const float* img,
                            float* rgb_out, float* depth_out, float* mpi_blend,
                            int B, int S, int H, int W, int bg_inf, int alpha,
                            hipStream_t stream) {
  dim3 grid(grid_x(H * W), B);
  const bool blend = img != nullptr;
  if (alpha) {  // alpha-compositing: no blend, no bg term (ref :19-39)
    hipLaunchKernelGGL((src_composite_fwd_kernel<false, false, true>), grid,
                       dim3(kBlock), 0, stream, mpi, depths, kinv, nullptr,
                       rgb_out, depth_out, mpi_blend, B, S, H, W);
    return;
  }
  DISPATCH_BOOL(blend, BLEND, {
    DISPATCH_BOOL(bg_inf, BG, {
      hipLaunchKernelGGL((src_composite_fwd_kernel<BLEND, BG>), grid,
                         dim3(kBlock), 0, stream, mpi, depths, kinv, img,
                         rgb_out, depth_out, mpi_blend, B, S, H, W);
    })
  })
}

void mine_src_composite_bwd(const float* mpi, const float* depths,
                            const float* kinv, const float* img,
                            const float* g_rgb, const float* g_depth,
                            const float* g_blend, float* grad_mpi,
                            int B, int S, int H, int W, int bg_inf, int alpha,
                            hipStream_t stream) {
  dim3 grid(grid_x(H * W), B);
  const bool blend = img != nullptr;
  if (alpha) {
    hipLaunchKernelGGL((src_composite_bwd_kernel<false, false, true>), grid,
                       dim3(kBlock), 0, stream, mpi, depths, kinv, nullptr,
                       g_rgb, g_depth, nullptr, grad_mpi, B, S, H, W);
    return;
  }
  DISPATCH_BOOL(blend, BLEND, {
    DISPATCH_BOOL(bg_inf, BG, {
      hipLaunchKernelGGL((src_composite_bwd_kernel<BLEND, BG>), grid,
                         dim3(kBlock), 0, stream, mpi, depths, kinv, img,
                         g_rgb, g_depth, g_blend, grad_mpi, B, S, H, W);
    })
  })
}

void mine_tgt_composite_fwd(const float* mpi, const float* hinv,
                            const float* m_rki, const float* tvec,
                            const float* depths, float* rgb_out,
                            float* depth_out, float* mask_out,
                            int B, int S, int H, int W, int bg_inf, int alpha,
                            hipStream_t stream) {
  dim3 grid(grid_x(H * W), B);
  if (alpha) {
    hipLaunchKernelGGL((tgt_composite_fwd_kernel<false, true>), grid,
                       dim3(kBlock), 0, stream, mpi, hinv, m_rki, tvec,
                       depths, rgb_out, depth_out, mask_out, B, S, H, W);
    return;
  }
  DISPATCH_BOOL(bg_inf, BG, {
    hipLaunchKernelGGL((tgt_composite_fwd_kernel<BG>), grid, dim3(kBlock), 0,
                       stream, mpi, hinv, m_rki, tvec, depths, rgb_out,
                       depth_out, mask_out, B, S, H, W);
  })
}

// V cameras, one MPI: the same kernel over V*B view rows (VIEW ROWS)
void mine_tgt_views_fwd(const float* mpi, const float* hinv,
                        const float* m_rki, const float* tvec,
                        const float* depths, float* rgb_out, float* depth_out,
                        float* mask_out, int V, int B, int S, int H, int W,
                        int bg_inf, int alpha, hipStream_t stream) {
  dim3 grid(grid_x(H * W), V * B);
  if (alpha) {
    hipLaunchKernelGGL((tgt_composite_fwd_kernel<false, true>), grid,
                       dim3(kBlock), 0, stream, mpi, hinv, m_rki, tvec,
                       depths, rgb_out, depth_out, mask_out, B, S, H, W);
    return;
  }
  DISPATCH_BOOL(bg_inf, BG, {
    hipLaunchKernelGGL((tgt_composite_fwd_kernel<BG>), grid, dim3(kBlock), 0,
                       stream, mpi, hinv, m_rki, tvec, depths, rgb_out,
                       depth_out, mask_out, B, S, H, W);
  })
}

// collect pass alone: grad_mpi (no fill needed) = pull of `payload`
void mine_tgt_collect(const float* payload, const float* hinv,
                      const float* hfwd, float* grad_mpi, int B, int S, int H,
                      int W, hipStream_t stream) {
  launch_collect(false, payload, hinv, hfwd, grad_mpi, B, S, H, W, stream);
}

// mode 0: scatter everywhere (round-1 path); mode 1: gather redesign
// (payload + hfwd required; grad_mpi pre-zeroed, payload need not be);
// mode 2: order-fixed emit + collect (payload + hfwd required; neither
// buffer needs a fill, grad_mpi is stored by the collect pass alone).
//
// `accum` (mode 2 only) selects the collect pass that adds to grad_mpi;
// modes 0 and 1 add to grad_mpi in any case.
static void tgt_bwd_one_view(const float* mpi, const float* hinv,
                             const float* hfwd, const float* m_rki,
                             const float* tvec, const float* depths,
                             const float* g_rgb, const float* g_depth,
                             float* grad_mpi, float* payload,
                             int B, int S, int H, int W, int bg_inf, int mode,
                             int alpha, bool accum, hipStream_t stream) {
  dim3 grid(grid_x(H * W), B);
#define TGT_BWD_LAUNCH(BGv, MODEv, ALv, GM, PAY)                              \
  hipLaunchKernelGGL((tgt_composite_bwd_kernel<BGv, MODEv, ALv>), grid,       \
                     dim3(kBlock), 0, stream, mpi, hinv, m_rki, tvec,         \
                     depths, g_rgb, g_depth, GM, PAY, B, S, H, W)
#define TGT_BWD_BODY(BGv, ALv)                                                \
  if (mode == 2) {                                                            \
    TGT_BWD_LAUNCH(BGv, kTgtEmit, ALv, nullptr, payload);                     \
    launch_collect(accum, payload, hinv, hfwd, grad_mpi, B, S, H, W, stream); \
  } else if (mode == 1) {                                                     \
    TGT_BWD_LAUNCH(BGv, kTgtGather, ALv, grad_mpi, payload);                  \
    const int tiles_x = (W + GT - 1) / GT;                                    \
    const int tiles_y = (H + GT - 1) / GT;                                    \
    dim3 ggrid(tiles_x * tiles_y, S, B);                                      \
    hipLaunchKernelGGL(tgt_gather_kernel, ggrid, dim3(kGBlock), 0, stream,    \
                       payload, hinv, hfwd, grad_mpi, B, S, H, W, tiles_x);   \
  } else {                                                                    \
    TGT_BWD_LAUNCH(BGv, kTgtScatter, ALv, grad_mpi, nullptr);                 \
  }
  if (alpha) {
    TGT_BWD_BODY(false, true)
    return;
  }
  DISPATCH_BOOL(bg_inf, BG, { TGT_BWD_BODY(BG, false) })
#undef TGT_BWD_BODY
#undef TGT_BWD_LAUNCH
}

void mine_tgt_composite_bwd(const float* mpi, const float* hinv,
                            const float* hfwd, const float* m_rki,
                            const float* tvec, const float* depths,
                            const float* g_rgb, const float* g_depth,
                            float* grad_mpi, float* payload,
                            int B, int S, int H, int W, int bg_inf, int mode,
                            int alpha, hipStream_t stream) {
  tgt_bwd_one_view(mpi, hinv, hfwd, m_rki, tvec, depths, g_rgb, g_depth,
                   grad_mpi, payload, B, S, H, W, bg_inf, mode, alpha, false,
                   stream);
}

// View after view in stream order, each at its own offsets into the
// view-major geometry and upstream gradients; ONE payload and ONE
// grad_mpi serve all of them. Modes 0 and 1 add into the zero-filled
// grad_mpi (atomics, and the gather flush's read-add-write); mode 2
// stores view 0 and accumulates the later ones in ascending order.
void mine_tgt_views_bwd(const float* mpi, const float* hinv, const float* hfwd,
                        const float* m_rki, const float* tvec,
                        const float* depths, const float* g_rgb,
                        const float* g_depth, float* grad_mpi, float* payload,
                        int V, int B, int S, int H, int W, int bg_inf,
                        int mode, int alpha, hipStream_t stream) {
  const int64_t HW = (int64_t)H * W;
  for (int v = 0; v < V; ++v) {
    const int64_t r = (int64_t)v * B;  // first view row
    tgt_bwd_one_view(mpi, hinv + r * S * 9, hfwd ? hfwd + r * S * 9 : nullptr,
                     m_rki + r * 9, tvec + r * 3, depths,
                     g_rgb ? g_rgb + r * 3 * HW : nullptr,
                     g_depth ? g_depth + r * HW : nullptr, grad_mpi, payload,
                     B, S, H, W, bg_inf, mode, alpha, v > 0, stream);
  }
}

}  // extern "C"
