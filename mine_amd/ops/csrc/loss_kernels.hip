// Fused edge-aware smoothness v2 (the TRAINED smoothness term, ref
// network/layers.py:83-99):
//   d = disp / (mean(disp) + 1e-7)
//   L = mean(|dx d| * exp(-mean_c |dx img|)) + (same for y)
// The eager form is ~15 elementwise/reduction launches per call, 8
// calls per step; here forward is ONE reduction kernel (plus the tiny
// per-image disp mean, kept in torch) and backward is a gather pass
// (each pixel re-derives its <=4 difference terms — no atomics beyond
// the per-image dot-product scalar) plus an elementwise finish for the
// mean-normalization chain rule.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float img_gx(const float* img, int64_t b_off,
                                        int64_t sc, int64_t sy, int64_t sx,
                                        int y, int x) {
  // mean over 3 channels of |img[y,x] - img[y,x+1]|
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t o = b_off + c * sc + y * sy + x * sx;
    s += fabsf(img[o] - img[o + sx]);
  }
  return s * (1.0f / 3.0f);
}

__device__ __forceinline__ float img_gy(const float* img, int64_t b_off,
                                        int64_t sc, int64_t sy, int64_t sx,
                                        int y, int x) {
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t o = b_off + c * sc + y * sy + x * sx;
    s += fabsf(img[o] - img[o + sy]);
  }
  return s * (1.0f / 3.0f);
}

// DET (deterministic mode), here and in eav2_bwd_gd_kernel: instead of
// one atomicAdd per block, each block stores its (already scaled)
// partial into a workspace row and det_rows_sum_kernel adds the rows in
// an order fixed by their count — the scheme of the deterministic BN
// finish. The scaling stays where it is, so the two modes differ by
// summation order alone.
template <bool DET>
__global__ void __launch_bounds__(kBlock)
eav2_fwd_kernel(const float* __restrict__ disp,  // (B,H,W)
                const float* __restrict__ img,   // strided (B,3,H,W)
                const float* __restrict__ mean_d,  // (B)
                // (2) pre-zeroed; DET: (2, B, gridDim.x) unfilled
                float* __restrict__ out,
                int B, int H, int W,
                int64_t isb, int64_t isc, int64_t isy, int64_t isx) {
  const int b = blockIdx.y;
  const float inv_m = 1.0f / (mean_d[b] + 1e-7f);
  const int64_t b_off = (int64_t)b * isb;
  const float* db = disp + (int64_t)b * H * W;
  const int HW = H * W;
  float sx = 0.0f, sy = 0.0f;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < HW;
       i += gridDim.x * kBlock) {
    const int y = i / W;
    const int x = i - y * W;
    // difference first, then the scale: see eav2_bwd_gd_kernel
    const float d0 = db[i];
    if (x + 1 < W) {
      sx += fabsf((d0 - db[i + 1]) * inv_m) *
            __expf(-img_gx(img, b_off, isc, isy, isx, y, x));
    }
    if (y + 1 < H) {
      sy += fabsf((d0 - db[i + W]) * inv_m) *
            __expf(-img_gy(img, b_off, isc, isy, isx, y, x));
    }
  }
  __shared__ float red[2][kBlock];
  red[0][threadIdx.x] = sx;
  red[1][threadIdx.x] = sy;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (DET) {
      const int64_t row = (int64_t)b * gridDim.x + blockIdx.x;
      out[row] = red[0][0] / ((float)B * H * (W - 1));
      out[(int64_t)B * gridDim.x + row] = red[1][0] / ((float)B * (H - 1) * W);
    } else {
      atomicAdd(&out[0], red[0][0] / ((float)B * H * (W - 1)));
      atomicAdd(&out[1], red[1][0] / ((float)B * (H - 1) * W));
    }
  }
}

// out[r] = sum of ws[r * n .. r * n + n): one block per output, thread t
// adds entries t, t + kBlock, ... in ascending order, then a fixed LDS
// tree. The order depends on n alone.
__global__ void __launch_bounds__(kBlock)
det_rows_sum_kernel(const float* __restrict__ ws, int n,
                    float* __restrict__ out) {
  __shared__ float red[kBlock];
  const float* row = ws + (int64_t)blockIdx.x * n;
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += kBlock) s += row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// pass 1: g_d[i] = dL/dd_i (gathered from the <=4 difference terms) and
// the per-image dot T_b = sum_i g_d[i] * disp[i]
template <bool DET>
__global__ void __launch_bounds__(kBlock)
eav2_bwd_gd_kernel(const float* __restrict__ disp,
                   const float* __restrict__ img,
                   const float* __restrict__ mean_d,
                   float* __restrict__ g_d,    // (B,H,W)
                   // (B) pre-zeroed; DET: (B, gridDim.x) unfilled
                   float* __restrict__ Tb,
                   int B, int H, int W,
                   int64_t isb, int64_t isc, int64_t isy, int64_t isx) {
  const int b = blockIdx.y;
  const float inv_m = 1.0f / (mean_d[b] + 1e-7f);
  const int64_t b_off = (int64_t)b * isb;
  const float* db = disp + (int64_t)b * H * W;
  float* gb = g_d + (int64_t)b * H * W;
  const int HW = H * W;
  const float nx = 1.0f / ((float)B * H * (W - 1));
  const float ny = 1.0f / ((float)B * (H - 1) * W);
  const float sm = inv_m < 0.f ? -1.f : 1.f;
  float tpart = 0.0f;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < HW;
       i += gridDim.x * kBlock) {
    const int y = i / W;
    const int x = i - y * W;
    // The sign comes from the difference of the RAW disparities (exact
    // in sign, exactly 0 at a tie). d0*inv_m - d1*inv_m contracts to
    // fma(-d1, inv_m, round(d0*inv_m)), which at d0 == d1 returns the
    // rounding error of the first product: a tie then gets sgn = +-1
    // and a full-size spurious gradient. sm keeps the sign of the scale.
    const float d0 = db[i];
    float g = 0.0f;
    if (x + 1 < W) {  // right edge term (i is the left element)
      const float diff = (d0 - db[i + 1]) * sm;
      const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
      g += sgn * __expf(-img_gx(img, b_off, isc, isy, isx, y, x)) * nx;
    }
    if (x > 0) {      // left edge term (i is the right element)
      const float diff = (db[i - 1] - d0) * sm;
      const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
      g -= sgn * __expf(-img_gx(img, b_off, isc, isy, isx, y, x - 1)) * nx;
    }
    if (y + 1 < H) {
      const float diff = (d0 - db[i + W]) * sm;
      const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
      g += sgn * __expf(-img_gy(img, b_off, isc, isy, isx, y, x)) * ny;
    }
    if (y > 0) {
      const float diff = (db[i - W] - d0) * sm;
      const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
      g -= sgn * __expf(-img_gy(img, b_off, isc, isy, isx, y - 1, x)) * ny;
    }
    gb[i] = g;
    tpart += g * db[i];
  }
  __shared__ float red[kBlock];
  red[threadIdx.x] = tpart;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (DET) Tb[(int64_t)b * gridDim.x + blockIdx.x] = red[0];
    else atomicAdd(&Tb[b], red[0]);
  }
}

// pass 2: grad_disp = gl * (g_d - T_b / ((m+eps) * HW)) / (m+eps)
__global__ void __launch_bounds__(kBlock)
eav2_bwd_finish_kernel(const float* __restrict__ g_d,
                       const float* __restrict__ disp,
                       const float* __restrict__ mean_d,
                       const float* __restrict__ Tb,
                       const float* __restrict__ gl,  // scalar dL
                       float* __restrict__ grad,      // (B,H,W)
                       int B, int H, int W) {
  const int b = blockIdx.y;
  const float m = mean_d[b] + 1e-7f;
  const float corr = Tb[b] / (m * (float)(H * W));
  const float g0 = gl[0];
  const int HW = H * W;
  const int64_t off = (int64_t)b * HW;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < HW;
       i += gridDim.x * kBlock) {
    grad[off + i] = g0 * (g_d[off + i] - corr) / m;
  }
  (void)disp;
}

// Backward of the sparse-point gather out[b,c,n] = img[b,c,idx[b,n]]
// (deterministic mode) without atomics. Several points may share a
// pixel; the FIRST of them in point order owns it and adds the upstream
// gradients of all of them in point order, the others store nothing.
// N is a few hundred, so the quadratic scan costs nothing. grad_img is
// pre-zeroed (pixels no point lands on).
__global__ void __launch_bounds__(kBlock)
gather_pxpy_bwd_kernel(const float* __restrict__ g,       // (B,C,N)
                       const int64_t* __restrict__ idx,   // (B,N)
                       float* __restrict__ grad_img,      // (B,C,HW)
                       int B, int C, int N, int64_t HW) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= B * C * N) return;
  const int n = i % N;
  const int bc = i / N;
  const int64_t* ib = idx + (int64_t)(bc / C) * N;
  const int64_t p = ib[n];
  if (p < 0 || p >= HW) return;
  for (int m = 0; m < n; ++m) {
    if (ib[m] == p) return;  // an earlier point owns this pixel
  }
  const float* gr = g + (int64_t)bc * N;
  float s = gr[n];
  for (int m = n + 1; m < N; ++m) {
    if (ib[m] == p) s += gr[m];
  }
  grad_img[(int64_t)bc * HW + p] = s;
}

inline int gx_of(int HW) {
  int g = (HW + kBlock - 1) / kBlock;
  return g < 1024 ? g : 1024;
}

}  // namespace

extern "C" {

// grid.x of the eav2 launches: the row count of the deterministic
// workspaces
int mine_eav2_grid(int HW) { return gx_of(HW); }

// ws == nullptr: atomics into the pre-zeroed out (2). Otherwise ws is an
// unfilled (2, B, mine_eav2_grid) workspace and out needs no fill.
void mine_eav2_fwd(const float* disp, const float* img, const float* mean_d,
                   float* out, float* ws, int B, int H, int W, int64_t isb,
                   int64_t isc, int64_t isy, int64_t isx,
                   hipStream_t stream) {
  dim3 grid(gx_of(H * W), B);
  if (ws == nullptr) {
    hipLaunchKernelGGL(eav2_fwd_kernel<false>, grid, dim3(kBlock), 0, stream,
                       disp, img, mean_d, out, B, H, W, isb, isc, isy, isx);
    return;
  }
  hipLaunchKernelGGL(eav2_fwd_kernel<true>, grid, dim3(kBlock), 0, stream,
                     disp, img, mean_d, ws, B, H, W, isb, isc, isy, isx);
  hipLaunchKernelGGL(det_rows_sum_kernel, dim3(2), dim3(kBlock), 0, stream,
                     ws, B * (int)grid.x, out);
}

// ws == nullptr: atomics into the pre-zeroed Tb (B). Otherwise ws is an
// unfilled (B, mine_eav2_grid) workspace and Tb needs no fill.
void mine_eav2_bwd(const float* disp, const float* img, const float* mean_d,
                   float* g_d, float* Tb, float* ws, const float* gl,
                   float* grad, int B, int H, int W, int64_t isb, int64_t isc,
                   int64_t isy, int64_t isx, hipStream_t stream) {
  dim3 grid(gx_of(H * W), B);
  if (ws == nullptr) {
    hipLaunchKernelGGL(eav2_bwd_gd_kernel<false>, grid, dim3(kBlock), 0,
                       stream, disp, img, mean_d, g_d, Tb, B, H, W, isb, isc,
                       isy, isx);
  } else {
    hipLaunchKernelGGL(eav2_bwd_gd_kernel<true>, grid, dim3(kBlock), 0,
                       stream, disp, img, mean_d, g_d, ws, B, H, W, isb, isc,
                       isy, isx);
    hipLaunchKernelGGL(det_rows_sum_kernel, dim3(B), dim3(kBlock), 0, stream,
                       ws, (int)grid.x, Tb);
  }
  hipLaunchKernelGGL(eav2_bwd_finish_kernel, grid, dim3(kBlock), 0, stream,
                     g_d, disp, mean_d, Tb, gl, grad, B, H, W);
}

void mine_gather_pxpy_bwd(const float* g, const int64_t* idx, float* grad_img,
                          int B, int C, int N, int64_t HW,
                          hipStream_t stream) {
  const int total = B * C * N;
  hipLaunchKernelGGL(gather_pxpy_bwd_kernel, dim3((total + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, stream, g, idx, grad_img, B, C, N, HW);
}

}  // extern "C"
