// Fused reflection-pad + 3x3 stride-1 conv, NHWC bf16 or fp16, MFMA
// 16x16x32. The element type is a template parameter (elem16.h); the
// fragment maps, LDS image and store pattern are the same for both.
// (the reference's ConvBlock conv, ref network/monodepth2/layers.py:106-138)
//
// The decoder's hot remaining convs are small-channel 3x3 blocks at
// full resolution (16->16, 16->4, 32->16... at (B*S)=256 batch). They
// are memory-bound: ~0.5 TFLOP against ~5 GB per direction per step.
// This kernel folds the pad into the LDS stage (no padded tensor ever
// exists) and is built so that instruction issue stays out of the way
// of the stream: C and K are template parameters, every tap / segment /
// LDS offset is a constant, and each lane stores whole 8-byte groups.
//
// Fragment layout (measured on gfx950 with tools/mfma_probe.hip):
//   A:   row = lane & 15,  k = (lane>>4)*8 + e   (8 CONSECUTIVE k)
//   B:   col = lane & 15,  k = (lane>>4)*8 + e
//   C/D: col = lane & 15,  row = (lane>>4)*4 + r
//
// GEMM view: A = WEIGHTS (row = output channel), B = PIXELS (col =
// pixel). The A and B lane maps are identical, so the packed weight
// fragments of mine_amd/ops/conv.py serve as A unchanged, and D comes
// out with col = pixel, row = output channel: a lane holds channels
// (lane>>4)*4 .. +3 of pixel lane&15 — one 8-byte store, 16 pixels x
// 2K bytes contiguous per wave.
//
// K-dim = 9*C zero-padded to a multiple of 32 in the order
// k = seg*8 + ci, seg = cb*9 + tap, tap = dy*3 + dx, c = cb*8 + ci;
// lane group g = lane>>4 of chunk kc carries seg = 4*kc + g. A lane's 8
// B-elements are 8 consecutive input channels at ONE tap: a single
// ds_read_b128. Each output element is the same sequence of fp32
// products as in the first version of this kernel.
//
// Workgroup: 4 waves; output tile = TILE_H rows x 64 pixels x <=64
// output channels; wave w owns pixels 16w..16w+15 of every row. The K
// chunks are the OUTER (fully unrolled) loop: a chunk's weight
// fragments are fetched once per tile and the TILE_H rows run under
// them, accumulators TILE_H x NK x 4 VGPRs.
//
// LDS image, in 16-byte vectors (8 channels of one pixel):
//   vec(cb, row, x) = cb*CB_PITCH + row*ROW_PITCH + x
// with x the staged pixel 0..65 (input x0-1 .. x0+64), row 0..5.
// ds_read_b128 is served in four groups of 16 lanes, each made of 8
// lanes of an even g with pixels S and 8 lanes of the next g with the
// complementary pixels S' (S = {0-3,12-15} or {4-11}); the group is
// conflict-free iff the 16 vector indices are distinct mod 16 (or the
// same address). The two g's hold consecutive segments:
//   same (cb,dy), dx -> dx+1 : indices p+dx (p in S), p+dx+1 (p in S')
//                              -> a window of 16, one shared address
//   dx 2 -> 0, dy -> dy+1    : needs ROW_PITCH     == 2 (mod 16)
//   tap 8 -> tap 0, cb -> +1 : needs CB_PITCH - 2*ROW_PITCH == 2
// so ROW_PITCH = 66 (exactly the staged width) and CB_PITCH = 406
// (6*66 + 10 pad vectors). tests/test_conv_lds_sim.py replays this map.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "elem16.h"
#include "launchers.h"

namespace {

using elem16::Elem16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kBlock = 256;
constexpr int TILE_W = 64;          // output pixels per row tile
constexpr int TILE_H = 4;           // output rows per workgroup
constexpr int STAGE_W = TILE_W + 2; // 66
constexpr int STAGE_H = TILE_H + 2; // 6 staged input rows (halo shared)
constexpr int STAGE_BATCH = 7;      // 16-byte loads in flight per thread
constexpr int ROW_PITCH = STAGE_W;                 // 66  == 2 (mod 16)
constexpr int CB_PITCH = STAGE_H * ROW_PITCH + 10; // 406 == 6 (mod 16)
static_assert(ROW_PITCH % 16 == 2 && (CB_PITCH - 2 * ROW_PITCH) % 16 == 2,
              "LDS pitches must keep the B-fragment reads conflict-free");

enum PadMode { PAD_REFLECT = 0, PAD_ZERO = 1 };

template <int PAD>
__device__ __forceinline__ int map_coord(int v, int n, int src_n, int off) {
  // reflect: -1 -> 1, n -> n-2 (pad 1); zero: OOB -> -1 sentinel.
  // (src_n, off) give the backing array's extent when the LOGICAL image
  // is a zero-embedded ring around it (the transposed-conv use: logical
  // H = src_H + 2, off = 1); for the plain forward src_n == n, off == 0.
  if (PAD == PAD_REFLECT) {
    if (v < 0) v = -v;
    if (v >= n) v = 2 * (n - 1) - v;
    // rows/columns past the image (partial tiles) are staged but never
    // stored; keep their source address inside the tensor
    return min(max(v, 0), n - 1);
  }
  v -= off;
  return (v < 0 || v >= src_n) ? -1 : v;
}

// LDS vector offset of segment `seg` relative to (row 0, pixel 0). The
// zero-padded segments past nseg re-read the last real one (their
// fragment is zeroed after the read), which keeps their lane group on
// the same conflict-free pattern.
__host__ __device__ constexpr int seg_vec_off(int seg, int nseg) {
  const int s = seg < nseg ? seg : nseg - 1;
  const int cb = s / 9, tap = s % 9;
  return cb * CB_PITCH + (tap / 3) * ROW_PITCH + (tap % 3);
}

// One staged vector per call: which (cb, row, x) thread `tid` handles in
// pass `it`, kept as running counters so the loop has no division.
template <int CV>
struct StageIdx {
  static constexpr int PX_STEP = kBlock / CV;       // pixels per pass
  static constexpr int CV_STEP = kBlock % CV;
  static constexpr int ROW_STEP = PX_STEP / STAGE_W;
  static constexpr int X_STEP = PX_STEP % STAGE_W;
  int cv, x, row;
  __device__ __forceinline__ explicit StageIdx(int tid) {
    cv = tid % CV;  // CV is a constant: mask or multiply
    x = tid / CV;   // < 256
    row = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (x >= STAGE_W) { x -= STAGE_W; ++row; }
  }
  __device__ __forceinline__ void next() {
    x += X_STEP;
    row += ROW_STEP;
    if (CV_STEP) {
      cv += CV_STEP;
      if (cv >= CV) { cv -= CV; ++x; }
    }
    if (x >= STAGE_W) { x -= STAGE_W; ++row; }
  }
};

// CV = input channels / 8, NK = 16-wide output-channel tiles of this
// launch, CIN4 = the input tensor has 4 channels per pixel (the
// dispconv gradient), staged with 8-byte loads into the lower half of
// an 8-channel vector.
//
// Register budget: the second launch bound asks for 6 workgroups per CU
// (6 waves/SIMD, what the first version of this kernel ran at) up to
// K = 32; with the 48 / 64 accumulators of NK = 3 / 4 the compiler
// needs 4 / 3 to stay out of scratch (C = 64 is at 3 by its LDS anyway).
// KVEC: K % 4 == 0, so a lane's 4 channels go out as one 8-byte store.
template <typename T, int PAD, int CV, int NK, bool CIN4, bool KVEC>
__global__ void __launch_bounds__(kBlock, (NK <= 2 ? 6 : NK == 3 ? 4 : 3))
conv3x3_fwd_kernel(const T* __restrict__ x,               // (N,sH,sW,C)
                   const typename Elem16<T>::frag8* __restrict__ wp,  // frags
                   const float* __restrict__ bias,        // (K) or null
                   T* __restrict__ out,                   // (N,H,W,K)
                   int H, int W, int K, int k0,
                   int sH, int sW, int off) {
  using E = Elem16<T>;
  using raw = typename E::raw;
  using frag8 = typename E::frag8;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  frag8* s_in = reinterpret_cast<frag8*>(s_raw);
  constexpr int CPIX = CIN4 ? 4 : CV * 8;    // channels per pixel in memory
  constexpr int NSEG = 9 * CV;               // segments of 8 k
  constexpr int NCH = (NSEG + 3) / 4;        // 32-wide K chunks
  constexpr int NIT = (STAGE_H * STAGE_W * CV + kBlock - 1) / kBlock;

  const int x0 = blockIdx.x * TILE_W;
  const int y0 = blockIdx.y * TILE_H;
  const int n = blockIdx.z;
  const int tid = threadIdx.x;

  // ---- stage 6 rows x 66 pixels x C in batches of up to STAGE_BATCH
  // vectors per thread: a batch's loads are all issued before its LDS
  // writes, so a thread keeps that many 16-byte loads in flight ----
  {
    const T* x_n = x + (int64_t)n * sH * sW * CPIX;
    StageIdx<CV> si(tid), sj(tid);
#pragma unroll
    for (int b0 = 0; b0 < NIT; b0 += STAGE_BATCH) {
      frag8 v[STAGE_BATCH];
#pragma unroll
      for (int it = 0; it < STAGE_BATCH; ++it) {
        if (b0 + it >= NIT) break;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[it][e] = (raw)0.0f;
        if (si.row < STAGE_H) {
          const int yy = map_coord<PAD>(y0 + si.row - 1, H, sH, off);
          const int xx = map_coord<PAD>(x0 + si.x - 1, W, sW, off);
          if (yy >= 0 && xx >= 0) {
            const T* src =
                x_n + ((int64_t)yy * sW + xx) * CPIX + si.cv * 8;
            if (CIN4) {
              using frag4 = typename E::frag4;
              const frag4 h = *reinterpret_cast<const frag4*>(src);
#pragma unroll
              for (int e = 0; e < 4; ++e) v[it][e] = h[e];
            } else {
              v[it] = *reinterpret_cast<const frag8*>(src);
            }
          }
        }
        si.next();
      }
#pragma unroll
      for (int it = 0; it < STAGE_BATCH; ++it) {
        if (b0 + it >= NIT) break;
        if (sj.row < STAGE_H)
          s_in[sj.cv * CB_PITCH + sj.row * ROW_PITCH + sj.x] = v[it];
        sj.next();
      }
    }
  }
  __syncthreads();

  // ---- MFMA tiles ----
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int px_base = wave * 16;            // this wave's 16 pixels
  // a wave whose 16 pixels all lie past the image edge has nothing to
  // compute or store (wave-uniform; no barrier follows)
  if (x0 + px_base >= W) return;
  const int p = lane & 15;                  // B col / output pixel offset
  const int g = lane >> 4;                  // segment within a chunk

  f32x4 acc[TILE_H][NK];
#pragma unroll
  for (int r = 0; r < TILE_H; ++r)
#pragma unroll
    for (int a = 0; a < NK; ++a) acc[r][a] = f32x4{0.f, 0.f, 0.f, 0.f};

  const frag8* s_lane = s_in + px_base + p;
  const frag8* w_lane = wp + lane;

#pragma unroll
  for (int kc = 0; kc < NCH; ++kc) {
    // constants after unrolling: three selects per chunk
    const int o = g == 0 ? seg_vec_off(kc * 4 + 0, NSEG)
                : g == 1 ? seg_vec_off(kc * 4 + 1, NSEG)
                : g == 2 ? seg_vec_off(kc * 4 + 2, NSEG)
                         : seg_vec_off(kc * 4 + 3, NSEG);
    frag8 wf[NK];
#pragma unroll
    for (int a = 0; a < NK; ++a) wf[a] = w_lane[(a * NCH + kc) * 64];
#pragma unroll
    for (int r = 0; r < TILE_H; ++r) {
      frag8 b = s_lane[o + r * ROW_PITCH];
      if (kc * 4 + 3 >= NSEG) {  // the zero-padded tail of the K-dim
        if (kc * 4 + g >= NSEG) {
#pragma unroll
          for (int e = 0; e < 8; ++e) b[e] = (raw)0.0f;
        }
      }
#pragma unroll
      for (int a = 0; a < NK; ++a)
        acc[r][a] = E::mfma(wf[a], b, acc[r][a]);
    }
  }

  // ---- epilogue: bias in fp32, one rounding, 8-byte stores ----
  const int pix = x0 + px_base + p;
  if (pix >= W) return;
#pragma unroll
  for (int a = 0; a < NK; ++a) {
    const int kout = k0 + a * 16 + g * 4;   // this lane's 4 channels
    if (kout >= K) continue;
    float b4[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kout + r < K) b4[r] = bias[kout + r];
    }
#pragma unroll
    for (int r = 0; r < TILE_H; ++r) {
      const int y = y0 + r;
      if (y >= H) break;
      T* dst = out + (((int64_t)n * H + y) * W + pix) * K + kout;
      T h[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) h[c] = E::from_float(acc[r][a][c] + b4[c]);
      if (KVEC) {
        uint2 u;
        u.x = E::bits(h[0]) | (E::bits(h[1]) << 16);
        u.y = E::bits(h[2]) | (E::bits(h[3]) << 16);
        *reinterpret_cast<uint2*>(dst) = u;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (kout + c < K) dst[c] = h[c];
      }
    }
  }
}

template <typename T, int PAD, int CV, int NK, bool CIN4>
void launch(const void* x, const void* wp, const float* bias, void* out,
            int N, int H, int W, int K, int k0, int sH, int sW, int off,
            hipStream_t stream) {
  constexpr int NCH = (9 * CV + 3) / 4;
  const dim3 grid((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H, N);
  using frag8 = typename Elem16<T>::frag8;
  const size_t lds = (size_t)CV * CB_PITCH * sizeof(frag8);
  // weights of output-channel tile k0/16 onwards
  const frag8* wk =
      reinterpret_cast<const frag8*>(wp) + (size_t)(k0 / 16) * NCH * 64;
  if (K % 4 == 0)
    hipLaunchKernelGGL((conv3x3_fwd_kernel<T, PAD, CV, NK, CIN4, true>), grid,
                       dim3(kBlock), lds, stream,
                       reinterpret_cast<const T*>(x), wk, bias,
                       reinterpret_cast<T*>(out), H, W, K, k0, sH, sW, off);
  else
    hipLaunchKernelGGL((conv3x3_fwd_kernel<T, PAD, CV, NK, CIN4, false>), grid,
                       dim3(kBlock), lds, stream,
                       reinterpret_cast<const T*>(x), wk, bias,
                       reinterpret_cast<T*>(out), H, W, K, k0, sH, sW, off);
}

template <typename T, int PAD, int CV, bool CIN4>
void launch_nk(int nk, const void* x, const void* wp, const float* bias,
               void* out, int N, int H, int W, int K, int k0, int sH, int sW,
               int off, hipStream_t s) {
  switch (nk) {
    case 1: launch<T, PAD, CV, 1, CIN4>(x, wp, bias, out, N, H, W, K, k0, sH, sW, off, s); break;
    case 2: launch<T, PAD, CV, 2, CIN4>(x, wp, bias, out, N, H, W, K, k0, sH, sW, off, s); break;
    case 3: launch<T, PAD, CV, 3, CIN4>(x, wp, bias, out, N, H, W, K, k0, sH, sW, off, s); break;
    default: launch<T, PAD, CV, 4, CIN4>(x, wp, bias, out, N, H, W, K, k0, sH, sW, off, s); break;
  }
}

template <typename T, int PAD>
bool launch_cv(int cv, bool cin4, int nk, const void* x, const void* wp,
               const float* bias, void* out, int N, int H, int W, int K,
               int k0, int sH, int sW, int off, hipStream_t s) {
  if (cin4) {
    if (PAD != PAD_ZERO || cv != 1) return false;
    launch_nk<T, PAD_ZERO, 1, true>(nk, x, wp, bias, out, N, H, W, K, k0, sH, sW, off, s);
    return true;
  }
  switch (cv) {
#define MINE_CONV_CV(V)                                                       \
    case V: launch_nk<T, PAD, V, false>(nk, x, wp, bias, out, N, H, W, K, k0,\
                                     sH, sW, off, s); return true;
    MINE_CONV_CV(1) MINE_CONV_CV(2) MINE_CONV_CV(3) MINE_CONV_CV(4)
    MINE_CONV_CV(5) MINE_CONV_CV(6) MINE_CONV_CV(7) MINE_CONV_CV(8)
#undef MINE_CONV_CV
  }
  return false;
}

template <typename T>
int conv3x3_fwd_t(const void* x, const void* wp, const float* bias, void* out,
                  int N, int H, int W, int C, int c_mem, int K, int pad_mode,
                  int src_h, int src_w, int off, hipStream_t stream) {
  const bool cin4 = c_mem != C;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int nk = (((K - k0) < 64 ? (K - k0) : 64) + 15) / 16;
    const bool ok =
        pad_mode == PAD_REFLECT
            ? launch_cv<T, PAD_REFLECT>(C / 8, cin4, nk, x, wp, bias, out, N,
                                        H, W, K, k0, src_h, src_w, off, stream)
            : launch_cv<T, PAD_ZERO>(C / 8, cin4, nk, x, wp, bias, out, N, H,
                                     W, K, k0, src_h, src_w, off, stream);
    if (!ok) return kNoKernel;
  }
  return kLaunched;
}

}  // namespace

// C = logical input channels (multiple of 8, <= 64); c_mem = channels
// per pixel in memory: C, or 4 with C == 8 in zero-embed mode. Output
// channels beyond 64 run as further launches over the same input.
// x, wp and out share the element type `elem`, bf16 or fp16.
// Returns kNoKernel when no kernel is instantiated for the shape or type.
extern "C" int mine_conv3x3_fwd(const void* x, const void* wp,
                                const float* bias, void* out, int N, int H,
                                int W, int C, int c_mem, int K, int pad_mode,
                                int src_h, int src_w, int off, int elem,
                                hipStream_t stream) {
  if (C % 8 || C < 8 || C > 64 || K < 1) return kNoKernel;
  if (c_mem != C && !(c_mem == 4 && C == 8)) return kNoKernel;
  MINE_ELEM_SWITCH16(elem, return conv3x3_fwd_t<T>(x, wp, bias, out, N, H, W,
                                                   C, c_mem, K, pad_mode,
                                                   src_h, src_w, off, stream))
  return kNoKernel;
}

// Gather a (K,C,3,3) weight into MFMA fragment order in one launch:
// out[i] = TOUT(w[lut[i]]), or 0 where lut[i] is the one-past-the-end
// pad slot. fp32 -> bf16 / fp16 rounds to nearest even, as torch's cast
// does.
namespace {
template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(kBlock)
conv3x3_pack_kernel(const TIN* __restrict__ w, const int64_t* __restrict__ lut,
                    TOUT* __restrict__ out, int64_t n_out, int64_t n_w) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_out) return;
  const int64_t j = lut[i];
  out[i] = (j >= 0 && j < n_w) ? (TOUT)(float)w[j] : (TOUT)0.0f;
}

template <typename TOUT>
int pack_t(const void* w, int w_elem, const int64_t* lut, void* out,
           int64_t n_out, int64_t n_w, hipStream_t stream) {
  const dim3 grid((unsigned)((n_out + kBlock - 1) / kBlock));
  MINE_ELEM_SWITCH(w_elem,
                   hipLaunchKernelGGL((conv3x3_pack_kernel<T, TOUT>), grid,
                                      dim3(kBlock), 0, stream,
                                      reinterpret_cast<const T*>(w), lut,
                                      reinterpret_cast<TOUT*>(out), n_out,
                                      n_w))
  return kLaunched;
}
}  // namespace

extern "C" int mine_conv3x3_pack(const void* w, int w_elem, const int64_t* lut,
                                 void* out, int out_elem, int64_t n_out,
                                 int64_t n_w, hipStream_t stream) {
  MINE_ELEM_SWITCH16(out_elem,
                     return pack_t<T>(w, w_elem, lut, out, n_out, n_w, stream))
  return kNoKernel;
}
