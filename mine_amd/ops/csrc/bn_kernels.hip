// Fused training-mode BatchNorm + activation, CDNA4 (gfx950).
//
// bf16, fp16 (or fp32) activations in channels_last (logical (N,H,W,C), C
// stride 1), fp32 statistics/parameters — the numerically standard
// mixed-precision BN. Replaces the eager chain
//   cast-to-f32 -> MIOpen BN (2-3 kernels) -> cast-to-bf16 -> activation
// (and its backward mirror) with:
//   fwd: one stats-reduction kernel + one normalize+activate kernel
//   bwd: one dgamma/dbeta-reduction kernel + one dx kernel
// Activation variants: none / ReLU / LeakyReLU(0.1) / ELU / add+ReLU
// (the ResNet bottleneck residual join, ref resnet bottleneck
// out = relu(bn3(conv3) + identity)).
//
// Every kernel is templated on V, the channels a thread owns: 16 bytes of
// T (one 16-byte access per row) when C is a multiple of that, else 1.
// All of them share one lane map (LaneMap below), and the tensors arrive
// as void* because a kernel only ever views them as vectors of V elements.
//
// Reductions (bn_reduce): each workgroup owns one channel-slab; lanes
// stride the N*H*W axis (coalesced along C across lanes in
// channels_last), reduce through LDS, then one fp32 atomicAdd per block
// into the output accumulator. ~1e-8-relative partial-sum error at the
// flagship sizes; backward is the same shape.
//
// Deterministic mode (DET = true instantiations of the three reduction
// kernels): same lane map and grid, so every thread sums the same rows,
// but no atomics. Each thread stores its partials to LDS at
// [row-in-block][channel]; after the barrier one thread per channel adds
// the kBlock/cgv rows in ascending order and stores the block's (2, nc)
// result with plain stores into a workspace [gridDim.x][2][C].
// bn_det_finish_kernel then adds the gridDim.x partials per channel in a
// fixed order (see its comment) and optionally finalizes.
//
// Small-layer path (small_plan below; both modes): two launches per
// direction, no zero fill, no global atomic, no finalize or counter
// launch. The DET reductions run on a grid chosen by work — few partial
// rows G, many rows per thread, U loads in flight — and store G partials
// [G][2][C]; the WS instantiations of the normalize and dx kernels add
// them in a prologue. Summation order, depending on (M, C, G, cgv) only:
//   thread:   its rows in ascending order (the unrolled body issues its
//             loads first and adds in row order);
//   block:    the kBlock/cgv rows-in-block in ascending order
//             (det_block_flush);
//   partials: ascending g (ws_sum), by every consumer workgroup for its
//             own channels, so all workgroups obtain the same bits.
// Single owner: the workgroups with blockIdx.x == 0 alone store mean /
// invstd (forward) or the (2, C) sums (backward) and update the running
// statistics; thread 0 of block (0, 0) increments num_batches_tracked.
// Data crosses workgroups only at the kernel boundary.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kBlock = 256;

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_ELU = 3,
                 ACT_ADD_RELU = 4 };

// The activation is a template parameter: the host switches on `act`
// once per launch, so the element loop carries no branch chain.
template <int ACT>
__device__ __forceinline__ float act_fwd_t(float z) {
  if constexpr (ACT == ACT_RELU || ACT == ACT_ADD_RELU)
    return z > 0.0f ? z : 0.0f;
  else if constexpr (ACT == ACT_LRELU)
    return z > 0.0f ? z : 0.1f * z;
  else if constexpr (ACT == ACT_ELU)
    return z > 0.0f ? z : __expf(z) - 1.0f;
  else
    return z;
}

// derivative as a function of the PRE-activation z
template <int ACT>
__device__ __forceinline__ float act_grad_t(float z) {
  if constexpr (ACT == ACT_RELU || ACT == ACT_ADD_RELU)
    return z > 0.0f ? 1.0f : 0.0f;
  else if constexpr (ACT == ACT_LRELU)
    return z > 0.0f ? 1.0f : 0.1f;
  else if constexpr (ACT == ACT_ELU)
    return z > 0.0f ? 1.0f : __expf(z);
  else
    return 1.0f;
}

// V consecutive channels of one row. fp16 is the compiler's native half
// (_Float16): same bits as __half / at::Half, and its float conversions
// (RNE, overflow to inf) survive __HIP_NO_HALF_CONVERSIONS__.
template <typename T, int V>
struct alignas(sizeof(T) * V) BnVec {
  T v[V];
};

// channel-group width: the smallest power of two >= min(Cv, 64), so
// small-C layers (the decoder's C=16 blocks) keep every lane busy
// instead of idling 3/4 of the block.
inline __host__ __device__ int chan_group(int Cv) {
  int g = 1;
  while (g < Cv && g < 64) g <<= 1;
  return g;
}

// ---------------------------------------------------------------------------
// Lane map shared by every kernel below: a thread owns ONE channel vector
// (lane_cv = tid & (cgv-1), channel chunks of cgv vectors on blockIdx.y)
// and walks rows m = row0, row0 + rstride, ... with
// rstride = gridDim.x * (kBlock / cgv). Its per-channel parameters are
// loaded once into registers before the row loop, so the loop body holds
// only 16-byte data accesses and arithmetic — no per-element modulo, no
// parameter loads. cgv is a power of two <= 64; a non-power-of-two Cv
// (C=24 -> Cv=3) idles the lanes with lane_cv >= ncv.
//
// Row / Stride are the integer widths of row0 / rstride: 64-bit in the
// elementwise kernels, which step a 64-bit offset by them; int in the
// reductions (the join: 64-bit row0), whose rstride <= kMaxGridReduce *
// kBlock.
// ---------------------------------------------------------------------------
template <typename Row, typename Stride>
struct LaneMap {
  int cgv, c0v, ncv, lane_cv;

  __device__ __forceinline__ LaneMap(int Cv, int cgv_)
      : cgv(cgv_),
        c0v(blockIdx.y * cgv),
        ncv(min(cgv, Cv - c0v)),
        lane_cv(threadIdx.x & (cgv - 1)) {}

  // the thread's channel vector, and whether it has one
  __device__ __forceinline__ int col() const { return c0v + lane_cv; }
  __device__ __forceinline__ bool active() const { return lane_cv < ncv; }

  // Functions, not members: the elementwise kernels retire their idle
  // lanes before this division, and with it ahead of that return the
  // compiler spends 8-17 more registers on dx, one wave per SIMD.
  __device__ __forceinline__ int rows_per_blk() const { return kBlock / cgv; }
  __device__ __forceinline__ Row row0() const {
    return (Row)blockIdx.x * rows_per_blk() + threadIdx.x / cgv;
  }
  __device__ __forceinline__ Stride rstride() const {
    return (Stride)gridDim.x * rows_per_blk();
  }
};

// ---------------------------------------------------------------------------
// reductions: two per-channel sums over the N*H*W axis
// ---------------------------------------------------------------------------

// Deterministic block combine. The caller has stored its V partials at
// s_a/s_b[threadIdx.x * V + j], which IS [row][channel] with rows of
// `width` = cgv*V floats (tid = row*cgv + lane_cv). Column i of row r sits
// at r*width + i, so consecutive threads read consecutive banks. Rows are
// added in ascending order; the result goes to ws[blockIdx.x][2][C] at
// channel col0 + i.
__device__ __forceinline__ void det_block_flush(
    const float* __restrict__ s_a, const float* __restrict__ s_b, int width,
    int rows, int ncols, float* __restrict__ ws, int C, int col0) {
  float* wa = ws + (int64_t)blockIdx.x * 2 * C + col0;
  for (int i = threadIdx.x; i < ncols; i += kBlock) {
    float ta = 0.0f, tb = 0.0f;
    for (int r = 0; r < rows; ++r) {
      ta += s_a[r * width + i];
      tb += s_b[r * width + i];
    }
    wa[i] = ta;
    wa[C + i] = tb;
  }
}

// The body of every reduction kernel. row_loop(lm, a, b) adds the
// thread's rows into its V partials of each sum; the block's partials are
// then combined through LDS into out, (2,C): LDS atomics and one global
// atomicAdd per channel, or with DET in fixed order into the workspace
// out[gridDim.x][2][C].
template <int V, bool DET, typename Row, typename RowLoop>
__device__ __forceinline__ void bn_reduce(int C, int cgv,
                                          float* __restrict__ out,
                                          RowLoop&& row_loop) {
  const LaneMap<Row, int> lm(C / V, cgv);
  __shared__ float s_a[(DET ? kBlock : 64) * V], s_b[(DET ? kBlock : 64) * V];
  if constexpr (!DET) {
    for (int i = threadIdx.x; i < cgv * V; i += kBlock) {
      s_a[i] = 0.0f;
      s_b[i] = 0.0f;
    }
    __syncthreads();
  }
  if (lm.active()) {
    float a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = b[j] = 0.0f;
    row_loop(lm, a, b);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if constexpr (DET) {
        s_a[threadIdx.x * V + j] = a[j];
        s_b[threadIdx.x * V + j] = b[j];
      } else {
        atomicAdd(&s_a[lm.lane_cv * V + j], a[j]);
        atomicAdd(&s_b[lm.lane_cv * V + j], b[j]);
      }
    }
  }
  __syncthreads();
  if constexpr (DET) {
    det_block_flush(s_a, s_b, cgv * V, lm.rows_per_blk(), lm.ncv * V, out, C,
                    lm.c0v * V);
  } else {
    for (int i = threadIdx.x; i < lm.ncv * V; i += kBlock) {
      atomicAdd(&out[lm.c0v * V + i], s_a[i]);
      atomicAdd(&out[C + lm.c0v * V + i], s_b[i]);
    }
  }
}

// stats: per-channel sum and sum-of-squares
// U > 1 (the small-layer path): U rows in flight, loads first, adds after
// in row order — the sums are those of U = 1.
template <typename T, int V, bool DET, int U = 1>
__global__ void __launch_bounds__(kBlock)
bn_stats_vec_kernel(const void* __restrict__ x, float* __restrict__ sums,
                    int64_t M, int C, int cgv) {
  using Vec = BnVec<T, V>;
  bn_reduce<V, DET, int>(
      C, cgv, sums, [&](const auto& lm, float (&acc)[V], float (&asq)[V]) {
        const int Cv = C / V;
        const Vec* xv = static_cast<const Vec*>(x);
        const int rstride = lm.rstride();
        int64_t m = lm.row0();
        if constexpr (U > 1) {
          for (; m + (int64_t)(U - 1) * rstride < M; m += (int64_t)U * rstride) {
            Vec val[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
              val[u] = xv[(m + (int64_t)u * rstride) * Cv + lm.col()];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
              for (int j = 0; j < V; ++j) {
                const float f = (float)val[u].v[j];
                acc[j] += f;
                asq[j] += f * f;
              }
            }
          }
        }
        for (; m < M; m += rstride) {
          const Vec val = xv[m * Cv + lm.col()];
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float f = (float)val.v[j];
            acc[j] += f;
            asq[j] += f * f;
          }
        }
      });
}

// mean, biased variance and invstd of one channel from its sums: the one
// formula behind bn_finalize, the deterministic finish and the small-layer
// forward, so equal sums give equal bits in all three
struct BnMoments {
  float mu, var, invstd;
};
__device__ __forceinline__ BnMoments bn_moments(float sum, float sumsq,
                                                int64_t M, float eps) {
  const float mu = sum / (float)M;
  float var = sumsq / (float)M - mu * mu;
  var = var > 0.0f ? var : 0.0f;
  return {mu, var, rsqrtf(var + eps)};
}

// stores mean/invstd of channel c; updates the running stats where given
__device__ __forceinline__ void bn_store_channel(
    const BnMoments& mo, int c, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, int64_t M, float momentum) {
  mean[c] = mo.mu;
  invstd[c] = mo.invstd;
  if (running_mean) {
    running_mean[c] += momentum * (mo.mu - running_mean[c]);
    const float unbiased =
        M > 1 ? mo.var * (float)M / (float)(M - 1) : mo.var;
    running_var[c] += momentum * (unbiased - running_var[c]);
  }
}

__device__ __forceinline__ void bn_finalize_channel(
    float sum, float sumsq, int c, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, int64_t M, float eps, float momentum) {
  bn_store_channel(bn_moments(sum, sumsq, M, eps), c, mean, invstd,
                   running_mean, running_var, M, momentum);
}

__global__ void bn_finalize_kernel(const float* __restrict__ sums,
                                   float* __restrict__ mean,
                                   float* __restrict__ invstd,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   int64_t M, int C, float eps,
                                   float momentum) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  bn_finalize_channel(sums[c], sums[C + c], c, mean, invstd, running_mean,
                      running_var, M, eps, momentum);
}

// Deterministic finish: adds the G per-block partials ws[g][2][C] of each
// channel in a FIXED TWO-LEVEL ORDER that depends only on (G, C):
//   level 1: with cw = min(chan_group(C), 16) channels per block and
//            np = kBlock/cw >= 16 partial lanes, lane p adds blocks
//            g = p, p+np, p+2np, ... in ascending g (cw is capped so the
//            2048-partial chains of the wide layers stay <= 128 long;
//            four loads are issued ahead of their adds, the adds stay in
//            order);
//   level 2: one thread per channel adds the np lane partials in
//            ascending p.
// Then it writes the (2, C) sums to `out` (bn_sums, bn_join_stats,
// bn_act_bwd_reduce) and/or, when `mean` is given, finalizes as
// bn_finalize_kernel does (bn_stats) — so the mode adds no launch. A
// separate launch after the reduction: no device-wide fence, no
// last-block-to-arrive.
__global__ void __launch_bounds__(kBlock)
bn_det_finish_kernel(const float* __restrict__ ws, int G, int C, int cw,
                     float* __restrict__ out, float* __restrict__ mean,
                     float* __restrict__ invstd,
                     float* __restrict__ running_mean,
                     float* __restrict__ running_var, int64_t M, float eps,
                     float momentum) {
  __shared__ float s_a[kBlock], s_b[kBlock];
  const int lane_c = threadIdx.x & (cw - 1);
  const int p = threadIdx.x / cw;
  const int np = kBlock / cw;
  const int c = blockIdx.x * cw + lane_c;
  float a = 0.0f, b = 0.0f;
  if (c < C) {
    const int64_t step = (int64_t)np * 2 * C;
    const float* row = ws + (int64_t)p * 2 * C + c;
    int g = p;
    for (; g + 3 * np < G; g += 4 * np, row += 4 * step) {
      float va[4], vb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        va[u] = row[u * step];
        vb[u] = row[u * step + C];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a += va[u];
        b += vb[u];
      }
    }
    for (; g < G; g += np, row += step) {
      a += row[0];
      b += row[C];
    }
  }
  s_a[threadIdx.x] = a;  // [p][lane_c]
  s_b[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x >= cw || c >= C) return;
  float ta = 0.0f, tb = 0.0f;
  for (int q = 0; q < np; ++q) {
    ta += s_a[q * cw + lane_c];
    tb += s_b[q * cw + lane_c];
  }
  if (out) {
    out[c] = ta;
    out[C + c] = tb;
  }
  if (mean)
    bn_finalize_channel(ta, tb, c, mean, invstd, running_mean, running_var, M,
                        eps, momentum);
}

// backward reduction: dbeta = sum g', dgamma = sum g' * xhat
//   where g' = gy * act'(z), z recomputed from x
//   U > 1 as in bn_stats_vec_kernel
template <typename T, int V, int ACT, bool DET, int U = 1>
__global__ void __launch_bounds__(kBlock)
bn_act_bwd_reduce_vec_kernel(const void* __restrict__ x,
                             const void* __restrict__ res,
                             const void* __restrict__ gy,
                             const float* __restrict__ mean,
                             const float* __restrict__ invstd,
                             const float* __restrict__ gamma,
                             const float* __restrict__ beta,
                             float* __restrict__ out,  // (2,C)
                             int64_t M, int C, int cgv) {
  using Vec = BnVec<T, V>;
  bn_reduce<V, DET, int>(
      C, cgv, out, [&](const auto& lm, float (&db)[V], float (&dg)[V]) {
        const int Cv = C / V;
        const int cb = lm.col() * V;
        float mu[V], is[V], ga[V], be[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          mu[j] = mean[cb + j];
          is[j] = invstd[cb + j];
          ga[j] = gamma[cb + j];
          be[j] = beta[cb + j];
        }
        const Vec* xv = static_cast<const Vec*>(x);
        const Vec* gv = static_cast<const Vec*>(gy);
        const Vec* rv = static_cast<const Vec*>(res);
        const int rstride = lm.rstride();
        auto add_row = [&](const Vec& xval, const Vec& rval, const Vec& gval) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float xh = ((float)xval.v[j] - mu[j]) * is[j];
            float z = xh * ga[j] + be[j];
            if constexpr (ACT == ACT_ADD_RELU) z += (float)rval.v[j];
            const float g = (float)gval.v[j] * act_grad_t<ACT>(z);
            db[j] += g;
            dg[j] += g * xh;
          }
        };
        int64_t m = lm.row0();
        if constexpr (U > 1) {
          for (; m + (int64_t)(U - 1) * rstride < M; m += (int64_t)U * rstride) {
            Vec xval[U], gval[U], rval[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int64_t off = (m + (int64_t)u * rstride) * Cv + lm.col();
              xval[u] = xv[off];
              gval[u] = gv[off];
              if constexpr (ACT == ACT_ADD_RELU) rval[u] = rv[off];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) add_row(xval[u], rval[u], gval[u]);
          }
        }
        for (; m < M; m += rstride) {
          const int64_t off = m * Cv + lm.col();
          const Vec xval = xv[off];
          const Vec gval = gv[off];
          Vec rval;
          if constexpr (ACT == ACT_ADD_RELU) rval = rv[off];
          add_row(xval, rval, gval);
        }
      });
}

// ---------------------------------------------------------------------------
// SplitConvBlock join fused into the statistics pass (T = bf16 or fp16):
//   x[bs,p,:] = T(T(y_base[b,p,:] + bias[bs,:]) + y_dec[bs,p,:])
// with bs = b*S + s over rows m = bs*HW + p, plus the per-channel
// (sum, sumsq) of the ROUNDED x — what bn_stats_vec_kernel would read
// back. The two explicit roundings reproduce the eager 16-bit add chain
// bit for bit. (p, bs, b) advance incrementally with the fixed row
// stride, so the loop has no division.
// ---------------------------------------------------------------------------

template <typename T, int V, bool DET>
__global__ void __launch_bounds__(kBlock)
bn_join_stats_vec_kernel(const void* __restrict__ y_dec,
                         const void* __restrict__ y_base,
                         const void* __restrict__ bias, void* __restrict__ x,
                         float* __restrict__ sums,  // (2,C)
                         int64_t M, int HW, int S, int C, int cgv) {
  using Vec = BnVec<T, V>;
  bn_reduce<V, DET, int64_t>(
      C, cgv, sums, [&](const auto& lm, float (&acc)[V], float (&asq)[V]) {
        const int Cv = C / V;
        const Vec* dv = static_cast<const Vec*>(y_dec) + lm.col();
        const Vec* bv = static_cast<const Vec*>(y_base) + lm.col();
        const Vec* pv = static_cast<const Vec*>(bias) + lm.col();
        Vec* xv = static_cast<Vec*>(x) + lm.col();
        const int64_t row0 = lm.row0();
        const int rstride = lm.rstride();
        // row m = bs*HW + p, bs = b*S + s; per-step deltas of (p, s, b)
        const int dq = rstride / HW, dr = rstride % HW;
        const int dq_b = dq / S, dq_s = dq % S;
        int64_t bs = row0 / HW;
        int p = (int)(row0 - bs * HW);
        int64_t b = bs / S;
        int s = (int)(bs - b * S);
        for (int64_t m = row0; m < M; m += rstride) {
          const Vec dval = dv[m * Cv];
          const Vec bval = bv[(b * HW + p) * Cv];
          const Vec pval = pv[bs * Cv];
          Vec out;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T yb = (T)((float)bval.v[j] + (float)pval.v[j]);
            const T xo = (T)((float)yb + (float)dval.v[j]);
            out.v[j] = xo;
            const float f = (float)xo;
            acc[j] += f;
            asq[j] += f * f;
          }
          xv[m * Cv] = out;
          p += dr;
          const int carry = p >= HW ? 1 : 0;
          p -= carry ? HW : 0;
          bs += dq + carry;
          s += dq_s + carry;  // < 2*S: at most one wrap
          b += dq_b;
          if (s >= S) {
            s -= S;
            ++b;
          }
        }
      });
}

// ---------------------------------------------------------------------------
// normalize + activation (and the optional residual add), and its backward
// ---------------------------------------------------------------------------

// Rows each thread keeps in flight in the elementwise kernels (loads
// issued first, math after). Chosen from the compiler's register report
// so that bf16 fwd stays at 8 waves/SIMD and dx at 5, as before the
// parameters moved into registers; add_relu carries a third stream and
// 8 more live registers per row, so it does not unroll.
constexpr int fwd_unroll(int act) { return act == ACT_ADD_RELU ? 1 : 3; }
constexpr int dx_unroll(int act) { return act == ACT_ADD_RELU ? 1 : 2; }
// Rows in flight in the small-layer reductions: their few hundred
// workgroups leave the memory parallelism to the thread.
constexpr int red_unroll(int act) { return act == ACT_ADD_RELU ? 2 : 4; }

// Where the normalize / dx kernels get their per-channel sums. WS = false:
// finished values from an earlier launch. WS = true (small-layer path):
// the G partials ws[G][2][C] of a DET reduction, which the workgroup adds
// itself (ws_prologue); the workgroups with blockIdx.x == 0 store the
// finished values, and with them the running statistics and the counter.
template <bool WS>
struct BnFwdStats {
  const float* __restrict__ mean;
  const float* __restrict__ invstd;
};
template <>
struct BnFwdStats<true> {
  const float* __restrict__ ws;
  int G;
  float* __restrict__ mean;          // out, saved for backward
  float* __restrict__ invstd;        // out
  float* __restrict__ running_mean;  // may be null, with running_var
  float* __restrict__ running_var;
  int64_t* __restrict__ num_batches_tracked;  // may be null
  float eps, momentum;
};
template <bool WS>
struct BnBwdSums {
  const float* __restrict__ red;  // (2,C)
};
template <>
struct BnBwdSums<true> {
  const float* __restrict__ ws;
  int G;
  float* __restrict__ red;  // out (2,C)
};

// One entry of the (2, C) sums from its G partials, ascending g: eight
// loads are issued ahead of their adds, the adds stay in order.
__device__ __forceinline__ float ws_sum(const float* __restrict__ p, int G,
                                        int64_t step) {
  float t = 0.0f;
  int g = 0;
  for (; g + 7 < G; g += 8, p += 8 * step) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[u * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) t += v[u];
  }
  for (; g < G; ++g, p += step) t += *p;
  return t;
}

// Prologue of the WS instantiations: the workgroup's nch = ncv*V channels
// of both sums go to s[0..nch) and s[64V..64V+nch), one entry per thread
// and pass, each by ws_sum — an order that depends on G alone. Every
// thread of the block arrives here, idle lanes included; they retire
// after the barrier.
template <int V, typename LM>
__device__ __forceinline__ void ws_prologue(const LM& lm,
                                            const float* __restrict__ ws,
                                            int G, int C,
                                            float (&s)[2 * 64 * V]) {
  const int nch = lm.ncv * V;
  const float* base = ws + lm.c0v * V;
  for (int i = threadIdx.x; i < 2 * nch; i += kBlock) {
    const int which = i >= nch ? 1 : 0;
    const int ci = i - which * nch;
    s[which * 64 * V + ci] = ws_sum(base + which * C + ci, G, 2 * (int64_t)C);
  }
  __syncthreads();
}

template <typename T, int V, int ACT>
__device__ __forceinline__ BnVec<T, V> bn_fwd_vec(
    const BnVec<T, V>& xval, const BnVec<T, V>& rval, const float (&mu)[V],
    const float (&is)[V], const float (&ga)[V], const float (&be)[V]) {
  BnVec<T, V> out;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float z = ((float)xval.v[j] - mu[j]) * is[j] * ga[j] + be[j];
    if constexpr (ACT == ACT_ADD_RELU) z += (float)rval.v[j];
    out.v[j] = (T)act_fwd_t<ACT>(z);
  }
  return out;
}

// also the eval-mode kernel: mean/invstd are then the running statistics
template <typename T, int V, int ACT, int U, bool WS = false>
__global__ void __launch_bounds__(kBlock)
bn_act_fwd_vec_kernel(const void* __restrict__ x, const void* __restrict__ res,
                      const BnFwdStats<WS> st,
                      const float* __restrict__ gamma,
                      const float* __restrict__ beta, void* __restrict__ y,
                      int64_t M, int C, int cgv) {
  using Vec = BnVec<T, V>;
  const int Cv = C / V;
  const LaneMap<int64_t, int64_t> lm(Cv, cgv);
  float mu[V], is[V], ga[V], be[V];
  if constexpr (WS) {
    __shared__ float s_sum[2 * 64 * V];
    ws_prologue<V>(lm, st.ws, st.G, C, s_sum);
    if (!lm.active()) return;
    // the first row of threads of the blockIdx.x == 0 workgroups owns the
    // per-channel outputs
    const bool owner = blockIdx.x == 0 && threadIdx.x < cgv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int cl = lm.lane_cv * V + j;
      const BnMoments mo =
          bn_moments(s_sum[cl], s_sum[64 * V + cl], M, st.eps);
      mu[j] = mo.mu;
      is[j] = mo.invstd;
      if (owner)
        bn_store_channel(mo, lm.col() * V + j, st.mean, st.invstd,
                         st.running_mean, st.running_var, M, st.momentum);
    }
    if (owner && blockIdx.y == 0 && threadIdx.x == 0 &&
        st.num_batches_tracked)
      *st.num_batches_tracked += 1;
  } else {
    if (!lm.active()) return;
  }
  const int cb = lm.col() * V;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if constexpr (!WS) {
      mu[j] = st.mean[cb + j];
      is[j] = st.invstd[cb + j];
    }
    ga[j] = gamma[cb + j];
    be[j] = beta[cb + j];
  }
  const Vec* xv = static_cast<const Vec*>(x) + lm.col();
  const Vec* rv = static_cast<const Vec*>(res) + lm.col();
  Vec* yv = static_cast<Vec*>(y) + lm.col();
  const int64_t rstride = lm.rstride();
  const int64_t step = rstride * Cv;  // vectors between a thread's rows
  int64_t m = lm.row0();
  int64_t off = lm.row0() * Cv;
  for (; m + (U - 1) * rstride < M; m += U * rstride, off += U * step) {
    Vec xval[U], rval[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xval[u] = xv[off + u * step];
    if constexpr (ACT == ACT_ADD_RELU) {
#pragma unroll
      for (int u = 0; u < U; ++u) rval[u] = rv[off + u * step];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      yv[off + u * step] =
          bn_fwd_vec<T, V, ACT>(xval[u], rval[u], mu, is, ga, be);
  }
  for (; m < M; m += rstride, off += step) {
    const Vec xval = xv[off];
    Vec rval;
    if constexpr (ACT == ACT_ADD_RELU) rval = rv[off];
    yv[off] = bn_fwd_vec<T, V, ACT>(xval, rval, mu, is, ga, be);
  }
}

// dx = gamma*invstd * (g' - (dbeta + xhat*dgamma)/M); optional dres = g'
template <typename T, int V, int ACT>
__device__ __forceinline__ void bn_dx_vec(
    const BnVec<T, V>& xval, const BnVec<T, V>& rval, const BnVec<T, V>& gval,
    const float (&mu)[V], const float (&is)[V], const float (&ga)[V],
    const float (&be)[V], const float (&r0)[V], const float (&r1)[V],
    float invM, BnVec<T, V>& dxo, BnVec<T, V>& dro) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float xh = ((float)xval.v[j] - mu[j]) * is[j];
    float z = xh * ga[j] + be[j];
    if constexpr (ACT == ACT_ADD_RELU) z += (float)rval.v[j];
    const float g = (float)gval.v[j] * act_grad_t<ACT>(z);
    if constexpr (ACT == ACT_ADD_RELU) dro.v[j] = (T)g;
    dxo.v[j] = (T)(ga[j] * is[j] * (g - (r0[j] + xh * r1[j]) * invM));
  }
}

template <typename T, int V, int ACT, int U, bool WS = false>
__global__ void __launch_bounds__(kBlock)
bn_act_bwd_dx_vec_kernel(const void* __restrict__ x,
                         const void* __restrict__ res,
                         const void* __restrict__ gy,
                         const float* __restrict__ mean,
                         const float* __restrict__ invstd,
                         const float* __restrict__ gamma,
                         const float* __restrict__ beta,
                         const BnBwdSums<WS> sums,
                         void* __restrict__ dx, void* __restrict__ dres,
                         int64_t M, int C, int cgv) {
  using Vec = BnVec<T, V>;
  const int Cv = C / V;
  const float invM = 1.0f / (float)M;
  const LaneMap<int64_t, int64_t> lm(Cv, cgv);
  float mu[V], is[V], ga[V], be[V], r0[V], r1[V];
  if constexpr (WS) {
    __shared__ float s_sum[2 * 64 * V];
    ws_prologue<V>(lm, sums.ws, sums.G, C, s_sum);
    if (!lm.active()) return;
    const bool owner = blockIdx.x == 0 && threadIdx.x < cgv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int cl = lm.lane_cv * V + j;
      r0[j] = s_sum[cl];
      r1[j] = s_sum[64 * V + cl];
      if (owner) {
        sums.red[lm.col() * V + j] = r0[j];
        sums.red[C + lm.col() * V + j] = r1[j];
      }
    }
  } else {
    if (!lm.active()) return;
  }
  const int cb = lm.col() * V;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[cb + j];
    is[j] = invstd[cb + j];
    ga[j] = gamma[cb + j];
    be[j] = beta[cb + j];
    if constexpr (!WS) {
      r0[j] = sums.red[cb + j];
      r1[j] = sums.red[C + cb + j];
    }
  }
  const Vec* xv = static_cast<const Vec*>(x) + lm.col();
  const Vec* rv = static_cast<const Vec*>(res) + lm.col();
  const Vec* gv = static_cast<const Vec*>(gy) + lm.col();
  Vec* dxv = static_cast<Vec*>(dx) + lm.col();
  Vec* drv = static_cast<Vec*>(dres) + lm.col();
  const int64_t rstride = lm.rstride();
  const int64_t step = rstride * Cv;
  int64_t m = lm.row0();
  int64_t off = lm.row0() * Cv;
  for (; m + (U - 1) * rstride < M; m += U * rstride, off += U * step) {
    Vec xval[U], gval[U], rval[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xval[u] = xv[off + u * step];
      gval[u] = gv[off + u * step];
    }
    if constexpr (ACT == ACT_ADD_RELU) {
#pragma unroll
      for (int u = 0; u < U; ++u) rval[u] = rv[off + u * step];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      Vec dxo, dro;
      bn_dx_vec<T, V, ACT>(xval[u], rval[u], gval[u], mu, is, ga, be, r0, r1,
                           invM, dxo, dro);
      dxv[off + u * step] = dxo;
      if constexpr (ACT == ACT_ADD_RELU) drv[off + u * step] = dro;
    }
  }
  for (; m < M; m += rstride, off += step) {
    const Vec xval = xv[off];
    const Vec gval = gv[off];
    Vec rval, dxo, dro;
    if constexpr (ACT == ACT_ADD_RELU) rval = rv[off];
    bn_dx_vec<T, V, ACT>(xval, rval, gval, mu, is, ga, be, r0, r1, invM, dxo,
                         dro);
    dxv[off] = dxo;
    if constexpr (ACT == ACT_ADD_RELU) drv[off] = dro;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// grid.x caps. The reductions keep 2048 blocks: the cap fixes which rows
// a thread sums, so keeping it keeps the summation grouping, and the
// statistics differ from run to run only by the order of the atomics.
// The elementwise kernels sum nothing, so their grid is free: 1024
// blocks, four on each of the 256 CUs, measured 5-10 % faster than 2048
// on the decoder's 100-805 MB layers (768 level with it, 512 slower).
// max_blocks > 0 forces a smaller grid.x so a test can drive the strided
// row loop and its tail at a small shape.
constexpr int kMaxGridReduce = 2048;
constexpr int kMaxGridStream = 1024;

inline int cap_blocks(int64_t want, int cap, int max_blocks) {
  int64_t g = want < cap ? want : cap;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return (int)(g < 1 ? 1 : g);
}

inline dim3 grid_rows_v(int64_t M, int Cv, int cgv, int cap, int max_blocks) {
  const int rows_per_blk = kBlock / cgv;
  return dim3(
      cap_blocks((M + rows_per_blk - 1) / rows_per_blk, cap, max_blocks),
      (Cv + cgv - 1) / cgv);
}

// Run the statements with V, Cv and cgv bound for (T, C): V is 16 bytes of
// T when C is a multiple of that, else 1.
#define BN_VEC_CASE(VEC, C, ...)    \
  {                                 \
    constexpr int V = VEC;          \
    const int Cv = (C) / V;         \
    const int cgv = chan_group(Cv); \
    __VA_ARGS__;                    \
  }
#define BN_VEC_SWITCH(T, C, ...)                         \
  if ((C) % (16 / (int)sizeof(T)) == 0)                  \
    BN_VEC_CASE(16 / (int)sizeof(T), C, __VA_ARGS__)     \
  else                                                   \
    BN_VEC_CASE(1, C, __VA_ARGS__)

// the host switches on `act` once; the kernels take it as a template
// parameter
#define BN_ACT_SWITCH(act, LAUNCH)                 \
  switch (act) {                                   \
    case ACT_RELU: LAUNCH(ACT_RELU); break;        \
    case ACT_LRELU: LAUNCH(ACT_LRELU); break;      \
    case ACT_ELU: LAUNCH(ACT_ELU); break;          \
    case ACT_ADD_RELU: LAUNCH(ACT_ADD_RELU); break;\
    default: LAUNCH(ACT_NONE); break;              \
  }

// grid.x of the reduction kernels for (M, C): the deterministic mode's
// workspace has that many (2, C) partials.
template <typename T>
int reduce_grid_x(int64_t M, int C, int max_blocks) {
  BN_VEC_SWITCH(
      T, C, return (int)grid_rows_v(M, Cv, cgv, kMaxGridReduce, max_blocks).x)
}

// DET: `sums` is the [grid.x][2][C] workspace (no zero fill needed)
template <typename T, bool DET>
void launch_bn_stats(const void* x, float* sums, int64_t M, int C,
                     int max_blocks, hipStream_t s) {
  BN_VEC_SWITCH(
      T, C,
      hipLaunchKernelGGL(
          (bn_stats_vec_kernel<T, V, DET>),
          grid_rows_v(M, Cv, cgv, kMaxGridReduce, max_blocks), dim3(kBlock), 0,
          s, x, sums, M, C, cgv))
}

template <typename T>
void launch_bn_act_fwd(const void* x, const void* res, const float* mean,
                       const float* invstd, const float* gamma,
                       const float* beta, void* y, int64_t M, int C, int act,
                       int max_blocks, hipStream_t s) {
#define BN_LAUNCH(A)                                                          \
  hipLaunchKernelGGL((bn_act_fwd_vec_kernel<T, V, A, fwd_unroll(A)>),         \
                     grid_rows_v(M, Cv, cgv, kMaxGridStream, max_blocks),     \
                     dim3(kBlock), 0, s, x, res,                              \
                     BnFwdStats<false>{mean, invstd}, gamma, beta, y, M, C,   \
                     cgv)
  BN_VEC_SWITCH(T, C, BN_ACT_SWITCH(act, BN_LAUNCH))
#undef BN_LAUNCH
}

// DET: `out` is the [grid.x][2][C] workspace
template <typename T, bool DET>
void launch_bn_act_bwd_reduce(const void* x, const void* res, const void* gy,
                              const float* mean, const float* invstd,
                              const float* gamma, const float* beta,
                              float* out, int64_t M, int C, int act,
                              int max_blocks, hipStream_t s) {
#define BN_LAUNCH(A)                                                       \
  hipLaunchKernelGGL((bn_act_bwd_reduce_vec_kernel<T, V, A, DET>),         \
                     grid_rows_v(M, Cv, cgv, kMaxGridReduce, max_blocks),  \
                     dim3(kBlock), 0, s, x, res, gy, mean, invstd, gamma,  \
                     beta, out, M, C, cgv)
  BN_VEC_SWITCH(T, C, BN_ACT_SWITCH(act, BN_LAUNCH))
#undef BN_LAUNCH
}

template <typename T>
void launch_bn_act_bwd_dx(const void* x, const void* res, const void* gy,
                          const float* mean, const float* invstd,
                          const float* gamma, const float* beta,
                          const float* red, void* dx, void* dres, int64_t M,
                          int C, int act, int max_blocks, hipStream_t s) {
#define BN_LAUNCH(A)                                                        \
  hipLaunchKernelGGL((bn_act_bwd_dx_vec_kernel<T, V, A, dx_unroll(A)>),     \
                     grid_rows_v(M, Cv, cgv, kMaxGridStream, max_blocks),   \
                     dim3(kBlock), 0, s, x, res, gy, mean, invstd, gamma,   \
                     beta, BnBwdSums<false>{red}, dx, dres, M, C, cgv)
  BN_VEC_SWITCH(T, C, BN_ACT_SWITCH(act, BN_LAUNCH))
#undef BN_LAUNCH
}

// x = T(T(y_base + bias) + y_dec) and its (sum, sumsq); C % 8 == 0
template <typename T, bool DET>
void launch_bn_join_stats(const void* y_dec, const void* y_base,
                          const void* bias, void* x, float* sums, int64_t M,
                          int HW, int S, int C, int max_blocks,
                          hipStream_t s) {
  BN_VEC_CASE(
      8, C,
      hipLaunchKernelGGL(
          (bn_join_stats_vec_kernel<T, V, DET>),
          grid_rows_v(M, Cv, cgv, kMaxGridReduce, max_blocks), dim3(kBlock), 0,
          s, y_dec, y_base, bias, x, sums, M, HW, S, C, cgv))
}

// ---------------------------------------------------------------------------
// small-layer path: the plan and its four launchers
// ---------------------------------------------------------------------------

// The plan for (M, C) of T, from the sweep in profiles/r14_bn_small.md.
//   G:         a consumer workgroup reads G * 2 * nch * 4 bytes of partials
//              (nch = its channels), so G = budget / (8 * nch): 32 KiB, or
//              64 KiB for tensors of 8 MiB and more, where the reduction
//              needs the workgroups more than the consumer minds the
//              reads. That is 8..128, a multiple of the 8 loads ws_sum
//              keeps in flight.
//   reduction: channel chunks of 4 vectors (64 bytes of a row) on
//              blockIdx.y, which gives the few partial rows the most
//              workgroups; wider where a thread would be left without a
//              row, and G halved where even that leaves it none.
//   consumer:  today's lane map, kSmallRows rows per thread, at most
//              kSmallMaxConsumers workgroups in all.
// "small" is the size rule alone: every encoder, neck and first-decoder
// shape up to 12.6 MB beats today's path by 1.5-4x in device time; beyond
// kSmallMaxBytes the plan is unmeasured and today's path stays.
constexpr int kSmallRows = 4;
constexpr int kSmallMaxConsumers = 1024;
constexpr int kSmallPrologueBytes = 32 << 10;
constexpr int64_t kSmallWideBytes = (int64_t)8 << 20;  // budget doubles
constexpr int kSmallMinCgv = 4;
constexpr int64_t kSmallMaxBytes = (int64_t)16 << 20;
constexpr int kSmallMaxG = 4096;  // what a forced G may ask for

struct BnSmallPlan {
  bool small;
  int G, cgv, grid_x;
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T>
BnSmallPlan small_plan(int64_t M, int C) {
  BN_VEC_SWITCH(T, C, {
    const int64_t bytes = M * C * (int64_t)sizeof(T);
    const int nch = (Cv < cgv ? Cv : cgv) * V;
    const int budget =
        kSmallPrologueBytes * (bytes >= kSmallWideBytes ? 2 : 1);
    int G = budget / (8 * nch);
    G = G < 1 ? 1 : G;
    int rc = cgv < kSmallMinCgv ? cgv : kSmallMinCgv;
    while (rc < cgv && M < (int64_t)G * (kBlock / rc)) rc <<= 1;
    while (G > 1 && M < (int64_t)G * (kBlock / rc)) G >>= 1;
    int64_t consumers = ceil_div(M * Cv, (int64_t)kBlock * kSmallRows);
    consumers = consumers < kSmallMaxConsumers ? consumers : kSmallMaxConsumers;
    const int64_t gx = consumers / ceil_div(Cv, cgv);
    return BnSmallPlan{bytes <= kSmallMaxBytes, G, rc,
                       (int)(gx < 1 ? 1 : gx)};
  })
}

// grid (G, channel chunks of cgv_r vectors): ws[G][2][C], unfilled
template <typename T>
void launch_bn_stats_partials(const void* x, float* ws, int64_t M, int C,
                              int G, int cgv_r, hipStream_t s) {
  BN_VEC_SWITCH(
      T, C,
      hipLaunchKernelGGL((bn_stats_vec_kernel<T, V, true, 4>),
                         dim3(G, (Cv + cgv_r - 1) / cgv_r), dim3(kBlock), 0, s,
                         x, ws, M, C, cgv_r))
}

template <typename T>
void launch_bn_act_fwd_ws(const void* x, const void* res,
                          const BnFwdStats<true>& st, const float* gamma,
                          const float* beta, void* y, int64_t M, int C,
                          int act, int grid_x, hipStream_t s) {
#define BN_LAUNCH(A)                                                       \
  hipLaunchKernelGGL((bn_act_fwd_vec_kernel<T, V, A, fwd_unroll(A), true>), \
                     dim3(grid_x, (Cv + cgv - 1) / cgv), dim3(kBlock), 0, s, \
                     x, res, st, gamma, beta, y, M, C, cgv)
  BN_VEC_SWITCH(T, C, BN_ACT_SWITCH(act, BN_LAUNCH))
#undef BN_LAUNCH
}

template <typename T>
void launch_bn_act_bwd_reduce_partials(const void* x, const void* res,
                                       const void* gy, const float* mean,
                                       const float* invstd,
                                       const float* gamma, const float* beta,
                                       float* ws, int64_t M, int C, int act,
                                       int G, int cgv_r, hipStream_t s) {
#define BN_LAUNCH(A)                                                         \
  hipLaunchKernelGGL(                                                        \
      (bn_act_bwd_reduce_vec_kernel<T, V, A, true, red_unroll(A)>),          \
      dim3(G, (Cv + cgv_r - 1) / cgv_r), dim3(kBlock), 0, s, x, res, gy,     \
      mean, invstd, gamma, beta, ws, M, C, cgv_r)
  BN_VEC_SWITCH(T, C, BN_ACT_SWITCH(act, BN_LAUNCH))
#undef BN_LAUNCH
}

template <typename T>
void launch_bn_act_bwd_dx_ws(const void* x, const void* res, const void* gy,
                             const float* mean, const float* invstd,
                             const float* gamma, const float* beta,
                             const BnBwdSums<true>& sums, void* dx, void* dres,
                             int64_t M, int C, int act, int grid_x,
                             hipStream_t s) {
#define BN_LAUNCH(A)                                                          \
  hipLaunchKernelGGL(                                                         \
      (bn_act_bwd_dx_vec_kernel<T, V, A, dx_unroll(A), true>),                \
      dim3(grid_x, (Cv + cgv - 1) / cgv), dim3(kBlock), 0, s, x, res, gy,     \
      mean, invstd, gamma, beta, sums, dx, dres, M, C, cgv)
  BN_VEC_SWITCH(T, C, BN_ACT_SWITCH(act, BN_LAUNCH))
#undef BN_LAUNCH
}

// a power of two in [1, 64]
inline bool valid_cgv(int cgv) {
  return cgv >= 1 && cgv <= 64 && (cgv & (cgv - 1)) == 0;
}
inline bool valid_grid(int g) { return g >= 1 && g <= kSmallMaxG; }
// the channel chunks of a reduction fit grid.y (Cv <= C)
inline bool valid_chunks(int C, int cgv) { return C / cgv < 65535; }

}  // namespace

extern "C" int mine_bn_small_plan(int64_t M, int C, int elem, int* G, int* cgv,
                                  int* grid_x) {
  BnSmallPlan p{};
  MINE_ELEM_SWITCH(elem, p = small_plan<T>(M, C))
  *G = p.G;
  *cgv = p.cgv;
  *grid_x = p.grid_x;
  return p.small ? 1 : 0;
}

extern "C" int mine_bn_stats_partials(const void* x, float* ws, int64_t M,
                                      int C, int G, int cgv, int elem,
                                      hipStream_t s) {
  if (!valid_grid(G) || !valid_cgv(cgv) || !valid_chunks(C, cgv))
    return kNoKernel;
  MINE_ELEM_SWITCH(elem, launch_bn_stats_partials<T>(x, ws, M, C, G, cgv, s))
  return kLaunched;
}

extern "C" int mine_bn_act_fwd_ws(const void* x, const void* res,
                                  const float* ws, int G, const float* gamma,
                                  const float* beta, void* y, float* mean,
                                  float* invstd, float* running_mean,
                                  float* running_var,
                                  int64_t* num_batches_tracked, int64_t M,
                                  int C, int act, int grid_x, float eps,
                                  float momentum, int elem, hipStream_t s) {
  if (!valid_grid(G) || !valid_grid(grid_x)) return kNoKernel;
  const BnFwdStats<true> st{ws,           G,           mean,
                            invstd,       running_mean, running_var,
                            num_batches_tracked, eps,  momentum};
  MINE_ELEM_SWITCH(elem, launch_bn_act_fwd_ws<T>(x, res, st, gamma, beta, y, M,
                                                 C, act, grid_x, s))
  return kLaunched;
}

extern "C" int mine_bn_act_bwd_reduce_partials(
    const void* x, const void* res, const void* gy, const float* mean,
    const float* invstd, const float* gamma, const float* beta, float* ws,
    int64_t M, int C, int act, int G, int cgv, int elem, hipStream_t s) {
  if (!valid_grid(G) || !valid_cgv(cgv) || !valid_chunks(C, cgv))
    return kNoKernel;
  MINE_ELEM_SWITCH(elem, launch_bn_act_bwd_reduce_partials<T>(
                             x, res, gy, mean, invstd, gamma, beta, ws, M, C,
                             act, G, cgv, s))
  return kLaunched;
}

extern "C" int mine_bn_act_bwd_dx_ws(const void* x, const void* res,
                                     const void* gy, const float* mean,
                                     const float* invstd, const float* gamma,
                                     const float* beta, const float* ws, int G,
                                     float* red, void* dx, void* dres,
                                     int64_t M, int C, int act, int grid_x,
                                     int elem, hipStream_t s) {
  if (!valid_grid(G) || !valid_grid(grid_x)) return kNoKernel;
  const BnBwdSums<true> sums{ws, G, red};
  MINE_ELEM_SWITCH(elem, launch_bn_act_bwd_dx_ws<T>(x, res, gy, mean, invstd,
                                                    gamma, beta, sums, dx,
                                                    dres, M, C, act, grid_x,
                                                    s))
  return kLaunched;
}

extern "C" int mine_bn_reduce_grid(int64_t M, int C, int max_blocks,
                                   int elem) {
  int grid = kNoKernel;
  MINE_ELEM_SWITCH(elem, grid = reduce_grid_x<T>(M, C, max_blocks))
  return grid;
}

extern "C" int mine_bn_stats(const void* x, float* sums, int64_t M, int C,
                             int max_blocks, int det, int elem,
                             hipStream_t s) {
  MINE_ELEM_SWITCH(
      elem, det ? launch_bn_stats<T, true>(x, sums, M, C, max_blocks, s)
                : launch_bn_stats<T, false>(x, sums, M, C, max_blocks, s))
  return kLaunched;
}

extern "C" int mine_bn_join_stats(const void* y_dec, const void* y_base,
                                  const void* bias, void* x, float* sums,
                                  int64_t M, int HW, int S, int C,
                                  int max_blocks, int det, int elem,
                                  hipStream_t s) {
  MINE_ELEM_SWITCH16(
      elem, det ? launch_bn_join_stats<T, true>(y_dec, y_base, bias, x, sums,
                                                M, HW, S, C, max_blocks, s)
                : launch_bn_join_stats<T, false>(y_dec, y_base, bias, x, sums,
                                                 M, HW, S, C, max_blocks, s))
  return kLaunched;
}

extern "C" int mine_bn_act_fwd(const void* x, const void* res,
                               const float* mean, const float* invstd,
                               const float* gamma, const float* beta, void* y,
                               int64_t M, int C, int act, int max_blocks,
                               int elem, hipStream_t s) {
  MINE_ELEM_SWITCH(elem, launch_bn_act_fwd<T>(x, res, mean, invstd, gamma,
                                              beta, y, M, C, act, max_blocks,
                                              s))
  return kLaunched;
}

extern "C" int mine_bn_act_bwd_reduce(const void* x, const void* res,
                                      const void* gy, const float* mean,
                                      const float* invstd, const float* gamma,
                                      const float* beta, float* out, int64_t M,
                                      int C, int act, int max_blocks, int det,
                                      int elem, hipStream_t s) {
  MINE_ELEM_SWITCH(
      elem, det ? launch_bn_act_bwd_reduce<T, true>(x, res, gy, mean, invstd,
                                                    gamma, beta, out, M, C,
                                                    act, max_blocks, s)
                : launch_bn_act_bwd_reduce<T, false>(x, res, gy, mean, invstd,
                                                     gamma, beta, out, M, C,
                                                     act, max_blocks, s))
  return kLaunched;
}

extern "C" int mine_bn_act_bwd_dx(const void* x, const void* res,
                                  const void* gy, const float* mean,
                                  const float* invstd, const float* gamma,
                                  const float* beta, const float* red,
                                  void* dx, void* dres, int64_t M, int C,
                                  int act, int max_blocks, int elem,
                                  hipStream_t s) {
  MINE_ELEM_SWITCH(elem, launch_bn_act_bwd_dx<T>(x, res, gy, mean, invstd,
                                                 gamma, beta, red, dx, dres, M,
                                                 C, act, max_blocks, s))
  return kLaunched;
}

// deterministic finish over ws[G][2][C]: writes `out` (2,C) if given and
// finalizes into mean/invstd (+ running stats) if given
extern "C" void mine_bn_det_finish(const float* ws, int G, int C, float* out,
                                   float* mean, float* invstd,
                                   float* running_mean, float* running_var,
                                   int64_t M, float eps, float momentum,
                                   hipStream_t s) {
  const int cg = chan_group(C);
  const int cw = cg < 16 ? cg : 16;
  hipLaunchKernelGGL(bn_det_finish_kernel, dim3((C + cw - 1) / cw),
                     dim3(kBlock), 0, s, ws, G, C, cw, out, mean, invstd,
                     running_mean, running_var, M, eps, momentum);
}

extern "C" void mine_bn_finalize(const float* sums, float* mean, float* invstd,
                                 float* running_mean, float* running_var,
                                 int64_t M, int C, float eps, float momentum,
                                 hipStream_t s) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, s, sums, mean, invstd, running_mean,
                     running_var, M, C, eps, momentum);
}
