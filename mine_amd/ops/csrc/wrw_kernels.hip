// Weight gradient (wrw) of the fused reflect-pad 3x3 conv, with the bias
// gradient in the same pass:
//   dW[k, c, dy, dx] = sum_{n,y,x} gy[n,y,x,k] * xpad[n, y+dy, x+dx, c]
//   db[k]            = sum_{n,y,x} gy[n,y,x,k]
// as a GEMM with M = K (out-channels), N = 9*C taps, contraction over
// the pixels, on v_mfma_f32_16x16x32_bf16 or _f16 (the element type is a
// template parameter, elem16.h; the kernel moves raw 16-bit words, so only
// the MFMA and the 1.0 of the bias sum depend on it).
//
// v3 design: every tensor is read once and the work is split by output,
// not by contraction.
//
//  * Grid = (pixel slabs, K/64 blocks). A workgroup owns a slab of image
//    rows and accumulates the whole (16*KT k) x (9 * 16*CT c) partial
//    for it in registers; KT, CT are template parameters, so every
//    accumulator index is a compile-time constant.
//  * Waves split the output tiles where there are enough of them
//    (CT = 2: two c-groups x two pixel halves; CT = 4: one c-group per
//    wave, all waves walk the same pixels), and the pixels otherwise.
//  * Row bands with a rolling halo: a step brings R = 2 new gy rows and
//    R new x rows into LDS. The x rows live in a ring of R + 2 slots
//    indexed by the padded row number, so each x row is staged once and
//    serves all three dy taps. A slab (or an image inside a slab)
//    starts with one load-only step that brings the first two x rows.
//  * The next step's global loads are issued into registers BEFORE the
//    current step is contracted and are written to LDS after it, so
//    they are in flight under the MFMAs.
//  * One LDS image per operand: plain [pixel][16 ch] rows of 32 B, with
//    the two 128-B halves of every odd 256-B block swapped,
//        byte(j) = 32 * (j ^ ((j >> 1) & 4)).
//    ds_read_b64_tr_b16 takes a row address from every lane, so the dx
//    tap is a per-lane address offset and no shifted copy exists. The
//    swap makes the two 16-lane groups of a 32-lane half land on
//    disjoint banks for dx = 0, 1, 2 (replayed in
//    tests/test_wrw_lds_sim.py).
//  * K = 4 is staged with 8-byte loads into the zero-padded 16-channel
//    rows. There is no per-element load.
//  * No atomics: each workgroup stores its partial, accumulator by
//    accumulator as contiguous 1-KiB wave stores, into a
//    [slab][k block][record][lane] workspace; conv3x3_wrw_finish_kernel
//    sums the slabs in a fixed order and scatters into (K, C, 3, 3).
//    dW and db are therefore bitwise reproducible.
//
// Supported: C % 16 == 0 and C <= 64; gy channel stride 4 or a multiple
// of 8 (the binding pads anything else); any W >= 2, H >= 2.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "elem16.h"
#include "launchers.h"

namespace {

using elem16::Elem16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using s16x4 = __attribute__((ext_vector_type(4))) short;
using s16x8 = __attribute__((ext_vector_type(8))) short;
using lds_char = __attribute__((address_space(3))) unsigned char;
using lds_s16x4 = __attribute__((address_space(3))) s16x4;
using lds_s16x8 = __attribute__((address_space(3))) s16x8;
using lds_f32x4 = __attribute__((address_space(3))) f32x4;

constexpr int kBlock = 256;
constexpr int R = 2;               // gy rows per step
constexpr int XSLOTS = R + 2;      // ring of x rows, slot = padded row & 3
constexpr int TW_ALL = 384;        // pixels per row tile at CT = KT = 1

template <int CT, int KT>
struct Cfg {
  static constexpr int TW = TW_ALL / (CT > KT ? CT : KT);  // tile width
  // bytes per 16-channel sub-image of one row; both strides are
  // 32 mod 128 so the 16-B staging stores of one pixel's sub-images
  // fall on different banks
  static constexpr int XS = (TW + 9) * 32;   // pixels -1 .. TW (+ swap room)
  static constexpr int GS = (TW + 1) * 32;
  static constexpr int XROW = CT * XS;
  static constexpr int GROW = KT * GS;
  static constexpr int X_BYTES = XSLOTS * XROW;
  static constexpr int STAGE_BYTES = X_BYTES + R * GROW;
  static constexpr int NWC = CT == 3 ? 1 : CT;  // waves across c-groups
  static constexpr int CPW = CT / NWC;          // c-groups per wave
  static constexpr int NWP = 4 / NWC;           // waves across pixels
  static constexpr int NTILE = CT * KT;
  static constexpr int NREC = NTILE * 9 + KT;   // f32x4-per-lane records
  static constexpr int RED_BYTES = NWP > 1 ? NREC * 1024 : 0;
  static constexpr int LDS_BYTES =
      STAGE_BYTES > RED_BYTES ? STAGE_BYTES : RED_BYTES;
  static constexpr int XVPR = ((TW + 2) * 2 * CT + kBlock - 1) / kBlock;
  static constexpr int GVPR = (TW * 2 * KT + kBlock - 1) / kBlock;
  static constexpr int G4VPR = (TW + kBlock - 1) / kBlock;
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
  static_assert(TW % 32 == 0, "a tile is whole 32-pixel chunks");
};

__device__ __forceinline__ int reflect1(int v, int n) {
  if (v < 0) v = -v;
  if (v >= n) v = 2 * (n - 1) - v;
  return v;
}

// pixel slot inside a sub-image: the halves of odd 8-pixel blocks swap
__device__ __forceinline__ int swz(int j) { return j ^ ((j >> 1) & 4); }

// One MFMA operand (16 channels x 32 pixels) by two transpose reads.
// ds_read_b64_tr_b16 has no internal lane offset: lane 4q+p of a
// 16-lane group passes the address of pixel q, channels 4p..4p+3, and
// lane i gets channel i of the four pixels. o0 / o1 are the lane's
// addresses for pixels 8g+q and 8g+q+4. EXEC must be all ones here.
template <typename F8>
__device__ __forceinline__ F8 tr2(lds_char* base, int o0, int o1) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o0));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o1));
  s16x8 s = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(F8, s);
}

// One step of the slab walk: nxr new x rows (padded rows py0 ..) and
// ngr gy rows (y0 ..) of image n. nxr == 0 marks the end.
struct Step {
  int n, y0, ngr, py0, nxr;
};

template <typename T, int CT, int KT, bool K4>
__global__ void __launch_bounds__(kBlock)
conv3x3_wrw_kernel(const short* __restrict__ x,    // (N,H,W,C) as T
                   const short* __restrict__ gy,   // (N,H,W,Kmem) as T
                   float* __restrict__ ws, int N, int H, int W, int Kmem,
                   int n_slabs, int want_bias) {
  using E = Elem16<T>;
  using frag8 = typename E::frag8;
  using G = Cfg<CT, KT>;
  constexpr int C = 16 * CT;
  constexpr int TW = G::TW;
  constexpr int NGV = K4 ? G::G4VPR : G::GVPR;
  __shared__ __attribute__((aligned(256))) unsigned char lds_raw[G::LDS_BYTES];
  lds_char* lds = (lds_char*)lds_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cw = wave % G::NWC;   // first c-group of this wave
  const int wp = wave / G::NWC;   // pixel share of this wave
  const int slab = (int)blockIdx.x;
  const int kb0 = (int)blockIdx.y * KT * 16;
  const int64_t rows_total = (int64_t)N * H;
  const int64_t r_begin = rows_total * slab / n_slabs;
  const int64_t r_end = rows_total * (slab + 1) / n_slabs;

  // channels 4..15 of a 4-channel gy are never staged: they stay zero
  // from this fill (the 16-byte path writes its padding octets as zeros)
  for (int i = tid * 16; i < G::LDS_BYTES; i += kBlock * 16)
    *(lds_s16x8*)(lds + i) = s16x8{0, 0, 0, 0, 0, 0, 0, 0};

  // per-lane transpose-read offsets for the three dx taps
  int loff[3][2];
  {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        loff[dx][h] = swz(8 * g + q + 4 * h + dx) * 32 + p * 8;
  }

  f32x4 acc[G::CPW][KT][9];
  f32x4 accb[KT];
#pragma unroll
  for (int a = 0; a < G::CPW; ++a)
#pragma unroll
    for (int b = 0; b < KT; ++b)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[a][b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < KT; ++b) accb[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const short one = E::kOne;  // 1.0 as T
  const frag8 ones = __builtin_bit_cast(
      frag8, (s16x8{one, one, one, one, one, one, one, one}));

  s16x8 xv[R * G::XVPR];
  s16x8 gv[R * NGV];

  for (int x0 = 0; x0 < W; x0 += TW) {
    const int Wt = (W - x0) < TW ? (W - x0) : TW;
    const int nch = (Wt + 31) >> 5;     // 32-pixel chunks per row
    const int gpmax = nch * 32;         // gy pixels staged (tail zeroed)
    const int jmax = gpmax + 1;         // last x position read

    int64_t grow = r_begin;
    bool cont = false;                  // the ring holds this image's halo
    auto next_step = [&]() -> Step {
      Step s{0, 0, 0, 0, 0};
      if (grow >= r_end) return s;
      const int n = (int)(grow / H);
      const int y = (int)(grow - (int64_t)n * H);
      if (!cont) {
        s = Step{n, y, 0, y, 2};
        cont = true;
      } else {
        int nr = H - y < R ? H - y : R;
        if (r_end - grow < nr) nr = (int)(r_end - grow);
        s = Step{n, y, nr, y + 2, nr};
        grow += nr;
        if (y + nr == H) cont = false;
      }
      return s;
    };

    auto issue = [&](const Step& s) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < s.nxr) {
          const int yy = reflect1(s.py0 + r - 1, H);
          const short* rowp = x + ((int64_t)s.n * H + yy) * W * C;
#pragma unroll
          for (int v = 0; v < G::XVPR; ++v) {
            const int idx = tid + kBlock * v;
            const int oct = idx % (2 * CT), j = idx / (2 * CT);
            if (j <= jmax) {
              int u = reflect1(x0 + j - 1, W);   // past the tail: any pixel
              u = u < 0 ? 0 : (u > W - 1 ? W - 1 : u);
              xv[r * G::XVPR + v] =
                  *reinterpret_cast<const s16x8*>(rowp + u * C + oct * 8);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < s.ngr) {
          const short* rowp =
              gy + (((int64_t)s.n * H + s.y0 + r) * W + x0) * Kmem + kb0;
#pragma unroll
          for (int v = 0; v < NGV; ++v) {
            const int idx = tid + kBlock * v;
            s16x8 val{0, 0, 0, 0, 0, 0, 0, 0};
            if constexpr (K4) {
              if (idx < Wt) {
                const s16x4 t =
                    *reinterpret_cast<const s16x4*>(rowp + idx * 4);
                val[0] = t[0]; val[1] = t[1]; val[2] = t[2]; val[3] = t[3];
              }
            } else {
              const int oct = idx % (2 * KT), pp = idx / (2 * KT);
              if (pp < Wt && kb0 + oct * 8 < Kmem)
                val = *reinterpret_cast<const s16x8*>(rowp + pp * Kmem +
                                                      oct * 8);
            }
            gv[r * NGV + v] = val;
          }
        }
      }
    };

    auto write_lds = [&](const Step& s) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < s.nxr) {
          const int slot = ((s.py0 + r) & (XSLOTS - 1)) * G::XROW;
#pragma unroll
          for (int v = 0; v < G::XVPR; ++v) {
            const int idx = tid + kBlock * v;
            const int oct = idx % (2 * CT), j = idx / (2 * CT);
            if (j <= jmax)
              *(lds_s16x8*)(lds + slot + (oct >> 1) * G::XS + swz(j) * 32 +
                            (oct & 1) * 16) = xv[r * G::XVPR + v];
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < s.ngr) {
          const int slot = G::X_BYTES + r * G::GROW;
#pragma unroll
          for (int v = 0; v < NGV; ++v) {
            const int idx = tid + kBlock * v;
            const s16x8 val = gv[r * NGV + v];
            if constexpr (K4) {
              if (idx < gpmax)
                *(lds_s16x4*)(lds + slot + swz(idx) * 32) =
                    s16x4{val[0], val[1], val[2], val[3]};
            } else {
              const int oct = idx % (2 * KT), pp = idx / (2 * KT);
              if (pp < gpmax)
                *(lds_s16x8*)(lds + slot + (oct >> 1) * G::GS + swz(pp) * 32 +
                              (oct & 1) * 16) = val;
            }
          }
        }
      }
    };

    auto compute = [&](const Step& s) {
      const int units = s.ngr * nch;
      for (int u = wp; u < units; u += G::NWP) {   // wave-uniform
        const int row = u >= nch ? 1 : 0;
        const int ch = u - row * nch;
        const int gbase = G::X_BYTES + row * G::GROW + ch * 1024;
        frag8 a[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
          a[kt] = tr2<frag8>(lds, gbase + kt * G::GS + loff[0][0],
                      gbase + kt * G::GS + loff[0][1]);
        if (want_bias && cw == 0) {
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
            accb[kt] = E::mfma(a[kt], ones, accb[kt]);
        }
        // the three dx operands of one (dy, c-group) are read one
        // group ahead of the MFMAs that use them, so the LDS latency
        // runs under the previous group's MFMAs
        auto load_b = [&](int grp, frag8 (&b)[3]) {
          const int dy = grp / G::CPW, cp = grp % G::CPW;
          const int cbase =
              ((s.y0 + row + dy) & (XSLOTS - 1)) * G::XROW + ch * 1024 +
              (cw + cp * G::NWC) * G::XS;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx)
            b[dx] = tr2<frag8>(lds, cbase + loff[dx][0], cbase + loff[dx][1]);
        };
        frag8 bq[2][3];
        load_b(0, bq[0]);
#pragma unroll
        for (int grp = 0; grp < 3 * G::CPW; ++grp) {
          if (grp + 1 < 3 * G::CPW) load_b(grp + 1, bq[(grp + 1) & 1]);
          const int dy = grp / G::CPW, cp = grp % G::CPW;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
              acc[cp][kt][dy * 3 + dx] = E::mfma(
                  a[kt], bq[grp & 1][dx], acc[cp][kt][dy * 3 + dx]);
        }
      }
    };

    Step cur = next_step();
    issue(cur);
    __syncthreads();      // zero fill / previous tile's reads are done
    write_lds(cur);
    __syncthreads();
    for (;;) {
      const Step nx = next_step();
      const bool more = nx.nxr > 0;
      if (more) issue(nx);     // in flight under the MFMAs below
      compute(cur);
      if (!more) break;
      __syncthreads();
      write_lds(nx);
      __syncthreads();
      cur = nx;
    }
  }

  // ---- partial out: record (ct, kt, tap) then the KT bias records -----
  // A record is one accumulator, 16 B per lane: 1 KiB per wave store.
  // Waves that share tiles (NWP > 1) add up in wave order through LDS.
  f32x4* part = reinterpret_cast<f32x4*>(
      ws + ((int64_t)slab * gridDim.y + blockIdx.y) * (G::NREC * 256));
  lds_f32x4* red = (lds_f32x4*)lds;
#pragma unroll
  for (int turn = 0; turn < G::NWP; ++turn) {
    if (G::NWP > 1) __syncthreads();
    if (wp == turn) {
      auto flush = [&](int rec, f32x4 v) {
        if (turn > 0) v += red[rec * 64 + lane];
        if (turn == G::NWP - 1)
          part[rec * 64 + lane] = v;
        else
          red[rec * 64 + lane] = v;
      };
#pragma unroll
      for (int cp = 0; cp < G::CPW; ++cp)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int t = 0; t < 9; ++t)
            flush(((cw + cp * G::NWC) * KT + kt) * 9 + t, acc[cp][kt][t]);
      if (want_bias && cw == 0) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) flush(G::NTILE * 9 + kt, accb[kt]);
      }
    }
  }
}

// Sums the slab partials in a fixed order (16 interleaved slab groups,
// each in slab order, then the groups in order) and scatters the result
// into dW (K, C, 3, 3) and db (K).
__global__ void __launch_bounds__(kBlock)
conv3x3_wrw_finish_kernel(const float* __restrict__ ws,
                          float* __restrict__ dw, float* __restrict__ db,
                          int n_slabs, int nkb, int CT, int KT, int K,
                          int want_bias) {
  __shared__ f32x4 s_part[16][16];
  const int tid = threadIdx.x;
  const int ev = tid & 15, sg = tid >> 4;
  const int nrec = CT * KT * 9 + KT;
  const int per_kb = nrec * 64;            // f32x4 elements per partial
  const int e = (int)blockIdx.x * 16 + ev;
  const bool in = e < nkb * per_kb;
  const int kb = in ? e / per_kb : 0;
  const int loc = in ? e - kb * per_kb : 0;
  const int rec = loc >> 6, ln = loc & 63;
  const bool is_bias = rec >= CT * KT * 9;
  const bool live = in && (!is_bias || want_bias);
  f32x4 sum{0.f, 0.f, 0.f, 0.f};
  if (live) {
    const f32x4* src = reinterpret_cast<const f32x4*>(ws);
    for (int s = sg; s < n_slabs; s += 16)
      sum += src[((int64_t)s * nkb + kb) * per_kb + loc];
  }
  s_part[sg][ev] = sum;
  __syncthreads();
  if (sg != 0 || !live) return;
  f32x4 tot = s_part[0][ev];
  for (int i = 1; i < 16; ++i) tot += s_part[i][ev];
  const int C = 16 * CT;
  if (!is_bias) {
    const int tile = rec / 9, tap = rec - tile * 9;
    const int ct = tile / KT, kt = tile - ct * KT;
    const int c = ct * 16 + (ln & 15);
    for (int r = 0; r < 4; ++r) {
      const int k = (kb * KT + kt) * 16 + (ln >> 4) * 4 + r;
      if (k < K) dw[((int64_t)k * C + c) * 9 + tap] = tot[r];
    }
  } else if ((ln & 15) == 0) {
    const int kt = rec - CT * KT * 9;
    for (int r = 0; r < 4; ++r) {
      const int k = (kb * KT + kt) * 16 + (ln >> 4) * 4 + r;
      if (k < K) db[k] = tot[r];
    }
  }
}

// k tiles per workgroup for a gy channel stride of Kmem
int kt_for(int CT, int Kmem) {
  const int need = (Kmem + 15) / 16;
  int kt = need <= 1 ? 1 : (need <= 2 ? 2 : 4);
  if (CT == 3 && kt > 2) kt = 2;   // 3 c-groups per wave: 54 accumulators
  return kt;
}

}  // namespace

// Slab count, k blocks and workspace floats for one call. max_slabs = 0:
// one slab per workgroup that is resident at once on 256 CUs -- two per
// CU, one where 36 or more accumulators per wave leave room for one wave
// per SIMD (c-groups per wave x KT >= 4: <1,4>, <2,4>, <3,2>, <4,4>) --
// so no workgroup waits for a CU and the workspace stays small.
extern "C" void mine_conv3x3_wrw_plan(int C, int Kmem, int64_t rows,
                                      int max_slabs, int* slabs, int* nkb,
                                      int64_t* ws_floats) {
  const int CT = C / 16, KT = kt_for(CT, Kmem);
  const int cpw = CT == 3 ? 3 : 1;
  int s = max_slabs > 0 ? max_slabs : (cpw * KT >= 4 ? 256 : 512);
  if ((int64_t)s > rows) s = (int)rows;
  *slabs = s;
  *nkb = ((Kmem + 15) / 16 + KT - 1) / KT;
  *ws_floats = (int64_t)s * *nkb * (CT * KT * 9 + KT) * 256;
}

namespace {
template <typename T>
void wrw_launch_t(const short* xs, const short* gs, float* ws, int N, int H,
                  int W, int Kmem, int CT, int KT, bool k4, dim3 grid,
                  int slabs, int wb, hipStream_t stream) {
#define WRW_LAUNCH(ct, kt, k4v)                                              \
  hipLaunchKernelGGL((conv3x3_wrw_kernel<T, ct, kt, k4v>), grid,             \
                     dim3(kBlock), 0, stream, xs, gs, ws, N, H, W, Kmem,     \
                     slabs, wb)
#define WRW_CT(ct)                                                           \
  if (k4) WRW_LAUNCH(ct, 1, true);                                           \
  else if (KT == 1) WRW_LAUNCH(ct, 1, false);                                \
  else if (KT == 2) WRW_LAUNCH(ct, 2, false);                                \
  else WRW_LAUNCH(ct, (ct == 3 ? 2 : 4), false)
  switch (CT) {
    case 1: WRW_CT(1); break;
    case 2: WRW_CT(2); break;
    case 3: WRW_CT(3); break;
    default: WRW_CT(4); break;
  }
#undef WRW_CT
#undef WRW_LAUNCH
}
}  // namespace

// x (N,H,W,C), gy (N,H,W,Kmem), both of type `elem` (bf16 or fp16) -> dw
// (K,C,3,3) fp32 and, where db is not null, db (K) fp32. Kmem is 4 or a
// multiple of 8 with Kmem >= K; ws comes from mine_conv3x3_wrw_plan.
// Returns kNoKernel if there is no kernel for (C, Kmem) or the type.
extern "C" int mine_conv3x3_wrw(const void* x, const void* gy, float* ws,
                                float* dw, float* db, int N, int H, int W,
                                int C, int Kmem, int K, int slabs, int elem,
                                hipStream_t stream) {
  if (C % 16 != 0 || C < 16 || C > 64) return kNoKernel;
  if (Kmem != 4 && Kmem % 8 != 0) return kNoKernel;
  const int CT = C / 16, KT = kt_for(CT, Kmem);
  const bool k4 = Kmem == 4;
  const int nkb = ((Kmem + 15) / 16 + KT - 1) / KT;
  const dim3 grid(slabs, nkb);
  const short* xs = reinterpret_cast<const short*>(x);
  const short* gs = reinterpret_cast<const short*>(gy);
  const int wb = db != nullptr;
  MINE_ELEM_SWITCH16(elem, wrw_launch_t<T>(xs, gs, ws, N, H, W, Kmem, CT, KT,
                                           k4, grid, slabs, wb, stream))
  // a refused launch stays pending for the caller's status check; the
  // finish would only sum an unwritten workspace
  if (hipPeekAtLastError() != hipSuccess) return kLaunched;
  const int n_vec = nkb * (CT * KT * 9 + KT) * 64;
  hipLaunchKernelGGL(conv3x3_wrw_finish_kernel, dim3((n_vec + 15) / 16),
                     dim3(kBlock), 0, stream, ws, dw, db, slabs, nkb, CT, KT,
                     K, wb);
  return kLaunched;
}
