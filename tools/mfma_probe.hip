// MFMA fragment-layout probe for v_mfma_f32_16x16x32_bf16 and
// v_mfma_f32_16x16x32_f16 (gfx950).
//
// Empirically determines the lane/element -> (row, k) mapping of the A
// and B operands: each of the 64x8 (lane, element) slots is set to a
// one-hot in turn against an all-ones other operand; the fired D row
// (C/D map is documented: row = (lane>>4)*4 + reg, col = lane&15) gives
// A's row map; pairing one-hot A against one-hot B gives the k
// equivalence classes. Output: two 64x8 int tables (row/k for A, col/k
// for B) per element type, printed by main(), which also says whether
// the f16 maps equal the bf16 ones (the pack LUTs of mine_amd/ops/conv.py
// and conv_general.py are shared between the two only if they do).
//
//   hipcc --offload-arch=gfx950 -O2 tools/mfma_probe.hip -o tools/mfma_probe

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdio>
#include <cstring>

#include "../mine_amd/ops/csrc/elem16.h"

namespace {

using elem16::Elem16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <typename T>
__device__ inline typename Elem16<T>::frag8 make_onehot(int lane, int elem,
                                                        int my_lane) {
  typename Elem16<T>::frag8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    v[e] = (typename Elem16<T>::raw)((my_lane == lane && e == elem) ? 1.0f
                                                                    : 0.0f);
  return v;
}

template <typename T>
__device__ inline typename Elem16<T>::frag8 make_ones() {
  typename Elem16<T>::frag8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (typename Elem16<T>::raw)1.0f;
  return v;
}

// out_a: 64x8 rows of A; out_b: 64x8 cols of B;
// out_ka: 64x8 k-class of A elems (index into lane0..3 x elem of B basis)
template <typename T>
__global__ void probe_kernel(int* out_a_row, int* out_b_col, int* out_k) {
  using E = Elem16<T>;
  using frag8 = typename E::frag8;
  const int lane = threadIdx.x;  // one wave
  const frag8 ones = make_ones<T>();

  for (int l = 0; l < 64; ++l) {
    for (int e = 0; e < 8; ++e) {
      // ---- A one-hot vs B ones: D[i][*] = 1 at i = row(l,e)
      frag8 a = make_onehot<T>(l, e, lane);
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
      d = E::mfma(a, ones, d);
      // lane holds D rows (lane>>4)*4+r, col lane&15
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (d[r] > 0.5f && (lane & 15) == 0) {
          out_a_row[l * 8 + e] = (lane >> 4) * 4 + r;
        }
      }
      // ---- A ones vs B one-hot: D[*][j] = 1 at j = col(l,e)
      frag8 b = make_onehot<T>(l, e, lane);
      f32x4 d2 = {0.f, 0.f, 0.f, 0.f};
      d2 = E::mfma(ones, b, d2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (d2[r] > 0.5f && ((lane >> 4) * 4 + r) == 0) {
          out_b_col[l * 8 + e] = lane & 15;
        }
      }
      // ---- k-class: A one-hot (l,e) vs B one-hot basis (lb in row-group
      // {0,16,32,48}, eb 0..7): fires iff k_A(l,e) == k_B(lb,eb).
      for (int g = 0; g < 4; ++g) {
        const int lb = g * 16;  // B lanes 0,16,32,48 share col j=0
        for (int eb = 0; eb < 8; ++eb) {
          frag8 b1 = make_onehot<T>(lb, eb, lane);
          f32x4 d3 = {0.f, 0.f, 0.f, 0.f};
          d3 = E::mfma(a, b1, d3);
          float any = d3[0] + d3[1] + d3[2] + d3[3];
          // reduce across the wave: if ANY lane saw a hit, classes match
          any = __shfl(any, 0) + __shfl(any, 16) + __shfl(any, 32) +
                __shfl(any, 48);
          // cheap wave-or: use ballot on the local value
          const unsigned long long m =
              __ballot(d3[0] + d3[1] + d3[2] + d3[3] > 0.5f);
          if (m != 0ull && lane == 0) {
            out_k[l * 8 + e] = g * 8 + eb;  // k-class id of basis slot
          }
        }
      }
    }
  }
}

// runs the probe for one element type; fills ha / hb / hk (512 ints each)
template <typename T>
int run_probe(const char* name, int* ha, int* hb, int* hk) {
  int *a_row, *b_col, *k_class;
  const size_t bytes = 64 * 8 * sizeof(int);
  if (hipMalloc(&a_row, bytes) != hipSuccess ||
      hipMalloc(&b_col, bytes) != hipSuccess ||
      hipMalloc(&k_class, bytes) != hipSuccess)
    return 1;
  (void)hipMemset(a_row, 0xff, bytes);
  (void)hipMemset(b_col, 0xff, bytes);
  (void)hipMemset(k_class, 0xff, bytes);
  hipLaunchKernelGGL(probe_kernel<T>, dim3(1), dim3(64), 0, 0, a_row, b_col,
                     k_class);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  (void)hipMemcpy(ha, a_row, bytes, hipMemcpyDeviceToHost);
  (void)hipMemcpy(hb, b_col, bytes, hipMemcpyDeviceToHost);
  (void)hipMemcpy(hk, k_class, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(a_row);
  (void)hipFree(b_col);
  (void)hipFree(k_class);
  printf("== %s ==\nA row map (lane e0..e7):\n", name);
  for (int l = 0; l < 64; ++l) {
    printf("lane %2d:", l);
    for (int e = 0; e < 8; ++e) printf(" %2d", ha[l * 8 + e]);
    printf("   k-class:");
    for (int e = 0; e < 8; ++e) printf(" %2d", hk[l * 8 + e]);
    printf("\n");
  }
  printf("B col map (lane e0..e7):\n");
  for (int l = 0; l < 64; ++l) {
    printf("lane %2d:", l);
    for (int e = 0; e < 8; ++e) printf(" %2d", hb[l * 8 + e]);
    printf("\n");
  }
  return 0;
}

// the map the kernels assume: row/col = lane & 15, k = (lane>>4)*8 + e
bool is_expected(const int* ha, const int* hb, const int* hk) {
  for (int l = 0; l < 64; ++l)
    for (int e = 0; e < 8; ++e)
      if (ha[l * 8 + e] != (l & 15) || hb[l * 8 + e] != (l & 15) ||
          hk[l * 8 + e] != (l >> 4) * 8 + e)
        return false;
  return true;
}

}  // namespace

int main() {
  static int a0[512], b0[512], k0[512], a1[512], b1[512], k1[512];
  if (run_probe<__hip_bfloat16>("bf16", a0, b0, k0)) return 1;
  if (run_probe<_Float16>("f16", a1, b1, k1)) return 1;
  const bool same = !memcmp(a0, a1, sizeof(a0)) && !memcmp(b0, b1, sizeof(b0)) &&
                    !memcmp(k0, k1, sizeof(k0));
  printf("bf16 map is row/col = lane&15, k = (lane>>4)*8+e: %s\n",
         is_expected(a0, b0, k0) ? "yes" : "NO");
  printf("f16 A/B lane maps equal the bf16 maps: %s\n", same ? "yes" : "NO");
  return same ? 0 : 2;
}
