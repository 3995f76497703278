// Host launchers of the mine_amd HIP kernels: the one place each is declared.
//
// bindings.hip and every *_kernels.hip include this file, so a definition
// that disagrees with its declaration here fails to compile instead of
// linking against a stale copy (extern "C" symbols carry no types).
//
// Conventions
//  - Pointers are device pointers into dense buffers of the stated layout;
//    a launcher checks nothing about them. The bindings validate every
//    tensor before its pointer gets here.
//  - "may be null" is said where it holds; every other pointer is required.
//  - `elem` is the element-type code below. A launcher with no instance for
//    the code it is given launches nothing and returns kNoKernel; it never
//    falls into a default branch. Launchers without a code return void.
//  - A return value covers dispatch only. Whether the launch itself was
//    accepted is read by the caller from hipGetLastError().
//  - `ws` / `det`: in deterministic mode the reduction kernels store
//    per-block partials into an unfilled workspace and a finishing kernel
//    adds them in index order; otherwise they add atomically into a
//    zero-filled output.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// element-type code of the multi-dtype launchers
constexpr int kElemF32 = 0;
constexpr int kElemBF16 = 1;
constexpr int kElemF16 = 2;

// launcher return codes
constexpr int kLaunched = 0;
constexpr int kNoKernel = -1;

// For the kernel files: run CALL with T bound to the type of `elem`, or
// return kNoKernel from the enclosing launcher. MINE_ELEM_SWITCH16 has no
// f32 instance.
#define MINE_ELEM_CASE(CODE, TYPE, ...) \
  case CODE: {                          \
    using T = TYPE;                     \
    __VA_ARGS__;                        \
  } break;
#define MINE_ELEM_SWITCH16(elem, ...)                      \
  switch (elem) {                                          \
    MINE_ELEM_CASE(kElemBF16, __hip_bfloat16, __VA_ARGS__) \
    MINE_ELEM_CASE(kElemF16, _Float16, __VA_ARGS__)        \
    default: return kNoKernel;                             \
  }
#define MINE_ELEM_SWITCH(elem, ...)                        \
  switch (elem) {                                          \
    MINE_ELEM_CASE(kElemF32, float, __VA_ARGS__)           \
    MINE_ELEM_CASE(kElemBF16, __hip_bfloat16, __VA_ARGS__) \
    MINE_ELEM_CASE(kElemF16, _Float16, __VA_ARGS__)        \
    default: return kNoKernel;                             \
  }

extern "C" {

// ---------------------------------------------------------------------------
// render_kernels.hip — all f32
// ---------------------------------------------------------------------------

// mpi (B,S,H,W,4), depths (B,S), kinv (B,3,3) -> rgb_out (B,3,H,W),
// depth_out (B,1,H,W). img (B,H,W,3) may be null (no blend); mpi_blend
// (B,S,H,W,4) may be null exactly then. S <= 192.
void mine_src_composite_fwd(const float* mpi, const float* depths,
                            const float* kinv, const float* img,
                            float* rgb_out, float* depth_out, float* mpi_blend,
                            int B, int S, int H, int W, int bg_inf, int alpha,
                            hipStream_t stream);
// layouts as the forward; img, g_rgb (B,3,H,W), g_depth (B,1,H,W) and
// g_blend (B,S,H,W,4) may each be null; grad_mpi needs no fill.
void mine_src_composite_bwd(const float* mpi, const float* depths,
                            const float* kinv, const float* img,
                            const float* g_rgb, const float* g_depth,
                            const float* g_blend, float* grad_mpi, int B,
                            int S, int H, int W, int bg_inf, int alpha,
                            hipStream_t stream);
// mpi (B,S,H,W,4), hinv (B,S,3,3), m_rki (B,3,3), tvec (B,3), depths (B,S)
// -> rgb_out (B,3,H,W), depth_out and mask_out (B,1,H,W). S <= 192,
// H*W*4 < 2^31.
void mine_tgt_composite_fwd(const float* mpi, const float* hinv,
                            const float* m_rki, const float* tvec,
                            const float* depths, float* rgb_out,
                            float* depth_out, float* mask_out, int B, int S,
                            int H, int W, int bg_inf, int alpha,
                            hipStream_t stream);
// mode 0: atomic scatter into the zero-filled grad_mpi; hfwd and payload
// null. mode 1: gather; hfwd (B,S,3,3) and payload (B,S,H,W,4, unfilled)
// required, grad_mpi zero-filled. mode 2: order-fixed emit + collect; hfwd
// and payload required, neither buffer needs a fill. g_rgb (B,3,H,W) and
// g_depth (B,1,H,W) may be null.
void mine_tgt_composite_bwd(const float* mpi, const float* hinv,
                            const float* hfwd, const float* m_rki,
                            const float* tvec, const float* depths,
                            const float* g_rgb, const float* g_depth,
                            float* grad_mpi, float* payload, int B, int S,
                            int H, int W, int bg_inf, int mode, int alpha,
                            hipStream_t stream);
// V cameras read one MPI. Geometry and outputs are view-major with row
// r = v*B + b: hinv (V*B,S,3,3), m_rki (V*B,3,3), tvec (V*B,3) -> rgb_out
// (V*B,3,H,W), depth_out and mask_out (V*B,1,H,W). Row r reads mpi
// (B,S,H,W,4) and depths (B,S) at r % B. One launch of the kernel of
// mine_tgt_composite_fwd; V*B <= 65535, other limits as there.
void mine_tgt_views_fwd(const float* mpi, const float* hinv,
                        const float* m_rki, const float* tvec,
                        const float* depths, float* rgb_out, float* depth_out,
                        float* mask_out, int V, int B, int S, int H, int W,
                        int bg_inf, int alpha, hipStream_t stream);
// Backward of the above into ONE grad_mpi (B,S,H,W,4) through ONE payload
// (B,S,H,W,4): the kernels of mine_tgt_composite_bwd run view after view
// in stream order at row offset v*B. hfwd (V*B,S,3,3), g_rgb (V*B,3,H,W)
// and g_depth (V*B,1,H,W) may be null as there; fills as there (modes 0
// and 1 zero-filled once, mode 2 none: view 0 stores, later views add in
// ascending order with the accumulate form of the collect pass).
void mine_tgt_views_bwd(const float* mpi, const float* hinv, const float* hfwd,
                        const float* m_rki, const float* tvec,
                        const float* depths, const float* g_rgb,
                        const float* g_depth, float* grad_mpi, float* payload,
                        int V, int B, int S, int H, int W, int bg_inf,
                        int mode, int alpha, hipStream_t stream);
// collect pass alone: payload (B,S,H,W,4), hinv and hfwd (B,S,3,3) ->
// grad_mpi (B,S,H,W,4), no fill needed. B, S <= 65535.
void mine_tgt_collect(const float* payload, const float* hinv,
                      const float* hfwd, float* grad_mpi, int B, int S, int H,
                      int W, hipStream_t stream);

// ---------------------------------------------------------------------------
// ssim_kernels.hip — all f32
// ---------------------------------------------------------------------------

// host_win11: 11 floats in HOST memory, copied to the constant window
void mine_ssim_set_window(const float* host_win11);
// tiles per (H, W) plane: the deterministic workspace has BC * tiles floats
int mine_ssim_tiles(int H, int W);
// img1, img2 (BC,H,W) -> out_sum (1). ws null: atomics into the zero-filled
// out_sum; else ws is unfilled (BC * mine_ssim_tiles) and out_sum too.
void mine_ssim_fwd(const float* img1, const float* img2, float* out_sum,
                   float* ws, int BC, int H, int W, hipStream_t stream);
// img1, img2 (BC,H,W), gscale (1) -> grad1 (BC,H,W); F1..F3 are (BC,H,W)
// scratch planes, unfilled.
void mine_ssim_bwd(const float* img1, const float* img2, const float* gscale,
                   float* F1, float* F2, float* F3, float* grad1, int BC,
                   int H, int W, hipStream_t stream);

// ---------------------------------------------------------------------------
// pad_kernels.hip — f32, bf16 or fp16
// ---------------------------------------------------------------------------

// in (N,H,W,C) -> out (N,H+2pad,W+2pad,C); pad < H, W
int mine_reflect_pad_fwd(const void* in, void* out, int N, int H, int W, int C,
                         int pad, int elem, hipStream_t stream);
// gout (N,H+2pad,W+2pad,C) -> gin (N,H,W,C), no fill needed
int mine_reflect_pad_bwd(const void* gout, void* gin, int N, int H, int W,
                         int C, int pad, int elem, hipStream_t stream);

// ---------------------------------------------------------------------------
// bn_kernels.hip — x, res, gy, y, dx, dres of type `elem` over a flat
// (M,C); mean, invstd, gamma, beta (C) and every sum f32
// ---------------------------------------------------------------------------

// grid.x of the reduction kernels for (M, C): the deterministic workspace
// has that many (2,C) partials. kNoKernel for an unknown elem.
int mine_bn_reduce_grid(int64_t M, int C, int max_blocks, int elem);
// det 0: sums (2,C) zero-filled; det 1: sums is the unfilled
// (mine_bn_reduce_grid,2,C) workspace
int mine_bn_stats(const void* x, float* sums, int64_t M, int C, int max_blocks,
                  int det, int elem, hipStream_t s);
// y_dec (B*S,HW,C), y_base (B,HW,C), bias (B*S,C) -> x (M = B*S*HW, C) and
// its sums, as mine_bn_stats. bf16 / fp16 only; C % 8 == 0.
int mine_bn_join_stats(const void* y_dec, const void* y_base, const void* bias,
                       void* x, float* sums, int64_t M, int HW, int S, int C,
                       int max_blocks, int det, int elem, hipStream_t s);
// sums ws (G,2,C) in order: out (2,C) if not null; mean/invstd (C) if not
// null, then running_mean/running_var (C) too if not null
void mine_bn_det_finish(const float* ws, int G, int C, float* out, float* mean,
                        float* invstd, float* running_mean, float* running_var,
                        int64_t M, float eps, float momentum, hipStream_t s);
// sums (2,C) -> mean, invstd (C); running_mean/running_var (C) may be null
void mine_bn_finalize(const float* sums, float* mean, float* invstd,
                      float* running_mean, float* running_var, int64_t M,
                      int C, float eps, float momentum, hipStream_t s);
// res (M,C) is required for act 4 (add_relu) and may be null otherwise
int mine_bn_act_fwd(const void* x, const void* res, const float* mean,
                    const float* invstd, const float* gamma, const float* beta,
                    void* y, int64_t M, int C, int act, int max_blocks,
                    int elem, hipStream_t s);
// out: (2,C) zero-filled (dbeta, dgamma), or with det the unfilled
// (mine_bn_reduce_grid,2,C) workspace. res as above.
int mine_bn_act_bwd_reduce(const void* x, const void* res, const void* gy,
                           const float* mean, const float* invstd,
                           const float* gamma, const float* beta, float* out,
                           int64_t M, int C, int act, int max_blocks, int det,
                           int elem, hipStream_t s);
// red (2,C); dres (M,C) is required for act 4 and may be null otherwise
int mine_bn_act_bwd_dx(const void* x, const void* res, const void* gy,
                       const float* mean, const float* invstd,
                       const float* gamma, const float* beta, const float* red,
                       void* dx, void* dres, int64_t M, int C, int act,
                       int max_blocks, int elem, hipStream_t s);

// Small-layer path: two launches per direction, order-fixed, no fill. The
// reductions store G partials into ws (G,2,C), unfilled; the consumers add
// them in ascending g. G and grid_x in [1, 4096], cgv a power of two in
// [1, 64]; otherwise kNoKernel.
//
// The plan for (M, C) of `elem`: *G partial rows, the reduction's channel
// chunk *cgv (vectors), the consumer's *grid_x. Returns 1 where the layer
// should take the path, 0 where today's kernels win (the plan is valid
// either way), kNoKernel for an unknown elem.
int mine_bn_small_plan(int64_t M, int C, int elem, int* G, int* cgv,
                       int* grid_x);
// x (M,C) -> ws (G,2,C) partial (sum, sumsq)
int mine_bn_stats_partials(const void* x, float* ws, int64_t M, int C, int G,
                           int cgv, int elem, hipStream_t s);
// ws (G,2,C) partial (sum, sumsq) -> y (M,C), mean, invstd (C); updates
// running_mean/running_var (C) once and adds 1 to num_batches_tracked (1),
// each where not null. res as in mine_bn_act_fwd.
int mine_bn_act_fwd_ws(const void* x, const void* res, const float* ws, int G,
                       const float* gamma, const float* beta, void* y,
                       float* mean, float* invstd, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked,
                       int64_t M, int C, int act, int grid_x, float eps,
                       float momentum, int elem, hipStream_t s);
// as mine_bn_act_bwd_reduce with det: ws (G,2,C) partial (dbeta, dgamma)
int mine_bn_act_bwd_reduce_partials(const void* x, const void* res,
                                    const void* gy, const float* mean,
                                    const float* invstd, const float* gamma,
                                    const float* beta, float* ws, int64_t M,
                                    int C, int act, int G, int cgv, int elem,
                                    hipStream_t s);
// ws (G,2,C) partial (dbeta, dgamma) -> dx, dres as mine_bn_act_bwd_dx, and
// red (2,C), the finished sums
int mine_bn_act_bwd_dx_ws(const void* x, const void* res, const void* gy,
                          const float* mean, const float* invstd,
                          const float* gamma, const float* beta,
                          const float* ws, int G, float* red, void* dx,
                          void* dres, int64_t M, int C, int act, int grid_x,
                          int elem, hipStream_t s);

// ---------------------------------------------------------------------------
// head_kernels.hip — z f32, bf16 or fp16; the packed MPI is f32
// ---------------------------------------------------------------------------

// z (N,4) -> out (N,4) f32
int mine_mpi_head_fwd(const void* z, float* out, int64_t N, int alpha,
                      int elem, hipStream_t s);
// z (N,4), gout (N,4) f32 -> gz (N,4) of z's type
int mine_mpi_head_bwd(const void* z, const float* gout, void* gz, int64_t N,
                      int alpha, int elem, hipStream_t s);

// ---------------------------------------------------------------------------
// conv_kernels.hip — bf16 or fp16
// ---------------------------------------------------------------------------

// x (N,src_h,src_w,c_mem), wp packed by mine_conv3x3_pack, out (N,H,W,K),
// all of type `elem`; bias (K) f32 may be null. C % 8 == 0, C <= 64; c_mem
// is C, or 4 with C == 8 in zero-embed mode. Also kNoKernel when no kernel
// is instantiated for the shape.
int mine_conv3x3_fwd(const void* x, const void* wp, const float* bias,
                     void* out, int N, int H, int W, int C, int c_mem, int K,
                     int pad_mode, int src_h, int src_w, int off, int elem,
                     hipStream_t stream);
// out[i] = w[lut[i]], or 0 where lut[i] is outside [0, n_w). w (n_w) is
// any w_elem; out (n_out) is out_elem, bf16 or fp16.
int mine_conv3x3_pack(const void* w, int w_elem, const int64_t* lut, void* out,
                      int out_elem, int64_t n_out, int64_t n_w,
                      hipStream_t stream);

// ---------------------------------------------------------------------------
// wrw_kernels.hip — bf16 or fp16
// ---------------------------------------------------------------------------

// slab count, k blocks and workspace floats of one mine_conv3x3_wrw call
// over rows = N*H; max_slabs 0 = automatic
void mine_conv3x3_wrw_plan(int C, int Kmem, int64_t rows, int max_slabs,
                           int* slabs, int* nkb, int64_t* ws_floats);
// x (N,H,W,C), gy (N,H,W,Kmem) 16-byte aligned -> dw (K,C,3,3) f32 and, if
// not null, db (K) f32. ws: the plan's ws_floats, unfilled (always
// order-fixed). C in {16,32,48,64}; Kmem is 4 or a multiple of 8, >= K.
int mine_conv3x3_wrw(const void* x, const void* gy, float* ws, float* dw,
                     float* db, int N, int H, int W, int C, int Kmem, int K,
                     int slabs, int elem, hipStream_t stream);

// ---------------------------------------------------------------------------
// resample_kernels.hip — f32 (C % 4 == 0), bf16 or fp16 (C % 8 == 0)
// ---------------------------------------------------------------------------

// in (N,H,W,C) -> out (N,2H,2W,C)
int mine_upsample2x_fwd(const void* in, void* out, int64_t N, int64_t H,
                        int64_t W, int64_t C, int elem, hipStream_t stream);
// gout (N,2H,2W,C) -> gin (N,H,W,C), no fill needed
int mine_upsample2x_bwd(const void* gout, void* gin, int64_t N, int64_t H,
                        int64_t W, int64_t C, int elem, hipStream_t stream);

// ---------------------------------------------------------------------------
// igemm_kernels.hip — bf16 or fp16
// ---------------------------------------------------------------------------

// out[i] = w[lut[i]], or 0 where lut[i] < 0. w is any w_elem and must
// cover every index in lut (n); out (n) is out_elem, bf16 or fp16.
int mine_pack_gather(const void* w, const int* lut, void* out, int64_t n,
                     int w_elem, int out_elem, hipStream_t stream);
// x: the (Hs,Ws,C) images that (SA,SB,SD,SE) map the M = N*P*Q output pixels
// onto; wp: packed fragments for (K,C,R,S); out (M,K); bias (K) f32 may be
// null. (R,S) is 1x1, 3x3 or 7x7; C % 8 == 0. splitz > 1 requires ws:
// zero-filled f32 (M,K), or with det an unfilled (splitz,M,K); else null.
int mine_conv_igemm_fwd(const void* x, const void* wp, const float* bias,
                        void* out, float* ws, int64_t M, int P, int Q, int K,
                        int Hs, int Ws, int C, int R, int S, int SA, int SB,
                        int SD, int SE, int pad_mode, int splitz, int det,
                        int elem, hipStream_t stream);
// pixel slabs (grid.x) of the weight gradient: the deterministic workspace
// holds that many (K,C,R,S) partials
int mine_conv_igemm_wrw_slabs(int64_t M, int K, int C, int R, int S);
// x as above, gy (M,K) -> dw (K,C,R,S) f32. ws_det null: atomics into the
// zero-filled dw; else ws_det is unfilled (slabs,K,C,R,S) and dw too.
int mine_conv_igemm_wrw(const void* x, const void* gy, float* dw,
                        float* ws_det, int64_t M, int P, int Q, int K, int Hs,
                        int Ws, int C, int R, int S, int SA, int SB, int SD,
                        int SE, int pad_mode, int elem, hipStream_t stream);

// ---------------------------------------------------------------------------
// loss_kernels.hip — all f32
// ---------------------------------------------------------------------------

// grid.x of the eav2 launches: the row length of their workspaces
int mine_eav2_grid(int HW);
// disp (B,1,H,W); img (B,3,H,W) through element strides (isb,isc,isy,isx);
// mean_d (B) -> out (2). ws null: atomics into the zero-filled out; else ws
// is unfilled (2,B,mine_eav2_grid) and out too.
void mine_eav2_fwd(const float* disp, const float* img, const float* mean_d,
                   float* out, float* ws, int B, int H, int W, int64_t isb,
                   int64_t isc, int64_t isy, int64_t isx, hipStream_t stream);
// as the forward, gl (1) -> grad (B,1,H,W); g_d (B,1,H,W) scratch. ws null:
// atomics into the zero-filled Tb (B); else ws is unfilled
// (B,mine_eav2_grid) and Tb too.
void mine_eav2_bwd(const float* disp, const float* img, const float* mean_d,
                   float* g_d, float* Tb, float* ws, const float* gl,
                   float* grad, int B, int H, int W, int64_t isb, int64_t isc,
                   int64_t isy, int64_t isx, hipStream_t stream);
// g (B,C,N), idx (B,N) in [0,HW) -> grad_img (B,C,HW), zero-filled.
// B*C*N < 2^31.
void mine_gather_pxpy_bwd(const float* g, const int64_t* idx, float* grad_img,
                          int B, int C, int N, int64_t HW, hipStream_t stream);

}  // extern "C"
