// Launchers for the NHWC bf16 conv torso kernels (conv_torso.hip).
// Activations are NHWC bf16 (void* = raw bf16 bits), weights fp32 TF HWIO
// [3][3][CIN][COUT], weight/bias gradients fp32 and ACCUMULATED (zero first).
// pb_h/pb_w: TF-SAME pad_before of the 3x3/2 max-pool.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sa {
namespace conv {

int res_conv_rows(int H, int W);
// Sets a launch knob (value < 0: query only); returns the previous value or
// -1 for an unknown key.
int conv_tune_set(const char* key, int value);

// C = 3 (RGB) or 4 (stacked Atari frames) uint8 channels per pixel.
void conv1_pool_fwd_launch(const uint8_t* x, const float* w, const float* b,
                           void* pooled, uint8_t* argmax, int N, int H, int W,
                           int C, int pb_h, int pb_w, hipStream_t s);
void conv_pool_fwd_launch(const void* x, const float* w, const float* b,
                          void* pooled, uint8_t* argmax, int N, int H, int W,
                          int CIN, int COUT, int pb_h, int pb_w, hipStream_t s);
void res_conv_fwd_launch(const void* x, const float* w, const float* b,
                         const void* resid, void* y, int N, int H, int W,
                         int C, bool post_relu, bool relu_in, hipStream_t s);
// Whole residual block: t = relu(conv1(relu(x)) + b1) (written, for the
// backward), y = conv2(t) + b2 + x [then relu].
void res_block_fwd_launch(const void* x, const float* w1, const float* b1,
                          const float* w2, const float* b2, void* t, void* y,
                          int N, int H, int W, int C, bool post_relu,
                          hipStream_t s);
void res_conv_bwd_launch(const void* dy, const void* act, const void* skip,
                         const float* w, void* dx, float* dw, float* db, int N,
                         int H, int W, int C, bool relu_act, hipStream_t s,
                         float* part = nullptr);
void pool_conv_bwd_launch(const void* dP, const uint8_t* argmax, const void* x,
                          const float* w, void* dx, float* dw, float* db, int N,
                          int H, int W, int CIN, int COUT, int pb_h, int pb_w,
                          hipStream_t s, float* part = nullptr);
void conv1_pool_bwd_launch(const void* dP, const uint8_t* argmax,
                           const uint8_t* x, float* dw, float* db, int N,
                           int H, int W, int C, int pb_h, int pb_w, hipStream_t s,
                           float* part = nullptr);
// Deterministic mode (conv_tune("deterministic", 1)): the wgrad launches
// above take a slot workspace of this many floats (0 = mode off) and add the
// per-workgroup slots in a fixed order instead of with float atomics.
int64_t wgrad_part_floats(int cin, int cout, bool conv1);

// The whole shallow torso (8x8/4 -> 32, 4x4/2 -> 64, 3x3/2 -> 128, TF-SAME,
// bias + ReLU each) of uint8 NHWC frames [N,H,W,C] in one launch on bf16 MFMA
// (conv_shallow_bf16.hip): x / 255, the three convs, bf16 NHWC features
// [N,H3,W3,128].  w1p/w2p/w3p: bf16 weights in the B-operand layout
// [kstep][ntile][lane][8] (8 x 2 x 64 x 8, 16 x 4 x 64 x 8, 18 x 8 x 64 x 8
// elements, 16-byte aligned); biases fp32.  False (nothing launched) where
// shallow_bf16_form declines or a pointer is misaligned (frames 4, out 8
// bytes).  Reports family "shallow_bf16" (grid, ntiles = N) to launch_info;
// conv_tune("shallow_bf16_grid", g) caps the grid at g workgroups (0: none).
bool shallow_bf16_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                             const void* w2p, const float* b2, const void* w3p,
                             const float* b3, void* out, int N, int H, int W, int C,
                             hipStream_t s);
// 1 where shallow_bf16_fwd_launch takes N x [H, W, C] uint8 frames (72x96,
// 84x84 or 72x128 with C <= 4, 1 <= N <= 512), else 0.
int shallow_bf16_form(int N, int H, int W, int C);
// Between conv_shallow_bf16.hip and conv_torso.hip (grid cap, launch record).
int shallow_bf16_grid_max();
void shallow_bf16_note(int grid, int grid_max, int ntiles);

// One-launch stages of the bf16 deep torso's no-grad forward
// (stage_fwd_kernel), one workgroup per image with the stage's maps in LDS;
// bitwise conv_pool_fwd + two res_block_fwd.  stage_bf16_form: 1 ("stage":
// x is the stage's [N,H,W,CIN] input, CIN = 16 or 32 -> COUT = 32; head conv
// w/b, max-pool, both blocks), 2 ("tail", CIN == COUT == 16: x is a pooled
// [N,H,W,16] map; both blocks; w/b unused) or 0 where the stage does not fit
// (channels, 1 <= N <= 512, the kernel's LDS against 160 KB).  Host only.
// wb: {w1, b1, w2, b2} of block 0 then block 1.  y: [N,Hm,Wm,COUT] (the
// pooled size for form 1, H x W for form 2); last: final ReLU.  Throws where
// the form is 0.  Reports family "stage_bf16" (grid = min(N, grid_max),
// ntiles = N) to launch_info; conv_tune("stage_bf16_grid", g) caps the grid.
int stage_bf16_form(int N, int H, int W, int CIN, int COUT);
void stage_bf16_fwd_launch(const void* x, const float* w, const float* b,
                           const float* const wb[8], void* y, int N, int H, int W,
                           int CIN, int COUT, int pb_h, int pb_w, bool last,
                           hipStream_t s);

// Read-only record of the last launch of a launcher family (host side; the
// tests assert from it that the path they mean to test actually ran).
struct LaunchInfo {
  const char* family;  // "res_conv_fwd", ..., "conv1_pool_bwd"; "" = none yet
  int grid;            // workgroups launched
  int grid_max;        // persistent grid before the min with ntiles
  int ntiles;          // tiles the workgroups walked
  int rows;            // tile height (pooled rows for the pool forwards)
  bool specialized;    // a compile-time geometry was picked
};
// family == nullptr or "": the most recent launch of any family.  An unknown
// family, or one not launched yet, gives a record with family "".
LaunchInfo launch_info(const char* family);

}  // namespace conv
}  // namespace sa
