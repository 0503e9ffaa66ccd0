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
// Stage 0 on frames of 5 to 16 uint8 channels (conv_wide_bf16.hip): the
// outputs, argmax codes and gradients of the two launches above, in the same
// layouts; the frame's channels are zero-padded to Cp = 8 (C <= 8) or 16 in
// LDS.  Families "conv1w_pool_fwd" / "conv1w_pool_bwd" in launch_info; tile
// heights follow px_conv1_fwd / px_conv1_bwd under the kernels' own LDS rules.
void conv1w_pool_fwd_launch(const uint8_t* x, const float* w, const float* b,
                            void* pooled, uint8_t* argmax, int N, int H, int W,
                            int C, int pb_h, int pb_w, hipStream_t s);
void conv1w_pool_bwd_launch(const void* dP, const uint8_t* argmax,
                            const uint8_t* x, float* dw, float* db, int N,
                            int H, int W, int C, int pb_h, int pb_w, hipStream_t s,
                            float* part = nullptr);
// Between conv_wide_bf16.hip and conv_torso.hip (grid, launch record, the
// deterministic mode's slot reduce).
int conv1w_grid(int ntiles, size_t smem, bool bwd, int* grid_max);
void conv1w_note(bool bwd, int grid, int grid_max, int ntiles, int rows,
                 bool specialized);
void wgrad_reduce_slots(const float* part, int slots, int nel, int ndw, float* dw,
                        float* db, hipStream_t s);
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
// The same torso on frames of 5 <= C <= 16 channels (shallow_bf16w_kernel):
// the frame is padded to Cp = C rounded up to a multiple of 4 (8, 12 or 16)
// bf16 per pixel and layer 1 runs in bands of output rows.  w1p: the layout
// above over Wflat = [64 Cp, 32] (8 Cp / 4 K steps: 2 Cp x 2 x 64 x 8
// elements); w2p / w3p, the alignment rules and the features as above.
// Reports family "shallow_bf16w" (grid, ntiles = N, rows = the band count);
// the same conv_tune key caps its grid.  shallow_bf16w_form: 1 for 72x96,
// 84x84 or 72x128 frames with 5 <= C <= 16 and 1 <= N <= 512, else 0.
bool shallow_bf16w_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                              const void* w2p, const float* b2, const void* w3p,
                              const float* b3, void* out, int N, int H, int W, int C,
                              hipStream_t s);
int shallow_bf16w_form(int N, int H, int W, int C);
// Between conv_shallow_bf16.hip and conv_torso.hip (grid cap, launch record).
int shallow_bf16_grid_max();
void shallow_bf16_note(int grid, int grid_max, int ntiles);
void shallow_bf16w_note(int grid, int grid_max, int ntiles, int bands);

// The training form of that torso on 1-4 channel frames
// (conv_shallow_bf16_train.hip): only the three convs run in bf16, features
// and parameter gradients are fp32.  Maps are dense NHWC: a1 [N,H1,W1,32],
// a2 [N,H2,W2,64] (post-ReLU bf16), feats [N,H3,W3,128] (post-ReLU fp32,
// bitwise shallow_bf16_fwd's output once rounded to bf16).  Every launcher
// returns false (nothing launched) where shallow_bf16_train_form declines or a
// pointer is not 16-byte aligned (frames: 4), walks the images with one
// 512-thread workgroup each under the shallow_bf16_grid cap, and reports
// family "shallow_bf16_train_fwd" / "_bwd_data" / "_wgrad" (grid, ntiles = N).
// 1 for 72x96, 84x84 or 72x128 frames with 1 <= C <= 4 and 1 <= N <= 8192.
int shallow_bf16_train_form(int N, int H, int W, int C);
// fp32 HWIO weights -> the forward's packed operands (shallow_bf16_pack's
// layout and bits) and the two data gradients' operands
//   wd[tap][kq][ct][lane][8] = bf16(W[tap][16 ct + (lane & 15)][32 kq + 8 (lane >> 4) + j])
// (wd2: 16 x 2 x 2, wd3: 9 x 4 x 4 fragments of 64 x 8), in one launch.
void shallow_bf16_train_pack_launch(const float* w1, const float* w2, const float* w3,
                                    void* w1p, void* w2p, void* w3p, void* wd2, void* wd3,
                                    int C, hipStream_t s);
bool shallow_bf16_train_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                                   const void* w2p, const float* b2, const void* w3p,
                                   const float* b3, float* feats, void* a1, void* a2, int N,
                                   int H, int W, int C, hipStream_t s);
// dY3m = bf16(dfeats where feats > 0), dA2 = bf16(dgrad3(dY3m) where a2 > 0),
// dA1 = bf16(dgrad2(dA2) where a1 > 0); fp32 accumulation, one rounding each.
bool shallow_bf16_bwd_data_launch(const float* dfeats, const float* feats, const void* a2,
                                  const void* a1, const void* wd3, const void* wd2, void* dy3m,
                                  void* da2, void* da1, int N, int H, int W, int C,
                                  hipStream_t s);
// dw_l += sum over images and pixels of patches(in_l)^T dOut_l (layer 1: the
// byte sums / 255), db_l += column sums of dOut_l.  One launch per layer
// writes each workgroup's fp32 partial sums to its own slot of `part`
// (shallow_bf16_wgrad_part_floats(N) floats), then one launch adds the slots
// in a fixed order: no float atomics, bitwise reproducible.
int64_t shallow_bf16_wgrad_part_floats(int N);
bool shallow_bf16_wgrad_launch(const uint8_t* frames, const void* a1, const void* a2,
                               const void* dy3m, const void* da2, const void* da1, float* part,
                               float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                               float* db3, int N, int H, int W, int C, hipStream_t s);
// The same on frames of 5 <= C <= 16 channels.  shallow_bf16w_train_form: 1
// for the three frame sizes with 5 <= C <= 16 and 1 <= N <= 8192.  The pack
// launcher above takes such a w1 (w1p: shallow_bf16w_pack's layout and bits,
// 2 Cp K steps).  The forward is shallow_bf16w_kernel's banded image loop with
// the saved maps (family "shallow_bf16w_train_fwd"; feats.to(bf16) is bitwise
// shallow_bf16w_fwd's output).  The data gradient is
// shallow_bf16_bwd_data_launch: it reads no frame bytes and takes whatever
// shallow_bf16_train_back_form accepts (the three sizes, 1 <= C <= 16).  The
// weight-gradient launcher runs layers 2 and 3 as above (family
// "shallow_bf16_wgrad"), layer 1 band by band (family "shallow_bf16w_wgrad1")
// and the same fixed-order reduce; part:
// shallow_bf16w_wgrad_part_floats(N, C) floats.
int shallow_bf16w_train_form(int N, int H, int W, int C);
int shallow_bf16_train_back_form(int N, int H, int W, int C);
bool shallow_bf16w_train_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                                    const void* w2p, const float* b2, const void* w3p,
                                    const float* b3, float* feats, void* a1, void* a2, int N,
                                    int H, int W, int C, hipStream_t s);
int64_t shallow_bf16w_wgrad_part_floats(int N, int C);
bool shallow_bf16w_wgrad_launch(const uint8_t* frames, const void* a1, const void* a2,
                                const void* dy3m, const void* da2, const void* da1, float* part,
                                float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                float* db3, int N, int H, int W, int C, hipStream_t s);
// which: 0 fwd, 1 bwd_data, 2 wgrad, 3 the wide fwd, 4 the wide layer-1 wgrad
// (conv_torso.hip keeps the launch records)
void shallow_bf16_train_note(int which, int grid, int grid_max, int ntiles);

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
  const char* family;  // "res_conv_fwd", ..., "shallow_bf16w"; "" = none yet
  int grid;            // workgroups launched
  int grid_max;        // persistent grid before the min with ntiles
  int ntiles;          // tiles the workgroups walked
  int rows;            // tile height (pooled rows for the pool forwards; the band
                       // count for "shallow_bf16w")
  bool specialized;    // a compile-time geometry was picked
};
// family == nullptr or "": the most recent launch of any family.  An unknown
// family, or one not launched yet, gives a record with family "".
LaunchInfo launch_info(const char* family);

}  // namespace conv
}  // namespace sa
