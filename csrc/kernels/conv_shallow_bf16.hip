// The shallow conv torso for bf16 actor inference in ONE launch (gfx950).
//
// uint8 NHWC frames [N,H,W,C] -> x / 255 -> conv 8x8/4 (32) -> conv 4x4/2
// (64) -> conv 3x3/2 (128), TF-SAME, bias + ReLU each -> bf16 NHWC features
// [N,H3,W3,128].  One 512-thread workgroup per image (a grid-stride walk over
// the images when the grid is capped); every intermediate stays in LDS.
//
// LDS (bf16, NHWC, the TF-SAME pad ring stored as zeros, so no tap is ever
// out of bounds or masked):
//   fr [Hp0][Wp0][4]    the frame, bytes as exact bf16 integers 0..255,
//                       channels zero-padded to 4
//   a1 [Hp1][Wp1][40]   layer-1 output (32 channels, pixel pitch 40); the
//                       raw uint8 frame is staged through it first
//   a2 [Hp2][Wp2][72]   layer-2 output (64 channels, pixel pitch 72)
// Hp/Wp = (out - 1) * stride + kernel of the layer that READS the map.  The
// pixel pitches 40 / 72 keep the 16 pixels of an operand read (2 pixels
// apart) on different banks.  72x128x3, the largest frame: 80256 + 54400 +
// 26928 = 161584 of the 163840 bytes.
//
// Every layer is an implicit GEMM on v_mfma_f32_16x16x32_bf16, computed
// transposed (conv_common.h): A = 16 output channels of the packed weights,
// B = 16 output pixels, so a lane ends with 4 consecutive channels of one
// pixel (one 8-byte NHWC store).  A K = 32 step is 32 contiguous bf16 of the
// staged map - layer 1: one ky (8 pixels x 4 channels), 8 steps; layer 2: one
// (ky, kx), 16 steps; layer 3: one (ky, kx, half), 18 steps - so a lane's
// pixel operand is one 16-byte LDS read.  Lanes of a partial last pixel tile
// read pixel 0 and store nothing.  The weight operand comes from global
// memory (L2) in the packed layout of shallow_bf16_pack,
//   wp[kstep][ntile][lane][8] = bf16(Wflat[32 kstep + 8 (lane >> 4) + j]
//                                         [16 ntile + (lane & 15)]),
// Wflat = HWIO flattened to [kh * kw * cin, cout] (layer 1: cin zero-padded
// to 4).  The 8 waves split (channel tile) x (pixel-tile class); a wave holds
// its channel tile's fragments of a whole layer in registers, loaded one
// layer ahead.
//
// Rounding points: weights RNE to bf16 once (pack); frame bytes exact bf16
// integers; fp32 accumulation; layer 1: acc / 255 as a correctly rounded fp32
// division, + bias in fp32; layers 2 and 3: acc + bias in fp32; then ReLU and
// ONE RNE rounding to bf16 per stored value.  1 / 255 is applied to the
// accumulator, never folded into the weights, and as a DIVISION: 255 k / 255
// = k exactly, so a frame of bytes 0 / 255 gives exact sums of bf16(w1).  A
// multiply by fl(1 / 255) would not do: that constant rounds upward by more
// than half an ulp of some k (255 * fl(1 / 255) = 1 + 2^-24, and 255 k
// fl(1 / 255) rounds to k + ulp for k = 129..255 among others;
// tests/test_shallow_bf16_flag.py shows both facts on the host).
//
// No cross-workgroup synchronisation, no atomics, no spin waits; every loop
// is bounded by N and the geometry.  Reports family "shallow_bf16" to
// sa::conv::launch_info (grid, ntiles = N); conv_tune("shallow_bf16_grid", g)
// caps the grid at g workgroups (0 = no cap).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "conv_common.h"
#include "conv_launchers.h"
#include "conv_shallow_bf16.h"  // the tile body, the layer split, the geometry

namespace sa {
namespace conv {

namespace {

__global__ __launch_bounds__(kSbThreads) void shallow_bf16_kernel(ShallowBf16Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* fr = reinterpret_cast<bf16_t*>(sb_smem);
  bf16_t* a1 = fr + a.Hp0 * a.Wp0 * 4;
  bf16_t* a2 = a1 + a.Hp1 * a.Wp1 * kSbPitch1;
  const int n1 = a.Hp1 * a.Wp1 * kSbPitch1;  // bf16 elements, multiples of 8
  const int n2 = a.Hp2 * a.Wp2 * kSbPitch2;
  const int lane = lane_id(), wave = wave_id();
  const uint4 z4 = make_uint4(0, 0, 0, 0);

  // a2's pad ring is written here once: the epilogues only store interiors
  for (int e = threadIdx.x; e < n2 / 8; e += kSbThreads) reinterpret_cast<uint4*>(a2)[e] = z4;

  const int ndw = (a.H * a.W * a.C) >> 2;  // whole dwords (shallow_bf16_form)
  const int P3 = a.H3 * a.W3;
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    // opaque per image: hoisted out of the image loop, the three layers'
    // fragments (168 registers) would be live at once and the kernel spills
    int z = 0;
    asm volatile("" : "+s"(z));
    const uint4 *w1 = a.w1 + z, *w2 = a.w2 + z, *w3 = a.w3 + z;
    uint4 wf1[8], wf2[16], wf3[18];
    load_frags<8, 2>(w1, wave % 2, lane, wf1);
    // raw bytes -> a1 (free: the previous image's layer 2 ended with a barrier)
    const uint32_t* src =
        reinterpret_cast<const uint32_t*>(a.frames + static_cast<int64_t>(n) * ndw * 4);
    uint32_t* raw = reinterpret_cast<uint32_t*>(a1);
    for (int d = threadIdx.x; d < ndw; d += kSbThreads) raw[d] = src[d];
    __syncthreads();
    // bytes -> bf16 integers, 4 channels per pixel, zero ring and pad channels
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(a1);
    const int np0 = a.Hp0 * a.Wp0;
    for (int e = threadIdx.x; e < np0; e += kSbThreads) {
      const int r = e / a.Wp0, c = e - r * a.Wp0;
      const int iy = r - a.pt1, ix = c - a.pl1;
      uint2 v = make_uint2(0, 0);
      if (static_cast<unsigned>(iy) < static_cast<unsigned>(a.H) &&
          static_cast<unsigned>(ix) < static_cast<unsigned>(a.W)) {
        const uint8_t* px = rb + (iy * a.W + ix) * a.C;
        uint32_t h[4] = {0, 0, 0, 0};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < a.C) h[ch] = __float_as_uint(static_cast<float>(px[ch])) >> 16;  // exact
        v = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
      }
      reinterpret_cast<uint2*>(fr)[e] = v;
    }
    __syncthreads();  // the raw bytes are dead
    for (int e = threadIdx.x; e < n1 / 8; e += kSbThreads) reinterpret_cast<uint4*>(a1)[e] = z4;
    load_frags<16, 4>(w2, wave % 4, lane, wf2);  // in flight during layer 1
    __syncthreads();

    {
      const int Wp0 = a.Wp0, Wp1 = a.Wp1, pt = a.pt2, pl = a.pl2;
      sb_layer<8, 2, kSbMt1, 4, 4, true>(
          wf1, fr, Wp0, a.H1, a.W1, a.b1,
          [=](int ks) { return ks * Wp0 * 4; },
          [=](int, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a1 + ((oy + pt) * Wp1 + ox + pl) * kSbPitch1 + co) = v;
          });
    }
    load_frags<18, 8>(w3, wave, lane, wf3);  // in flight during layer 2
    __syncthreads();
    {
      const int Wp1 = a.Wp1, Wp2 = a.Wp2, pt = a.pt3, pl = a.pl3;
      sb_layer<16, 4, kSbMt2, 2, kSbPitch1, false>(
          wf2, a1, Wp1, a.H2, a.W2, a.b2,
          [=](int ks) { return ((ks >> 2) * Wp1 + (ks & 3)) * kSbPitch1; },
          [=](int, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a2 + ((oy + pt) * Wp2 + ox + pl) * kSbPitch2 + co) = v;
          });
    }
    __syncthreads();
    {
      const int Wp2 = a.Wp2;
      bf16_t* o = a.out + static_cast<int64_t>(n) * P3 * 128;
      sb_layer<18, 8, kSbMt3, 2, kSbPitch2, false>(
          wf3, a2, Wp2, a.H3, a.W3, a.b3,
          [=](int ks) {
            const int tap = ks >> 1;
            return ((tap / 3) * Wp2 + tap % 3) * kSbPitch2 + (ks & 1) * 32;
          },
          [=](int p, int, int, int co, uint2 v) {
            *reinterpret_cast<uint2*>(o + p * 128 + co) = v;
          });
    }
    // the next image's first write to a2 (layer 2) is behind four barriers
  }
}

// ---- frames of 5 to 16 channels: shallow_bf16w_kernel ----
//
// The frame at Cp = 8 / 12 / 16 bf16 per pixel (C rounded up to a multiple of
// 4, pad channels zero) does not fit LDS beside a1 and a2, so layer 1 runs in
// BANDS of R output rows.  LDS: band [4 R + 4][Wp0][Cp] (padded input rows
// 4 oy0 .. of the band that starts at output row oy0), then a1 and a2 as
// above.  One ky row of a pixel's 8x8 window is 8 Cp contiguous bf16 = Cp / 4
// K steps of 32, so layer 1 has 16 / 24 / 32 steps, every operand read is one
// aligned 16-byte LDS read and its packed weights are the layout above over
// Wflat = [64 Cp, 32].  A wave keeps its channel tile's layer-1 fragments
// (64 / 96 / 128 registers) for all bands of an image.
//
// A thread stages at most kSbwPx band pixels: it loads the dwords that cover
// the pixel's C bytes (image rows are dword multiples, a pixel may start at
// any byte), aligns them with v_alignbyte_b32, clears the bytes past C and
// expands each byte to a bf16 integer on the way into LDS - no raw-byte
// buffer.  The loads of band b + 1 are issued before the MFMAs of band b and
// stay in registers until the barrier behind those MFMAs; the last band's
// registers hold the layer-2 fragments instead.  a1's and a2's pad rings are
// zeroed once per workgroup: the epilogues only ever store interiors.
// Rounding points, grid walk and grid cap are those above; it reports family
// "shallow_bf16w" (grid, ntiles = N, rows = the band count) to launch_info.
// (kSbwMt1, kSbwPx, the staging pair sbw_fetch / sbw_put and sbw_plan live in
// conv_shallow_bf16.h: the learner's wide kernels share them.)
template <int CPQ>
__global__ __launch_bounds__(kSbThreads) void shallow_bf16w_kernel(ShallowBf16wArgs wa) {
  constexpr int CP = 4 * CPQ, KS1 = 8 * CPQ;
  const ShallowBf16Args& a = wa.g;
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* band = reinterpret_cast<bf16_t*>(sb_smem);
  bf16_t* a1 = band + (4 * wa.R + 4) * a.Wp0 * CP;
  bf16_t* a2 = a1 + a.Hp1 * a.Wp1 * kSbPitch1;
  const int n12 = a.Hp1 * a.Wp1 * kSbPitch1 + a.Hp2 * a.Wp2 * kSbPitch2;  // multiple of 8
  const uint4 z4 = make_uint4(0, 0, 0, 0);

  // both maps' pad rings, once: the first band's barrier orders it
  for (int e = threadIdx.x; e < n12 / 8; e += kSbThreads) reinterpret_cast<uint4*>(a1)[e] = z4;

  const int ndw = (a.H * a.W * a.C) >> 2;  // whole dwords (shallow_bf16w_form)
  const int P3 = a.H3 * a.W3;
  const int Wp0 = a.Wp0, Wp1 = a.Wp1, Wp2 = a.Wp2, R = wa.R;
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    int z = 0;  // opaque per image, as in shallow_bf16_kernel
    asm volatile("" : "+s"(z));
    const uint4 *w1 = a.w1 + z, *w2 = a.w2 + z, *w3 = a.w3 + z;
    uint4 wf1[KS1], wf2[16], wf3[18];
    // and the thread's number: the staged pixels' and the fragments'
    // addresses and predicates would otherwise be kept across the image loop
    // (they spilled)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t* img = reinterpret_cast<const uint32_t*>(a.frames) + static_cast<int64_t>(n) * ndw;
    // one band of layer 1; rows oy0 .. of a1 (the band buffer's row 0 is the
    // padded frame's row 4 oy0)
    auto layer1 = [&](int oy0) {
      const int pt = a.pt2, pl = a.pl2;
      sb_layer<KS1, 2, kSbwMt1, 4, CP, true>(
          wf1, band, Wp0, min(R, a.H1 - oy0), a.W1, a.b1,
          [=](int ks) { return (ks / CPQ) * Wp0 * CP + (ks % CPQ) * 32; },
          [=](int, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a1 + ((oy0 + oy + pt) * Wp1 + ox + pl) * kSbPitch1 + co) = v;
          });
    };
    auto band_rows = [&](int oy0) { return 4 * min(R, a.H1 - oy0) + 4; };
    {
      // the band buffer is free: the previous image's last band ended with a
      // barrier
      uint32_t q[kSbwPx][CPQ];
      sbw_fetch<CPQ>(a, img, tid, 0, band_rows(0), q);
      load_frags<KS1, 2>(w1, wave % 2, lane, wf1);
      sbw_put<CPQ>(q, tid, band_rows(0) * Wp0, band);
    }
    __syncthreads();
    int oy0 = 0;
    for (; oy0 + R < a.H1; oy0 += R) {
      uint32_t q[kSbwPx][CPQ];
      sbw_fetch<CPQ>(a, img, tid, 4 * (oy0 + R), band_rows(oy0 + R), q);  // in flight during the MFMAs
      layer1(oy0);
      __syncthreads();  // the band's reads are done
      sbw_put<CPQ>(q, tid, band_rows(oy0 + R) * Wp0, band);
      __syncthreads();
    }
    // in flight during the last band where the registers allow it: beside
    // the 128 of Cp = 16 they do not (the kernel spilled)
    if constexpr (CPQ < 4) load_frags<16, 4>(w2, wave % 4, lane, wf2);
    layer1(oy0);
    if constexpr (CPQ == 4) load_frags<16, 4>(w2, wave % 4, lane, wf2);
    load_frags<18, 8>(w3, wave, lane, wf3);  // in flight during layer 2
    __syncthreads();
    {
      const int pt = a.pt3, pl = a.pl3;
      sb_layer<16, 4, kSbMt2, 2, kSbPitch1, false>(
          wf2, a1, Wp1, a.H2, a.W2, a.b2,
          [=](int ks) { return ((ks >> 2) * Wp1 + (ks & 3)) * kSbPitch1; },
          [=](int, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a2 + ((oy + pt) * Wp2 + ox + pl) * kSbPitch2 + co) = v;
          });
    }
    __syncthreads();
    {
      bf16_t* o = a.out + static_cast<int64_t>(n) * P3 * 128;
      sb_layer<18, 8, kSbMt3, 2, kSbPitch2, false>(
          wf3, a2, Wp2, a.H3, a.W3, a.b3,
          [=](int ks) {
            const int tap = ks >> 1;
            return ((tap / 3) * Wp2 + tap % 3) * kSbPitch2 + (ks & 1) * 32;
          },
          [=](int p, int, int, int co, uint2 v) {
            *reinterpret_cast<uint2*>(o + p * 128 + co) = v;
          });
    }
    // the next image's first write to a1 (band 0's epilogue) is behind one
    // barrier and layer 2's reads ended at the barrier before layer 3; its
    // first write to a2 (layer 2) is behind at least two
  }
}

}  // namespace

int shallow_bf16_form(int N, int H, int W, int C) {
  if (N < 1 || N > 512 || C < 1 || C > 4) return 0;
  if (!((H == 72 && W == 96) || (H == 84 && W == 84) || (H == 72 && W == 128))) return 0;
  ShallowBf16Args a{};
  return sb_plan(H, W, C, &a) > 0 ? 1 : 0;
}

bool shallow_bf16_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                             const void* w2p, const float* b2, const void* w3p,
                             const float* b3, void* out, int N, int H, int W, int C,
                             hipStream_t s) {
  if (!shallow_bf16_form(N, H, W, C)) return false;
  auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
  if (mis(frames, 3) || mis(w1p, 15) || mis(w2p, 15) || mis(w3p, 15) || mis(out, 7))
    return false;
  ShallowBf16Args a{};
  const size_t lds = sb_plan(H, W, C, &a);
  a.frames = frames;
  a.w1 = static_cast<const uint4*>(w1p);
  a.w2 = static_cast<const uint4*>(w2p);
  a.w3 = static_cast<const uint4*>(w3p);
  a.b1 = b1; a.b2 = b2; a.b3 = b3;
  a.out = static_cast<bf16_t*>(out);
  a.N = N;
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(shallow_bf16_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(lds)) != hipSuccess)
    (void)hipGetLastError();  // the launch itself reports an LDS request it cannot meet
  shallow_bf16_note(G, grid_max, N);
  hipLaunchKernelGGL(shallow_bf16_kernel, dim3(G), dim3(kSbThreads), lds, s, a);
  return true;
}

int shallow_bf16w_form(int N, int H, int W, int C) {
  if (N < 1 || N > 512 || C < 5 || C > 16) return 0;
  if (!((H == 72 && W == 96) || (H == 84 && W == 84) || (H == 72 && W == 128))) return 0;
  ShallowBf16wArgs wa{};
  return sbw_plan(H, W, C, &wa) > 0 ? 1 : 0;
}

bool shallow_bf16w_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                              const void* w2p, const float* b2, const void* w3p,
                              const float* b3, void* out, int N, int H, int W, int C,
                              hipStream_t s) {
  if (!shallow_bf16w_form(N, H, W, C)) return false;
  auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
  if (mis(frames, 3) || mis(w1p, 15) || mis(w2p, 15) || mis(w3p, 15) || mis(out, 7))
    return false;
  ShallowBf16wArgs wa{};
  const size_t lds = sbw_plan(H, W, C, &wa);
  ShallowBf16Args& a = wa.g;
  a.frames = frames;
  a.w1 = static_cast<const uint4*>(w1p);
  a.w2 = static_cast<const uint4*>(w2p);
  a.w3 = static_cast<const uint4*>(w3p);
  a.b1 = b1; a.b2 = b2; a.b3 = b3;
  a.out = static_cast<bf16_t*>(out);
  a.N = N;
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  auto go = [&](auto kernel) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(lds)) != hipSuccess)
      (void)hipGetLastError();  // the launch itself reports an LDS request it cannot meet
    hipLaunchKernelGGL(kernel, dim3(G), dim3(kSbThreads), lds, s, wa);
  };
  shallow_bf16w_note(G, grid_max, N, wa.bands);
  if (C <= 8) go(shallow_bf16w_kernel<2>);
  else if (C <= 12) go(shallow_bf16w_kernel<3>);
  else go(shallow_bf16w_kernel<4>);
  return true;
}

}  // namespace conv
}  // namespace sa
