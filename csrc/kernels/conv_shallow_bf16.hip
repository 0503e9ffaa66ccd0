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

namespace sa {
namespace conv {

namespace {

constexpr int kSbThreads = 512;
constexpr int kSbWaves = kSbThreads / 64;
constexpr int kSbPitch1 = 40, kSbPitch2 = 72;  // bf16 per pixel of a1 / a2
constexpr int kSbMt1 = 9, kSbMt2 = 5, kSbMt3 = 3;  // pixel tiles per wave
constexpr size_t kSbLdsMax = 160 * 1024;

struct ShallowBf16Args {
  const uint8_t* frames;          // [N, H, W, C]
  const uint4 *w1, *w2, *w3;      // packed bf16 fragments
  const float *b1, *b2, *b3;
  bf16_t* out;                    // [N, H3, W3, 128]
  int N, H, W, C;
  int H1, W1, pt1, pl1, Hp0, Wp0;  // layer outputs, pad_before, padded input
  int H2, W2, pt2, pl2, Hp1, Wp1;
  int H3, W3, pt3, pl3, Hp2, Wp2;
};

template <int KS, int NT>
__device__ __forceinline__ void load_frags(const uint4* __restrict__ wp, int nt, int lane,
                                           uint4 (&wf)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) wf[ks] = wp[(ks * NT + nt) * 64 + lane];
}

// CNT pixel tiles (pslot + PW j, j < CNT: all real tiles) of one layer for
// this wave's channel tile.  `in` is the padded LDS map [..][Wp][PIN] of the
// layer's input, koff(ks) the element offset of K step ks from an output
// pixel's top-left tap, store(p, oy, ox, co, v) takes the 4 finished channels
// co..co+3 of pixel p.
template <int CNT, int KS, int PW, int S, int PIN, bool DIV255, typename KOff, typename Store>
__device__ __forceinline__ void sb_tiles(const uint4 (&wf)[KS], const bf16_t* in, int Wp, int P,
                                         int Wo, int pslot, int co,
                                         const float* __restrict__ bias, KOff koff,
                                         Store store) {
  const int lane = lane_id();
  const int g = lane >> 4, m = lane & 15;
  const bf16_t* base[CNT];
  f4 acc[CNT];
#pragma unroll
  for (int j = 0; j < CNT; ++j) {
    const int p = (pslot + PW * j) * 16 + m;
    const int pp = p < P ? p : 0;  // partial tile: an in-bounds read, not stored
    const int oy = pp / Wo, ox = pp - oy * Wo;
    base[j] = in + (oy * S * Wp + ox * S) * PIN + 8 * g;
    acc[j] = f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int off = koff(ks);
    const bf8 a = __builtin_bit_cast(bf8, wf[ks]);
    bf8 b[CNT];
#pragma unroll
    for (int j = 0; j < CNT; ++j) b[j] = *reinterpret_cast<const bf8*>(base[j] + off);
#pragma unroll
    for (int j = 0; j < CNT; ++j) acc[j] = mfma32(a, b[j], acc[j]);
  }
  float bv[4];  // biases are views of a flat parameter buffer: 4-byte aligned
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = bias[co + r];
#pragma unroll
  for (int j = 0; j < CNT; ++j) {
    const int p = (pslot + PW * j) * 16 + m;
    if (p >= P) continue;
    const int oy = p / Wo, ox = p - oy * Wo;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float t = DIV255 ? __fdiv_rn(acc[j][r], 255.0f) : acc[j][r];
      v[r] = fmaxf(__fadd_rn(t, bv[r]), 0.f);
    }
    store(p, oy, ox, co, make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])));
  }
}

// One layer.  The 8 waves split NT channel tiles x PW = 8 / NT pixel-tile
// classes; a wave's tile count (wave-uniform, <= MT by sb_plan) picks a fully
// unrolled body, so no MFMA sits behind a branch.
template <int KS, int NT, int MT, int S, int PIN, bool DIV255, typename KOff, typename Store>
__device__ __forceinline__ void sb_layer(const uint4 (&wf)[KS], const bf16_t* in, int Wp,
                                         int Ho, int Wo, const float* __restrict__ bias,
                                         KOff koff, Store store) {
  constexpr int PW = kSbWaves / NT;
  const int wave = wave_id();
  const int nt = wave % NT, pslot = wave / NT;
  const int P = Ho * Wo;
  const int ntiles = (P + 15) >> 4;
  const int cnt = (ntiles - pslot + PW - 1) / PW;
  const int co = 16 * nt + 4 * (lane_id() >> 4);
#define SA_SB_CASE(C)                                                                  \
  if constexpr (MT >= C)                                                               \
    if (cnt == C)                                                                      \
      sb_tiles<C, KS, PW, S, PIN, DIV255>(wf, in, Wp, P, Wo, pslot, co, bias, koff, store);     
  SA_SB_CASE(1) SA_SB_CASE(2) SA_SB_CASE(3) SA_SB_CASE(4) SA_SB_CASE(5)
  SA_SB_CASE(6) SA_SB_CASE(7) SA_SB_CASE(8) SA_SB_CASE(9)
#undef SA_SB_CASE
  static_assert(MT <= 9, "tile-count cases");
}

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

// TF-SAME geometry of one conv: output size, pad_before, padded input size
// (0 where the pad would be negative: not a shape of this torso).
bool sb_geom(int n, int k, int s, int* out, int* before, int* padded) {
  *out = (n + s - 1) / s;
  const int total = (*out - 1) * s + k - n;
  *before = total / 2;
  *padded = n + total;
  return total >= 0;
}

// Geometry and LDS bytes on [H, W, C] frames; 0 where it does not fit the
// kernel's buffers and wave split.
size_t sb_plan(int H, int W, int C, ShallowBf16Args* a) {
  a->H = H; a->W = W; a->C = C;
  bool ok = sb_geom(H, 8, 4, &a->H1, &a->pt1, &a->Hp0);
  ok = sb_geom(W, 8, 4, &a->W1, &a->pl1, &a->Wp0) && ok;
  ok = sb_geom(a->H1, 4, 2, &a->H2, &a->pt2, &a->Hp1) && ok;
  ok = sb_geom(a->W1, 4, 2, &a->W2, &a->pl2, &a->Wp1) && ok;
  ok = sb_geom(a->H2, 3, 2, &a->H3, &a->pt3, &a->Hp2) && ok;
  ok = sb_geom(a->W2, 3, 2, &a->W3, &a->pl3, &a->Wp2) && ok;
  if (!ok) return 0;
  const size_t f0 = static_cast<size_t>(a->Hp0) * a->Wp0 * 4 * 2;
  const size_t f1 = static_cast<size_t>(a->Hp1) * a->Wp1 * kSbPitch1 * 2;
  const size_t f2 = static_cast<size_t>(a->Hp2) * a->Wp2 * kSbPitch2 * 2;
  const size_t frame = static_cast<size_t>(H) * W * C;
  // 16-byte operand reads: an even padded frame width, 16-byte regions
  if (a->Wp0 % 2 != 0 || f0 % 16 != 0 || f1 % 16 != 0 || f2 % 16 != 0) return 0;
  if (frame % 4 != 0 || frame > f1) return 0;  // dword copy, staged in a1
  const int PW1 = kSbWaves / 2, PW2 = kSbWaves / 4, PW3 = kSbWaves / 8;
  if ((a->H1 * a->W1 + 15) / 16 > PW1 * kSbMt1 || (a->H2 * a->W2 + 15) / 16 > PW2 * kSbMt2 ||
      (a->H3 * a->W3 + 15) / 16 > PW3 * kSbMt3)
    return 0;
  const size_t bytes = f0 + f1 + f2;
  return bytes <= kSbLdsMax ? bytes : 0;
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

}  // namespace conv
}  // namespace sa
