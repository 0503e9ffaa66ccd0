// Shared between the shallow torso's bf16 kernels: the inference launch
// (conv_shallow_bf16.hip) and the learner's forward (conv_shallow_bf16_train.hip)
// run the same tile body and layer split over the same LDS geometry, so the
// two accumulate every element in the same order.  See conv_shallow_bf16.hip
// for the layout and the rounding points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "conv_common.h"

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
// co..co+3 of pixel p: packed bf16 (uint2), or with F32OUT the unrounded fp32
// values (f4).
template <int CNT, int KS, int PW, int S, int PIN, bool DIV255, bool F32OUT, typename KOff,
          typename Store>
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
    if constexpr (F32OUT)
      store(p, oy, ox, co, f4{v[0], v[1], v[2], v[3]});
    else
      store(p, oy, ox, co, make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])));
  }
}

// One layer.  The 8 waves split NT channel tiles x PW = 8 / NT pixel-tile
// classes; a wave's tile count (wave-uniform, <= MT by sb_plan) picks a fully
// unrolled body, so no MFMA sits behind a branch.
template <int KS, int NT, int MT, int S, int PIN, bool DIV255, bool F32OUT = false,
          typename KOff, typename Store>
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
      sb_tiles<C, KS, PW, S, PIN, DIV255, F32OUT>(wf, in, Wp, P, Wo, pslot, co, bias,  \
                                                  koff, store);
  SA_SB_CASE(1) SA_SB_CASE(2) SA_SB_CASE(3) SA_SB_CASE(4) SA_SB_CASE(5)
  SA_SB_CASE(6) SA_SB_CASE(7) SA_SB_CASE(8) SA_SB_CASE(9)
#undef SA_SB_CASE
  static_assert(MT <= 9, "tile-count cases");
}

// TF-SAME geometry of one conv: output size, pad_before, padded input size
// (0 where the pad would be negative: not a shape of this torso).
inline bool sb_geom(int n, int k, int s, int* out, int* before, int* padded) {
  *out = (n + s - 1) / s;
  const int total = (*out - 1) * s + k - n;
  *before = total / 2;
  *padded = n + total;
  return total >= 0;
}

// The three layers' geometry on [H, W, C] frames.
inline bool sb_dims(int H, int W, int C, ShallowBf16Args* a) {
  a->H = H; a->W = W; a->C = C;
  bool ok = sb_geom(H, 8, 4, &a->H1, &a->pt1, &a->Hp0);
  ok = sb_geom(W, 8, 4, &a->W1, &a->pl1, &a->Wp0) && ok;
  ok = sb_geom(a->H1, 4, 2, &a->H2, &a->pt2, &a->Hp1) && ok;
  ok = sb_geom(a->W1, 4, 2, &a->W2, &a->pl2, &a->Wp1) && ok;
  ok = sb_geom(a->H2, 3, 2, &a->H3, &a->pt3, &a->Hp2) && ok;
  ok = sb_geom(a->W2, 3, 2, &a->W3, &a->pl3, &a->Wp2) && ok;
  return ok;
}

// Geometry and LDS bytes on [H, W, C] frames; 0 where it does not fit the
// kernel's buffers and wave split.
inline size_t sb_plan(int H, int W, int C, ShallowBf16Args* a) {
  if (!sb_dims(H, W, C, a)) return 0;
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

// ---- frames of 5 to 16 channels (shallow_bf16w_kernel and the learner's wide
// kernels; see conv_shallow_bf16.hip for the band layout) ----
constexpr int kSbwMt1 = 3;  // layer-1 pixel tiles per wave and band
constexpr int kSbwPx = 6;   // band pixels staged per thread

struct ShallowBf16wArgs {
  ShallowBf16Args g;  // pointers and geometry as above; g.C = the frame's C
  int R, bands;       // layer-1 output rows per band; ceil(H1 / R)
};

// bytes b0..b3 of v -> four bf16 integers (exact: 8 significant bits)
__device__ __forceinline__ uint2 sbw_expand(uint32_t v) {
  const uint32_t f0 = __float_as_uint(static_cast<float>(v & 0xffu));
  const uint32_t f1 = __float_as_uint(static_cast<float>((v >> 8) & 0xffu));
  const uint32_t f2 = __float_as_uint(static_cast<float>((v >> 16) & 0xffu));
  const uint32_t f3 = __float_as_uint(static_cast<float>(v >> 24));
  return make_uint2((f0 >> 16) | (f1 & 0xffff0000u), (f2 >> 16) | (f3 & 0xffff0000u));
}

// This thread's pixels of the band of `nrows` padded rows from padded row r0
// of one image (img: its first dword): q[u] = the pixel's bytes, channels
// past C and pixels of the TF-SAME ring zero.
template <int CPQ>
__device__ __forceinline__ void sbw_fetch(const ShallowBf16Args& a,
                                          const uint32_t* __restrict__ img, int tid, int r0,
                                          int nrows, uint32_t (&q)[kSbwPx][CPQ]) {
  const int npx = nrows * a.Wp0;
  const uint32_t tail = 0xffffffffu >> (8 * (4 * CPQ - a.C));  // C in (Cp - 4, Cp]
#pragma unroll
  for (int u = 0; u < kSbwPx; ++u) {
    const int e = tid + u * kSbThreads;
    const int r = e / a.Wp0, x = e - r * a.Wp0;
    const int iy = r0 + r - a.pt1, ix = x - a.pl1;
#pragma unroll
    for (int k = 0; k < CPQ; ++k) q[u][k] = 0u;
    if (e < npx && static_cast<unsigned>(iy) < static_cast<unsigned>(a.H) &&
        static_cast<unsigned>(ix) < static_cast<unsigned>(a.W)) {
      const uint32_t o = static_cast<uint32_t>((iy * a.W + ix) * a.C);
      // uniform base + 32-bit byte offset: one address register per pixel
      const uint32_t* s = reinterpret_cast<const uint32_t*>(
          reinterpret_cast<const unsigned char*>(img) + (o & ~3u));
      // the pixel's last byte is in dword CPQ - 1 or CPQ from s; the image
      // ends on a dword, so nothing past it is read
      const bool extra = ((o + a.C - 1) >> 2) - (o >> 2) >= static_cast<uint32_t>(CPQ);
      uint32_t d[CPQ + 1];
#pragma unroll
      for (int k = 0; k < CPQ; ++k) d[k] = s[k];
      d[CPQ] = extra ? s[CPQ] : 0u;
#pragma unroll
      for (int k = 0; k < CPQ; ++k) q[u][k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], o & 3u);
      q[u][CPQ - 1] &= tail;
    }
  }
}

template <int CPQ>
__device__ __forceinline__ void sbw_put(const uint32_t (&q)[kSbwPx][CPQ], int tid, int npx,
                                        bf16_t* band) {
#pragma unroll
  for (int u = 0; u < kSbwPx; ++u) {
    const int e = tid + u * kSbThreads;
    if (e >= npx) continue;
    uint2* dst = reinterpret_cast<uint2*>(band + e * (4 * CPQ));
#pragma unroll
    for (int k = 0; k < CPQ; ++k) dst[k] = sbw_expand(q[u][k]);
  }
}

// shallow_bf16w_kernel on [H, W, C] frames, 5 <= C <= 16: geometry, the band
// height R and the LDS bytes; 0 where it does not fit.  R is the most rows
// whose band [4 R + 4][Wp0][Cp] fits beside a1 and a2 in 160 KB (72x128x16:
// 82512 bytes at 4224 per row, R = 3; 72x96x16: 101648 at 3200, R = 6) within
// the kernel's kSbwPx staged pixels per thread and kSbwMt1 tiles per wave,
// then evened out over the band count.
size_t sbw_plan(int H, int W, int C, ShallowBf16wArgs* wa) {
  ShallowBf16Args* a = &wa->g;
  if (C < 5 || C > 16 || !sb_dims(H, W, C, a)) return 0;
  const int Cp = (C + 3) / 4 * 4;
  const size_t row = static_cast<size_t>(a->Wp0) * Cp * 2;
  const size_t f1 = static_cast<size_t>(a->Hp1) * a->Wp1 * kSbPitch1 * 2;
  const size_t f2 = static_cast<size_t>(a->Hp2) * a->Wp2 * kSbPitch2 * 2;
  // 16-byte operand reads and regions; whole dwords per image
  if (a->Wp0 % 2 != 0 || f1 % 16 != 0 || f2 % 16 != 0) return 0;
  if ((static_cast<size_t>(H) * W * C) % 4 != 0) return 0;
  const int PW2 = kSbWaves / 4, PW3 = kSbWaves / 8;
  if ((a->H2 * a->W2 + 15) / 16 > PW2 * kSbMt2 || (a->H3 * a->W3 + 15) / 16 > PW3 * kSbMt3)
    return 0;
  if (f1 + f2 + 8 * row > kSbLdsMax) return 0;
  int rows = static_cast<int>((kSbLdsMax - f1 - f2) / row);
  rows = std::min(rows, kSbwPx * kSbThreads / a->Wp0);
  int R = (rows - 4) / 4;
  R = std::min(R, (kSbWaves / 2) * kSbwMt1 * 16 / a->W1);
  R = std::min(R, a->H1);
  if (R < 1) return 0;
  wa->bands = (a->H1 + R - 1) / R;
  wa->R = (a->H1 + wa->bands - 1) / wa->bands;
  return (4 * wa->R + 4) * row + f1 + f2;
}

}  // namespace
}  // namespace conv
}  // namespace sa
