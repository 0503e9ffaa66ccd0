// The shallow conv torso's bf16 TRAINING form (gfx950): forward with saved
// maps, data gradient, weight / bias gradients.  Only the three convs run in
// bf16 (v_mfma_f32_16x16x32_bf16, fp32 accumulation); features and parameter
// gradients are fp32.  72x96, 84x84 or 72x128 frames: 1-4 channels with the
// kernels described first, 5-16 channels with the wide forward
// (sbtw_fwd_kernel, family shallow_bf16w_train_fwd) and the wide layer-1
// weight gradient (sbtw_wgrad1_kernel, family shallow_bf16w_wgrad1) described
// where they stand; the data gradient, the layer 2 / 3 weight gradients, the
// pack and the reduce serve both.
//
// Every kernel walks the images with one 512-thread workgroup per image in a
// grid-stride loop (conv_tune("shallow_bf16_grid", g) caps the grid).  No
// cross-workgroup waits, no atomics, every loop bounded by N and the geometry.
//
// shallow_bf16_train_fwd   the inference kernel's image loop (conv_shallow_
//   bf16.hip: same LDS maps, tile body, layer split, packed weights, rounding
//   points and accumulation order, shared through conv_shallow_bf16.h) that
//   also stores the post-ReLU a1 / a2 as dense bf16 NHWC and the layer-3
//   output as fp32 (accumulator + bias, ReLU, NOT rounded): feats.to(bf16) is
//   bitwise the inference kernel's output.
//
// shallow_bf16_bwd_data    per image: dY3m = bf16(dfeats where feats > 0) is
//   staged into LDS as [H3+2][W3+2][136] with a zero ring; the layer-3 data
//   gradient (3x3/2, 128 -> 64) and then the layer-2 one (4x4/2, 64 -> 32,
//   reading dA2 from LDS [H2+2][W2+2][72]) run as MFMA implicit GEMMs over
//   (tap, cout), decomposed by the parity of the padded input pixel: an input
//   pixel u = iy + pad_before only meets taps ky = u (mod 2), at output row
//   (u - ky) / 2, so the four phases have 4 / 2 / 2 / 1 taps (3x3) or 4 each
//   (4x4) and no MFMA lands on a dilation zero; the one-pixel zero ring takes
//   the taps that fall outside the output (TF-SAME's asymmetric pads change
//   only the first pixel of each parity).  Computed transposed like the
//   forward: A = 16 input channels of the packed weights wd (read from L2),
//   B = 16 pixels of one phase, K = 32 output channels of one tap.  The ReLU
//   masks come from the saved maps at the epilogue (one 8-byte load per lane:
//   the 4 channels it finished); dA2 is rounded once to bf16 and goes to LDS
//   and HBM, dA1 to HBM.  Layer 1 has no data gradient.
//
// shallow_bf16_wgrad       dW_l = sum over images of patches(in_l)^T dOut_l,
//   one launch per layer so that each fills the whole card.  The MFMA K axis
//   is 32 output pixels: B = dOut_l transposed on its way into LDS
//   ([cout][pixels], pixels zero-padded to 32), A = 16 rows of the patch
//   matrix (one (ky, kx, ci) each) gathered from the padded NHWC input map in
//   LDS through a table of the pixels' window origins.  Layer 1's input is the
//   frame as exact bf16 integers; its single division by 255 is applied to
//   the finished sum in the reduce.  A workgroup keeps its whole layer in
//   accumulators across its images (8 waves x 4 / 16 / 36 tiles), the bias
//   gradient rides along as a row of ones, and the partial sums go to the
//   workgroup's own slot.  sbt_reduce_kernel adds the slots in a fixed order
//   into the fp32 gradients: the step is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "conv_common.h"
#include "conv_launchers.h"
#include "conv_shallow_bf16.h"

namespace sa {
namespace conv {

namespace {

constexpr int kSbtMaxN = 8192;
constexpr int kSbtPitchD3 = 136, kSbtPitchD2 = 72;  // bf16 per pixel of dY3m / dA2 in LDS
constexpr int kSbtMaxT3 = 2, kSbtMaxT2 = 3;         // phase pixel tiles per wave

// ---- weight pack ----
constexpr int kPk2 = 16 * 4 * 512, kPk3 = 18 * 8 * 512;
constexpr int kPkD2 = 16 * 2 * 2 * 512, kPkD3 = 9 * 4 * 4 * 512;
constexpr int kPkRest = kPk2 + kPk3 + kPkD2 + kPkD3;
// layer 1: 2 Cp K steps x 2 channel tiles (Cp = 4, or 8 / 12 / 16 for the wide kernels)
__host__ __device__ constexpr int sbt_pk1(int Cp) { return 2 * Cp * 2 * 512; }

struct SbtPackArgs {
  const float *w1, *w2, *w3;
  bf16_t *w1p, *w2p, *w3p, *wd2, *wd3;
  int C, Cp;  // w1's input channels, and as the forward stages them
};

__global__ __launch_bounds__(256) void sbt_pack_kernel(SbtPackArgs a) {
  int e = blockIdx.x * 256 + threadIdx.x;
  const int pk1 = sbt_pk1(a.Cp);
  if (e >= pk1 + kPkRest) return;
  const int j = e & 7, lane = (e >> 3) & 63, g = lane >> 4, m = lane & 15;
  // forward operand [kstep][ntile][lane][8] over Wflat [K, cout]
  auto fwd = [&](int f, int NT, int* k, int* co) {
    *co = 16 * (f % NT) + m;
    *k = 32 * (f / NT) + 8 * g + j;
  };
  // dgrad operand [tap][kq][ct][lane][8]: rows ci, k = co
  auto dg = [&](int f, int CT, int KQ, int CIN, int COUT) {
    const int ci = 16 * (f % CT) + m, co = 32 * ((f / CT) % KQ) + 8 * g + j;
    return ((f / (CT * KQ)) * CIN + ci) * COUT + co;
  };
  int k, co;
  if (e < pk1) {
    fwd(e >> 9, 2, &k, &co);
    const int tap = k / a.Cp, ci = k - tap * a.Cp;
    a.w1p[e] = ci < a.C ? f2bf(a.w1[(tap * a.C + ci) * 32 + co]) : bf16_t{0};
    return;
  }
  e -= pk1;
  if (e < kPk2) {
    fwd(e >> 9, 4, &k, &co);
    a.w2p[e] = f2bf(a.w2[k * 64 + co]);
    return;
  }
  e -= kPk2;
  if (e < kPk3) {
    fwd(e >> 9, 8, &k, &co);
    a.w3p[e] = f2bf(a.w3[k * 128 + co]);
    return;
  }
  e -= kPk3;
  if (e < kPkD2) {
    a.wd2[e] = f2bf(a.w2[dg(e >> 9, 2, 2, 32, 64)]);
    return;
  }
  e -= kPkD2;
  a.wd3[e] = f2bf(a.w3[dg(e >> 9, 4, 4, 64, 128)]);
}

// ---- forward ----
struct SbtFwdArgs {
  ShallowBf16Args g;  // g.out unused
  float* feats;       // [N, H3, W3, 128]
  bf16_t *a1, *a2;    // [N, H1, W1, 32], [N, H2, W2, 64]
};

__global__ __launch_bounds__(kSbThreads) void sbt_fwd_kernel(SbtFwdArgs ta) {
  const ShallowBf16Args& a = ta.g;
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* fr = reinterpret_cast<bf16_t*>(sb_smem);
  bf16_t* a1 = fr + a.Hp0 * a.Wp0 * 4;
  bf16_t* a2 = a1 + a.Hp1 * a.Wp1 * kSbPitch1;
  const int n1 = a.Hp1 * a.Wp1 * kSbPitch1;
  const int n2 = a.Hp2 * a.Wp2 * kSbPitch2;
  const int lane = lane_id(), wave = wave_id();
  const uint4 z4 = make_uint4(0, 0, 0, 0);

  for (int e = threadIdx.x; e < n2 / 8; e += kSbThreads) reinterpret_cast<uint4*>(a2)[e] = z4;

  const int ndw = (a.H * a.W * a.C) >> 2;
  const int P1 = a.H1 * a.W1, P2 = a.H2 * a.W2, P3 = a.H3 * a.W3;
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    int z = 0;  // opaque per image, as in shallow_bf16_kernel (fragment liveness)
    asm volatile("" : "+s"(z));
    const uint4 *w1 = a.w1 + z, *w2 = a.w2 + z, *w3 = a.w3 + z;
    uint4 wf1[8], wf2[16], wf3[18];
    load_frags<8, 2>(w1, wave % 2, lane, wf1);
    const uint32_t* src =
        reinterpret_cast<const uint32_t*>(a.frames + static_cast<int64_t>(n) * ndw * 4);
    uint32_t* raw = reinterpret_cast<uint32_t*>(a1);
    for (int d = threadIdx.x; d < ndw; d += kSbThreads) raw[d] = src[d];
    __syncthreads();
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
    load_frags<16, 4>(w2, wave % 4, lane, wf2);
    __syncthreads();

    {
      const int Wp0 = a.Wp0, Wp1 = a.Wp1, pt = a.pt2, pl = a.pl2;
      bf16_t* o = ta.a1 + static_cast<int64_t>(n) * P1 * 32;
      sb_layer<8, 2, kSbMt1, 4, 4, true>(
          wf1, fr, Wp0, a.H1, a.W1, a.b1,
          [=](int ks) { return ks * Wp0 * 4; },
          [=](int p, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a1 + ((oy + pt) * Wp1 + ox + pl) * kSbPitch1 + co) = v;
            *reinterpret_cast<uint2*>(o + p * 32 + co) = v;
          });
    }
    load_frags<18, 8>(w3, wave, lane, wf3);
    __syncthreads();
    {
      const int Wp1 = a.Wp1, Wp2 = a.Wp2, pt = a.pt3, pl = a.pl3;
      bf16_t* o = ta.a2 + static_cast<int64_t>(n) * P2 * 64;
      sb_layer<16, 4, kSbMt2, 2, kSbPitch1, false>(
          wf2, a1, Wp1, a.H2, a.W2, a.b2,
          [=](int ks) { return ((ks >> 2) * Wp1 + (ks & 3)) * kSbPitch1; },
          [=](int p, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a2 + ((oy + pt) * Wp2 + ox + pl) * kSbPitch2 + co) = v;
            *reinterpret_cast<uint2*>(o + p * 64 + co) = v;
          });
    }
    __syncthreads();
    {
      const int Wp2 = a.Wp2;
      float* o = ta.feats + static_cast<int64_t>(n) * P3 * 128;
      sb_layer<18, 8, kSbMt3, 2, kSbPitch2, false, true>(
          wf3, a2, Wp2, a.H3, a.W3, a.b3,
          [=](int ks) {
            const int tap = ks >> 1;
            return ((tap / 3) * Wp2 + tap % 3) * kSbPitch2 + (ks & 1) * 32;
          },
          [=](int p, int, int, int co, f4 v) { *reinterpret_cast<f4*>(o + p * 128 + co) = v; });
    }
  }
}

// ---- forward, frames of 5 to 16 channels ----
// shallow_bf16w_kernel's image loop (conv_shallow_bf16.hip: layer 1 in bands
// of R output rows, the same stager, fragments, K steps and barriers) with the
// three extra stores.  a1 leaves from the band epilogue that writes it into
// LDS: the lane holds the packed value there, a band's rows are whole rows of
// the dense map (pixel oy0 W1 + p), and a pass over LDS per image would cost a
// barrier and a walk of the pitch-40 map for the same bytes.
struct SbtwFwdArgs {
  ShallowBf16wArgs w;  // w.g.out unused
  float* feats;
  bf16_t *a1, *a2;
};

template <int CPQ>
__global__ __launch_bounds__(kSbThreads) void sbtw_fwd_kernel(SbtwFwdArgs ta) {
  constexpr int CP = 4 * CPQ, KS1 = 8 * CPQ;
  const ShallowBf16Args& a = ta.w.g;
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* band = reinterpret_cast<bf16_t*>(sb_smem);
  bf16_t* a1 = band + (4 * ta.w.R + 4) * a.Wp0 * CP;
  bf16_t* a2 = a1 + a.Hp1 * a.Wp1 * kSbPitch1;
  const int n12 = a.Hp1 * a.Wp1 * kSbPitch1 + a.Hp2 * a.Wp2 * kSbPitch2;  // multiple of 8
  const uint4 z4 = make_uint4(0, 0, 0, 0);

  for (int e = threadIdx.x; e < n12 / 8; e += kSbThreads) reinterpret_cast<uint4*>(a1)[e] = z4;

  const int ndw = (a.H * a.W * a.C) >> 2;
  const int P1 = a.H1 * a.W1, P2 = a.H2 * a.W2, P3 = a.H3 * a.W3;
  const int Wp0 = a.Wp0, Wp1 = a.Wp1, Wp2 = a.Wp2, R = ta.w.R;
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    int z = 0;  // opaque per image, as in shallow_bf16w_kernel
    asm volatile("" : "+s"(z));
    const uint4 *w1 = a.w1 + z, *w2 = a.w2 + z, *w3 = a.w3 + z;
    uint4 wf1[KS1], wf2[16], wf3[18];
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t* img = reinterpret_cast<const uint32_t*>(a.frames) + static_cast<int64_t>(n) * ndw;
    auto layer1 = [&](int oy0) {
      const int pt = a.pt2, pl = a.pl2;
      bf16_t* o = ta.a1 + (static_cast<int64_t>(n) * P1 + oy0 * a.W1) * 32;
      sb_layer<KS1, 2, kSbwMt1, 4, CP, true>(
          wf1, band, Wp0, min(R, a.H1 - oy0), a.W1, a.b1,
          [=](int ks) { return (ks / CPQ) * Wp0 * CP + (ks % CPQ) * 32; },
          [=](int p, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a1 + ((oy0 + oy + pt) * Wp1 + ox + pl) * kSbPitch1 + co) = v;
            *reinterpret_cast<uint2*>(o + p * 32 + co) = v;
          });
    };
    auto band_rows = [&](int oy0) { return 4 * min(R, a.H1 - oy0) + 4; };
    {
      uint32_t q[kSbwPx][CPQ];
      sbw_fetch<CPQ>(a, img, tid, 0, band_rows(0), q);
      load_frags<KS1, 2>(w1, wave % 2, lane, wf1);
      sbw_put<CPQ>(q, tid, band_rows(0) * Wp0, band);
    }
    __syncthreads();
    int oy0 = 0;
    for (; oy0 + R < a.H1; oy0 += R) {
      uint32_t q[kSbwPx][CPQ];
      sbw_fetch<CPQ>(a, img, tid, 4 * (oy0 + R), band_rows(oy0 + R), q);
      layer1(oy0);
      __syncthreads();
      sbw_put<CPQ>(q, tid, band_rows(oy0 + R) * Wp0, band);
      __syncthreads();
    }
    if constexpr (CPQ < 4) load_frags<16, 4>(w2, wave % 4, lane, wf2);
    layer1(oy0);
    if constexpr (CPQ == 4) load_frags<16, 4>(w2, wave % 4, lane, wf2);
    load_frags<18, 8>(w3, wave, lane, wf3);
    __syncthreads();
    {
      const int pt = a.pt3, pl = a.pl3;
      bf16_t* o = ta.a2 + static_cast<int64_t>(n) * P2 * 64;
      sb_layer<16, 4, kSbMt2, 2, kSbPitch1, false>(
          wf2, a1, Wp1, a.H2, a.W2, a.b2,
          [=](int ks) { return ((ks >> 2) * Wp1 + (ks & 3)) * kSbPitch1; },
          [=](int p, int oy, int ox, int co, uint2 v) {
            *reinterpret_cast<uint2*>(a2 + ((oy + pt) * Wp2 + ox + pl) * kSbPitch2 + co) = v;
            *reinterpret_cast<uint2*>(o + p * 64 + co) = v;
          });
    }
    __syncthreads();
    {
      float* o = ta.feats + static_cast<int64_t>(n) * P3 * 128;
      sb_layer<18, 8, kSbMt3, 2, kSbPitch2, false, true>(
          wf3, a2, Wp2, a.H3, a.W3, a.b3,
          [=](int ks) {
            const int tap = ks >> 1;
            return ((tap / 3) * Wp2 + tap % 3) * kSbPitch2 + (ks & 1) * 32;
          },
          [=](int p, int, int, int co, f4 v) { *reinterpret_cast<f4*>(o + p * 128 + co) = v; });
    }
  }
}

// ---- data gradient ----
struct SbtBwdArgs {
  const float *dfeats, *feats;  // [N, H3, W3, 128]
  const bf16_t *a2, *a1;        // saved post-ReLU maps
  const uint4 *wd3, *wd2;       // packed dgrad operands
  bf16_t *dy3m, *da2, *da1;     // dense NHWC
  int N;
  int H1, W1, H2, W2, H3, W3;
  int pt2, pl2, pt3, pl3;
};

// Pixels of one parity of a padded axis: the first padded coordinate u0 >= pad
// with u0 = par (mod 2) and how many there are among pad .. pad + n - 1.
__host__ __device__ inline void sbt_phase(int n, int pad, int par, int* u0, int* cnt) {
  *u0 = pad + ((par - pad) & 1);
  *cnt = *u0 <= pad + n - 1 ? (pad + n - 1 - *u0) / 2 + 1 : 0;
}

// The data gradient of one KHxKH / 2 conv, COUT -> CIN channels, for one
// image.  dout: LDS [Ho + 2][Wo + 2][PD] with a zero ring.  The 8 waves split
// CIN / 16 channel tiles x the pixel tiles of each phase; epi(iy, ix, ci, acc)
// takes input channels ci..ci+3 of input pixel (iy, ix).
template <int KH, int CIN, int COUT, int PD, int MAXT, typename Epi>
__device__ __forceinline__ void sbt_dgrad(const bf16_t* dout, int Wo, int Hi, int Wi, int pt,
                                          int pl, const uint4* __restrict__ wd, Epi epi) {
  constexpr int CT = CIN / 16, KQ = COUT / 32, PW = kSbWaves / CT;
  const int wave = wave_id(), lane = lane_id(), g = lane >> 4, m = lane & 15;
  const int ct = wave % CT, pslot = wave / CT;
  const int Wd = Wo + 2;
  for (int ph = 0; ph < 4; ++ph) {
    const int py = ph >> 1, px = ph & 1;
    int u0, R, v0, Cc;
    sbt_phase(Hi, pt, py, &u0, &R);
    sbt_phase(Wi, pl, px, &v0, &Cc);
    const int P = R * Cc;
    const int cnt = (((P + 15) >> 4) - pslot + PW - 1) / PW;  // wave-uniform, <= MAXT by the plan
    if (cnt <= 0) continue;
    int base[MAXT];
    f4 acc[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
      const int p = (pslot + PW * j) * 16 + m;
      const int pp = p < P ? p : 0;  // partial tile: an in-bounds read, not stored
      const int r = pp / Cc, c = pp - r * Cc;
      base[j] = ((r + 1) * Wd + c + 1) * PD + 8 * g;
      acc[j] = f4{0.f, 0.f, 0.f, 0.f};
    }
    for (int ky = py; ky < KH; ky += 2) {
      for (int kx = px; kx < KH; kx += 2) {
        // u0 - ky and v0 - kx are even: output pixel ((u - ky) / 2, (v - kx) / 2)
        const int toff = (((u0 - ky) / 2) * Wd + (v0 - kx) / 2) * PD;
        const uint4* wt = wd + ((ky * KH + kx) * KQ * CT + ct) * 64 + lane;
        uint4 wf[KQ];
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) wf[kq] = wt[kq * CT * 64];
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) {
          const bf8 av = __builtin_bit_cast(bf8, wf[kq]);
#pragma unroll
          for (int j = 0; j < MAXT; ++j)
            if (j < cnt)
              acc[j] = mfma32(av, *reinterpret_cast<const bf8*>(dout + base[j] + toff + 32 * kq),
                              acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
      const int p = (pslot + PW * j) * 16 + m;
      if (j >= cnt || p >= P) continue;
      const int r = p / Cc, c = p - r * Cc;
      epi(u0 + 2 * r - pt, v0 + 2 * c - pl, 16 * ct + 4 * g, acc[j]);
    }
  }
}

// acc where the saved post-ReLU activation is not zero, rounded once to bf16
__device__ __forceinline__ uint2 sbt_mask_pack(f4 acc, uint2 act) {
  const float v0 = (act.x & 0x7fffu) ? acc[0] : 0.f;
  const float v1 = (act.x & 0x7fff0000u) ? acc[1] : 0.f;
  const float v2 = (act.y & 0x7fffu) ? acc[2] : 0.f;
  const float v3 = (act.y & 0x7fff0000u) ? acc[3] : 0.f;
  return make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
}

__global__ __launch_bounds__(kSbThreads) void sbt_bwd_data_kernel(SbtBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* d3 = reinterpret_cast<bf16_t*>(sb_smem);
  const int Wd3 = a.W3 + 2, Wd2 = a.W2 + 2;
  const int n3 = (a.H3 + 2) * Wd3 * kSbtPitchD3, n2 = (a.H2 + 2) * Wd2 * kSbtPitchD2;
  bf16_t* d2 = d3 + n3;
  // both zero rings, once: only interiors are stored below
  for (int e = threadIdx.x; e < (n3 + n2) / 8; e += kSbThreads)
    reinterpret_cast<uint4*>(d3)[e] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int P1 = a.H1 * a.W1, P2 = a.H2 * a.W2, P3 = a.H3 * a.W3;
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    {
      const int64_t o = static_cast<int64_t>(n) * P3 * 128;
      const float4* df = reinterpret_cast<const float4*>(a.dfeats + o);
      const float4* ft = reinterpret_cast<const float4*>(a.feats + o);
      uint2* dg = reinterpret_cast<uint2*>(a.dy3m + o);
      for (int e = threadIdx.x; e < P3 * 32; e += kSbThreads) {
        const float4 d = df[e], f = ft[e];
        const uint2 v = make_uint2(pack_bf16x2(f.x > 0.f ? d.x : 0.f, f.y > 0.f ? d.y : 0.f),
                                   pack_bf16x2(f.z > 0.f ? d.z : 0.f, f.w > 0.f ? d.w : 0.f));
        const int p = e >> 5, oy = p / a.W3, ox = p - oy * a.W3;
        *reinterpret_cast<uint2*>(d3 + ((oy + 1) * Wd3 + ox + 1) * kSbtPitchD3 + (e & 31) * 4) = v;
        dg[e] = v;
      }
    }
    __syncthreads();
    {
      const int W2 = a.W2;
      const bf16_t* act = a.a2 + static_cast<int64_t>(n) * P2 * 64;
      bf16_t* o = a.da2 + static_cast<int64_t>(n) * P2 * 64;
      sbt_dgrad<3, 64, 128, kSbtPitchD3, kSbtMaxT3>(
          d3, a.W3, a.H2, a.W2, a.pt3, a.pl3, a.wd3, [=](int iy, int ix, int ci, f4 acc) {
            const int q = (iy * W2 + ix) * 64 + ci;
            const uint2 v = sbt_mask_pack(acc, *reinterpret_cast<const uint2*>(act + q));
            *reinterpret_cast<uint2*>(d2 + ((iy + 1) * Wd2 + ix + 1) * kSbtPitchD2 + ci) = v;
            *reinterpret_cast<uint2*>(o + q) = v;
          });
    }
    __syncthreads();
    {
      const int W1 = a.W1;
      const bf16_t* act = a.a1 + static_cast<int64_t>(n) * P1 * 32;
      bf16_t* o = a.da1 + static_cast<int64_t>(n) * P1 * 32;
      sbt_dgrad<4, 32, 64, kSbtPitchD2, kSbtMaxT2>(
          d2, a.W2, a.H1, a.W1, a.pt2, a.pl2, a.wd2, [=](int iy, int ix, int ci, f4 acc) {
            const int q = (iy * W1 + ix) * 32 + ci;
            *reinterpret_cast<uint2*>(o + q) =
                sbt_mask_pack(acc, *reinterpret_cast<const uint2*>(act + q));
          });
    }
    // the next image's dY3m staging touches d3 only (layer 3 ended at a
    // barrier); its first write to d2 is behind the staging barrier
  }
}

// ---- weight and bias gradients ----
// Per layer: kernel size, stride, channels and pixel pitch of the padded input
// map, output channels; RT patch-row tiles x CW output-channel tiles per wave
// (K / 16 / RT row groups x COUT / 16 / CW channel groups = 8 waves).
template <int L> struct SbtWg;
template <> struct SbtWg<1> { static constexpr int KH = 8, S = 4, CIN = 4, PIN = 4, COUT = 32, RT = 2, CW = 2; };
template <> struct SbtWg<2> { static constexpr int KH = 4, S = 2, CIN = 32, PIN = kSbPitch1, COUT = 64, RT = 4, CW = 4; };
template <> struct SbtWg<3> { static constexpr int KH = 3, S = 2, CIN = 64, PIN = kSbPitch2, COUT = 128, RT = 9, CW = 4; };
template <int L> constexpr int sbt_k() { return SbtWg<L>::KH * SbtWg<L>::KH * SbtWg<L>::CIN; }
template <int L> constexpr int sbt_slot() { return (sbt_k<L>() + 1) * SbtWg<L>::COUT; }
// layer 1 at Cp staged channels: 64 Cp patch rows and the bias row
__host__ __device__ constexpr int sbt_slot1(int Cp) { return (64 * Cp + 1) * 32; }
static_assert(sbt_slot1(4) == sbt_slot<1>(), "the narrow layer-1 slot");

struct SbtWgArgs {
  const uint8_t* frames;  // layer 1: [N, H, W, C]
  const bf16_t* in;       // layers 2 / 3: a1 / a2, dense NHWC
  const bf16_t* dout;     // dA1 / dA2 / dY3m, dense NHWC
  float* part;            // this layer's slots [grid][(K + 1) * COUT]
  int N, C;
  int Hi, Wi, pt, pl, Hp, Wp;  // input map, pad_before, padded size
  int Ho, Wo, Ppad;            // output pixels, rounded up to 32
};

template <int L>
__global__ __launch_bounds__(kSbThreads) void sbt_wgrad_kernel(SbtWgArgs a) {
  using G = SbtWg<L>;
  constexpr int K = sbt_k<L>(), RGS = K / 16 / G::RT;
  static_assert(RGS * (G::COUT / 16 / G::CW) == kSbWaves && RGS * G::RT * 16 == K, "wave split");
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* map = reinterpret_cast<bf16_t*>(sb_smem);  // [Hp][Wp][PIN], zero ring
  const int nmap = a.Hp * a.Wp * G::PIN, pitchT = a.Ppad + 8;
  bf16_t* dT = map + nmap;  // [COUT][pitchT]: dOut transposed, pad pixels zero
  int* tbl = reinterpret_cast<int*>(dT + G::COUT * pitchT);  // [Ppad] window origins
  uint32_t* raw = reinterpret_cast<uint32_t*>(tbl + a.Ppad);  // layer 1: the frame's bytes
  const int P = a.Ho * a.Wo, Pin = a.Hi * a.Wi;
  const int lane = lane_id(), wave = wave_id(), g = lane >> 4, m = lane & 15;
  const int rg = wave % RGS, ch = wave / RGS;

  for (int e = threadIdx.x; e < (nmap + G::COUT * pitchT) / 8; e += kSbThreads)
    reinterpret_cast<uint4*>(map)[e] = make_uint4(0, 0, 0, 0);
  for (int p = threadIdx.x; p < a.Ppad; p += kSbThreads) {
    const int oy = p / a.Wo, ox = p - oy * a.Wo;
    tbl[p] = p < P ? (oy * G::S * a.Wp + ox * G::S) * G::PIN : 0;  // pad pixels: dOut is zero
  }
  int eoff[G::RT];  // this lane's patch rows: (ky, kx, ci) as a map offset
#pragma unroll
  for (int r = 0; r < G::RT; ++r) {
    const int e = 16 * (rg * G::RT + r) + m;
    const int t = e / G::CIN;
    eoff[r] = ((t / G::KH) * a.Wp + t % G::KH) * G::PIN + e % G::CIN;
  }
  f4 acc[G::RT][G::CW], accb[G::CW];
#pragma unroll
  for (int c = 0; c < G::CW; ++c) {
    accb[c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < G::RT; ++r) acc[r][c] = f4{0.f, 0.f, 0.f, 0.f};
  }
  const uint32_t one2 = 0x3f803f80u;  // bf16 1.0 twice
  const bf8 ones = __builtin_bit_cast(bf8, make_uint4(one2, one2, one2, one2));
  const int ndw = L == 1 ? (a.Hi * a.Wi * a.C) >> 2 : 0;
  __syncthreads();

  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    // dOut^T: a thread takes 8 channels of one pixel; neighbours take
    // neighbouring pixels (neighbouring LDS halfwords of the same rows)
    const bf16_t* dsrc = a.dout + static_cast<int64_t>(n) * P * G::COUT;
    for (int e = threadIdx.x; e < P * (G::COUT / 8); e += kSbThreads) {
      const int c8 = (e / P) * 8, p = e - (e / P) * P;
      const uint4 v = *reinterpret_cast<const uint4*>(dsrc + p * G::COUT + c8);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dT[(c8 + 2 * i) * pitchT + p] = static_cast<bf16_t>(w[i] & 0xffffu);
        dT[(c8 + 2 * i + 1) * pitchT + p] = static_cast<bf16_t>(w[i] >> 16);
      }
    }
    if constexpr (L == 1) {
      const uint32_t* src =
          reinterpret_cast<const uint32_t*>(a.frames) + static_cast<int64_t>(n) * ndw;
      for (int d = threadIdx.x; d < ndw; d += kSbThreads) raw[d] = src[d];
      __syncthreads();
      // bytes -> exact bf16 integers, 4 channels per pixel (pad channels zero)
      const uint8_t* rb = reinterpret_cast<const uint8_t*>(raw);
      for (int e = threadIdx.x; e < Pin; e += kSbThreads) {
        const int iy = e / a.Wi, ix = e - iy * a.Wi;
        const uint8_t* px = rb + e * a.C;
        uint32_t h[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < a.C) h[c] = __float_as_uint(static_cast<float>(px[c])) >> 16;
        reinterpret_cast<uint2*>(map)[(iy + a.pt) * a.Wp + ix + a.pl] =
            make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
      }
    } else {
      const bf16_t* src = a.in + static_cast<int64_t>(n) * Pin * G::CIN;
      for (int e = threadIdx.x; e < Pin * (G::CIN / 8); e += kSbThreads) {
        const int pix = e / (G::CIN / 8), part = e - pix * (G::CIN / 8);
        const int iy = pix / a.Wi, ix = pix - iy * a.Wi;
        *reinterpret_cast<uint4*>(map + ((iy + a.pt) * a.Wp + ix + a.pl) * G::PIN + part * 8) =
            *reinterpret_cast<const uint4*>(src + e * 8);
      }
    }
    __syncthreads();
    for (int st = 0; st < a.Ppad / 32; ++st) {
      const int4 t0 = *reinterpret_cast<const int4*>(tbl + 32 * st + 8 * g);
      const int4 t1 = *reinterpret_cast<const int4*>(tbl + 32 * st + 8 * g + 4);
      const int pb[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
      bf8 b[G::CW];
#pragma unroll
      for (int c = 0; c < G::CW; ++c)
        b[c] = *reinterpret_cast<const bf8*>(dT + (16 * (ch * G::CW + c) + m) * pitchT + 32 * st +
                                             8 * g);
      if (rg == 0) {  // the bias gradient: a row of ones
#pragma unroll
        for (int c = 0; c < G::CW; ++c) accb[c] = mfma32(ones, b[c], accb[c]);
      }
#pragma unroll
      for (int r = 0; r < G::RT; ++r) {
        uint32_t h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = map[pb[j] + eoff[r]];
        const bf8 av = __builtin_bit_cast(
            bf8, make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                            h[6] | (h[7] << 16)));
#pragma unroll
        for (int c = 0; c < G::CW; ++c) acc[r][c] = mfma32(av, b[c], acc[r][c]);
      }
    }
    __syncthreads();  // the maps are free for the next image
  }

  float* slot = a.part + static_cast<int64_t>(blockIdx.x) * sbt_slot<L>();
#pragma unroll
  for (int c = 0; c < G::CW; ++c) {
    const int co = 16 * (ch * G::CW + c) + m;
#pragma unroll
    for (int r = 0; r < G::RT; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        slot[(16 * (rg * G::RT + r) + 4 * g + i) * G::COUT + co] = acc[r][c][i];
    if (rg == 0 && g == 0) slot[K * G::COUT + co] = accb[c][0];
  }
}

// ---- layer-1 weight gradient, frames of 5 to 16 channels ----
// The frame at Cp bf16 per pixel does not fit LDS, so the image is walked in
// the forward's bands of R layer-1 output rows: LDS holds the band's padded
// input rows [4 R + 4][Wp0][Cp] (sbw_fetch / sbw_put), that band's dA1 rows
// transposed to dT [32][ppad + 8] (pixels zero-padded to a multiple of 32:
// the last K step of a band never reads the next band) and the window origins
// of a band's pixels.  The loads of band b + 1 (frame dwords and dA1) are
// issued before the MFMAs of band b and wait in registers behind its barrier.
//
// The patch matrix has 64 Cp rows (ky, kx, ci) against 32 output channels:
// 4 Cp x 2 tiles of 16x16, every wave takes 32 CPQ consecutive rows x both
// channel tiles (8 / 12 / 16 accumulator tiles), kept across all bands and
// images of the workgroup.  Rows are dealt to tiles in PAIRS: tiles 2 q and
// 2 q + 1 of a wave hold the even and the odd rows of 32 consecutive ones, so
// lane m's two rows are channels ci, ci + 1 of one tap and one 4-byte LDS read
// per pixel feeds both tiles (8 reads and 8 v_perm-style merges for 4 MFMAs).
// Pad channels C .. Cp - 1 are staged as zeros and computed; the reduce never
// reads their rows.  The bias row of ones rides on wave 0.
constexpr int kSbwgDa = 2;  // (pixel, 8 channels) items of dA1 a thread stages per band

struct SbtwWgArgs {
  ShallowBf16Args g;   // frames and geometry; g.C = the frame's C
  const bf16_t* dout;  // dA1, dense NHWC
  float* part;         // slots [grid][sbt_slot1(Cp)]
  int R, bands, ppad;  // band rows, ceil(H1 / R), R W1 rounded up to 32
};

template <int CPQ>
__global__ __launch_bounds__(kSbThreads) void sbtw_wgrad1_kernel(SbtwWgArgs wa) {
  constexpr int CP = 4 * CPQ, RT = 2 * CPQ;  // row tiles per wave
  const ShallowBf16Args& a = wa.g;
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
  bf16_t* band = reinterpret_cast<bf16_t*>(sb_smem);
  const int nband = (4 * wa.R + 4) * a.Wp0 * CP, pitchT = wa.ppad + 8;
  bf16_t* dT = band + nband;
  int* tbl = reinterpret_cast<int*>(dT + 32 * pitchT);
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id(), g = lane >> 4, m = lane & 15;
  const int R = wa.R, W1 = a.W1, H1 = a.H1, Wp0 = a.Wp0;

  // stale rows of a short last band and dT's pad columns must be finite
  for (int e = tid; e < (nband + 32 * pitchT) / 8; e += kSbThreads)
    reinterpret_cast<uint4*>(band)[e] = make_uint4(0, 0, 0, 0);
  for (int p = tid; p < wa.ppad; p += kSbThreads) {
    const int oy = p / W1, ox = p - oy * W1;
    tbl[p] = p < R * W1 ? (oy * 4 * Wp0 + ox * 4) * CP : 0;  // pad pixels: dT is zero
  }
  int eoff[CPQ];  // this lane's row pairs: (ky, kx, even ci) as a band offset
#pragma unroll
  for (int q = 0; q < CPQ; ++q) {
    const int e = 32 * (wave * CPQ + q) + 2 * m;
    const int t = e / CP;
    eoff[q] = ((t >> 3) * Wp0 + (t & 7)) * CP + (e - t * CP);
  }
  f4 acc[RT][2], accb[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    accb[c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r][c] = f4{0.f, 0.f, 0.f, 0.f};
  }
  const uint32_t one2 = 0x3f803f80u;
  const bf8 ones = __builtin_bit_cast(bf8, make_uint4(one2, one2, one2, one2));
  const int ndw = (a.H * a.W * a.C) >> 2;
  __syncthreads();

  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    const uint32_t* img = reinterpret_cast<const uint32_t*>(a.frames) + static_cast<int64_t>(n) * ndw;
    const bf16_t* dsrc = wa.dout + static_cast<int64_t>(n) * H1 * W1 * 32;
    auto band_rows = [&](int oy0) { return 4 * min(R, H1 - oy0) + 4; };
    auto band_px = [&](int oy0) { return min(R, H1 - oy0) * W1; };
    // dA1 of the band from output row oy0: a thread takes 8 channels of a
    // pixel, neighbours take neighbouring pixels; pad pixels are zeros
    auto da_fetch = [&](int oy0, uint4 (&dq)[kSbwgDa]) {
      const int Pb = band_px(oy0), pp = (Pb + 31) & ~31;
#pragma unroll
      for (int u = 0; u < kSbwgDa; ++u) {
        const int e = tid + u * kSbThreads;
        const int c8 = e / pp, p = e - c8 * pp;
        dq[u] = make_uint4(0, 0, 0, 0);
        if (c8 < 4 && p < Pb)
          dq[u] = *reinterpret_cast<const uint4*>(dsrc + (oy0 * W1 + p) * 32 + c8 * 8);
      }
    };
    auto da_put = [&](int oy0, const uint4 (&dq)[kSbwgDa]) {
      const int pp = (band_px(oy0) + 31) & ~31;
#pragma unroll
      for (int u = 0; u < kSbwgDa; ++u) {
        const int e = tid + u * kSbThreads;
        const int c8 = e / pp, p = e - c8 * pp;
        if (c8 >= 4) continue;
        const uint32_t w[4] = {dq[u].x, dq[u].y, dq[u].z, dq[u].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dT[(c8 * 8 + 2 * i) * pitchT + p] = static_cast<bf16_t>(w[i] & 0xffffu);
          dT[(c8 * 8 + 2 * i + 1) * pitchT + p] = static_cast<bf16_t>(w[i] >> 16);
        }
      }
    };
    auto steps = [&](int oy0) {
      const int nst = (band_px(oy0) + 31) >> 5;
      for (int st = 0; st < nst; ++st) {
        const int4 t0 = *reinterpret_cast<const int4*>(tbl + 32 * st + 8 * g);
        const int4 t1 = *reinterpret_cast<const int4*>(tbl + 32 * st + 8 * g + 4);
        const int pb[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        bf8 b[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
          b[c] = *reinterpret_cast<const bf8*>(dT + (16 * c + m) * pitchT + 32 * st + 8 * g);
        if (wave == 0) {  // the bias gradient: a row of ones
#pragma unroll
          for (int c = 0; c < 2; ++c) accb[c] = mfma32(ones, b[c], accb[c]);
        }
#pragma unroll
        for (int q = 0; q < CPQ; ++q) {
          uint32_t v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            v[j] = *reinterpret_cast<const uint32_t*>(band + pb[j] + eoff[q]);
          uint32_t ev[4], od[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ev[j] = (v[2 * j] & 0xffffu) | (v[2 * j + 1] << 16);
            od[j] = (v[2 * j] >> 16) | (v[2 * j + 1] & 0xffff0000u);
          }
          const bf8 ae = __builtin_bit_cast(bf8, make_uint4(ev[0], ev[1], ev[2], ev[3]));
          const bf8 ao = __builtin_bit_cast(bf8, make_uint4(od[0], od[1], od[2], od[3]));
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            acc[2 * q][c] = mfma32(ae, b[c], acc[2 * q][c]);
            acc[2 * q + 1][c] = mfma32(ao, b[c], acc[2 * q + 1][c]);
          }
        }
      }
    };
    {
      // band and dT are free: the previous image ended with a barrier
      uint32_t q[kSbwPx][CPQ];
      uint4 dq[kSbwgDa];
      sbw_fetch<CPQ>(a, img, tid, 0, band_rows(0), q);
      da_fetch(0, dq);
      sbw_put<CPQ>(q, tid, band_rows(0) * Wp0, band);
      da_put(0, dq);
    }
    __syncthreads();
    int oy0 = 0;
    for (; oy0 + R < H1; oy0 += R) {
      uint32_t q[kSbwPx][CPQ];
      uint4 dq[kSbwgDa];
      sbw_fetch<CPQ>(a, img, tid, 4 * (oy0 + R), band_rows(oy0 + R), q);  // in flight during the MFMAs
      da_fetch(oy0 + R, dq);
      steps(oy0);
      __syncthreads();  // the band's reads are done
      sbw_put<CPQ>(q, tid, band_rows(oy0 + R) * Wp0, band);
      da_put(oy0 + R, dq);
      __syncthreads();
    }
    steps(oy0);
    __syncthreads();
  }

  float* slot = wa.part + static_cast<int64_t>(blockIdx.x) * sbt_slot1(CP);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int co = 16 * c + m;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        slot[(32 * (wave * CPQ + (r >> 1)) + 2 * (4 * g + i) + (r & 1)) * 32 + co] = acc[r][c][i];
    if (wave == 0 && g == 0) slot[64 * CP * 32 + co] = accb[c][0];
  }
}

struct SbtReduceArgs {
  const float* part;  // layer 1 slots, then layer 2, then layer 3
  float *dw1, *db1, *dw2, *db2, *dw3, *db3;
  int slots, C, Cp;  // layer 1: Cp channels per tap in a slot (4, or the wide 8 / 12 / 16)
};

// One thread per gradient element: its slots added in slot order, layer 1's
// weight sums divided by 255 (the forward's x / 255), accumulated into the
// gradient.
__global__ __launch_bounds__(256) void sbt_reduce_kernel(SbtReduceArgs a) {
  int e = blockIdx.x * 256 + threadIdx.x;
  const int n1 = 64 * a.C * 32, n2 = sbt_k<2>() * 64, n3 = sbt_k<3>() * 128;
  const float* p = a.part;
  float* dst;
  int stride, src;
  bool div = false;
  const int slot1 = sbt_slot1(a.Cp);
  if (e < n1 + 32) {
    stride = slot1;
    if (e < n1) {
      const int co = e & 31, t = e >> 5;  // t = (ky * 8 + kx) * C + ci
      src = ((t / a.C) * a.Cp + t % a.C) * 32 + co;
      dst = a.dw1 + e;
      div = true;
    } else {
      src = 64 * a.Cp * 32 + e - n1;
      dst = a.db1 + (e - n1);
    }
  } else if ((e -= n1 + 32) < n2 + 64) {
    p += static_cast<int64_t>(a.slots) * slot1;
    stride = sbt_slot<2>();
    src = e;
    dst = e < n2 ? a.dw2 + e : a.db2 + (e - n2);
  } else if ((e -= n2 + 64) < n3 + 128) {
    p += static_cast<int64_t>(a.slots) * (slot1 + sbt_slot<2>());
    stride = sbt_slot<3>();
    src = e;
    dst = e < n3 ? a.dw3 + e : a.db3 + (e - n3);
  } else {
    return;
  }
  float s = 0.f;
  for (int k = 0; k < a.slots; ++k) s = __fadd_rn(s, p[static_cast<int64_t>(k) * stride + src]);
  if (div) s = __fdiv_rn(s, 255.0f);
  *dst = __fadd_rn(*dst, s);
}

// ---- host: geometry, LDS plans, launchers ----
struct SbtPlan {
  ShallowBf16Args g;
  size_t lds_fwd, lds_bwd, lds_wg[3];
  int ppad[3];
};

int sbt_phase_tiles(int Hi, int Wi, int pt, int pl) {
  int most = 0;
  for (int ph = 0; ph < 4; ++ph) {
    int u0, R, v0, Cc;
    sbt_phase(Hi, pt, ph >> 1, &u0, &R);
    sbt_phase(Wi, pl, ph & 1, &v0, &Cc);
    most = std::max(most, (R * Cc + 15) / 16);
  }
  return most;
}

// The kernels behind layer 1 (data gradient, weight gradients of layers 2 and
// 3; with `layer1` the 1-4 channel layer-1 weight gradient too) on p->g's
// geometry.  The data gradient reads no frame bytes and layers 2 / 3 depend on
// the frame's size only, so they serve 1 to 16 channels.
bool sbt_plan_back(SbtPlan* p, bool layer1) {
  const ShallowBf16Args& a = p->g;
  const int H = a.H, W = a.W, C = a.C;
  // a one-pixel ring takes every outside tap when pad_before <= 1 (sbt_dgrad)
  if (a.pt2 > 1 || a.pl2 > 1 || a.pt3 > 1 || a.pl3 > 1) return false;
  if ((sbt_phase_tiles(a.H2, a.W2, a.pt3, a.pl3) + 1) / 2 > kSbtMaxT3 ||
      (sbt_phase_tiles(a.H1, a.W1, a.pt2, a.pl2) + 3) / 4 > kSbtMaxT2)
    return false;
  p->lds_bwd = (static_cast<size_t>(a.H3 + 2) * (a.W3 + 2) * kSbtPitchD3 +
                static_cast<size_t>(a.H2 + 2) * (a.W2 + 2) * kSbtPitchD2) * 2;
  const size_t maps[3] = {static_cast<size_t>(a.Hp0) * a.Wp0 * 4,
                          static_cast<size_t>(a.Hp1) * a.Wp1 * kSbPitch1,
                          static_cast<size_t>(a.Hp2) * a.Wp2 * kSbPitch2};
  const int px[3] = {a.H1 * a.W1, a.H2 * a.W2, a.H3 * a.W3};
  const int cout[3] = {32, 64, 128};
  bool ok = p->lds_bwd <= kSbLdsMax;
  for (int l = layer1 ? 0 : 1; l < 3; ++l) {
    p->ppad[l] = (px[l] + 31) / 32 * 32;
    p->lds_wg[l] = maps[l] * 2 + static_cast<size_t>(cout[l]) * (p->ppad[l] + 8) * 2 +
                   static_cast<size_t>(p->ppad[l]) * 4 +
                   (l == 0 ? static_cast<size_t>(H) * W * C : 0);
    ok = ok && maps[l] % 8 == 0 && p->lds_wg[l] <= kSbLdsMax;
  }
  return ok;
}

bool sbt_plan(int H, int W, int C, SbtPlan* p) {
  p->lds_fwd = sb_plan(H, W, C, &p->g);
  return p->lds_fwd && sbt_plan_back(p, true);
}

bool sbt_frame_size(int H, int W) {
  return (H == 72 && W == 96) || (H == 84 && W == 84) || (H == 72 && W == 128);
}

// The wide layer-1 weight gradient on [H, W, C] frames: the most band rows R
// within kSbwPx staged pixels and kSbwgDa dA1 items per thread and 160 KB,
// evened out over the band count; LDS bytes, 0 where it does not fit.
// 72x96: R = 6 (3 bands), 84x84: 7 (3), 72x128: 4 (5); at Cp = 16 that is
// 100992 / 101504 / 93696 bytes (band 89600 / 90112 / 84480, dT 10752 / 10752
// / 8704, origins 640 / 640 / 512).
size_t sbtw_wg_plan(int H, int W, int C, SbtwWgArgs* wa) {
  ShallowBf16Args* a = &wa->g;
  if (C < 5 || C > 16 || !sb_dims(H, W, C, a)) return 0;
  if (a->Wp0 % 2 != 0 || (static_cast<size_t>(H) * W * C) % 4 != 0) return 0;
  const int Cp = (C + 3) / 4 * 4;
  auto bytes = [&](int R) -> size_t {
    const int ppad = (R * a->W1 + 31) / 32 * 32;
    if (ppad * 4 > kSbwgDa * kSbThreads || (4 * R + 4) * a->Wp0 > kSbwPx * kSbThreads) return 0;
    const size_t b = static_cast<size_t>(4 * R + 4) * a->Wp0 * Cp * 2 +
                     static_cast<size_t>(32) * (ppad + 8) * 2 + static_cast<size_t>(ppad) * 4;
    return b <= kSbLdsMax ? b : 0;
  };
  int R = a->H1;
  while (R >= 1 && !bytes(R)) --R;
  if (R < 1) return 0;
  wa->bands = (a->H1 + R - 1) / R;
  wa->R = (a->H1 + wa->bands - 1) / wa->bands;
  wa->ppad = (wa->R * a->W1 + 31) / 32 * 32;
  return bytes(wa->R);
}

// Every plan of the wide training form; fw / wg may be null.
bool sbtw_plan(int H, int W, int C, SbtPlan* p, ShallowBf16wArgs* fw, SbtwWgArgs* wg) {
  ShallowBf16wArgs f{};
  SbtwWgArgs g{};
  p->lds_fwd = sbw_plan(H, W, C, &f);
  p->lds_wg[0] = sbtw_wg_plan(H, W, C, &g);
  p->g = f.g;
  if (!p->lds_fwd || !p->lds_wg[0] || !sbt_plan_back(p, false)) return false;
  if (fw) *fw = f;
  if (wg) *wg = g;
  return true;
}

bool sbt_mis(const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; }

template <typename Kern>
void sbt_lds(Kern kernel, size_t lds) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(lds)) != hipSuccess)
    (void)hipGetLastError();  // the launch itself reports an LDS request it cannot meet
}

}  // namespace

int shallow_bf16_train_form(int N, int H, int W, int C) {
  if (N < 1 || N > kSbtMaxN || C < 1 || C > 4) return 0;
  if (!((H == 72 && W == 96) || (H == 84 && W == 84) || (H == 72 && W == 128))) return 0;
  SbtPlan p{};
  return sbt_plan(H, W, C, &p) ? 1 : 0;
}

int shallow_bf16w_train_form(int N, int H, int W, int C) {
  if (N < 1 || N > kSbtMaxN || C < 5 || C > 16 || !sbt_frame_size(H, W)) return 0;
  SbtPlan p{};
  return sbtw_plan(H, W, C, &p, nullptr, nullptr) ? 1 : 0;
}

int shallow_bf16_train_back_form(int N, int H, int W, int C) {
  if (N < 1 || N > kSbtMaxN || C < 1 || C > 16 || !sbt_frame_size(H, W)) return 0;
  SbtPlan p{};
  return sb_dims(H, W, C, &p.g) && sbt_plan_back(&p, false) ? 1 : 0;
}

void shallow_bf16_train_pack_launch(const float* w1, const float* w2, const float* w3,
                                    void* w1p, void* w2p, void* w3p, void* wd2, void* wd3,
                                    int C, hipStream_t s) {
  SbtPackArgs a{w1, w2, w3, static_cast<bf16_t*>(w1p), static_cast<bf16_t*>(w2p),
                static_cast<bf16_t*>(w3p), static_cast<bf16_t*>(wd2), static_cast<bf16_t*>(wd3), C,
                C <= 4 ? 4 : (C + 3) / 4 * 4};
  hipLaunchKernelGGL(sbt_pack_kernel, dim3((sbt_pk1(a.Cp) + kPkRest + 255) / 256), dim3(256), 0,
                     s, a);
}

bool shallow_bf16_train_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                                   const void* w2p, const float* b2, const void* w3p,
                                   const float* b3, float* feats, void* a1, void* a2, int N,
                                   int H, int W, int C, hipStream_t s) {
  if (!shallow_bf16_train_form(N, H, W, C)) return false;
  if (sbt_mis(frames, 3) || sbt_mis(w1p, 15) || sbt_mis(w2p, 15) || sbt_mis(w3p, 15) ||
      sbt_mis(feats, 15) || sbt_mis(a1, 15) || sbt_mis(a2, 15))
    return false;
  SbtPlan p{};
  sbt_plan(H, W, C, &p);
  SbtFwdArgs ta{p.g, feats, static_cast<bf16_t*>(a1), static_cast<bf16_t*>(a2)};
  ShallowBf16Args& a = ta.g;
  a.frames = frames;
  a.w1 = static_cast<const uint4*>(w1p);
  a.w2 = static_cast<const uint4*>(w2p);
  a.w3 = static_cast<const uint4*>(w3p);
  a.b1 = b1; a.b2 = b2; a.b3 = b3;
  a.out = nullptr;
  a.N = N;
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  sbt_lds(sbt_fwd_kernel, p.lds_fwd);
  shallow_bf16_train_note(0, G, grid_max, N);
  hipLaunchKernelGGL(sbt_fwd_kernel, dim3(G), dim3(kSbThreads), p.lds_fwd, s, ta);
  return true;
}

bool shallow_bf16w_train_fwd_launch(const uint8_t* frames, const void* w1p, const float* b1,
                                    const void* w2p, const float* b2, const void* w3p,
                                    const float* b3, float* feats, void* a1, void* a2, int N,
                                    int H, int W, int C, hipStream_t s) {
  if (!shallow_bf16w_train_form(N, H, W, C)) return false;
  if (sbt_mis(frames, 3) || sbt_mis(w1p, 15) || sbt_mis(w2p, 15) || sbt_mis(w3p, 15) ||
      sbt_mis(feats, 15) || sbt_mis(a1, 15) || sbt_mis(a2, 15))
    return false;
  SbtPlan p{};
  SbtwFwdArgs ta{};
  sbtw_plan(H, W, C, &p, &ta.w, nullptr);
  ta.feats = feats;
  ta.a1 = static_cast<bf16_t*>(a1);
  ta.a2 = static_cast<bf16_t*>(a2);
  ShallowBf16Args& a = ta.w.g;
  a.frames = frames;
  a.w1 = static_cast<const uint4*>(w1p);
  a.w2 = static_cast<const uint4*>(w2p);
  a.w3 = static_cast<const uint4*>(w3p);
  a.b1 = b1; a.b2 = b2; a.b3 = b3;
  a.out = nullptr;
  a.N = N;
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  auto go = [&](auto kernel) {
    sbt_lds(kernel, p.lds_fwd);
    hipLaunchKernelGGL(kernel, dim3(G), dim3(kSbThreads), p.lds_fwd, s, ta);
  };
  shallow_bf16_train_note(3, G, grid_max, N);
  if (C <= 8) go(sbtw_fwd_kernel<2>);
  else if (C <= 12) go(sbtw_fwd_kernel<3>);
  else go(sbtw_fwd_kernel<4>);
  return true;
}

bool shallow_bf16_bwd_data_launch(const float* dfeats, const float* feats, const void* a2,
                                  const void* a1, const void* wd3, const void* wd2, void* dy3m,
                                  void* da2, void* da1, int N, int H, int W, int C,
                                  hipStream_t s) {
  if (!shallow_bf16_train_back_form(N, H, W, C)) return false;
  const void* ptrs[9] = {dfeats, feats, a2, a1, wd3, wd2, dy3m, da2, da1};
  for (const void* q : ptrs)
    if (sbt_mis(q, 15)) return false;
  SbtPlan p{};
  sb_dims(H, W, C, &p.g);
  sbt_plan_back(&p, false);
  const ShallowBf16Args& g = p.g;
  SbtBwdArgs a{dfeats, feats, static_cast<const bf16_t*>(a2), static_cast<const bf16_t*>(a1),
               static_cast<const uint4*>(wd3), static_cast<const uint4*>(wd2),
               static_cast<bf16_t*>(dy3m), static_cast<bf16_t*>(da2), static_cast<bf16_t*>(da1),
               N, g.H1, g.W1, g.H2, g.W2, g.H3, g.W3, g.pt2, g.pl2, g.pt3, g.pl3};
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  sbt_lds(sbt_bwd_data_kernel, p.lds_bwd);
  shallow_bf16_train_note(1, G, grid_max, N);
  hipLaunchKernelGGL(sbt_bwd_data_kernel, dim3(G), dim3(kSbThreads), p.lds_bwd, s, a);
  return true;
}

int64_t shallow_bf16_wgrad_part_floats(int N) {
  const int64_t G = std::min(std::max(N, 1), shallow_bf16_grid_max());
  return G * (sbt_slot<1>() + sbt_slot<2>() + sbt_slot<3>());
}

bool shallow_bf16_wgrad_launch(const uint8_t* frames, const void* a1, const void* a2,
                               const void* dy3m, const void* da2, const void* da1, float* part,
                               float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                               float* db3, int N, int H, int W, int C, hipStream_t s) {
  if (!shallow_bf16_train_form(N, H, W, C)) return false;
  const void* ptrs[5] = {a1, a2, dy3m, da2, da1};
  for (const void* q : ptrs)
    if (sbt_mis(q, 15)) return false;
  if (sbt_mis(frames, 3) || sbt_mis(part, 3)) return false;
  SbtPlan p{};
  sbt_plan(H, W, C, &p);
  const ShallowBf16Args& g = p.g;
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  SbtWgArgs w1{frames, nullptr, static_cast<const bf16_t*>(da1), part, N, C,
               g.H, g.W, g.pt1, g.pl1, g.Hp0, g.Wp0, g.H1, g.W1, p.ppad[0]};
  SbtWgArgs w2{nullptr, static_cast<const bf16_t*>(a1), static_cast<const bf16_t*>(da2),
               part + static_cast<int64_t>(G) * sbt_slot<1>(), N, C,
               g.H1, g.W1, g.pt2, g.pl2, g.Hp1, g.Wp1, g.H2, g.W2, p.ppad[1]};
  SbtWgArgs w3{nullptr, static_cast<const bf16_t*>(a2), static_cast<const bf16_t*>(dy3m),
               part + static_cast<int64_t>(G) * (sbt_slot<1>() + sbt_slot<2>()), N, C,
               g.H2, g.W2, g.pt3, g.pl3, g.Hp2, g.Wp2, g.H3, g.W3, p.ppad[2]};
  sbt_lds(sbt_wgrad_kernel<1>, p.lds_wg[0]);
  sbt_lds(sbt_wgrad_kernel<2>, p.lds_wg[1]);
  sbt_lds(sbt_wgrad_kernel<3>, p.lds_wg[2]);
  shallow_bf16_train_note(2, G, grid_max, N);
  hipLaunchKernelGGL(sbt_wgrad_kernel<3>, dim3(G), dim3(kSbThreads), p.lds_wg[2], s, w3);
  hipLaunchKernelGGL(sbt_wgrad_kernel<2>, dim3(G), dim3(kSbThreads), p.lds_wg[1], s, w2);
  hipLaunchKernelGGL(sbt_wgrad_kernel<1>, dim3(G), dim3(kSbThreads), p.lds_wg[0], s, w1);
  SbtReduceArgs r{part, dw1, db1, dw2, db2, dw3, db3, G, C, 4};
  const int nel = 64 * C * 32 + 32 + sbt_k<2>() * 64 + 64 + sbt_k<3>() * 128 + 128;
  hipLaunchKernelGGL(sbt_reduce_kernel, dim3((nel + 255) / 256), dim3(256), 0, s, r);
  return true;
}

int64_t shallow_bf16w_wgrad_part_floats(int N, int C) {
  const int64_t G = std::min(std::max(N, 1), shallow_bf16_grid_max());
  return G * (sbt_slot1((C + 3) / 4 * 4) + sbt_slot<2>() + sbt_slot<3>());
}

bool shallow_bf16w_wgrad_launch(const uint8_t* frames, const void* a1, const void* a2,
                                const void* dy3m, const void* da2, const void* da1, float* part,
                                float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                float* db3, int N, int H, int W, int C, hipStream_t s) {
  if (!shallow_bf16w_train_form(N, H, W, C)) return false;
  const void* ptrs[5] = {a1, a2, dy3m, da2, da1};
  for (const void* q : ptrs)
    if (sbt_mis(q, 15)) return false;
  if (sbt_mis(frames, 3) || sbt_mis(part, 3)) return false;
  SbtPlan p{};
  SbtwWgArgs w1{};
  sbtw_plan(H, W, C, &p, nullptr, &w1);
  const ShallowBf16Args& g = p.g;
  const int grid_max = shallow_bf16_grid_max();
  const int G = std::min(N, grid_max);
  const int Cp = (C + 3) / 4 * 4;
  w1.g.frames = frames;
  w1.g.N = N;
  w1.dout = static_cast<const bf16_t*>(da1);
  w1.part = part;
  // layers 2 and 3: the launches of shallow_bf16_wgrad_launch
  SbtWgArgs w2{nullptr, static_cast<const bf16_t*>(a1), static_cast<const bf16_t*>(da2),
               part + static_cast<int64_t>(G) * sbt_slot1(Cp), N, C,
               g.H1, g.W1, g.pt2, g.pl2, g.Hp1, g.Wp1, g.H2, g.W2, p.ppad[1]};
  SbtWgArgs w3{nullptr, static_cast<const bf16_t*>(a2), static_cast<const bf16_t*>(dy3m),
               part + static_cast<int64_t>(G) * (sbt_slot1(Cp) + sbt_slot<2>()), N, C,
               g.H2, g.W2, g.pt3, g.pl3, g.Hp2, g.Wp2, g.H3, g.W3, p.ppad[2]};
  sbt_lds(sbt_wgrad_kernel<2>, p.lds_wg[1]);
  sbt_lds(sbt_wgrad_kernel<3>, p.lds_wg[2]);
  shallow_bf16_train_note(2, G, grid_max, N);
  hipLaunchKernelGGL(sbt_wgrad_kernel<3>, dim3(G), dim3(kSbThreads), p.lds_wg[2], s, w3);
  hipLaunchKernelGGL(sbt_wgrad_kernel<2>, dim3(G), dim3(kSbThreads), p.lds_wg[1], s, w2);
  auto go = [&](auto kernel) {
    sbt_lds(kernel, p.lds_wg[0]);
    hipLaunchKernelGGL(kernel, dim3(G), dim3(kSbThreads), p.lds_wg[0], s, w1);
  };
  shallow_bf16_train_note(4, G, grid_max, N);
  if (C <= 8) go(sbtw_wgrad1_kernel<2>);
  else if (C <= 12) go(sbtw_wgrad1_kernel<3>);
  else go(sbtw_wgrad1_kernel<4>);
  SbtReduceArgs r{part, dw1, db1, dw2, db2, dw3, db3, G, C, Cp};
  const int nel = 64 * C * 32 + 32 + sbt_k<2>() * 64 + 64 + sbt_k<3>() * 128 + 128;
  hipLaunchKernelGGL(sbt_reduce_kernel, dim3((nel + 255) / 256), dim3(256), 0, s, r);
  return true;
}

}  // namespace conv
}  // namespace sa
