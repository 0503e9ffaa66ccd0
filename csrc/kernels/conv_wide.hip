// Wide-frame (5..16 channel) stage 0 of the deep fp32 torso for gfx950: the
// uint8 -> fp32 x / 255 image with Cp = C rounded up to a multiple of 4
// channels, the fused conv3x3 (Cp -> 16) + bias + max-pool forward on
// v_mfma_f32_16x16x4_f32, and the scatter-form weight / bias gradient.  The
// launchers are reached through conv_f32.hip's frames_f32_launch,
// conv_pool_fwd_launch and wgrad_launch.  This file is compiled without
// packed fp32 arithmetic (csrc/build.py).
#include "conv_f32.h"
#include "knobs.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace sa {
namespace cf32 {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr size_t kLdsSoft = 80 * 1024;   // two workgroups per CU
constexpr size_t kLdsHard = 156 * 1024;  // one workgroup per CU

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
template <int VPL>
__device__ __forceinline__ void lds_get(const float* p, float (&v)[VPL]) {
  if constexpr (VPL == 4) {
    const f4 t = *reinterpret_cast<const f4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    const f2 t = *reinterpret_cast<const f2*>(p);
    v[0] = t[0]; v[1] = t[1];
  }
}
// x / d for 0 <= x < 2^20, 1 <= d <= 2^10 (exact: see conv_f32.hip fdiv)
__device__ __forceinline__ int fdiv(int x, float rd) {
  return static_cast<int>((static_cast<float>(x) + 0.5f) * rd);
}

template <typename Kern>
void allow_lds(Kern k, size_t bytes) {
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(bytes));
    if (e != hipSuccess) (void)hipGetLastError();  // the launch reports it
  }
}

// Wide frames: uint8 [P pixels][Cs], 5 <= Cs <= 16, -> fp32 [P][Cp] with
// Cp = Cs rounded up to a multiple of 4: the same table, zero pad channels.
// A tile is 256 pixels (<= 4 KB of frame bytes).  Pixels of Cs bytes are in
// general not dword multiples (nor is the tensor's start, for a row range of
// a larger buffer), so the tile's flat byte range is loaded as the aligned
// dwords that cover it (whole dwords where all four bytes lie inside the
// tensor, else its bytes one by one), the bytes are regrouped into channel
// quads out of LDS, and consecutive threads write consecutive 16-B quads.
constexpr int kWidePix = 256;
__global__ __launch_bounds__(256) void frames_f32_wide_kernel(const uint8_t* __restrict__ x,
                                                              f4* __restrict__ y, int64_t P,
                                                              int Cs, int QP) {
  __shared__ float lut[256];
  __shared__ uint32_t raw[kWidePix * 16 / 4 + 1];
  lut[threadIdx.x] = static_cast<float>(static_cast<double>(threadIdx.x) / 255.0);
  const int64_t ntiles = (P + kWidePix - 1) / kWidePix;
  const int64_t nbytes_all = P * Cs;
  const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(x) & 3);
  const uint32_t* xa = reinterpret_cast<const uint32_t*>(x - mis);  // aligned base
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(raw);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * kWidePix;
    const int np = static_cast<int>(P - p0 < kWidePix ? P - p0 : kWidePix);
    const int nbytes = np * Cs;
    const int64_t b0 = p0 * Cs + mis;  // the tile's first byte, from xa
    const int sh = static_cast<int>(b0 & 3);
    const int64_t d0 = b0 >> 2;
    const int nd = (sh + nbytes + 3) >> 2;
    __syncthreads();  // previous tile's LDS reads (and the table) done
    for (int d = threadIdx.x; d < nd; d += 256) {
      const int64_t tb = (d0 + d) * 4 - mis;  // tensor byte index of the dword's byte 0
      uint32_t v = 0;
      if (tb >= 0 && tb + 4 <= nbytes_all) {
        v = xa[d0 + d];
      } else {
        for (int b = 0; b < 4; ++b)
          if (tb + b >= 0 && tb + b < nbytes_all)
            v |= static_cast<uint32_t>(x[tb + b]) << (8 * b);
      }
      raw[d] = v;
    }
    __syncthreads();
    const int nq = np * QP;
    for (int e = threadIdx.x; e < nq; e += 256) {
      const int pix = e / QP, q = e - pix * QP;
      const uint8_t* s = rb + sh + pix * Cs + 4 * q;
      f4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * q + c < Cs) v[c] = lut[s[c]];
      y[p0 * QP + e] = v;
    }
  }
}


// ------------------------------------------- wide-frame stage 0: conv + pool
// Stage-0 head of the deep torso on wide frames: the fp32 x / 255 image
// [N,H,W,CP], CP in {8, 12, 16} (5..16 frame channels, zero pad channels)
// -> conv3x3/1 SAME (CP -> 16) + bias -> 3x3/2 SAME max-pool with the first
// maximal tap's code, one persistent kernel; the pre-pool map lives in LDS.
//
// GEMM: D^T = Wk^T X^T on v_mfma_f32_16x16x4_f32 as in conv_fwd_kernel: i =
// output channel (16 = one MFMA tile), j = 16 consecutive pixels, K = 9 taps
// x CP channels.  Lane group g = lane >> 4 holds the VPL = CP / 4 channels
// VPL g .. VPL g + VPL - 1 of its pixel, so one LDS read per (tap, pixel
// group) feeds VPL consecutive MFMAs: 18 / 27 / 36 k-steps per output.  The
// accumulation order per output is conv_fwd_kernel's at the same CINP, so the
// pooled map is bitwise conv_fwd + maxpool_fwd on the same image.
//
// LDS pixel layout: CP = 16 keeps the NHWC pixel (lane group g reads quad g
// with one ds_read_b128) at a pitch of 24 floats = 6 16-B units: the four lane
// groups of a pixel and the 16 pixels of a group then start at 16-B units
// 6 p + g, which fall on each of the 8 units of a 128-B bank row twice per
// 16-lane read phase pair - the pitch/4 = 2 mod 4 rule of the other forward
// images.  CP = 12 stores the pixel as four padded triples (channel c at
// float c + c / 3, slots 3, 7, 11, 15 unused) at the same pitch, so its lane
// groups also read one aligned b128 each and use three of the four values.
// CP = 8 keeps the NHWC pixel at pitch 8: the lane groups read one b64 each
// and the 64 lanes of a read cover 512 contiguous bytes.
//
// Work split: a tile is R pooled rows of one image, i.e. CR = 2 R + 1 conv
// rows (one conv row recomputed per band seam: 1.5x the MFMA work at R = 1,
// 1.25x at 2, 1.17x at 3) and 2 R + 3 image rows with the halo.  The tile's
// CR W conv pixels are cut into 16-pixel groups dealt round-robin to the four
// waves, four groups in flight per wave so the next tap's operand reads hide
// behind 4 VPL MFMAs; every wave holds the whole [9 CP, 16] weight slice's A
// fragments addressable in LDS.  Then all 256 threads pool the band.
//
// LDS (floats): weights 9 CP 16 (4.5 / 6.75 / 9 KB) + image (2R+3)(W+2) PP +
// pre-pool band (2R+1)(W+2) 20 (16 channels + 4 pad, -inf border columns).
// At W = 96: CP = 8 takes R = 2 in 66 KB, two workgroups per CU; CP = 12 /
// 16 would need 114 KB for that, which leaves one workgroup per CU anyway,
// so they take the tallest band under 156 KB that the staging registers hold
// (R = 3, 149 KB).
//
// Staging: the next tile's image rows are prefetched into registers
// (kWideMaxC 16-B chunks per thread) while the current tile computes, through
// a buffer descriptor over the whole image: rows and columns outside the
// image get an offset past the range, and the hardware range check returns
// the zero padding.
constexpr int kWideMaxC = 14;
__host__ __device__ constexpr int wide_pitch(int cp) { return cp == 8 ? 8 : 24; }

template <int CP>
__global__ __launch_bounds__(kThreads) void wide_conv_pool_kernel(
    ConvArgs a, int R, int tiles_per_img, int ntiles, int pbh, int pbw, int Hp, int Wp,
    float* __restrict__ pooled, uint8_t* __restrict__ parg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  static_assert(CP == 8 || CP == 12 || CP == 16, "CP");
  constexpr int KK = 9, COUT = 16;
  constexpr int PP = wide_pitch(CP);
  constexpr int VPL = CP / 4;            // channels per lane group
  constexpr int LV = CP == 8 ? 2 : 4;    // floats per operand read (b64 / b128)
  constexpr int QP = CP / 4;             // 16-B chunks per image pixel
  constexpr int YP = COUT + 4;
  constexpr int C4 = COUT / 4;
  const int H = a.Ho, W = a.Wo;
  const int Wl = W + 2;
  const int CR = 2 * R + 1;
  const int rows = CR + 2;
  const int total = rows * Wl * QP;
  float* w_s = smem;                     // [tap][g][co][LV]
  float* x_s = w_s + KK * 4 * COUT * LV; // [rows][Wl][PP]
  const int YW = W + 2;
  float* y_s = x_s + rows * Wl * PP;     // [CR][YW][YP]
  for (int e = threadIdx.x; e < CR * 2 * (YP / 4); e += kThreads) {
    const int q4 = e % (YP / 4), t = e / (YP / 4);
    const int col = (t & 1) ? W + 1 : 0;
    *reinterpret_cast<f4*>(y_s + ((t >> 1) * YW + col) * YP + 4 * q4) =
        f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  }
  for (int e = threadIdx.x; e < KK * 4 * COUT * LV; e += kThreads) {
    const int v = e % LV, o = (e / LV) % COUT, g_ = (e / (LV * COUT)) % 4, tap = e / (LV * COUT * 4);
    const int i = VPL * g_ + v;          // input channel of k slot g_, MFMA v
    float val = 0.f;
    if (v < VPL && i < a.wcin) val = a.w[(static_cast<int64_t>(tap) * a.wcin + i) * a.wcout + o];
    w_s[e] = val;
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  float bias[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bias[r] = a.bias[4 * g + r];
  const float* wl = w_s + (g * COUT + c16) * LV;
  const float rw = 1.f / static_cast<float>(W), rwp = 1.f / static_cast<float>(Wp);
  const float rwl = 1.f / static_cast<float>(Wl);
  const __amdgpu_buffer_rsrc_t srcr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(a.src), 0,
      static_cast<int>(static_cast<uint32_t>(static_cast<int64_t>(a.N) * H * W * CP * 4)),
      0x00020000);

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  f4 stg[kWideMaxC];
  auto prefetch = [&](int t) {
    const int n = t / tiles_per_img;
    const int j0 = 2 * (t - n * tiles_per_img) * R - pbh - 1;  // image row of LDS row 0
#pragma unroll
    for (int k = 0; k < kWideMaxC; ++k) {
      const int e = threadIdx.x + k * kThreads;
      const int pix = e / QP, ch = e - pix * QP;
      const int r = fdiv(pix, rwl), c = pix - r * Wl;
      const int j = j0 + r, i = c - 1;
      const bool ok = e < total && j >= 0 && j < H && i >= 0 && i < W;
      const uint32_t off =
          ok ? static_cast<uint32_t>(((n * H + j) * W + i) * QP + ch) * 16u : 0xFFFFFFF0u;
      stg[k] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(srcr, off, 0, 0));
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < kWideMaxC; ++k) {
      const int e = threadIdx.x + k * kThreads;
      if (e < total) {
        const int pix = e / QP, ch = e - pix * QP;
        float* d = x_s + pix * PP;
        if constexpr (CP == 12) {
          // channel c of the pixel at float c + c / 3 (padded triples)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 4 * ch + r;
            d[c + c / 3] = stg[k][r];
          }
        } else {
          *reinterpret_cast<f4*>(d + 4 * ch) = stg[k];
        }
      }
    }
  };
  prefetch(tile);
  const int P = CR * W;
  const int ngroups = (P + 15) >> 4;
  for (;;) {
    __syncthreads();  // previous tile: conv reads of x_s and pool reads of y_s done
    commit();
    __syncthreads();
    const int cur = tile;
    tile += gridDim.x;
    prefetch(tile < ntiles ? tile : cur);  // unconditional: see conv_fwd_kernel
    const int n = cur / tiles_per_img;
    const int pi0 = (cur - n * tiles_per_img) * R;
    const int cr0 = 2 * pi0 - pbh;  // image row of the tile's conv row 0
    auto mma = [&](auto NGc, int g0) {
      constexpr int NG = decltype(NGc)::value;
      f4 acc[NG];
      int xb[NG], q[NG];
      bool inimg[NG];
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        const int p = (g0 + 4 * gi) * 16 + c16;
        const int pp = p < P ? p : 0;
        const int oy = fdiv(pp, rw), ox = pp - oy * W;
        q[gi] = p < P ? (oy * YW + ox + 1) * YP : -1;
        inimg[gi] = cr0 + oy >= 0 && cr0 + oy < H;
        xb[gi] = (oy * Wl + ox) * PP + LV * g;
        acc[gi] = f4{0.f, 0.f, 0.f, 0.f};
      }
      float av[2][LV], bv[2][NG][LV];
      auto load_step = [&](int tap, int buf) {
        const int ky = tap / 3, kx = tap - (tap / 3) * 3;
        const int toff = (ky * Wl + kx) * PP;
        lds_get<LV>(wl + tap * 4 * COUT * LV, av[buf]);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) lds_get<LV>(x_s + xb[gi] + toff, bv[buf][gi]);
      };
      load_step(0, 0);
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) {
        const int cb = tap & 1;
        if (tap + 1 < KK) load_step(tap + 1, cb ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int v = 0; v < VPL; ++v)
#pragma unroll
          for (int gi = 0; gi < NG; ++gi) acc[gi] = mfma4(av[cb][v], bv[cb][gi][v], acc[gi]);
      }
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        if (q[gi] < 0) continue;
        f4 v = acc[gi];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = inimg[gi] ? v[r] + bias[r] : -INFINITY;
        *reinterpret_cast<f4*>(y_s + q[gi] + 4 * g) = v;
      }
    };
    int grp = wave;
    for (; grp + 12 < ngroups; grp += 16) mma(std::integral_constant<int, 4>{}, grp);
    for (; grp + 4 < ngroups; grp += 8) mma(std::integral_constant<int, 2>{}, grp);
    if (grp < ngroups) mma(std::integral_constant<int, 1>{}, grp);
    __syncthreads();
    // pool the band's conv rows (as conv_pool_fwd_kernel: out-of-image taps
    // read -inf, which never wins the strict first-max compare)
    const int Rv = min(R, Hp - pi0);
    const int nel = Rv * Wp * C4;
    for (int e = threadIdx.x; e < nel; e += kThreads) {
      const int c4 = e % C4;
      const int t = e / C4;
      const int pr = fdiv(t, rwp), pc = t - pr * Wp;
      const float* yb = y_s + ((2 * pr) * YW + 2 * pc - pbw + 1) * YP + 4 * c4;
      float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int code[4] = {0, 0, 0, 0};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const float* yr = yb + dy * YW * YP;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const f4 v = *reinterpret_cast<const f4*>(yr + dx * YP);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool gt = v[r] > best[r];
            best[r] = gt ? v[r] : best[r];
            code[r] = gt ? dy * 3 + dx : code[r];
          }
        }
      }
      const int64_t o = ((static_cast<int64_t>(n) * Hp + pi0 + pr) * Wp + pc) * COUT + 4 * c4;
      *reinterpret_cast<f4*>(pooled + o) = f4{best[0], best[1], best[2], best[3]};
      *reinterpret_cast<uint32_t*>(parg + o) =
          static_cast<uint32_t>(code[0]) | (static_cast<uint32_t>(code[1]) << 8) |
          (static_cast<uint32_t>(code[2]) << 16) | (static_cast<uint32_t>(code[3]) << 24);
    }
    if (tile >= ntiles) break;
  }
}

// The same scatter-form gradient for the wide-frame stage 0: x is the fp32
// image [N,H,W,CP], CP in {8, 12, 16}, staged in LDS as QP = CP / 4 quads per
// pixel at the row pitch of the 4-channel kernel; thread = (pooled-pixel
// slot, co) with 9 CP + 1 exact-FMA accumulators (145 at CP = 16, in a
// 512-register budget: one workgroup of four waves per SIMD set, two per CU).
// Partials in the slot layout [rows = tap * CP + ci, row 9 CP = bias][16 co],
// summed by the fixed-order slot reduction, which writes only the frame's real
// input channels (dw_cin).
template <int CP>
__global__ __launch_bounds__(kThreads) void wide_pool_wgrad_kernel(
    const f4* __restrict__ x, const float* __restrict__ dP, const uint8_t* __restrict__ arg,
    int H, int W, int Hp, int Wp, int pbh, int pbw, int tiles_per_img, int ntiles, int mt16,
    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) f4 xs[];  // [2*kPwRows+3][Wl][QP]
  constexpr int QP = CP / 4;
  constexpr int NR = 9 * CP + 1;
  const int co = threadIdx.x & 15, ps = threadIdx.x >> 4;
  const int Wl = pw_pitch(W);
  float acc[9][CP];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[t][c] = 0.f;
  float accb = 0.f;
  constexpr int kPer = (kPwRows * 64 + 15) / 16;  // pooled pixels per thread (Wp <= 64)
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / tiles_per_img;
    const int py0 = (tile - n * tiles_per_img) * kPwRows;
    const int rp = min(kPwRows, Hp - py0);
    const int ybase = 2 * py0 - pbh - 1;  // image row of LDS row 0
    const int rows = 2 * rp + 3;
    const int np = rp * Wp;
    float g[kPer];
    uint32_t code[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int p = ps + 16 * k;
      g[k] = 0.f;
      code[k] = 0;
      if (p < np) {
        const int64_t o = (static_cast<int64_t>(n) * Hp + py0) * Wp * 16 + p * 16 + co;
        g[k] = dP[o];
        code[k] = arg[o];
      }
    }
    __syncthreads();  // the previous tile's LDS reads are done
    for (int e = threadIdx.x; e < rows * Wl * QP; e += kThreads) {
      const int pix = e / QP, q = e - pix * QP;
      const int r = pix / Wl, c = pix - r * Wl;
      const int yy = ybase + r, xx = c - 1;
      f4 v = {0.f, 0.f, 0.f, 0.f};
      if (yy >= 0 && yy < H && xx >= 0 && xx < W)
        v = x[((static_cast<int64_t>(n) * H + yy) * W + xx) * QP + q];
      xs[e] = v;
    }
    __syncthreads();
    int pyl = 0, px = ps;  // (row, col) of pooled pixel p = ps + 16 k
    while (px >= Wp) {
      px -= Wp;
      ++pyl;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (ps + 16 * k < np) {
        const int dy = (code[k] * 11) >> 5;  // code / 3 for code <= 8
        const int dx = code[k] - 3 * dy;
        // LDS pixel of tap (0, 0): row 2 pyl + dy, col 2 px - pbw + dx (the
        // argmax never lies in the pool's padding; clamped for safety)
        const int base = min(max(0, (2 * pyl + dy) * Wl + 2 * px - pbw + dx),
                             (rows - 2) * Wl - 3);
        const float gv = g[k];
        accb += gv;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int q = 0; q < QP; ++q) {
              const f4 v = xs[(base + ky * Wl + kx) * QP + q];
#pragma unroll
              for (int c = 0; c < 4; ++c)
                acc[3 * ky + kx][4 * q + c] = fmaf(gv, v[c], acc[3 * ky + kx][4 * q + c]);
            }
      }
      px += 16;
      while (px >= Wp) {
        px -= Wp;
        ++pyl;
      }
    }
  }
  // the 16 pixel slots of each co in a fixed order, as pool_wgrad_kernel
  __syncthreads();
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][NR][16]
  const int wave = threadIdx.x >> 6;
  auto wsum = [&](float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
  };
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float v = wsum(acc[t][c]);
      if ((threadIdx.x & 63) < 16) red[(wave * NR + CP * t + c) * 16 + co] = v;
    }
  {
    const float v = wsum(accb);
    if ((threadIdx.x & 63) < 16) red[(wave * NR + 9 * CP) * 16 + co] = v;
  }
  __syncthreads();
  float* dst = part + static_cast<int64_t>(blockIdx.x) * (mt16 * 16);
  for (int e = threadIdx.x; e < NR * 16; e += kThreads)
    dst[e] = (red[e] + red[NR * 16 + e]) + (red[2 * NR * 16 + e] + red[3 * NR * 16 + e]);
}

template <int CP>
bool run_wide_conv_pool(const ConvArgs& a, int pbh, int pbw, float* pooled, uint8_t* arg,
                        hipStream_t s) {
  constexpr int PP = wide_pitch(CP);
  constexpr int LV = CP == 8 ? 2 : 4;
  const int W = a.Wo, Wl = W + 2;
  const int Hp = (a.Ho + 1) / 2, Wp = (a.Wo + 1) / 2;
  // one buffer descriptor over the image; 20-bit pixel counts in the stagers
  if (static_cast<int64_t>(a.N) * a.Ho * W * CP * 4 >= 0xFFFFFF00ll || W > 1024) return false;
  if ((reinterpret_cast<uintptr_t>(a.src) & 15) != 0) return false;
  auto bytes = [&](int R) {
    return static_cast<size_t>(4) *
           (9 * 4 * 16 * LV + (2 * R + 3) * Wl * PP + (2 * R + 1) * (W + 2) * 20);
  };
  const size_t budget = bytes(2) <= kLdsSoft ? kLdsSoft : kLdsHard;
  static const int rcap = sa::measure_knob("SA_F32_WIDE_R", 1 << 20);
  int R = 0;
  for (int r = 1; r <= std::min(Hp, rcap); ++r) {
    if (bytes(r) > budget || (2 * r + 3) * Wl * (CP / 4) > kWideMaxC * kThreads) break;
    R = r;
  }
  if (R == 0) return false;
  const int nt = (Hp + R - 1) / R;
  R = (Hp + nt - 1) / nt;
  const int ntiles = a.N * nt;
  const int per_cu = std::max<int>(1, std::min<size_t>(2, (160 * 1024) / (bytes(R) + 512)));
  const int G = wide_grid(std::max(1, std::min(ntiles, conv_cus() * per_cu)));
  auto kern = wide_conv_pool_kernel<CP>;
  allow_lds(kern, bytes(R));
  wide_note_launch("wide_conv_pool", G, ntiles, R, nt);
  hipLaunchKernelGGL(kern, dim3(G), dim3(kThreads), bytes(R), s, a, R, nt, ntiles, pbh, pbw,
                     Hp, Wp, pooled, arg);
  return true;
}

template <int CP>
bool run_wide_pool_wgrad(const WgradArgs& a, float* ws, hipStream_t s) {
  const PoolGeom& pg = a.pool;
  if (pg.Hp != (a.Ho + 1) / 2 || pg.Wp != (a.Wo + 1) / 2 || pg.Wp > 64 || a.Ho != a.H ||
      a.Wo != a.W || a.pt != 1 || a.pl != 1 || a.relu_in || pg.pbh < 0 || pg.pbh > 1 ||
      pg.pbw < 0 || pg.pbw > 1 || (reinterpret_cast<uintptr_t>(a.src) & 15) != 0)
    return false;
  constexpr int NR = 9 * CP + 1, MT16 = (9 * CP + 16) / 16 * 16;
  const int tpi = (pg.Hp + kPwRows - 1) / kPwRows;
  const int ntiles = a.N * tpi;
  const int G = wide_grid(std::min(ntiles, kWidePoolWgradSlots));
  wide_note_launch("wide_pool_wgrad", G, ntiles, kPwRows, tpi);
  const size_t lds = std::max<size_t>(sizeof(float) * CP * (2 * kPwRows + 3) * pw_pitch(a.W),
                                      sizeof(float) * 4 * NR * 16);
  if (lds > kLdsHard) return false;
  auto kern = wide_pool_wgrad_kernel<CP>;
  allow_lds(kern, lds);
  hipLaunchKernelGGL(kern, dim3(G), dim3(kThreads), lds, s, static_cast<const f4*>(a.src), a.dy,
                     pg.arg, a.H, a.W, pg.Hp, pg.Wp, pg.pbh, pg.pbw, tpi, ntiles, MT16, ws);
  wide_wgrad_reduce(ws, G, MT16, CP, a.dw_cin > 0 ? a.dw_cin : a.Cin, a.dw, a.db, s);
  return true;
}

}  // namespace

bool wide_conv_pool_launch(const ConvArgs& a, int pbh, int pbw, float* pooled, uint8_t* arg,
                           hipStream_t s) {
  if (a.Cout != 16 || a.wcout != 16 || a.bias == nullptr) return false;
  if (a.Cs == 8) return run_wide_conv_pool<8>(a, pbh, pbw, pooled, arg, s);
  if (a.Cs == 12) return run_wide_conv_pool<12>(a, pbh, pbw, pooled, arg, s);
  if (a.Cs == 16) return run_wide_conv_pool<16>(a, pbh, pbw, pooled, arg, s);
  return false;
}

bool wide_pool_wgrad_launch(const WgradArgs& a, float* ws, hipStream_t s) {
  if (a.Cout != 16 || a.pool.arg == nullptr) return false;
  if (a.Cin == 8) return run_wide_pool_wgrad<8>(a, ws, s);
  if (a.Cin == 12) return run_wide_pool_wgrad<12>(a, ws, s);
  if (a.Cin == 16) return run_wide_pool_wgrad<16>(a, ws, s);
  return false;
}

void frames_f32_wide_launch(const uint8_t* x, float* y, int64_t P, int Cs, hipStream_t s) {
  const int blocks = wide_grid(static_cast<int>(
      std::max<int64_t>(1, std::min<int64_t>((P + kWidePix - 1) / kWidePix, 8192))));
  wide_note_launch("frames_wide", blocks, 0, 0, 0);
  hipLaunchKernelGGL(frames_f32_wide_kernel, dim3(blocks), dim3(256), 0, s, x,
                     reinterpret_cast<f4*>(y), P, Cs, (Cs + 3) / 4);
}

}  // namespace cf32
}  // namespace sa
