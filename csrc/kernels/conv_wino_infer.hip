// The fp32 Winograd kernels only a no-grad board launch uses, their launchers and
// "form" functions.  The learner's kernels and the launch state: conv_wino.hip.
#include "conv_f32.h"
#include "knobs.h"
#include "wino_core.h"

namespace sa {
namespace cf32 {
namespace {

using namespace wino;  // the shared phase functions and device utilities (wino_core.h)

// `rows` rows of image n (raw, [H][W][C] in a buffer of N images) from image row
// y_first on into an LDS image [rows][Wl][C + 4], pixel x at column x + 1, zeros
// around it (a buffer load past the end returns zeros).  WLC > 0: Wl, a constant.
template <int C, int NTH, int WLC = 0>
__device__ __forceinline__ void stage_rows(float* img, const float* src, int N, int n, int H,
                                           int W, int y_first, int rows, int Wl, float rWl) {
  constexpr int PP = C + 4, C4 = C / 4, LC4 = C4 == 4 ? 2 : 3, KB = 4;
  const auto srcr = buf_rsrc(src, static_cast<int64_t>(N) * H * W * C);
  const int nx = rows * Wl * C4;
  for (int e0 = threadIdx.x; e0 < nx; e0 += KB * NTH) {
    f4 stg[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int e = e0 + k * NTH;
      const int ch = e & (C4 - 1), pix = e >> LC4;
      int L;
      if constexpr (WLC > 0) L = pix / WLC; else L = fdivi(pix, rWl);
      const int col = pix - L * Wl;
      const int y = y_first + L, xc = col - 1;
      const bool in = e < nx && y >= 0 && y < H && xc >= 0 && xc < W;
      stg[k] = bload(srcr, in ? static_cast<uint32_t>(((n * H + y) * W + xc) * C + 4 * ch) * 4u
                              : kOOB);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int e = e0 + k * NTH;
      if (e < nx) *reinterpret_cast<f4*>(img + (e >> LC4) * PP + 4 * (e & (C4 - 1))) = stg[k];
    }
  }
}

// U of an HWIO [3, 3, 16 NB, CO] weight tensor
template <int NB, int CO, int NTH>
__device__ __forceinline__ void wino_u_hwio(float* U_s, const float* __restrict__ w) {
  wino_u_to_lds<NB, CO, NTH>(U_s, 16 * NB * CO, [&](int ky, int kx, int ci, int co) {
    return w[((ky * 3 + kx) * 16 * NB + ci) * CO + co];
  });
}

// ------------------------------------------------- fused residual block
// One whole residual block of the deep torso for actor inference (small
// no-grad batches, where every conv launch sits at its fixed cost):
//   t = relu(conv1(relu(x)) + b1);  y = conv2(t) + b2 + x  [then relu]
// in ONE launch, t only in LDS.  A workgroup owns a band of R output rows of
// one image (all columns).  It stages the raw x rows y0 - 3 .. y0 + R + 2
// (zero outside the image; conv1 applies the ReLU when it reads a patch, the
// residual add reads the raw value), computes t for the tile rows that cover
// rows y0 - 2 .. y0 + R + 1 (the band plus conv2's one-tile-row halo above
// and below, conv1 recomputed there: (R + 4) / R of its work) into an LDS
// image whose out-of-image rows and columns stay zero (conv2's SAME padding
// pads t, not x), transforms w2 into the U buffer w1's transform occupied,
// and computes y from the t image.  Workgroups are independent; the only
// synchronisation is __syncthreads.
//
// Per output element the arithmetic is wino_conv_kernel's: both call the
// same weight / input / output transforms (wino_core.h), wino_mfma_block is
// that kernel's k-step order, and the epilogue order is the same (bias,
// residual, ReLU), so the result is bitwise that of the two launches
// (tests/test_res_block_f32_gpu.py).
struct ResBlockArgs {
  const float* x;   // [N, H, W, C]
  const float* w1;  // HWIO [3, 3, C, C]
  const float* b1;  // [C]
  const float* w2;
  const float* b2;
  float* y;         // [N, H, W, C]
  int N, H, W, TY, TX, nbands, last;
  float rTX, rWl;
};

// One 16-tile x 16-channel task (LDS image of pitch C + 4, U [16 xi][C/16][4 g][C][4])
template <int C, bool RELU>
__device__ __forceinline__ F4x4 res_tile(const float* xp, int rowstr, const float* up) {
  return wino_tile<C / 16, RELU, true>(xp, rowstr, C + 4, up, C * C, 4 * C * 4);
}

// LDS of one workgroup: U, the x rows and the t rows
template <int C, int R>
constexpr size_t res_block_bytes(int TX) {
  return sizeof(float) * (16 * C * C + static_cast<size_t>(2 * R + 10) * (2 * TX + 2) * (C + 4));
}

template <int C, int R, int NW>
__global__ __launch_bounds__(64 * NW) void wino_res_block_kernel(ResBlockArgs a) {
  constexpr int NTH = 64 * NW, PP = C + 4, NS = C / 16;
  constexpr int XR = R + 6, TR = R + 4;  // staged x rows / t rows
  static_assert(C == 16 || C == 32, "C");
  static_assert(R % 2 == 0 && R >= 2, "band of whole tile rows");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Wl = 2 * a.TX + 2, rowstr = Wl * PP;
  float* U_s = smem;                 // [16 xi][C/16][4 g][C][4]
  float* x_s = smem + 16 * C * C;    // [XR][Wl][PP]: image row y0 - 3 + L, column c - 1
  float* t_s = x_s + XR * rowstr;    // [TR][Wl][PP]: image row y0 - 2 + L, column c - 1

  const int n = blockIdx.x / a.nbands, band = blockIdx.x - n * a.nbands;
  const int y0 = band * R, ty0 = band * (R / 2);

  // ---- stage the raw x rows, zero the t image, transform w1.  Not stage_rows: behind
  // any inlined call this kernel compiles to other code (res16 at 36x64: +0.7 %)
  constexpr int C4 = C / 4, LC4 = C4 == 4 ? 2 : 3, KB = 4;
  const auto srcr = buf_rsrc(a.x, static_cast<int64_t>(a.N) * a.H * a.W * C);
  const int nx = XR * Wl * C4;
  for (int e0 = threadIdx.x; e0 < nx; e0 += KB * NTH) {
    f4 stg[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int e = e0 + k * NTH;
      const int ch = e & (C4 - 1), pix = e >> LC4;
      const int L = fdivi(pix, a.rWl), col = pix - L * Wl;
      const int y = y0 - 3 + L, xc = col - 1;
      const bool in = e < nx && y >= 0 && y < a.H && xc >= 0 && xc < a.W;
      stg[k] = bload(srcr, in ? static_cast<uint32_t>(((n * a.H + y) * a.W + xc) * C + 4 * ch) * 4u
                              : kOOB);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int e = e0 + k * NTH;
      if (e < nx) *reinterpret_cast<f4*>(x_s + (e >> LC4) * PP + 4 * (e & (C4 - 1))) = stg[k];
    }
  }
  for (int e = threadIdx.x; e < TR * rowstr / 4; e += NTH)
    reinterpret_cast<f4*>(t_s)[e] = f4{0.f, 0.f, 0.f, 0.f};
  auto u_transform = [&](const float* w) __attribute__((always_inline)) {
    wino_u_hwio<C / 16, C, NTH>(U_s, w);
  };  // a direct wino_u_hwio call compiles the C = 16 instances to other instructions
  u_transform(a.w1);
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c16 = lane & 15;

  // ---- conv1 over the t tile rows inside the image: local tile row tyl is
  // tile row ty0 - 1 + tyl, its patch at x rows 2 tyl .., its outputs at t
  // rows 2 tyl, 2 tyl + 1
  {
    const int lo = band == 0 ? 1 : 0;
    const int hi = min(R / 2 + 1, a.TY - ty0);
    const int nt = (hi - lo + 1) * a.TX, ng = (nt + 15) >> 4;
    for (int task = wave; task < ng * NS; task += NW) {
      const int sl = task / ng, grp = task - sl * ng;
      const int co0 = 16 * sl;
      int t = 16 * grp + c16;
      const bool valid = t < nt;
      if (!valid) t = 0;
      const int tr = fdivi(t, a.rTX), tx = t - tr * a.TX;
      const int tyl = lo + tr;
      const F4x4 Ys = res_tile<C, true>(x_s + (2 * tyl * Wl + 2 * tx) * PP + 4 * g, rowstr,
                                        U_s + (g * C + co0 + c16) * 4);
      const f4 (&Y)[4] = Ys.v;
      const int co = co0 + 4 * g;
      const f4 bv = *reinterpret_cast<const f4*>(a.b1 + co);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int oy = y0 - 2 + 2 * tyl + dy, ox = 2 * tx + dx;
          if (!valid || oy < 0 || oy >= a.H || ox >= a.W) continue;  // t stays zero there
          f4 v = Y[2 * dy + dx] + bv;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = relu0(v[k]);
          *reinterpret_cast<f4*>(t_s + ((2 * tyl + dy) * Wl + ox + 1) * PP + co) = v;
        }
    }
  }
  __syncthreads();  // t complete, every wave done with w1's U
  u_transform(a.w2);
  __syncthreads();

  // ---- conv2 over the band's tile rows: local tile row tyl is tile row
  // ty0 + tyl, its patch at t rows 2 tyl + 1 ..
  {
    const int nt = min(R / 2, a.TY - ty0) * a.TX, ng = (nt + 15) >> 4;
    for (int task = wave; task < ng * NS; task += NW) {
      const int sl = task / ng, grp = task - sl * ng;
      const int co0 = 16 * sl;
      int t = 16 * grp + c16;
      const bool valid = t < nt;
      if (!valid) t = 0;
      const int tyl = fdivi(t, a.rTX), tx = t - tyl * a.TX;
      const F4x4 Ys = res_tile<C, false>(t_s + ((2 * tyl + 1) * Wl + 2 * tx) * PP + 4 * g,
                                         rowstr, U_s + (g * C + co0 + c16) * 4);
      const f4 (&Y)[4] = Ys.v;
      const int co = co0 + 4 * g;
      const f4 bv = *reinterpret_cast<const f4*>(a.b2 + co);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int ly = 2 * tyl + dy, ox = 2 * tx + dx;
          const int oy = y0 + ly;
          if (!valid || oy >= a.H || ox >= a.W) continue;
          f4 v = Y[2 * dy + dx] + bv;
          v += *reinterpret_cast<const f4*>(x_s + ((ly + 3) * Wl + ox + 1) * PP + co);
          if (a.last) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = relu0(v[k]);
          }
          const int64_t o = ((static_cast<int64_t>(n) * a.H + oy) * a.W + ox) * C + co;
          *reinterpret_cast<f4*>(a.y + o) = v;
        }
    }
  }
}

template <int C, int R, int NW>
bool run_res_block(const ResBlockArgs& a, hipStream_t s) {
  const size_t bytes = res_block_bytes<C, R>(a.TX);
  if (bytes > 160 * 1024) return false;
  ResBlockArgs b = a;
  b.nbands = (a.H + R - 1) / R;
  auto kern = wino_res_block_kernel<C, R, NW>;
  allow_lds_w(kern, bytes);
  hipLaunchKernelGGL(kern, dim3(a.N * b.nbands), dim3(64 * NW), bytes, s, b);
  return true;
}

// ------------------------------------------------- fused last stage
// The deep torso's last stage for actor inference, one workgroup per image:
// both residual blocks of a 32-channel stage whose WHOLE map fits in LDS
// (9x12, 11x11, 9x16: the last maps of the three frame ladders),
//   t  = relu(conv1a(relu(x)) + b1a);   x' = conv2a(t) + b2a + x
//   t  = relu(conv1b(relu(x')) + b1b);  y  = conv2b(t) + b2b + x'  [then relu]
// with x, x' and t only in LDS.  No band, so no halo: conv1 is computed once
// per tile, each weight tensor is transformed once per image (into the one U
// buffer, between barriers), and the map never visits HBM between the four
// convs.  The x and t images are [2 TY + 2][2 TX + 2][C + 4] with image pixel
// (y, x) at (y + 1, x + 1); everything outside the image stays zero (conv2's
// SAME padding pads t, conv1b's pads x'): only cells inside the image are
// ever written, which also keeps the row / column an odd map's last tiles
// overhang at zero.  x' is written over x by the lane that read x there as
// its residual operand (raw, not ReLU'd: conv1 applies the ReLU when it loads
// a patch), so that write needs no barrier of its own.
//
// HEAD (the 18x24 -> 9x12 stage of the 72x96 frame): the stage head's conv and
// 3x3 / 2 max-pool run first in the same workgroup, as in
// wino_conv_pool_img_kernel: the staged input (75 KB), then the pre-pool map
// over it.  U, that region and an x image do not fit in 160 KB together, so a
// thread holds its (at most two) pooled float4s in registers across the
// barrier that ends the pool's reads, and the x and t images then take the
// region's place.  No argmax: inference keeps nothing for a backward.
//
// Per output element the arithmetic is that of the launches replaced: the
// same transforms, wino_mfma_block's k-step order, bias - residual - ReLU,
// strict > over row-major taps (tests/test_stage_fused_f32_gpu.py: bitwise).
struct StageArgs {
  const float* x;     // [N, H, W, C]; HEAD: the head's input [N, 18, 24, C]
  const float* wh;    // HEAD: the head's weights HWIO [3, 3, C, C] and bias
  const float* bh;
  const float* w[4];  // conv1a, conv2a, conv1b, conv2b: HWIO [3, 3, C, C]
  const float* b[4];  // [C]
  float* y;           // [N, H, W, C]
  int N, H, W, TY, TX, last;  // the residual map and its tile grid
  float rTX, rWl;
};

// One conv over a whole LDS image: the (16 tiles x 16 output channels) tasks
// of the TY x TX tile grid over the workgroup's NW waves; epi(ty, tx, co, Y)
// gets a lane's 2x2 outputs of 4 channels (only for tiles of the grid).  The banded
// kernels keep their loops: through this one res16 measured +1.2 %, head 0 +2.7 .. 4.1 %
template <int C, int NW, bool RELU, typename Epi>
__device__ __forceinline__ void stage_conv(const float* img, const float* U_s, int TY, int TX,
                                           float rTX, int Wl, Epi epi) {
  constexpr int PP = C + 4, NS = C / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int nt = TY * TX, ng = (nt + 15) >> 4;
  for (int task = wave; task < ng * NS; task += NW) {
    const int sl = task / ng, grp = task - sl * ng;
    const int co0 = 16 * sl;
    int t = 16 * grp + c16;
    const bool valid = t < nt;
    if (!valid) t = 0;
    const int ty = fdivi(t, rTX), tx = t - ty * TX;
    const F4x4 Ys = res_tile<C, RELU>(img + (2 * ty * Wl + 2 * tx) * PP + 4 * g, Wl * PP,
                                      U_s + (g * C + co0 + c16) * 4);
    if (valid) epi(ty, tx, co0 + 4 * g, Ys);
  }
}

template <int C, bool HEAD>
constexpr size_t stage_tail_bytes(int TY, int TX) {
  const size_t imgs = static_cast<size_t>(2) * (2 * TY + 2) * (2 * TX + 2) * (C + 4);
  const size_t head = HEAD ? PoolImgGeo<C, C, 18, 24>::XREG : 0;
  return sizeof(float) * (16 * C * C + (imgs > head ? imgs : head));
}

template <int C, bool HEAD = false>
__global__ __launch_bounds__(512, 1) void wino_stage_tail_kernel(StageArgs a) {
  constexpr int NW = 8, NTH = 64 * NW, PP = C + 4, C4 = C / 4;
  static_assert(C == 32, "C");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Wl = 2 * a.TX + 2, IH = 2 * a.TY + 2, rowstr = Wl * PP;
  float* U_s = smem;               // [16 xi][C/16][4 g][C][4]
  float* x_s = smem + 16 * C * C;  // [IH][Wl][PP]: x, then x'
  float* t_s = x_s + IH * rowstr;  // [IH][Wl][PP]
  const int n = blockIdx.x;

  auto u_transform = [&](const float* w) __attribute__((always_inline)) {
    wino_u_hwio<C / 16, C, NTH>(U_s, w);
  };  // direct wino_u_hwio calls compile both instances to other instructions
  auto zero_t = [&]() __attribute__((always_inline)) {
    for (int e = threadIdx.x; e < IH * rowstr / 4; e += NTH)
      reinterpret_cast<f4*>(t_s)[e] = f4{0.f, 0.f, 0.f, 0.f};
  };

  if constexpr (HEAD) {
    // ---- the stage head: conv + bias over the staged 18x24 input, the
    // pre-pool map over it, the pooled map into registers
    using P = PoolImgGeo<C, C, 18, 24>;
    constexpr int HH = 18, HW = 24, HWl = P::Wl, hrow = HWl * PP, IPP = P::IPP;
    constexpr int Hp = HH / 2, Wp = HW / 2, CQ = C / 4;
    static_assert(P::NW == NW && P::NTASK <= 2 * NW && Hp * Wp * CQ <= 2 * NTH, "head");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    float* img = x_s;  // [HH][HW][IPP], over the staged rows
    u_transform(a.wh);
    stage_rows<C, NTH>(x_s, a.x, a.N, n, HH, HW, -1, P::ROWS, HWl, 1.f / HWl);
    __syncthreads();
    f4 Yt[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int task = wave + NW * i;
      const int grp = task % P::NG, sl = task / P::NG;
      const int t0 = 16 * grp + c16;
      const int t = t0 < P::NTI ? t0 : 0;
      const int ty = t / P::TX, tx = t - ty * P::TX;
#pragma unroll
      for (int q = 0; q < 4; ++q) Yt[i][q] = f4{0.f, 0.f, 0.f, 0.f};
      if (task < P::NTASK) {
        const F4x4 Ys = wino_tile<C / 16, false, false>(
            x_s + (2 * ty * HWl + 2 * tx) * PP + 4 * g, hrow, PP,
            U_s + (g * C + 16 * sl + c16) * 4, C * C, 4 * C * 4);
        const f4 bv = *reinterpret_cast<const f4*>(a.bh + 16 * sl + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) Yt[i][q] = Ys.v[q] + bv;
      }
    }
    __syncthreads();  // every wave's patch reads are done: the region becomes the image
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int task = wave + NW * i;
      const int grp = task % P::NG, sl = task / P::NG;
      const int t = 16 * grp + c16;
      if (task < P::NTASK && t < P::NTI) {
        const int ty = t / P::TX, tx = t - ty * P::TX;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx)
            *reinterpret_cast<f4*>(img + ((2 * ty + dy) * HW + 2 * tx + dx) * IPP + sl * 16 +
                                   4 * g) = Yt[i][2 * dy + dx];
      }
    }
    __syncthreads();
    constexpr float kNegInf = -__builtin_inff();
    constexpr PoolLaneMap<CQ, IPP> kMap{};
    const int lmap = kMap.pj[lane] * CQ + kMap.pq[lane];
    f4 pooled[2];
    int pcell[2];  // the item's float offset in the x image, -1: none
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = (threadIdx.x & ~63) + k * NTH + lmap;
      pooled[k] = f4{kNegInf, kNegInf, kNegInf, kNegInf};
      pcell[k] = -1;
      if (e < Hp * Wp * CQ) {
        const int pr = e / (Wp * CQ), rem = e - pr * (Wp * CQ);
        const int pc = rem / CQ, pq = rem - pc * CQ;
        int code[4] = {0, 0, 0, 0};
        pool_window_img<HH, HW, IPP>(img, pr, pc, pq, pooled[k], code);
        pcell[k] = ((pr + 1) * Wl + pc + 1) * PP + 4 * pq;
      }
    }
    __syncthreads();  // the pool's reads are done: the region becomes the x and t images
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (pcell[k] >= 0) *reinterpret_cast<f4*>(x_s + pcell[k]) = pooled[k];
    for (int e = threadIdx.x; e < IH * Wl * C4; e += NTH) {  // x's zero border
      const int pix = e / C4, r = fdivi(pix, a.rWl), c = pix - r * Wl;
      if (r < 1 || r > a.H || c < 1 || c > a.W)
        *reinterpret_cast<f4*>(x_s + pix * PP + 4 * (e % C4)) = f4{0.f, 0.f, 0.f, 0.f};
    }
    zero_t();
  } else {
    stage_rows<C, NTH>(x_s, a.x, a.N, n, a.H, a.W, -1, IH, Wl, a.rWl);
    zero_t();
  }
  u_transform(a.w[0]);
  __syncthreads();

#pragma unroll 1
  for (int blk = 0; blk < 2; ++blk) {
    const float* w1 = blk ? a.w[2] : a.w[0];
    const float* w2 = blk ? a.w[3] : a.w[1];
    const float* b1 = blk ? a.b[2] : a.b[0];
    const float* b2 = blk ? a.b[3] : a.b[1];
    if (blk) {
      __syncthreads();  // x' complete, every wave done with t and conv2a's U
      u_transform(w1);
      __syncthreads();
    }
    // ---- conv1: t = relu(conv(relu(x)) + b1) inside the image
    stage_conv<C, NW, true>(x_s, U_s, a.TY, a.TX, a.rTX, Wl,
                            [&](int ty, int tx, int co, const F4x4& Ys) {
      const f4 bv = *reinterpret_cast<const f4*>(b1 + co);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int oy = 2 * ty + dy, ox = 2 * tx + dx;
          if (oy >= a.H || ox >= a.W) continue;  // t stays zero there
          f4 v = Ys.v[2 * dy + dx] + bv;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = relu0(v[k]);
          *reinterpret_cast<f4*>(t_s + ((oy + 1) * Wl + ox + 1) * PP + co) = v;
        }
    });
    __syncthreads();  // t complete, every wave done with w1's U
    u_transform(w2);
    __syncthreads();
    // ---- conv2: conv(t) + b2 + x, over x in LDS (first block) or to HBM
    stage_conv<C, NW, false>(t_s, U_s, a.TY, a.TX, a.rTX, Wl,
                             [&](int ty, int tx, int co, const F4x4& Ys) {
      const f4 bv = *reinterpret_cast<const f4*>(b2 + co);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int oy = 2 * ty + dy, ox = 2 * tx + dx;
          if (oy >= a.H || ox >= a.W) continue;  // x' stays zero there
          f4* xc = reinterpret_cast<f4*>(x_s + ((oy + 1) * Wl + ox + 1) * PP + co);
          f4 v = Ys.v[2 * dy + dx] + bv;
          v += *xc;
          if (blk == 0) {
            *xc = v;
            continue;
          }
          if (a.last) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = relu0(v[k]);
          }
          const int64_t o = ((static_cast<int64_t>(n) * a.H + oy) * a.W + ox) * C + co;
          *reinterpret_cast<f4*>(a.y + o) = v;
        }
    });
  }
}

template <bool HEAD>
bool run_stage_tail(const StageArgs& a, hipStream_t s) {
  const size_t bytes = stage_tail_bytes<32, HEAD>(a.TY, a.TX);
  if (bytes > 160 * 1024) return false;
  auto kern = wino_stage_tail_kernel<32, HEAD>;
  allow_lds_w(kern, bytes);
  hipLaunchKernelGGL(kern, dim3(a.N), dim3(512), bytes, s, a);
  return true;
}

// ------------------------------------------------- inference stage heads
// The stage-0 and stage-1 heads of the deep torso for actor inference:
//   pooled = maxpool3x3/2 SAME (conv3x3/1 SAME (x) + b)
// in ONE launch that writes only the pooled map: no argmax, no side buffers,
// no fix-up launch, and for stage 0 no fp32 x / 255 image (the uint8 rows are
// staged as dwords and expanded through the 256-entry correctly rounded
// x / 255 table of frames_f32_tile_kernel, so the staged values are bitwise
// that image's; channels past Cs and weight rows past wcin are zero).
//
// A workgroup owns a band of BP pooled rows p0 .. p0 + BP - 1 of one image
// (grid N x bands).  Pooled row p reads pixel rows 2p .. 2p + 2 (pad-before 0
// for even H), so the band computes tile rows p0 .. p0 + BP of the 2x2 tile
// grid the other Winograd kernels use: its own BP and one more for the single
// pixel row below its last pair, recomputed as wino_res_block_kernel
// recomputes its halo ((BP + 1) / BP of the conv's work).  Tile rows at or
// past H / 2 are not computed and the pool skips their taps, as it skips
// column W (padding loses).  It stages input pixel rows 2 p0 - 1 ..
// 2 p0 + 2 BP + 2 (zeros outside the image), writes Y + b of its tile rows
// into a pre-pool LDS image and pools from it.  Workgroups are independent:
// the only synchronisation is __syncthreads, every loop has a fixed bound.
//
// Per pre-pool element the arithmetic is wino_conv_pool_kernel's: the same
// weight / input / output transforms (wino_core.h), for CIN == 4 its channel
// planes (odd plane stride) and one scalar-transformed channel per lane
// group, for CIN == 16 wino_conv_kernel's [pixel][CIN + 4] rows through
// wino_tile; max is exact, so the pooled map is bitwise that of
// frames_f32 + wino_conv_pool_fwd (tests/test_head_infer_f32_gpu.py).  The
// pool phase takes the conflict-free PoolLaneMap of pitches 20 and 36.
//
// Instances (8 pooled rows never fit: the pre-pool image dominates), LDS bytes
// = U + staged rows + pre-pool image (+ the table), one workgroup per CU each:
//   stage 0   W  96  BP 6  8 waves  4096 +  25104 + 107520 + 1024 = 137744
//             W  84  BP 6  8 waves  4096 +  22032 +  94080 + 1024 = 121232
//             W 128  BP 4  8 waves  4096 +  24976 + 102400 + 1024 = 132496
//   stage 1   W  48  BP 3 12 waves 32768 +  40000 +  55296        = 128064
//             W  42  BP 3 12 waves 32768 +  35200 +  48384        = 116352
//             W  64  BP 3  8 waves 32768 +  52800 +  73728        = 159296
// 76 frames launch 456 - 684 workgroups, two to three rounds of one per CU.
// Registers and timings: profiles/experiments.md, "One-launch inference stage heads".
struct HeadArgs {
  const void* x;      // uint8 [N, H, W, Cs] (CIN 4) or float [N, H, W, 16]
  const float* w;     // HWIO [3, 3, wcin, COUT]
  const float* bias;  // [COUT]
  float* pooled;      // [N, H/2, W/2, COUT]
  int N, H, Cs, wcin, nbands;
};

template <int CIN, int COUT, int W, int BP>
struct HeadGeo {
  static constexpr int TX = W / 2, WP = W / 2, CQ = COUT / 4, Wl = W + 2;
  static constexpr int ROWS = 2 * BP + 4;             // staged pixel rows
  static constexpr int IROWS = 2 * BP + 2;            // pre-pool rows (BP + 1 tile rows)
  static constexpr int PP = CIN == 4 ? 4 : CIN + 4;   // staged pixel pitch (floats)
  static constexpr int IPP = COUT + 4;                // pre-pool image pixel pitch
  static constexpr int PS = (ROWS * Wl) | 1;          // CIN 4: channel-plane stride
  static constexpr int XS = ((CIN == 4 ? 4 * PS : ROWS * Wl * PP) + 3) & ~3;
  static constexpr int IMG = IROWS * W * IPP;
  static constexpr int LUT = CIN == 4 ? 256 : 0;
  static constexpr size_t bytes = sizeof(float) * (16 * CIN * COUT + XS + IMG + LUT);
};

template <int CIN, int COUT, int W, int BP, int NW>
__global__ __launch_bounds__(64 * NW) void wino_head_infer_kernel(HeadArgs a) {
  using P = HeadGeo<CIN, COUT, W, BP>;
  constexpr int NTH = 64 * NW, TX = P::TX, WP = P::WP, CQ = P::CQ, Wl = P::Wl;
  constexpr int ROWS = P::ROWS, PP = P::PP, IPP = P::IPP, PS = P::PS, NS = COUT / 16;
  static_assert((CIN == 4 && COUT == 16) || (CIN == 16 && COUT == 32), "stage 0 or 1");
  static_assert(W % 2 == 0 && NTH >= 256 && P::bytes <= 160 * 1024, "shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // U: CIN 16 [16 xi][4 g][COUT][4 v] (f4 A fragments), CIN 4 [16 xi][4 ci][COUT]
  float* U_s = smem;
  float* x_s = smem + 16 * CIN * COUT;  // CIN 4: planes [4][ROWS][Wl]; 16: [ROWS][Wl][PP]
  float* img = x_s + P::XS;             // [IROWS][W][IPP]: pixel row 2 p0 + L

  const int n = blockIdx.x / a.nbands, band = blockIdx.x - n * a.nbands;
  const int p0 = band * BP;
  const int H = a.H, Hp = H / 2;  // Hp: pooled rows = tile rows

  if constexpr (CIN == 16) {
    wino_u_hwio<1, COUT, NTH>(U_s, a.w);
    stage_rows<CIN, NTH, Wl>(x_s, static_cast<const float*>(a.x), a.N, n, H, W, 2 * p0 - 1, ROWS,
                             Wl, 0.f);
  } else {
    for (int e = threadIdx.x; e < CIN * COUT; e += NTH) {
      const int co = e % COUT, ci = e / COUT;
      float gk[3][3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
          gk[ky][kx] = ci < a.wcin ? a.w[((ky * 3 + kx) * a.wcin + ci) * COUT + co] : 0.f;
      float u[16];
      wino_weight_transform(gk, u);
#pragma unroll
      for (int xi = 0; xi < 16; ++xi) U_s[(xi * 4 + ci) * COUT + co] = u[xi];
    }
    // the x / 255 table (the correctly rounded quotients, as
    // frames_f32_tile_kernel), zero planes (padding, channels past Cs), then
    // the band's uint8 rows as dwords: byte i of a row is channel i % Cs of
    // pixel i / Cs; a row outside the image reads zeros (lut[0] = 0)
    float* lut = img + P::IMG;
    if (threadIdx.x < 256)
      lut[threadIdx.x] = static_cast<float>(static_cast<double>(threadIdx.x) / 255.0);
    for (int e = threadIdx.x; e < P::XS; e += NTH) x_s[e] = 0.f;
    __syncthreads();
    const int Cs = a.Cs, RD = W * Cs / 4, nd = ROWS * RD;
    const auto srcr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(a.x), 0,
        static_cast<int>(static_cast<uint32_t>(static_cast<int64_t>(a.N) * H * W * Cs)),
        0x00020000);
    constexpr int KB = 4;
    for (int e0 = threadIdx.x; e0 < nd; e0 += KB * NTH) {
      uint32_t stg[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const int e = e0 + k * NTH;
        const int L = e / RD, d = e - L * RD;
        const int y = 2 * p0 - 1 + L;
        const bool in = e < nd && y >= 0 && y < H;
        stg[k] = __builtin_amdgcn_raw_buffer_load_b32(
            srcr, in ? static_cast<uint32_t>((n * H + y) * RD + d) * 4u : kOOB, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const int e = e0 + k * NTH;
        if (e >= nd) continue;
        const int L = e / RD, d = e - L * RD;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = 4 * d + q;
          const int pix = Cs == 4 ? d : (Cs == 3 ? i / 3 : (Cs == 2 ? i >> 1 : i));
          const int ch = i - pix * Cs;
          x_s[ch * PS + L * Wl + pix + 1] = lut[(stg[k] >> (8 * q)) & 255u];
        }
      }
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c16 = lane & 15;

  // ---- conv + bias over the band's tile rows inside the image: local tile
  // row tr is tile row p0 + tr, its patch at staged rows 2 tr .., its outputs
  // at image rows 2 tr, 2 tr + 1
  {
    const int ntr = min(BP + 1, Hp - p0);
    const int nt = ntr * TX, ng = (nt + 15) >> 4;
    for (int task = wave; task < ng * NS; task += NW) {
      const int sl = task / ng, grp = task - sl * ng;
      const int co0 = 16 * sl;
      int t = 16 * grp + c16;
      const bool valid = t < nt;
      if (!valid) t = 0;
      const int tr = t / TX, tx = t - tr * TX;
      F4x4 Ys;
      if constexpr (CIN == 16) {
        Ys = wino_tile<1, false, false>(x_s + (2 * tr * Wl + 2 * tx) * PP + 4 * g, Wl * PP, PP,
                                        U_s + (g * COUT + co0 + c16) * 4, 16 * COUT, 0);
      } else {
        // channel g of the tile's 4x4 patch, one MFMA per xi (k = the 4 lane
        // groups' channels), as wino_conv_pool_kernel
        const float* xp = x_s + g * PS + 2 * tr * Wl + 2 * tx;
        const float* up = U_s + g * COUT + co0 + c16;
        Tile16<float> d;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
          for (int dx = 0; dx < 4; ++dx) d.v[4 * dy + dx] = xp[dy * Wl + dx];
        const Tile16<float> Vs = wino_input_transform(d);
        f4 acc[16];
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) acc[xi] = f4{0.f, 0.f, 0.f, 0.f};
        float ua[16];
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) ua[xi] = up[xi * 4 * COUT];
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) acc[xi] = mfma4(ua[xi], Vs.v[xi], acc[xi]);
        Ys = wino_output_transform(acc);
      }
      const f4 bv = *reinterpret_cast<const f4*>(a.bias + co0 + 4 * g);
      if (valid) {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx)
            *reinterpret_cast<f4*>(img + ((2 * tr + dy) * W + 2 * tx + dx) * IPP + co0 + 4 * g) =
                Ys.v[2 * dy + dx] + bv;
      }
    }
  }
  __syncthreads();

  // ---- pool: the band's windows (pad-before 0: the tap row H / column W is
  // padding and skipped), row-major taps, strict >; lanes permuted inside
  // each 64-element chunk by the conflict-free pool lane map.  Its own scan: one
  // shared with pool_window_img measured +0.6 / +2.1 / +0.1 % at the stage-0 heads.
  {
    constexpr float kNegInf = -__builtin_inff();
    constexpr PoolLaneMap<CQ, IPP> kMap{};
    const int lmap = kMap.pj[lane] * CQ + kMap.pq[lane];
    const int ne = min(BP, Hp - p0) * (WP * CQ);
    for (int e0 = threadIdx.x & ~63; e0 < ne; e0 += NTH) {
      const int e = e0 + lmap;
      if (e >= ne) continue;
      const int pr = e / (WP * CQ), rem = e - pr * (WP * CQ);
      const int pc = rem / CQ, pq = rem - pc * CQ;
      f4 best = {kNegInf, kNegInf, kNegInf, kNegInf};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int yl = 2 * pr + dy, x = 2 * pc + dx;
          if (2 * p0 + yl < H && x < W) {
            const f4 v = *reinterpret_cast<const f4*>(img + (yl * W + x) * IPP + 4 * pq);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (v[q] > best[q]) best[q] = v[q];
          }
        }
      const int64_t o = ((static_cast<int64_t>(n) * Hp + p0 + pr) * WP + pc) * COUT + 4 * pq;
      *reinterpret_cast<f4*>(a.pooled + o) = best;
    }
  }
}

template <int CIN, int COUT, int W, int BP, int NW>
bool run_head_infer(const HeadArgs& a0, hipStream_t s) {
  using P = HeadGeo<CIN, COUT, W, BP>;
  if (t_wino_probe) return true;
  HeadArgs a = a0;
  a.nbands = (a.H / 2 + BP - 1) / BP;
  auto kern = wino_head_infer_kernel<CIN, COUT, W, BP, NW>;
  allow_lds_w(kern, P::bytes);
  hipLaunchKernelGGL(kern, dim3(a.N * a.nbands), dim3(64 * NW), P::bytes, s, a);
  return true;
}

// N maps of H x W and their 2x2 tile grid into ResBlockArgs / StageArgs
template <typename Args>
void fill_tile_grid(Args& a, int N, int H, int W) {
  a.N = N; a.H = H; a.W = W;
  a.TY = (H + 1) / 2; a.TX = (W + 1) / 2;
  a.rTX = 1.f / static_cast<float>(a.TX);
  a.rWl = 1.f / static_cast<float>(2 * a.TX + 2);
}

// The 3x3 / 1 SAME conv x [N, H, W, Cin] -> out [N, H, W, Cout] of a replaced launch
ConvArgs same_conv_args(const void* x, const float* w, const float* b, float* out, int N, int H,
                        int W, int Cin, int Cout) {
  ConvArgs c{};
  c.src = x; c.w = w; c.bias = b; c.out = out;
  c.N = N; c.Hs = H; c.Ws = W; c.Cs = Cin;
  c.Ho = H; c.Wo = W; c.Cout = Cout;
  c.pt = 1; c.pl = 1; c.D = 1;
  c.wcin = Cin; c.wcout = Cout;
  return c;
}

// Whether both convs of a residual block at this shape run the Winograd forward
// (the direct kernel they would fall to sums in another order); launches nothing
bool res_convs_take_wino(const float* x, const float* w1, const float* b1, const float* w2,
                         const float* b2, float* y, int N, int H, int W, int C, bool last,
                         hipStream_t s) {
  ConvArgs c = same_conv_args(x, w1, b1, y, N, H, W, C, C);
  c.relu_in = 1; c.relu_out = 1;
  const WinoProbe probe;
  if (!wino_conv_launch(c, false, s)) return false;
  c.w = w2; c.bias = b2; c.add = x;
  c.relu_in = 0; c.relu_out = last ? 1 : 0;
  return wino_conv_launch(c, false, s);
}

}  // namespace

// Band heights (output rows per workgroup) of the fused residual block: per
// channel count the taller instance where its LDS fits the map's width, else
// the shorter one.  C = 16: 12 rows (36x48: 3 bands of 152 KB, 42x42: 4
// bands), 8 rows (36x64: 5 bands); C = 32, where U alone is 64 KB: 6 rows
// (18x24 and 21x21: 3 / 4 bands, 9x12 and 11x11: 2), 4 rows (18x32: 5 bands,
// 9x16: 3).  76-150 images then launch 150-750 workgroups of one per CU.
int wino_res_block_band(int C, int W) {
  const int TX = (W + 1) / 2;
  if (C == 16) {
    if (res_block_bytes<16, 12>(TX) <= 160 * 1024) return 12;
    if (res_block_bytes<16, 8>(TX) <= 160 * 1024) return 8;
  } else if (C == 32) {
    if (res_block_bytes<32, 6>(TX) <= 160 * 1024) return 6;
    if (res_block_bytes<32, 4>(TX) <= 160 * 1024) return 4;
  }
  return 0;
}

bool wino_res_block_launch(const float* x, const float* w1, const float* b1, const float* w2,
                           const float* b2, float* y, int N, int H, int W, int C, bool last,
                           hipStream_t s) {
  if (N < 1 || N > kResBlockMaxFrames || !wino_enabled()) return false;
  const int R = wino_res_block_band(C, W);
  if (R == 0) return false;
  // the two launches this replaces must both run the Winograd forward (the
  // direct kernel they would fall to sums in another order)
  if (!res_convs_take_wino(x, w1, b1, w2, b2, y, N, H, W, C, last, s)) return false;
  ResBlockArgs a{};
  a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.y = y;
  fill_tile_grid(a, N, H, W);
  a.last = last ? 1 : 0;
  if (C == 16) {
    if (R == 12) return run_res_block<16, 12, 12>(a, s);
    return run_res_block<16, 8, 12>(a, s);
  }
  if (R == 6) return run_res_block<32, 6, 8>(a, s);
  return run_res_block<32, 4, 8>(a, s);
}

namespace {

// the checks both stage launchers share; fills the residual map's geometry
bool stage_tail_args(StageArgs& a, const float* const* w, const float* const* b,
                     float* y, int N, int H, int W, int C, bool last, hipStream_t s) {
  if (N < 1 || N > kResBlockMaxFrames || C != 32 || H < 1 || W < 1 || !wino_enabled())
    return false;
  fill_tile_grid(a, N, H, W);
  if (a.TY > 1024 || a.TX > 1024 || stage_tail_bytes<32, false>(a.TY, a.TX) > 160 * 1024)
    return false;
  // each of the four launches this replaces must run the Winograd forward;
  // the first block never applies the torso's final ReLU
  if (!res_convs_take_wino(y, w[0], b[0], w[1], b[1], y, N, H, W, C, false, s) ||
      !res_convs_take_wino(y, w[2], b[2], w[3], b[3], y, N, H, W, C, last, s))
    return false;
  for (int i = 0; i < 4; ++i) {
    a.w[i] = w[i];
    a.b[i] = b[i];
  }
  a.y = y;
  a.last = last ? 1 : 0;
  return true;
}

// Whether the stage head here is the whole-image Winograd conv + pool; no launch
bool stage_head_takes_wino(const float* x, const float* wh, const float* bh, float* y, int N,
                           int H, int W, int C, hipStream_t s) {
  if (H != 18 || W != 24 || C != 32 || N < 1 || N > kResBlockMaxFrames) return false;
  const WinoProbe probe;
  return wino_conv_pool_launch(x, wh, bh, y, nullptr, nullptr, 0, N, H, W, C, C, -1, s);
}

}  // namespace

bool wino_stage_tail_launch(const float* x, const float* const* w,
                            const float* const* b, float* y, int N, int H, int W, int C,
                            bool last, hipStream_t s) {
  StageArgs a{};
  if (!stage_tail_args(a, w, b, y, N, H, W, C, last, s)) return false;
  a.x = x;
  return run_stage_tail<false>(a, s);
}

bool wino_stage_launch(const float* x, const float* wh, const float* bh,
                       const float* const* w, const float* const* b, float* y, int N,
                       int H, int W, int C, bool last, hipStream_t s) {
  StageArgs a{};
  if (!stage_head_takes_wino(x, wh, bh, y, N, H, W, C, s) ||
      !stage_tail_args(a, w, b, y, N, H / 2, W / 2, C, last, s))
    return false;
  a.x = x; a.wh = wh; a.bh = bh;
  return run_stage_tail<true>(a, s);
}

int wino_stage_form(int N, int H, int W, int C) {
  static const float dummy[4] = {};
  float* y = const_cast<float*>(dummy);  // geometry checks only: never read or written
  const float* const w[4] = {dummy, dummy, dummy, dummy};
  StageArgs a{};
  if (stage_head_takes_wino(dummy, dummy, dummy, y, N, H, W, C, nullptr) &&
      stage_tail_args(a, w, w, y, N, H / 2, W / 2, C, true, nullptr) &&
      stage_tail_bytes<32, true>(a.TY, a.TX) <= 160 * 1024)
    return 2;
  return stage_tail_args(a, w, w, y, N, (H + 1) / 2, (W + 1) / 2, C, true, nullptr) ? 1 : 0;
}

// Pooled rows per workgroup of the inference stage heads (see the table at
// wino_head_infer_kernel): stage 0 (cin <= 4) at widths 96 / 84 / 128, stage 1
// (cin 16) at 48 / 42 / 64; 0: no instance
int wino_head_band(int H, int W, int cin) {
  if (H < 4 || H % 2 != 0) return 0;
  if (cin >= 1 && cin <= 4) return W == 96 || W == 84 ? 6 : (W == 128 ? 4 : 0);
  if (cin == 16) return W == 48 || W == 42 || W == 64 ? 3 : 0;
  return 0;
}

namespace {

// The checks of wino_head_infer_launch; with t_wino_probe set nothing runs
bool head_infer(const void* x, bool is_u8, const float* w, int wcin, const float* b,
                float* pooled, int N, int H, int W, int Cs, int Cout, hipStream_t s) {
  if (N < 1 || N > kResBlockMaxFrames || !wino_enabled()) return false;
  if (wino_head_band(H, W, Cs) == 0) return false;
  if (static_cast<int64_t>(N) * H * W * (is_u8 ? Cs : 4 * Cs) > kMaxBufBytes) return false;
  HeadArgs a{};
  a.x = x; a.w = w; a.bias = b; a.pooled = pooled;
  a.N = N; a.H = H; a.Cs = Cs; a.wcin = wcin;
  if (is_u8) {
    // the launches replaced: frames_f32 and the Winograd conv + pool of the
    // 4-channel image (tile-row pairs: H % 4 == 0), not the direct conv + pool
    static const int pool_on = env_knob("SA_F32_WINO_POOL", 7);
    if (Cs < 1 || Cs > 4 || Cout != 16 || (wcin != Cs && wcin != 4) || (W * Cs) % 4 != 0 ||
        H % 4 != 0 || !(pool_on & 2))
      return false;
    if (W == 96) return run_head_infer<4, 16, 96, 6, 8>(a, s);
    if (W == 84) return run_head_infer<4, 16, 84, 6, 8>(a, s);
    return run_head_infer<4, 16, 128, 4, 8>(a, s);
  }
  if (Cs != 16 || wcin != 16 || Cout != 32) return false;
  // the launches replaced compute the conv in Winograd form (the fused conv +
  // pool, or wino_conv_kernel + maxpool_fwd: bitwise the same pooled values)
  const ConvArgs c = same_conv_args(x, w, b, pooled, N, H, W, Cs, Cout);
  if (const WinoProbe probe; !wino_conv_launch(c, false, s)) return false;
  if (W == 48) return run_head_infer<16, 32, 48, 3, 12>(a, s);
  if (W == 42) return run_head_infer<16, 32, 42, 3, 12>(a, s);
  return run_head_infer<16, 32, 64, 3, 8>(a, s);
}

}  // namespace

bool wino_head_infer_launch(const void* x, bool is_u8, const float* w, int wcin, const float* b,
                            float* pooled, int N, int H, int W, int Cs, int Cout,
                            hipStream_t s) {
  // dword row loads / 16-B rows
  if (reinterpret_cast<uintptr_t>(x) % (is_u8 ? 4 : 16) != 0) return false;
  return head_infer(x, is_u8, w, wcin, b, pooled, N, H, W, Cs, Cout, s);
}

int wino_head_form(int N, int H, int W, int cin, int cout, bool is_u8) {
  static const float dummy[4] = {};
  float* y = const_cast<float*>(dummy);  // geometry checks only: never read or written
  const WinoProbe probe;
  return head_infer(dummy, is_u8, dummy, cin, dummy, y, N, H, W, cin, cout, nullptr) ? 1 : 0;
}

}  // namespace cf32
}  // namespace sa
