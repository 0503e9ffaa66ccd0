// The Winograd F(2x2, 3x3) phases shared by the fp32 conv kernels of
// conv_wino.hip and conv_wino_infer.hip, their device utilities and the stage
// heads' pool helpers.  The two fused stage heads and the inference kernels
// are built from these functions alone; the forward / data-gradient kernel
// calls the weight transform, the stager and the input / output transforms;
// the two fused backward kernels the weight transform and the slot tables.
// Where a kernel keeps text of its own, a comment there says what was measured.
//
//   Y(2x2 tile) = A^T [ sum_ci (G g_ci,co G^T) .* (B^T d_ci B) ] A
//
//   wino_weight_transform   U = G g G^T of one (ci, co)
//   wino_u_to_lds           ... of a whole weight tensor into MFMA A fragments
//   wino_load_patch         a lane's 4x4 input patch, 4 channels per pixel
//   wino_input_transform    V = B^T d B
//   wino_mfma_block         M[xi] += U[xi] V[xi] over one 16-channel block
//   wino_output_transform   Y = A^T M A
//   wino_slots / wino_prefetch   the register-prefetch stager
//
// Everything is forced inline and works on register arrays of compile-time
// size: after unrolling no array is left in memory, and pointers into LDS
// keep their address space at the call site.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sa {
namespace cf32 {
namespace wino {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

// Measurement knobs (SA_WINO_ABLATE / SA_FUSED_ABLATE: drop parts of a
// kernel's work to time the rest) exist only in builds with
// -DSA_MEASURE_KNOBS=1; in production builds every knob test folds to false,
// so no environment variable can remove a synchronisation or a store.
#ifndef SA_MEASURE_KNOBS
#define SA_MEASURE_KNOBS 0
#endif
__device__ __forceinline__ bool knob(int v, int bit) {
  return SA_MEASURE_KNOBS && (v & bit) != 0;
}

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Pricing builds only (-DSA_WINO_XMFMA=bits, never a production build): the
// MFMA at an odd (compile-time, unrolled) index becomes ONE VALU FMA on the
// same operands - half the matrix work, wrong results, everything else
// unchanged - to measure how much of a kernel the matrix pipe sets.  Bit 0:
// forward / data-gradient MFMAs, bit 1: weight-gradient MFMAs.
#ifndef SA_WINO_XMFMA
#define SA_WINO_XMFMA 0
#endif
template <int BIT>
__device__ __forceinline__ f4 mfma4x(float a, float b, f4 c, int idx) {
  if ((SA_WINO_XMFMA & BIT) && (idx & 1)) {
    c[0] = fmaf(a, b, c[0]);
    return c;
  }
  return mfma4(a, b, c);
}

// 16-B loads through a buffer descriptor: an offset at or past the buffer's
// end returns zeros (the hardware range check), so a stager's padding and
// out-of-image elements need no select when they are committed to LDS, and
// the per-lane address is a 32-bit byte offset.  Launchers refuse tensors
// of >= 4 GB.
constexpr uint32_t kOOB = 0xFFFFFFF0u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const float* p, int64_t floats) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0,
                                           static_cast<int>(static_cast<uint32_t>(floats * 4)),
                                           0x00020000);
}
__device__ __forceinline__ f4 bload(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
constexpr int64_t kMaxBufBytes = 0xFFFFFF00ll;

// x / d for 0 <= x < 2^22, 1 <= d <= 2^10 (exact: (x + 0.5) / d lies at
// least 0.5 / d from an integer, far above the fp32 product's error)
__device__ __forceinline__ int fdivi(int x, float rd) {
  return static_cast<int>((static_cast<float>(x) + 0.5f) * rd);
}

// Winograd transform add / subtract, on float4 channel quads or scalars.  (A
// packed v_pk_add_f32 form was measured in round 4 and removed: the backend
// keeps <2 x float> arithmetic scalar, an inline-asm form read MFMA
// accumulators without the required wait states, and packed f32 beside MFMAs
// is an anti-lever on gfx950.)
template <typename T>
__device__ __forceinline__ T tadd(T a, T b) { return a + b; }
template <typename T>
__device__ __forceinline__ T tsub(T a, T b) { return a - b; }

// ReLU as one integer max on the bit pattern (negative floats, -0 and
// negative NaNs have the sign bit set: signed-int max with 0 gives +0);
// fmaxf(x, 0) is two instructions under IEEE mode (a canonicalising
// v_max_f32 x, x first)
__device__ __forceinline__ float relu0(float x) {
  return __int_as_float(max(__float_as_int(x), 0));
}

// ------------------------------------------------------- weight transform
// U = G g G^T of one (ci, co): gk[ky][kx] -> u[xi = 4 ra + rb], rows (G g)
// first, then columns
__device__ __forceinline__ void wino_weight_transform(const float (&gk)[3][3], float (&u)[16]) {
  float t[4][3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    t[0][kx] = gk[0][kx];
    t[1][kx] = 0.5f * ((gk[0][kx] + gk[1][kx]) + gk[2][kx]);
    t[2][kx] = 0.5f * ((gk[0][kx] - gk[1][kx]) + gk[2][kx]);
    t[3][kx] = gk[2][kx];
  }
#pragma unroll
  for (int ra = 0; ra < 4; ++ra) {
    u[4 * ra + 0] = t[ra][0];
    u[4 * ra + 1] = 0.5f * ((t[ra][0] + t[ra][1]) + t[ra][2]);
    u[4 * ra + 2] = 0.5f * ((t[ra][0] - t[ra][1]) + t[ra][2]);
    u[4 * ra + 3] = t[ra][2];
  }
}

// The workgroup's U into LDS as MFMA A fragments [16 xi][NB][4 g][CO][4]:
// element (ci, co) of block b = ci >> 4 sits at [xi][b][(ci >> 2) & 3][co]
// [ci & 3], so lane (co, g) reads its 4 k values with one 16-B load.
// tap(ky, kx, ci, co) fetches one weight (forward, flipped / transposed for
// a data gradient, bounds-checked); n = NB * 16 * CO, or 0 to skip.
template <int NB, int CO, int NTH, typename Tap>
__device__ __forceinline__ void wino_u_to_lds(float* U_s, int n, Tap tap) {
  constexpr int USTR = NB * 4 * CO * 4;  // floats per xi
  for (int e = threadIdx.x; e < n; e += NTH) {
    const int co = e % CO, ci = e / CO;
    float gk[3][3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) gk[ky][kx] = tap(ky, kx, ci, co);
    float u[16];
    wino_weight_transform(gk, u);
    const int b = NB > 1 ? ci >> 4 : 0, gq = (ci >> 2) & 3, v = ci & 3;
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) U_s[xi * USTR + ((b * 4 + gq) * CO + co) * 4 + v] = u[xi];
  }
}

// ------------------------------------------------- input / output transform
// Patches and transformed tiles travel by value (a struct of 16 or 4
// registers): with arrays taken by reference wino_conv_kernel's instances
// scheduled worse (profiles/experiments.md).
template <typename T>
struct Tile16 { T v[16]; };
typedef Tile16<f4> F16;
struct F4x4 { f4 v[4]; };

// The lane's 4x4 patch d[4 dy + dx] (4 channels per pixel) from an LDS image
// of row stride rowstr and pixel pitch pp floats.  RELU: ReLU on load.
template <bool RELU = false>
__device__ __forceinline__ F16 wino_load_patch(const float* xp, int rowstr, int pp) {
  F16 d;
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      f4 v = *reinterpret_cast<const f4*>(xp + dy * rowstr + dx * pp);
      if constexpr (RELU) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = relu0(v[q]);
      }
      d.v[4 * dy + dx] = v;
    }
  return d;
}

// V = B^T d B of a 4x4 patch d[4 dy + dx] -> V[xi = 4 a + b]; T = f4 (4
// channels per lane) or float (one)
template <typename T>
__device__ __forceinline__ Tile16<T> wino_input_transform(Tile16<T> dd) {
  const T (&d)[16] = dd.v;
  Tile16<T> VV;
  T (&V)[16] = VV.v;
  T s[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[q] = tsub(d[q], d[8 + q]);
    s[4 + q] = tadd(d[4 + q], d[8 + q]);
    s[8 + q] = tsub(d[8 + q], d[4 + q]);
    s[12 + q] = tsub(d[4 + q], d[12 + q]);
  }
#pragma unroll
  for (int ra = 0; ra < 4; ++ra) {
    V[4 * ra + 0] = tsub(s[4 * ra + 0], s[4 * ra + 2]);
    V[4 * ra + 1] = tadd(s[4 * ra + 1], s[4 * ra + 2]);
    V[4 * ra + 2] = tsub(s[4 * ra + 2], s[4 * ra + 1]);
    V[4 * ra + 3] = tsub(s[4 * ra + 1], s[4 * ra + 3]);
  }
  return VV;
}

// One 16-channel block of M[xi] += U[xi] V[xi]: 16 xi x 4 k-steps, two xi
// chains interleaved (the 16x16x4 f32 MFMA's dependent latency is 40 cycles,
// issue 32).  ub: the lane's A fragments of the block, ustr floats per xi.
// PRICED: the MFMAs take part in SA_WINO_XMFMA bit 0.
template <bool PRICED>
__device__ __forceinline__ void wino_mfma_block(const float* ub, int ustr, const f4 (&V)[16],
                                                f4 (&acc)[16]) {
#pragma unroll
  for (int xp2 = 0; xp2 < 8; ++xp2) {
    f4 ua[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) ua[q] = *reinterpret_cast<const f4*>(ub + (2 * xp2 + q) * ustr);
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int xi = 2 * xp2 + q;
        acc[xi] = PRICED ? mfma4x<1>(ua[q][v], V[xi][v], acc[xi], v)
                         : mfma4(ua[q][v], V[xi][v], acc[xi]);
      }
  }
}

// Y = A^T M A: acc[xi = 4 a + b] -> Y[2 dy + dx]
__device__ __forceinline__ F4x4 wino_output_transform(const f4 (&acc)[16]) {
  F4x4 YY;
  f4 (&Y)[4] = YY.v;
  f4 tt[4][2];
#pragma unroll
  for (int ra = 0; ra < 4; ++ra) {
    tt[ra][0] = tadd(tadd(acc[4 * ra], acc[4 * ra + 1]), acc[4 * ra + 2]);
    tt[ra][1] = tsub(tsub(acc[4 * ra + 1], acc[4 * ra + 2]), acc[4 * ra + 3]);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    Y[c] = tadd(tadd(tt[0][c], tt[1][c]), tt[2][c]);
    Y[2 + c] = tsub(tsub(tt[1][c], tt[2][c]), tt[3][c]);
  }
  return YY;
}

// One (16 tiles x 16 output channels) task over NB input-channel blocks:
// returns Y[2 dy + dx] = A^T M A with M[xi] = sum_ci U[xi][co][ci] (B^T d B)[xi][ci].
// xp: the lane's 4x4 patch (tile = lane & 15, channel quad = lane >> 4) in
// an LDS image of pixel pitch pp; up: the lane's A fragments of block 0
// ([16 xi][NB][4 g][CO][4]: ustr floats per xi, bstr per block).
template <int NB, bool RELU, bool PRICED>
__device__ __forceinline__ F4x4 wino_tile(const float* xp, int rowstr, int pp, const float* up,
                                          int ustr, int bstr) {
  f4 acc[16];
#pragma unroll
  for (int xi = 0; xi < 16; ++xi) acc[xi] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const F16 V = wino_input_transform(wino_load_patch<RELU>(xp + 16 * b, rowstr, pp));
    wino_mfma_block<PRICED>(up + b * bstr, ustr, V.v, acc);
  }
  return wino_output_transform(acc);
}

// ------------------------------------------------------------------ stager
// Register prefetch of a range's rows.  Thread slot k of a range always
// stages LDS element e = threadIdx.x + k NTH = (row L, column, channel quad)
// of an image of WL0-pixel rows (one pixel of zero padding on each side) and
// C channels: the column / quad part of its global offset is fixed per
// thread (sl_x, -1 in the padding), and the per-range (image, row) part
// comes from a small row table in LDS that each kernel builds for its own
// row arithmetic (-1: no such row).  sl_L: the slot's LDS row, -1 past
// maxrows.
template <int MAXC, int NTH, int C>
__device__ __forceinline__ void wino_slots(int WL0, int maxrows, int W, int (&sl_L)[MAXC],
                                           int (&sl_x)[MAXC]) {
  constexpr int C4 = C / 4, LC4 = C4 == 8 ? 3 : (C4 == 4 ? 2 : 0);
  static_assert(MAXC <= 32 && (C4 == 1 || C4 == 4 || C4 == 8), "stager");
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int e = threadIdx.x + k * NTH;
    const int ch = e & (C4 - 1), pix = e >> LC4;
    const int L = pix / WL0, col = pix - L * WL0;
    sl_L[k] = L < maxrows ? L : -1;
    sl_x[k] = (col >= 1 && col <= W) ? (col - 1) * C + 4 * ch : -1;
  }
}

// Every load is issued unconditionally (an invalid element reads past the
// buffer's end: zeros): a branch or a use right after a load makes the
// compiler wait for it, serialising the prefetch.  The table holds float
// offsets; off: a measurement knob that skips the global loads.
template <int MAXC>
__device__ __forceinline__ void wino_prefetch(__amdgpu_buffer_rsrc_t src, const int* tab_s,
                                              const int (&sl_L)[MAXC], const int (&sl_x)[MAXC],
                                              bool off, f4 (&stg)[MAXC]) {
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int rb = sl_L[k] >= 0 ? tab_s[sl_L[k]] : -1;
    const bool in = rb >= 0 && sl_x[k] >= 0 && !off;
    stg[k] = bload(src, in ? static_cast<uint32_t>(rb + sl_x[k]) * 4u : kOOB);
  }
}

// ------------------------------- the stage heads' 3x3 / 2 SAME max-pool
__device__ __forceinline__ void pool_take(f4& best, int (&code)[4], const f4 v, int c) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (v[q] > best[q]) {  // strict: the first maximal tap wins
      best[q] = v[q];
      code[q] = c;
    }
}

// Pool-phase lane -> (pooled column, channel quad) map of one wave (64 / CQ
// columns x CQ quads): every 16-lane group of a ds_read_b128 (gfx950 lane
// groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59},
// {36-43,48-51,60-63}) reads 16 distinct 16-B bank segments of the pre-pool
// image (pixel pitch IPP floats, pooled column pj -> pixel 2 pj): each
// segment s = (pj IPP / 2 + pq) mod 16 is taken by exactly one (pj, pq) per
// group.  The natural map (pq = lane % CQ) put 2-4 lanes of a group on one
// segment.
__host__ __device__ constexpr int b128_group(int l) {
  const int h = l & 31;
  const int g = (h < 4 || (h >= 12 && h < 16) || (h >= 20 && h < 28)) ? 0 : 1;
  return g + 2 * (l >> 5);
}
template <int CQ, int IPP>
struct PoolLaneMap {
  unsigned char pj[64] = {}, pq[64] = {};
  constexpr PoolLaneMap() {
    constexpr int NP = 64 / CQ;
    bool used[64] = {};
    for (int g = 0; g < 4; ++g) {
      int next = 0;  // next lane of group g to assign
      for (int seg = 0; seg < 16; ++seg) {
        int pick = -1;
        for (int c = 0; c < NP && pick < 0; ++c)
          for (int q = 0; q < CQ && pick < 0; ++q)
            if (!used[c * CQ + q] && (c * (IPP / 2) + q) % 16 == seg) pick = c * CQ + q;
        while (b128_group(next) != g) ++next;
        used[pick] = true;
        pj[next] = static_cast<unsigned char>(pick / CQ);
        pq[next] = static_cast<unsigned char>(pick % CQ);
        ++next;
      }
    }
  }
};
template <int CQ, int IPP>
constexpr bool pool_lane_map_ok() {
  constexpr PoolLaneMap<CQ, IPP> m{};
  bool seen[64] = {};
  for (int l = 0; l < 64; ++l) {
    const int id = m.pj[l] * CQ + m.pq[l];
    if (m.pj[l] >= 64 / CQ || seen[id]) return false;
    seen[id] = true;
  }
  return true;
}
static_assert(pool_lane_map_ok<8, 36>() && pool_lane_map_ok<4, 20>(), "pool lane map");

// LDS plan of a conv + pool over one WHOLE image per workgroup
template <int CIN, int COUT, int H, int W>
struct PoolImgGeo {
  static constexpr int TY = H / 2, TX = W / 2, NTI = TY * TX;
  static constexpr int RT = (NTI + 15) / 16 * 16;
  static constexpr int NG = RT / 16, NS = COUT / 16, NTASK = NG * NS;
  static constexpr int NW = 8;                       // tasks: two per wave (0..5), one (6, 7)
  static constexpr int ROWS = H + 2, Wl = W + 2;
  static constexpr int PP = CIN + 4, IPP = COUT + 4;
  static constexpr int XREG = (ROWS * Wl * PP > H * W * IPP) ? ROWS * Wl * PP : H * W * IPP;
  // only the image interior is staged (the zero border is rewritten per image)
  static constexpr int MAXC = (H * W * (CIN / 4) + 64 * NW - 1) / (64 * NW);
  static constexpr size_t bytes = sizeof(float) * (16 * CIN * COUT + XREG + ROWS);
};

// The 3x3 / 2 window of pooled element (pr, pc), channel quad pq, over a whole
// pre-pool LDS image [H][W][IPP] (pad-before 0: the tap row / column past the
// map is padding), taps in row-major order
template <int H, int W, int IPP>
__device__ __forceinline__ void pool_window_img(const float* img, int pr, int pc, int pq, f4& best,
                                                int (&code)[4]) {
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int y = 2 * pr + dy, x = 2 * pc + dx;
      if (y < H && x < W)
        pool_take(best, code, *reinterpret_cast<const f4*>(img + (y * W + x) * IPP + 4 * pq),
                  3 * dy + dx);
    }
}

template <typename Kern>
void allow_lds_w(Kern k, size_t bytes) {
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(bytes));
    if (e != hipSuccess) (void)hipGetLastError();  // the launch reports it
  }
}

// While set, a Winograd launcher answers whether it would run the shape and
// launches nothing.  Defined in conv_wino.hip; set only by a WinoProbe, which nests.
extern thread_local bool t_wino_probe;
struct WinoProbe {
  const bool prev = t_wino_probe;
  WinoProbe() { t_wino_probe = true; }
  ~WinoProbe() { t_wino_probe = prev; }
};

}  // namespace wino
}  // namespace cf32
}  // namespace sa
