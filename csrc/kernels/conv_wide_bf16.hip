// Stage 0 of the bf16 deep torso on uint8 frames of 5 to 16 channels (gfx950):
//
//   conv1w_pool_fwd : uint8 [N,H,W,C] -> conv3x3(C->16) + b -> max-pool 3x3/2
//                     SAME; pooled bf16 + argmax (u8) in conv1_pool_fwd's
//                     layout and tie rule (the first maximal in-image tap).
//   conv1w_pool_bwd : weight and bias gradient from (dP, argmax, frames).
//
// conv1_pool_fwd/bwd (conv_torso.hip) pack one pixel's 3 or 4 channels into a
// bf16x4 operand; here a pixel's channels are zero-padded to Cp = 8 (C <= 8)
// or 16 values in LDS and the product runs on v_mfma_f32_16x16x32_bf16 as
// D^T = W^T X^T: a lane feeds 8 contiguous channel values of one pixel with
// one ds_read_b128.  Cp = 8: the four lane groups are kx = 0..3 of one kernel
// row (kx = 3 zero-weight), 3 MFMAs per 16 pixels.  Cp = 16: a lane group
// reads half a pixel, two taps fill one K = 32, 5 MFMAs with a zero-weight
// tenth tap.  1/255 is folded into the bf16 weights (raw byte values are exact
// in bf16), so the forward computes sum bf16(w / 255) * byte.
//
// Staging.  A full-width band of NHWC uint8 rows is one contiguous byte span;
// it is prefetched as 16-byte chunks from the span's aligned-down start
// (ByteSpan) while the previous tile computes.  C need not divide 16 and the
// span need not start on a chunk, so the commit goes through a RAW-BYTE LDS
// buffer and a second pass (expand_rows) instead of converting in registers:
// in registers every byte needs its own (pixel, channel) division by a runtime
// C and a 2-byte LDS store (16 of each per chunk); the second pass does one
// division per (pixel, 8-channel half), reads the half's 8 bytes as three
// aligned dwords and writes it, expanded to bf16 with channels >= C zeroed,
// as one ds_write_b128 into the [rows][W+2][pitch] halo tile, halo columns,
// out-of-image rows and trailing pad pixels included (every pixel the MFMAs
// read is written once per tile).  The raw buffer costs no LDS: it aliases
// the pre-pool key map (forward) or the dY tile (backward), both dead between
// a tile's barrier and its expansion.
//
// LDS pixel pitch: 8 elements at Cp = 8 (16 consecutive pixels x 16 B are one
// conflict-free ds_read_b128 wavefront quarter).  At Cp = 16 a 32-B pitch
// would put the 16 lanes of a quarter (one half of 16 consecutive pixels) on
// every other 16-B bank group, 2-way conflicted; a pitch of 24 elements (48 B)
// makes 48 i mod 256 distinct for i < 16.  Elements 16..23 are never touched.
#include "conv_common.h"
#include "conv_launchers.h"
#include "conv_tile.h"

#include <stdexcept>
#include <string>
#include <type_traits>

namespace sa {
namespace conv {
namespace {

constexpr int kCout = 16;
constexpr int kSpanRegs = 4;  // 16-B chunks per lane of the frame span (ByteSpan v0..v3)
// bytes of a staged span: kSpanRegs chunks per lane, less the alignment head
constexpr int kSpanBytes = kSpanRegs * kThreads * 16 - 16;
constexpr int kPadPx = 4;  // zero pixels after the tile (zero-weight kx = 3)

__host__ __device__ constexpr int px_pitch(int CP) { return CP == 16 ? 24 : 8; }
__host__ __device__ constexpr int fwd_mfmas(int CP) { return CP == 16 ? 5 : 3; }

// Rows [r_begin, r_begin + rows) of frame n, clipped to the image, as 16-B
// chunks from the aligned-down start of the span.  Every lane issues all its
// loads (index clamped to the last chunk: every chunk read holds a byte of
// the span) so that the staging registers are always written by a load
// (RowStager's note on vmcnt).
// A native vector, not uint4: copies of HIP's uint4 class between two address
// spaces are memcpys that kept the whole stager in scratch.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct ByteSpan {
  u32x4 v0, v1, v2, v3;
  int head;   // bytes of chunk 0 before the span
  int row0;   // first staged row (tile coordinates)
  int nrows;  // staged image rows
  int total;  // chunks
  __device__ __forceinline__ void issue(const uint8_t* __restrict__ src, int n, int H,
                                        int W, int C, int r_begin, int rows) {
    const int rlo = max(r_begin, 0), rhi = min(r_begin + rows, H);
    row0 = rlo - r_begin;
    nrows = rhi > rlo ? rhi - rlo : 0;
    const uint8_t* p = src + (static_cast<int64_t>(n) * H + rlo) * W * C;
    head = static_cast<int>(reinterpret_cast<uintptr_t>(p) & 15);
    total = (head + nrows * W * C + 15) >> 4;
    const u32x4* a = reinterpret_cast<const u32x4*>(p - head);
    const int last = max(total - 1, 0), t = threadIdx.x;
    v0 = a[min(t, last)];
    v1 = a[min(t + kThreads, last)];
    v2 = a[min(t + 2 * kThreads, last)];
    v3 = a[min(t + 3 * kThreads, last)];
  }
  __device__ __forceinline__ void commit(uint8_t* raw) const {
    const int t = threadIdx.x;
    u32x4* r = reinterpret_cast<u32x4*>(raw);
    if (t < total) r[t] = v0;
    if (t + kThreads < total) r[t + kThreads] = v1;
    if (t + 2 * kThreads < total) r[t + 2 * kThreads] = v2;
    if (t + 3 * kThreads < total) r[t + 3 * kThreads] = v3;
  }
};

// Raw span bytes -> bf16 halo tile x_s [rows][W+2][px_pitch(CP)] + kPadPx
// zero pixels, one (pixel, 8-channel half) per thread and step.
template <int CP>
__device__ __forceinline__ void expand_rows(int head, int row0, int nrows,
                                            const uint8_t* raw, bf16_t* x_s, int W,
                                            int C, int rows) {
  constexpr int PX = px_pitch(CP), NH = CP / 8;
  const int Wp = W + 2;
  const int total = (rows * Wp + kPadPx) * NH;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int half = NH == 2 ? (e & 1) : 0;
    const int pix = NH == 2 ? (e >> 1) : e;
    const int rr = pix / Wp, cc = pix - rr * Wp;
    const int ir = rr - row0;  // pad pixels: rr == rows, ir >= nrows
    uint4 o = make_uint4(0, 0, 0, 0);
    if (cc >= 1 && cc <= W && ir >= 0 && ir < nrows) {
      const int b = head + (ir * W + cc - 1) * C + 8 * half;
      const int nb = C - 8 * half;  // channels of this half present in the frame
      const uint32_t* d = reinterpret_cast<const uint32_t*>(raw + (b & ~3));
      const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
      uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, b & 3);
      uint32_t hi = __builtin_amdgcn_alignbyte(d2, d1, b & 3);
      // channels >= C are the next pixel's bytes: zero them
      lo = nb >= 4 ? lo : (lo & ((1u << (8 * nb)) - 1u));
      hi = nb >= 8 ? hi : (nb <= 4 ? 0u : (hi & ((1u << (8 * (nb - 4))) - 1u)));
      // byte values are exact in bf16: the top half of the fp32
      uint32_t f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        f[j] = __float_as_uint(static_cast<float>(((j < 4 ? lo : hi) >> (8 * (j & 3))) & 0xFF));
      o.x = __builtin_amdgcn_perm(f[1], f[0], 0x07060302u);
      o.y = __builtin_amdgcn_perm(f[3], f[2], 0x07060302u);
      o.z = __builtin_amdgcn_perm(f[5], f[4], 0x07060302u);
      o.w = __builtin_amdgcn_perm(f[7], f[6], 0x07060302u);
    }
    *reinterpret_cast<uint4*>(x_s + pix * PX + 8 * half) = o;
  }
}

// conv1_pool_fwd_kernel's scaffold (persistent tiles of Rp pooled rows, the
// next tile's span in flight during the compute, the pre-pool map only in LDS
// as order keys) on the Cp-padded tile.  The weight operand (3 or 5 bf8 per
// lane) is read from LDS once and stays in registers.  The pool's pad columns
// are rewritten every tile because the raw bytes lie over the key map.
template <int CP, int HC, int WC, int RC>
__global__ __launch_bounds__(kThreads) void conv1w_pool_fwd_kernel(
    const uint8_t* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ bias, bf16_t* __restrict__ pooled,
    uint8_t* __restrict__ argmax, int N, int H_, int W_, int Rp_, int C, int pb_h,
    int pb_w, int xcd) {
  constexpr int PX = px_pitch(CP), NM = fwd_mfmas(CP);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = HC ? HC : H_, W = WC ? WC : W_, Rp = RC ? RC : Rp_;
  const int Hp = (H + 1) / 2, Wo = (W + 1) / 2;
  const int Wp = W + 2;
  bf16_t* w_s = reinterpret_cast<bf16_t*>(smem);       // [NM][16 co][32 k]
  bf16_t* y_s = w_s + NM * 512;                          // [2Rp+1][W+2][16]
  bf16_t* x_s = y_s + (2 * Rp + 1) * Wp * kCout;         // [2Rp+3][W+2][PX] + pad
  uint8_t* raw = reinterpret_cast<uint8_t*>(y_s);
  for (int e = threadIdx.x; e < NM * 512; e += blockDim.x) {
    const int mm = e >> 9, co = (e >> 5) & 15, k = e & 31;
    // Cp = 8: k = 8 kx + ci of kernel row mm; Cp = 16: k = 16 (tap & 1) + ci
    const int tap = CP == 8 ? 3 * mm + (k >> 3) : 2 * mm + (k >> 4);
    const int ci = CP == 8 ? (k & 7) : (k & 15);
    const bool real = (CP == 8 ? (k >> 3) < 3 : tap < 9) && ci < C;
    w_s[e] = real ? f2bf(w[(tap * C + ci) * kCout + co] * (1.0f / 255.0f)) : 0;
  }
  const int lane = lane_id();
  const int wave = wave_id();
  const int grp = lane >> 4;
  float breg[1][4];
  bias_regs<kCout>(bias, reinterpret_cast<float*>(x_s), breg);  // barrier: w_s complete
  const float b0 = breg[0][0], b1 = breg[0][1], b2 = breg[0][2], b3 = breg[0][3];
  bf8 a[NM];
  int off[NM];  // this lane's tap offsets in the halo tile
#pragma unroll
  for (int mm = 0; mm < NM; ++mm) {
    a[mm] = *reinterpret_cast<const bf8*>(w_s + (mm * 16 + (lane & 15)) * 32 + 8 * grp);
    if constexpr (CP == 8) {
      off[mm] = (mm * Wp + grp) * PX;
    } else {
      const int t = min(2 * mm + (grp >> 1), 8);  // the tenth tap re-reads the ninth
      off[mm] = ((t / 3) * Wp + t % 3) * PX + 8 * (grp & 1);
    }
  }
  const int tpi = (Hp + Rp - 1) / Rp;
  const int ntiles = N * tpi;
  ByteSpan sx;
  auto issue = [&](int t) {
    const int n = t / tpi, i0 = (t - n * tpi) * Rp, Rpv = min(Rp, Hp - i0);
    sx.issue(x, n, H, W, C, 2 * i0 - pb_h - 1, 2 * Rpv + 3);
  };
  const TileIter it(ntiles, xcd);
  int tile = it.first;
  if (it.valid(tile)) issue(tile);
  for (; it.valid(tile); tile = it.next(tile)) {
    const int n = tile / tpi, i0 = (tile - n * tpi) * Rp, Rpv = min(Rp, Hp - i0);
    const int cr0 = 2 * i0 - pb_h;
    const int Rc = 2 * Rpv + 1;
    const int npix = Rc * W;
    __syncthreads();  // the previous tile's pool (y_s) and MFMA reads (x_s) are done
    sx.commit(raw);
    const int head = sx.head, row0 = sx.row0, nrows = sx.nrows;
    __syncthreads();
    // unconditional (no next tile: re-issue this one, unused) - a conditional
    // issue leaves a join at the loop back-edge
    issue(it.valid(it.next(tile)) ? it.next(tile) : tile);
    expand_rows<CP>(head, row0, nrows, raw, x_s, W, C, Rc + 2);
    __syncthreads();  // raw bytes consumed: y_s is the key map again
    init_pool_pads<kCout>(y_s, Rc, W);
    const int ngroups = (npix + 15) / 16;
    for (int g = wave; g < ngroups; g += kWaves) {
      int q = g * 16 + (lane & 15);
      const bool valid = q < npix;
      if (!valid) q = 0;
      const int qr = q / W, qc = q - (q / W) * W;
      const bf16_t* xb = x_s + (qr * Wp + qc) * PX;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int mm = 0; mm < NM; ++mm)
        acc = mfma32(a[mm], *reinterpret_cast<const bf8*>(xb + off[mm]), acc);
      if (valid) {
        const float v[4] = {acc[0] + b0, acc[1] + b1, acc[2] + b2, acc[3] + b3};
        store4_ord_in(y_s + (q + 2 * qr + 1) * kCout + 4 * grp, v,
                      static_cast<unsigned>(cr0 + qr) < static_cast<unsigned>(H));
      }
    }
    __syncthreads();
    pool_tile<kCout>(y_s, W, Wo, pb_w, n, Hp, i0, Rpv, pooled, argmax);
  }
}

// dW[tap][ci][co] += sum_p X[p + tap][ci] dY[p][co] as a pixel-reduction GEMM
// on 16x16x16 bf16 MFMA, both operands read transposed from LDS (lds_tr4, as
// conv1_pool_bwd_kernel): an A tile is 4 pixels x 16 contiguous LDS values.
// Cp = 16: one tile per tap, 9 accumulators.  Cp = 8: two neighbouring taps of
// a kernel row are 16 contiguous values (pitch 8), tiles (kx 0, 1) and (kx 2,
// a never-flushed kx 3), 6 accumulators.  dY comes from
// gather_pool_grad_blocks; the bias gradient from a ones-row MFMA.  The fp32
// accumulators live across the persistent tile loop and are scaled by 1/255
// at the flush: float atomics, or (part != nullptr) one slot per wave for
// slot_reduce_kernel.  Only the frame's C channels of dw are written.
template <int CP, int HC, int WC, int RC>
__global__ __launch_bounds__(kThreads) void conv1w_pool_bwd_kernel(
    const bf16_t* __restrict__ dP, const uint8_t* __restrict__ argmax,
    const uint8_t* __restrict__ x, float* __restrict__ dw, float* __restrict__ db,
    int N, int H_, int W_, int R_, int C, int pb_h, int pb_w, int xcd,
    float* __restrict__ part) {
  constexpr int PX = px_pitch(CP), NT = CP == 16 ? 9 : 6;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = HC ? HC : H_, W = WC ? WC : W_, R = RC ? RC : R_;
  const int Wp = W + 2;
  const int Hp = (H + 1) / 2, Wo = (W + 1) / 2;
  const int d_elems = (R + 2) * Wp * kCout;
  const int prow_max = (R + 2) / 2 + 2;
  bf16_t* d_s = reinterpret_cast<bf16_t*>(smem);        // dY halo tile + a zero pixel
  bf16_t* x_s = d_s + d_elems + kCout;                    // [R+2][W+2][PX] + pad
  bf16_t* p_s = x_s + ((R + 2) * Wp + kPadPx) * PX;
  uint8_t* g_s = reinterpret_cast<uint8_t*>(p_s + prow_max * Wo * kCout);
  uint8_t* raw = reinterpret_cast<uint8_t*>(d_s);         // below the zero pixel
  for (int e = threadIdx.x; e < kCout; e += blockDim.x) d_s[d_elems + e] = 0;
  const int lane = lane_id();
  const int wave = wave_id();
  const int sub = lane & 15;
  f4 accw[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accw[t] = f4{0.f, 0.f, 0.f, 0.f};
  f4 accb = f4{0.f, 0.f, 0.f, 0.f};
  s4 ones;
  ones[0] = ones[1] = ones[2] = ones[3] = 0x3F80;
  const int tpi = (H + R - 1) / R;
  const int ntiles = N * tpi;
  ByteSpan sx;
  SpanStager<NREG> sp, sg;
  const int prow_bytes = Wo * kCout;
  auto issue = [&](int t) {
    const int n = t / tpi, r0 = (t - n * tpi) * R, Rv = min(R, H - r0);
    sx.issue(x, n, H, W, C, r0 - 1, Rv + 2);
    int lo, hi;
    pooled_rows(r0 - 1, Rv + 2, pb_h, Hp, &lo, &hi);
    const int64_t prow0 = static_cast<int64_t>(n) * Hp + lo;
    sp.issue(reinterpret_cast<const uint8_t*>(dP), prow0 * prow_bytes * 2,
             (hi - lo + 1) * prow_bytes * 2);
    sg.issue(argmax, prow0 * prow_bytes, (hi - lo + 1) * prow_bytes);
  };
  const TileIter it(ntiles, xcd);
  int tile = it.first;
  if (it.valid(tile)) issue(tile);
  for (; it.valid(tile); tile = it.next(tile)) {
    const int n = tile / tpi, r0 = (tile - n * tpi) * R, Rv = min(R, H - r0);
    int lo, hi;
    pooled_rows(r0 - 1, Rv + 2, pb_h, Hp, &lo, &hi);
    __syncthreads();  // the previous tile's MFMA reads are done
    sx.commit(raw);
    sp.commit(reinterpret_cast<uint8_t*>(p_s));
    sg.commit(g_s);
    const int head = sx.head, row0 = sx.row0, nrows = sx.nrows;
    __syncthreads();
    issue(it.valid(it.next(tile)) ? it.next(tile) : tile);  // unconditional, as forward
    expand_rows<CP>(head, row0, nrows, raw, x_s, W, C, Rv + 2);
    __syncthreads();  // raw bytes consumed: the gather owns d_s (it writes every cell)
    const int npix = Rv * W;
    gather_pool_grad_blocks<kCout>(p_s, g_s, lo, hi, W, Wo, pb_h, pb_w, r0 - 1, Rv + 2,
                                   d_s);
    __syncthreads();
    const int ngroups = (npix + 15) / 16;
    for (int g = wave; g < ngroups; g += kWaves) {
      const int qb = g * 16 + 4 * (lane >> 4) + (sub >> 2);
      const bool vb = qb < npix;
      const int qbr = vb ? qb / W : 0, qbc = vb ? qb - qbr * W : 0;
      const s4 bd = lds_tr4(d_s + (vb ? ((qbr + 1) * Wp + qbc + 1) * kCout : d_elems) +
                            (sub & 3) * 4);
      // row = pixel qb (invalid pixels pair the zero dY pixel with the tile's
      // first pixels), columns = 16 contiguous values at halo pixel (qbr + ky,
      // qbc + kx)
      const bf16_t* xb = x_s + (vb ? qbr * Wp + qbc : 0) * PX + (sub & 3) * 4;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int ky = CP == 16 ? t / 3 : t / 2, kx = CP == 16 ? t % 3 : 2 * (t % 2);
        accw[t] = mfma16(lds_tr4(xb + (ky * Wp + kx) * PX), bd, accw[t]);
      }
      accb = mfma16(ones, bd, accb);
    }
  }
  // D[m = 4 (lane >> 4) + i][co = sub]: m = ci of the tap (Cp = 16), or
  // 8 (kx & 1) + ci of the tile's two taps (Cp = 8)
  const int nel = 9 * C * kCout + kCout;
  float* slot = part ? part + (static_cast<int64_t>(blockIdx.x) * kWaves + wave) * nel
                     : nullptr;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mrow = 4 * (lane >> 4) + i;
      const int ky = CP == 16 ? t / 3 : t / 2;
      const int kx = CP == 16 ? t % 3 : 2 * (t % 2) + (mrow >> 3);
      const int ci = CP == 16 ? mrow : (mrow & 7);
      if (kx < 3 && ci < C) {
        const int o = ((ky * 3 + kx) * C + ci) * kCout + sub;
        const float v = accw[t][i] * (1.0f / 255.0f);
        if (slot) slot[o] = v;
        else atomicAdd(dw + o, v);
      }
    }
  if ((lane >> 4) == 0) {
    if (slot) slot[9 * C * kCout + sub] = accb[0];
    else atomicAdd(db + sub, accb[0]);
  }
}

template <typename K>
void set_smem(K kernel, size_t bytes) {
  if (bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(bytes)) != hipSuccess)
    (void)hipGetLastError();  // the launch itself reports an LDS request it cannot meet
}

// ----- tile-height rules: constexpr, so that the same rule picks the compiled
// geometry and the runtime tile height.  Written for the instance's Cp (the
// widest frame it takes), not the frame's C.  The x tile is 2 (Cp = 8) or 6
// (Cp = 16) times conv1_pool_fwd's, so the rules size a tile for the
// workgroups per CU each instance is meant to keep resident, counted as
// grid_for counts them (1 KB of slack per workgroup): forward 3 at Cp = 8
// and 2 at Cp = 16 (72x96: 4 and 3 pooled rows), backward 2 (11 and 6 rows).
constexpr int kLdsBytes = 160 * 1024;
constexpr int fwd_per_cu(int CP) { return CP == 16 ? 2 : 3; }
constexpr int kBwdPerCu = 2;

constexpr int fwd_lds(int CP, int Rp, int W) {
  return (fwd_mfmas(CP) * 512 + (2 * Rp + 1) * (W + 2) * kCout +
          ((2 * Rp + 3) * (W + 2) + kPadPx) * px_pitch(CP)) * 2;
}
// the span fits the staging registers, and (with its alignment head and the
// expansion's dword over-read) the map it is committed over
constexpr bool span_fits(int rows, int W, int CP, int over_bytes) {
  return rows * W * CP <= kSpanBytes && rows * W * CP + 32 <= over_bytes;
}
constexpr bool fwd_fits(int CP, int Rp, int W) {
  return span_fits(2 * Rp + 3, W, CP, (2 * Rp + 1) * (W + 2) * kCout * 2);
}
constexpr int rows_fwd(int H, int W, int CP, int px) {
  const int Hp = (H + 1) / 2;
  int Rp = (px / W - 1) / 2;
  if (Rp < 1) Rp = 1;
  while (Rp > 1 && (!fwd_fits(CP, Rp, W) ||
                    (fwd_lds(CP, Rp, W) + 1024) * fwd_per_cu(CP) > kLdsBytes))
    --Rp;
  return balance_rows(Hp, Rp > Hp ? Hp : Rp);
}

constexpr int bwd_lds(int CP, int R, int W) {
  const int Wo = (W + 1) / 2, prow_max = (R + 2) / 2 + 2;
  return ((R + 2) * (W + 2) * kCout + kCout + ((R + 2) * (W + 2) + kPadPx) * px_pitch(CP) +
          prow_max * Wo * kCout) * 2 + prow_max * Wo * kCout;
}
constexpr bool bwd_fits(int CP, int R, int W) {
  return span_fits(R + 2, W, CP, (R + 2) * (W + 2) * kCout * 2) &&
         ((R + 2) / 2 + 2) * ((W + 1) / 2) * kCout * 2 <= NREG * kThreads * 16;
}
constexpr int rows_bwd(int H, int W, int CP, int px) {
  int R = px / W;
  if (R < 1) R = 1;
  while (R > 1 && (!bwd_fits(CP, R, W) || (bwd_lds(CP, R, W) + 1024) * kBwdPerCu > kLdsBytes))
    --R;
  return balance_rows(H, R > H ? H : R);
}

constexpr int kPxFwd = 900, kPxBwd = 1176;  // ConvTune's px_conv1_fwd / px_conv1_bwd defaults
template <int CP>
struct RowsFwd {
  static constexpr int rows(int H, int W) { return rows_fwd(H, W, CP, kPxFwd); }
};
template <int CP>
struct RowsBwd {
  static constexpr int rows(int H, int W) { return rows_bwd(H, W, CP, kPxBwd); }
};

void require_fit(bool ok, const char* what) {
  if (!ok)
    throw std::invalid_argument(std::string(what) +
                                ": frame too wide for the conv tile staging");
}

template <int V>
using IC = std::integral_constant<int, V>;

// f(IC<H>, IC<W>, IC<R>) with the compiled geometry that matches (the IMPALA,
// Atari and Doom frames at the default tile height), else with zeros: the
// runtime-geometry kernel.  Returns whether one matched.
template <int HH, int WW, int RR, typename F>
bool geo_try(int H, int W, int R, F& f) {
  if (H == HH && W == WW && R == RR) {
    f(IC<HH>{}, IC<WW>{}, IC<RR>{});
    return true;
  }
  return false;
}
template <typename RF, typename F>
bool with_geo(int H, int W, int R, F&& f) {
  if (conv_tune_set("specialize", -1)) {
    if (geo_try<72, 96, RF::rows(72, 96)>(H, W, R, f)) return true;
    if (geo_try<84, 84, RF::rows(84, 84)>(H, W, R, f)) return true;
    if (geo_try<72, 128, RF::rows(72, 128)>(H, W, R, f)) return true;
  }
  f(IC<0>{}, IC<0>{}, IC<0>{});
  return false;
}

template <int CP>
void fwd_launch(const uint8_t* x, const float* w, const float* b, bf16_t* pooled,
                uint8_t* argmax, int N, int H, int W, int C, int pb_h, int pb_w,
                hipStream_t s) {
  const int Hp = (H + 1) / 2;
  const int Rp = rows_fwd(H, W, CP, conv_tune_set("px_conv1_fwd", -1));
  const size_t smem = fwd_lds(CP, Rp, W);
  require_fit(fwd_fits(CP, Rp, W) && smem <= static_cast<size_t>(kLdsBytes),
              "conv1w_pool_fwd");
  const int ntiles = N * ((Hp + Rp - 1) / Rp);
  int grid_max = 0;
  const int grid = conv1w_grid(ntiles, smem, false, &grid_max);
  const int xcd = conv_tune_set("xcd", -1);
  const bool spec = with_geo<RowsFwd<CP>>(H, W, Rp, [&](auto h, auto ww, auto r) {
    auto k = conv1w_pool_fwd_kernel<CP, decltype(h)::value, decltype(ww)::value,
                                    decltype(r)::value>;
    set_smem(k, smem);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kThreads), smem, s, x, w, b, pooled, argmax,
                       N, H, W, Rp, C, pb_h, pb_w, xcd);
  });
  conv1w_note(false, grid, grid_max, ntiles, Rp, spec);
}

template <int CP>
void bwd_launch(const bf16_t* dP, const uint8_t* argmax, const uint8_t* x, float* dw,
                float* db, int N, int H, int W, int C, int pb_h, int pb_w,
                hipStream_t s, float* part) {
  const int R = rows_bwd(H, W, CP, conv_tune_set("px_conv1_bwd", -1));
  const size_t smem = bwd_lds(CP, R, W);
  require_fit(bwd_fits(CP, R, W) && smem <= static_cast<size_t>(kLdsBytes),
              "conv1w_pool_bwd");
  const int ntiles = N * ((H + R - 1) / R);
  int grid_max = 0;
  const int grid = conv1w_grid(ntiles, smem, true, &grid_max);
  const int xcd = conv_tune_set("xcd", -1);
  const bool spec = with_geo<RowsBwd<CP>>(H, W, R, [&](auto h, auto ww, auto r) {
    auto k = conv1w_pool_bwd_kernel<CP, decltype(h)::value, decltype(ww)::value,
                                    decltype(r)::value>;
    set_smem(k, smem);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kThreads), smem, s, dP, argmax, x, dw, db, N,
                       H, W, R, C, pb_h, pb_w, xcd, part);
  });
  conv1w_note(true, grid, grid_max, ntiles, R, spec);
  if (part)
    wgrad_reduce_slots(part, grid * kWaves, 9 * C * kCout + kCout, 9 * C * kCout, dw, db,
                       s);
}

}  // namespace

void conv1w_pool_fwd_launch(const uint8_t* x, const float* w, const float* b,
                            void* pooled, uint8_t* argmax, int N, int H, int W,
                            int C, int pb_h, int pb_w, hipStream_t s) {
  require_fit(C >= 5 && C <= 16, "conv1w_pool_fwd: 5 to 16 frame channels");
  auto P = static_cast<bf16_t*>(pooled);
  if (C <= 8) fwd_launch<8>(x, w, b, P, argmax, N, H, W, C, pb_h, pb_w, s);
  else fwd_launch<16>(x, w, b, P, argmax, N, H, W, C, pb_h, pb_w, s);
}

void conv1w_pool_bwd_launch(const void* dP, const uint8_t* argmax, const uint8_t* x,
                            float* dw, float* db, int N, int H, int W, int C,
                            int pb_h, int pb_w, hipStream_t s, float* part) {
  require_fit(C >= 5 && C <= 16, "conv1w_pool_bwd: 5 to 16 frame channels");
  auto DP = static_cast<const bf16_t*>(dP);
  if (C <= 8) bwd_launch<8>(DP, argmax, x, dw, db, N, H, W, C, pb_h, pb_w, s, part);
  else bwd_launch<16>(DP, argmax, x, dw, db, N, H, W, C, pb_h, pb_w, s, part);
}

}  // namespace conv
}  // namespace sa
