// Tile-loop helpers shared by the bf16 conv-torso translation units
// (conv_torso.hip, conv_wide_bf16.hip): the persistent tile schedule, the
// span stager, the order-key max-pool with argmax, the pooled-gradient gather
// and the row-balancing rule.  Internal linkage: each translation unit
// compiles its own copy.
#pragma once
#include "conv_common.h"

namespace sa {
namespace conv {
namespace {

constexpr int kThreads = 256;
// Phase ablation for timing studies (tools/conv_bench.py, knob "ablate":
// 1 pool/gather, 2 wgrad, 4 conv, 8 LDS commit) exists only in builds with
// -DSA_CONV_ABLATE: the runtime branches around the staging commit make the
// compiler's vmcnt bookkeeping conservative (it then drains the prefetch).
#ifndef SA_LATE_PREFETCH
#define SA_LATE_PREFETCH 0
#endif
constexpr bool kLatePrefetch = SA_LATE_PREFETCH;
#ifdef SA_CONV_ABLATE
__device__ __forceinline__ bool kKeep(int xcd, int bit) { return !((xcd >> 8) & bit); }
#else
__device__ __forceinline__ constexpr bool kKeep(int, int) { return true; }
#endif
constexpr int kWaves = kThreads / 64;
constexpr int GPW = 4;  // 16-pixel groups per wave per chunk
constexpr int NREG = 4;  // staging registers (uint4) per lane per stream

// LDS halo images [rows][W+2][C].  32-channel images (64-B pixels) get 32 B
// of padding per row, so a row starts 2 slots (mod 4) after the previous
// one; their MFMA column groups are 2 rows x 8 pixels (GroupMap).  A
// ds_read_b128 of such a group (16 lanes x one 16-B chunk) is then
// conflict-free for any starting pixel; 16 consecutive 64-B pixels of one row
// would be 2-way conflicted.  16-channel images are unpadded, their groups
// 16 consecutive pixels (paired-tap reads of 32-B pixels are conflict-free).
__host__ __device__ constexpr int row_pitch(int C, int W) {
  return (W + 2) * C + (C == 32 ? 16 : 0);
}
__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Persistent tile schedule.  xcd == 0: tile = blockIdx.x + k * gridDim.x.
// xcd == 1: XCD-aware - workgroups are dispatched round-robin over the 8 XCDs
// (b % 8), so each XCD gets one CONTIGUOUS range of tiles (proportional to
// its workgroup count) and its workgroups sweep that range together; the
// halo rows neighbouring tiles share then hit the XCD's own L2.
struct TileIter {
  int first, stride, end;
  __device__ __forceinline__ TileIter(int ntiles, int xcd) {
    if (!(xcd & 1)) {
      first = blockIdx.x;
      stride = gridDim.x;
      end = ntiles;
      return;
    }
    const int G = gridDim.x, x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int gx = G / 8 + (x < G % 8 ? 1 : 0);
    const int before = x * (G / 8) + min(x, G % 8);
    const int lo = static_cast<int>(static_cast<int64_t>(ntiles) * before / G);
    end = static_cast<int>(static_cast<int64_t>(ntiles) * (before + gx) / G);
    first = lo + j;
    stride = gx;
  }
  __device__ __forceinline__ bool valid(int t) const { return t < end; }
  __device__ __forceinline__ int next(int t) const { return t + stride; }
};

// Bias of this lane's output channels (co0 = 16 h + 4 (lane >> 4)) into
// registers, bounced through LDS `scratch` (contains a barrier; scratch is
// free again after the caller's next barrier).  Loading them with a global
// load straight into the registers used inside the tile loop makes the
// compiler re-check vmcnt there, which (in-order counter) also waits for
// the next tile's prefetch.
template <int COUT>
__device__ __forceinline__ void bias_regs(const float* __restrict__ bias,
                                          float* scratch, float breg[COUT / 16][4]) {
  for (int e = threadIdx.x; e < COUT; e += blockDim.x) scratch[e] = bias[e];
  __syncthreads();
#pragma unroll
  for (int h = 0; h < COUT / 16; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) breg[h][i] = scratch[16 * h + 4 * (lane_id() >> 4) + i];
}

// Pre-pool conv outputs are stored in LDS as order-preserving 16-bit keys
// (bf16 bits with the magnitude bits of negatives flipped, so signed-int16
// order == float order).  The pooling then needs one v_and_or/v_lshl_or and
// one v_max_i32 per channel and tap: key32 = ord16 << 16 | (15 - tap code),
// so the max also yields the first maximal tap of the 3x3 window.
__device__ __forceinline__ uint32_t bf2_to_ord(uint32_t u) {
  return u ^ (((u >> 15) & 0x00010001u) * 0x7FFFu);
}

// Pre-pool LDS image y_s: order keys [Rc conv rows from cr0][W + 2][COUT],
// columns -1 and W are permanent pad columns holding kOrdMin keys (written
// once per kernel by init_pool_pads), and conv rows outside the image are
// stored as kOrdMin keys by the conv epilogue (store4_ord_in).  A pad key
// (0x8000 as int16) is below every real key (-inf is 0x807F), so the window
// max needs no bounds checks and the first maximal tap is unchanged.
constexpr uint32_t kOrdMin2 = 0x80008000u;

__device__ __forceinline__ void store4_ord_in(bf16_t* dst, const float v[4],
                                              bool in_image) {
  uint2 o;
  o.x = pack_bf16x2(v[0], v[1]);
  o.y = pack_bf16x2(v[2], v[3]);
  o.x = in_image ? bf2_to_ord(o.x) : kOrdMin2;
  o.y = in_image ? bf2_to_ord(o.y) : kOrdMin2;
  *reinterpret_cast<uint2*>(dst) = o;
}

template <int COUT>
__device__ __forceinline__ void init_pool_pads(bf16_t* y_s, int rows, int W) {
  constexpr int CH = COUT / 8;
  for (int e = threadIdx.x; e < rows * 2 * CH; e += blockDim.x) {
    const int part = e % CH, side = (e / CH) & 1, r = e / (2 * CH);
    *reinterpret_cast<uint4*>(y_s + (r * (W + 2) + (side ? W + 1 : 0)) * COUT +
                              part * 8) =
        make_uint4(kOrdMin2, kOrdMin2, kOrdMin2, kOrdMin2);
  }
}

// 3x3/2 max-pool (TF SAME padding offsets pb_h/pb_w) of the padded conv tile
// in y_s -> pooled bf16 + argmax code dy*3+dx, one 8-channel slice per
// thread.  key32 = ord16 << 16 | (15 - tap): one v_lshl_or / v_and_or and one
// v_max_i32 per channel and tap; the 9 taps are immediate-offset ds_read_b128
// from one base address.  The epilogue unpacks two channels per v_perm.
template <int COUT>
__device__ __forceinline__ void pool_tile(const bf16_t* y_s, int W, int Wo,
                                          int pb_w, int n, int Hp, int i0,
                                          int Rpv, bf16_t* __restrict__ pooled,
                                          uint8_t* __restrict__ argmax) {
  constexpr int CH = COUT / 8;
  const int Wt = W + 2;
  const int total = Rpv * Wo * CH;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int part = e % CH;
    const int pj = (e / CH) % Wo;
    const int pi = e / (CH * Wo);
    // window origin: local conv row 2 pi, padded column 2 pj - pb_w + 1
    const bf16_t* base = y_s + ((2 * pi) * Wt + 2 * pj - pb_w) * COUT + COUT + part * 8;
    int best[8];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + (dy * Wt + dx) * COUT);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
        const uint32_t K = 15 - (dy * 3 + dx);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int key = static_cast<int>((c & 1) ? ((u[c >> 1] & 0xFFFF0000u) | K)
                                                   : ((u[c >> 1] << 16) | K));
          best[c] = (dy | dx) ? max(best[c], key) : key;
        }
      }
    }
    const int64_t o = ((static_cast<int64_t>(n) * Hp + i0 + pi) * Wo + pj) * COUT + part * 8;
    uint32_t pv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)  // high halves of best[2k], best[2k+1]
      pv[k] = bf2_to_ord(__builtin_amdgcn_perm(static_cast<uint32_t>(best[2 * k + 1]),
                                               static_cast<uint32_t>(best[2 * k]),
                                               0x07060302u));
    *reinterpret_cast<uint4*>(pooled + o) = make_uint4(pv[0], pv[1], pv[2], pv[3]);
    uint32_t lo[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // low bytes (15 - tap) of best[4k..4k+3]
      const uint32_t a = __builtin_amdgcn_perm(static_cast<uint32_t>(best[4 * k + 1]),
                                               static_cast<uint32_t>(best[4 * k]),
                                               0x0c0c0400u);
      const uint32_t b = __builtin_amdgcn_perm(static_cast<uint32_t>(best[4 * k + 3]),
                                               static_cast<uint32_t>(best[4 * k + 2]),
                                               0x0c0c0400u);
      lo[k] = 0x0F0F0F0Fu - (a | (b << 16));
    }
    *reinterpret_cast<uint2*>(argmax + o) = make_uint2(lo[0], lo[1]);
  }
}

// Contiguous byte span [off, off+bytes) of `src` (16-B aligned) -> LDS.
template <int NREG>
struct SpanStager {
  uint4 v[NREG];
  int total;
  __device__ __forceinline__ void issue(const uint8_t* __restrict__ src,
                                        int64_t off, int bytes) {
    total = bytes / 16;
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const int e = threadIdx.x + k * kThreads;
      v[k] = make_uint4(0, 0, 0, 0);
      if (e < total) v[k] = *reinterpret_cast<const uint4*>(src + off + e * 16);
    }
  }
  __device__ __forceinline__ void commit(uint8_t* lds) const {
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const int e = threadIdx.x + k * kThreads;
      if (e < total) *reinterpret_cast<uint4*>(lds + e * 16) = v[k];
    }
  }
};

// dY of the conv feeding a max-pool as an LDS halo tile (rows [r_begin,
// r_begin+rows) x cols [-1, W], pitch row_pitch(COUT, W)), built per 2x2
// block of conv positions.  Block (i, j)
// holds conv rows 2i-pb_h+{0,1} x cols 2j-pb_w+{0,1}; its cells can only be
// the argmax of pooled windows (i,j), (i-1,j), (i,j-1), (i-1,j-1) (a window's
// dy/dx = 2 cells are the next block's offset-0 cells).  Each thread loads
// those 4 windows once and writes 4 cells:
//   (1,1) <- (i,j):4       (0,1) <- (i,j):1 + (i-1,j):7
//   (1,0) <- (i,j):3 + (i,j-1):5
//   (0,0) <- (i,j):0 + (i-1,j):6 + (i,j-1):2 + (i-1,j-1):8
// (window:code).  ~2x fewer VALU ops and 4x fewer LDS reads than checking
// every window of every cell.  Halo columns are zeroed separately.
template <int COUT>
__device__ __forceinline__ void gather_pool_grad_blocks(
    const bf16_t* p_s, const uint8_t* g_s, int i_lo, int i_hi, int W, int Wo,
    int pb_h, int pb_w, int r_begin, int rows, bf16_t* d_s) {
  constexpr int CH = COUT / 8;
  const int RPd = row_pitch(COUT, W);
  // halo columns -1 and W
  for (int e = threadIdx.x; e < rows * 2 * CH; e += blockDim.x) {
    const int part = e % CH;
    const int side = (e / CH) & 1;
    const int rr = e / (2 * CH);
    *reinterpret_cast<uint4*>(d_s + rr * RPd + (side ? W + 1 : 0) * COUT +
                              part * 8) = make_uint4(0, 0, 0, 0);
  }
  // blocks whose rows intersect [r_begin, r_begin + rows)
  const int t0 = r_begin + pb_h;
  const int ib0 = t0 >= 0 ? t0 / 2 : -((1 - t0) / 2);  // floor(t0 / 2)
  const int ib1 = (r_begin + rows - 1 + pb_h) / 2;
  const int nbr = ib1 - ib0 + 1;
  const int total = nbr * Wo * CH;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int part = e % CH;
    const int jb = (e / CH) % Wo;
    const int ib = ib0 + e / (CH * Wo);
    uint32_t cw[4][2];  // codes of windows (i,j), (i-1,j), (i,j-1), (i-1,j-1)
    uint32_t vw[4][4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int i = ib - (w & 1), j = jb - (w >> 1);
      if (i >= i_lo && i <= i_hi && j >= 0) {
        const int o = ((i - i_lo) * Wo + j) * COUT + part * 8;
        const uint2 c = *reinterpret_cast<const uint2*>(g_s + o);
        const uint4 v = *reinterpret_cast<const uint4*>(p_s + o);
        cw[w][0] = c.x; cw[w][1] = c.y;
        vw[w][0] = v.x; vw[w][1] = v.y; vw[w][2] = v.z; vw[w][3] = v.w;
      } else {
        cw[w][0] = cw[w][1] = 0xFFFFFFFFu;  // matches no code
        vw[w][0] = vw[w][1] = vw[w][2] = vw[w][3] = 0;
      }
    }
    float cell[4][8];  // (a,b) = (0,0), (0,1), (1,0), (1,1)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float v[4];
      int code[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const uint32_t u = vw[w][k >> 1];
        v[w] = __uint_as_float((k & 1) ? (u & 0xFFFF0000u) : (u << 16));
        code[w] = (cw[w][k >> 2] >> (8 * (k & 3))) & 0xFF;
      }
      cell[3][k] = code[0] == 4 ? v[0] : 0.f;
      cell[1][k] = (code[0] == 1 ? v[0] : 0.f) + (code[1] == 7 ? v[1] : 0.f);
      cell[2][k] = (code[0] == 3 ? v[0] : 0.f) + (code[2] == 5 ? v[2] : 0.f);
      cell[0][k] = (code[0] == 0 ? v[0] : 0.f) + (code[1] == 6 ? v[1] : 0.f) +
                   (code[2] == 2 ? v[2] : 0.f) + (code[3] == 8 ? v[3] : 0.f);
    }
#pragma unroll
    for (int cidx = 0; cidx < 4; ++cidx) {
      const int rr = 2 * ib - pb_h + (cidx >> 1) - r_begin;
      const int cc = 2 * jb - pb_w + (cidx & 1);
      if (rr >= 0 && rr < rows && cc >= 0 && cc < W) {
        uint4 o;
        o.x = pack_bf16x2(cell[cidx][0], cell[cidx][1]);
        o.y = pack_bf16x2(cell[cidx][2], cell[cidx][3]);
        o.z = pack_bf16x2(cell[cidx][4], cell[cidx][5]);
        o.w = pack_bf16x2(cell[cidx][6], cell[cidx][7]);
        *reinterpret_cast<uint4*>(d_s + rr * RPd + (cc + 1) * COUT + part * 8) = o;
      }
    }
  }
}

__host__ __device__ __forceinline__ void pooled_rows(int r_begin, int rows,
                                                     int pb_h, int Hp, int* lo,
                                                     int* hi) {
  const int a = r_begin + pb_h - 1;
  *lo = a < 0 ? 0 : a / 2;
  int h = (r_begin + rows - 1 + pb_h) / 2;
  *hi = h > Hp - 1 ? Hp - 1 : h;
}

// SA_ROWS_BALANCE=1: when a rule's tallest fitting tile R leaves a last tile
// of under R / 4 rows, the image's ceil(H / R) tiles are made equally tall
// (ceil(H / n) rows): the same number of tiles and staged halo rows without
// the sliver (Atari 21 rows: 7+7+7 instead of 10+10+1; 42 rows of the
// 16->32 head backward: 9+9+9+9+6 instead of 10+10+10+10+2).  Measured
// (bf16 learner, one box, 3 runs per arm): Atari 84x84x4 4.767-4.779 ->
// 4.714-4.731 ms with every tile balanced; balancing the IMPALA 18x24 maps
// too (8+8+2 -> 6+6+6) cost the 72x96 learner 0.02-0.04 ms, hence the R / 4
// threshold, which leaves every 72x96 tile unchanged.
#ifndef SA_ROWS_BALANCE
#define SA_ROWS_BALANCE 1
#endif
constexpr int balance_rows(int H, int R) {
  if (!SA_ROWS_BALANCE || R >= H || R < 1) return R;
  const int n = (H + R - 1) / R;
  const int last = H - (n - 1) * R;
  return 4 * last < R ? (H + n - 1) / n : R;
}

}  // namespace
}  // namespace conv
}  // namespace sa
