// Actor inference core step in ONE launch on the bf16 MFMA (T = 1): what
// actor_core_step_kernel (actor_core.hip) does, with the K + 256 deep gate
// product on v_mfma_f32_16x16x32_bf16.  Replaces, after the torso-FC GEMM of a
// bf16 inference step, the x-projection GEMM + its split-K reduce +
// lstm_fwd_step_kernel + actor_head_sample_kernel + board_epilogue_kernel.
//
//   gates = bf16(h_aug[:, :K]) bf16(W_x[:K]) + b + bf16(keep ? h_in : 0) bf16(W_h)
//   c2 = f (keep c_in) + i g ; h2 = o tanh(c2)   (TF order i, c~, f, o; forget
//                                                 bias +1: lstm.hip)
//   heads, sample, board epilogue: actor_core_tail.h, on the fp32 h2
//
// Rounding points:
//   * h_aug[:, :K] and keep ? h_in : 0 are rounded to bf16 (RNE) once, when
//     they are loaded; keep is a select, so a done row's old state (whatever
//     it holds) never enters the sum.
//   * W_x[:K] and W_h are rounded to bf16 (RNE) once, by the pack kernel.
//   * The products are accumulated in fp32: in the MFMA along a wave's
//     k-steps, then the 4 K-parts of a column in part order.
//   * Bias, gate math, c_in, c2, h2, the heads and the sample stay fp32.
// This is the rounding of the learner's bf16 gang recurrence (lstm_gang.hip),
// not that of the bf16 `ops` inference step, whose lstm_fwd_step_kernel takes
// h_in W_h in exact fp32: the two inference paths are close, not bitwise.
//
// K padding: the packed weights hold W_x in kmax rows (a multiple of 32, zero
// rows past f_in) followed by W_h.  A step reads kpad = K rounded up to 32
// rows of them; its A-operand elements at k >= K are zero in registers and
// are never loaded (ld may exceed K and the storage past K may hold
// anything), so the W_x rows in [K, kpad) - instruction rows when the step
// has no instruction - meet zeros.
//
// Grid = 32 column groups x 16-row tiles, 8 waves.  A workgroup owns 8 hidden
// units (32 gate columns, packed n = 4 u + g: two MFMA column blocks) of one
// row tile.  Wave w = (column block w & 1, K-part w >> 1): the kpad / 32 + 8
// <= 20 k-steps are split into 4 contiguous parts of <= 5, both operands come
// straight from global (all loads issued up front; B is one 16-byte load per
// lane and step, 1 KB contiguous per wave) and the parts are reduced once
// through LDS in part order.  128 threads then run the gate math.
//
// The tail is the fp32 kernel's (actor_core_tail.h): no workgroup waits for
// another, the tile's last arriver (of 32) finishes it, tickets and the
// sampler's pair are re-armed for graph replay, the commit target may alias
// c_in / h_in.
#include "actor_core_tail.h"

namespace sa {
namespace {

using namespace actor_core;

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

constexpr int kNW = 8;     // waves per workgroup
constexpr int kCB = 2;     // MFMA column blocks (4 units each) per workgroup
constexpr int kParts = kNW / kCB;
constexpr int kNSMax = 5;  // k-steps per wave: (kpad / 32 + 8) / 4 <= 5
constexpr int kUnits = 4 * kCB;

// two floats -> packed bf16 pair, RNE (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2v{lo, hi}, bf2v));
}

template <int W>
__global__ __launch_bounds__(64 * kNW) void actor_core_bf16_step_kernel(ActorCoreArgs a) {
  __shared__ f4v red[kNW][64];
  __shared__ float g_s[kRows][16 * kCB + 1];
  __shared__ int last_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int blk = blockIdx.x;   // 8 hidden units
  const int tile = blockIdx.y;  // 16 rows
  const int r0 = tile * kRows;
  const int R = a.R, K = a.K;
  // gate-thread operands (thread = (row er, unit eu) for tid < 128), issued
  // up front from clamped addresses and consumed in the epilogue
  const int er = tid / kUnits, eu = tid % kUnits;
  const int egr = r0 + er;
  const int ej = blk * kUnits + eu;
  float bi = 0.f, bc = 0.f, bf = 0.f, bo = 0.f, cp = 0.f;
  uint32_t edone = 1u;
  if (tid < kUnits * kRows) {
    const int egc = egr < R ? egr : R - 1;
    bi = a.b_lstm[ej];
    bc = a.b_lstm[kH + ej];
    bf = a.b_lstm[2 * kH + ej];
    bo = a.b_lstm[3 * kH + ej];
    cp = a.c_in[static_cast<int64_t>(egc) * kH + ej];
    edone = a.done[egc];
  }
  // A[row = r0 + (l&15)][k], B[k][n = l&15], k = 32 s + 8 (l>>4) + j over
  // [h_aug[:, :K], 0 to kpad | keep ? h_in : 0]: steps [0, nsx) are x steps,
  // [nsx, nsx + 8) h steps; this wave owns [s0, s0 + nspw) of them
  const int cb = wave % kCB, part = wave / kCB;
  const int nsx = (K + 31) >> 5;
  const int nsteps = nsx + kH / 32;
  const int nspw = (nsteps + kParts - 1) / kParts;
  const int s0 = part * nspw;
  const int arow = r0 + (lane & 15);
  const int arc = arow < R ? arow : R - 1;
  const int kq = lane >> 4;
  const uint32_t adone = a.done[arc];
  const float* xa = a.h_aug + static_cast<int64_t>(arc) * a.ld;
  const float* ha = a.h_in + static_cast<int64_t>(arc) * kH + 8 * kq;
  const int nst_pk = a.kp >> 5;  // packed k-steps of one column group
  const uint4* wsrc = a.wpk16 + static_cast<int64_t>(blk * kCB + cb) * nst_pk * 64 + lane;
  float av[kNSMax][8];
  uint4 bv[kNSMax];
#pragma unroll
  for (int j = 0; j < kNSMax; ++j) {
    // steps past this wave's range reload step 0 (valid addresses) and are
    // skipped below
    const int s = (j < nspw && s0 + j < nsteps) ? s0 + j : 0;
    if (s < nsx) {  // uniform per wave
      const int k0 = 32 * s + 8 * kq;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        const float v = xa[k < K ? k : K - 1];
        av[j][e] = k < K ? v : 0.f;
      }
      bv[j] = wsrc[s * 64];
    } else {
      const int hs = s - nsx;
      const float4 lo = *reinterpret_cast<const float4*>(ha + 32 * hs);
      const float4 hi = *reinterpret_cast<const float4*>(ha + 32 * hs + 4);
      av[j][0] = lo.x; av[j][1] = lo.y; av[j][2] = lo.z; av[j][3] = lo.w;
      av[j][4] = hi.x; av[j][5] = hi.y; av[j][6] = hi.z; av[j][7] = hi.w;
#pragma unroll
      for (int e = 0; e < 8; ++e) av[j][e] = adone ? 0.f : av[j][e];
      bv[j] = wsrc[((a.kh0 >> 5) + hs) * 64];
    }
  }
  f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kNSMax; ++j) {
    if (j < nspw && s0 + j < nsteps) {  // uniform per wave
      const u4v ap = {pack2(av[j][0], av[j][1]), pack2(av[j][2], av[j][3]),
                      pack2(av[j][4], av[j][5]), pack2(av[j][6], av[j][7])};
      const u4v bp = {bv[j].x, bv[j].y, bv[j].z, bv[j].w};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, ap),
                                                    __builtin_bit_cast(bf8v, bp), acc, 0, 0, 0);
    }
  }
  red[wave][lane] = acc;
  __syncthreads();
  // D[m = 4 (l>>4) + i][n = l&15] of column block cb; fixed part order
  {
    const int m = tid / (16 * kCB), n2 = tid % (16 * kCB);
    const int rcb = n2 >> 4, n = n2 & 15;
    const int src_lane = ((m >> 2) << 4) | n;
    const int i = m & 3;
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < kParts; ++p) sum += red[p * kCB + rcb][src_lane][i];
    g_s[m][n2] = sum;
  }
  __syncthreads();
  if (tid < kUnits * kRows && egr < R) {
    lstm_cell_store(a, static_cast<int64_t>(egr) * kH + ej, g_s[er][eu * 4 + 0],
                    g_s[er][eu * 4 + 1], g_s[er][eu * 4 + 2], g_s[er][eu * 4 + 3], bi, bc, bf,
                    bo, cp, edone);
  }
  // publish this workgroup's c2 / h2 slice and take a ticket of the row tile
  publish_and_finish<W, kNW>(a, tile, &last_s);
}

// lstm_kernel [f_in + 256, 1024] fp32 -> the step kernel's B operand in bf16
// (RNE): [64 column groups of 4 units][(kmax + 256) / 32 k-steps][64 lanes][8],
// lane l of step s holding packed rows k = 32 s + 8 (l>>4) + j, j = 0..7, of
// column n = l & 15 = 4 (u & 3) + g.  Packed rows [0, f_in) are W_x, rows
// [f_in, kmax) zero, rows [kmax, kmax + 256) W_h.  One thread per 16-byte
// fragment.
__global__ __launch_bounds__(256) void actor_core_bf16_pack_kernel(
    const float* __restrict__ w, uint4* __restrict__ wpk16, int f_in, int kmax) {
  const int nst = (kmax + kH) >> 5;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 64 * nst * 64) return;
  const int l = idx & 63, s = (idx >> 6) % nst, cg = (idx >> 6) / nst;
  const int n = l & 15;
  const int col = (n & 3) * kH + cg * 4 + (n >> 2);  // gate g, unit u
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 32 * s + 8 * (l >> 4) + j;
    v[j] = 0.f;
    if (k < f_in)
      v[j] = w[static_cast<int64_t>(k) * 4 * kH + col];
    else if (k >= kmax)
      v[j] = w[static_cast<int64_t>(f_in + k - kmax) * 4 * kH + col];
  }
  wpk16[idx] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]),
                          pack2(v[6], v[7]));
}

}  // namespace

int actor_core_bf16_max_k() { return (kNSMax * kParts - kH / 32) * 32; }

ActorCoreBf16Info actor_core_bf16_info(int R, int K, int A) {
  ActorCoreBf16Info i{};
  i.grid_x = kH / kUnits;
  i.grid_y = (R + kRows - 1) / kRows;
  i.kpad = (K + 31) / 32 * 32;
  i.ksteps = i.kpad / 32 + kH / 32;
  i.width = A <= 32 ? 32 : 64;
  return i;
}

void actor_core_bf16_pack_launch(const float* w, uint16_t* wpk16, int f_in, int kmax,
                                 hipStream_t stream) {
  const int n = 64 * ((kmax + kH) / 32) * 64;
  hipLaunchKernelGGL(actor_core_bf16_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, w,
                     reinterpret_cast<uint4*>(wpk16), f_in, kmax);
}

void actor_core_bf16_step_launch(const ActorCoreStep& p, const uint16_t* wpk16,
                                 hipStream_t stream) {
  if (p.R <= 0) return;
  ActorCoreArgs a = make_args(p);
  a.wpk16 = reinterpret_cast<const uint4*>(wpk16);
  const ActorCoreBf16Info i = actor_core_bf16_info(p.R, p.K, p.A);
  auto kernel = i.width == 32 ? actor_core_bf16_step_kernel<32> : actor_core_bf16_step_kernel<64>;
  hipLaunchKernelGGL(kernel, dim3(i.grid_x, i.grid_y), dim3(64 * kNW), 0, stream, a);
}

}  // namespace sa
