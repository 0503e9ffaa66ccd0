// Actor inference core step in ONE launch (exact fp32, T = 1): the
// x-projection, the LSTM-256 step with done-reset, the policy / baseline
// heads, the Gumbel-max sample and (optionally) the inference board's masked
// state commit + slot-major output packing.  Replaces, after the torso-FC
// GEMM, the x-projection GEMM + its split-K reduce + lstm_fwd_step_kernel +
// actor_head_sample_kernel + board_epilogue_kernel.
//
//   gates = h_aug[:, :K] W_x[:K] + b + (keep h_in) W_h      keep = !done
//   c2 = f (keep c_in) + i g ; h2 = o tanh(c2)   (TF order i, c~, f, o; forget
//                                                 bias +1: lstm.hip)
//   logits = h2 Wp + bp ; baseline = h2 Wb[:, 0] + bb[0]
//   action = argmax_a (logits_a - log(-log u_a)), u from Philox4x32-10 with
//            counter (row, a, offset), key = seed (actor_io.hip)
//
// Grid = 64 column groups x 16-row tiles, 8 waves.  A workgroup owns 4 hidden
// units (16 gate columns, packed n = 4 u + g) of one row tile; the K + 256
// deep product runs on the exact-fp32 MFMA with both operands loaded straight
// from global (all loads issued up front), K split across the waves in
// contiguous step ranges and reduced once through LDS in wave order.
//
// No workgroup waits for another.  Each workgroup stores its slice of c2 / h2,
// publishes it (every wave drains its stores, barrier, one lane: agent-scope
// release, drain, relaxed ticket add) and leaves; the workgroup that draws
// the row tile's last ticket acquires (agent scope, one lane, drain, barrier)
// and finishes the tile: one wave per row recomputes nothing of the LSTM, it
// reads the row's complete h2 and forms the heads exactly as
// actor_head_sample_kernel does (head_sample.h: lane-local 4-term partials,
// butterfly for A <= 32, reduce-scatter for 33..63), so
// the sums have one fixed order and there are no per-workgroup head partials
// to re-read (they would be 64 x 16 x (A + 1) floats per tile against the
// 16 KB of h2 the finisher needs anyway for the packing).  The ticket words
// live in a zero-initialised device tensor and are re-armed by the last
// arriver, as is the sampler's {offset, waves done} pair: the launch replays
// from captured graphs.
//
// h_in is every workgroup's A operand, so h2 is a distinct buffer.  The
// board's commit target may be h_in / c_in themselves: the finisher writes a
// tile's rows only after every reader of those rows has taken its ticket.
#include "actor_core_tail.h"

namespace sa {
namespace {

using namespace actor_core;  // ActorCoreArgs, the gate math, the tail

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kNW = 8;       // waves per workgroup
constexpr int kNSMax = 20;   // MFMA k-steps per wave: (K + 256) / 4 / 8 <= 20

// W: the finisher's head accumulator width (32: A <= 32, 64: A <= 63); the
// launcher picks the instance, nothing before the finisher depends on it
template <int W>
__global__ __launch_bounds__(64 * kNW) void actor_core_step_kernel(ActorCoreArgs a) {
  __shared__ f4v red[kNW][64];
  __shared__ float g_s[kRows][17];
  __shared__ int last_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int blk = blockIdx.x;   // 4 hidden units
  const int tile = blockIdx.y;  // 16 rows
  const int r0 = tile * kRows;
  const int R = a.R, K = a.K;
  // gate-thread operands (thread = (row er, unit eu) for tid < 64), issued
  // up front from clamped addresses and consumed in the epilogue (lstm.hip)
  const int er = tid >> 2, eu = tid & 3;
  const int egr = r0 + er;
  const int ej = blk * 4 + eu;
  float bi = 0.f, bc = 0.f, bf = 0.f, bo = 0.f, cp = 0.f;
  uint32_t edone = static_cast<uint32_t>(R);
  if (tid < 4 * kRows) {
    const int egc = egr < R ? egr : R - 1;
    bi = a.b_lstm[ej];
    bc = a.b_lstm[kH + ej];
    bf = a.b_lstm[2 * kH + ej];
    bo = a.b_lstm[3 * kH + ej];
    cp = a.c_in[static_cast<int64_t>(egc) * kH + ej];
    edone = a.done[egc];
  }
  // A[row = r0 + (l&15)][k], B[k][n = l&15], k = 4 s + (l>>4) over the
  // concatenated [h_aug[:, :K] | keep h_in]; wave w owns steps [w nspw, ...)
  const int nsteps = (K + kH) >> 2;
  const int nspw = (nsteps + kNW - 1) / kNW;
  const int s0 = wave * nspw;
  const int arow = r0 + (lane & 15);
  const int arc = arow < R ? arow : R - 1;
  const int kq = lane >> 4;
  const uint32_t adone = a.done[arc];
  const float* xa = a.h_aug + static_cast<int64_t>(arc) * a.ld;
  const float* ha = a.h_in + static_cast<int64_t>(arc) * kH;
  const float* wsrc = a.wpk + static_cast<int64_t>(blk) * a.kp * 16 + (lane & 15);
  float av[kNSMax], bv[kNSMax];
#pragma unroll
  for (int j = 0; j < kNSMax; ++j) {
    const int s = s0 + j;
    // steps past this wave's range reload step 0 (a valid address) and are
    // zeroed below: every load is unconditional
    const int k = (j < nspw && s < nsteps) ? 4 * s + kq : kq;
    const bool inx = k < K;
    const float* ap = inx ? xa + k : ha + (k - K);
    const int kk = inx ? k : a.kh0 + (k - K);
    av[j] = *ap;
    bv[j] = wsrc[kk * 16];
  }
  f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kNSMax; ++j) {
    const int s = s0 + j;
    const bool ok = j < nspw && s < nsteps;
    const bool hpart = 4 * s + kq >= K;
    const float v = (!ok || (hpart && adone)) ? 0.f : av[j];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v, bv[j], acc, 0, 0, 0);
  }
  red[wave][lane] = acc;
  __syncthreads();
  // D[m = 4 (l>>4) + i][n = l&15]; fixed wave order
  if (tid < 16 * kRows) {
    const int m = tid >> 4, n = tid & 15;
    const int src_lane = ((m >> 2) << 4) | n;
    const int i = m & 3;
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < kNW; ++w) sum += red[w][src_lane][i];
    g_s[m][n] = sum;
  }
  __syncthreads();
  if (tid < 4 * kRows && egr < R) {
    lstm_cell_store(a, static_cast<int64_t>(egr) * kH + ej, g_s[er][eu * 4 + 0],
                    g_s[er][eu * 4 + 1], g_s[er][eu * 4 + 2], g_s[er][eu * 4 + 3], bi, bc, bf,
                    bo, cp, edone);
  }
  // publish this workgroup's c2 / h2 slice and take a ticket of the row tile
  // (the tile's last arriver finishes its rows: actor_core_tail.h)
  publish_and_finish<W, kNW>(a, tile, &last_s);
}

// lstm_kernel [f_in + 256, 1024] -> the step kernel's B operand
// [64 unit groups][kp = kmax + 256][4 units][4 gates]: rows [0, f_in) are
// W_x, rows [f_in, kmax) zero (K padding), rows [kmax, kp) are W_h.  The
// forward layout of lstm_pack_weights_kernel (w4) extended by the x rows; no
// backward packing.
__global__ __launch_bounds__(256) void actor_core_pack_kernel(
    const float* __restrict__ w, float* __restrict__ wpk, int f_in, int kmax) {
  const int kp = kmax + kH;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kp * 4 * kH) return;
  const int k = idx / (4 * kH), n = idx - k * 4 * kH;
  float v = 0.f;
  if (k < f_in)
    v = w[static_cast<int64_t>(k) * 4 * kH + n];
  else if (k >= kmax)
    v = w[static_cast<int64_t>(f_in + k - kmax) * 4 * kH + n];
  const int g = n / kH, u = n - g * kH;
  wpk[((static_cast<int64_t>(u >> 2) * kp + k) * 4 + (u & 3)) * 4 + g] = v;
}

}  // namespace

int actor_core_max_k() { return kNSMax * kNW * 4 - kH; }

void actor_core_pack_launch(const float* w, float* wpk, int f_in, int kmax, hipStream_t stream) {
  const int n = (kmax + kH) * 4 * kH;
  hipLaunchKernelGGL(actor_core_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, w,
                     wpk, f_in, kmax);
}

void actor_core_step_launch(const ActorCoreStep& p, hipStream_t stream) {
  if (p.R <= 0) return;
  const ActorCoreArgs a = make_args(p);
  auto kernel = p.A <= 32 ? actor_core_step_kernel<32> : actor_core_step_kernel<64>;
  hipLaunchKernelGGL(kernel, dim3(kH / 4, (p.R + kRows - 1) / kRows), dim3(64 * kNW), 0, stream,
                     a);
}

}  // namespace sa
