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
#include "head_sample.h"
#include "launchers.h"

namespace sa {
namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kH = 256;
constexpr int kNW = 8;       // waves per workgroup
constexpr int kNSMax = 20;   // MFMA k-steps per wave: (K + 256) / 4 / 8 <= 20
constexpr int kRows = 16;    // rows per tile

struct ActorCoreArgs {
  const float* h_aug;   // [R, ld]
  const uint8_t* done;  // [R]
  const float* c_in;    // [R, 256]
  const float* h_in;    // [R, 256]
  const float* wpk;     // [64][kp][16]: rows [0, K) of W_x, rows kh0.. of W_h
  const float* b_lstm;  // [1024]
  const float* wp;      // [256, A]
  const float* bp;      // [A]
  const float* wb;      // [256, Kv] (head 0 is read)
  const float* bb;      // [Kv]
  float* c2;            // [R, 256]
  float* h2;            // [R, 256]
  float* logits;        // [R, A]
  float* baseline;      // [R]
  int64_t* action;      // [R]
  unsigned* tickets;    // [row tiles], zero between launches
  unsigned long long* counter;  // nullptr or {offset, waves done}
  unsigned long long seed, offset;
  int R, ld, K, kh0, kp, A, Kv;
  // board epilogue (out == nullptr: none)
  const float* mask;    // [R]
  float* c;             // commit targets (may be c_in / h_in)
  float* h;
  uint32_t* out;
  int off_dw[5];        // action, logits, baseline, c, h
  int M, slot_dw, masked_only;
};

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// heads + Gumbel-max sample (+ board commit / packing) of one finished row
template <int W>
__device__ __forceinline__ void finish_row(const ActorCoreArgs& a, int row, int lane,
                                           unsigned long long offset) {
  const int A = a.A;
  const float4 x = reinterpret_cast<const float4*>(a.h2 + static_cast<int64_t>(row) * kH)[lane];
  const HeadSample hs = head_sample_row<W, false>(x, a.wp, a.bp, a.wb, a.bb, a.Kv, a.logits, A,
                                                  a.seed, offset, row, lane);
  const float mine = hs.logit, base = hs.baseline;
  const int idx = hs.action;
  if (lane == 0) {
    a.baseline[row] = base;
    a.action[row] = idx;
  }
  if (a.out == nullptr) return;
  // board epilogue of this row (board_epilogue_kernel's semantics)
  const bool keep = a.mask[row] > 0.f;
  const float4 cv = reinterpret_cast<const float4*>(a.c2 + static_cast<int64_t>(row) * kH)[lane];
  if (keep) {
    reinterpret_cast<float4*>(a.c + static_cast<int64_t>(row) * kH)[lane] = cv;
    reinterpret_cast<float4*>(a.h + static_cast<int64_t>(row) * kH)[lane] = x;
  }
  if (a.masked_only && !keep) return;  // uniform per wave
  const int s = row / a.M, m = row - s * a.M;
  uint32_t* dst = a.out + static_cast<int64_t>(s) * a.slot_dw;
  if (lane < 2) dst[a.off_dw[0] + m * 2 + lane] = lane == 0 ? static_cast<uint32_t>(idx) : 0u;
  if (lane < A) dst[a.off_dw[1] + m * A + lane] = __float_as_uint(mine);
  if (lane == 0) dst[a.off_dw[2] + m] = __float_as_uint(base);
  reinterpret_cast<float4*>(dst + a.off_dw[3] + m * kH)[lane] = cv;
  reinterpret_cast<float4*>(dst + a.off_dw[4] + m * kH)[lane] = x;
  if (a.masked_only) __threadfence_system();
}

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
    const float ekeep = edone ? 0.f : 1.f;
    const float i = sigm(g_s[er][eu * 4 + 0] + bi);
    const float g = tanhf(g_s[er][eu * 4 + 1] + bc);
    const float f = sigm(g_s[er][eu * 4 + 2] + bf + 1.0f);
    const float o = sigm(g_s[er][eu * 4 + 3] + bo);
    const float c = f * ekeep * cp + i * g;
    const int64_t hj = static_cast<int64_t>(egr) * kH + ej;
    a.c2[hj] = c;
    a.h2[hj] = o * tanhf(c);
  }
  // publish this workgroup's c2 / h2 slice and take a ticket of the row tile
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev = __hip_atomic_fetch_add(a.tickets + tile, 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // re-arm for the next launch (nobody else touches it in this one)
      __hip_atomic_store(a.tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last_s = last;
  }
  __syncthreads();
  if (!last_s) return;
  // ---- the row tile's last arriver: every c2 / h2 byte of the tile is
  // visible behind the acquire above
  unsigned long long offset = a.offset;
  if (a.counter != nullptr)
    offset = __hip_atomic_load(a.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int rr = wave; rr < kRows; rr += kNW) {
    const int row = r0 + rr;
    if (row < R) finish_row<W>(a, row, lane, offset);
  }
  // the sampler's counter pair {offset, waves done}: every finishing wave
  // counts itself after its sampling; the last one of the launch stores
  // offset + 1 and re-arms the count (actor_head_sample_kernel's protocol)
  if (a.counter != nullptr && lane == 0) {
    const unsigned long long waves = static_cast<unsigned long long>(gridDim.y) * kNW;
    const unsigned long long done = __hip_atomic_fetch_add(
        a.counter + 1, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (done == waves - 1) {
      __hip_atomic_store(a.counter, offset + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.counter + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
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
  ActorCoreArgs a{};
  a.h_aug = p.h_aug;
  a.done = p.done;
  a.c_in = p.c_in;
  a.h_in = p.h_in;
  a.wpk = p.wpk;
  a.b_lstm = p.b_lstm;
  a.wp = p.wp;
  a.bp = p.bp;
  a.wb = p.wb;
  a.bb = p.bb;
  a.c2 = p.c2;
  a.h2 = p.h2;
  a.logits = p.logits;
  a.baseline = p.baseline;
  a.action = p.action;
  a.tickets = p.tickets;
  a.counter = p.counter;
  a.seed = p.seed;
  a.offset = p.offset;
  a.R = p.R;
  a.ld = p.ld;
  a.K = p.K;
  a.kh0 = p.kmax;
  a.kp = p.kmax + kH;
  a.A = p.A;
  a.Kv = p.Kv;
  a.mask = p.mask;
  a.c = p.c;
  a.h = p.h;
  a.out = static_cast<uint32_t*>(p.out);
  for (int f = 0; f < 5; ++f) a.off_dw[f] = p.off_dw[f];
  a.M = p.M;
  a.slot_dw = p.slot_dw;
  a.masked_only = p.masked_only;
  auto kernel = p.A <= 32 ? actor_core_step_kernel<32> : actor_core_step_kernel<64>;
  hipLaunchKernelGGL(kernel, dim3(kH / 4, (p.R + kRows - 1) / kRows), dim3(64 * kNW), 0, stream,
                     a);
}

}  // namespace sa
