// What the one-launch actor core steps share (actor_core.hip: exact fp32,
// actor_core_bf16.hip: bf16 MFMA operands): the kernel arguments, the gate
// math, and the tail - a workgroup publishes its slice of c2 / h2 and takes a
// ticket of its row tile; the tile's last arriver forms the heads, samples
// and (board) commits + packs.  The protocol is described in actor_core.hip.
#pragma once
#include "head_sample.h"
#include "launchers.h"

namespace sa {
namespace actor_core {

constexpr int kH = 256;
constexpr int kRows = 16;  // rows per tile

struct ActorCoreArgs {
  const float* h_aug;   // [R, ld]
  const uint8_t* done;  // [R]
  const float* c_in;    // [R, 256]
  const float* h_in;    // [R, 256]
  const float* wpk;     // fp32: [64][kp][16]: rows [0, K) of W_x, rows kh0.. of W_h
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
  const uint4* wpk16;   // bf16: [64][(kh0 + 256) / 32][64 lanes] x 8 bf16
};

// kh0: the packed row of W_h's first row (the W_x rows before it are padded)
inline ActorCoreArgs make_args(const ActorCoreStep& p) {
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
  return a;
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// One unit of one row: gate pre-activations without bias (TF order i, c~, f,
// o; forget bias +1), cp = c_in (ignored on a done row) -> c2 / h2 stored.
__device__ __forceinline__ void lstm_cell_store(const ActorCoreArgs& a, int64_t hj, float gi,
                                                float gc, float gf, float go, float bi,
                                                float bc, float bf, float bo, float cp,
                                                uint32_t done) {
  const float ekeep = done ? 0.f : 1.f;
  const float i = sigm(gi + bi);
  const float g = tanhf(gc + bc);
  const float f = sigm(gf + bf + 1.0f);
  const float o = sigm(go + bo);
  const float c = f * ekeep * cp + i * g;
  a.c2[hj] = c;
  a.h2[hj] = o * tanhf(c);
}

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

// Called by every thread of a workgroup of NW waves after its c2 / h2 stores:
// publishes the slice, takes a ticket of row tile `tile` (gridDim.x tickets
// per tile) and, in the tile's last arriver only, finishes the tile's rows.
// last_s: one shared int.
template <int W, int NW>
__device__ __forceinline__ void publish_and_finish(const ActorCoreArgs& a, int tile,
                                                   int* last_s) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r0 = tile * kRows;
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
    *last_s = last;
  }
  __syncthreads();
  if (!*last_s) return;
  // ---- the row tile's last arriver: every c2 / h2 byte of the tile is
  // visible behind the acquire above
  unsigned long long offset = a.offset;
  if (a.counter != nullptr)
    offset = __hip_atomic_load(a.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int rr = wave; rr < kRows; rr += NW) {
    const int row = r0 + rr;
    if (row < a.R) finish_row<W>(a, row, lane, offset);
  }
  // the sampler's counter pair {offset, waves done}: every finishing wave
  // counts itself after its sampling; the last one of the launch stores
  // offset + 1 and re-arms the count (actor_head_sample_kernel's protocol)
  if (a.counter != nullptr && lane == 0) {
    const unsigned long long waves = static_cast<unsigned long long>(gridDim.y) * NW;
    const unsigned long long done = __hip_atomic_fetch_add(
        a.counter + 1, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (done == waves - 1) {
      __hip_atomic_store(a.counter, offset + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.counter + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace actor_core
}  // namespace sa
