// The actor-inference heads + Gumbel-max sample of one row, shared by
// actor_head_sample_kernel (actor_io.hip) and the finisher of
// actor_core_step_kernel (actor_core.hip).  One 64-lane wave per row, no LDS,
// no barriers.
//
// Lane l holds x = h[4l..4l+3] and forms its 4-term partial dot product for
// every policy column and for value head 0.  The row sums are finished across
// the wave, lane a < A ends with logit a, draws u_a from Philox4x32-10
// (key = seed, counter = (row, a, offset)) and the action is
// argmax_a (logit_a - log(-log u_a)), the lower index winning ties.
//
// W is the accumulator width.  W = 32 (A <= 32): every column's partials run
// through the 6-step butterfly, so every lane ends with every logit (33
// accumulators, 198 exchanges).  W = 64 (A <= 63): a lane only needs its own
// logit, so the 64 columns are reduce-scattered by recursive halving: at step
// m = 32, 16, ..., 1 a lane keeps the half of its columns whose bit m equals
// its own lane bit m and adds its partner's (lane ^ m) partials of that half;
// 63 exchanges, and lane a is left with logit a.  Both forms add the 64 lane
// partials of a column as the same balanced tree over the lane bits 32 ... 1,
// so a column's sum does not depend on W; the baseline takes the plain 6-step
// butterfly in both.
//
// kUnitKv: the value weights are one head [256] (a 16-byte load per lane);
// otherwise [256, Kv] and head 0 is read with stride Kv.
#pragma once
#include "launchers.h"
#include "philox.h"

namespace sa {

constexpr int kActorMaxActions = 63;  // the learner heads' limit (A + 1 <= 64)

struct HeadSample {
  float logit;     // lane a < A: logit a (bias added)
  float baseline;  // every lane
  int action;      // every lane
};

template <int W, bool kUnitKv>
__device__ __forceinline__ HeadSample head_sample_row(
    const float4 x, const float* __restrict__ wp, const float* __restrict__ bp,
    const float* __restrict__ wb, const float* __restrict__ bb, int Kv,
    float* __restrict__ logits, int A, unsigned long long seed, unsigned long long offset,
    int row, int lane) {
  static_assert(W == 32 || W == 64, "accumulator width");
  const float* w0 = wp + (4 * lane) * A;
  float acc[W + 1];
#pragma unroll
  for (int a = 0; a < W; ++a)
    acc[a] = a < A ? x.x * w0[a] + x.y * w0[A + a] + x.z * w0[2 * A + a] +
                         x.w * w0[3 * A + a]
                   : 0.f;
  if constexpr (kUnitKv) {
    const float4 wv = reinterpret_cast<const float4*>(wb)[lane];
    acc[W] = x.x * wv.x + x.y * wv.y + x.z * wv.z + x.w * wv.w;
  } else {
    const float* v0 = wb + static_cast<int64_t>(4 * lane) * Kv;
    acc[W] = x.x * v0[0] + x.y * v0[Kv] + x.z * v0[2 * static_cast<int64_t>(Kv)] +
             x.w * v0[3 * static_cast<int64_t>(Kv)];
  }
  float mine = -INFINITY;
  if constexpr (W == 32) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int a = 0; a <= W; ++a)
        if (a < A || a == W) acc[a] += __shfl_xor(acc[a], m, 64);
    }
#pragma unroll
    for (int a = 0; a < W; ++a)
      if (a == lane) mine = acc[a];
  } else {
    // after step m, acc[j] (j < m) is column j + (lane & ~(m - 1) & 63)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const bool up = (lane & m) != 0;
#pragma unroll
      for (int j = 0; j < m; ++j) {
        const float keep = up ? acc[j + m] : acc[j];
        const float send = up ? acc[j] : acc[j + m];
        acc[j] = keep + __shfl_xor(send, m, 64);
      }
    }
    mine = acc[0];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[W] += __shfl_xor(acc[W], m, 64);
  }
  float key = -INFINITY;
  if (lane < A) {
    mine += bp[lane];
    logits[(int64_t)row * A + lane] = mine;
    const uint4 r = philox4x32_10(
        make_uint4((unsigned)row, (unsigned)lane, (unsigned)offset,
                   (unsigned)(offset >> 32)),
        make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const float u = ((r.x >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
    key = mine - __logf(-__logf(u));
  }
  int idx = lane;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ok = __shfl_xor(key, m, 64);
    const int oi = __shfl_xor(idx, m, 64);
    if (ok > key || (ok == key && oi < idx)) {
      key = ok;
      idx = oi;
    }
  }
  return {mine, acc[W] + bb[0], idx};
}

}  // namespace sa
