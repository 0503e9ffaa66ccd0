// Fused V-trace + IMPALA loss + analytic gradients on given
// logits and values: the unfused path of compute_loss (past 63 actions).
//
// Reference semantics: vtrace.py:71-280 (from_logits / from_importance_
// weights) and experiment.py:324-343, 377-407 (losses, reward clipping,
// discounts).  The reference runs V-trace on the CPU with a serial tf.scan;
// here the whole thing is ONE single-workgroup launch of the per-step
// functions of head_core.h (the fused head kernels run the same ones):
//
//   phase 1 (all T*B elements in parallel): vtrace_step;
//   phase 2 (per batch column, one wave): the reverse recursion as a
//            wave-level affine suffix scan over 64 lanes of time chunks;
//   phase 3 (parallel): loss_step without PopArt, then the block's sums.
// V-trace targets are stop-gradient, so the bootstrap value gets no gradient.
#include "head_core.h"
#include "launchers.h"

namespace sa {
namespace {

constexpr int kThreads = kHeadThreads;

__global__ __launch_bounds__(kThreads) void vtrace_loss_kernel(
    const float* __restrict__ behaviour, const float* __restrict__ target,
    const int64_t* __restrict__ actions, const float* __restrict__ rewards,
    const uint8_t* __restrict__ done, const float* __restrict__ values,
    const float* __restrict__ bootstrap, int T, int B, int A,
    float discounting, int clip_mode, float clip_rho, float clip_pg_rho,
    float baseline_cost, float entropy_cost, float* __restrict__ loss,
    float* __restrict__ dlogits, float* __restrict__ dvalues,
    float* __restrict__ vs_out, float* __restrict__ pg_adv_out,
    float* __restrict__ work) {
  const int N = T * B;
  float* w_a = work;            // gamma_t * c_t
  float* w_delta = work + N;    // delta_t
  float* w_pg = work + 2 * N;   // clipped pg rho
  float* w_vs = work + 3 * N;   // vs_t
  const int tid = threadIdx.x;

  // ---------------- phase 1
  for (int idx = tid; idx < N; idx += kThreads) {
    const int t = idx / B;
    const int b = idx - t * B;
    const VtraceStep s = vtrace_step(
        target + static_cast<int64_t>(idx) * A, behaviour + static_cast<int64_t>(idx) * A,
        A, static_cast<int>(actions[idx]), clip_reward(rewards[idx], clip_mode),
        done[idx] ? 0.f : discounting, values[idx],
        (t + 1 < T) ? values[idx + B] : bootstrap[b], clip_rho, clip_pg_rho);
    w_a[idx] = s.a;
    w_delta[idx] = s.delta;
    w_pg[idx] = s.pg_rho;
  }
  __syncthreads();

  // ---------------- phase 2: per-column reverse affine scan, one wave each
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int C = (T + 63) / 64;  // time steps per lane
  for (int b = wave; b < B; b += kHeadWaves) {
    const int t0 = lane * C;
    const int t1 = min(t0 + C, T);
    float ca = 1.f, cb = 0.f;  // acc_{t0} = cb + ca * acc_{t1}
    for (int t = t1 - 1; t >= t0; --t) {
      const float at = w_a[t * B + b];
      cb = w_delta[t * B + b] + at * cb;
      ca = at * ca;
    }
    wave_affine_suffix(ca, cb, lane);
    float acc = __shfl_down(cb, 1, 64);  // acc at this chunk's end
    if (lane == 63) acc = 0.f;
    for (int t = t1 - 1; t >= t0; --t) {
      acc = w_delta[t * B + b] + w_a[t * B + b] * acc;
      w_vs[t * B + b] = acc + values[t * B + b];
    }
  }
  __syncthreads();

  // ---------------- phase 3
  LossSums l;
  for (int idx = tid; idx < N; idx += kThreads) {
    const int t = idx / B;
    const int b = idx - t * B;
    const float v = values[idx];
    loss_step<true>(target + static_cast<int64_t>(idx) * A, A,
                    static_cast<int>(actions[idx]), v, v, w_vs[idx],
                    (t + 1 < T) ? w_vs[idx + B] : bootstrap[b], w_pg[idx],
                    clip_reward(rewards[idx], clip_mode), done[idx] ? 0.f : discounting,
                    0.f, 1.f, baseline_cost, entropy_cost, idx, dlogits, dvalues, vs_out,
                    pg_adv_out, l);
  }
  __shared__ float red[3][kHeadWaves];
  reduce_to_waves(l, red);
  if (tid == 0) write_loss(loss, sum_waves(red), baseline_cost, entropy_cost);
}

}  // namespace

void vtrace_loss_launch(const float* behaviour, const float* target,
                        const int64_t* actions, const float* rewards,
                        const uint8_t* done, const float* values,
                        const float* bootstrap, int T, int B, int A,
                        float discounting, int clip_mode, float clip_rho,
                        float clip_pg_rho, float baseline_cost,
                        float entropy_cost, float* loss, float* dlogits,
                        float* dvalues, float* vs_out, float* pg_adv_out,
                        float* work, hipStream_t stream) {
  hipLaunchKernelGGL(vtrace_loss_kernel, dim3(1), dim3(kThreads), 0, stream,
                     behaviour, target, actions, rewards, done, values,
                     bootstrap, T, B, A, discounting, clip_mode, clip_rho,
                     clip_pg_rho, baseline_cost, entropy_cost, loss, dlogits,
                     dvalues, vs_out, pg_adv_out, work);
}

}  // namespace sa
