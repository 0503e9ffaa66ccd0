// The V-trace / IMPALA-loss column core shared by the learner head kernels:
// learner_head_fwd and learner_head_fwd_tiled (learner_io.hip) run every
// phase below, vtrace_loss (vtrace_loss.hip, the unfused path) runs the step
// terms, the wave scan, the loss terms and the wave reduction on logits and
// values it is handed.  One definition each (the one legacy rounding
// difference is a template flag of loss_step).  Everything is forced inline:
// pointers into LDS keep their address space at the call site.
// The phases of one batch column (vtrace.py:71-280, experiment.py:324-407)
// are described at their functions, the LDS layouts at their structs.
#pragma once
#include "launchers.h"

namespace sa {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kHeadThreads = 1024;
constexpr int kHeadWaves = kHeadThreads / 64;
// PopArt sigma bounds (popart.py SIGMA_MIN / SIGMA_MAX)
constexpr float kPopArtSigmaMin = 1e-4f;
constexpr float kPopArtSigmaMax = 1e6f;

__device__ __forceinline__ float clip_reward(float r, int mode) {
  if (mode == 0) return fminf(fmaxf(r, -1.f), 1.f);       // abs_one
  const float sq = tanhf(r / 5.0f);                         // soft_asymmetric
  return (r < 0.f ? 0.3f * sq : sq) * 5.0f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------ LDS layouts
// The dynamic LDS of the two head kernels in 4-byte words: the kernel carves
// its arrays from the offsets, the host sizes the launch by `total`.
struct LdsCursor {
  int at = 0;
  __host__ __device__ int take(int words) {
    const int o = at;
    at += words;
    return o;
  }
};

// W image [256][MAXC] with its 4 x 16 words of k-quarter skew (HeadImage)
__host__ __device__ constexpr int head_image_words(int maxc) { return 256 * maxc + 64; }

// learner_head_fwd: the whole column of T steps
struct HeadLds {
  int w, lv, beh, a, d, p, vs, r, act, disc, total;
  __host__ __device__ HeadLds(int maxc, int T, int A) {
    LdsCursor c;
    w = c.take(head_image_words(maxc));
    lv = c.take((T + 1) * (A + 1));  // [T+1][A+1]: logits then value
    beh = c.take(T * A);             // [T][A] behaviour logits
    a = c.take(T);                   // gamma_t c_t
    d = c.take(T);                   // delta_t
    p = c.take(T);                   // clipped pg rho
    vs = c.take(T + 1);              // vs_t, vs[T] = bootstrap
    r = c.take(T);                   // clipped reward
    act = c.take(T);                 // action (int)
    disc = c.take(T);                // gamma_t (0 at done)
    total = c.at;
  }
};

// learner_head_fwd_tiled: one time tile of TC steps
struct HeadTiledLds {
  int w, lv, beh, a, d, p, r, act, disc, vs, slack, total;
  __host__ __device__ HeadTiledLds(int maxc, int TC, int A) {
    LdsCursor c;
    w = c.take(head_image_words(maxc));
    lv = c.take((TC + 1) * (A + 1));  // rows c0 .. c1 of the tile
    beh = c.take(TC * A);
    a = c.take(TC);
    d = c.take(TC);
    p = c.take(TC);
    r = c.take(TC);
    act = c.take(TC);
    disc = c.take(TC);
    vs = c.take(TC + 1);              // vs_t, vs[n] = vs_{c1}
    // unused: keeps the footprint at 8 TC words past behaviour, the size
    // learner_head_tile_auto's tiles (and so every tiled result) were fixed at
    slack = c.take(TC - 1);
    total = c.at;
  }
};

// ------------------------------------------------------- column statistics
// The column's value head kt and its PopArt statistics (identity without).
// A task id outside [0, K) reads head 0 (no out-of-bounds access) with a NaN
// sigma: the column's gradients turn NaN and the RMSProp step guard drops
// the update (counted in skipped_updates) instead of training on it.
struct ColumnStats {
  int kt;
  float sig, mu, rsig;
};

__device__ __forceinline__ ColumnStats column_stats(const HeadTasks& tk, int b) {
  const int64_t kt_raw = tk.task != nullptr ? tk.task[b] : 0;
  const bool kt_bad = kt_raw < 0 || kt_raw >= tk.K;
  ColumnStats s;
  s.kt = kt_bad ? 0 : static_cast<int>(kt_raw);
  s.sig = 1.f;
  s.mu = 0.f;
  if (tk.mu != nullptr) {
    s.mu = tk.mu[s.kt];
    const float var = fmaxf(tk.nu[s.kt] - s.mu * s.mu, kPopArtSigmaMin * kPopArtSigmaMin);
    s.sig = fminf(fmaxf(sqrtf(var), kPopArtSigmaMin), kPopArtSigmaMax);
  }
  if (kt_bad) s.sig = __builtin_nanf("");
  s.rsig = 1.f / s.sig;
  return s;
}

// ------------------------------------------------------------------ heads
// [16 rows x 256] x [256 x MAXC] per wave on fp32 MFMA (16x16x4).  W = [Wp |
// Wb[:, kt] | 0] is staged once per column: (k, c) at k MAXC + 16 (k / 64) +
// c, so the 4 k-quarters of a wave's B operand reads land 16 banks apart.
// Lane l = (arow = l & 15, kq = l >> 4) holds the A operand of row arow for
// k in [64 kq, +64) as float4 k-steps and receives D[row 4 kq + i][col arow].
template <int MAXC>
struct HeadImage {
  static constexpr int H = 256;
  static constexpr int NCT = MAXC / 16;                // 16-wide column tiles
  static constexpr int WPT = H * MAXC / kHeadThreads;  // W words per thread

  // load / store are split: a kernel can put other loads in flight between
  static __device__ __forceinline__ void load(float (&wv)[WPT], float (&bias)[NCT],
                                              const float* __restrict__ wp,
                                              const float* __restrict__ wb,
                                              const float* __restrict__ bp,
                                              const float* __restrict__ bb, int A, int K,
                                              int kt) {
    const int tid = threadIdx.x, arow = tid & 15;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int c = 16 * ct + arow;
      bias[ct] = c < A ? bp[c] : (c == A ? bb[kt] : 0.f);
    }
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int i = tid + j * kHeadThreads;
      const int k = i / MAXC, c = i - k * MAXC;
      wv[j] = c < A ? wp[k * A + c] : (c == A ? wb[k * K + kt] : 0.f);
    }
  }

  static __device__ __forceinline__ void store(float* w_s, const float (&wv)[WPT]) {
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int i = threadIdx.x + j * kHeadThreads;
      w_s[i + 16 * ((i / MAXC) >> 6)] = wv[j];
    }
  }

  static __device__ __forceinline__ void zero(f4v (&acc)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f4v{0.f, 0.f, 0.f, 0.f};
  }

  // acc += x (one float4 k-step of this lane's A operand) x W rows k .. k + 3,
  // wk = w_s + (64 kq + k) MAXC + 16 kq + arow.  By value, the k-step loop in
  // the kernel: an array reference here splits the A loads into 16 branches.
  static __device__ __forceinline__ void mac4(f4v (&acc)[NCT], float4 x, const float* wk) {
    const float av[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], wk[q * MAXC + 16 * ct],
                                                       acc[ct], 0, 0, 0);
    }
  }

  // rows [row0, row0 + 16) below `rows`, columns below A1, into lv_s [.][A1]
  static __device__ __forceinline__ void write(float* lv_s, const f4v (&acc)[NCT],
                                               const float (&bias)[NCT], int row0,
                                               int rows, int A1) {
    const int lane = threadIdx.x & 63, arow = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int c = 16 * ct + arow;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 4 * kq + i;
        if (row < rows && c < A1) lv_s[row * A1 + c] = acc[ct][i] + bias[ct];
      }
    }
  }
};

// ------------------------------------------------------------ V-trace step
// vtrace.py:143-147, 235-262: two log-softmax gathers at the action, rho,
// then a_t = gamma_t min(1, rho), delta_t = min(clip_rho, rho) (r + gamma_t
// v_{t+1} - v_t) and the clipped pg rho.  zt / zb: target / behaviour
// logits [A]; r the clipped reward; disc = gamma_t; v, v1 de-normalised.
struct VtraceStep {
  float a, delta, pg_rho;
};

__device__ __forceinline__ VtraceStep vtrace_step(const float* zt, const float* zb, int A,
                                                  int a, float r, float disc, float v,
                                                  float v1, float clip_rho,
                                                  float clip_pg_rho) {
  float mt = -INFINITY, mb = -INFINITY;
  for (int j = 0; j < A; ++j) {
    mt = fmaxf(mt, zt[j]);
    mb = fmaxf(mb, zb[j]);
  }
  float st = 0.f, sb = 0.f;
  for (int j = 0; j < A; ++j) {
    st += __expf(zt[j] - mt);
    sb += __expf(zb[j] - mb);
  }
  const float log_pi = zt[a] - mt - __logf(st);
  const float log_mu = zb[a] - mb - __logf(sb);
  const float rho = __expf(log_pi - log_mu);
  VtraceStep s;
  s.a = disc * fminf(1.0f, rho);
  s.delta = fminf(clip_rho, rho) * (r + disc * v1 - v);
  s.pg_rho = fminf(clip_pg_rho, rho);
  return s;
}

// ------------------------------------------------------ affine suffix scan
// Lane l holds the map acc -> cb + ca acc of its steps; afterwards it holds
// the inclusive suffix composition f_l o f_{l+1} o ... o f_63 of its wave.
__device__ __forceinline__ void wave_affine_suffix(float& ca, float& cb, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float na = __shfl_down(ca, d, 64);
    const float nb = __shfl_down(cb, d, 64);
    if (lane + d < 64) {
      cb = cb + ca * nb;
      ca = ca * na;
    }
  }
}

// The workgroup scan: scan_a / scan_b [kHeadThreads] hold every thread's wave
// suffix.  acc entering this thread's steps from the right, given the acc
// entering the workgroup's last step: the later waves' totals, then the next
// lane's inclusive suffix in this wave.
__device__ __forceinline__ float enter_from_right(const float* scan_a, const float* scan_b,
                                                  float acc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int w = kHeadWaves - 1; w > wave; --w) acc = scan_b[w * 64] + scan_a[w * 64] * acc;
  if (lane < 63) acc = scan_b[tid + 1] + scan_a[tid + 1] * acc;
  return acc;
}

// -------------------------------------------------------------- loss terms
// One step's policy-gradient advantage, loss terms and analytic gradients:
//   dL/dz = (softmax - onehot) pg_adv + entropy_cost p (log p + H),
//   dL/dn = -baseline_cost err.
// PopArt: advantages in normalised units, baseline error against the
// normalised target; n the head's output, v = sig n + mu, vs / vs1 the
// V-trace targets of the step and the next (mu = 0, rsig = 1, v = n: the
// plain IMPALA loss, bitwise).  The targets are stop-gradient.  Outputs at
// element idx of [T, B]; vs_out / pg_adv_out may be null.
struct LossSums {
  float pg = 0.f, bl = 0.f, ent = 0.f;
};

template <bool kFuseErr>
__device__ __forceinline__ void loss_step(const float* zt, int A, int a, float n, float v,
                                          float vs, float vs1, float pg_rho, float r,
                                          float disc, float mu, float rsig,
                                          float baseline_cost, float entropy_cost,
                                          int64_t idx, float* dlogits, float* dvalues,
                                          float* vs_out, float* pg_adv_out, LossSums& l) {
  float* dz = dlogits + idx * A;
  const float pg_adv = pg_rho * (r + disc * vs1 - v) * rsig;
  // Legacy difference, kept bit for bit: left to the compiler's contraction,
  // the whole-column kernel rounded the error once (fused) and the tiled one
  // twice.  They differ in the last bit under PopArt only (rsig = 1: exact
  // either way); kFuseErr spells out each caller's form.
  float err;
  if (kFuseErr) {
    err = fmaf(vs - mu, rsig, -n);
  } else {
#pragma clang fp contract(off)
    err = (vs - mu) * rsig - n;
  }
  if (vs_out != nullptr) vs_out[idx] = vs;
  float m = -INFINITY;
  for (int j = 0; j < A; ++j) m = fmaxf(m, zt[j]);
  float s = 0.f;
  for (int j = 0; j < A; ++j) s += __expf(zt[j] - m);
  const float lse = m + __logf(s);
  float Hn = 0.f;
  for (int j = 0; j < A; ++j) {
    const float lp = zt[j] - lse;
    Hn -= __expf(lp) * lp;
  }
  for (int j = 0; j < A; ++j) {
    const float lp = zt[j] - lse;
    const float p = __expf(lp);
    dz[j] = (p - (j == a ? 1.f : 0.f)) * pg_adv + entropy_cost * p * (lp + Hn);
  }
  dvalues[idx] = -baseline_cost * err;
  if (pg_adv_out != nullptr) pg_adv_out[idx] = pg_adv;
  l.pg += (lse - zt[a]) * pg_adv;
  l.bl += 0.5f * err * err;
  l.ent -= Hn;
}

// ------------------------------------------------------------- loss finish
// Every thread's sums -> one value per wave in red; ends with a barrier.
__device__ __forceinline__ void reduce_to_waves(LossSums l, float (*red)[kHeadWaves]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  l.pg = wave_sum(l.pg);
  l.bl = wave_sum(l.bl);
  l.ent = wave_sum(l.ent);
  if (lane == 0) {
    red[0][wave] = l.pg;
    red[1][wave] = l.bl;
    red[2][wave] = l.ent;
  }
  __syncthreads();
}

__device__ __forceinline__ LossSums sum_waves(const float (*red)[kHeadWaves]) {
  LossSums s;
  for (int w = 0; w < kHeadWaves; ++w) {
    s.pg += red[0][w];
    s.bl += red[1][w];
    s.ent += red[2][w];
  }
  return s;
}

__device__ __forceinline__ void write_loss(float* loss, LossSums s, float baseline_cost,
                                           float entropy_cost) {
  loss[1] = s.pg;
  loss[2] = s.bl;
  loss[3] = s.ent;
  loss[0] = s.pg + baseline_cost * s.bl + entropy_cost * s.ent;
}

// One thread per workgroup: publish column b's sums write-through (sc1), wait
// for them, then take a ticket; true for the last workgroup to arrive, which
// reads the partials with sc1 loads after its add returned - no L2
// write-back / invalidate fences (MI355X_MICROARCH.md, inter-workgroup
// visibility, the one-lane sc1 hand-off).
__device__ __forceinline__ bool publish_column(float* partial, unsigned* ticket, int b,
                                               LossSums s) {
  __hip_atomic_store(partial + b * 3 + 0, s.pg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(partial + b * 3 + 1, s.bl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(partial + b * 3 + 2, s.ent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  return prev == static_cast<unsigned>(gridDim.x) - 1;
}

// The last workgroup's thread: all B columns in a fixed order (deterministic),
// the four loss sums, and the ticket re-armed for the next launch.
__device__ __forceinline__ void total_loss(const float* partial, unsigned* ticket, int B,
                                           float baseline_cost, float entropy_cost,
                                           float* loss) {
  LossSums s;
  for (int j = 0; j < B; ++j) {
    s.pg += __hip_atomic_load(partial + j * 3 + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s.bl += __hip_atomic_load(partial + j * 3 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s.ent += __hip_atomic_load(partial + j * 3 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  write_loss(loss, s, baseline_cost, entropy_cost);
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace sa
