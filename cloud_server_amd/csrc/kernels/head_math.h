// The 10-way classifier head's maths, once: loss / dlogits / argmax conventions, the label
// lookup, the step bookkeeping and the row-logits block shared by the head kernels
// (head.hip, head_dgrad.h) and the evaluation kernels (eval.hip).  Device code only.
//
// Conventions (construct_distribute.py:285-298, :381-382): softmax cross-entropy
// ('entropy', loss == 0) has the row term lse - z[y] and dlogits (softmax - onehot) *
// grad_scale / M; 'mse' has the row term sum_j (z_j - onehot_j)^2 and dlogits
// (z - onehot) * 2 grad_scale / (10 M).  The prediction is the LOWEST class index attaining
// the max (tf.argmax).  Every helper keeps the summation order of the kernel that calls it:
// the lane-per-class epilogue takes its reducer as a parameter for that reason.
#pragma once
#include "common.h"

namespace csa {

constexpr int NCLS = 10;

__device__ __forceinline__ float xent_scale(float grad_scale, int M) { return grad_scale / (float)M; }
__device__ __forceinline__ float mse_scale(float grad_scale, int M) { return 2.f * grad_scale / (float)(M * NCLS); }
__device__ __forceinline__ float xent_dlogit(float z, float lse, bool hot, float inv) {
  return (__expf(z - lse) - (hot ? 1.f : 0.f)) * inv;
}

// One thread advances the device step counter and, when the step's batch is staged (its
// kernels no longer read the cursor), the batch stream's cursor (mod wrap).
__device__ __forceinline__ void head_advance(int64_t* step, int64_t* adv_cursor, long wrap) {
  *step += 1;
  if (adv_cursor) {
    const int64_t c = *adv_cursor + 1;
    *adv_cursor = (wrap > 0 && c >= wrap) ? 0 : c;
  }
}

// This step's rows of the batch index stream.
__device__ __forceinline__ const int64_t* head_rows(const int64_t* idx, const int64_t* cursor, int M) {
  return cursor ? idx + cursor[0] * M : idx;
}

// Label of batch row m: the staged labels[m] (idx null), or the dataset's through the stream.
__device__ __forceinline__ int head_label(const int64_t* labels, const int64_t* idx, const int64_t* cursor, int M,
                                          int m) {
  if (!idx) return (int)labels[m];
  return (int)labels[head_rows(idx, cursor, M)[m]];
}

// ---- one thread per batch row ----
// z[10] = logits + bias (registers or an LDS row).  Writes the row's dlogits to dl (which
// may be z itself), adds its loss term to ls and returns its prediction.
__device__ __forceinline__ int head_thread_epilogue(const float* z, float* dl, int y, int loss, float grad_scale,
                                                    int M, float& ls) {
  float mx = z[0];
  int am = 0;
#pragma unroll
  for (int j = 1; j < NCLS; ++j)
    if (z[j] > mx) { mx = z[j]; am = j; }
  if (loss == 0) {
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < NCLS; ++j) se += __expf(z[j] - mx);
    const float lse = mx + __logf(se);
    ls += lse - z[y];
    const float inv = xent_scale(grad_scale, M);
#pragma unroll
    for (int j = 0; j < NCLS; ++j) dl[j] = xent_dlogit(z[j], lse, j == y, inv);
  } else {
    const float inv = mse_scale(grad_scale, M);
#pragma unroll
    for (int j = 0; j < NCLS; ++j) {
      const float d = z[j] - (j == y ? 1.f : 0.f);
      ls += d * d;
      dl[j] = d * inv;
    }
  }
  return am;
}

// ---- one lane per class ----
// Where a row's ten classes live in the wave and how they are reduced: max / sum over the
// row's lanes and the lowest hit of a ballot among them.
struct Wave64Shfl {                      // lanes 0..9 of the wave, 64-lane shuffles
  static __device__ __forceinline__ float max(float v) { return wave_max(v); }
  static __device__ __forceinline__ float sum(float v) { return wave_sum(v); }
  static __device__ __forceinline__ int first(unsigned long long hit) { return __builtin_ctzll(hit); }
};
struct Row16Dpp {                        // lanes 0..9 of the wave, DPP inside their 16-lane row
  static __device__ __forceinline__ float max(float v) { return row16_max(v); }
  static __device__ __forceinline__ float sum(float v) { return row16_sum(v); }
  static __device__ __forceinline__ int first(unsigned long long hit) { return __builtin_ctzll(hit); }
};
struct Group16Shfl {                     // one row per 16-lane group, shuffles inside the group
  static __device__ __forceinline__ float max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  }
  static __device__ __forceinline__ float sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
  static __device__ __forceinline__ int first(unsigned long long hit) {
    const unsigned mine = (unsigned)(hit >> (threadIdx.x & 48)) & 0xffffu;
    return mine ? __builtin_ctz(mine) : 0;
  }
};

// The lane of class j (cls: this lane holds a class at all) has z = logit j + bias, every
// other lane of the row -inf.  Every lane of the wave must call (ballot / shuffles).  am
// and ls (the row's prediction and loss term) reach every lane of the row, d is this lane's
// dlogit; the caller decides what to store.
template <class R>
__device__ __forceinline__ void head_lane_epilogue(float z, bool cls, int j, int label, int loss, float grad_scale,
                                                   int M, int& am, float& d, float& ls) {
  const float mx = R::max(z);
  am = R::first(__ballot(cls && z == mx));
  float lterm = 0.f;
  d = 0.f;
  if (loss == 0) {
    const float e = cls ? __expf(z - mx) : 0.f;
    const float se = R::sum(e);
    const float lse = mx + __logf(se);
    if (cls) {
      d = xent_dlogit(z, lse, j == label, xent_scale(grad_scale, M));
      lterm = j == label ? lse - z : 0.f;
    }
  } else if (cls) {
    const float t = z - (j == label ? 1.f : 0.f);
    lterm = t * t;
    d = t * mse_scale(grad_scale, M);
  }
  ls = R::sum(lterm);
}

// ---- row logits of ONE batch row by a 256-thread workgroup (thread t: k = t + 256 u) ----
constexpr int HROW_T = 256;

// Every load first: this thread's h values and Wh rows, clamped addresses.
template <int KPT>
__device__ __forceinline__ void head_row_load(const float* h_row, const float* w, int K, float (&hv)[KPT],
                                              float (&wv)[KPT][NCLS]) {
#pragma unroll
  for (int u = 0; u < KPT; ++u) {
    const int k = min(u * HROW_T + (int)threadIdx.x, K - 1);
    hv[u] = h_row[k];
#pragma unroll
    for (int j = 0; j < NCLS; j += 2) {
      const float2 t = *reinterpret_cast<const float2*>(w + (long)k * NCLS + j);
      wv[u][j] = t.x; wv[u][j + 1] = t.y;
    }
  }
}

// hv becomes the post-activation value (0 past K); the ten partial logits of each wave go
// to s_part[wave].  The caller's barrier follows.
template <int KPT>
__device__ __forceinline__ void head_row_partials(float (&hv)[KPT], const float (&wv)[KPT][NCLS], int K, int in_act,
                                                  float in_alpha, float (*s_part)[NCLS]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[NCLS];
#pragma unroll
  for (int j = 0; j < NCLS; ++j) acc[j] = 0.f;
#pragma unroll
  for (int u = 0; u < KPT; ++u) {
    const bool ok = u * HROW_T + tid < K;
    hv[u] = ok ? act_fwd(hv[u], in_act, in_alpha) : 0.f;
#pragma unroll
    for (int j = 0; j < NCLS; ++j) acc[j] = fmaf(hv[u], wv[u][j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < NCLS; ++j) {
    const float t = wave_sum_dpp(acc[j]);
    if (lane == 0) s_part[wave][j] = t;
  }
}

// Lane j < 10: logit j + bias, the four waves folded in fixed order; -inf elsewhere.
__device__ __forceinline__ float head_row_fold(const float (*s_part)[NCLS], int lane, float bias) {
  float z = -INFINITY;
  if (lane < NCLS) z = s_part[0][lane] + s_part[1][lane] + s_part[2][lane] + s_part[3][lane] + bias;
  return z;
}

}  // namespace csa
