// Dropout (gfx950 / CDNA4): y = keep ? act(x) * s : 0, masks from the counter RNG.
//
// The reference feeds keep_prob = 0.5 on every training step and never applies it
// (construct_distribute.py:364-417; the tf.nn.dropout line is a comment).  Here the mask
// is a pure function of (seed, layer, step, element) -- ops/dropout_ref.py is the one
// definition -- so no mask tensor is stored: the backward redraws it.  Element (b, f) of a
// per-rank batch with F features draws crng(seed, step, (b * row_mul + row_add) * F + f):
// row_mul = world and row_add = rank give the element's place in the global batch.
//
// The forward reads the device step counter and records it in a word the unit owns; the
// backward reads that word, never the counter, which some lowerings advance between a
// layer's forward and its backward.  The tensors are tiny (50 x 512 floats in the flagship
// net), so both launches are latency-bound: one float4 per thread, no LDS, no atomics.
#include "common.h"
#include "crng.h"

// bit-parity of the unactivated forward with the NumPy reference: one multiply, unfused
#pragma clang fp contract(off)

namespace csa {

constexpr int DROP_THREADS = 256;

struct DropArgs {
  const float* x;            // the unit's input (pre-activation)
  const float* dy;           // backward only
  float* out;                // y (forward) or dx (backward)
  long n, F, row_mul, row_add;
  uint64_t seed;
  const long long* dstep;    // forward, train: the engine's step counter
  long long* used_step;      // written by the forward, read by the backward
  uint32_t T;                // keep iff (draw >> 8) < T
  float s;                   // float32(1 / keep_prob)
  int act; float alpha;
  int train;
  long n4;                   // float4 groups (0 when a pointer is not 16-byte aligned)
};

// the activation at full fp32 accuracy (the fast v_exp / v_rcp forms of common.h buy
// nothing in a latency-bound launch)
__device__ __forceinline__ float drop_act(float x, int act, float alpha) {
  switch (act) {
    case ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
    case ACT_RELU: return x > 0.f ? x : 0.f;
    case ACT_LEAKY: return fmaxf(x, alpha * x);
    default: return x;
  }
}

__device__ __forceinline__ bool drop_keep(const DropArgs& a, uint64_t step, long b, long f) {
  const uint64_t j = (uint64_t)((b * a.row_mul + a.row_add) * a.F + f);
  return (crng(a.seed, step, j) >> 8) < a.T;
}

template <bool BWD>
__device__ __forceinline__ float drop_one(const DropArgs& a, uint64_t step, long b, long f, float x, float g) {
  if (!BWD) {
    const float v = drop_act(x, a.act, a.alpha);
    if (!a.train) return v;
    return drop_keep(a, step, b, f) ? v * a.s : 0.f;
  }
  if (!drop_keep(a, step, b, f)) return 0.f;
  return act_bwd(g * a.s, x, drop_act(x, a.act, a.alpha), a.act, a.alpha);
}

template <bool BWD>
__global__ __launch_bounds__(DROP_THREADS) void drop_kernel(DropArgs a) {
  const long tid = (long)blockIdx.x * DROP_THREADS + threadIdx.x;
  const long nth = (long)gridDim.x * DROP_THREADS;
  uint64_t step = 0;
  if (BWD) {
    step = (uint64_t)*a.used_step & 0xFFFFFFFFull;
  } else if (a.train) {
    const long long d = *a.dstep;
    if (tid == 0) *a.used_step = d;
    step = (uint64_t)d & 0xFFFFFFFFull;
  }
  for (long i4 = tid; i4 < a.n4; i4 += nth) {
    const long e = 4 * i4;
    const float4 xv = reinterpret_cast<const float4*>(a.x)[i4];
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (BWD) gv = reinterpret_cast<const float4*>(a.dy)[i4];
    long b = e / a.F, f = e - b * a.F;
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
    float o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      o[u] = drop_one<BWD>(a, step, b, f, xs[u], gs[u]);
      if (++f == a.F) { f = 0; ++b; }
    }
    reinterpret_cast<float4*>(a.out)[i4] = make_float4(o[0], o[1], o[2], o[3]);
  }
  // scalar tail: n % 4 elements (all n when the float4 body is off)
  for (long e = 4 * a.n4 + tid; e < a.n; e += nth) {
    const long b = e / a.F, f = e - b * a.F;
    a.out[e] = drop_one<BWD>(a, step, b, f, a.x[e], BWD ? a.dy[e] : 0.f);
  }
}

static unsigned drop_grid(long n4, long n) {
  const long items = n4 > (n - 4 * n4) ? n4 : (n - 4 * n4);
  const long g = (items + DROP_THREADS - 1) / DROP_THREADS;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace csa

using namespace csa;

// y = drop(act(x)) over n elements, F features per batch row.  train = 1 draws the mask of
// step *dstep and records that step in *used_step; train = 0 writes act(x) and reads neither.
CSA_API int csa_drop_fwd(const float* x, float* y, long n, long F, long row_mul, long row_add, uint64_t seed,
                         const long long* dstep, long long* used_step, int T, float s, int act, float alpha,
                         int train, hipStream_t st) {
  if (n <= 0 || F <= 0 || n % F || row_mul < 1 || row_add < 0 || row_add >= row_mul || T < 1 || T > (1 << 24))
    return -1;
  if (train && (!dstep || !used_step)) return -2;
  const long n4 = (aligned16(x) && aligned16(y)) ? n >> 2 : 0;
  DropArgs a{x, nullptr, y, n, F, row_mul, row_add, seed, dstep, used_step, (uint32_t)T, s, act, alpha, train, n4};
  hipLaunchKernelGGL(drop_kernel<false>, dim3(drop_grid(n4, n)), dim3(DROP_THREADS), 0, st, a);
  return (int)hipGetLastError();
}

// dx = mask * s * act'(x) * dy with the mask of the step the forward recorded in *used_step.
CSA_API int csa_drop_bwd(const float* x, const float* dy, float* dx, long n, long F, long row_mul, long row_add,
                         uint64_t seed, const long long* used_step, int T, float s, int act, float alpha,
                         hipStream_t st) {
  if (n <= 0 || F <= 0 || n % F || row_mul < 1 || row_add < 0 || row_add >= row_mul || T < 1 || T > (1 << 24))
    return -1;
  if (!used_step) return -2;
  const long n4 = (aligned16(x) && aligned16(dy) && aligned16(dx)) ? n >> 2 : 0;
  DropArgs a{x, dy, dx, n, F, row_mul, row_add, seed, nullptr, const_cast<long long*>(used_step), (uint32_t)T, s,
             act, alpha, 1, n4};
  hipLaunchKernelGGL(drop_kernel<true>, dim3(drop_grid(n4, n)), dim3(DROP_THREADS), 0, st, a);
  return (int)hipGetLastError();
}
