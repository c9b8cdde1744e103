// Local response normalisation (gfx950 / CDNA4), fp32 NHWC: tf.nn.lrn and its gradient.
//
// The reference never builds one; the DSL's {"layer": "lrn"} lowers to a standalone unit over
// these launches.  Semantics, per pixel (a row of C channels; N = B * H * W rows), with the
// window W(c) = [max(0, c - r), min(C - 1, c + r)] clipped to the row (nothing is padded in):
//   s_c  = k + alpha * sum_{j in W(c)} x_j^2          (alpha is NOT divided by the window size)
//   y_c  = x_c * s_c^(-beta)
//   dx_c = dy_c * s_c^(-beta) - 2 alpha beta * x_c * sum_{j in W(c)} dy_j * y_j / s_j
// Every window sum adds its taps in ascending j, in every form, as the eager model's shifted
// adds do; products and sums are never contracted.  s^(-beta) is 1 / sqrtf(s) at beta = 0.5,
// 1 / s at beta = 1, 1 / (sqrtf(s) * sqrtf(sqrtf(s))) at beta = 0.75 and powf(s, -beta)
// otherwise (correctly rounded divisions and square roots; no fast intrinsics).
//
// The forward of a training program keeps s (one tensor): the backward then needs one
// s^(-beta) per element (form 2; per tap in form 1), where a recompute would need a
// (4r + 1)-wide window of x per element.  Forward-only programs pass keep = null and store
// nothing.
//
// The tensors are small (50 x 28 x 28 x 20 floats at most in the project's networks), so
// every launch is latency-bound.  Two forms each way:
//   form 1: one thread per element, or per four channels with 16-byte accesses when
//     C % 4 == 0 and every base is 16-byte aligned; the thread walks its clipped window
//     from global memory (L1-resident: a row is at most a few cache lines).
//   form 2: a row is loaded ONCE.  C <= 64: 64 / C consecutive rows share a wave, a lane per
//     element (one coalesced load), and the window sums come from min(2 min(r, C - 1) + 1, C)
//     cross-lane moves.  64 < C <= LRN_ROW_MAX: a wave per row stages it in its own LDS row
//     (the backward: the per-channel terms, one s^(-beta) per element) and every lane walks
//     its windows there.  Wider rows have no form 2.
// No atomics anywhere and a fixed summation order: run-to-run results are bitwise equal and
// deterministic mode runs the same kernels.  LDS is static: 16 KB forward, 48 KB backward.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace csa {

constexpr int LRN_THREADS = 256;
constexpr int LRN_WAVES = LRN_THREADS / 64;
constexpr int LRN_MAX_BLOCKS = 2048;        // grid cap; the kernels stride over the rest
constexpr long LRN_MAX_ELEMS = 1L << 30;    // x, y, keep are indexed with 32-bit ints
constexpr int LRN_ROW_MAX = 1024;           // widest row of form 2's LDS variant
// Windows of at least this many taps (2 min(r, C - 1) + 1) take form 2 when form = 0: every
// window, wherever form 2 exists.  Measured with scripts/lrn_cost.py on C = 8 .. 160 and
// r = 0 .. 63 (profiles/r18_notes.md): the backward in form 2 is never slower (3.0 against
// 7.0 us at the sample's 50 x 14 x 14 x 20, r = 5: form 1 pays one s^(-beta) per TAP); the
// forward in form 2 wins at every shape of the project's networks (3.1 against 4.0 us there)
// and loses by at most 16 % at 50 x 28 x 28 x 20 from r = 9 and at C = 160 from r = 14.
constexpr int LRN_WAVE_TAPS = 1;            // C <= 64: the cross-lane variant
constexpr int LRN_ROW_TAPS = 1;             // 64 < C <= LRN_ROW_MAX: the LDS-row variant
constexpr int LRN_NEVER = 0x7fffffff;

struct LrnGeom { int N, C, r; };
enum LrnPow : int { LRN_POW = 0, LRN_HALF = 1, LRN_ONE = 2, LRN_3Q = 3 };
struct LrnParam { float k, alpha, beta, coef; int mode; };   // coef = 2 alpha beta

// s^(-beta); s >= k > 0
__device__ __forceinline__ float lrn_pow(float s, const LrnParam& p) {
  switch (p.mode) {
    case LRN_HALF: return 1.0f / sqrtf(s);
    case LRN_ONE: return 1.0f / s;
    case LRN_3Q: { const float h = sqrtf(s); return 1.0f / (h * sqrtf(h)); }
    default: return powf(s, -p.beta);
  }
}

// the backward's per-channel term dy_j * y_j / s_j, from s^(-beta) = pw
__device__ __forceinline__ float lrn_term(float x, float dy, float s, float pw) { return (dy * (x * pw)) / s; }

__device__ __forceinline__ float lrn_dx(float g, float x, float sum, const LrnParam& p) {
  return g - (p.coef * x) * sum;              // g = dy * s^(-beta)
}

// ---------------------------------------------------------------- form 1, a thread per element
__global__ __launch_bounds__(LRN_THREADS) void lrn_fwd_thread_kernel(const float* __restrict__ x,
                                                                    float* __restrict__ y,
                                                                    float* __restrict__ keep, LrnGeom g,
                                                                    LrnParam p) {
  const int n = g.N * g.C, R = min(g.r, g.C - 1);
  for (int i = blockIdx.x * LRN_THREADS + threadIdx.x; i < n; i += gridDim.x * LRN_THREADS) {
    const int row = i / g.C, c = i - row * g.C;
    const float* xr = x + (i - c);
    const int lo = max(c - R, 0), hi = min(c + R, g.C - 1);
    float acc = 0.f;
    for (int j = lo; j <= hi; ++j) {
      const float v = xr[j];
      acc += v * v;
    }
    const float s = p.k + p.alpha * acc;
    if (keep) keep[i] = s;
    y[i] = xr[c] * lrn_pow(s, p);
  }
}

__global__ __launch_bounds__(LRN_THREADS) void lrn_bwd_thread_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ keep,
                                                                    const float* __restrict__ dy,
                                                                    float* __restrict__ dx, LrnGeom g, LrnParam p) {
  const int n = g.N * g.C, R = min(g.r, g.C - 1);
  for (int i = blockIdx.x * LRN_THREADS + threadIdx.x; i < n; i += gridDim.x * LRN_THREADS) {
    const int row = i / g.C, c = i - row * g.C;
    const int base = i - c;
    const int lo = max(c - R, 0), hi = min(c + R, g.C - 1);
    float acc = 0.f, own_g = 0.f, own_x = 0.f;
    for (int j = lo; j <= hi; ++j) {
      const float xv = x[base + j], gv = dy[base + j], sv = keep[base + j];
      const float pw = lrn_pow(sv, p);
      acc += lrn_term(xv, gv, sv, pw);
      if (j == c) {
        own_g = gv * pw;
        own_x = xv;
      }
    }
    dx[i] = lrn_dx(own_g, own_x, acc, p);
  }
}

// ---------------------------------------------------------------- form 1, four channels per thread
// C % 4 == 0 and 16-byte aligned bases: the thread owns channels c0 .. c0 + 3 and walks the
// float4s that cover the union of their windows; tap j enters channel c's sum when |j - c| <= R.
__device__ __forceinline__ float f4_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

__global__ __launch_bounds__(LRN_THREADS) void lrn_fwd_thread4_kernel(const float* __restrict__ x,
                                                                     float* __restrict__ y,
                                                                     float* __restrict__ keep, LrnGeom g,
                                                                     LrnParam p) {
  const int C4 = g.C >> 2, n = g.N * C4, R = min(g.r, g.C - 1);
  for (int i = blockIdx.x * LRN_THREADS + threadIdx.x; i < n; i += gridDim.x * LRN_THREADS) {
    const int row = i / C4, c0 = (i - row * C4) << 2;
    const float* xr = x + row * g.C;
    const int lo4 = max(c0 - R, 0) & ~3, hi = min(c0 + 3 + R, g.C - 1);     // (hi | 3) < C
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int jb = lo4; jb <= hi; jb += 4) {
      const float4 v = *reinterpret_cast<const float4*>(xr + jb);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = f4_get(v, e), sq = t * t;
        const int d = jb + e - c0;                 // tap - channel, for channel c0
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += (d - u >= -R && d - u <= R) ? sq : 0.f;
      }
    }
    const float4 own = *reinterpret_cast<const float4*>(xr + c0);
    float4 s, o;
    s.x = p.k + p.alpha * acc[0]; s.y = p.k + p.alpha * acc[1];
    s.z = p.k + p.alpha * acc[2]; s.w = p.k + p.alpha * acc[3];
    o.x = own.x * lrn_pow(s.x, p); o.y = own.y * lrn_pow(s.y, p);
    o.z = own.z * lrn_pow(s.z, p); o.w = own.w * lrn_pow(s.w, p);
    if (keep) *reinterpret_cast<float4*>(keep + (size_t)i * 4) = s;
    *reinterpret_cast<float4*>(y + (size_t)i * 4) = o;
  }
}

__global__ __launch_bounds__(LRN_THREADS) void lrn_bwd_thread4_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ keep,
                                                                     const float* __restrict__ dy,
                                                                     float* __restrict__ dx, LrnGeom g, LrnParam p) {
  const int C4 = g.C >> 2, n = g.N * C4, R = min(g.r, g.C - 1);
  for (int i = blockIdx.x * LRN_THREADS + threadIdx.x; i < n; i += gridDim.x * LRN_THREADS) {
    const int row = i / C4, c0 = (i - row * C4) << 2;
    const int base = row * g.C;
    const int lo4 = max(c0 - R, 0) & ~3, hi = min(c0 + 3 + R, g.C - 1);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, own_g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int jb = lo4; jb <= hi; jb += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(x + base + jb);
      const float4 gv = *reinterpret_cast<const float4*>(dy + base + jb);
      const float4 sv = *reinterpret_cast<const float4*>(keep + base + jb);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xe = f4_get(xv, e), ge = f4_get(gv, e), se = f4_get(sv, e);
        const float pw = lrn_pow(se, p);
        const float t = lrn_term(xe, ge, se, pw);
        const int d = jb + e - c0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[u] += (d - u >= -R && d - u <= R) ? t : 0.f;
          if (d == u) own_g[u] = ge * pw;
        }
      }
    }
    const float4 own = *reinterpret_cast<const float4*>(x + base + c0);
    float4 o;
    o.x = lrn_dx(own_g[0], own.x, acc[0], p); o.y = lrn_dx(own_g[1], own.y, acc[1], p);
    o.z = lrn_dx(own_g[2], own.z, acc[2], p); o.w = lrn_dx(own_g[3], own.w, acc[3], p);
    *reinterpret_cast<float4*>(dx + (size_t)i * 4) = o;
  }
}

// ---------------------------------------------------------------- form 2, C <= 64: rows share a wave
// Lane l of a wave holds element (row0 + l / C, l % C) of 64 / C consecutive rows: ONE
// contiguous load.  The sum over a lane's window: the lanes at distance d = -R .. R of the
// same row, in ascending d; a tap outside the row adds 0.
// Windows wider than the row (2R + 1 > C) visit the row's C channels by their index instead:
// C moves, the same taps in the same order.
__device__ __forceinline__ float lrn_window_lanes(float v, int lane, int c, int C, int R) {
  float acc = 0.f;
  if (2 * R + 1 <= C) {                            // (wave-uniform)
    for (int d = -R; d <= R; ++d) {
      const float t = __shfl(v, (lane + d) & 63, 64);
      acc += ((unsigned)(c + d) < (unsigned)C) ? t : 0.f;
    }
  } else {
    const int first = lane - c;                    // the row's channel 0
    for (int j = 0; j < C; ++j) {
      const float t = __shfl(v, (first + j) & 63, 64);
      acc += (j - c >= -R && j - c <= R) ? t : 0.f;
    }
  }
  return acc;
}

__global__ __launch_bounds__(LRN_THREADS) void lrn_fwd_wave_kernel(const float* __restrict__ x,
                                                                  float* __restrict__ y, float* __restrict__ keep,
                                                                  LrnGeom g, LrnParam p) {
  const int lane = threadIdx.x & 63, R = min(g.r, g.C - 1);
  const int per = 64 / g.C;                        // rows per wave
  const int pp = lane / g.C, c = lane - pp * g.C;
  const int ngroup = (g.N + per - 1) / per, nwave = gridDim.x * LRN_WAVES;
  for (int wv = (blockIdx.x * LRN_THREADS + threadIdx.x) >> 6; wv < ngroup; wv += nwave) {   // (wave-uniform)
    const int row = wv * per + pp;
    const bool on = pp < per && row < g.N;
    const int i = row * g.C + c;
    const float xv = on ? x[i] : 0.f;
    const float acc = lrn_window_lanes(xv * xv, lane, c, g.C, R);
    if (on) {
      const float s = p.k + p.alpha * acc;
      if (keep) keep[i] = s;
      y[i] = xv * lrn_pow(s, p);
    }
  }
}

__global__ __launch_bounds__(LRN_THREADS) void lrn_bwd_wave_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ keep,
                                                                  const float* __restrict__ dy,
                                                                  float* __restrict__ dx, LrnGeom g, LrnParam p) {
  const int lane = threadIdx.x & 63, R = min(g.r, g.C - 1);
  const int per = 64 / g.C;
  const int pp = lane / g.C, c = lane - pp * g.C;
  const int ngroup = (g.N + per - 1) / per, nwave = gridDim.x * LRN_WAVES;
  for (int wv = (blockIdx.x * LRN_THREADS + threadIdx.x) >> 6; wv < ngroup; wv += nwave) {
    const int row = wv * per + pp;
    const bool on = pp < per && row < g.N;
    const int i = row * g.C + c;
    float xv = 0.f, gv = 0.f, sv = 1.f;
    if (on) {
      xv = x[i];
      gv = dy[i];
      sv = keep[i];
    }
    const float pw = lrn_pow(sv, p);
    const float acc = lrn_window_lanes(lrn_term(xv, gv, sv, pw), lane, c, g.C, R);
    if (on) dx[i] = lrn_dx(gv * pw, xv, acc, p);
  }
}

// ---------------------------------------------------------------- form 2, 64 < C <= LRN_ROW_MAX: a wave per row
// Every wave of a workgroup runs the same number of passes (the barriers are workgroup-wide);
// a wave past the last row only waits.
__global__ __launch_bounds__(LRN_THREADS) void lrn_fwd_row_kernel(const float* __restrict__ x,
                                                                 float* __restrict__ y, float* __restrict__ keep,
                                                                 LrnGeom g, LrnParam p) {
  __shared__ float s_x[LRN_WAVES][LRN_ROW_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, R = min(g.r, g.C - 1);
  float* sx = s_x[w];
  for (int row0 = blockIdx.x * LRN_WAVES; row0 < g.N; row0 += gridDim.x * LRN_WAVES) {
    const int row = row0 + w;
    const bool on = row < g.N;
    const int base = row * g.C;
    if (on)
      for (int c = lane; c < g.C; c += 64) sx[c] = x[base + c];
    __syncthreads();
    if (on)
      for (int c = lane; c < g.C; c += 64) {
        const int lo = max(c - R, 0), hi = min(c + R, g.C - 1);
        float acc = 0.f;
        for (int j = lo; j <= hi; ++j) {
          const float v = sx[j];
          acc += v * v;
        }
        const float s = p.k + p.alpha * acc;
        if (keep) keep[base + c] = s;
        y[base + c] = sx[c] * lrn_pow(s, p);
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(LRN_THREADS) void lrn_bwd_row_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ keep,
                                                                 const float* __restrict__ dy,
                                                                 float* __restrict__ dx, LrnGeom g, LrnParam p) {
  __shared__ float s_t[LRN_WAVES][LRN_ROW_MAX];    // dy_j y_j / s_j
  __shared__ float s_g[LRN_WAVES][LRN_ROW_MAX];    // dy_j s_j^(-beta)
  __shared__ float s_x[LRN_WAVES][LRN_ROW_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, R = min(g.r, g.C - 1);
  float *st = s_t[w], *sg = s_g[w], *sx = s_x[w];
  for (int row0 = blockIdx.x * LRN_WAVES; row0 < g.N; row0 += gridDim.x * LRN_WAVES) {
    const int row = row0 + w;
    const bool on = row < g.N;
    const int base = row * g.C;
    if (on)
      for (int c = lane; c < g.C; c += 64) {
        const float xv = x[base + c], gv = dy[base + c], sv = keep[base + c];
        const float pw = lrn_pow(sv, p);
        st[c] = lrn_term(xv, gv, sv, pw);
        sg[c] = gv * pw;
        sx[c] = xv;
      }
    __syncthreads();
    if (on)
      for (int c = lane; c < g.C; c += 64) {
        const int lo = max(c - R, 0), hi = min(c + R, g.C - 1);
        float acc = 0.f;
        for (int j = lo; j <= hi; ++j) acc += st[j];
        dx[base + c] = lrn_dx(sg[c], sx[c], acc, p);
      }
    __syncthreads();
  }
}

static LrnGeom lrn_geom(const int* g) { return LrnGeom{g[0], g[1], g[2]}; }

// Everything the kernels handle: at least one row and one channel, a radius >= 0 (any: the
// window is clipped to the row), tensors of at most 2^30 elements (32-bit indices), a finite
// bias > 0 (so s > 0), a finite alpha >= 0 and a finite beta > 0.
static bool lrn_ok(const LrnGeom& g, float k, float alpha, float beta) {
  if (g.N < 1 || g.C < 1 || g.r < 0) return false;
  if ((long)g.N * g.C > LRN_MAX_ELEMS) return false;
  if (!isfinite(k) || !isfinite(alpha) || !isfinite(beta)) return false;
  return k > 0.f && alpha >= 0.f && beta > 0.f;
}

static LrnParam lrn_param(float k, float alpha, float beta) {
  const int mode = beta == 0.5f ? LRN_HALF : beta == 1.0f ? LRN_ONE : beta == 0.75f ? LRN_3Q : LRN_POW;
  return LrnParam{k, alpha, beta, 2.0f * alpha * beta, mode};
}

// The window size (2 min(r, C - 1) + 1 taps) from which form = 0 picks form 2 at C channels.
static int lrn_auto_taps(int C) {
  if (C > LRN_ROW_MAX) return LRN_NEVER;
  return C <= 64 ? LRN_WAVE_TAPS : LRN_ROW_TAPS;
}

static int lrn_pick(const LrnGeom& g, int form) {
  if (form != 0) return form;
  const int taps = 2 * (g.r < g.C - 1 ? g.r : g.C - 1) + 1;
  return taps >= lrn_auto_taps(g.C) ? 2 : 1;
}

static unsigned lrn_grid(long items) {
  const long n = (items + LRN_THREADS - 1) / LRN_THREADS;
  return (unsigned)(n < 1 ? 1 : (n > LRN_MAX_BLOCKS ? LRN_MAX_BLOCKS : n));
}

static unsigned lrn_grid2(const LrnGeom& g) {      // form 2: 64-lane items
  const long waves = g.C <= 64 ? ((long)g.N + 64 / g.C - 1) / (64 / g.C) : (long)g.N;
  return lrn_grid(waves * 64);
}

static bool lrn_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace csa

using namespace csa;

// g = {N = B * H * W, C, depth_radius}.  The refusal of csa_lrn_fwd / csa_lrn_bwd, asked at
// plan time (host only).
CSA_API int csa_lrn_ok(const int* g, float k, float alpha, float beta) {
  return g && lrn_ok(lrn_geom(g), k, alpha, beta) ? 1 : 0;
}

// The window size in taps from which form = 0 picks form 2 at C channels (INT_MAX: never).
CSA_API int csa_lrn_row_taps(int C) { return lrn_auto_taps(C); }

// The widest row form 2 takes.
CSA_API int csa_lrn_row_max() { return LRN_ROW_MAX; }

// y = x * s^(-beta), s = k + alpha * (window sum of x^2); keep (may be null) receives s.
// form: 0 = the host's choice, 1 = a thread per element / four channels, 2 = a row loaded once
// (refused for C > csa_lrn_row_max()).
CSA_API int csa_lrn_fwd(const float* x, float* y, float* keep, const int* g, float k, float alpha, float beta,
                        int form, hipStream_t st) {
  if (!x || !y || !g || form < 0 || form > 2) return -2;
  const LrnGeom q = lrn_geom(g);
  if (!lrn_ok(q, k, alpha, beta)) return -1;
  if (form == 2 && q.C > LRN_ROW_MAX) return -1;
  const LrnParam p = lrn_param(k, alpha, beta);
  const dim3 block(LRN_THREADS);
  if (lrn_pick(q, form) == 1) {
    const bool v4 = q.C % 4 == 0 && lrn_aligned16(x) && lrn_aligned16(y) && lrn_aligned16(keep);
    if (v4) hipLaunchKernelGGL(lrn_fwd_thread4_kernel, dim3(lrn_grid((long)q.N * (q.C / 4))), block, 0, st, x, y, keep, q, p);
    else hipLaunchKernelGGL(lrn_fwd_thread_kernel, dim3(lrn_grid((long)q.N * q.C)), block, 0, st, x, y, keep, q, p);
  } else if (q.C <= 64) {
    hipLaunchKernelGGL(lrn_fwd_wave_kernel, dim3(lrn_grid2(q)), block, 0, st, x, y, keep, q, p);
  } else {
    hipLaunchKernelGGL(lrn_fwd_row_kernel, dim3(lrn_grid2(q)), block, 0, st, x, y, keep, q, p);
  }
  return (int)hipGetLastError();
}

// keep = the forward's s.  Every element of dx is written.
CSA_API int csa_lrn_bwd(const float* x, const float* keep, const float* dy, float* dx, const int* g, float k,
                        float alpha, float beta, int form, hipStream_t st) {
  if (!x || !keep || !dy || !dx || !g || form < 0 || form > 2) return -2;
  const LrnGeom q = lrn_geom(g);
  if (!lrn_ok(q, k, alpha, beta)) return -1;
  if (form == 2 && q.C > LRN_ROW_MAX) return -1;
  const LrnParam p = lrn_param(k, alpha, beta);
  const dim3 block(LRN_THREADS);
  if (lrn_pick(q, form) == 1) {
    const bool v4 = q.C % 4 == 0 && lrn_aligned16(x) && lrn_aligned16(keep) && lrn_aligned16(dy) && lrn_aligned16(dx);
    if (v4) hipLaunchKernelGGL(lrn_bwd_thread4_kernel, dim3(lrn_grid((long)q.N * (q.C / 4))), block, 0, st, x, keep, dy, dx, q, p);
    else hipLaunchKernelGGL(lrn_bwd_thread_kernel, dim3(lrn_grid((long)q.N * q.C)), block, 0, st, x, keep, dy, dx, q, p);
  } else if (q.C <= 64) {
    hipLaunchKernelGGL(lrn_bwd_wave_kernel, dim3(lrn_grid2(q)), block, 0, st, x, keep, dy, dx, q, p);
  } else {
    hipLaunchKernelGGL(lrn_bwd_row_kernel, dim3(lrn_grid2(q)), block, 0, st, x, keep, dy, dx, q, p);
  }
  return (int)hipGetLastError();
}
