// Average pooling (gfx950 / CDNA4), fp32 NHWC: tf.nn.avg_pool and its gradient.
//
// The reference only ever builds tf.nn.max_pool (construct_distribute.py:121-130); the DSL's
// {"layer": "pool", "mode": "avg"} and "kernel": "global" lower to a standalone unit over
// these launches.  Semantics: an output is the sum of its window's IN-IMAGE taps, in (dy, dx)
// row-major order, divided (a true division) by the number of in-image taps, so SAME padding
// enters neither the sum nor the divisor; the backward gives an input pixel the sum, over the
// windows that contain it in (oy, ox) order, of dy[o] / n_o, and 0 where no window covers it.
// Adds and divisions only: there is nothing to contract.
//
// The tensors are small (50 x 28 x 28 x 20 floats at most in the project's networks), so every
// launch is latency-bound: few, wide instructions and no avoidable index arithmetic.
//   forward, form 1 (small windows): one thread per output element, or per four channels with
//     16-byte loads and stores; the (b, oy, ox, c) split once per element, the window clipped
//     to the image once, the divisor from the clipped range.
//   forward, form 2 (large windows; global pooling always): one wave per (b, oy, ox).  The
//     lanes cover contiguous NHWC runs of (tap, channel) -- 64 / C taps per load instruction
//     -- each lane sums its taps in order, and the lanes of one channel fold through a fixed
//     shuffle tree; one division and one store per channel.
//   backward: gather form, one thread per input element (or four channels), over the windows
//     [oy0..oy1] x [ox0..ox1] that cover it; every input element is written.
// No atomics anywhere: run-to-run results are bitwise equal, deterministic mode runs the same
// kernels.  Geometry layout: the PoolGeom of norm_pool.hip.
#include "common.h"

#pragma clang fp contract(off)

namespace csa {

constexpr int AP_THREADS = 256;
constexpr int AP_MAX_BLOCKS = 2048;        // grid cap; the kernels stride over the rest
constexpr long AP_MAX_ELEMS = 1L << 30;    // x and y are indexed with 32-bit ints
// Windows of at least this many positions take form 2.  Measured on [50, 14, 14, 20]
// (profiles/r17_notes.md): form 1 wins at 4 x 4 (3.49 against 3.92 us), form 2 from 5 x 5 on
// (4.11 against 4.37 us; 3.2 against 23.7 us at the 196 positions of a global pool).
constexpr int AP_WAVE_TAPS = 25;

struct AvgGeom { int B, H, W, C, kh, kw, sh, sw, pt, pl, OH, OW; };

template <int V> struct ApVec;
template <> struct ApVec<1> {
  float v;
  __device__ __forceinline__ static ApVec zero() { return {0.f}; }
  __device__ __forceinline__ static ApVec load(const float* p) { return {*p}; }
  __device__ __forceinline__ void store(float* p) const { *p = v; }
  __device__ __forceinline__ void add(const ApVec& o) { v += o.v; }
  __device__ __forceinline__ void add_div(const ApVec& o, float n) { v += o.v / n; }
  __device__ __forceinline__ ApVec div(float n) const { return {v / n}; }
  __device__ __forceinline__ ApVec from_lane(int src) const { return {__shfl(v, src, 64)}; }
};
template <> struct ApVec<4> {
  float4 v;
  __device__ __forceinline__ static ApVec zero() { return {make_float4(0.f, 0.f, 0.f, 0.f)}; }
  __device__ __forceinline__ static ApVec load(const float* p) { return {*reinterpret_cast<const float4*>(p)}; }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ void add(const ApVec& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
  __device__ __forceinline__ void add_div(const ApVec& o, float n) {
    v.x += o.v.x / n; v.y += o.v.y / n; v.z += o.v.z / n; v.w += o.v.w / n;
  }
  __device__ __forceinline__ ApVec div(float n) const { return {make_float4(v.x / n, v.y / n, v.z / n, v.w / n)}; }
  __device__ __forceinline__ ApVec from_lane(int src) const {
    return {make_float4(__shfl(v.x, src, 64), __shfl(v.y, src, 64), __shfl(v.z, src, 64), __shfl(v.w, src, 64))};
  }
};

// ---------------------------------------------------------------- forward, form 1
template <int V>
__global__ __launch_bounds__(AP_THREADS) void avgpool_fwd_thread_kernel(const float* __restrict__ x,
                                                                       float* __restrict__ y, AvgGeom g) {
  using T = ApVec<V>;
  const int CV = g.C / V;                          // channel groups of V
  const int n = g.B * g.OH * g.OW * CV;
  const int row_stride = g.W * g.C;
  for (int i = blockIdx.x * AP_THREADS + threadIdx.x; i < n; i += gridDim.x * AP_THREADS) {
    int r = i / CV;
    const int cg = i - r * CV;
    const int q = r / g.OW;
    const int ox = r - q * g.OW;
    const int b = q / g.OH;
    const int oy = q - b * g.OH;
    // the window clipped to the image: [y0, y1) x [x0, x1), never empty (avgpool_ok)
    const int ys = oy * g.sh - g.pt, xs = ox * g.sw - g.pl;
    const int y0 = max(ys, 0), y1 = min(ys + g.kh, g.H);
    const int x0 = max(xs, 0), x1 = min(xs + g.kw, g.W);
    const float* row = x + ((b * g.H + y0) * g.W + x0) * g.C + cg * V;
    T acc = T::zero();
    for (int yy = y0; yy < y1; ++yy, row += row_stride) {
      const float* p = row;
      for (int xx = x0; xx < x1; ++xx, p += g.C) acc.add(T::load(p));
    }
    acc.div((float)((y1 - y0) * (x1 - x0))).store(y + (size_t)i * V);
  }
}

// ---------------------------------------------------------------- forward, form 2
template <int V>
__global__ __launch_bounds__(AP_THREADS) void avgpool_fwd_wave_kernel(const float* __restrict__ x,
                                                                     float* __restrict__ y, AvgGeom g) {
  using T = ApVec<V>;
  const int lane = threadIdx.x & 63;
  const int CV = g.C / V;
  const int cw = CV < 64 ? CV : 64;                // channel groups the wave covers at a time
  const int per = 64 / cw;                         // taps per load instruction
  const int j = lane / cw, c = lane - j * cw;      // this lane's tap slot (idle: j >= per) and channel group
  int P = 1;                                       // fold tree width: per rounded up to a power of two
  while (P < per) P <<= 1;
  const int npos = g.B * g.OH * g.OW;
  const int nwave = gridDim.x * (AP_THREADS / 64);
  for (int o = (blockIdx.x * AP_THREADS + threadIdx.x) >> 6; o < npos; o += nwave) {     // (wave-uniform)
    const int q = o / g.OW;
    const int ox = o - q * g.OW;
    const int b = q / g.OH;
    const int oy = q - b * g.OH;
    const int ys = oy * g.sh - g.pt, xs = ox * g.sw - g.pl;
    const int y0 = max(ys, 0), y1 = min(ys + g.kh, g.H);
    const int x0 = max(xs, 0), x1 = min(xs + g.kw, g.W);
    const float nf = (float)((y1 - y0) * (x1 - x0));
    int rows = y1 - y0, wx = x1 - x0;
    if (wx == g.W) {                               // full-width rows are ONE contiguous run
      wx *= rows;
      rows = 1;
    }
    const int row_stride = g.W * g.C, tap_stride = per * g.C;
    const float* base = x + ((b * g.H + y0) * g.W + x0) * g.C;
    for (int c0 = 0; c0 < CV; c0 += 64) {
      const int cc = c0 + c;
      T acc = T::zero();
      if (j < per && cc < CV) {
        const float* row = base + j * g.C + cc * V;
        for (int yy = 0; yy < rows; ++yy, row += row_stride) {
          const float* p = row;
#pragma unroll 4
          for (int t = j; t < wx; t += per, p += tap_stride) acc.add(T::load(p));
        }
      }
      // fold the tap slots of each channel group: slot j takes slot j + s, s = P/2 .. 1
      for (int s = P >> 1; s >= 1; s >>= 1) {
        const T other = acc.from_lane(lane + s * cw);
        if (j + s < per) acc.add(other);
      }
      if (j == 0 && cc < CV) acc.div(nf).store(y + (size_t)o * g.C + cc * V);
    }
  }
}

// ---------------------------------------------------------------- backward (gather form)
template <int V>
__global__ __launch_bounds__(AP_THREADS) void avgpool_bwd_kernel(const float* __restrict__ dy,
                                                                float* __restrict__ dx, AvgGeom g) {
  using T = ApVec<V>;
  const int CV = g.C / V;
  const int n = g.B * g.H * g.W * CV;
  for (int i = blockIdx.x * AP_THREADS + threadIdx.x; i < n; i += gridDim.x * AP_THREADS) {
    int r = i / CV;
    const int cg = i - r * CV;
    const int q = r / g.W;
    const int xx = r - q * g.W;
    const int b = q / g.H;
    const int yy = q - b * g.H;
    // output windows covering (yy, xx): oy*sh - pt <= yy <= oy*sh - pt + kh - 1
    const int ty = yy + g.pt, tx = xx + g.pl;
    const int oy0 = ty - g.kh + 1 > 0 ? (ty - g.kh + 1 + g.sh - 1) / g.sh : 0;
    const int oy1 = min(ty / g.sh, g.OH - 1);
    const int ox0 = tx - g.kw + 1 > 0 ? (tx - g.kw + 1 + g.sw - 1) / g.sw : 0;
    const int ox1 = min(tx / g.sw, g.OW - 1);
    T acc = T::zero();
    for (int oy = oy0; oy <= oy1; ++oy) {
      const int ys = oy * g.sh - g.pt;
      const int ny = min(ys + g.kh, g.H) - max(ys, 0);
      const float* p = dy + ((b * g.OH + oy) * g.OW + ox0) * g.C + cg * V;
      for (int ox = ox0; ox <= ox1; ++ox, p += g.C) {
        const int xs = ox * g.sw - g.pl;
        const int nx = min(xs + g.kw, g.W) - max(xs, 0);
        acc.add_div(T::load(p), (float)(ny * nx));
      }
    }
    acc.store(dx + (size_t)i * V);
  }
}

static AvgGeom avg_geom(const int* g) {
  return AvgGeom{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11]};
}

// Everything the kernels handle: positive sizes, every window with at least one in-image
// tap (true of TF's SAME and VALID geometry), and tensors of at most 2^30 elements (the
// kernels index x and y with 32-bit ints).
static bool avgpool_ok(const AvgGeom& p) {
  if (p.B < 1 || p.H < 1 || p.W < 1 || p.C < 1 || p.kh < 1 || p.kw < 1 || p.sh < 1 || p.sw < 1 || p.OH < 1 ||
      p.OW < 1)
    return false;
  if (p.pt < 0 || p.pl < 0 || p.pt >= p.kh || p.pl >= p.kw) return false;
  if ((long)(p.OH - 1) * p.sh - p.pt >= p.H || (long)(p.OW - 1) * p.sw - p.pl >= p.W) return false;
  if ((long)p.kh * p.kw > AP_MAX_ELEMS) return false;
  return (long)p.B * p.H * p.W * p.C <= AP_MAX_ELEMS && (long)p.B * p.OH * p.OW * p.C <= AP_MAX_ELEMS;
}

static unsigned ap_grid(long items) {
  const long g = (items + AP_THREADS - 1) / AP_THREADS;
  return (unsigned)(g < 1 ? 1 : (g > AP_MAX_BLOCKS ? AP_MAX_BLOCKS : g));
}

static bool ap_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace csa

using namespace csa;

// The refusal of csa_avgpool_fwd / csa_avgpool_bwd, asked at plan time (host only).
CSA_API int csa_avgpool_ok(const int* g) { return g && avgpool_ok(avg_geom(g)) ? 1 : 0; }

// The window size (kh * kw) from which form = 0 picks form 2.
CSA_API int csa_avgpool_wave_taps() { return AP_WAVE_TAPS; }

// g = {B, H, W, C, kh, kw, sh, sw, pad_top, pad_left, OH, OW}.  form: 0 = the host's choice,
// 1 = a thread per output element, 2 = a wave per output position (tests, measurements).
CSA_API int csa_avgpool_fwd(const float* x, float* y, const int* g, int form, hipStream_t st) {
  if (!x || !y || !g || form < 0 || form > 2) return -2;
  const AvgGeom p = avg_geom(g);
  if (!avgpool_ok(p)) return -1;
  if (form == 0) form = p.kh * p.kw >= AP_WAVE_TAPS ? 2 : 1;
  const bool v4 = p.C % 4 == 0 && ap_aligned16(x) && ap_aligned16(y);
  const long npos = (long)p.B * p.OH * p.OW;
  if (form == 1) {
    const dim3 grid(ap_grid(npos * (v4 ? p.C / 4 : p.C)));
    if (v4) hipLaunchKernelGGL(avgpool_fwd_thread_kernel<4>, grid, dim3(AP_THREADS), 0, st, x, y, p);
    else hipLaunchKernelGGL(avgpool_fwd_thread_kernel<1>, grid, dim3(AP_THREADS), 0, st, x, y, p);
  } else {
    const dim3 grid(ap_grid(npos * 64));
    if (v4) hipLaunchKernelGGL(avgpool_fwd_wave_kernel<4>, grid, dim3(AP_THREADS), 0, st, x, y, p);
    else hipLaunchKernelGGL(avgpool_fwd_wave_kernel<1>, grid, dim3(AP_THREADS), 0, st, x, y, p);
  }
  return (int)hipGetLastError();
}

// dx[p] = sum over the windows o containing p of dy[o] / n_o; every element of dx is written.
CSA_API int csa_avgpool_bwd(const float* dy, float* dx, const int* g, hipStream_t st) {
  if (!dy || !dx || !g) return -2;
  const AvgGeom p = avg_geom(g);
  if (!avgpool_ok(p)) return -1;
  const bool v4 = p.C % 4 == 0 && ap_aligned16(dy) && ap_aligned16(dx);
  const dim3 grid(ap_grid((long)p.B * p.H * p.W * (v4 ? p.C / 4 : p.C)));
  if (v4) hipLaunchKernelGGL(avgpool_bwd_kernel<4>, grid, dim3(AP_THREADS), 0, st, dy, dx, p);
  else hipLaunchKernelGGL(avgpool_bwd_kernel<1>, grid, dim3(AP_THREADS), 0, st, dy, dx, p);
  return (int)hipGetLastError();
}
