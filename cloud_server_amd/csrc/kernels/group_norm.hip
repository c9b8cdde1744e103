// Layer / group / instance normalisation (gfx950 / CDNA4), fp32 NHWC, forward and backward.
//
// The reference never builds one; the DSL's {"layer": "norm", "mode": "layer" | "group" |
// "instance"} lowers to a standalone unit over these launches.  With G groups per sample,
// D = C / G channels per group and x seen as [B, HW, G, D], every (sample, group) is normalised
// on its own over its m = HW * D elements (TF's biased moments):
//   mean = sum x / m,  var = sum (x - mean)^2 / m,  rstd = 1 / sqrt(var + eps)
//   xhat = (x - mean) * rstd,  z = xhat * scale_c + offset_c,  y = act(z)
// Layer norm is G = 1, instance norm G = C.  The variance is the centred two-pass form with the
// first pass's rounding folded back in: d = x - mean0, mean = mean0 + sum d / m,
// var = sum d^2 / m - (sum d / m)^2.  E[x^2] - mean^2 is never formed.
// Backward, with dz the gradient through the activation (z is recomputed from x and the kept
// {mean, rstd}, so any leaky alpha works and y is never read) and a = dz * scale_c:
//   s1 = sum a * xhat,  s2 = sum a,  dx = rstd * (a - (s2 + xhat * s1) / m)
// and the same launch stores this group's per-channel sums over its HW positions of dz * xhat
// and dz into row b of a slab [B][2][C]: every (b, g) owns its own channels of its own row.
// csa_gn_bwd_params folds the rows in order b = 0 .. B - 1 and STORES dscale / doffset.
//
// One wave or one workgroup owns one (sample, group); three forms:
//   form 1: a wave (a 64-thread workgroup) holds the group in registers, m <= 1024;
//   form 2: a 256-thread workgroup holds it in registers, m <= 4096 (the sample's
//     14 x 14 x 20 with G = 1 is 3920); wave sums by DPP, LDS across the waves;
//   form 3: a 1024-thread workgroup streams the group three times through L2, any m.
// In forms 1 and 2 the group is loaded once: moments and output come from the registers.
// Addressing is ((b * HW + p) * C + g * D + j); accesses are 16 bytes wide when D % 4 == 0 and
// every base is 16-byte aligned, and with G = 1 the sample is one contiguous run of HW * C
// floats (16 bytes wide when HW * C % 4 == 0).  The per-channel sums of the backward re-read
// the group's x and dy (L1 / L2 resident: the launch has just read them) in a fixed
// (segment, position) order, as compensated sums.  No atomics anywhere and one summation
// order per form: two runs give equal bits and deterministic mode runs the same kernels.
// Static LDS, at most 8.2 KB.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace csa {

constexpr int GN_R = 16;                    // elements a thread of forms 1 and 2 holds
constexpr int GN_T1 = 64, GN_T2 = 256, GN_T3 = 1024;
constexpr int GN_M1 = GN_T1 * GN_R;         // largest group of form 1
constexpr int GN_M2 = GN_T2 * GN_R;         // ... of form 2
// What form = 0 picks, by the group's size m (scripts/gn_cost.py on an MI355X, per launch,
// profiles/r19_notes.md).  Up to GN_AUTO1 elements a wave: 50 x 14 x 14 x 20 as instance norm
// (m = 196, 1000 groups) took 6.0 / 10.2 us forward / backward in form 1 against 6.8 / 18.2 in
// form 2.  Up to GN_AUTO2 a 256-thread workgroup: at m = 512 (50 groups) and m = 980 (200
// groups) form 2 won (3.5 / 4.1 against 3.9 / 6.3 and 4.9 / 7.9 against 6.8 / 13.4).  Beyond,
// streaming, although the group would still fit form 2's registers: at m = 3920 (the sample's
// layer norm, 50 groups) 1024 threads with a float4 each beat 256 threads with four (4.7 / 8.7
// against 5.6 / 11.1 us): the launch is latency-bound and the re-reads hit L2.
constexpr int GN_AUTO1 = 256;
constexpr int GN_AUTO2 = 2048;
constexpr int GN_MAX_BLOCKS = 2048;         // grid cap; the kernels stride over the rest
constexpr long GN_MAX_ELEMS = 1L << 30;     // tensors are indexed with 32-bit ints

// B, HW, C, G, D = C / G as given; fHW, fC (row stride), fD the view the moments walk: the
// same, or with G = 1 the whole sample as one row (fHW = 1, fC = fD = HW * C).
struct GnGeom { int B, HW, C, G, D, fHW, fC, fD; };

template <int V> __device__ __forceinline__ void gn_load(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
    v[0] = *p;
  }
}

template <int V> __device__ __forceinline__ void gn_store(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// Offset of element e of group g, which starts at base, and the element's channel c0: one
// integer division per element (block-uniform branches).  In the G = 1 view the group is the
// contiguous sample and the channel is e % C (nothing to divide for a flat input, HW = 1).
__device__ __forceinline__ int gn_off(const GnGeom& q, int base, int g, int e, int& c0) {
  if (q.fHW == 1) {
    c0 = q.HW == 1 ? g * q.D + e : e % q.C;
    return base + e;
  }
  const int p = e / q.fD, j = e - p * q.fD;
  c0 = g * q.D + j;
  return base + p * q.fC + j;
}

// channel of the k-th element of a quad that starts at channel c0
__device__ __forceinline__ int gn_chan(const GnGeom& q, int c0, int k) {
  const int c = c0 + k;
  return c < q.C ? c : c % q.C;               // (a quad wraps only in the G = 1 view)
}

// Sum of a over the workgroup, every thread gets it; red holds T / 64 floats.  The same order
// as gn_block_sum2.
template <int T> __device__ __forceinline__ float gn_block_sum(float a, float* red) {
  a = wave_sum_dpp(a);
  if constexpr (T > 64) {
    constexpr int NW = T / 64;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    float sa = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) sa += red[i];
    a = sa;
    __syncthreads();                          // (red is free again)
  }
  return a;
}

// Sums of a and b over the workgroup, every thread gets both; red holds 2 * T / 64 floats.
// Fixed order: the DPP tree inside a wave, then the waves in ascending order.
template <int T> __device__ __forceinline__ void gn_block_sum2(float& a, float& b, float* red) {
  a = wave_sum_dpp(a);
  b = wave_sum_dpp(b);
  if constexpr (T > 64) {
    constexpr int NW = T / 64;
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      red[w] = a;
      red[NW + w] = b;
    }
    __syncthreads();
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      sa += red[i];
      sb += red[NW + i];
    }
    a = sa;
    b = sb;
    __syncthreads();                          // (red is free again)
  }
}

// A compensated (Kahan) running sum: the long serial sums of the per-channel pass (one thread
// walks up to HW positions, then the segments, then the B slab rows) keep an error of about
// one rounding whatever their length.  No fast-math: the correction term is not simplified away.
struct GnSum {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

__device__ __forceinline__ float gn_dz(float dy, float xhat, float sc, float of, int act, float alpha) {
  if (act == ACT_NONE) return dy;
  const float z = xhat * sc + of;
  return act_bwd(dy, z, act_fwd(z, act, alpha), act, alpha);
}

// ---------------------------------------------------------------- forms 1 and 2, forward
template <int T, int V>
__global__ __launch_bounds__(T) void gn_fwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                       const float* __restrict__ offset, float* __restrict__ y,
                                                       float* __restrict__ stat, GnGeom q, float eps, int act,
                                                       float alpha) {
  constexpr int NI = GN_R / V;
  __shared__ float red[2 * (T / 64)];
  const int t = threadIdx.x, m = q.fHW * q.fD, ni = m / V;
  const float mf = (float)m;
  for (int bg = blockIdx.x; bg < q.B * q.G; bg += gridDim.x) {   // (workgroup-uniform)
    const int b = bg / q.G, g = bg - b * q.G;
    const int base = b * q.fHW * q.fC + g * q.fD;
    float v[NI][V];
    int off[NI], ch[NI];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int i = t + k * T;
      off[k] = -1;
      ch[k] = 0;
#pragma unroll
      for (int e = 0; e < V; ++e) v[k][e] = 0.f;
      if (i < ni) {
        off[k] = gn_off(q, base, g, i * V, ch[k]);
        gn_load<V>(x + off[k], v[k]);
      }
#pragma unroll
      for (int e = 0; e < V; ++e) s += v[k][e];
    }
    const float mean0 = gn_block_sum<T>(s, red) / mf;
    float sd = 0.f, sq = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = off[k] >= 0 ? v[k][e] - mean0 : 0.f;
        v[k][e] = d;
        sd += d;
        sq += d * d;
      }
    gn_block_sum2<T>(sd, sq, red);
    const float delta = sd / mf;
    const float var = fmaxf(sq / mf - delta * delta, 0.f);
    const float rstd = 1.0f / sqrtf(var + eps);
    if (stat && t == 0) {
      stat[2 * bg] = mean0 + delta;
      stat[2 * bg + 1] = rstd;
    }
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (off[k] >= 0) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int c = gn_chan(q, ch[k], e);
          o[e] = act_fwd(((v[k][e] - delta) * rstd) * scale[c] + offset[c], act, alpha);
        }
        gn_store<V>(y + off[k], o);
      }
  }
}

// ---------------------------------------------------------------- form 3, forward
template <int T, int V>
__global__ __launch_bounds__(T) void gn_fwd_stream_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ offset, float* __restrict__ y,
                                                          float* __restrict__ stat, GnGeom q, float eps, int act,
                                                          float alpha) {
  __shared__ float red[2 * (T / 64)];
  const int t = threadIdx.x, m = q.fHW * q.fD, ni = m / V;
  const float mf = (float)m;
  for (int bg = blockIdx.x; bg < q.B * q.G; bg += gridDim.x) {
    const int b = bg / q.G, g = bg - b * q.G;
    const int base = b * q.fHW * q.fC + g * q.fD;
    float s = 0.f;
    int c0;
    for (int i = t; i < ni; i += T) {
      float v[V];
      gn_load<V>(x + gn_off(q, base, g, i * V, c0), v);
#pragma unroll
      for (int e = 0; e < V; ++e) s += v[e];
    }
    const float mean0 = gn_block_sum<T>(s, red) / mf;
    float sd = 0.f, sq = 0.f;
    for (int i = t; i < ni; i += T) {
      float v[V];
      gn_load<V>(x + gn_off(q, base, g, i * V, c0), v);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = v[e] - mean0;
        sd += d;
        sq += d * d;
      }
    }
    gn_block_sum2<T>(sd, sq, red);
    const float delta = sd / mf;
    const float var = fmaxf(sq / mf - delta * delta, 0.f);
    const float rstd = 1.0f / sqrtf(var + eps);
    if (stat && t == 0) {
      stat[2 * bg] = mean0 + delta;
      stat[2 * bg + 1] = rstd;
    }
    for (int i = t; i < ni; i += T) {
      const int off = gn_off(q, base, g, i * V, c0);
      float v[V], o[V];
      gn_load<V>(x + off, v);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int c = gn_chan(q, c0, e);
        o[e] = act_fwd((((v[e] - mean0) - delta) * rstd) * scale[c] + offset[c], act, alpha);
      }
      gn_store<V>(y + off, o);
    }
  }
}

// ---------------------------------------------------------------- backward: per-channel sums
// Row b of the slab, channels g * D .. g * D + D - 1: sum over the HW positions of dz * xhat
// ([0][c]) and of dz ([1][c]).  D <= T: min(T / D, HW) segments of consecutive positions, a
// thread per (segment, channel) walking its positions in ascending order, then the segments
// folded in ascending order.  D > T: a thread per channel walks every position.
// part holds 2 * T floats.  Every thread of the workgroup must call it.
template <int T>
__device__ __forceinline__ void gn_channel_sums(const float* __restrict__ x, const float* __restrict__ dy,
                                                const float* __restrict__ scale, const float* __restrict__ offset,
                                                float* __restrict__ slab, const GnGeom& q, int b, int g, float mean,
                                                float rstd, int act, float alpha, float* part) {
  const int t = threadIdx.x;
  const int base = b * q.HW * q.C + g * q.D;
  float* row = slab + (size_t)b * 2 * q.C + g * q.D;
  if (q.D > T) {                                             // (workgroup-uniform)
    for (int j = t; j < q.D; j += T) {
      const float sc = scale[g * q.D + j], of = offset[g * q.D + j];
      GnSum a1, a2;
      for (int p = 0; p < q.HW; ++p) {
        const int off = base + p * q.C + j;
        const float xhat = (x[off] - mean) * rstd;
        const float dz = gn_dz(dy[off], xhat, sc, of, act, alpha);
        a1.add(dz * xhat);
        a2.add(dz);
      }
      row[j] = a1.s;
      row[q.C + j] = a2.s;
    }
    return;
  }
  const int S = min(T / q.D, q.HW);
  if (t < S * q.D) {
    const int s = t / q.D, j = t - s * q.D;
    const int p0 = (int)((long)s * q.HW / S), p1 = (int)((long)(s + 1) * q.HW / S);
    const float sc = scale[g * q.D + j], of = offset[g * q.D + j];
    GnSum a1, a2;
    for (int p = p0; p < p1; ++p) {
      const int off = base + p * q.C + j;
      const float xhat = (x[off] - mean) * rstd;
      const float dz = gn_dz(dy[off], xhat, sc, of, act, alpha);
      a1.add(dz * xhat);
      a2.add(dz);
    }
    part[t] = a1.s;
    part[T + t] = a2.s;
  }
  __syncthreads();
  if (t < q.D) {
    GnSum a1, a2;
    for (int s = 0; s < S; ++s) {
      a1.add(part[s * q.D + t]);
      a2.add(part[T + s * q.D + t]);
    }
    row[t] = a1.s;
    row[q.C + t] = a2.s;
  }
  __syncthreads();                                           // (part is free again)
}

// ---------------------------------------------------------------- forms 1 and 2, backward
template <int T, int V>
__global__ __launch_bounds__(T) void gn_bwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                       const float* __restrict__ offset,
                                                       const float* __restrict__ stat, const float* __restrict__ dy,
                                                       float* __restrict__ dx, float* __restrict__ slab, GnGeom q,
                                                       int act, float alpha) {
  constexpr int NI = GN_R / V;
  __shared__ float red[2 * (T / 64)];
  __shared__ float part[2 * T];
  const int t = threadIdx.x, m = q.fHW * q.fD, ni = m / V;
  const float mf = (float)m;
  for (int bg = blockIdx.x; bg < q.B * q.G; bg += gridDim.x) {
    const int b = bg / q.G, g = bg - b * q.G;
    const int base = b * q.fHW * q.fC + g * q.fD;
    const float mean = stat[2 * bg], rstd = stat[2 * bg + 1];
    float a[NI][V], xh[NI][V];
    int off[NI];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int i = t + k * T;
      off[k] = -1;
#pragma unroll
      for (int e = 0; e < V; ++e) a[k][e] = xh[k][e] = 0.f;
      if (i < ni) {
        int c0;
        off[k] = gn_off(q, base, g, i * V, c0);
        float xv[V], gv[V];
        gn_load<V>(x + off[k], xv);
        gn_load<V>(dy + off[k], gv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int c = gn_chan(q, c0, e);
          const float sc = scale[c];
          const float xhat = (xv[e] - mean) * rstd;
          xh[k][e] = xhat;
          a[k][e] = gn_dz(gv[e], xhat, sc, offset[c], act, alpha) * sc;
        }
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        s1 += a[k][e] * xh[k][e];
        s2 += a[k][e];
      }
    }
    gn_block_sum2<T>(s1, s2, red);
    if (dx) {
#pragma unroll
      for (int k = 0; k < NI; ++k)
        if (off[k] >= 0) {
          float o[V];
#pragma unroll
          for (int e = 0; e < V; ++e) o[e] = rstd * (a[k][e] - (s2 + xh[k][e] * s1) / mf);
          gn_store<V>(dx + off[k], o);
        }
    }
    gn_channel_sums<T>(x, dy, scale, offset, slab, q, b, g, mean, rstd, act, alpha, part);
  }
}

// ---------------------------------------------------------------- form 3, backward
template <int T, int V>
__global__ __launch_bounds__(T) void gn_bwd_stream_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ offset,
                                                          const float* __restrict__ stat,
                                                          const float* __restrict__ dy, float* __restrict__ dx,
                                                          float* __restrict__ slab, GnGeom q, int act, float alpha) {
  __shared__ float red[2 * (T / 64)];
  __shared__ float part[2 * T];
  const int t = threadIdx.x, m = q.fHW * q.fD, ni = m / V;
  const float mf = (float)m;
  for (int bg = blockIdx.x; bg < q.B * q.G; bg += gridDim.x) {
    const int b = bg / q.G, g = bg - b * q.G;
    const int base = b * q.fHW * q.fC + g * q.fD;
    const float mean = stat[2 * bg], rstd = stat[2 * bg + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int i = t; i < ni; i += T) {
      int c0;
      const int off = gn_off(q, base, g, i * V, c0);
      float xv[V], gv[V];
      gn_load<V>(x + off, xv);
      gn_load<V>(dy + off, gv);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int c = gn_chan(q, c0, e);
        const float sc = scale[c];
        const float xhat = (xv[e] - mean) * rstd;
        const float av = gn_dz(gv[e], xhat, sc, offset[c], act, alpha) * sc;
        s1 += av * xhat;
        s2 += av;
      }
    }
    gn_block_sum2<T>(s1, s2, red);
    if (dx) {
      for (int i = t; i < ni; i += T) {
        int c0;
        const int off = gn_off(q, base, g, i * V, c0);
        float xv[V], gv[V], o[V];
        gn_load<V>(x + off, xv);
        gn_load<V>(dy + off, gv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int c = gn_chan(q, c0, e);
          const float sc = scale[c];
          const float xhat = (xv[e] - mean) * rstd;
          const float av = gn_dz(gv[e], xhat, sc, offset[c], act, alpha) * sc;
          o[e] = rstd * (av - (s2 + xhat * s1) / mf);
        }
        gn_store<V>(dx + off, o);
      }
    }
    gn_channel_sums<T>(x, dy, scale, offset, slab, q, b, g, mean, rstd, act, alpha, part);
  }
}

// dscale_c = sum_b slab[b][0][c], doffset_c = sum_b slab[b][1][c], rows in ascending order; stored.
__global__ __launch_bounds__(256) void gn_params_kernel(const float* __restrict__ slab, int B, int C,
                                                        float* __restrict__ dscale, float* __restrict__ doffset) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c < C; c += gridDim.x * 256) {
    GnSum a1, a2;
    for (int b0 = 0; b0 < B; b0 += 16) {          // 16 rows in flight, added in row order
      float u[16], w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const bool on = b0 + k < B;
        u[k] = on ? slab[((size_t)(b0 + k) * 2) * C + c] : 0.f;
        w[k] = on ? slab[((size_t)(b0 + k) * 2 + 1) * C + c] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (b0 + k < B) {
          a1.add(u[k]);
          a2.add(w[k]);
        }
    }
    dscale[c] = a1.s;
    doffset[c] = a2.s;
  }
}

// Everything the kernels handle: positive dimensions, G dividing C, at most 2^30 elements.
static bool gn_ok(const int* g) {
  if (!g || g[0] < 1 || g[1] < 1 || g[2] < 1 || g[3] < 1) return false;
  if (g[2] % g[3] != 0) return false;
  return (long)g[0] * g[1] * g[2] <= GN_MAX_ELEMS;
}

static GnGeom gn_geom(const int* g) {
  GnGeom q{g[0], g[1], g[2], g[3], g[2] / g[3], g[1], g[2], g[2] / g[3]};
  if (q.G == 1) {
    q.fHW = 1;
    q.fC = q.fD = q.HW * q.C;
  }
  return q;
}

static int gn_auto_form(const GnGeom& q) {
  const long m = (long)q.fHW * q.fD;
  return m <= GN_AUTO1 ? 1 : m <= GN_AUTO2 ? 2 : 3;
}

// the form a launcher runs, or 0 when the named form does not take this group size
static int gn_pick(const GnGeom& q, int form) {
  const long m = (long)q.fHW * q.fD;
  if (form == 0) return gn_auto_form(q);
  if ((form == 1 && m > GN_M1) || (form == 2 && m > GN_M2)) return 0;
  return form;
}

static bool gn_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// 16-byte accesses: the group's rows are whole float4s at 16-byte aligned addresses
static bool gn_vec(const GnGeom& q) { return q.fD % 4 == 0 && q.fC % 4 == 0; }

static unsigned gn_grid(const GnGeom& q) {
  const long n = (long)q.B * q.G;
  return (unsigned)(n > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : n);
}

}  // namespace csa

using namespace csa;

// geom = {B, HW, C, G}; a flat [B, F] input has HW = 1 and C = F.  The geometry refusal of the
// launchers, asked at plan time (host only).
CSA_API int csa_gn_ok(const int* geom) { return gn_ok(geom) ? 1 : 0; }

// The form that form = 0 picks (1: a wave, 2: a workgroup, 3: streaming); 0 when refused.
CSA_API int csa_gn_form(const int* geom) { return gn_ok(geom) ? gn_auto_form(gn_geom(geom)) : 0; }

// The largest group (elements) a form takes (form 3: any, the tensor limit) and the grid cap.
CSA_API int csa_gn_form_max(int form) { return form == 1 ? GN_M1 : form == 2 ? GN_M2 : form == 3 ? (int)GN_MAX_ELEMS : 0; }
CSA_API int csa_gn_max_blocks() { return GN_MAX_BLOCKS; }

// kernel<T, 4> when v4 (16-byte accesses), else kernel<T, 1>: one workgroup per (sample, group) of q
#define GN_LAUNCH(kernel, T, v4, q, st, ...)                                                            \
  do {                                                                                                  \
    if (v4) hipLaunchKernelGGL((kernel<T, 4>), dim3(gn_grid(q)), dim3(T), 0, st, __VA_ARGS__);          \
    else hipLaunchKernelGGL((kernel<T, 1>), dim3(gn_grid(q)), dim3(T), 0, st, __VA_ARGS__);             \
  } while (0)

// y = act(xhat * scale + offset); stat (may be null: forward-only) receives {mean, rstd} per
// (b, g).  form: 0 = the host's choice, 1 / 2 / 3 as above (a form the group does not fit: refused).
// Refused without a launch (non-zero): a null pointer other than stat, a non-positive dimension,
// C % G != 0, more than 2^30 elements, an epsilon that is not finite and > 0, an unknown act or
// form, and a leaky alpha that is not finite (it multiplies every element).
CSA_API int csa_gn_fwd(const float* x, const float* scale, const float* offset, float* y, float* stat,
                       const int* geom, float eps, int act, float alpha, int form, hipStream_t st) {
  if (!x || !scale || !offset || !y || !geom) return -2;
  if (form < 0 || form > 3 || act < ACT_NONE || act > ACT_LEAKY) return -2;
  if (!gn_ok(geom) || !isfinite(eps) || !(eps > 0.f) || !isfinite(alpha)) return -1;
  const GnGeom q = gn_geom(geom);
  const int f = gn_pick(q, form);
  if (f == 0) return -1;
  const bool v4 = gn_vec(q) && gn_aligned16(x) && gn_aligned16(y);
  if (f == 1) GN_LAUNCH(gn_fwd_reg_kernel, GN_T1, v4, q, st, x, scale, offset, y, stat, q, eps, act, alpha);
  else if (f == 2) GN_LAUNCH(gn_fwd_reg_kernel, GN_T2, v4, q, st, x, scale, offset, y, stat, q, eps, act, alpha);
  else GN_LAUNCH(gn_fwd_stream_kernel, GN_T3, v4, q, st, x, scale, offset, y, stat, q, eps, act, alpha);
  return (int)hipGetLastError();
}

// stat = the forward's {mean, rstd}; dy = the gradient of y.  dx (may be null: the unit is
// first) receives the input gradient, every element; slab [B][2][C] receives every element of
// the per-sample channel sums either way.  The forward's refusals, without epsilon; a null dx is
// the one pointer besides it that may be null.
CSA_API int csa_gn_bwd(const float* x, const float* scale, const float* offset, const float* stat, const float* dy,
                       float* dx, float* slab, const int* geom, int act, float alpha, int form, hipStream_t st) {
  if (!x || !scale || !offset || !stat || !dy || !slab || !geom) return -2;
  if (form < 0 || form > 3 || act < ACT_NONE || act > ACT_LEAKY) return -2;
  if (!gn_ok(geom) || !isfinite(alpha)) return -1;
  const GnGeom q = gn_geom(geom);
  const int f = gn_pick(q, form);
  if (f == 0) return -1;
  const bool v4 = gn_vec(q) && gn_aligned16(x) && gn_aligned16(dy) && gn_aligned16(dx);
  if (f == 1) GN_LAUNCH(gn_bwd_reg_kernel, GN_T1, v4, q, st, x, scale, offset, stat, dy, dx, slab, q, act, alpha);
  else if (f == 2) GN_LAUNCH(gn_bwd_reg_kernel, GN_T2, v4, q, st, x, scale, offset, stat, dy, dx, slab, q, act, alpha);
  else GN_LAUNCH(gn_bwd_stream_kernel, GN_T3, v4, q, st, x, scale, offset, stat, dy, dx, slab, q, act, alpha);
  return (int)hipGetLastError();
}

// The slab's rows folded in order b = 0 .. B - 1, stored into dscale / doffset (C floats each).
CSA_API int csa_gn_bwd_params(const float* slab, int B, int C, float* dscale, float* doffset, hipStream_t st) {
  if (!slab || !dscale || !doffset) return -2;
  if (B < 1 || C < 1 || (long)B * C > GN_MAX_ELEMS) return -1;
  const int blocks = (C + 255) / 256;
  hipLaunchKernelGGL(gn_params_kernel, dim3(blocks > 64 ? 64 : blocks), dim3(256), 0, st, slab, B, C, dscale, doffset);
  return (int)hipGetLastError();
}
