// Depthwise convolution (gfx950 / CDNA4), fp32 NHWC: tf.nn.depthwise_conv2d, forward and backward.
//
// The reference never builds one; the DSL's {"layer": "depthwise"} lowers to a standalone unit
// over these launches.  x is [B, H, W, C], w is [kh, kw, C, M] (TF's filter layout, M the
// channel multiplier), bias [C * M] (may be absent), y is [B, OH, OW, C * M].  Output channel
// oc = c * M + q reads input channel c only, so w flattens to [tap][oc] with tap = di * kw + dj:
//   z[b, oh, ow, oc] = bias[oc] + sum_{di, dj} x[b, oh * sh + di - pt, ow * sw + dj - pl, c] * w[tap][oc]
//   y = act(z)
// over the in-image taps only, in (di, dj) row-major order, a multiply and an add each (nothing
// is contracted).  Backward, with dz the gradient through the activation, formed from y alone
// (so a leaky alpha < 0 is refused: it is not invertible from y):
//   dx[b, ih, iw, c] = sum over the windows (oh, ow) that contain the pixel, ascending, and q
//                      of dz[b, oh, ow, c * M + q] * w[tap][c * M + q];  0 where none does
//   dw[tap][oc]      = sum_{b, oh, ow} x[b, oh * sh + di - pt, ow * sw + dj - pl, c] * dz[b, oh, ow, oc]
//   dbias[oc]        = sum_{b, oh, ow} dz[b, oh, ow, oc]
//
// Forward, one thread per output element or per four output channels, lanes along the
// flattened (pixel, oc) index so loads and stores are contiguous:
//   form 1: the taps * C * M weights staged once per workgroup in LDS (up to 8192 floats);
//   form 2: the weights read from global memory through L1 / L2 (any size: 7 x 7 x 256 x 4 is
//     200 KB).
// Input gradient: gather form, one thread per input element (four channels when M = 1); every
// element is written.
// Weight and bias gradient, with L = (taps + 1) * C * M the gradients of one layer (the bias
// sums are row `taps`) and P = B * OH * OW pixels:
//   form 1 (split): workgroup r of R owns the pixels [r P / R, (r + 1) P / R) and stores row r
//     of a slab [R][L], every element.  With L <= 256 a thread per (slot, element), S = 256 / L
//     slots walking every S-th pixel of the range in ascending order, the slots folded in
//     ascending order; else a thread per element walks the range.  csa_dw_bwd_params folds the
//     rows in ascending order and STORES dw / dbias.  R = min(256, P / 32), at least 1.
//     Longest path: ceil(ceil(P / R) / S) + S + R additions.
//   form 2 (owner): a workgroup owns 16 output channels of one tap (or of the bias), 16 slots
//     walk every 16th pixel of all P in ascending order, folded in ascending order, stored
//     directly: no slab.  Longest path: ceil(P / 16) + 16 additions.
// Every serial sum is a compensated (Kahan) sum, so the error stays near one rounding of the
// sum of magnitudes whatever the path length.  No atomics anywhere and one summation order per
// form: two runs give equal bits, deterministic mode runs the same kernels; every output
// element and every slab row is stored whole by every launch.
// 16-byte accesses where C * M % 4 == 0 and every base is 16-byte aligned (x too when M = 1);
// a scalar path otherwise.  Static LDS, at most 32 KB.
//
// What form = 0 picks (scripts/dwconv_cost.py on an MI355X, us per launch, profiles/r20_notes.md).
// Forward: the two forms are within a few percent at most shapes and form 2 wins where there are
// many workgroups, each of which would stage every weight (50 x 14 x 14 x 128, 5 x 5: 12.6
// against 19.4; 3 x 3: 6.3 against 8.2; 50 x 28 x 28 x 10, 3 x 3: 4.7 against 5.7).  Form 1 won
// only with a multiplier at stride 1 and few weights (C = 10, M = 2, 5 x 5: 11.7 against 13.3;
// C = 20: 8.5 against 9.6), so it is picked for M > 1 up to DW_AUTO_LDS weights and form 2
// otherwise.  Backward: the split form up to DW_SPLIT_ROW slab floats a row (50 x 14 x 14 x 20,
// 3 x 3: 22.4 + 10.8 for the fold against 380 for the owner form, whose time is set by the
// B OH OW / 16 serial steps of a slot); the owner form caught up only with long rows: from 3328
// floats on 2450 pixels (C = 128, 5 x 5, stride 2: 79.5 against 167.1, where form = 0 still
// takes the split form) and at 6656 floats on 9800 (415 against 514).
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace csa {

constexpr int DW_T = 256;
constexpr int DW_MAX_BLOCKS = 2048;         // grid cap; the kernels stride over the rest
constexpr long DW_MAX_ELEMS = 1L << 30;     // tensors are indexed with 32-bit ints
constexpr int DW_LDS_FLOATS = 8192;         // forward form 1: the weights it stages at most
constexpr int DW_AUTO_LDS = 1024;           // form = 0: ... and picks it up to, with a multiplier
constexpr int DW_MAX_ROWS = 256;            // split form: slab rows at most
constexpr int DW_ROW_PIX = 32;              // ... and pixels a row covers at least
constexpr int DW_SPLIT_ROW = 8192;          // form = 0: the longest slab row of the split form
constexpr long DW_MAX_TAPS = 65534;         // the owner form's grid has taps + 1 rows
constexpr int DW_OWN_CH = 16, DW_OWN_SLOTS = DW_T / DW_OWN_CH;

// the thirteen ints of the launchers' geom, then CM = C * M and taps = kh * kw
struct DwGeom { int B, H, W, C, kh, kw, sh, sw, pt, pl, OH, OW, M, CM, taps; };

// A compensated (Kahan) running sum.  No fast-math: the correction term is not simplified away.
struct DwSum {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

template <int V> __device__ __forceinline__ void dw_load(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
    v[0] = *p;
  }
}

template <int V> __device__ __forceinline__ void dw_store(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// the gradient through the activation, from the output alone
__device__ __forceinline__ float dw_dz(float dy, float y, int act, float alpha) {
  return act == ACT_NONE ? dy : act_bwd(dy, y, y, act, alpha);
}

// ---------------------------------------------------------------- forward
template <int V, bool LDSW>
__global__ __launch_bounds__(DW_T) void dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y,
                                                      DwGeom g, int act, float alpha) {
  __shared__ __attribute__((aligned(16))) float s_w[LDSW ? DW_LDS_FLOATS : 4];
  if constexpr (LDSW) {
    stage_to_lds<4>(s_w, w, g.taps * g.CM, [](float v, int) { return v; });
    __syncthreads();
  }
  const int CV = g.CM / V;
  const int n = g.B * g.OH * g.OW * CV;
  for (int i = blockIdx.x * DW_T + threadIdx.x; i < n; i += gridDim.x * DW_T) {
    const int pix = i / CV, oc0 = (i - pix * CV) * V;
    const int r = pix / g.OW, ow = pix - r * g.OW;
    const int b = r / g.OH, oh = r - b * g.OH;
    // the window clipped to the image: taps [di0, di1) x [dj0, dj1), maybe none
    const int ys = oh * g.sh - g.pt, xs = ow * g.sw - g.pl;
    const int di0 = max(-ys, 0), di1 = min(g.kh, g.H - ys);
    const int dj0 = max(-xs, 0), dj1 = min(g.kw, g.W - xs);
    float acc[V];
    int ch[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      acc[e] = bias ? bias[oc0 + e] : 0.f;
      ch[e] = (oc0 + e) / g.M;
    }
    for (int di = di0; di < di1; ++di)
      for (int dj = dj0; dj < dj1; ++dj) {
        const int xi = ((b * g.H + ys + di) * g.W + xs + dj) * g.C;
        const int wi = (di * g.kw + dj) * g.CM + oc0;
        float xv[V], wv[V];
        if constexpr (LDSW) dw_load<V>(s_w + wi, wv);
        else dw_load<V>(w + wi, wv);
        if (V == 4 && g.M == 1) {
          dw_load<V>(x + xi + oc0, xv);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) xv[e] = x[xi + ch[e]];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += xv[e] * wv[e];
      }
    float o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = act_fwd(acc[e], act, alpha);
    dw_store<V>(y + (size_t)i * V, o);
  }
}

// ---------------------------------------------------------------- input gradient (gather form)
// V = 4 only with M = 1 (then oc = c and the four channels are contiguous everywhere).
template <int V>
__global__ __launch_bounds__(DW_T) void dw_bwd_dx_kernel(const float* __restrict__ w, const float* __restrict__ y,
                                                         const float* __restrict__ dy, float* __restrict__ dx,
                                                         DwGeom g, int act, float alpha) {
  const int CV = g.C / V;
  const int n = g.B * g.H * g.W * CV;
  for (int i = blockIdx.x * DW_T + threadIdx.x; i < n; i += gridDim.x * DW_T) {
    const int r = i / CV, c0 = (i - r * CV) * V;
    const int q1 = r / g.W, iw = r - q1 * g.W;
    const int b = q1 / g.H, ih = q1 - b * g.H;
    // output windows covering (ih, iw): oh * sh - pt <= ih <= oh * sh - pt + kh - 1
    const int ty = ih + g.pt, tx = iw + g.pl;
    const int oh0 = ty - g.kh + 1 > 0 ? (ty - g.kh + g.sh) / g.sh : 0;
    const int oh1 = min(ty / g.sh, g.OH - 1);
    const int ow0 = tx - g.kw + 1 > 0 ? (tx - g.kw + g.sw) / g.sw : 0;
    const int ow1 = min(tx / g.sw, g.OW - 1);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int oi = ((b * g.OH + oh) * g.OW + ow) * g.CM;
        const int wi = ((ty - oh * g.sh) * g.kw + (tx - ow * g.sw)) * g.CM;
        if constexpr (V == 4) {
          float gv[V], yv[V], wv[V];
          dw_load<V>(dy + oi + c0, gv);
          dw_load<V>(y + oi + c0, yv);
          dw_load<V>(w + wi + c0, wv);
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] += dw_dz(gv[e], yv[e], act, alpha) * wv[e];
        } else {
          for (int q = 0; q < g.M; ++q) {
            const int oc = c0 * g.M + q;
            acc[0] += dw_dz(dy[oi + oc], y[oi + oc], act, alpha) * w[wi + oc];
          }
        }
      }
    dw_store<V>(dx + (size_t)i * V, acc);
  }
}

// ---------------------------------------------------------------- weight and bias gradient
// Element j of a layer's L gradients (tap = j / CM, the bias sums at tap == taps) summed over
// the pixels p = p0, p0 + step, ... < p1 in ascending order.
__device__ __forceinline__ float dw_walk(const float* __restrict__ x, const float* __restrict__ y,
                                         const float* __restrict__ dy, const DwGeom& g, int j, int p0, int p1,
                                         int step, int act, float alpha) {
  const int tap = j / g.CM, oc = j - tap * g.CM;
  const int c = oc / g.M;
  const bool isb = tap == g.taps;
  const int di = tap / g.kw, dj = tap - di * g.kw;
  DwSum a;
  for (int p = p0; p < p1; p += step) {
    const int r = p / g.OW, ow = p - r * g.OW;
    const int b = r / g.OH, oh = r - b * g.OH;
    const int ih = oh * g.sh - g.pt + di, iw = ow * g.sw - g.pl + dj;
    if (!isb && (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W)) continue;
    const int oi = p * g.CM + oc;
    const float dz = dw_dz(dy[oi], y[oi], act, alpha);
    a.add(isb ? dz : x[((b * g.H + ih) * g.W + iw) * g.C + c] * dz);
  }
  return a.s;
}

// form 1: row r of the slab [R][L], every element
__global__ __launch_bounds__(DW_T) void dw_bwd_split_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ dy, float* __restrict__ slab,
                                                            DwGeom g, int R, int act, float alpha) {
  __shared__ float part[DW_T];
  const int L = (g.taps + 1) * g.CM;
  const int npix = g.B * g.OH * g.OW;
  const int t = threadIdx.x;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {          // (workgroup-uniform)
    const int p0 = (int)((long)r * npix / R), p1 = (int)((long)(r + 1) * npix / R);
    float* row = slab + (size_t)r * L;
    if (L > DW_T) {
      for (int j = t; j < L; j += DW_T) row[j] = dw_walk(x, y, dy, g, j, p0, p1, 1, act, alpha);
      continue;
    }
    const int S = DW_T / L;
    if (t < S * L) {
      const int s = t / L;
      part[t] = dw_walk(x, y, dy, g, t - s * L, p0 + s, p1, S, act, alpha);
    }
    __syncthreads();
    if (t < L) {
      DwSum a;
      for (int s = 0; s < S; ++s) a.add(part[s * L + t]);
      row[t] = a.s;
    }
    __syncthreads();                                         // (part is free again)
  }
}

// form 2: blockIdx.y is the tap (taps: the bias sums), blockIdx.x a block of 16 output channels
__global__ __launch_bounds__(DW_T) void dw_bwd_owner_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ dy, float* __restrict__ dw,
                                                            float* __restrict__ db, DwGeom g, int act, float alpha) {
  __shared__ float part[DW_T];
  const int t = threadIdx.x, ch = t & (DW_OWN_CH - 1), s = t / DW_OWN_CH;
  const int tap = blockIdx.y, oc = blockIdx.x * DW_OWN_CH + ch;
  const int npix = g.B * g.OH * g.OW;
  part[t] = oc < g.CM ? dw_walk(x, y, dy, g, tap * g.CM + oc, s, npix, DW_OWN_SLOTS, act, alpha) : 0.f;
  __syncthreads();
  if (t < DW_OWN_CH && oc < g.CM) {
    DwSum a;
    for (int k = 0; k < DW_OWN_SLOTS; ++k) a.add(part[k * DW_OWN_CH + t]);
    if (tap == g.taps) db[oc] = a.s;
    else dw[tap * g.CM + oc] = a.s;
  }
}

// The slab's rows folded in ascending order; element j < nw is stored into dw, the rest into db
// (may be null: a layer without a bias).
__global__ __launch_bounds__(DW_T) void dw_params_kernel(const float* __restrict__ slab, int R, int L, int nw,
                                                         float* __restrict__ dw, float* __restrict__ db) {
  for (int j = blockIdx.x * DW_T + threadIdx.x; j < L; j += gridDim.x * DW_T) {
    DwSum a;
    for (int r0 = 0; r0 < R; r0 += 16) {                     // 16 rows in flight, added in row order
      float u[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) u[k] = r0 + k < R ? slab[(size_t)(r0 + k) * L + j] : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (r0 + k < R) a.add(u[k]);
    }
    if (j < nw) dw[j] = a.s;
    else if (db) db[j - nw] = a.s;
  }
}

// Everything the kernels handle: positive sizes, pads inside the kernel window, at most 65534
// taps, and tensors, weights and strided extents inside the 2^30 range of the 32-bit index
// arithmetic.
static bool dw_ok(const int* g) {
  if (!g) return false;
  for (int k = 0; k < 13; ++k)
    if (k != 8 && k != 9 && g[k] < 1) return false;
  if (g[8] < 0 || g[9] < 0 || g[8] >= g[4] || g[9] >= g[5]) return false;
  const long B = g[0], H = g[1], W = g[2], C = g[3], OH = g[10], OW = g[11], M = g[12];
  const long taps = (long)g[4] * g[5];
  if (taps > DW_MAX_TAPS || C * M > DW_MAX_ELEMS || (taps + 1) * C * M > DW_MAX_ELEMS) return false;
  if (OH * g[6] + g[4] > DW_MAX_ELEMS || OW * g[7] + g[5] > DW_MAX_ELEMS) return false;
  if (B * H > DW_MAX_ELEMS || B * H * W > DW_MAX_ELEMS || B * OH > DW_MAX_ELEMS || B * OH * OW > DW_MAX_ELEMS)
    return false;
  return B * H * W * C <= DW_MAX_ELEMS && B * OH * OW * C * M <= DW_MAX_ELEMS;
}

static DwGeom dw_geom(const int* g) {
  return DwGeom{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12],
                g[3] * g[12], g[4] * g[5]};
}

static long dw_row(const DwGeom& q) { return (long)(q.taps + 1) * q.CM; }

// the form a launcher runs, or 0 when the named form does not take this geometry
static int dw_fwd_pick(const DwGeom& q, int form) {
  const bool fits = (long)q.taps * q.CM <= DW_LDS_FLOATS;
  if (form == 0) return q.M > 1 && (long)q.taps * q.CM <= DW_AUTO_LDS ? 1 : 2;
  return form == 1 && !fits ? 0 : form;
}

static int dw_bwd_pick(const DwGeom& q, int form) {
  if (form == 0) return dw_row(q) <= DW_SPLIT_ROW ? 1 : 2;
  return form;
}

static int dw_rows(const DwGeom& q) {
  const long r = (long)q.B * q.OH * q.OW / DW_ROW_PIX;
  return (int)(r < 1 ? 1 : r > DW_MAX_ROWS ? DW_MAX_ROWS : r);
}

static bool dw_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

static unsigned dw_grid(long items) {
  const long n = (items + DW_T - 1) / DW_T;
  return (unsigned)(n < 1 ? 1 : n > DW_MAX_BLOCKS ? DW_MAX_BLOCKS : n);
}

// leaky with alpha = 0 is relu (tf.maximum(x, 0 * x)); from y alone only relu's rule is right
static int dw_act(int act, float alpha) { return act == ACT_LEAKY && alpha == 0.f ? (int)ACT_RELU : act; }

}  // namespace csa

using namespace csa;

// geom = {B, H, W, C, kh, kw, sh, sw, pad_top, pad_left, OH, OW, M}.  The geometry refusal of
// the launchers, asked at plan time (host only).  Never a refusal for the size of the weights.
CSA_API int csa_dw_ok(const int* geom) { return dw_ok(geom) ? 1 : 0; }

// The forward form that form = 0 picks (1: weights in LDS, 2: from global memory) and the
// backward's (1: split with a slab, 2: owner); 0 when refused.
CSA_API int csa_dw_form(const int* geom) { return dw_ok(geom) ? dw_fwd_pick(dw_geom(geom), 0) : 0; }
CSA_API int csa_dw_bwd_form(const int* geom) { return dw_ok(geom) ? dw_bwd_pick(dw_geom(geom), 0) : 0; }

// The weights forward form 1 stages at most (floats), the split form's row cap, and the rows R
// of its slab [R][(taps + 1) * C * M] for a geometry (0 when refused).
CSA_API int csa_dw_lds_floats() { return DW_LDS_FLOATS; }
CSA_API int csa_dw_max_rows() { return DW_MAX_ROWS; }
CSA_API int csa_dw_slab_rows(const int* geom) { return dw_ok(geom) ? dw_rows(dw_geom(geom)) : 0; }

// y = act(conv + bias); bias may be null.  form: 0 = the host's choice, 1 / 2 as above (form 1
// with weights beyond its LDS budget: refused).  Refused without a launch (non-zero): a null
// pointer other than bias, a geometry csa_dw_ok refuses, an unknown act or form, a leaky alpha
// that is not finite.
CSA_API int csa_dw_fwd(const float* x, const float* w, const float* bias, float* y, const int* geom, int act,
                       float alpha, int form, hipStream_t st) {
  if (!x || !w || !y || !geom) return -2;
  if (form < 0 || form > 2 || act < ACT_NONE || act > ACT_LEAKY) return -2;
  if (!dw_ok(geom) || !isfinite(alpha)) return -1;
  const DwGeom q = dw_geom(geom);
  const int f = dw_fwd_pick(q, form);
  if (f == 0) return -1;
  const bool v4 = q.CM % 4 == 0 && dw_aligned16(x) && dw_aligned16(w) && dw_aligned16(bias) && dw_aligned16(y);
  const dim3 grid(dw_grid((long)q.B * q.OH * q.OW * (v4 ? q.CM / 4 : q.CM)));
  if (f == 1) {
    if (v4) hipLaunchKernelGGL((dw_fwd_kernel<4, true>), grid, dim3(DW_T), 0, st, x, w, bias, y, q, act, alpha);
    else hipLaunchKernelGGL((dw_fwd_kernel<1, true>), grid, dim3(DW_T), 0, st, x, w, bias, y, q, act, alpha);
  } else {
    if (v4) hipLaunchKernelGGL((dw_fwd_kernel<4, false>), grid, dim3(DW_T), 0, st, x, w, bias, y, q, act, alpha);
    else hipLaunchKernelGGL((dw_fwd_kernel<1, false>), grid, dim3(DW_T), 0, st, x, w, bias, y, q, act, alpha);
  }
  return (int)hipGetLastError();
}

// dx (may be null: the unit is first) receives the input gradient, every element.  form 1: slab
// [csa_dw_slab_rows][(taps + 1) * C * M] receives every row (csa_dw_bwd_params then stores the
// gradients; dw and db are not touched here and may be null).  form 2: dw [kh, kw, C, M] and db
// [C * M] (null: no bias) are stored directly and slab may be null.  form 0: the host's choice
// (csa_dw_bwd_form), which needs slab or dw accordingly.  The forward's refusals, and a leaky
// alpha < 0 (the backward reads y only).
CSA_API int csa_dw_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx, float* slab,
                       float* dw, float* db, const int* geom, int act, float alpha, int form, hipStream_t st) {
  if (!x || !w || !y || !dy || !geom) return -2;
  if (form < 0 || form > 2 || act < ACT_NONE || act > ACT_LEAKY) return -2;
  if (!dw_ok(geom) || !isfinite(alpha) || (act == ACT_LEAKY && alpha < 0.f)) return -1;
  const DwGeom q = dw_geom(geom);
  const int f = dw_bwd_pick(q, form);
  if ((f == 1 && !slab) || (f == 2 && !dw)) return -2;
  act = dw_act(act, alpha);
  if (dx) {
    const bool v4 = q.M == 1 && q.C % 4 == 0 && dw_aligned16(w) && dw_aligned16(y) && dw_aligned16(dy) &&
                    dw_aligned16(dx);
    const dim3 grid(dw_grid((long)q.B * q.H * q.W * (v4 ? q.C / 4 : q.C)));
    if (v4) hipLaunchKernelGGL(dw_bwd_dx_kernel<4>, grid, dim3(DW_T), 0, st, w, y, dy, dx, q, act, alpha);
    else hipLaunchKernelGGL(dw_bwd_dx_kernel<1>, grid, dim3(DW_T), 0, st, w, y, dy, dx, q, act, alpha);
  }
  if (f == 1) {
    const int R = dw_rows(q);
    hipLaunchKernelGGL(dw_bwd_split_kernel, dim3(R), dim3(DW_T), 0, st, x, y, dy, slab, q, R, act, alpha);
  } else {
    const dim3 grid((q.CM + DW_OWN_CH - 1) / DW_OWN_CH, q.taps + (db ? 1 : 0));
    hipLaunchKernelGGL(dw_bwd_owner_kernel, grid, dim3(DW_T), 0, st, x, y, dy, dw, db, q, act, alpha);
  }
  return (int)hipGetLastError();
}

// The split form's slab rows folded in order r = 0 .. R - 1, stored into dw (taps * C * M
// floats) and db (C * M floats; null: no bias).  rows must be csa_dw_slab_rows(geom).
CSA_API int csa_dw_bwd_params(const float* slab, int rows, const int* geom, float* dw, float* db, hipStream_t st) {
  if (!slab || !dw || !geom) return -2;
  if (!dw_ok(geom)) return -1;
  const DwGeom q = dw_geom(geom);
  if (rows != dw_rows(q)) return -1;
  const long L = dw_row(q);
  hipLaunchKernelGGL(dw_params_kernel, dim3(dw_grid(L)), dim3(DW_T), 0, st, slab, rows, (int)L, q.taps * q.CM, dw,
                     db);
  return (int)hipGetLastError();
}
