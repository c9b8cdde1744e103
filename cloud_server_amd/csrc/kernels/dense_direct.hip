// Register-direct f32 MFMA kernels for the skinny dense layers of the training step
// (gfx950).  The reference's dense layers (construct_distribute.py:168-182, 252-264) are
// [B=50] x [in] x [out] GEMMs: one dimension is the tiny batch, the weights are the only
// big operand.  The LDS-staged split-K GEMM (gemm.hip) spends most of its 7-20 us per
// launch in staging, barriers and the intra-WG K reduction; here operands go straight
// from global memory (L2) into MFMA registers:
//
//   * dd_fwd    Y[M][N]  (+)= act(X)[M][K] . W[K][N] + b      ("NN")
//   * dd_dgrad  dX[M][F]  = dY[M][N] . W[F][N]^T, epilogue through the forward input
//               transform: dz = act'(g), per-channel {sum dz, sum dz*xhat} (BN backward)
//   * dd_wgrad  dW[F][N] = act(X)^T[F][M] . dY[M][N] (K = batch), epilogue either the
//               plain gradient store or the OPTIMIZER UPDATE itself (optim_common.h):
//               W, its slots and the bias are updated in place and the gradient never
//               exists in memory.
//
// MFMA v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md §3):
//   A: lane l holds A[i = l&31][k = l>>5];  B: lane l holds B[k = l>>5][j = l&31];
//   D: reg r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31].
// K-contiguous operands ("row of A" / "row of W^T") are loaded as ONE float4 per lane
// covering k0+4h..k0+4h+3 (h = l>>5) and fed over 4 MFMA steps, step s taking component
// s: step s multiplies k = k0+4h+s from both operands, so the sum over k is complete
// (the k order inside the 8-block is permuted, the products are the same).
// Each wave owns a 64-row (two 32-row sub-tiles) x 32-column output tile: the 32x8 B
// fragment is loaded once for both sub-tiles.  The 4 waves of a workgroup split the
// workgroup's K range; their partials meet in LDS in fixed wave order.
//
// The forward has a second form, dd_fwd_wide_kernel (round 12, further down): 16 waves per
// workgroup, one 32x32 accumulator per wave, the sixteen partial tiles folded in LDS before
// anything is emitted, so a launch adds a quarter of the split-K atomic bytes into Y (fc1:
// 3.03 MB -> 0.78 MB measured).  dd_fwd_plan picks it for the one-process-per-GPU atomic
// profile; deterministic mode, the packed and the shared-GPU profile, K % 4 != 0, the
// forward chain and the grouped forward keep dd_fwd_body.  Its BN form, dd_fwd_wide_bn_kernel
// (round 14, csa_dd_fwd_bn), also applies the producer's BatchNorm + activation to A on load and
// writes xt, the BatchNorm tables and the carried update's cleared flag: fc1's forward in the
// one-GPU training program, where bn_act_apply (elementwise.hip) was a launch of its own.
#include "common.h"
#include "optim_common.h"
#include "head_dgrad.h"
#include <cstdlib>

namespace csa {

typedef float dd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int DD_THREADS = 256;
constexpr int DD_WAVES = 4;
constexpr int DD_SLAB_ROWS = 16;      // BN-backward slab rows (same contract as gemm.hip)
constexpr int DD_MAXC = 128;
constexpr int DD_U = 4;               // 8-k blocks whose loads are in flight together

// diagnostics: block-0 phase stamps [0..3] + the earliest block start [4] and the latest
// block end [5] of a launch (s_memtime ticks); null disables
__constant__ long long* g_dd_dbg = nullptr;
#define DD_STAMP(i)                                                                           \
  do {                                                                                        \
    if (g_dd_dbg && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) \
      g_dd_dbg[i] = (long long)__builtin_amdgcn_s_memtime();                                  \
  } while (0)
#define DD_SPAN_BEGIN()                                                                       \
  do {                                                                                        \
    if (g_dd_dbg && threadIdx.x == 0)                                                         \
      atomicMin((unsigned long long*)&g_dd_dbg[4], (unsigned long long)__builtin_amdgcn_s_memtime()); \
  } while (0)
#define DD_SPAN_END()                                                                         \
  do {                                                                                        \
    if (g_dd_dbg && threadIdx.x == 0)                                                         \
      atomicMax((unsigned long long*)&g_dd_dbg[5], (unsigned long long)__builtin_amdgcn_s_memtime()); \
  } while (0)

// diagnostic build only (-DCSA_DD_PHASES): phase p of every workgroup of the BN forward at
// [8 + 8 b + p] (s_memrealtime, 100 MHz): 0 start | 1 table in LDS, barrier passed | 2 X landed |
// 3 transform done | 4 W landed | 5 MFMAs issued, xt stores out (scripts/mb/graph_life.py)
#ifdef CSA_DD_PHASES
#define DD_PHASE(p)                                                                           \
  do {                                                                                        \
    if (g_dd_dbg && threadIdx.x == 0)                                                         \
      g_dd_dbg[8 + 8 * (int)blockIdx.x + (p)] = (long long)__builtin_amdgcn_s_memrealtime();  \
  } while (0)
#else
#define DD_PHASE(p) do {} while (0)
#endif

__device__ __forceinline__ int dd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ void dd_pin4(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ __forceinline__ void dd_pin(float& v) { asm volatile("" : "+v"(v)); }

__device__ __forceinline__ float dd_c(const float4& v, int s) {
  return s == 0 ? v.x : (s == 1 ? v.y : (s == 2 ? v.z : v.w));
}

// Sum the DD_WAVES partial tiles (2 x 16 values per lane) in fixed wave order; every
// thread then owns 8 of the tile's 2048 values: returns them with their (row, col).
struct DDTile { float v[8]; int row[8]; int col[8]; };

__device__ __forceinline__ DDTile dd_reduce(float* s_red, const dd_f32x16& a0, const dd_f32x16& a1) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // layout [wave][v = 0..31][lane]
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s_red[(w * 32 + r) * 64 + lane] = a0[r];
    s_red[(w * 32 + 16 + r) * 64 + lane] = a1[r];
  }
  __syncthreads();
  DDTile out;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int idx = t + q * DD_THREADS;          // 0..2047
    const int v = idx >> 6, ln = idx & 63;
    float s = s_red[(0 * 32 + v) * 64 + ln];
#pragma unroll
    for (int ww = 1; ww < DD_WAVES; ++ww) s += s_red[(ww * 32 + v) * 64 + ln];
    out.v[q] = s;
    out.row[q] = (v >> 4) * 32 + dd_row(v & 15, ln);
    out.col[q] = ln & 31;
  }
  return out;
}

// K range of wave w inside the workgroup's slice [k0, k1): contiguous, multiple of 8.
__device__ __forceinline__ void dd_wave_range(int k0, int k1, int& a, int& b) {
  const int w = threadIdx.x >> 6;
  const int n8 = (k1 - k0 + 7) >> 3;
  const int per = (n8 + DD_WAVES - 1) / DD_WAVES;
  a = min(k1, k0 + w * per * 8);
  b = min(k1, a + per * 8);
}

// ------------------------------------------------------------------ forward
struct DDFwd {
  const float* x; const float* w; const float* bias; float* y;
  int M, N, K, act; float alpha; int ksplit, kper;   // kper: K per workgroup (multiple of 8)
  int life_base;                                     // (diagnostics: first stamp slot)
};

// diagnostics: per-workgroup start / end of the forward (s_memrealtime, 100 MHz) at
// [base + 2 b], b the linear block index; base advances by 2 x grid per launch, so one
// buffer holds a step's two forwards (csa_dd_life_debug; scripts/mb/graph_life.py)
__constant__ long long* g_dd_life = nullptr;


// (Applying a producer's BatchNorm while loading A — from its statistic slab, or from a
// table the conv pair's last workgroup folded — was measured slower than the separate
// bn_act_apply launch in this 4-wave form, three times: profiles/r2_dense_direct.md,
// profiles/r3_notes.md.  The fourth attempt, on the 16-wave forward below
// (dd_fwd_wide_bn_kernel, round 14), is faster than the two launches: 10.3 us against
// 5.5 + 6.5 in the kernel trace, the step 1.8 % shorter — less than the launch boundary and
// bn_act_apply's span together, because the fused workgroup lives 7.2 us where the plain one
// lives 4.6: profiles/r14_notes.md.)
template <bool V4>
__device__ __forceinline__ void dd_fwd_body(const DDFwd& a, const int nt, const int mb, const int ks, float* s_red);


template <bool V4>
__global__ __launch_bounds__(DD_THREADS) void dd_fwd_kernel(DDFwd a) {
  __shared__ float s_red[DD_WAVES * 32 * 64];
  DD_STAMP(0);
  DD_SPAN_BEGIN();
  const long lb = blockIdx.x + (long)gridDim.x * (blockIdx.y + (long)gridDim.y * blockIdx.z);
  if (g_dd_life && threadIdx.x == 0) g_dd_life[2 * lb + 2 * a.life_base] = (long long)__builtin_amdgcn_s_memrealtime();
  dd_fwd_body<V4>(a, blockIdx.x, blockIdx.y, blockIdx.z, s_red);
  if (g_dd_life && threadIdx.x == 0) g_dd_life[2 * lb + 2 * a.life_base + 1] = (long long)__builtin_amdgcn_s_memrealtime();
  DD_STAMP(3);
  DD_SPAN_END();
}

// Grouped forward (round 6 prototype): G same-shape forwards of G packed
// jobs in ONE launch — blockIdx.z = job * ksplit + k-split, a per-job argument table.
constexpr int DD_GMAX = 16;
struct DDFwdGroup { DDFwd a[DD_GMAX]; int g, ks; };

template <bool V4>
__global__ __launch_bounds__(DD_THREADS) void dd_fwd_group_kernel(DDFwdGroup grp) {
  __shared__ float s_red[DD_WAVES * 32 * 64];
  const int j = (int)blockIdx.z / grp.ks, ks = (int)blockIdx.z - j * grp.ks;
  dd_fwd_body<V4>(grp.a[j], blockIdx.x, blockIdx.y, ks, s_red);
}

// ---------------------------------------------------------------------------------------
// Fused forward chain (round 6): fc1 forward -> fc2 forward -> head_dgrad as ONE launch.
// In the one-GPU step each of these was its own launch, and every boundary cost ~2-3 us
// between the last workgroup of one and the first of the next (scripts/mb/graph_life.py:
// the end-of-kernel write-back + the next dispatch).  Here the stages are blockIdx ranges
// [fc1 | fc2 | head]; dispatch is in order, so a stage's workgroups are all dispatched
// before any of the next, and a later stage's workgroup waits (bounded) on the earlier
// stage's ticket.  Both forwards are split-K with device-scope atomic outputs, so a
// workgroup's results are performed once its waves' atomics have returned (the barrier's
// s_waitcnt) — a relaxed ticket add after that barrier publishes them; the consumer's one
// agent-scope acquire after its poll invalidates its stale lines (the carrier's tail uses
// the same argument, conv_pair.hip).  A forward with one k-split (plain stores) releases
// before its ticket.  A timed-out wait (1 s) sets the error word and skips that
// workgroup's work (never a hung launch); the job's health check reads it.
// ---------------------------------------------------------------------------------------

constexpr int CH_LINE = 16;                          // words on their own 64-byte lines
constexpr int CH_GO = 16;                            // go-flag lines per stage (spread polling)
constexpr int CH_WORDS = (3 + 2 * CH_GO) * CH_LINE;  // counts [3] | go of fc2 [16] | go of head [16]
struct ChainArgs {
  DDFwd f[2];
  int n1, n2, n3;                                    // workgroups of fc1, fc2, head
  HeadDgradArgs h;
  unsigned* tk;                                      // [CH_WORDS] zero between launches
  int* err;
};

__device__ __forceinline__ unsigned* chain_go(unsigned* tk, int stage, int j) {
  return tk + (3 + stage * CH_GO + j) * CH_LINE;
}

// A waiting workgroup polls ITS go line (one of CH_GO per stage: hundreds of pollers on
// one word made every poll and the producers' atomics queue at that word's channel —
// measured: the stages started 15-20 us late), which the producing stage's last workgroup
// sets.
__device__ __forceinline__ bool chain_wait(unsigned* tk, int stage, int bid, int* err) {
  __shared__ int s_ok;
  if (threadIdx.x == 0) {
    const unsigned* go = chain_go(tk, stage, bid % CH_GO);
    const unsigned long long t0 = wall_clock64();
    int ok = 1;
    while (__hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      if (wall_clock64() - t0 > 100000000ull) {       // 1 s
        __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    s_ok = ok;
  }
  __syncthreads();
  return s_ok != 0;
}

// this workgroup's results are out (its waves' stores / atomics drained): count it
__device__ __forceinline__ unsigned chain_ticket(unsigned* tk, bool release) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __shared__ unsigned s_prev;
  if (threadIdx.x == 0) {
    if (release) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    s_prev = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return s_prev;
}

template <bool V4>
__device__ __forceinline__ void dd_fwd_body(const DDFwd& a, const int nt, const int mb, const int ks, float* s_red);

template <int KPT, int KQ>
__global__ __launch_bounds__(DD_THREADS) void fwd_chain_kernel(ChainArgs c) {
  __shared__ float s_red[DD_WAVES * 32 * 64];
  const int bid = (int)blockIdx.x;
  if (bid < c.n1 + c.n2) {
    const int st = bid < c.n1 ? 0 : 1;
    const DDFwd& a = c.f[st];
    const int lb = st ? bid - c.n1 : bid;
    bool go = true;
    if (st == 1) go = chain_wait(c.tk, 0, lb, c.err);
    if (g_dd_life && threadIdx.x == 0) g_dd_life[2 * (lb + a.life_base)] = (long long)__builtin_amdgcn_s_memrealtime();
    if (go) {
      const int ntile = (a.N + 31) / 32, mbn = (a.M + 63) / 64;
      dd_fwd_body<true>(a, lb % ntile, (lb / ntile) % mbn, lb / (ntile * mbn), s_red);
    }
    if (g_dd_life && threadIdx.x == 0) g_dd_life[2 * (lb + a.life_base) + 1] = (long long)__builtin_amdgcn_s_memrealtime();
    const unsigned prev = chain_ticket(c.tk + st * CH_LINE, a.ksplit == 1);
    if (threadIdx.x < CH_GO && prev == (unsigned)(st ? c.n2 : c.n1) - 1)   // the stage is done
      __hip_atomic_store(chain_go(c.tk, st, threadIdx.x), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int hb = bid - c.n1 - c.n2;
  if (chain_wait(c.tk, 1, hb, c.err)) head_dgrad_body<KPT, KQ>(c.h, hb);
  const unsigned prev = chain_ticket(c.tk + 2 * CH_LINE, false);
  if (threadIdx.x < 3 + 2 * CH_GO && prev == (unsigned)c.n3 - 1)   // every wait is over: reset
    __hip_atomic_store(c.tk + threadIdx.x * CH_LINE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool V4>
__device__ __forceinline__ void dd_fwd_body(const DDFwd& a, const int nt, const int mb, const int ks, float* s_red) {
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int n0 = nt * 32, m0 = mb * 64;
  const int kg0 = ks * a.kper, kg1 = min(a.K, kg0 + a.kper);
  int ka, kb;
  dd_wave_range(kg0, kg1, ka, kb);
  const int mA = min(m0 + i, a.M - 1), mB = min(m0 + 32 + i, a.M - 1);
  const float vA = m0 + i < a.M ? 1.f : 0.f, vB = m0 + 32 + i < a.M ? 1.f : 0.f;
  const int n = min(n0 + i, a.N - 1);
  const float* xa = a.x + (long)mA * a.K;
  const float* xb = a.x + (long)mB * a.K;
  float4 pa[DD_U], pb[DD_U];
  float bw[DD_U][4];
  // one group of DD_U 8-k blocks: every load in flight before the first MFMA
  auto load = [&](int k) {
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      const int kk = k + 8 * u + 4 * h;
      if (V4) {                    // branch-free: clamped float4 (terms past kb get B = 0)
        const int kc = min(kk, a.K - 4);
        pa[u] = *reinterpret_cast<const float4*>(xa + kc);
        pb[u] = *reinterpret_cast<const float4*>(xb + kc);
      } else {
        float t0[4], t1[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int kc = min(kk + s, a.K - 1);
          t0[s] = xa[kc];
          t1[s] = xb[kc];
        }
        pa[u] = make_float4(t0[0], t0[1], t0[2], t0[3]);
        pb[u] = make_float4(t1[0], t1[1], t1[2], t1[3]);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) bw[u][s] = a.w[(long)min(kk + s, a.K - 1) * a.N + n];
    }
  };
  load(ka);
  dd_f32x16 acc0 = {}, acc1 = {};
  for (int k = ka; k < kb; k += 8 * DD_U) {
    if (k != ka) load(k);
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      dd_pin4(pa[u]);
      dd_pin4(pb[u]);
#pragma unroll
      for (int s = 0; s < 4; ++s) dd_pin(bw[u][s]);
    }
    // the group's activation first, the MFMA chain after it
    float ta_[DD_U][4], tb_[DD_U][4];
#pragma unroll
    for (int u = 0; u < DD_U; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        ta_[u][s] = dd_c(pa[u], s);
        tb_[u][s] = dd_c(pb[u], s);
      }
    if (a.act != ACT_NONE) {
#pragma unroll
      for (int u = 0; u < DD_U; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          ta_[u][s] = act_fwd(ta_[u][s], a.act, a.alpha);
          tb_[u][s] = act_fwd(tb_[u][s], a.act, a.alpha);
        }
    }
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      const int kk0 = k + 8 * u + 4 * h;
      float* ta = ta_[u];
      float* tb = tb_[u];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int kk = kk0 + s;
        const float b = kk < kb ? bw[u][s] : 0.f;     // outside this wave's range: no term
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[s] * vA, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(tb[s] * vB, b, acc1, 0, 0, 0);
      }
    }
  }
  DD_STAMP(1);
  const DDTile t = dd_reduce(s_red, acc0, acc1);
  DD_STAMP(2);
  // the bias is read BEFORE the first atomic: vmcnt is in order, so a load issued after
  // an atomic waits for it (one serial round trip per element otherwise)
  const int nb_ = n0 + (threadIdx.x & 31);        // every value of a thread shares its column
  float bias = (a.bias && ks == 0) ? a.bias[min(nb_, a.N - 1)] : 0.f;
  dd_pin(bias);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int m = m0 + t.row[q], nn = n0 + t.col[q];
    if (m >= a.M || nn >= a.N) continue;
    const float v = t.v[q] + bias;
    float* p = a.y + (long)m * a.N + nn;
    if (a.ksplit > 1) atomicAdd(p, v); else *p = v;
  }
}

// ------------------------------------------------------------------ dgrad
struct DDDgrad {
  const float* dy; const float* w; float* dx;
  int M, F, N; int ksplit, kper;
  const float* x; int act; float alpha;            // forward input (pre transform) + act
  BNRef bn; float* bwd_slab;                       // bn.slab == null: no BatchNorm
};

template <bool V4>
__global__ __launch_bounds__(DD_THREADS) void dd_dgrad_kernel(DDDgrad a) {
  __shared__ float s_red[DD_WAVES * 32 * 64];
  __shared__ float s_bn[4 * DD_MAXC + 2 * DD_MAXC];
  __shared__ float s_acc[2 * DD_MAXC];
  DD_STAMP(0);
  DD_SPAN_BEGIN();
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int ft = blockIdx.x, mb = blockIdx.y, ks = blockIdx.z;
  const int f0 = ft * 32, m0 = mb * 64;
  const bool has_bn = a.bn.slab != nullptr;
  if (has_bn) {
    bn_reduce_to_lds(a.bn, s_bn, s_bn + DD_MAXC, s_bn + 2 * DD_MAXC, s_bn + 3 * DD_MAXC, s_bn + 4 * DD_MAXC);
    for (int c = threadIdx.x; c < 2 * DD_MAXC; c += DD_THREADS) s_acc[c] = 0.f;
  }
  const int kg0 = ks * a.kper, kg1 = min(a.N, kg0 + a.kper);
  int ka, kb;
  dd_wave_range(kg0, kg1, ka, kb);
  const int mA = min(m0 + i, a.M - 1), mB = min(m0 + 32 + i, a.M - 1);
  const float vA = m0 + i < a.M ? 1.f : 0.f, vB = m0 + 32 + i < a.M ? 1.f : 0.f;
  const int f = min(f0 + i, a.F - 1);
  const float* ya = a.dy + (long)mA * a.N;
  const float* yb = a.dy + (long)mB * a.N;
  const float* wr = a.w + (long)f * a.N;
  dd_f32x16 acc0 = {}, acc1 = {};
  for (int k = ka; k < kb; k += 8 * DD_U) {
    float4 pa[DD_U], pb[DD_U], pw[DD_U];
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      const int kk = k + 8 * u + 4 * h;
      if (V4) {                    // branch-free: clamped float4 (terms past kb get W = 0)
        const int kc = min(kk, a.N - 4);
        pa[u] = *reinterpret_cast<const float4*>(ya + kc);
        pb[u] = *reinterpret_cast<const float4*>(yb + kc);
        pw[u] = *reinterpret_cast<const float4*>(wr + kc);
      } else {
        float t0[4], t1[4], t2[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int kc = min(kk + s, a.N - 1);
          t0[s] = ya[kc];
          t1[s] = yb[kc];
          t2[s] = wr[kc];
        }
        pa[u] = make_float4(t0[0], t0[1], t0[2], t0[3]);
        pb[u] = make_float4(t1[0], t1[1], t1[2], t1[3]);
        pw[u] = make_float4(t2[0], t2[1], t2[2], t2[3]);
      }
    }
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      dd_pin4(pa[u]);
      dd_pin4(pb[u]);
      dd_pin4(pw[u]);
    }
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float w = k + 8 * u + 4 * h + s < kb ? dd_c(pw[u], s) : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(dd_c(pa[u], s) * vA, w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(dd_c(pb[u], s) * vB, w, acc1, 0, 0, 0);
      }
    }
  }
  DD_STAMP(1);
  const DDTile t = dd_reduce(s_red, acc0, acc1);
  DD_STAMP(2);
  // epilogue: forward inputs first (all loads in flight), then the transform backward
  const int C = has_bn ? a.bn.C : 1;
  float xv[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int m = min(m0 + t.row[q], a.M - 1), ff = min(f0 + t.col[q], a.F - 1);
    xv[q] = (a.x && (a.act != ACT_NONE || has_bn)) ? a.x[(long)m * a.F + ff] : 0.f;
  }
  float sd = 0.f, sdx = 0.f;
  const int ff = f0 + (threadIdx.x & 31);         // every value of a thread shares its column
  const int ch = has_bn ? ff % C : 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int m = m0 + t.row[q];
    if (m >= a.M || ff >= a.F) continue;
    float d = t.v[q];
    if (a.act != ACT_NONE || has_bn) {
      const float z = has_bn ? xv[q] * s_bn[2 * DD_MAXC + ch] + s_bn[3 * DD_MAXC + ch] : xv[q];
      d = act_bwd(d, z, act_fwd(z, a.act, a.alpha), a.act, a.alpha);   // linear in the partial
      if (has_bn) {
        sd += d;
        sdx += d * (xv[q] - s_bn[ch]) * s_bn[DD_MAXC + ch];
      }
    }
    float* p = a.dx + (long)m * a.F + ff;
    if (a.ksplit > 1) atomicAdd(p, d); else *p = d;
  }
  if (has_bn) {
    if (ff < a.F) {
      atomicAdd(&s_acc[ch], sd);
      atomicAdd(&s_acc[DD_MAXC + ch], sdx);
    }
    __syncthreads();
    float* row = a.bwd_slab + (size_t)(((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) % DD_SLAB_ROWS) * 2 * C;
    for (int c = threadIdx.x; c < 2 * C; c += DD_THREADS)
      atomicAdd(&row[c], s_acc[c < C ? c : DD_MAXC + c - C]);
  }
  DD_STAMP(3);
  DD_SPAN_END();
}

// ------------------------------------------------------------------ wgrad (+ update)
// One wave: 32 features x 32 outputs, K = batch in steps of 2 (2x the waves of a 32x64
// tile: at one wave per SIMD every memory round trip is exposed, so parallelism wins
// over A-fragment reuse, which L2 serves anyway).  Workgroup = 4 waves along the output
// dimension (128 columns).
struct DDWgrad {
  const float* x; const float* dy; int M, F, N; int act; float alpha; float gscale;
  float* dw; float* db;                         // store mode (opt < 0)
  float* w; float* b; float* sw0; float* sw1; float* sb0; float* sb1;   // update mode
  int opt; float lr; const int64_t* step;
  int ftiles, ntiles;                           // ntiles: 128-column groups
  LrSched sched;                                // learning-rate schedule (all-zero: constant)
};

constexpr int DD_KC = 32;   // MFMA k-steps (x2 batch rows) per register chunk

__global__ __launch_bounds__(DD_THREADS) void dd_wgrad_kernel(DDWgrad a) {
  DD_STAMP(0);
  DD_SPAN_BEGIN();
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5, w = threadIdx.x >> 6;
  const int nw = a.ftiles * a.ntiles;
  if ((int)blockIdx.x >= nw) {
    // bias blocks: 64 columns x 4 batch quarters per block, all loads of a thread in
    // flight at once, quarters summed in LDS in fixed order
    __shared__ float s_b[DD_WAVES][64];
    const int n = ((int)blockIdx.x - nw) * 64 + lane;
    const int nc = min(n, a.N - 1);
    const int per = (a.M + DD_WAVES - 1) / DD_WAVES;
    const int m0 = w * per;
    float v[16];
    float g = 0.f;
    for (int c = 0; c < per; c += 16) {
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = a.dy[(long)min(m0 + c + u, a.M - 1) * a.N + nc];
#pragma unroll
      for (int u = 0; u < 16; ++u) dd_pin(v[u]);
#pragma unroll
      for (int u = 0; u < 16; ++u) g += (c + u < per && m0 + c + u < a.M) ? v[u] : 0.f;
    }
    s_b[w][lane] = g;
    __syncthreads();
    if (w != 0 || n >= a.N) return;
    g = (s_b[0][lane] + s_b[1][lane] + s_b[2][lane] + s_b[3][lane]) * a.gscale;
    if (a.opt < 0) {
      a.db[n] = g;
    } else {
      const float lr = opt_step_lr(a.opt, a.lr, a.step, a.sched);
      float wv = a.b[n], s0 = a.sb0 ? a.sb0[n] : 0.f, s1 = a.sb1 ? a.sb1[n] : 0.f;
      opt_update(a.opt, lr, wv, g, s0, s1);
      a.b[n] = wv;
      if (a.sb0) a.sb0[n] = s0;
      if (a.sb1) a.sb1[n] = s1;
    }
    return;
  }
  const int ft = (int)blockIdx.x / a.ntiles, ng = (int)blockIdx.x % a.ntiles;
  const int f0 = ft * 32, n0 = ng * 128 + w * 32;
  if (n0 >= a.N) return;
  const int f = min(f0 + i, a.F - 1);
  const int nn = n0 + i, nc = min(nn, a.N - 1);
  // update mode: this lane's 16 weights and slots are requested BEFORE the K loop, so
  // their HBM latency overlaps the gradient GEMM
  const bool upd = a.opt >= 0;
  const int ns = upd ? opt_nslots(a.opt) : 0;
  float wv[16], s0[16], s1[16];
  if (upd) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long idx = (long)min(f0 + dd_row(r, lane), a.F - 1) * a.N + nc;
      wv[r] = a.w[idx];
      s0[r] = ns > 0 ? a.sw0[idx] : 0.f;
      s1[r] = ns > 1 ? a.sw1[idx] : 0.f;
    }
  }
  dd_f32x16 acc = {};
  for (int c0 = 0; c0 < a.M; c0 += 2 * DD_KC) {
    float xa[DD_KC], ya[DD_KC];
#pragma unroll
    for (int s = 0; s < DD_KC; ++s) {
      const int m = min(c0 + 2 * s + h, a.M - 1);
      xa[s] = a.x[(long)m * a.F + f];
      ya[s] = a.dy[(long)m * a.N + nc];
    }
#pragma unroll
    for (int s = 0; s < DD_KC; ++s) {
      dd_pin(xa[s]);
      dd_pin(ya[s]);
    }
#pragma unroll
    for (int s = 0; s < DD_KC; ++s) {
      if (c0 + 2 * s >= a.M) break;              // wave-uniform
      const float ok = c0 + 2 * s + h < a.M ? 1.f : 0.f;
      float xv = a.act != ACT_NONE ? act_fwd(xa[s], a.act, a.alpha) : xa[s];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv * ok, ya[s], acc, 0, 0, 0);
    }
  }
  DD_STAMP(1);
  // epilogue: D[row f][col n]; lanes 0-31 consecutive columns (coalesced rows of W)
  if (!upd) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ff = f0 + dd_row(r, lane);
      if (ff < a.F && nn < a.N) a.dw[(long)ff * a.N + nn] = acc[r] * a.gscale;
    }
    return;
  }
  const float lr = opt_step_lr(a.opt, a.lr, a.step, a.sched);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dd_pin(wv[r]);
    dd_pin(s0[r]);
    dd_pin(s1[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ff = f0 + dd_row(r, lane);
    if (ff >= a.F || nn >= a.N) continue;
    const long idx = (long)ff * a.N + nn;
    opt_update(a.opt, lr, wv[r], acc[r] * a.gscale, s0[r], s1[r]);
    a.w[idx] = wv[r];
    if (ns > 0) a.sw0[idx] = s0[r];
    if (ns > 1) a.sw1[idx] = s1[r];
  }
  DD_STAMP(3);
  DD_SPAN_END();
}

// ------------------------------------------------------------------ forward, 16 waves
// The one-GPU training forward (round 12).  dd_fwd_kernel folds 4 waves before it emits, so
// fc1 (K = 3920, 31 K slices) added 31 x [50][512] floats into Y with atomics, and global
// float atomics run at one chip-wide rate whatever issues them.  Here sixteen waves fold on
// chip first: a quarter of the atomic bytes.
//
//   workgroup  1024 threads, one per (32-column tile, 32-row batch block, K slice); the
//              linear block index is (mb * ksplit + ks) * ntile + nt, so the batch blocks of
//              one (tile, slice), which read the same W, lie ntile * ksplit blocks apart
//              (fc1: 128, the same XCD under round-robin placement; for speed only).
//   wave       a contiguous k range of the slice, a multiple of 8 (fc1: 32 k), ONE 32x32
//              accumulator.  Fragments and the float4-over-4-steps trick as in dd_fwd_body.
//              A group (DD_U 8-k blocks) is requested whole before its first MFMA; a further
//              group of the range lands under the current group's MFMAs.  8-k blocks past
//              the range are neither loaded nor multiplied; addresses are clamped into the
//              operands and the terms of a cut last block get B = 0.  Batch rows >= M read a
//              clamped (valid) row: a row of Y depends on its own row of X only, and those
//              rows are never written.
//   fold       the 16 tiles meet in LDS once as [wave][reg][lane] (64 KB, conflict-free both
//              ways); wave r then sums register r over the waves in wave order, adds the
//              bias (K slice 0) and emits it: two 128-byte row segments per instruction,
//              atomicAdd when the launch has more than one K slice, a plain store otherwise.
//
// (A wave keeping both 32-row sub-tiles - a 64x32 tile per workgroup, W read once, fc1 as
// 16 tiles x 16 slices with twice the atomic bytes - was measured slower in the step:
// 0.0649-0.0652 against 0.0637-0.0639 ms, profiles/r12_notes.md.)
constexpr int DW_WAVES = 16;
constexpr int DW_THREADS = 64 * DW_WAVES;
constexpr size_t DW_LDS = (size_t)DW_WAVES * 16 * 64 * sizeof(float);

struct DWGroup { float4 x[DD_U]; float b[DD_U][4]; };

// The BN form (round 14): X is the producer's raw output, and the launch applies
// xt = act(x * a[c] + b[c]), c = k % C, to the A fragments in registers, where bn_act_apply was
// a launch of its own in front of this one.
//   table      2C threads (lanes 2c, 2c + 1: sum x, sum x^2 of channel c) ask for their slab column
//              BEFORE the operand loads (loads return in order: behind them the fold would wait
//              for W) and add the rows in row order; the even lane derives mean / rstd / a / b
//              with bn_reduce_to_lds's formulas and writes them to LDS; ONE barrier, the operand
//              loads in flight across it.  No atomics: every workgroup of the launch derives the
//              same bits, so the sixteen column tiles that transform an element agree with the
//              one that stores it.
//   transform  a whole load group in registers before its MFMAs; X is requested ahead of W so
//              the transform runs under W's flight.  The channel of a lane's first k comes from
//              one FastDiv, then add-and-wrap.
//   xt         every column tile holds the same (batch block, K slice, wave) chunk: tile nt
//              stores the chunks of the waves w with w % min(ntile, 16) == nt, after the group's
//              MFMAs, rows < M and k < K only.
//   tab, flag  workgroup 0 writes [4][C] mean | rstd | a | b and zeroes the pending flag, as
//              bn_act_apply's block 0 did.
struct DDFwdBN {
  BNRef bn; float* xt; float* tab; unsigned* clear;
  FastDiv dc; int step8;                                              // k % C; 8 % C
};
constexpr int DW_SU = 32;                                             // slab rows in flight per thread

template <bool BN>
__device__ __forceinline__ void dd_fwd_wide_body(DDFwd a, int ntile, const DDFwdBN q, float* s_part,
                                                 float2* s_ab, float* s_mr) {
  DD_STAMP(0);
  DD_SPAN_BEGIN();
  const int lb = (int)blockIdx.x, tid = threadIdx.x;
  if (g_dd_life && tid == 0) g_dd_life[2 * lb + 2 * a.life_base] = (long long)__builtin_amdgcn_s_memrealtime();
  const int lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = lb % ntile, ks = (lb / ntile) % a.ksplit, mb = lb / (ntile * a.ksplit);
  const int n0 = nt * 32, m0 = mb * 32;
  // this wave's k range [ka, kb) inside the slice
  const int kg0 = ks * a.kper, kg1 = min(a.K, kg0 + a.kper);
  const int per = (((kg1 - kg0 + 7) >> 3) + DW_WAVES - 1) / DW_WAVES;
  const int ka = min(kg1, kg0 + wave * per * 8), kb = min(kg1, ka + per * 8);
  const float* xr = a.x + (long)min(m0 + i, a.M - 1) * a.K;
  const float* wc = a.w + min(n0 + i, a.N - 1);
  // the epilogue's bias, requested with the operands (a load issued behind an atomic waits for it)
  const int er = wave;                                                // the register this wave emits
  float bias = (a.bias && ks == 0) ? a.bias[min(n0 + i, a.N - 1)] : 0.f;

  // BN: this thread's slab column (the last DW_SU rows stay in flight across the operand loads)
  float sv[DW_SU], ssum = 0.f, sco = 0.f;
  int srow = 0;
  const int C = BN ? q.bn.C : 1;
  if constexpr (BN) {
    if (tid < 2 * C) {
      const int c = tid >> 1;
      sco = (tid & 1) ? q.bn.offset[c] : q.bn.scale[c];
      const float* col = q.bn.slab + (tid & 1) * C + c;
      for (; srow + DW_SU < q.bn.nslab; srow += DW_SU) {              // (slabs of more than DW_SU rows)
#pragma unroll
        for (int u = 0; u < DW_SU; ++u) sv[u] = col[(size_t)(srow + u) * 2 * C];
#pragma unroll
        for (int u = 0; u < DW_SU; ++u) dd_pin(sv[u]);
#pragma unroll
        for (int u = 0; u < DW_SU; ++u) ssum += sv[u];
      }
#pragma unroll
      for (int u = 0; u < DW_SU; ++u) sv[u] = col[(size_t)min(srow + u, q.bn.nslab - 1) * 2 * C];
    }
    asm volatile("" ::: "memory");                                    // the operands are requested behind these
  }

  auto load = [&](DWGroup& g, int k) {
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      if (k + 8 * u >= kb) break;                                     // wave-uniform
      const int kk = k + 8 * u + 4 * h;                               // K % 4 == 0: kk < K <=> kk <= K - 4
      g.x[u] = *reinterpret_cast<const float4*>(xr + min(kk, a.K - 4));
#pragma unroll
      for (int s = 0; s < 4; ++s) g.b[u][s] = wc[(long)min(kk + s, a.K - 1) * a.N];
    }
  };
  // BN: a whole group whatever the range (addresses are clamped into the operands), X ahead
  // of W: a fixed number of loads behind the slab's, so the fold waits for the slab alone
  auto load_all = [&](DWGroup& g, int k) {
#pragma unroll
    for (int u = 0; u < DD_U; ++u)
      g.x[u] = *reinterpret_cast<const float4*>(xr + min(k + 8 * u + 4 * h, a.K - 4));
#pragma unroll
    for (int u = 0; u < DD_U; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) g.b[u][s] = wc[(long)min(k + 8 * u + 4 * h + s, a.K - 1) * a.N];
  };
  dd_f32x16 acc = {};
  auto mac = [&](DWGroup& g, int k) {
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      if (k + 8 * u >= kb) break;                                     // wave-uniform
      dd_pin4(g.x[u]);
#pragma unroll
      for (int s = 0; s < 4; ++s) dd_pin(g.b[u][s]);
      float xv[4] = {g.x[u].x, g.x[u].y, g.x[u].z, g.x[u].w};
      if (a.act != ACT_NONE) {
#pragma unroll
        for (int s = 0; s < 4; ++s) xv[s] = act_fwd(xv[s], a.act, a.alpha);
      }
      const bool in = k + 8 * u + 4 * h < kb;                         // kb % 4 == 0: one test for the 4 steps
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[s], in ? g.b[u][s] : 0.f, acc, 0, 0, 0);
    }
  };
  // BN: the group's X becomes xt in place (terms outside the range: 0), then the MFMA chain
  int cu = 0;                                                         // channel of this lane's next 8-k block
  auto mac_bn = [&](DWGroup& g, int k) {
#pragma unroll
    for (int u = 0; u < DD_U; ++u) dd_pin4(g.x[u]);
    DD_PHASE(2);
    // (branch-free over the whole group: a block past the range holds clamped, valid data)
    float z[DD_U][4];
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      int c = cu;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float2 ab = s_ab[c];
        z[u][s] = dd_c(g.x[u], s) * ab.x + ab.y;
        c = (c + 1 == C) ? 0 : c + 1;
      }
      cu += q.step8;
      cu = cu >= C ? cu - C : cu;
    }
    // one branch on the activation for the group (act_fwd's own switch, per value, is a
    // chain of scalar branches in front of every v_exp)
#define DD_ACT_GROUP(ACT)                                                                     \
  _Pragma("unroll") for (int u = 0; u < DD_U; ++u)                                            \
  _Pragma("unroll") for (int s = 0; s < 4; ++s) z[u][s] = act_fwd(z[u][s], ACT, a.alpha)
    switch (a.act) {
      case ACT_SIGMOID: DD_ACT_GROUP(ACT_SIGMOID); break;
      case ACT_RELU: DD_ACT_GROUP(ACT_RELU); break;
      case ACT_LEAKY: DD_ACT_GROUP(ACT_LEAKY); break;
      default: break;
    }
#undef DD_ACT_GROUP
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      const bool in = k + 8 * u + 4 * h < kb;
#pragma unroll
      for (int s = 0; s < 4; ++s) dd_pin(z[u][s]);
      g.x[u] = make_float4(in ? z[u][0] : 0.f, in ? z[u][1] : 0.f, in ? z[u][2] : 0.f, in ? z[u][3] : 0.f);
    }
    DD_PHASE(3);
#ifdef CSA_DD_PHASES
#pragma unroll
    for (int u = 0; u < DD_U; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) dd_pin(g.b[u][s]);
    DD_PHASE(4);
#endif
#pragma unroll
    for (int u = 0; u < DD_U; ++u) {
      if (k + 8 * u >= kb) break;                                     // wave-uniform
#pragma unroll
      for (int s = 0; s < 4; ++s) dd_pin(g.b[u][s]);
      const bool in = k + 8 * u + 4 * h < kb;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dd_c(g.x[u], s), in ? g.b[u][s] : 0.f, acc, 0, 0, 0);
    }
  };
  if constexpr (BN) {
    DWGroup cur, nxt;
    DD_PHASE(0);
    load_all(cur, ka);
    // the table: rows in row order, lanes 2c / 2c + 1 meet, the even lane derives channel c
    if (tid < 2 * C) {
#pragma unroll
      for (int u = 0; u < DW_SU; ++u) dd_pin(sv[u]);
#pragma unroll
      for (int u = 0; u < DW_SU; ++u) ssum += srow + u < q.bn.nslab ? sv[u] : 0.f;
    }
    const float osum = __shfl_xor(ssum, 1, 64), oco = __shfl_xor(sco, 1, 64);
    if (tid < 2 * C && !(tid & 1)) {
      const int c = tid >> 1;
      float mean = ssum / q.bn.count;
      float var = fmaxf(osum / q.bn.count - mean * mean, 0.f);
      float rstd = rsqrtf(var + q.bn.eps);
      float sa = sco * rstd;
      s_mr[c] = mean;
      s_mr[DD_MAXC + c] = rstd;
      s_ab[c] = make_float2(sa, oco - mean * sa);
    }
    __syncthreads();
    DD_PHASE(1);
    if (lb == 0) {
      if (q.clear && tid == 0) *q.clear = 0u;
      if (q.tab && tid < C) {
        const float2 ab = s_ab[tid];
        q.tab[tid] = s_mr[tid];
        q.tab[C + tid] = s_mr[DD_MAXC + tid];
        q.tab[2 * C + tid] = ab.x;
        q.tab[3 * C + tid] = ab.y;
      }
    }
    int qq;
    q.dc.divmod(ka + 4 * h, qq, cu);
    // this wave's chunk of xt goes out from one column tile
    const bool put_ok = nt == wave % min(ntile, DW_WAVES) && m0 + i < a.M;
    float* xo = q.xt + (long)min(m0 + i, a.M - 1) * a.K;
    auto put = [&](DWGroup& g, int k) {
#pragma unroll
      for (int u = 0; u < DD_U; ++u) {
        if (k + 8 * u >= kb) break;                                   // wave-uniform
        const int kk = k + 8 * u + 4 * h;
        if (put_ok && kk < kb) *reinterpret_cast<float4*>(xo + kk) = g.x[u];
      }
    };
    for (int k = ka; k < kb; k += 8 * DD_U) {
      const bool more = k + 8 * DD_U < kb;                            // wave-uniform
      if (more) load_all(nxt, k + 8 * DD_U);
      mac_bn(cur, k);
      put(cur, k);
      DD_PHASE(5);
      if (more) cur = nxt;
    }
  } else if (ka < kb) {                                               // wave-uniform (K slice shorter than 16 ranges)
    DWGroup cur, nxt;
    load(cur, ka);
    for (int k = ka;; k += 8 * DD_U) {
      if (k + 8 * DD_U < kb) {
        load(nxt, k + 8 * DD_U);
        mac(cur, k);
        cur = nxt;
      } else {
        mac(cur, k);
        break;
      }
    }
  }
  DD_STAMP(1);
  dd_pin(bias);
#pragma unroll
  for (int r = 0; r < 16; ++r) s_part[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  float v = bias;
  {
    const float* src = s_part + er * 64 + lane;
    float s = src[0];
#pragma unroll
    for (int w = 1; w < DW_WAVES; ++w) s += src[w * 16 * 64];
    v += s;
  }
  DD_STAMP(2);
  const int m = m0 + dd_row(er, lane), nn = n0 + i;
  if (m < a.M && nn < a.N) {
    float* p = a.y + (long)m * a.N + nn;
    if (a.ksplit > 1) atomicAdd(p, v); else *p = v;
  }
  if (g_dd_life && tid == 0) g_dd_life[2 * lb + 2 * a.life_base + 1] = (long long)__builtin_amdgcn_s_memrealtime();
  DD_STAMP(3);
  DD_SPAN_END();
}

__global__ __launch_bounds__(DW_THREADS) void dd_fwd_wide_kernel(DDFwd a, int ntile) {
  extern __shared__ __attribute__((aligned(16))) float s_part[];      // [wave][reg][lane]
  dd_fwd_wide_body<false>(a, ntile, DDFwdBN{}, s_part, nullptr, nullptr);
}

__global__ __launch_bounds__(DW_THREADS) void dd_fwd_wide_bn_kernel(DDFwd a, int ntile, DDFwdBN q) {
  extern __shared__ __attribute__((aligned(16))) float s_part[];      // [wave][reg][lane]
  __shared__ float2 s_ab[DD_MAXC];                                    // (a, b) of channel c
  __shared__ float s_mr[2 * DD_MAXC];                                 // mean | rstd
  dd_fwd_wide_body<true>(a, ntile, q, s_part, s_ab, s_mr);
}

// K slices: enough workgroups for ~1 wave per SIMD (1024), each wave >= 16 k.
static int dd_splits(int tiles, int K) {
  if (g_csa_det) return 1;                 // deterministic mode: whole-K outputs, plain stores
  // waves per launch: swept 512 / 1024 / 2048 / 4096 -> graph step 125.4 / 120.3 / 119.5 / 122.5 us
  static const int target = [] {                   // (CSA_DD_TARGET: A/B knob)
    const char* e = std::getenv("CSA_DD_TARGET");
    const int v = e ? std::atoi(e) : 2048;
    return v >= 256 && v <= 16384 ? v : 2048;
  }();
  int ks = (target / DD_WAVES + tiles - 1) / tiles;
  const int maxks = (K + 8 * DD_WAVES * 2 - 1) / (8 * DD_WAVES * 2);   // >= 16 k per wave
  ks = ks < 1 ? 1 : ks;
  ks = ks > maxks ? maxks : ks;
  return ks < 1 ? 1 : ks;
}

static int dd_kper(int K, int ks) { return (((K + ks - 1) / ks) + 7) & ~7; }

// The forward's launch form: dd_fwd_wide_kernel (16-wave workgroups) in the one-process-per-GPU
// atomic profile, dd_fwd_kernel everywhere else.  Deterministic mode keeps its whole-K 4-wave
// form (its sums must not move); the packed and the shared-GPU profile keep 256-thread
// workgroups for the reasons written at du_cs (dense_update.hip).
//   CSA_DD_WIDE=0: dd_fwd_kernel everywhere (A/B knob)
//   CSA_DD_WIDE=1: the wide kernel in the packed profile too (A/B knob)
static bool dd_wide(int K) {
  static const int wide_env = [] { const char* e = std::getenv("CSA_DD_WIDE"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
  if (wide_env == 0 || g_csa_det || g_csa_shared || (g_csa_packed && wide_env != 1)) return false;
  return K % 4 == 0;
}

struct DDPlan { bool wide; int ks, kper; };

// K slices of the wide kernel: one workgroup per CU (256) for the shape's tiles, every wave
// of a slice >= 8 k.  fc1: 16 tiles x 2 batch blocks x 8 slices; fc2 (K = 512): 4 slices,
// swept in the graph at 1 / 2 / 4 -> workgroup life 4.30 / 2.63 / 2.05 us (dd_fwd_kernel:
// 3.60), profiles/r12_notes.md.  (CSA_DD_WIDE_KS caps the slices of every wide launch: the
// A/B knob of that sweep.)
static DDPlan dd_fwd_plan(int M, int N, int K) {
  DDPlan p;
  p.wide = dd_wide(K);
  if (p.wide) {
    static const int cap = [] { const char* e = std::getenv("CSA_DD_WIDE_KS"); return e ? std::atoi(e) : 0; }();
    const int tiles = ((N + 31) / 32) * ((M + 31) / 32);
    const int maxks = K / (8 * DW_WAVES);
    p.ks = 256 / tiles;
    p.ks = p.ks > maxks ? maxks : p.ks;
    p.ks = cap > 0 && p.ks > cap ? cap : p.ks;
    p.ks = p.ks < 1 ? 1 : p.ks;
  } else {
    p.ks = dd_splits(((N + 31) / 32) * ((M + 63) / 64), K);
  }
  p.kper = dd_kper(K, p.ks);
  p.ks = (K + p.kper - 1) / p.kper;
  return p;
}

}  // namespace csa

using namespace csa;

CSA_API int csa_dd_life_debug(long long* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dd_life), &p, sizeof(p));
}

CSA_API int csa_dd_debug(long long* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dd_dbg), &p, sizeof(p));
}

CSA_API int csa_dd_fwd_splits(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 1;
  return dd_fwd_plan(M, N, K).ks;
}

// 1 when csa_dd_fwd runs this shape as dd_fwd_wide_kernel under the current profile flags
CSA_API int csa_dd_fwd_wide(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return dd_fwd_plan(M, N, K).wide ? 1 : 0;
}

// Forward chain recording: between csa_chain_begin and csa_chain_end, the two forwards and
// the head_dgrad this thread issues are recorded, then launched as fwd_chain_kernel.
namespace csa { thread_local HDRecord g_hd_rec{}; }
static thread_local int g_chain_on = 0, g_chain_n = 0;
static thread_local DDFwd g_chain_f[2];
CSA_API void csa_chain_begin() { g_chain_on = 1; g_chain_n = 0; g_hd_rec.on = 1; g_hd_rec.has = 0; }
CSA_API void csa_chain_reset() { g_chain_on = 0; g_chain_n = 0; g_hd_rec.on = 0; g_hd_rec.has = 0; }
CSA_API int csa_chain_ok(int kh) { return kh == 256 || kh == 512 || kh == 1024 ? 1 : 0; }
// tk: csa_chain_words() zeroed uint32 (device), err: 1 int (device)
CSA_API int csa_chain_words() { return CH_WORDS; }
CSA_API int csa_chain_end(unsigned* tk, int* err, hipStream_t st) {
  const int n = g_chain_n, has = g_hd_rec.has, kq = g_hd_rec.kq;
  const HeadDgradArgs h = g_hd_rec.a;
  csa_chain_reset();
  if (n != 2 || !has || !tk || !err) return -1;
  ChainArgs c{};
  for (int j = 0; j < 2; ++j) {
    const DDFwd& a = g_chain_f[j];
    if (a.K % 4) return -2;
    c.f[j] = a;
  }
  c.n1 = ((c.f[0].N + 31) / 32) * ((c.f[0].M + 63) / 64) * c.f[0].ksplit;
  c.n2 = ((c.f[1].N + 31) / 32) * ((c.f[1].M + 63) / 64) * c.f[1].ksplit;
  c.n3 = ((h.M + HD_R - 1) / HD_R) * ((h.K1 + HD_FS - 1) / HD_FS);
  c.h = h; c.tk = tk; c.err = err;
  const dim3 grid((unsigned)(c.n1 + c.n2 + c.n3)), blk(DD_THREADS);
  static_assert(DD_THREADS == HD_T, "one block shape for every stage");
  if (kq == 4) hipLaunchKernelGGL((fwd_chain_kernel<1, 4>), grid, blk, 0, st, c);
  else if (kq == 8) hipLaunchKernelGGL((fwd_chain_kernel<2, 8>), grid, blk, 0, st, c);
  else if (kq == 16) hipLaunchKernelGGL((fwd_chain_kernel<4, 16>), grid, blk, 0, st, c);
  else return -3;
  return (int)hipGetLastError();
}

CSA_API int csa_chain_head_debug(long long* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_hd_dbg), &p, sizeof(p));
}

// Grouping (prototype): between csa_dd_group_begin and csa_dd_group_end the forwards this
// thread issues are recorded instead of launched, then run as ONE launch (same shapes).
static thread_local DDFwdGroup g_dd_group{};
static thread_local bool g_dd_grouping = false;
CSA_API void csa_dd_group_begin() { g_dd_grouping = true; g_dd_group.g = 0; }
CSA_API int csa_dd_group_end(hipStream_t st) {
  g_dd_grouping = false;
  const int G = g_dd_group.g;
  if (G == 0) return 0;
  const DDFwd& a0 = g_dd_group.a[0];
  for (int j = 1; j < G; ++j) {
    const DDFwd& a = g_dd_group.a[j];
    if (a.M != a0.M || a.N != a0.N || a.K != a0.K || a.ksplit != a0.ksplit || a.kper != a0.kper) return -2;
  }
  g_dd_group.ks = a0.ksplit;
  const dim3 grid((a0.N + 31) / 32, (a0.M + 63) / 64, a0.ksplit * G);
  if (a0.K % 4 == 0) hipLaunchKernelGGL(dd_fwd_group_kernel<true>, grid, dim3(DD_THREADS), 0, st, g_dd_group);
  else hipLaunchKernelGGL(dd_fwd_group_kernel<false>, grid, dim3(DD_THREADS), 0, st, g_dd_group);
  g_dd_group.g = 0;
  return (int)hipGetLastError();
}

// Y[M][N] (+)= act(X)[M][K] . W[K][N] + bias.  Y must be zeroed when splits > 1.
CSA_API int csa_dd_fwd(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K,
                       int act, float alpha, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0) return -1;
  const int nt = (N + 31) / 32, mb = (M + 63) / 64;
  // (a recorded chain or group runs dd_fwd_body with the planned slices: csa_dd_fwd_splits
  // has told the caller whether Y starts at zero)
  const DDPlan plan = dd_fwd_plan(M, N, K);
  const int ks = plan.ks, kper = plan.kper;
  DDFwd a{X, W, bias, Y, M, N, K, act, alpha, ks, kper, 0};
  a.life_base = K > 1024 ? 0 : 4096;                 // (diagnostics: wide layers first)
  if (g_chain_on) {
    if (g_chain_n >= 2) return -4;
    g_chain_f[g_chain_n++] = a;
    return 0;
  }
  if (g_dd_grouping) {
    if (g_dd_group.g >= DD_GMAX) return -3;
    g_dd_group.a[g_dd_group.g++] = a;
    return 0;
  }
  if (plan.wide) {
    static const bool attr = hipFuncSetAttribute((const void*)dd_fwd_wide_kernel,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_LDS) == hipSuccess;
    (void)attr;
    const unsigned blocks = (unsigned)(nt * ((M + 31) / 32) * ks);
    hipLaunchKernelGGL(dd_fwd_wide_kernel, dim3(blocks), dim3(DW_THREADS), DW_LDS, st, a, nt);
  } else if (K % 4 == 0) hipLaunchKernelGGL(dd_fwd_kernel<true>, dim3(nt, mb, ks), dim3(DD_THREADS), 0, st, a);
  else hipLaunchKernelGGL(dd_fwd_kernel<false>, dim3(nt, mb, ks), dim3(DD_THREADS), 0, st, a);
  return (int)hipGetLastError();
}

// 1 when csa_dd_fwd_bn takes this shape: it runs wide under the calling thread's profile flags
// and the producer's channels divide K (channel of k = k % C, NHWC flattened).
CSA_API int csa_dd_fwd_bn_ok(int M, int N, int K, int C) {
  if (M <= 0 || N <= 0 || K <= 0 || C <= 0 || C > DD_MAXC) return 0;
  if (K % 4 != 0 || K % C != 0) return 0;
  return dd_fwd_plan(M, N, K).wide ? 1 : 0;
}

// csa_bn_act_apply + csa_dd_fwd in one launch (dd_fwd_wide_bn_kernel):
//   xt[M][K] = act(X * a[c] + b[c]), Y[M][N] (+)= xt . W + bias
// with (a, b) from the BatchNorm forward slab; tab (optional) gets [4][C] mean | rstd | a | b,
// *clear (optional: the carried update's pending flag) gets 0.  Y zeroed when splits > 1.
// Never part of a recorded chain or group.
CSA_API int csa_dd_fwd_bn(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K,
                          int C, const float* bn_slab, int bn_nslab, float bn_count, float bn_eps,
                          const float* bn_scale, const float* bn_offset, int act, float alpha,
                          float* xt, float* tab, unsigned* clear, hipStream_t st) {
  if (!csa_dd_fwd_bn_ok(M, N, K, C) || !X || !xt || !bn_slab || bn_nslab <= 0 || !bn_scale || !bn_offset) return -1;
  if (g_chain_on || g_dd_grouping) return -5;
  const DDPlan plan = dd_fwd_plan(M, N, K);
  DDFwd a{X, W, bias, Y, M, N, K, act, alpha, plan.ks, plan.kper, 0};
  a.life_base = K > 1024 ? 0 : 4096;                 // (diagnostics: wide layers first)
  DDFwdBN q{BNRef{bn_slab, bn_nslab, C, bn_count, bn_eps, bn_scale, bn_offset}, xt, tab, clear, FastDiv(C), 8 % C};
  static const bool attr = hipFuncSetAttribute((const void*)dd_fwd_wide_bn_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)DW_LDS) == hipSuccess;
  (void)attr;
  const int nt = (N + 31) / 32;
  const unsigned blocks = (unsigned)(nt * ((M + 31) / 32) * plan.ks);
  hipLaunchKernelGGL(dd_fwd_wide_bn_kernel, dim3(blocks), dim3(DW_THREADS), DW_LDS, st, a, nt, q);
  return (int)hipGetLastError();
}

CSA_API int csa_dd_dgrad_splits(int M, int F, int N) {
  return dd_splits(((F + 31) / 32) * ((M + 63) / 64), N);
}

CSA_API int csa_dd_dgrad_slabs() { return DD_SLAB_ROWS; }

// dX[M][F] = dY[M][N] . W[F][N]^T through the forward input transform's backward (act,
// BatchNorm: bwd_slab [16][2][C] gets {sum dz, sum dz*xhat}).  dX zeroed when splits > 1.
CSA_API int csa_dd_dgrad(const float* dY, const float* W, float* dX, int M, int F, int N,
                         const float* x_fwd, int act, float alpha, const float* bn_slab, int bn_nslab, int bn_C,
                         float bn_count, float bn_eps, const float* bn_scale, const float* bn_offset,
                         float* bwd_slab, hipStream_t st) {
  if (M <= 0 || F <= 0 || N <= 0) return -1;
  if (bn_slab && (bn_C > DD_MAXC || bn_C <= 0 || !bwd_slab)) return -1;
  const int ft = (F + 31) / 32, mb = (M + 63) / 64;
  int ks = dd_splits(ft * mb, N);
  const int kper = dd_kper(N, ks);
  ks = (N + kper - 1) / kper;
  DDDgrad a{dY, W, dX, M, F, N, ks, kper, x_fwd, act, alpha,
            BNRef{bn_slab, bn_nslab, bn_C, bn_count, bn_eps, bn_scale, bn_offset}, bwd_slab};
  if (N % 4 == 0) hipLaunchKernelGGL(dd_dgrad_kernel<true>, dim3(ft, mb, ks), dim3(DD_THREADS), 0, st, a);
  else hipLaunchKernelGGL(dd_dgrad_kernel<false>, dim3(ft, mb, ks), dim3(DD_THREADS), 0, st, a);
  return (int)hipGetLastError();
}

// dW[F][N] = act(X)^T . dY * gscale, db = colsum(dY) * gscale (opt < 0), or the optimizer
// update of W / b and their slots with that gradient (opt >= 0; step = the device step
// counter after this step's increment).
// (sched: the step's learning-rate schedule, read here; null = constant)
CSA_API int csa_dd_wgrad_sched(const float* X, const float* dY, int M, int F, int N, int act, float alpha,
                               float gscale, float* dW, float* db, float* W, float* b, float* sW0, float* sW1,
                               float* sb0, float* sb1, int opt, float lr, const int64_t* step, hipStream_t st,
                               const LrSched* sched) {
  if (M <= 0 || F <= 0 || N <= 0) return -1;
  if (opt < 0 && (!dW || !db)) return -2;
  if (opt >= 0 && (!W || !b || (opt_nslots(opt) > 0 && (!sW0 || !sb0)) || (opt_nslots(opt) > 1 && (!sW1 || !sb1))))
    return -3;
  DDWgrad a{X, dY, M, F, N, act, alpha, gscale, dW, db, W, b, sW0, sW1, sb0, sb1, opt, lr, step,
            (F + 31) / 32, (N + 127) / 128, lr_sched_from(sched)};
  const int nb = a.ftiles * a.ntiles + (N + 63) / 64;
  hipLaunchKernelGGL(dd_wgrad_kernel, dim3(nb), dim3(DD_THREADS), 0, st, a);
  return (int)hipGetLastError();
}

CSA_API int csa_dd_wgrad(const float* X, const float* dY, int M, int F, int N, int act, float alpha, float gscale,
                         float* dW, float* db, float* W, float* b, float* sW0, float* sW1, float* sb0, float* sb1,
                         int opt, float lr, const int64_t* step, hipStream_t st) {
  return csa_dd_wgrad_sched(X, dY, M, F, N, act, alpha, gscale, dW, db, W, b, sW0, sW1, sb0, sb1, opt, lr, step, st,
                            nullptr);
}
