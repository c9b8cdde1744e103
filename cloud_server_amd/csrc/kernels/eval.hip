// Held-out evaluation on the device (runtime/validation.py): the consumer of a forward
// pass's head input (or logits) that never leaves HBM.
//
//   csa_eval_rows    once per evaluation batch of M rows, the LAST launch of that batch's
//                    forward: per row the prediction (lowest class index attaining the max,
//                    tf.argmax) and the loss term (head_loss conventions: softmax-xent
//                    lse - z[y], or MSE sum_j (z_j - onehot_j)^2), stored at the row's GLOBAL
//                    position g = cursor * M + m when g < n_total (the padded tail of the
//                    last batch writes nothing).  Two modes, one epilogue:
//                      fused  (K <= 1024): one 256-thread workgroup per row, the row-logits
//                             block of head_row_kernel (head_math.h) - no logits GEMM;
//                      logits (any head):  reads the [M, 10] logits csa_dense_fwd wrote, one
//                             row per 16-lane group.
//                    The last workgroup to arrive (agent-scope acq_rel counter, the
//                    head_rows_kernel pattern) advances the batch cursor for the NEXT
//                    launch; nothing in this launch reads the new value and no workgroup
//                    ever waits for another.
//   csa_eval_finish  once per sweep, one workgroup: confusion matrix conf[true][pred] (LDS
//                    integer atomics), its trace, and the loss sum in a FIXED order with
//                    double accumulation (strided per-thread slices, LDS tree), so two
//                    sweeps over the same parameters give identical bits.
//
// No float atomics to global memory; every output is a plain vector store.  The caller
// zeroes {cursor, arrival counter, result record} with one memset node per sweep.
#include "head_math.h"

namespace csa {

constexpr int EV_T = HROW_T;
constexpr int EV_KPT = 4;                 // fused mode: K <= EV_KPT * EV_T
constexpr int EV_REC_INTS = 2 + NCLS * NCLS;   // {n, correct, conf[100]} then double loss_sum

struct EvalArgs {
  const float* h; int M, K; int in_act; float in_alpha;      // fused: head input [M, K]
  const float* w; const float* b;                            // fused: Wh [K, 10], bh [10]
  const float* logits;                                       // logits mode: [M, 10]
  const int64_t* labels; const int64_t* rows; int64_t* cursor;
  int loss; int n_total; int n_batches;
  int* row_pred; float* row_loss; int* counter;
};

// One row per 16-lane group: lane j < 10 of the group holds logit j (-inf elsewhere).
// Every lane of the wave must call (ballot / shuffles); returns the row's prediction and
// loss term in every lane of the group (the dlogit is not kept).
__device__ __forceinline__ void eval_epilogue(float z, int label, int loss, int& am, float& ls) {
  const int j = threadIdx.x & 15;
  float d;
  head_lane_epilogue<Group16Shfl>(z, j < NCLS, j, label, loss, 0.f, 1, am, d, ls);
}

// Last arriver advances the cursor for the next launch and re-arms the counter.  Called by
// every thread after the workgroup's cursor-dependent loads were consumed.
__device__ __forceinline__ void eval_arrive(const EvalArgs& a, long c) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(a.counter, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (int)gridDim.x - 1) {
      const long nc = (c + 1 == (long)a.n_batches) ? 0 : c + 1;
      __hip_atomic_store(a.cursor, (int64_t)nc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.counter, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// A cursor outside [0, n_batches) (never produced by this file's kernels) is read as 0 so
// no row-table or output address can leave its buffer.
__device__ __forceinline__ long eval_cursor(const EvalArgs& a) {
  const long c = (long)__hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (c < 0 || c >= (long)a.n_batches) ? 0 : c;
}

// KPT = k per thread, the smallest that covers K (no clamped duplicate loads of Wh rows)
template <int KPT>
__global__ __launch_bounds__(EV_T) void eval_rows_fused_kernel(EvalArgs a) {
  __shared__ float s_part[EV_T / 64][NCLS];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  // every load first: this thread's h values and Wh rows (clamped addresses), the bias and
  // the row's label (the cursor -> row -> label chain runs under the h / Wh loads)
  float hv[KPT], wv[KPT][NCLS];
  head_row_load<KPT>(a.h + (long)m * K, a.w, K, hv, wv);
  const float bias = lane < NCLS ? a.b[lane] : 0.f;
  const long c = eval_cursor(a);
  const long g = c * a.M + m;
  int label = 0;
  if (wave == 0) label = (int)a.labels[a.rows[g]];
  head_row_partials<KPT>(hv, wv, K, a.in_act, a.in_alpha, s_part);
  __syncthreads();
  if (wave == 0) {
    // lane j < 10: logit j; lanes 0..15 are the row's group
    const float z = head_row_fold(s_part, lane, bias);
    int am; float ls;
    eval_epilogue(z, label, a.loss, am, ls);
    if (lane == 0 && g < (long)a.n_total) {
      a.row_pred[g] = am;
      a.row_loss[g] = ls;
    }
  }
  eval_arrive(a, c);
}

__global__ __launch_bounds__(EV_T) void eval_rows_logits_kernel(EvalArgs a) {
  const int tid = threadIdx.x, j = tid & 15;
  const int m = (int)blockIdx.x * (EV_T / 16) + (tid >> 4);
  const bool row = m < a.M;
  const long c = eval_cursor(a);
  const long g = c * a.M + (row ? m : 0);
  float z = -INFINITY;
  int label = 0;
  if (row) {
    if (j < NCLS) z = a.logits[(long)m * NCLS + j];
    label = (int)a.labels[a.rows[g]];
  }
  int am; float ls;
  eval_epilogue(z, label, a.loss, am, ls);
  if (row && j == 0 && g < (long)a.n_total) {
    a.row_pred[g] = am;
    a.row_loss[g] = ls;
  }
  eval_arrive(a, c);
}

struct EvalFinishArgs {
  const int* row_pred; const float* row_loss;
  const int64_t* labels; const int64_t* rows;
  int n_total; int* record;
};

__global__ __launch_bounds__(EV_T) void eval_finish_kernel(EvalFinishArgs a) {
  __shared__ int s_conf[NCLS * NCLS];
  __shared__ double s_sum[EV_T];
  const int tid = threadIdx.x;
  for (int i = tid; i < NCLS * NCLS; i += EV_T) s_conf[i] = 0;
  __syncthreads();
  // thread t: rows t, t + 256, ... in ascending order (a fixed slice, double accumulation)
  double acc = 0.0;
  for (int g = tid; g < a.n_total; g += EV_T) {
    const int p = a.row_pred[g];
    const int y = (int)a.labels[a.rows[g]];
    acc += (double)a.row_loss[g];
    if (p >= 0 && p < NCLS && y >= 0 && y < NCLS) atomicAdd(&s_conf[y * NCLS + p], 1);
  }
  s_sum[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int o = EV_T / 2; o > 0; o >>= 1) {           // fixed tree: the same order every sweep
    if (tid < o) s_sum[tid] += s_sum[tid + o];
    __syncthreads();
  }
  for (int i = tid; i < NCLS * NCLS; i += EV_T) a.record[2 + i] = s_conf[i];
  if (tid == 0) {
    int tr = 0;
    for (int i = 0; i < NCLS; ++i) tr += s_conf[i * NCLS + i];
    a.record[0] = a.n_total;
    a.record[1] = tr;
    *reinterpret_cast<double*>(a.record + EV_REC_INTS) = s_sum[0];    // byte 408: 8-aligned
  }
}

}  // namespace csa

using namespace csa;

// 1: csa_eval_rows takes the fused mode for this head (h / Wh / bh), 0: logits mode.
CSA_API int csa_eval_rows_fused_ok(int M, int K) { return M >= 1 && K >= 1 && K <= EV_KPT * EV_T ? 1 : 0; }

// int32 words of the result record {n, correct, conf[100], double loss_sum}.
CSA_API int csa_eval_record_ints(void) { return EV_REC_INTS + 2; }

// Fused mode when ``logits`` is null (h, w, b given; K <= 1024), logits mode otherwise.
// rows: [n_batches, M] row table, cursor: int64 batch index (advanced here), counter: one
// int32 arrival word; row_pred / row_loss: [>= n_total].
CSA_API int csa_eval_rows(const float* h, int M, int K, int in_act, float in_alpha, const float* w, const float* b,
                          const float* logits, const int64_t* labels, const int64_t* rows, int64_t* cursor,
                          int loss, int n_total, int n_batches, int* row_pred, float* row_loss, int* counter,
                          hipStream_t st) {
  if (M < 1 || n_batches < 1 || n_total < 1 || (long)n_batches * M < (long)n_total ||
      (long)n_batches * M > 0x7fffffffL || !labels || !rows || !cursor || !row_pred || !row_loss || !counter)
    return -1;
  EvalArgs a{h, M, K, in_act, in_alpha, w, b, logits, labels, rows, cursor, loss, n_total, n_batches,
             row_pred, row_loss, counter};
  if (logits) {
    hipLaunchKernelGGL(eval_rows_logits_kernel, dim3((unsigned)((M + EV_T / 16 - 1) / (EV_T / 16))), dim3(EV_T),
                       0, st, a);
    return (int)hipGetLastError();
  }
  if (!csa_eval_rows_fused_ok(M, K) || !h || !w || !b) return -1;
  if (reinterpret_cast<uintptr_t>(w) & 7) return -2;          // float2 loads of the Wh rows
  const dim3 grid((unsigned)M), blk(EV_T);
  if (K <= EV_T) hipLaunchKernelGGL(eval_rows_fused_kernel<1>, grid, blk, 0, st, a);
  else if (K <= 2 * EV_T) hipLaunchKernelGGL(eval_rows_fused_kernel<2>, grid, blk, 0, st, a);
  else if (K <= 3 * EV_T) hipLaunchKernelGGL(eval_rows_fused_kernel<3>, grid, blk, 0, st, a);
  else hipLaunchKernelGGL(eval_rows_fused_kernel<4>, grid, blk, 0, st, a);
  return (int)hipGetLastError();
}

CSA_API int csa_eval_finish(const int* row_pred, const float* row_loss, const int64_t* labels, const int64_t* rows,
                            int n_total, int* record, hipStream_t st) {
  if (!row_pred || !row_loss || !labels || !rows || !record || n_total < 1) return -1;
  if (reinterpret_cast<uintptr_t>(record) & 7) return -2;
  EvalFinishArgs a{row_pred, row_loss, labels, rows, n_total, record};
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(EV_T), 0, st, a);
  return (int)hipGetLastError();
}
