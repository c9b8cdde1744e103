// Per-element optimizer updates shared by the standalone optimizer launch (optim.hip) and
// the kernels that apply the update in their own epilogue (dense_update.hip), so a
// parameter sees bit-identical arithmetic whichever kernel updates it.
//
// Reference: tf.train.AdagradOptimizer(1e-4) (construct_distribute.py:372-373) plus the
// GD / Adam / Adadelta choices of apps/construction/util/options.py:26-37, with TF's
// defaults (Adam b1 0.9 b2 0.999 eps 1e-8; Adadelta rho 0.95 eps 1e-8; Adagrad
// accumulators start at 0.1, set by the host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csa {

enum Opt : int { OPT_SGD = 0, OPT_ADAGRAD = 1, OPT_ADAM = 2, OPT_ADADELTA = 3 };

// Learning-rate schedule (ops/lr_schedule.py is the definition): a pure function of the
// 1-based step t, evaluated on the device by the launch that applies the update, so it moves
// inside a replayed graph and needs no host state.  Passed by value in every update
// launch's argument struct; all-zero is the constant schedule.
// (LR_WARMUP: the constant type under a warm-up; LR_CONSTANT is no schedule at all)
enum LrKind : int { LR_CONSTANT = 0, LR_EXPONENTIAL = 1, LR_INVERSE_TIME = 2, LR_COSINE = 3, LR_WARMUP = 4 };
struct LrSched {
  int kind;            // LrKind
  int staircase;       // exponential / inverse_time: floor the step ratio
  int decay_steps;     // S >= 1
  int warmup_steps;    // W >= 0: linear warm-up on top of any kind
  float rate;          // r
  float alpha;         // cosine: floor, as a fraction of the base rate
};
static_assert(sizeof(LrSched) == 24, "LrSched is a 24-byte POD (ctypes mirror: ops/lr_schedule.py)");

// The host reads an entry point's optional schedule (null: constant).
__host__ inline LrSched lr_sched_from(const LrSched* s) { return s ? *s : LrSched{}; }

// Multiplier m of step t (g = t - 1 is TF's global_step: the first update uses g = 0).  fp32,
// operations in the order written (no contraction); the stair index is an INTEGER division
// of the counter, never the floor of a float quotient (3 * fl(1/3) floors to the wrong stair).
__device__ __forceinline__ float lr_sched_mult(const LrSched& s, int64_t t) {
#pragma clang fp contract(off)
  const int g = t > 0 ? (int)(t - 1) : 0;
  float m = 1.f;
  if (s.kind == LR_COSINE) {
    const float x = (float)(g < s.decay_steps ? g : s.decay_steps) / (float)s.decay_steps;
    m = s.alpha + (1.f - s.alpha) * 0.5f * (1.f + cosf(3.14159265358979323846f * x));
  } else if (s.kind == LR_EXPONENTIAL || s.kind == LR_INVERSE_TIME) {
    const float x = s.staircase ? (float)(g / s.decay_steps) : (float)g / (float)s.decay_steps;
    m = s.kind == LR_EXPONENTIAL ? powf(s.rate, x) : 1.f / (1.f + s.rate * x);
  }
  if (g < s.warmup_steps) m = m * ((float)(g + 1) / (float)s.warmup_steps);
  return m;
}

// Effective learning rate of this step.  ``step`` is the device step counter AFTER this
// step's increment (the head kernel advances it before any update runs): Adam's 1-based t.
__device__ __forceinline__ float opt_step_lr(int opt, float lr, const int64_t* step) {
  if (opt != OPT_ADAM) return lr;
  const float t = (float)(*step);
  return lr * sqrtf(1.f - powf(0.999f, t)) / (1.f - powf(0.9f, t));
}

// ... at a given 1-based step t under a schedule: lr_t = lr * m(t), then Adam's correction.
__device__ __forceinline__ float opt_step_lr_at(int opt, float lr, int64_t t, const LrSched& s) {
  if (s.kind != LR_CONSTANT) lr = lr * lr_sched_mult(s, t);
  if (opt != OPT_ADAM) return lr;
  const float tf = (float)t;
  return lr * sqrtf(1.f - powf(0.999f, tf)) / (1.f - powf(0.9f, tf));
}

// The base rate of this step under the schedule, as one scalar: lr itself (no load, no
// multiply) for the constant schedule, else lr * m(t) read from the counter.  For the bodies
// that are tight on registers: evaluated at the body's entry, before its operands are in
// flight, and handed to the schedule-free opt_step_lr where the rate was always formed.
// Uniform callers only (every lane sees the same step).
__device__ __forceinline__ float opt_sched_lr(float lr, const int64_t* step, const LrSched& s) {
  if (__builtin_expect(s.kind == LR_CONSTANT, 1)) return lr;   // (the scheduled block: off the straight path)
  const float v = lr * lr_sched_mult(s, *step);
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// ... read from the counter.  The constant schedule is the function above: no multiply, and
// no load of the counter unless Adam needs it.
__device__ __forceinline__ float opt_step_lr(int opt, float lr, const int64_t* step, const LrSched& s) {
  if (__builtin_expect(s.kind == LR_CONSTANT, 1)) return opt_step_lr(opt, lr, step);
  return opt_step_lr_at(opt, lr, *step, s);
}

// w, s0, s1 updated in place from gradient g (s1 only for Adam / Adadelta).
__device__ __forceinline__ void opt_update(int opt, float lr, float& w, float g, float& s0, float& s1) {
  if (opt == OPT_SGD) {
    w -= lr * g;
  } else if (opt == OPT_ADAGRAD) {
    s0 += g * g;
    w -= lr * g * rsqrtf(s0);
  } else if (opt == OPT_ADAM) {
    s0 = 0.9f * s0 + 0.1f * g;
    s1 = 0.999f * s1 + 0.001f * g * g;
    w -= lr * s0 / (sqrtf(s1) + 1e-8f);
  } else {  // Adadelta
    s0 = 0.95f * s0 + 0.05f * g * g;
    const float upd = sqrtf(s1 + 1e-8f) / sqrtf(s0 + 1e-8f) * g;
    s1 = 0.95f * s1 + 0.05f * upd * upd;
    w -= lr * upd;
  }
}

__host__ __device__ __forceinline__ int opt_nslots(int opt) {
  return opt == OPT_SGD ? 0 : (opt == OPT_ADAGRAD ? 1 : 2);
}

}  // namespace csa
