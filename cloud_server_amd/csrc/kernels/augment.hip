// Training-time augmentation (gfx950 / CDNA4): this step's batch, gathered through the
// device cursor and warped anew -- shift, rotation, zoom, one erased rectangle.
//
// The reference trains on the stored files only; its one augmentation is the offline
// /preprocess/ pipeline with its "copy twins" (apps/preprocess/preprocess.py), fixed draws
// stored once.  Here the augmented image is a pure function of (seed, step, dataset row):
// ops/augment_ref.py is the one definition and this kernel forms the same bytes, so nothing
// is stored and a resumed, packed, multi-step-graph or data-parallel run redraws them.
//
// One 256-thread workgroup per image.  The cursor -> row -> image chain is three dependent
// round trips; the step counter is read beside the cursor.  Lanes 0..7 make the eight draws
// while 196 threads stage the 784 source bytes in LDS as dwords; behind one barrier every
// thread derives the (workgroup-uniform) parameters, the angle / zoom tables come from the
// kernel's own argument block, and each of 196 threads forms four output pixels and stores
// one dword.  Only 28 x 28 uint8 images (the dataset's format).
#include "common.h"
#include "crng.h"

// Byte-parity with the NumPy float32 reference: every product and sum rounds on its own
// (the library is built with -ffp-contract=fast-honor-pragmas for the training kernels).
#pragma clang fp contract(off)

namespace csa {

constexpr int AUG_THREADS = 256;
constexpr int AUG_HW = 28, AUG_PIX = AUG_HW * AUG_HW, AUG_WORDS = AUG_PIX / 4;
constexpr int AUG_MAX_SHIFT = 8, AUG_MAX_ROTATE = 45, AUG_MAX_SCALE = 30, AUG_MAX_ERASE = 14;

// ops/augment_ref.py AugParamsC: the option's amounts and the host-built float32 tables
// (cos / sin of -R..R degrees, 100 / (100 + q) for q = -P..P)
struct AugParams {
  int shift, rotate, scale, erase_max, fill, erase_T;
  float cos_t[2 * AUG_MAX_ROTATE + 1], sin_t[2 * AUG_MAX_ROTATE + 1], inv_t[2 * AUG_MAX_SCALE + 1];
};

struct AugArgs {
  const uint8_t* img;          // the dataset [N][784]
  const int64_t* rows;         // the row table; this step's rows = rows[cursor * B ..]
  const int64_t* cursor;
  const long long* step;       // completed training steps (the engine's counter)
  uint32_t* out;               // [B][196] dwords
  uint64_t seed;
  int B;
  AugParams p;
};

__device__ __forceinline__ float aug_tap(const uint8_t* s, int y, int x, float fill) {
  const bool ok = (unsigned)y < (unsigned)AUG_HW && (unsigned)x < (unsigned)AUG_HW;
  return ok ? (float)s[ok ? y * AUG_HW + x : 0] : fill;
}

__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(AugArgs a) {
  __shared__ uint32_t s_img[AUG_WORDS];
  __shared__ uint32_t s_r[8];
  const int t = threadIdx.x, b = blockIdx.x;
  const uint64_t step = (uint64_t)*a.step & 0xFFFFFFFFull;
  const int64_t row = a.rows[*a.cursor * a.B + b];
  if (t < AUG_WORDS) s_img[t] = reinterpret_cast<const uint32_t*>(a.img + row * AUG_PIX)[t];
  if (t < 8) s_r[t] = crng(a.seed, step, (uint64_t)row * 8u + (uint64_t)t);
  __syncthreads();
  if (t >= AUG_WORDS) return;

  const AugParams& p = a.p;
  const uint32_t n = 2u * (uint32_t)p.shift + 1u;
  const float dx = (float)((int)(s_r[0] % n) - p.shift), dy = (float)((int)(s_r[1] % n) - p.shift);
  const uint32_t ai = s_r[2] % (2u * (uint32_t)p.rotate + 1u), zi = s_r[3] % (2u * (uint32_t)p.scale + 1u);
  const float ca = p.cos_t[ai], sa = p.sin_t[ai], inv = p.inv_t[zi];
  const bool erase = (s_r[4] >> 8) < (uint32_t)p.erase_T;
  const int eh = 1 + (int)(s_r[5] % (uint32_t)p.erase_max), ew = 1 + (int)(s_r[6] % (uint32_t)p.erase_max);
  const int etop = (int)((s_r[7] & 0xFFFFu) % (uint32_t)(AUG_HW - eh + 1));
  const int eleft = (int)((s_r[7] >> 16) % (uint32_t)(AUG_HW - ew + 1));
  const float fill = (float)p.fill;
  const uint8_t* s = reinterpret_cast<const uint8_t*>(s_img);

  const int y = t / (AUG_HW / 4), xb = 4 * (t - y * (AUG_HW / 4));
  constexpr float c = 13.5f;
  const float v = ((float)y - c) - dy;
  const bool erow = erase && y >= etop && y < etop + eh;
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x = xb + i;
    const float u = ((float)x - c) - dx;
    const float sx = ((ca * u) + (sa * v)) * inv + c;
    const float sy = ((ca * v) - (sa * u)) * inv + c;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float top = (1.0f - fx) * aug_tap(s, y0, x0, fill) + fx * aug_tap(s, y0, x0 + 1, fill);
    const float bot = (1.0f - fx) * aug_tap(s, y0 + 1, x0, fill) + fx * aug_tap(s, y0 + 1, x0 + 1, fill);
    const float val = (1.0f - fy) * top + fy * bot;
    uint32_t o = (uint32_t)fminf(floorf(val + 0.5f), 255.0f);
    if (erow && x >= eleft && x < eleft + ew) o = (uint32_t)p.fill;
    word |= o << (8 * i);
  }
  a.out[(long)b * AUG_WORDS + t] = word;
}

}  // namespace csa

using namespace csa;

// out[b] = augment(images[rows[cursor * B + b]]) for b < B at step *step (ops/augment_ref.py):
// uint8 [B][H * W].  H == W == 28; images and out 4-byte aligned.  Every argument is checked
// here; a bad one returns a negative code and launches nothing.
CSA_API int csa_augment_batch(const uint8_t* images, const int64_t* rows, const int64_t* cursor, int B, int H, int W,
                              const AugParams* params, uint64_t aug_seed, const long long* step, uint8_t* out,
                              hipStream_t st) {
  if (!images || !rows || !cursor || !params || !step || !out) return -2;
  if (B <= 0 || H != AUG_HW || W != AUG_HW) return -1;
  const AugParams& p = *params;
  if (p.shift < 0 || p.shift > AUG_MAX_SHIFT || p.rotate < 0 || p.rotate > AUG_MAX_ROTATE || p.scale < 0 ||
      p.scale > AUG_MAX_SCALE || p.erase_max < 1 || p.erase_max > AUG_MAX_ERASE || p.fill < 0 || p.fill > 255 ||
      p.erase_T < 0 || p.erase_T > (1 << 24))
    return -3;
  if (((uintptr_t)images & 3u) || ((uintptr_t)out & 3u)) return -4;
  AugArgs a{images, rows, cursor, step, reinterpret_cast<uint32_t*>(out), aug_seed, B, p};
  hipLaunchKernelGGL(augment_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, st, a);
  return (int)hipGetLastError();
}
