// augment.hip -- train-time scene augmentation and box targets on the device (eda_amd/augment.py; the point-dependent
// part of the reference's Joint3DDataset.__getitem__: _augment, _get_target_boxes, _get_scene_objects,
// _get_detected_objects and Scan._set_axis_align_bbox, src/joint_det_dataset.py / src/visual_data_handlers.py).
//
// Two launches per batch, both capturable (no host sync, no allocation):
//   points  grid (chunks, B): one thread per point -- flips, rot_z, rot_x, rot_y, + noise, + shift, * scale in fp64,
//           one rounding to fp32; colour ((c - mean) + mean) * f - mean; og_color copied; point_instance_label from
//           the scene's target ranks; per-object fp64 min / max of the augmented points, reduced in LDS and then
//           merged with 64-bit order-preserving integer atomics into the workspace
//   boxes   one workgroup per scene: _set_axis_align_bbox's chain, centre / size, jitter; the detector's boxes through
//           their 8 corners (rotations first, then flips: the reference's order), augment_det; resets the workspace
//           for the next batch and bumps the device counter
// The library is built with -ffp-contract=off and every sum is written in its order, so the numpy restatement in
// eda_amd/augment.py equals these kernels bit for bit.  The per-point draws come from Philox4x32-10 keyed by the
// seed, with the counter (point, scene position << 2 | call, device counter lo, hi); doubles are built from two words as
// numpy's random() builds them.
#include "eda_common.h"

namespace {

constexpr int AUG_THREADS = 256, AUG_PPT = 4, AUG_PTS_PER_BLOCK = AUG_THREADS * AUG_PPT;
constexpr int AUG_MAX_OBJ = 1024;   // objects per scan
constexpr int AUG_ROWS = 132;       // MAX_NUM_OBJ
// per-scene int32 row: slot, number of targets, 2 reserved, target object ids, keep mask, detected class ids (mode 2)
constexpr int AI_SLOT = 0, AI_NT = 1, AI_TIDS = 4, AI_KEEP = AI_TIDS + AUG_ROWS, AI_DCLS = AI_KEEP + AUG_ROWS,
              AI_STRIDE = AI_DCLS + AUG_ROWS;
// per-scene fp64 row: Rz, Rx, Ry (row-major 3 x 3 each), yz flip, xz flip, shift (3), scale, theta z / x / y (not read),
// target jitter factors (132 x 6), all_bboxes jitter factors (132 x 6), augment_det box draws (132 x 6), corrupt draws
// (132), class-id draws (132)
constexpr int AP_RZ = 0, AP_RX = 9, AP_RY = 18, AP_YZ = 27, AP_XZ = 28, AP_SHIFT = 29, AP_SCALE = 32, AP_JT = 36,
              AP_JA = AP_JT + AUG_ROWS * 6, AP_RB = AP_JA + AUG_ROWS * 6, AP_CR = AP_RB + AUG_ROWS * 6,
              AP_RC = AP_CR + AUG_ROWS, AP_STRIDE = AP_RC + AUG_ROWS;

constexpr unsigned long long KEY_MIN_INIT = ~0ull, KEY_MAX_INIT = 0ull;

// doubles -> unsigned keys with the same order (non-NaN values)
__device__ __forceinline__ unsigned long long dkey(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dval(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
  }
}
// numpy's random_standard_uniform: 53 bits from two 32-bit words
__device__ __forceinline__ double u53(unsigned a, unsigned b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// (R @ p): ((r0 * x + r1 * y) + r2 * z) per row
__device__ __forceinline__ void rot3(const double *R, double &x, double &y, double &z) {
  const double nx = (R[0] * x + R[1] * y) + R[2] * z;
  const double ny = (R[3] * x + R[4] * y) + R[5] * z;
  const double nz = (R[6] * x + R[7] * y) + R[8] * z;
  x = nx; y = ny; z = nz;
}

struct AugArgs {
  const double *xyz; const float *color; const short *obj; const double *det_box; const int *det_cls;
  const int *ints; const double *params; const double *noise; const double *colf;
  long long *counter;
  unsigned long long *ws;
  float *pc; float *og; long long *label;
  float *center; float *size; float *mask; float *all; float *det; long long *det_cls_out;
  long long counter_value;
  unsigned long long seed;
  long n_slots;
  int N, n_obj, B, augment, use_color, det_mode, augment_det;
};

__global__ __launch_bounds__(AUG_THREADS) void augment_points_kernel(AugArgs a) {
  extern __shared__ unsigned long long s_key[];                 // n_obj x (min x, y, z, max x, y, z)
  int *s_rank = (int *)(s_key + (size_t)a.n_obj * 6);           // object -> target rank, -1
  const int tid = threadIdx.x, b = blockIdx.y;
  const int *ib = a.ints + (size_t)b * AI_STRIDE;
  const long slot = ib[AI_SLOT];
  if (slot < 0 || slot >= a.n_slots) return;                   // (the host validates; nothing is read out of range)
  for (int e = tid; e < a.n_obj * 6; e += AUG_THREADS) s_key[e] = (e % 6) < 3 ? KEY_MIN_INIT : KEY_MAX_INIT;
  for (int o = tid; o < a.n_obj; o += AUG_THREADS) s_rank[o] = -1;
  __syncthreads();
  const int nt = min(max(ib[AI_NT], 0), AUG_ROWS);
  // point_instance_label[points of tids[t]] = t in order: a repeated object keeps its last rank
  for (int t = tid; t < nt; t += AUG_THREADS) {
    const int o = ib[AI_TIDS + t];
    if (o >= 0 && o < a.n_obj) atomicMax(&s_rank[o], t);
  }
  __syncthreads();

  const double *P = a.params + (size_t)b * AP_STRIDE;
  const bool yz = P[AP_YZ] != 0.0, xz = P[AP_XZ] != 0.0;
  const double sx = P[AP_SHIFT], sy = P[AP_SHIFT + 1], sz = P[AP_SHIFT + 2], scale = P[AP_SCALE];
  const long long ctr = a.counter ? a.counter[0] : a.counter_value;
  const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
  const double m0 = 109.8 / 256, m1 = 97.2 / 256, m2 = 83.8 / 256;
  const int C = a.use_color ? 6 : 3;
  const size_t sbase = (size_t)slot * a.N;
#pragma unroll
  for (int q = 0; q < AUG_PPT; ++q) {
    const int n = blockIdx.x * AUG_PTS_PER_BLOCK + q * AUG_THREADS + tid;
    if (n >= a.N) break;
    const size_t src = sbase + n, dst = (size_t)b * a.N + n;
    double x = a.xyz[src * 3 + 0], y = a.xyz[src * 3 + 1], z = a.xyz[src * 3 + 2];
    const float c0 = a.color[src * 3 + 0], c1 = a.color[src * 3 + 1], c2 = a.color[src * 3 + 2];
    double r = (double)c0 - m0, g = (double)c1 - m1, bl = (double)c2 - m2;
    if (a.augment) {
      double nz[3], cf[3];
      if (a.noise) {
        for (int k = 0; k < 3; ++k) { nz[k] = a.noise[dst * 3 + k]; cf[k] = a.colf[dst * 3 + k]; }
      } else {
        double u[6];
        for (int j = 0; j < 3; ++j) {
          unsigned w[4] = {(unsigned)n, ((unsigned)b << 2) | (unsigned)j, (unsigned)ctr, (unsigned)((unsigned long long)ctr >> 32)};
          philox4x32_10(w, k0, k1);
          u[2 * j] = u53(w[0], w[1]);
          u[2 * j + 1] = u53(w[2], w[3]);
        }
        for (int k = 0; k < 3; ++k) { nz[k] = u[k] * 5e-3; cf[k] = 0.98 + 0.04 * u[3 + k]; }
      }
      if (yz) x = -x;
      if (xz) y = -y;
      rot3(P + AP_RZ, x, y, z);
      rot3(P + AP_RX, x, y, z);
      rot3(P + AP_RY, x, y, z);
      x = x + nz[0]; y = y + nz[1]; z = z + nz[2];
      x += sx; y += sy; z += sz;
      x *= scale; y *= scale; z *= scale;
      r = (r + m0) * cf[0] - m0;
      g = (g + m1) * cf[1] - m1;
      bl = (bl + m2) * cf[2] - m2;
    }
    float *pc = a.pc + dst * C;
    pc[0] = (float)x; pc[1] = (float)y; pc[2] = (float)z;
    if (a.use_color) { pc[3] = (float)r; pc[4] = (float)g; pc[5] = (float)bl; }
    a.og[dst * 3 + 0] = c0; a.og[dst * 3 + 1] = c1; a.og[dst * 3 + 2] = c2;
    const int o = a.obj[src];
    const bool in = o >= 0 && o < a.n_obj;
    a.label[dst] = in ? (long long)s_rank[o] : -1ll;
    if (in) {
      unsigned long long *k = s_key + (size_t)o * 6;
      const unsigned long long kx = dkey(x), ky = dkey(y), kz = dkey(z);
      atomicMin(&k[0], kx); atomicMin(&k[1], ky); atomicMin(&k[2], kz);
      atomicMax(&k[3], kx); atomicMax(&k[4], ky); atomicMax(&k[5], kz);
    }
  }
  __syncthreads();
  unsigned long long *wsb = a.ws + (size_t)b * a.n_obj * 6;
  for (int e = tid; e < a.n_obj * 6; e += AUG_THREADS) {
    const unsigned long long k = s_key[e];
    if ((e % 6) < 3) {
      if (k != KEY_MIN_INIT) atomicMin(&wsb[e], k);
    } else if (k != KEY_MAX_INIT) {
      atomicMax(&wsb[e], k);
    }
  }
}

// Scan._set_axis_align_bbox of an object's augmented points, then (min + max) * 0.5 / max - min; an object without
// points gets a zero box (the reference raises on it)
__device__ __forceinline__ void object_box(const unsigned long long *k, double *c, double *s) {
  if (k[0] == KEY_MIN_INIT) {
    for (int d = 0; d < 3; ++d) { c[d] = 0.0; s[d] = 0.0; }
    return;
  }
  for (int d = 0; d < 3; ++d) {
    const double mn = dval(k[d]), mx = dval(k[3 + d]);
    const double cx = (mx + mn) / 2.0, l = mx - mn;
    const double lo = cx - l / 2.0, hi = cx + l / 2.0;
    c[d] = (lo + hi) * 0.5;
    s[d] = hi - lo;
  }
}

__global__ __launch_bounds__(AUG_THREADS) void augment_boxes_kernel(AugArgs a) {
  __shared__ double s_det[AUG_ROWS * 6], s_mn[6], s_mx[6];
  __shared__ long long s_cls[AUG_ROWS];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int *ib = a.ints + (size_t)b * AI_STRIDE;
  const long slot = ib[AI_SLOT];
  const bool ok = slot >= 0 && slot < a.n_slots;
  const double *P = a.params + (size_t)b * AP_STRIDE;
  const unsigned long long *wsb = a.ws + (size_t)b * a.n_obj * 6;
  const int nt = min(max(ib[AI_NT], 0), AUG_ROWS);
  const size_t rb = (size_t)b * AUG_ROWS;
  if (ok && tid < AUG_ROWS) {
    const int r = tid;
    // target rows: the boxes of tids in order, jittered; centre 1000 and size 0 beyond them
    double c[3] = {1000.0, 1000.0, 1000.0}, s[3] = {0.0, 0.0, 0.0};
    const int o = r < nt ? ib[AI_TIDS + r] : -1;
    if (r < nt) {
      if (o >= 0 && o < a.n_obj) {
        object_box(wsb + (size_t)o * 6, c, s);
      } else {
        for (int d = 0; d < 3; ++d) c[d] = 0.0;
      }
      if (a.augment)
        for (int d = 0; d < 3; ++d) { c[d] *= P[AP_JT + r * 6 + d]; s[d] *= P[AP_JT + r * 6 + 3 + d]; }
    }
    for (int d = 0; d < 3; ++d) { a.center[(rb + r) * 3 + d] = (float)c[d]; a.size[(rb + r) * 3 + d] = (float)s[d]; }
    a.mask[rb + r] = r < nt ? 1.f : 0.f;
    // all_bboxes: the kept objects among the first 132, zero rows elsewhere; all 132 rows jittered
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (r < a.n_obj && ib[AI_KEEP + r]) object_box(wsb + (size_t)r * 6, v, v + 3);
    if (a.augment)
      for (int d = 0; d < 6; ++d) v[d] *= P[AP_JA + r * 6 + d];
    for (int d = 0; d < 6; ++d) a.all[(rb + r) * 6 + d] = (float)v[d];
    // detected boxes: the detector's (mode 1) or a copy of all_bboxes (mode 2, butd_gt / butd_cls)
    double w[6] = {0, 0, 0, 0, 0, 0};
    long long cls = 0;
    if (a.det_mode == 1) {
      const double *db = a.det_box + ((size_t)slot * AUG_ROWS + r) * 6;
      for (int d = 0; d < 6; ++d) w[d] = db[d];
      cls = a.det_cls[(size_t)slot * AUG_ROWS + r];
      if (a.augment) {
        // box2points, rot_z, rot_x, rot_y, flips, + shift, * scale, points2box (padded zero rows included)
        double lo[3], hi[3], mn[3], mx[3];
        for (int d = 0; d < 3; ++d) { lo[d] = w[d] - w[3 + d] / 2; hi[d] = w[d] + w[3 + d] / 2; }
        for (int q = 0; q < 8; ++q) {
          double x = (q & 2) ? hi[0] : lo[0], y = (q & 1) ? hi[1] : lo[1], z = (q & 4) ? hi[2] : lo[2];
          rot3(P + AP_RZ, x, y, z);
          rot3(P + AP_RX, x, y, z);
          rot3(P + AP_RY, x, y, z);
          if (P[AP_YZ] != 0.0) x = -x;
          if (P[AP_XZ] != 0.0) y = -y;
          x += P[AP_SHIFT]; y += P[AP_SHIFT + 1]; z += P[AP_SHIFT + 2];
          x *= P[AP_SCALE]; y *= P[AP_SCALE]; z *= P[AP_SCALE];
          const double p[3] = {x, y, z};
          for (int d = 0; d < 3; ++d) {
            mn[d] = q ? fmin(mn[d], p[d]) : p[d];
            mx[d] = q ? fmax(mx[d], p[d]) : p[d];
          }
        }
        for (int d = 0; d < 3; ++d) { w[d] = (mn[d] + mx[d]) / 2; w[3 + d] = mx[d] - mn[d]; }
      }
    } else if (a.det_mode == 2) {
      for (int d = 0; d < 6; ++d) w[d] = v[d];
      cls = ib[AI_DCLS + r];
    }
    for (int d = 0; d < 6; ++d) s_det[r * 6 + d] = w[d];
    s_cls[r] = cls;
  }
  __syncthreads();
  const bool corrupt_on = ok && a.det_mode == 1 && a.augment && a.augment_det;
  if (corrupt_on && tid < 6) {                  // all_detected_bboxes.min(0) / .max(0)
    double mn = s_det[tid], mx = s_det[tid];
    for (int r = 1; r < AUG_ROWS; ++r) { mn = fmin(mn, s_det[r * 6 + tid]); mx = fmax(mx, s_det[r * 6 + tid]); }
    s_mn[tid] = mn;
    s_mx[tid] = mx;
  }
  __syncthreads();
  if (ok && tid < AUG_ROWS) {
    const int r = tid;
    const bool corrupt = corrupt_on && P[AP_CR + r] > 0.7;
    for (int d = 0; d < 6; ++d) {
      const double x = corrupt ? (s_mx[d] - s_mn[d]) * P[AP_RB + r * 6 + d] + s_mn[d] : s_det[r * 6 + d];
      a.det[(rb + r) * 6 + d] = (float)x;
    }
    a.det_cls_out[rb + r] = corrupt ? (long long)P[AP_RC + r] : s_cls[r];
  }
  // the workspace back to its initial state for the next batch (every read of it is above this barrier)
  __syncthreads();
  unsigned long long *wsw = a.ws + (size_t)b * a.n_obj * 6;
  for (int e = tid; e < a.n_obj * 6; e += AUG_THREADS) wsw[e] = (e % 6) < 3 ? KEY_MIN_INIT : KEY_MAX_INIT;
  if (b == 0 && tid == 0 && a.counter) a.counter[0] = a.counter[0] + 1;
}

}  // namespace

extern "C" int eda_augment_layout(int *out) {
  EDA_CHECK_ARG(out, "null pointer");
  const int v[6] = {AI_STRIDE, AP_STRIDE, AUG_ROWS, AUG_MAX_OBJ, AI_TIDS, AP_JT};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  return 0;
}

extern "C" int eda_augment_batch_f64(const double *xyz, const float *color, const short *obj, const double *det_box,
                                     const int *det_cls, long n_slots, int n_points, int n_obj, const int *ints,
                                     const double *params, int B, int augment, int use_color, int det_mode,
                                     int augment_det, const double *noise, const double *color_factor, long *counter,
                                     long counter_value, unsigned long long seed, unsigned long long *ws,
                                     float *point_clouds, float *og_color, long *point_instance_label,
                                     float *center_label, float *size_gts, float *box_label_mask, float *all_bboxes,
                                     float *det_boxes, long *det_class_ids, void *stream) {
  EDA_CHECK_ARG(B >= 0 && B <= 65535, "B must be in 0..65535");
  EDA_CHECK_ARG(n_points >= 1 && n_slots >= 1, "n_points and n_slots must be >= 1");
  EDA_CHECK_ARG(n_obj >= 1 && n_obj <= AUG_MAX_OBJ, "n_obj must be in 1..1024");
  EDA_CHECK_ARG(det_mode >= 0 && det_mode <= 2, "det_mode must be 0 (none), 1 (detector boxes) or 2 (copy all_bboxes)");
  EDA_CHECK_ARG((noise == nullptr) == (color_factor == nullptr), "noise and color_factor are given together or not at all");
  EDA_CHECK_ARG(xyz && color && obj && ints && params && ws && point_clouds && og_color && point_instance_label &&
                    center_label && size_gts && box_label_mask && all_bboxes && det_boxes && det_class_ids,
                "null pointer");
  EDA_CHECK_ARG(det_mode != 1 || (det_box && det_cls), "det_mode 1 needs the detector boxes");
  if (B == 0) return 0;
  AugArgs a{xyz, color, obj, det_box, det_cls, ints, params, noise, color_factor, (long long *)counter, ws,
            point_clouds, og_color, (long long *)point_instance_label, center_label, size_gts, box_label_mask,
            all_bboxes, det_boxes, (long long *)det_class_ids, (long long)counter_value, seed, n_slots, n_points,
            n_obj, B, augment ? 1 : 0, use_color ? 1 : 0, det_mode, augment_det ? 1 : 0};
  const size_t lds = (size_t)n_obj * 6 * sizeof(unsigned long long) + (size_t)n_obj * sizeof(int);
  const unsigned chunks = (unsigned)((n_points + AUG_PTS_PER_BLOCK - 1) / AUG_PTS_PER_BLOCK);
  hipLaunchKernelGGL(augment_points_kernel, dim3(chunks, (unsigned)B), dim3(AUG_THREADS), lds, (hipStream_t)stream, a);
  EDA_CHECK_LAUNCH();
  hipLaunchKernelGGL(augment_boxes_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
  EDA_CHECK_LAUNCH();
  return 0;
}
