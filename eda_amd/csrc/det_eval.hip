// det_eval.hip -- ScanNet detection mAP on the device: proposal decode, class-aware greedy 3D NMS, AP matching
// (eda_amd/ap_helper.py; the reference's models/ap_helper.py parse_predictions + utils/nms.py + utils/eval_det.py).
//
// All box and IoU arithmetic is fp64 in the reference's operation order (the library is built with -ffp-contract=off), so
// boxes, IoUs, keep decisions and TP flags equal a numpy float64 restatement bit for bit.  max/min propagate NaN as
// np.maximum / np.minimum do, so zero-volume boxes (0/0 IoUs) behave as the reference's comparisons do: a NaN IoU never
// suppresses and never matches.  Plain loads and stores only; no MFMA.
//
//   decode  one thread per proposal: camera-frame AABB (fp64), objectness, per-class probabilities, arg-max class
//   nms     one workgroup per scene (K <= 1024): rank by descending score (ties: larger index first, what a stable
//           ascending argsort gives), then the greedy scan with one barrier per KEPT box -- the winner's row is computed
//           on the fly by the threads that own the later boxes, nothing K x K is stored
//   match   one wave per (threshold, class, scene) segment: the segment's predictions ranked by descending confidence
//           (ties: ascending j, NaN last), each one matched against the scene's ground truth of that class (first
//           maximum IoU, TP when IoU > threshold and the box is not taken yet)
#include "eda_common.h"

namespace {

constexpr int DET_MAXK = 1024, DET_MAXG = 1024;
constexpr int NMS_THREADS = 256, NMS_PER = DET_MAXK / NMS_THREADS;

// np.maximum / np.minimum: a NaN operand wins
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a >= b ? a : b)); }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a <= b ? a : b)); }

// intersection volume ((l * w) * h) of two AABBs (x1, y1, z1, x2, y2, z2)
__device__ __forceinline__ double aabb_inter(const double *a, const double *b) {
  const double l = np_max(0.0, np_min(a[3], b[3]) - np_max(a[0], b[0]));
  const double w = np_max(0.0, np_min(a[4], b[4]) - np_max(a[1], b[1]));
  const double h = np_max(0.0, np_min(a[5], b[5]) - np_max(a[2], b[2]));
  return l * w * h;
}
__device__ __forceinline__ double aabb_vol(const double *a) { return (a[3] - a[0]) * (a[4] - a[1]) * (a[5] - a[2]); }

// ---------------------------------------------------------------------------------------------------------- decode
__global__ __launch_bounds__(256) void det_decode_kernel(const float *__restrict__ center, const float *__restrict__ size,
                                                         const float *__restrict__ logits, const float *__restrict__ obj_logits,
                                                         long n, int C1, double *__restrict__ aabb, float *__restrict__ obj_prob,
                                                         float *__restrict__ cls_prob, int *__restrict__ sem_cls) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int C = C1 - 1;
  // flip_axis_to_camera (x, -z, y) in fp32, half sizes in fp32 (l along x, h along y, w along z), sums in fp64
  const float cx = center[i * 3 + 0], cy = -center[i * 3 + 2], cz = center[i * 3 + 1];
  const float hl = size[i * 3 + 0] / 2, hw = size[i * 3 + 1] / 2, hh = size[i * 3 + 2] / 2;
  const double xa = (double)cx + (double)hl, xb = (double)cx + (double)(-hl);
  const double ya = (double)cy + (double)hh, yb = (double)cy + (double)(-hh);
  const double za = (double)cz + (double)hw, zb = (double)cz + (double)(-hw);
  double *o = aabb + i * 6;
  o[0] = np_min(xa, xb); o[1] = np_min(ya, yb); o[2] = np_min(za, zb);
  o[3] = np_max(xa, xb); o[4] = np_max(ya, yb); o[5] = np_max(za, zb);
  // softmax over C + 1 columns in fp32: exp(x - max) / sum; arg-max (first) of the raw logits over the first C
  const float *x = logits + i * C1;
  float mx = x[0];
  for (int c = 1; c < C1; ++c) mx = x[c] > mx ? x[c] : mx;
  int am = 0;
  float best = x[0];
  for (int c = 1; c < C; ++c)
    if (x[c] > best) { best = x[c]; am = c; }
  float sum = 0.f;
  for (int c = 0; c < C1; ++c) sum += expf(x[c] - mx);
  float *p = cls_prob + i * C;
  float obj;
  if (obj_logits) {
    obj = 1.f / (1.f + expf(-obj_logits[i]));
    for (int c = 0; c < C; ++c) p[c] = expf(x[c] - mx) / sum;
  } else {
    obj = 1.f - expf(x[C] - mx) / sum;
    for (int c = 0; c < C; ++c) p[c] = (expf(x[c] - mx) / sum) / obj;
  }
  obj_prob[i] = obj;
  sem_cls[i] = am;
}

// ------------------------------------------------------------------------------------------------------------- nms
// descending-score order: NaN first (a NaN is the largest key of an ascending numpy argsort), ties by larger index
__device__ __forceinline__ bool nms_before(double si, int i, double sj, int j) {
  const bool ni = si != si, nj = sj != sj;
  if (ni || nj) return ni && (!nj || i > j);
  return si > sj || (si == sj && i > j);
}

__global__ __launch_bounds__(NMS_THREADS) void det_nms_kernel(const double *__restrict__ aabb, const double *__restrict__ score,
                                                               const int *__restrict__ cls, int K, double thr, int old_type,
                                                               int cls_nms, unsigned char *__restrict__ keep) {
  __shared__ double s_box[DET_MAXK * 6];
  __shared__ double s_val[DET_MAXK];          // scores while ranking, then areas
  __shared__ int s_cls[DET_MAXK];
  __shared__ short s_order[DET_MAXK];         // rank -> index
  __shared__ unsigned char s_state[DET_MAXK]; // 0 suppressed, 1 open, 2 kept
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const double *box_b = aabb + b * K * 6;
  for (int e = tid; e < K * 6; e += NMS_THREADS) s_box[e] = box_b[e];
  for (int j = tid; j < K; j += NMS_THREADS) {
    s_val[j] = score[b * K + j];
    s_cls[j] = cls ? cls[b * K + j] : 0;
    s_state[j] = 1;
  }
  __syncthreads();
  int rank[NMS_PER];
#pragma unroll
  for (int q = 0; q < NMS_PER; ++q) {
    const int j = tid + q * NMS_THREADS;
    rank[q] = -1;
    if (j < K) {
      const double sj = s_val[j];
      int r = 0;
      for (int i = 0; i < K; ++i) r += nms_before(s_val[i], i, sj, j) ? 1 : 0;
      rank[q] = r;                          // a strict total order: the ranks are a permutation of 0..K-1
      s_order[r] = (short)j;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NMS_PER; ++q) {
    const int j = tid + q * NMS_THREADS;
    if (j < K) s_val[j] = aabb_vol(&s_box[j * 6]);
  }
  __syncthreads();
  for (int r = 0; r < K; ++r) {
    const int w = s_order[r];
    if (s_state[w] == 0) continue;          // (uniform: no thread writes a state between two barriers it could read)
    if (tid == 0) s_state[w] = 2;
    const double *bw = &s_box[w * 6];
    const double aw = s_val[w];
    const int cw = s_cls[w];
#pragma unroll
    for (int q = 0; q < NMS_PER; ++q) {
      const int j = tid + q * NMS_THREADS;
      if (j < K && rank[q] > r && s_state[j] == 1) {
        const double inter = aabb_inter(bw, &s_box[j * 6]);
        double o = old_type ? inter / s_val[j] : inter / ((aw + s_val[j]) - inter);
        if (cls_nms) o = o * (cw == s_cls[j] ? 1.0 : 0.0);
        if (o > thr) s_state[j] = 0;
      }
    }
    __syncthreads();
  }
  for (int j = tid; j < K; j += NMS_THREADS) keep[b * K + j] = s_state[j] == 2 ? 1 : 0;
}

// ----------------------------------------------------------------------------------------------------------- match
// descending confidence, NaN last (np.argsort(-conf) puts -NaN last), ties by ascending index
__device__ __forceinline__ bool match_before(double ci, int i, double cj, int j) {
  const bool ni = ci != ci, nj = cj != cj;
  if (ni || nj) return !ni || (nj && i < j);
  return ci > cj || (ci == cj && i < j);
}

struct DetMatchArgs {
  const double *pred_aabb, *conf, *gt_aabb, *thresh;
  const int *pred_cls, *gt_cls;
  const unsigned char *pred_valid;
  unsigned char *tp;
  int S, K, G, C, T, conf_cols;
};

__global__ __launch_bounds__(EDA_WAVE) void det_match_kernel(const DetMatchArgs a) {
  extern __shared__ double s_dyn[];
  const int K = a.K, G = a.G;
  double *s_conf = s_dyn;                                   // K
  double *s_gt = s_conf + K;                                // G x 6: the scene's boxes of this class, ascending g
  short *s_order = (short *)(s_gt + (long)G * 6);           // K
  unsigned char *s_tp = (unsigned char *)(s_order + K);     // K: 0 not a prediction / FP, 1 TP
  const int lane = threadIdx.x;
  const long s = blockIdx.x;
  const int c = blockIdx.y, t = blockIdx.z;
  const double thr = a.thresh[t];
  const long base = s * K;
  // the segment's predictions
  int npred = 0;
  for (int j0 = 0; j0 < K; j0 += EDA_WAVE) {
    const int j = j0 + lane;
    bool isp = false;
    if (j < K) {
      isp = a.pred_valid[base + j] != 0 && (a.pred_cls == nullptr || a.pred_cls[base + j] == c);
      s_conf[j] = isp ? a.conf[(base + j) * a.conf_cols + (a.conf_cols == 1 ? 0 : c)] : 0.0;
      s_tp[j] = 0;
      s_order[j] = (short)(isp ? 1 : 0);                    // (membership until the ranks are written)
    }
    npred += __builtin_popcountll(__ballot(isp));
  }
  // the scene's ground truth of class c, compacted in ascending g
  int ng = 0;
  for (int g0 = 0; g0 < G; g0 += EDA_WAVE) {
    const int g = g0 + lane;
    const bool m = g < G && a.gt_cls[s * G + g] == c;
    const unsigned long long bal = __ballot(m);
    if (m) {
      const int q = ng + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      for (int e = 0; e < 6; ++e) s_gt[q * 6 + e] = a.gt_aabb[(s * G + g) * 6 + e];
    }
    ng += __builtin_popcountll(bal);
  }
  __syncthreads();
  int myrank[DET_MAXK / EDA_WAVE];
#pragma unroll
  for (int q = 0; q < DET_MAXK / EDA_WAVE; ++q) {
    const int j = lane + q * EDA_WAVE;
    myrank[q] = -1;
    if (j < K && s_order[j] == 1) {
      const double cj = s_conf[j];
      int r = 0;
      for (int i = 0; i < K; ++i) r += (s_order[i] != 0 && match_before(s_conf[i], i, cj, j)) ? 1 : 0;
      myrank[q] = r;
    }
  }
  __syncthreads();                                          // every membership read is done before the ranks land
#pragma unroll
  for (int q = 0; q < DET_MAXK / EDA_WAVE; ++q)
    if (myrank[q] >= 0) s_order[myrank[q]] = (short)(lane + q * EDA_WAVE);
  __syncthreads();
  if (ng > 0) {
    unsigned taken = 0;                                     // bit u of lane l: compacted box l + 64 u is matched
    for (int r = 0; r < npred; ++r) {
      const int p = s_order[r];
      const double *pb = a.pred_aabb + (base + p) * 6;
      double bp[6];
      for (int e = 0; e < 6; ++e) bp[e] = pb[e];
      const double vp = aabb_vol(bp);
      double best = -__builtin_inf();
      int bq = -1;
      for (int q = lane; q < ng; q += EDA_WAVE) {
        const double *gb = &s_gt[q * 6];
        const double inter = aabb_inter(bp, gb);
        const double iou = inter / ((vp + aabb_vol(gb)) - inter);
        if (iou > best) { best = iou; bq = q; }
      }
      // first maximum over the wave: larger IoU, then smaller index (a NaN IoU never entered `best`)
      for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oq = __shfl_xor(bq, off);
        if (ob > best || (ob == best && oq >= 0 && (bq < 0 || oq < bq))) { best = ob; bq = oq; }
      }
      if (best > thr) {
        const int owner = bq & (EDA_WAVE - 1), bit = bq >> 6;
        const bool was = (__shfl((int)taken, owner) >> bit) & 1;
        if (!was) {
          if (lane == owner) taken |= 1u << bit;
          if (lane == 0) s_tp[p] = 1;
        }
      }
    }
  }
  __syncthreads();
  unsigned char *tp = a.tp + (((long)t * a.C + c) * a.S + s) * K;
  for (int j = lane; j < K; j += EDA_WAVE) tp[j] = s_tp[j];
}

size_t det_match_lds_bytes(int K, int G) {               // <= 60 416 bytes at K = G = 1024
  return (size_t)K * (sizeof(double) + sizeof(short) + 1) + (size_t)G * 6 * sizeof(double);
}

}  // namespace

extern "C" int eda_det_decode_f32(const float *center, const float *pred_size, const float *sem_cls_scores,
                                  const float *obj_logits, int B, int K, int C1, double *aabb, float *obj_prob,
                                  float *cls_prob, int *sem_cls, void *stream) {
  EDA_CHECK_ARG(B >= 0 && K >= 0, "B and K must be >= 0");
  EDA_CHECK_ARG(C1 >= 2, "sem_cls_scores needs C + 1 >= 2 columns");
  EDA_CHECK_ARG(center && pred_size && sem_cls_scores && aabb && obj_prob && cls_prob && sem_cls, "null pointer");
  const long n = (long)B * K;
  if (n == 0) return 0;
  hipLaunchKernelGGL(det_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, center,
                     pred_size, sem_cls_scores, obj_logits, n, C1, aabb, obj_prob, cls_prob, sem_cls);
  EDA_CHECK_LAUNCH();
  return 0;
}

extern "C" int eda_det_nms_f64(const double *aabb, const double *score, const int *cls, int B, int K, double iou_thresh,
                               int old_type, int cls_nms, unsigned char *keep, void *stream) {
  EDA_CHECK_ARG(B >= 0 && B <= 0x7fffffff, "B must be >= 0");
  EDA_CHECK_ARG(K >= 1 && K <= DET_MAXK, "K must be in 1..1024");
  EDA_CHECK_ARG(aabb && score && keep, "null pointer");
  EDA_CHECK_ARG(!cls_nms || cls, "cls_nms needs the class array");
  if (B == 0) return 0;
  hipLaunchKernelGGL(det_nms_kernel, dim3((unsigned)B), dim3(NMS_THREADS), 0, (hipStream_t)stream, aabb, score, cls, K,
                     iou_thresh, old_type ? 1 : 0, cls_nms ? 1 : 0, keep);
  EDA_CHECK_LAUNCH();
  return 0;
}

extern "C" int eda_det_match_f64(const double *pred_aabb, const double *conf, int conf_cols, const int *pred_cls,
                                 const unsigned char *pred_valid, const double *gt_aabb, const int *gt_cls,
                                 const double *thresholds, int S, int K, int G, int C, int T, unsigned char *tp,
                                 void *stream) {
  EDA_CHECK_ARG(S >= 0, "S must be >= 0");
  EDA_CHECK_ARG(K >= 1 && K <= DET_MAXK, "K must be in 1..1024");
  EDA_CHECK_ARG(G >= 0 && G <= DET_MAXG, "G must be in 0..1024");
  EDA_CHECK_ARG(C >= 1 && C <= 65535 && T >= 1 && T <= 65535, "C and T must be in 1..65535");
  EDA_CHECK_ARG(conf_cols == 1 || conf_cols == C, "conf_cols must be 1 or C");
  EDA_CHECK_ARG(pred_aabb && conf && pred_valid && thresholds && tp && (G == 0 || (gt_aabb && gt_cls)), "null pointer");
  if (S == 0) return 0;
  DetMatchArgs a{pred_aabb, conf, gt_aabb, thresholds, pred_cls, gt_cls, pred_valid, tp, S, K, G, C, T, conf_cols};
  if (G == 0) {                                             // (no box to read: a valid pointer for the kernel's loops)
    a.gt_aabb = pred_aabb;
    a.gt_cls = nullptr;
  }
  const size_t lds = det_match_lds_bytes(K, G);
  hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)S, (unsigned)C, (unsigned)T), dim3(EDA_WAVE), lds,
                     (hipStream_t)stream, a);
  EDA_CHECK_LAUNCH();
  return 0;
}
