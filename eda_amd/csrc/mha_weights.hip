// mha_weights.hip -- the attention PROBABILITIES of a forward that has already run (eda_mha_weights_f32, include/eda_hip.h).
//
// torch.nn.MultiheadAttention returns them with need_weights=True (head-averaged unless average_attn_weights=False); the
// reference throws them away ([0] of every call, models/encoder_decoder_layers.py:87-117, 149-153, 179-183, 366-401) and the
// fused kernels of csrc/mha2.hip never hold them.  The forward leaves lse[b,h,q] = ln sum_k exp(scale q.k) over the
// unmasked keys, so every probability is exp(scale q.k - lse) on its own: ONE pass over (query tile x key tile), no
// softmax reduction, no (B,H,Lq,Lk) intermediate for the head mean, no workspace, no atomics -- the same inputs give the
// same bits.
//
// Workgroup = 4 waves = 64 queries x 64 keys of one scene, looping over the heads 0..H-1 in order.  Per head: the 64 x 36
// K tile is staged in LDS (global -> registers one head ahead -> LDS double buffer, one barrier per head), every wave
// holds its 16 queries' operand in registers, S^T = K Q^T on v_mfma_f32_16x16x4_f32 (9 contraction steps, operand
// layout of mha2.hip's load_row_operand), p = exp2(S^T - lse log2 e) with log2(e) folded into the query scale as in the
// forward, dropout keep mask regenerated from the forward's hash (one 32-bit hash per key pair), head sum in registers.
// MFMA row i of key sub-tile j is key 16 (i / 4) + 4 j + (i % 4) of the tile -- so a lane ends up with 16 CONSECUTIVE
// keys of one query (four sub-tiles x four accumulator registers) and the tile leaves as one 64-byte run per lane, 256
// bytes per query row and wave; the LDS image is stored in MFMA row order (row stride 36: conflict-free b128 reads).
#include "eda_common.h"

namespace {

constexpr int HD = 36;
constexpr int KSTEPS = 9;
constexpr int TQ = 64, TK = 64;
constexpr int KGRAN = TK * HD / 4;          // 16-byte granules of a K tile (576)
constexpr float LOG2E = 1.4426950408889634f;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WeightsArgs {
  const float *q, *k;
  long q_sb, q_sl, k_sb, k_sl;
  const unsigned char *mask;
  const float *lse;
  int B, H, Lq, Lk;
  float scale, p_drop;
  const unsigned long long *seed_ptr;
  unsigned salt;
  float *w;
  int n_qt, n_kt;
  int vec;          // rows of w are 16-byte aligned (Lk % 4 == 0 and w aligned): float4 stores
};

__device__ __forceinline__ unsigned hash32(unsigned x) {          // the mask hash of csrc/mha2.hip
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}

// k-step s of lane group g contracts head dim 8g+s (s < 8) and 32+g (s = 8), as in mha2.hip
__device__ __forceinline__ void load_row_operand(float (&r)[KSTEPS], const float *row, int g) {
  const float4 x = *reinterpret_cast<const float4 *>(row + 8 * g);
  const float4 y = *reinterpret_cast<const float4 *>(row + 8 * g + 4);
  r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w;
  r[4] = y.x; r[5] = y.y; r[6] = y.z; r[7] = y.w;
  r[8] = row[32 + g];
}

template <bool DROP, bool PER_HEAD>
__global__ __launch_bounds__(256) void mha_weights_kernel(const WeightsArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[2][TK * HD];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const unsigned bid = blockIdx.x;
  const int kt = (int)(bid % (unsigned)a.n_kt);
  const unsigned rest = bid / (unsigned)a.n_kt;
  const int qt = (int)(rest % (unsigned)a.n_qt);
  const int b = (int)(rest / (unsigned)a.n_qt);
  const int k0 = kt * TK, q0 = qt * TQ;
  const int qi = q0 + 16 * wave + c;
  const bool qvalid = qi < a.Lq;
  const int qc = min(qi, a.Lq - 1);
  const bool wave_live = q0 + 16 * wave < a.Lq;          // uniform: any valid query in this wave

  // this lane's 16 keys are k0 + 16 g + [0, 16): bit i = key i is masked or beyond Lk
  unsigned dead = 0;
  {
    const unsigned char *mrow = a.mask ? a.mask + (long)b * a.Lk : nullptr;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = k0 + 16 * g + i;
      unsigned d = key >= a.Lk ? 1u : 0u;
      if (key < a.Lk && mrow) d = mrow[key] ? 1u : 0u;
      dead |= d << i;
    }
  }

  unsigned seed = 0u, thresh = 0u;
  float inv_keep = 1.f;
  if (DROP) {
    seed = hash32((unsigned)(*a.seed_ptr) * 0x9E3779B1u + a.salt);
    thresh = (unsigned)((double)a.p_drop * 65536.0 + 0.5);
    inv_keep = 1.f / (1.f - a.p_drop);
  }

  // K tile of the next head: global -> registers (rows beyond Lk repeat the last key; they are never stored)
  // (granule i of the tile = 16 bytes c4 of key row i / 9; thread t moves granules t, t + 256 and -- wave 0 only -- t + 512)
  const float *kb = a.k + (long)b * a.k_sb;
  const float *ksrc[3];
  int kdst[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int i = min(tid + 256 * u, KGRAN - 1);
    const int row = i / 9, c4 = i - 9 * row;
    ksrc[u] = kb + (long)min(k0 + row, a.Lk - 1) * a.k_sl + 4 * c4;
    kdst[u] = (16 * ((row >> 2) & 3) + 4 * (row >> 4) + (row & 3)) * HD + 4 * c4;       // sub-tile, MFMA row
  }
  const bool third = tid + 512 < KGRAN;
  float4 kst0, kst1, kst2;
  auto kload = [&](int h) {
    kst0 = *reinterpret_cast<const float4 *>(ksrc[0] + h * HD);
    kst1 = *reinterpret_cast<const float4 *>(ksrc[1] + h * HD);
    kst2 = *reinterpret_cast<const float4 *>(ksrc[2] + h * HD);
  };
  auto kstore = [&](float *dst) {
    *reinterpret_cast<float4 *>(dst + kdst[0]) = kst0;
    *reinterpret_cast<float4 *>(dst + kdst[1]) = kst1;
    if (third) *reinterpret_cast<float4 *>(dst + kdst[2]) = kst2;
  };
  float qn[KSTEPS], lse_n;
  const float *qb = a.q + (long)b * a.q_sb + (long)qc * a.q_sl;
  auto qload = [&](int h) {
    load_row_operand(qn, qb + h * HD, g);
    lse_n = a.lse[((long)b * a.H + h) * a.Lq + qc];
  };

  kload(0);
  qload(0);
  kstore(Ks[0]);
  __syncthreads();

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sc = a.scale * LOG2E;
  const float inv_h = 1.f / (float)a.H;

  auto emit = [&](float *row, const f32x4 (&v)[4]) {
    if (!qvalid) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k0 + 16 * g + 4 * j;
      if (a.vec) {
        if (kk < a.Lk) *reinterpret_cast<float4 *>(row + kk) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kk + r < a.Lk) row[kk + r] = v[j][r];
      }
    }
  };

#pragma unroll 1
  for (int h = 0; h < a.H; ++h) {
    float qreg[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) qreg[s] = qn[s] * sc;
    const float l2 = lse_n * LOG2E;
    if (h + 1 < a.H) {
      kload(h + 1);
      qload(h + 1);
    }
    if (wave_live) {
      const float *Kt = Ks[h & 1];
      f32x4 st[4];
      {
        float kreg[4][KSTEPS];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
          load_row_operand(kreg[j], Kt + (16 * j + c) * HD, g);
        }
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
          for (int j = 0; j < 4; ++j) st[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kreg[j][s], qreg[s], st[j], 0, 0, 0);
      }
      const unsigned rowbase = (((unsigned)b * (unsigned)a.H + (unsigned)h) * (unsigned)a.Lq + (unsigned)qi) * (unsigned)a.Lk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __builtin_amdgcn_exp2f(st[j][r] - l2);
          p = ((dead >> (4 * j + r)) & 1u) ? 0.f : p;            // masked keys: exactly 0
          st[j][r] = p;
        }
        if (DROP) {
#pragma unroll
          for (int r2 = 0; r2 < 4; r2 += 2) {
            const unsigned hh = hash32(seed ^ (rowbase + (unsigned)(k0 + 16 * g + 4 * j + r2)));
            st[j][r2] = (hh & 0xffffu) >= thresh ? st[j][r2] * inv_keep : 0.f;
            st[j][r2 + 1] = (hh >> 16) >= thresh ? st[j][r2 + 1] * inv_keep : 0.f;
          }
        }
        if (l2 == -INFINITY) st[j] = f32x4{NAN, NAN, NAN, NAN};     // every key masked: NaN row, like the forward
        if (!PER_HEAD) acc[j] += st[j];
      }
      if (PER_HEAD) emit(a.w + (((long)b * a.H + h) * a.Lq + qi) * (long)a.Lk, st);
    }
    if (h + 1 < a.H) kstore(Ks[(h + 1) & 1]);
    __syncthreads();
  }
  if (!PER_HEAD && wave_live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] *= inv_h;
    emit(a.w + ((long)b * a.Lq + qi) * (long)a.Lk, acc);
  }
}

inline bool mult4(long x) { return (x & 3) == 0; }
inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int eda_mha_weights_f32(const float *q, const float *k, long q_sb, long q_sl, long k_sb, long k_sl,
                                   const unsigned char *key_padding_mask, const float *lse, int B, int H, int Lq, int Lk,
                                   int head_dim, float scale, float p_drop, const unsigned long long *seed_ptr,
                                   unsigned salt, int per_head, float *weights, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (head_dim != HD || H < 1 || H > 8) {
    eda_set_error("%s: only head_dim 36 and 1..8 heads are built (head_dim %d, H %d)", __func__, head_dim, H);
    return EDA_ERR_UNSUPPORTED;
  }
  EDA_CHECK_ARG(B >= 0 && Lq >= 0 && Lk >= 0, "bad dimension");
  EDA_CHECK_ARG(per_head == 0 || per_head == 1, "per_head must be 0 or 1");
  if (B == 0 || Lq == 0 || Lk == 0) return 0;          // nothing to write
  EDA_CHECK_ARG(q && k && lse && weights, "null pointer");
  EDA_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || seed_ptr), "bad dropout arguments");
  EDA_CHECK_ARG(mult4(q_sb) && mult4(q_sl) && mult4(k_sb) && mult4(k_sl) && al16(q) && al16(k),
                "rows must be 16-byte aligned");
  EDA_CHECK_ARG(((uintptr_t)weights & 3) == 0 && ((uintptr_t)lse & 3) == 0, "weights / lse must be 4-byte aligned");
  WeightsArgs a = {};
  a.q = q; a.k = k; a.q_sb = q_sb; a.q_sl = q_sl; a.k_sb = k_sb; a.k_sl = k_sl;
  a.mask = key_padding_mask; a.lse = lse; a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  a.scale = scale; a.p_drop = p_drop; a.seed_ptr = seed_ptr; a.salt = salt; a.w = weights;
  a.n_qt = (Lq + TQ - 1) / TQ;
  a.n_kt = (Lk + TK - 1) / TK;
  a.vec = (Lk % 4 == 0 && al16(weights)) ? 1 : 0;
  const long blocks = (long)B * a.n_qt * a.n_kt;
  if (blocks > 0x7fffffffL) {
    eda_set_error("%s: %ld workgroups do not fit one launch", __func__, blocks);
    return EDA_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)blocks), block(256);
  const bool drop = p_drop > 0.f;
  if (drop && per_head) hipLaunchKernelGGL((mha_weights_kernel<true, true>), grid, block, 0, stream, a);
  else if (drop) hipLaunchKernelGGL((mha_weights_kernel<true, false>), grid, block, 0, stream, a);
  else if (per_head) hipLaunchKernelGGL((mha_weights_kernel<false, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((mha_weights_kernel<false, false>), grid, block, 0, stream, a);
  EDA_CHECK_LAUNCH();
  return 0;
}
