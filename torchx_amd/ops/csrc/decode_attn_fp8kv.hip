// fp8 (OCP e4m3) KV cache for the dense decode path, HD = 128, GQA:
// a prefill row quantiser, a quantising rope + append, and a decode
// attention kernel that reads every cached row ONCE for the whole GQA
// group. The bf16 cache and its kernels (decode_attn.hip, decode_core.h)
// are untouched.
//
// Cache layout: k8, v8 [B, T, Hkv, 128] e4m3 bytes, ks, vs [B, T, Hkv]
// fp32; the value stood for is k8 * ks. Quantisation contract, per (row,
// kv head) over the 128 bf16 values x (for K: the roped, bf16-rounded
// values the bf16 kernels would store):
//
//   amax  = max |x|
//   scale = amax / 448        (1.0 where amax == 0), fp32 IEEE division
//   y     = clamp(f32(x) / scale, -448, 448)      fp32 IEEE division
//   x8    = round-to-nearest-even(y) to e4m3      v_cvt_pk_fp8_f32
//
// The clamp is in front of the convert because the hardware convert turns
// overflow into NaN. ops.quantize_kv_rows is the same arithmetic in torch
// and both quantisers equal it bit for bit.
//
// Attention kernel (decode_attn_fp8kv_block):
//   work split  one 256-thread block per (b, kv head, head group[, slice])
//               serves HB = min(G, 4) q heads from one read of each row;
//               G = 8 runs two head groups.
//   lane map    8 lanes per cached row, 16 B = 16 d per lane; a wave load
//               covers 8 rows, the block 32. Wave w, slot r = lane >> 3
//               owns rows t_begin + 8 w + r + 32 i.
//   loads       the main loop takes U = 4 row iterations at a time: 4 K +
//               4 V 16-B loads and the 8 scale loads are issued before the
//               first convert (128 B per lane in flight). It runs while a
//               whole 128-row group fits the slice, so it needs no mask;
//               the tail takes one iteration at a time with the row
//               clamped into the slice and its score masked.
//   arithmetic  K: v_cvt_scalef32_pk_bf16_fp8 into v_dot2c_f32_bf16 against
//               the bf16 q pairs (QFrag); V: v_cvt_pk_f32_fp8 and fp32
//               FMAs. The converted fragment is shared by the HB heads.
//                 s_h = (ks[t] scale) * sum_d q_h[d] k8[d]
//               (row scale applied once, to the 8-lane-reduced sum),
//                 p = exp2(log2e (s - m)),  l += p,
//                 acc_h[d] += (p vs[t]) v8[d].
//               The running max moves once per U-row group (one alpha per
//               head per group). P stays fp32.
//   combine     the 8 row slots of a wave merge in registers (shfl_xor 8,
//               16, 32); 4 waves x HB heads x (m, l, o[128]) go through
//               LDS (8.3 KB at HB = 4) behind one barrier; wave 0 runs the
//               epilogue per head, 2 d per lane.
#include "common.h"

#define HD 128
#define FP8_MAX 448.0f
#define NEG_SCORE -3.0e38f
#define LOG2E_F 1.44269504f

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// ---- quantisation of one row held by a lane group ---------------------------

__device__ __forceinline__ float kv_row_scale(float amax) {
  return amax > 0.f ? amax / FP8_MAX : 1.0f;
}

__device__ __forceinline__ float kv_quant(float x, float scale) {
  return fminf(fmaxf(x / scale, -FP8_MAX), FP8_MAX);
}

// ---- prefill side: quantise and store S rows of K and V ---------------------
// 16 lanes per (row, kv head): one 16-B load (8 bf16), a 16-lane fmaxf
// butterfly, two v_cvt_pk_fp8_f32 pairs per 4 bytes, one 8-B store. A block
// holds 16 items; blockIdx.y picks K or V.
__global__ void __launch_bounds__(256)
kv_quantize_store_kernel(const unsigned short* __restrict__ k,  // [B,S,Hkv,128]
                         const unsigned short* __restrict__ v,
                         unsigned char* __restrict__ k8,  // [B,T,Hkv,128]
                         unsigned char* __restrict__ v8,
                         float* __restrict__ ks,  // [B,T,Hkv]
                         float* __restrict__ vs, long n_items, int S, int Hkv,
                         int T, int start) {
  const unsigned short* __restrict__ src = blockIdx.y ? v : k;
  unsigned char* __restrict__ dst8 = blockIdx.y ? v8 : k8;
  float* __restrict__ dsts = blockIdx.y ? vs : ks;
  const int dl = threadIdx.x & 15;
  const long item = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = item < n_items;
  const long it = live ? item : n_items - 1;  // whole 16-lane groups agree
  const long h = it % Hkv;
  const long bs = it / Hkv;
  const long s = bs % S;
  const long b = bs / S;
  const long drow = (b * T + start + s) * Hkv + h;

  const ushort8 xv = *(const ushort8*)(src + it * HD + dl * 8);
  float x[8];
  float amax = 0.f;
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = bf16_to_f32(xv[j]);
    amax = fmaxf(amax, fabsf(x[j]));
  }
  #pragma unroll
  for (int off = 8; off >= 1; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 16));
  const float scale = kv_row_scale(amax);
  #pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = kv_quant(x[j], scale);
  uint2_v out;
  out[0] = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0u, false);
  out[0] = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], out[0], true);
  out[1] = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0u, false);
  out[1] = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], out[1], true);
  if (live) {
    *(uint2_v*)(dst8 + drow * HD + dl * 8) = out;
    if (dl == 0) dsts[drow] = scale;
  }
}

extern "C" void kv_quantize_store_launch(const void* k, const void* v,
                                         void* k8, void* v8, void* ks,
                                         void* vs, int B, int S, int Hkv,
                                         int T, int start,
                                         hipStream_t stream) {
  const long n_items = (long)B * S * Hkv;
  hipLaunchKernelGGL(kv_quantize_store_kernel,
                     dim3((unsigned)((n_items + 15) / 16), 2), dim3(256), 0,
                     stream, (const unsigned short*)k,
                     (const unsigned short*)v, (unsigned char*)k8,
                     (unsigned char*)v8, (float*)ks, (float*)vs, n_items, S,
                     Hkv, T, start);
}

// ---- decode side: rope + quantising append of ONE position ------------------
// decode_rope_cache_kernel's contract (host pos, device scalar or device
// [B]); one wave per head of the packed qkv row, lane owns the rotation
// pair (lane, lane + 64). q heads: the same fmaf expressions as
// decode_rope_append. A k head is roped, rounded to bf16, quantised; a v
// head is quantised raw. The amax is a 64-lane reduce over the lane's two
// elements. The two bytes of a lane go out as byte stores (a wave's stores
// cover two runs of 64 consecutive bytes): this is a latency-floor kernel
// and a lane exchange to 4-byte stores only adds dependent instructions.
// `pos` is clamped to [0, T) and to the rope table.
__global__ void __launch_bounds__(64)
decode_rope_cache_fp8kv_kernel(const unsigned short* __restrict__ qkv,
                               unsigned short* __restrict__ qout,
                               unsigned char* __restrict__ k8,
                               unsigned char* __restrict__ v8,
                               float* __restrict__ ks, float* __restrict__ vs,
                               const float* __restrict__ cos_t,  // [R, 64]
                               const float* __restrict__ sin_t,
                               const int* __restrict__ pos_dev, int B, int Hq,
                               int Hkv, int T, int rope_rows, int pos_host,
                               int per_row) {
  const int nh = Hq + 2 * Hkv;
  const int b = blockIdx.x / nh;
  const int h = blockIdx.x % nh;
  const int lane = threadIdx.x;
  int pos = pos_dev ? pos_dev[per_row ? b : 0] : pos_host;
  pos = min(max(pos, 0), min(T, rope_rows) - 1);
  const unsigned short* src = qkv + ((long)b * nh + h) * HD;
  float y1 = bf16_to_f32(src[lane]);
  float y2 = bf16_to_f32(src[lane + 64]);
  if (h < Hq + Hkv) {  // q or k head: rotate, round to bf16
    const float c = cos_t[(long)pos * 64 + lane];
    const float s = sin_t[(long)pos * 64 + lane];
    const unsigned short r1 = f32_to_bf16(fmaf(y1, c, -s * y2));
    const unsigned short r2 = f32_to_bf16(fmaf(y2, c, s * y1));
    if (h < Hq) {
      unsigned short* dst = qout + ((long)b * Hq + h) * HD;
      dst[lane] = r1;
      dst[lane + 64] = r2;
      return;  // wave-uniform
    }
    y1 = bf16_to_f32(r1);
    y2 = bf16_to_f32(r2);
  }
  const bool is_k = h < Hq + Hkv;
  const long drow =
      ((long)b * T + pos) * Hkv + (is_k ? h - Hq : h - Hq - Hkv);
  const float amax = wave_reduce_max(fmaxf(fabsf(y1), fabsf(y2)));
  const float scale = kv_row_scale(amax);
  const unsigned int pk = __builtin_amdgcn_cvt_pk_fp8_f32(
      kv_quant(y1, scale), kv_quant(y2, scale), 0u, false);
  unsigned char* dst = (is_k ? k8 : v8) + drow * HD;
  dst[lane] = (unsigned char)(pk & 0xffu);
  dst[lane + 64] = (unsigned char)((pk >> 8) & 0xffu);
  if (lane == 0) (is_k ? ks : vs)[drow] = scale;
}

extern "C" void decode_rope_cache_fp8kv_launch(
    const void* qkv, void* qout, void* k8, void* v8, void* ks, void* vs,
    const void* cos_t, const void* sin_t, const void* pos_dev, int B, int Hq,
    int Hkv, int T, int rope_rows, int pos_host, int per_row,
    hipStream_t stream) {
  hipLaunchKernelGGL(decode_rope_cache_fp8kv_kernel,
                     dim3(B * (Hq + 2 * Hkv)), dim3(64), 0, stream,
                     (const unsigned short*)qkv, (unsigned short*)qout,
                     (unsigned char*)k8, (unsigned char*)v8, (float*)ks,
                     (float*)vs, (const float*)cos_t, (const float*)sin_t,
                     (const int*)pos_dev, B, Hq, Hkv, T, rope_rows, pos_host,
                     per_row);
}

// ---- attention ---------------------------------------------------------------

// 16 e4m3 bytes -> 16 floats (8 v_cvt_pk_f32_fp8)
__device__ __forceinline__ void fp8x16_to_f32(const uint4_v w, float (&f)[16]) {
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    f[4 * i + 0] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// The lane's q fragment of HB heads and its dot product with 16 K bytes,
// in the two convert forms. KDOT = true (what the ops run, 1.2x to 1.7x
// faster where the cache streams): the raw bf16 q pairs, K through
// v_cvt_scalef32_pk_bf16_fp8 into v_dot2c_f32_bf16 as in gemv_fp8.hip
// (byte pair (dword i, sel) meets q pair 2 i + sel; every e4m3 value is
// exact in bf16), 8 dot2, and `scale` moves behind the sum, into the
// row-scale multiply: s_h = (ks[t] scale) * sum_d q_h[d] k8[d]. KDOT =
// false (kept for the measurement in docs/kernels.md): q * scale in fp32,
// K through v_cvt_pk_f32_fp8, 16 FMAs.
template <int HB, bool KDOT>
struct QFrag {
  float v[HB][16];
  __device__ __forceinline__ void load(const unsigned short* qp, int dchunk,
                                       float scale) {
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      const ushort8 a = *(const ushort8*)(qp + h * HD + dchunk);
      const ushort8 c = *(const ushort8*)(qp + h * HD + dchunk + 8);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[h][j] = bf16_to_f32(a[j]) * scale;
        v[h][8 + j] = bf16_to_f32(c[j]) * scale;
      }
    }
  }
  __device__ __forceinline__ float row_scale(float ks) const { return ks; }
  __device__ __forceinline__ void dot(const uint4_v kq, float (&d)[HB]) const {
    float kf[16];
    fp8x16_to_f32(kq, kf);
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      d[h] = 0.f;
      #pragma unroll
      for (int j = 0; j < 16; ++j) d[h] = fmaf(v[h][j], kf[j], d[h]);
    }
  }
};

template <int HB>
struct QFrag<HB, true> {
  uint4_v v[HB][2];  // 8 bf16 pairs per head
  float scale;
  __device__ __forceinline__ void load(const unsigned short* qp, int dchunk,
                                       float sc) {
    scale = sc;
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      v[h][0] = *(const uint4_v*)(qp + h * HD + dchunk);
      v[h][1] = *(const uint4_v*)(qp + h * HD + dchunk + 8);
    }
  }
  __device__ __forceinline__ float row_scale(float ks) const {
    return ks * scale;
  }
  __device__ __forceinline__ void dot(const uint4_v kq, float (&d)[HB]) const {
    #pragma unroll
    for (int h = 0; h < HB; ++h) d[h] = 0.f;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x2 kp[2] = {
          __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(kq[i], 1.0f, false),
          __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(kq[i], 1.0f, true)};
      #pragma unroll
      for (int sel = 0; sel < 2; ++sel) {
        const int p = 2 * i + sel;
        #pragma unroll
        for (int h = 0; h < HB; ++h)
          d[h] = __builtin_amdgcn_fdot2_f32_bf16(
              ((const bf16x2*)&v[h][p >> 2])[p & 3], kp[sel], d[h], false);
      }
    }
  }
};

// Online-softmax state of one lane: HB heads x (m, l, 16 d of the
// accumulator). All 8 lanes of a row slot hold the same m and l.
template <int HB>
struct Fp8kvState {
  float m[HB], l[HB], acc[HB][16];
};

// U row iterations starting at block row `tb` (this lane: rows tb + 32 u).
// MASK: rows at or past t_end are clamped to t_end - 1 for the loads and
// contribute nothing.
template <int HB, int U, bool MASK, bool KDOT>
__device__ __forceinline__ void fp8kv_group(
    Fp8kvState<HB>& st, const QFrag<HB, KDOT>& qf,
    const unsigned char* __restrict__ kb, const unsigned char* __restrict__ vb,
    const float* __restrict__ ksb, const float* __restrict__ vsb, int Hkv,
    int tb, int t_end, int dchunk) {
  uint4_v kq[U], vq[U];
  float ksc[U], vsc[U];
  bool ok[U];
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = tb + 32 * u;
    ok[u] = !MASK || t < t_end;
    const long row = (long)(ok[u] ? t : t_end - 1) * Hkv;
    kq[u] = *(const uint4_v*)(kb + row * HD + dchunk);
    ksc[u] = ksb[row];
    vq[u] = *(const uint4_v*)(vb + row * HD + dchunk);
    vsc[u] = vsb[row];
  }

  float s[U][HB];
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    float dh[HB];
    qf.dot(kq[u], dh);
    const float rs = qf.row_scale(ksc[u]);
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      float d = dh[h];
      #pragma unroll
      for (int off = 4; off >= 1; off >>= 1) d += __shfl_xor(d, off, 8);
      s[u][h] = ok[u] ? d * rs : NEG_SCORE;
    }
  }

  float pv[U][HB];
  #pragma unroll
  for (int h = 0; h < HB; ++h) {
    float m_new = st.m[h];
    #pragma unroll
    for (int u = 0; u < U; ++u) m_new = fmaxf(m_new, s[u][h]);
    const float alpha =
        __builtin_amdgcn_exp2f(LOG2E_F * (st.m[h] - m_new));
    float l = st.l[h] * alpha;
    #pragma unroll
    for (int j = 0; j < 16; ++j) st.acc[h][j] *= alpha;
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const float e = __builtin_amdgcn_exp2f(LOG2E_F * (s[u][h] - m_new));
      const float p = ok[u] ? e : 0.f;  // a slot of masked rows only: m = NEG
      l += p;
      pv[u][h] = p * vsc[u];
    }
    st.l[h] = l;
    st.m[h] = m_new;
  }

  #pragma unroll
  for (int u = 0; u < U; ++u) {
    float vf[16];
    fp8x16_to_f32(vq[u], vf);
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      #pragma unroll
      for (int j = 0; j < 16; ++j)
        st.acc[h][j] = fmaf(pv[u][h], vf[j], st.acc[h][j]);
    }
  }
}

// The block body. `qp` points at q[b, hq0, 0] (HB consecutive heads), kb /
// vb at byte 0 of the kv head in row 0 of sequence b, ksb / vsb at its
// scale in row 0. SPLIT: store the unnormalised (m, l, o) partial of slice
// `slice` for decode_attn_merge_kernel; otherwise normalise and store bf16.
template <int HB, bool SPLIT, bool KDOT>
__device__ __forceinline__ void decode_attn_fp8kv_block(
    const unsigned short* __restrict__ qp,
    const unsigned char* __restrict__ kb, const unsigned char* __restrict__ vb,
    const float* __restrict__ ksb, const float* __restrict__ vsb, int Hkv,
    int t_begin, int t_end, float scale, unsigned short* __restrict__ o,
    float* __restrict__ ml, float* __restrict__ oacc, long bq0, int split,
    int slice) {
  constexpr int U = 4;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int dchunk = (lane & 7) * 16;

  QFrag<HB, KDOT> qf;
  qf.load(qp, dchunk, scale);

  Fp8kvState<HB> st;
  #pragma unroll
  for (int h = 0; h < HB; ++h) {
    st.m[h] = NEG_SCORE;
    st.l[h] = 0.f;
    #pragma unroll
    for (int j = 0; j < 16; ++j) st.acc[h][j] = 0.f;
  }

  // block-uniform loop bounds; `mine` is this lane's row offset in a
  // 32-row iteration
  const int mine = 8 * wave + (lane >> 3);
  int tb = t_begin;
  for (; tb + 32 * U <= t_end; tb += 32 * U)
    fp8kv_group<HB, U, false, KDOT>(st, qf, kb, vb, ksb, vsb, Hkv, tb + mine, t_end,
                              dchunk);
  for (; tb < t_end; tb += 32)
    fp8kv_group<HB, 1, true, KDOT>(st, qf, kb, vb, ksb, vsb, Hkv, tb + mine, t_end,
                             dchunk);

  // the wave's 8 row slots -> one state, in registers
  #pragma unroll
  for (int off = 8; off <= 32; off <<= 1) {
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      const float m_o = __shfl_xor(st.m[h], off, 64);
      const float l_o = __shfl_xor(st.l[h], off, 64);
      const float m_n = fmaxf(st.m[h], m_o);
      const float wa = __builtin_amdgcn_exp2f(LOG2E_F * (st.m[h] - m_n));
      const float wb = __builtin_amdgcn_exp2f(LOG2E_F * (m_o - m_n));
      st.l[h] = st.l[h] * wa + l_o * wb;
      #pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float a_o = __shfl_xor(st.acc[h][j], off, 64);
        st.acc[h][j] = st.acc[h][j] * wa + a_o * wb;
      }
      st.m[h] = m_n;
    }
  }

  // 4 waves x HB heads through LDS, one barrier
  __shared__ float sm[4][HB], sl[4][HB];
  __shared__ __attribute__((aligned(16))) float so[4][HB][HD];
  if (lane < 8) {
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      if (lane == 0) {
        sm[wave][h] = st.m[h];
        sl[wave][h] = st.l[h];
      }
      #pragma unroll
      for (int j = 0; j < 16; j += 4)
        *(f32x4*)&so[wave][h][dchunk + j] =
            f32x4{st.acc[h][j], st.acc[h][j + 1], st.acc[h][j + 2],
                  st.acc[h][j + 3]};
    }
  }
  __syncthreads();

  if (wave == 0) {
    const int d = lane * 2;
    #pragma unroll
    for (int h = 0; h < HB; ++h) {
      float m_t = NEG_SCORE;
      #pragma unroll
      for (int i = 0; i < 4; ++i) m_t = fmaxf(m_t, sm[i][h]);
      float l_t = 0.f, o0 = 0.f, o1 = 0.f;
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float w = __builtin_amdgcn_exp2f(LOG2E_F * (sm[i][h] - m_t));
        l_t += sl[i][h] * w;
        o0 = fmaf(so[i][h][d], w, o0);
        o1 = fmaf(so[i][h][d + 1], w, o1);
      }
      if (SPLIT) {
        const long p = (bq0 + h) * split + slice;
        if (lane == 0) {
          ml[p * 2] = m_t;  // m = NEG, l = 0 for an empty slice
          ml[p * 2 + 1] = l_t;
        }
        *(f32x2*)(oacc + p * HD + d) = f32x2{o0, o1};
      } else {
        const float inv = (l_t > 0.f) ? 1.0f / l_t : 0.f;
        const unsigned int pk =
            (unsigned int)f32_to_bf16(o0 * inv) |
            ((unsigned int)f32_to_bf16(o1 * inv) << 16);
        *(unsigned int*)(o + (bq0 + h) * HD + d) = pk;
      }
    }
  }
}

// grid.x = B * Hkv * NG with NG = G / HB head groups per kv head; grid.y =
// split. Length rule as dense_len: len_dev ? len_dev[per_row ? b : 0] + 1
// : L_host, clamped to [0, T]; chunk = ceil(L / split).
template <int G, bool SPLIT, bool KDOT>
__global__ void __launch_bounds__(256)
decode_attn_fp8kv_kernel(const unsigned short* __restrict__ q,  // [B,Hq,128]
                         const unsigned char* __restrict__ k8,  // [B,T,Hkv,128]
                         const unsigned char* __restrict__ v8,
                         const float* __restrict__ ks,  // [B,T,Hkv]
                         const float* __restrict__ vs,
                         unsigned short* __restrict__ o,  // [B,Hq,128]
                         float* __restrict__ ml,    // [B*Hq, split, 2]
                         float* __restrict__ oacc,  // [B*Hq, split, 128]
                         const int* __restrict__ len_dev, int Hkv, int T,
                         int L_host, int per_row, float scale) {
  constexpr int HB = G < 4 ? G : 4;
  constexpr int NG = G / HB;
  const int grp = blockIdx.x % NG;
  const int hkv = (blockIdx.x / NG) % Hkv;
  const int b = blockIdx.x / (NG * Hkv);
  const int Hq = Hkv * G;
  int L = len_dev ? (len_dev[per_row ? b : 0] + 1) : L_host;
  L = min(max(L, 0), T);
  const int split = SPLIT ? (int)gridDim.y : 1;
  const int chunk = (L + split - 1) / split;
  const int t0 = SPLIT ? (int)blockIdx.y * chunk : 0;
  const int t1 = min(L, t0 + chunk);
  const long bq0 = (long)b * Hq + (long)hkv * G + grp * HB;
  const long row0 = (long)b * T * Hkv + hkv;
  decode_attn_fp8kv_block<HB, SPLIT, KDOT>(
      q + bq0 * HD, k8 + row0 * HD, v8 + row0 * HD, ks + row0, vs + row0, Hkv,
      t0, t1, scale, o, ml, oacc, bq0, split, (int)blockIdx.y);
}

template <int G, bool SPLIT, bool KDOT>
static void fp8kv_launch_one(const void* q, const void* k8, const void* v8,
                             const void* ks, const void* vs, void* o,
                             void* ml, void* oacc, const void* len_dev,
                             int B, int Hkv, int T, int L, int split,
                             int per_row, float scale, hipStream_t stream) {
  constexpr int NG = G / (G < 4 ? G : 4);
  hipLaunchKernelGGL((decode_attn_fp8kv_kernel<G, SPLIT, KDOT>),
                     dim3(B * Hkv * NG, split), dim3(256), 0, stream,
                     (const unsigned short*)q, (const unsigned char*)k8,
                     (const unsigned char*)v8, (const float*)ks,
                     (const float*)vs, (unsigned short*)o, (float*)ml,
                     (float*)oacc, (const int*)len_dev, Hkv, T, L, per_row,
                     scale);
}

template <int G>
static void fp8kv_launch_g(const void* q, const void* k8, const void* v8,
                           const void* ks, const void* vs, void* o, void* ml,
                           void* oacc, const void* len_dev, int B, int Hkv,
                           int T, int L, int split, int per_row, float scale,
                           int kdot2, hipStream_t stream) {
  auto fn = split > 1
                ? (kdot2 ? fp8kv_launch_one<G, true, true>
                         : fp8kv_launch_one<G, true, false>)
                : (kdot2 ? fp8kv_launch_one<G, false, true>
                         : fp8kv_launch_one<G, false, false>);
  fn(q, k8, v8, ks, vs, o, ml, oacc, len_dev, B, Hkv, T, L, split, per_row,
     scale, stream);
}

// The merge of the split partials, shared with the bf16 kernels
// (decode_attn.hip).
extern "C" void decode_attn_merge_launch(const void* ml, const void* oacc,
                                         void* o, int BHq, int split,
                                         hipStream_t stream);

// G = Hq / Hkv must be 1, 2, 4 or 8 (checked by the binding). split == 1 is
// the single-pass kernel; split > 1 writes partials and runs the merge.
// kdot2 selects the dot2 convert form of the QK product (QFrag).
extern "C" void decode_attn_fp8kv_launch(const void* q, const void* k8,
                                         const void* v8, const void* ks,
                                         const void* vs, void* o, void* ml,
                                         void* oacc, const void* len_dev,
                                         int B, int Hq, int Hkv, int T, int L,
                                         int split, int per_row, float scale,
                                         int kdot2, hipStream_t stream) {
  switch (Hq / Hkv) {
    case 1:
      fp8kv_launch_g<1>(q, k8, v8, ks, vs, o, ml, oacc, len_dev, B, Hkv, T, L,
                        split, per_row, scale, kdot2, stream);
      break;
    case 2:
      fp8kv_launch_g<2>(q, k8, v8, ks, vs, o, ml, oacc, len_dev, B, Hkv, T, L,
                        split, per_row, scale, kdot2, stream);
      break;
    case 4:
      fp8kv_launch_g<4>(q, k8, v8, ks, vs, o, ml, oacc, len_dev, B, Hkv, T, L,
                        split, per_row, scale, kdot2, stream);
      break;
    default:
      fp8kv_launch_g<8>(q, k8, v8, ks, vs, o, ml, oacc, len_dev, B, Hkv, T, L,
                        split, per_row, scale, kdot2, stream);
      break;
  }
  if (split > 1)
    decode_attn_merge_launch(ml, oacc, o, B * Hq, split, stream);
}
