// The bodies of the fp8 (OCP e4m3) KV-cache kernels, HD = 128, GQA, shared
// by the dense kernels (decode_attn_fp8kv.hip) and the paged ones
// (paged_attn_fp8kv.hip): the row quantisers of the prefill store and of
// the rope + append, and the decode attention block. The quantisation
// contract and the attention design are described at the top of
// decode_attn_fp8kv.hip. A kernel chooses at compile time where row t of
// the cache lives (a row source, below); every arithmetic expression is the
// same, in the same order, which is why the paged and dense outputs are
// bit-identical on the same logical cache.
#pragma once

#include "decode_core.h"

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

// 8 floats -> 8 e4m3 bytes in element order (clamp, then two
// v_cvt_pk_fp8_f32 pairs per 4 bytes).
__device__ __forceinline__ uint2_v kv_quant_pack8(const float (&x)[8],
                                                  float scale) {
  float y[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = kv_quant(x[j], scale);
  uint2_v out;
  out[0] = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0u, false);
  out[0] = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], out[0], true);
  out[1] = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0u, false);
  out[1] = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], out[1], true);
  return out;
}

// Prefill side, one (row, kv head) item on 16 lanes: one 16-B load (8 bf16)
// of source row `it`, a 16-lane fmaxf butterfly, two v_cvt_pk_fp8_f32 pairs
// per 4 bytes, one 8-B store to row `drow` of dst8 and its scale. `dl` is
// the lane of the 16; a lane group that is not `live` computes on a valid
// source row and stores nothing.
__device__ __forceinline__ void kv_quantize_item(
    const unsigned short* __restrict__ src, long it,
    unsigned char* __restrict__ dst8, float* __restrict__ dsts, long drow,
    int dl, bool live) {
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
  const uint2_v out = kv_quant_pack8(x, scale);
  if (live) {
    *(uint2_v*)(dst8 + drow * HD + dl * 8) = out;
    if (dl == 0) dsts[drow] = scale;
  }
}

// Decode side, one wave for head h of qkv row b ([B, (Hq+2*Hkv)*128] packed
// wqkv output), lane owns the rotation pair (lane, lane + 64). q heads: the
// same fmaf expressions as decode_rope_append, stored to qout. A k head is
// roped with table row `pos`, rounded to bf16, quantised; a v head is
// quantised raw; both go to row `kv_row` of k8 / v8 [rows, Hkv, 128] and
// ks / vs [rows, Hkv]. The amax is a 64-lane reduce over the lane's two
// elements. The two bytes of a lane go out as byte stores (a wave's stores
// cover two runs of 64 consecutive bytes): this is a latency-floor kernel
// and a lane exchange to 4-byte stores only adds dependent instructions.
__device__ __forceinline__ void decode_rope_quant_append(
    const unsigned short* __restrict__ qkv, unsigned short* __restrict__ qout,
    unsigned char* __restrict__ k8, unsigned char* __restrict__ v8,
    float* __restrict__ ks, float* __restrict__ vs,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, int b,
    int h, int Hq, int Hkv, int pos, long kv_row) {
  const int lane = threadIdx.x;
  const int nh = Hq + 2 * Hkv;
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
  const long drow = kv_row * Hkv + (is_k ? h - Hq : h - Hq - Hkv);
  const float amax = wave_reduce_max(fmaxf(fabsf(y1), fabsf(y2)));
  const float scale = kv_row_scale(amax);
  const unsigned int pk = __builtin_amdgcn_cvt_pk_fp8_f32(
      kv_quant(y1, scale), kv_quant(y2, scale), 0u, false);
  unsigned char* dst = (is_k ? k8 : v8) + drow * HD;
  dst[lane] = (unsigned char)(pk & 0xffu);
  dst[lane + 64] = (unsigned char)((pk >> 8) & 0xffu);
  if (lane == 0) (is_k ? ks : vs)[drow] = scale;
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

// ---- row sources -------------------------------------------------------------
// kb / vb point at byte 0 of the kv head in row 0 of the cache (dense: of
// sequence b; paged: of the pool), ksb / vsb at its scale in row 0.
// `row(t)` is the index of logical row t in units of one [Hkv] row.

// Dense cache [B, T, Hkv, 128]: row t of the sequence is t rows down.
struct DenseRows8 {
  const unsigned char* kb;
  const unsigned char* vb;
  const float* ksb;
  const float* vsb;
  int Hkv;
  __device__ __forceinline__ long row(int t) const { return (long)t * Hkv; }
};

// Paged pools [num_pages, P, Hkv, 128] / [num_pages, P, Hkv], P = 1 << logP:
// logical row t is pool[bt_row[t >> logP]][t & (P-1)]. The table entry is
// loaded where the row is used. fp8kv_group asks for the U rows of a group
// back to back, so the U table loads of a lane go out together, one round
// trip in front of the group's 16 pool loads, and the 8 lanes of a row read
// the same entry. A register pipeline that carried the page ids one group
// ahead was measured against this form and did not pay for itself at 4096
// rows (docs/kernels.md).
//
// No table content can address outside the pools: the table index is
// clamped to [0, M-1], every page id to [0, num_pages), the kernel clamps
// the length to [0, M*P] (paged_len), and offsets are 64-bit.
struct PagedRows8 {
  const unsigned char* kb;
  const unsigned char* vb;
  const float* ksb;
  const float* vsb;
  const int* bt_row;  // this sequence's table row [M]
  int Hkv, M, num_pages, logP;
  __device__ __forceinline__ long row(int t) const {
    const int pg = min(max(bt_row[min(max(t >> logP, 0), M - 1)], 0),
                       num_pages - 1);
    return (((long)pg << logP) + (t & ((1 << logP) - 1))) * Hkv;
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
template <int HB, int U, bool MASK, bool KDOT, class Rows>
__device__ __forceinline__ void fp8kv_group(
    Fp8kvState<HB>& st, const QFrag<HB, KDOT>& qf, const Rows& rows, int tb,
    int t_end, int dchunk) {
  uint4_v kq[U], vq[U];
  float ksc[U], vsc[U];
  bool ok[U];
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = tb + 32 * u;
    ok[u] = !MASK || t < t_end;
    const long row = rows.row(ok[u] ? t : t_end - 1);
    kq[u] = *(const uint4_v*)(rows.kb + row * HD + dchunk);
    ksc[u] = rows.ksb[row];
    vq[u] = *(const uint4_v*)(rows.vb + row * HD + dchunk);
    vsc[u] = rows.vsb[row];
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

// The block body. `qp` points at q[b, hq0, 0] (HB consecutive heads), `rows`
// is the row source of sequence b's kv head. SPLIT: store the unnormalised
// (m, l, o) partial of slice `slice` for decode_attn_merge_kernel; otherwise
// normalise and store bf16.
template <int HB, bool SPLIT, bool KDOT, class Rows>
__device__ __forceinline__ void decode_attn_fp8kv_block(
    const unsigned short* __restrict__ qp, Rows rows, int t_begin, int t_end,
    float scale, unsigned short* __restrict__ o, float* __restrict__ ml,
    float* __restrict__ oacc, long bq0, int split, int slice) {
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
    fp8kv_group<HB, U, false, KDOT>(st, qf, rows, tb + mine, t_end, dchunk);
  for (; tb < t_end; tb += 32)
    fp8kv_group<HB, 1, true, KDOT>(st, qf, rows, tb + mine, t_end, dchunk);

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
