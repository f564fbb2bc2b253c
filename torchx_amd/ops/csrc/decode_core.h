// The one body of single-position (decode) attention, bf16, GQA, HD = 128,
// shared by the dense kernels (decode_attn.hip) and the paged ones
// (paged_attn.hip), and the one rope + cache-append rotation.
//
//   o[b,hq,:] = softmax(scale * q[b,hq,:] . K[:L]^T) . V[:L]
//
// One 256-thread block per (b, hq[, split slice]). 16 lanes per cached row
// (16 x 8 d = 128, ushort8 loads), so a wave covers 4 rows per iteration
// and the block 16; each wave keeps its OWN online-softmax state (m, l,
// 8-float o partial per lane) over its rows — flash-decode style — and
// the 16 (wave, row-slot) states merge through LDS once at the end (one
// barrier). A kernel chooses two things at compile time: where row t of
// K/V lives (a row source) and what happens to the combined state (an
// epilogue). Everything else is the same expressions in the same order,
// which is why paged and dense outputs are bit-identical on the same
// logical cache.
#pragma once

#include "common.h"

#define HD 128

// ---- row sources: kb / vb and the element offset of logical row t ---------
// kb / vb point at d = 0 of the kv head in row 0.

// Dense cache [B, T, Hkv, 128]: row t of the sequence is t rows down.
struct DenseRows {
  const unsigned short* kb;
  const unsigned short* vb;
  long row_stride;
  __device__ __forceinline__ long off(int t) { return (long)t * row_stride; }
};

// Paged pools [num_pages, P, Hkv, 128], P = 1 << logP: logical row t is
// pool[bt_row[t / P]][t % P]. The table entry is reloaded only when t / P
// changes (the 16 lanes of a row read the same entry).
//
// No table content can address outside the pools: every physical page id
// read from a table is clamped to [0, num_pages), the callers clamp L to
// [0, M*P] (paged_len) and the append position to [0, M*P) and to the rope
// table, so table indices stay below M, and all pool offsets are 64-bit.
struct PagedRows {
  const unsigned short* kb;
  const unsigned short* vb;
  const int* bt_row;  // this sequence's table row [M]
  long row_stride;
  int num_pages, logP;
  int cur_j = -1;
  long page_base = 0;  // first row of the current physical page
  __device__ __forceinline__ long off(int t) {
    const int j = t >> logP;
    if (j != cur_j) {
      const int pg = min(max(bt_row[j], 0), num_pages - 1);
      page_base = (long)pg << logP;
      cur_j = j;
    }
    return (page_base + (t & ((1 << logP) - 1))) * row_stride;
  }
};

// ---- epilogues: what wave 0 does with the block's (m, l, o[128]) ----------

// normalise and store the bf16 output row; `o` points at o[b, hq, 0]
struct StoreOutput {
  unsigned short* o;
  __device__ __forceinline__ void operator()(float m_t, float l_t,
                                             const float (&out)[8], int lane,
                                             int dchunk) const {
    const float inv = (l_t > 0.f) ? 1.0f / l_t : 0.f;
    if ((lane >> 4) == 0) {  // 16 lanes cover all 128 d
      ushort8 ov;
      #pragma unroll
      for (int j = 0; j < 8; ++j) ov[j] = f32_to_bf16(out[j] * inv);
      *(ushort8*)(o + dchunk) = ov;
    }
  }
};

// store the UNNORMALIZED partial of one split slice to f32 scratch for
// decode_attn_merge_kernel; `ml` / `oacc` point at the slice's entries
struct StorePartial {
  float* ml;    // [2]
  float* oacc;  // [128]
  __device__ __forceinline__ void operator()(float m_t, float l_t,
                                             const float (&out)[8], int lane,
                                             int dchunk) const {
    if (lane == 0) {
      ml[0] = m_t;  // m = -inf, l = 0 for an empty slice
      ml[1] = l_t;
    }
    if ((lane >> 4) == 0) {
      #pragma unroll
      for (int j = 0; j < 8; ++j) oacc[dchunk + j] = out[j];
    }
  }
};

// ---- the block body --------------------------------------------------------
// `qp` points at q[b, hq, 0]; the block covers rows [t_begin, t_end), wave w
// owning t = t_begin + 4*w + tsub + 16*i.
template <class Rows, class Epilogue>
__device__ __forceinline__ void decode_attn_block(
    const unsigned short* __restrict__ qp, Rows rows, int t_begin, int t_end,
    float scale, Epilogue epilogue) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int tsub = lane >> 4;          // wave's row slot 0..3
  const int dchunk = (lane & 15) * 8;  // this lane's 8 d's

  // q fragment for this lane's d-chunk (f32)
  float qv[8];
  {
    ushort8 v = *(const ushort8*)(qp + dchunk);
    #pragma unroll
    for (int j = 0; j < 8; ++j) qv[j] = bf16_to_f32(v[j]) * scale;
  }

  float m_run = -3.0e38f, l_run = 0.f;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  for (int t = t_begin + 4 * wave + tsub; t < t_end; t += 16) {
    const long roff = rows.off(t);
    ushort8 kv8 = *(const ushort8*)(rows.kb + roff + dchunk);
    float s = 0.f;
    #pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf(qv[j], bf16_to_f32(kv8[j]), s);
    // reduce the 16-lane group -> every lane of the group has the score
    #pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
      s += __shfl_xor(s, off, 16);
    }
    // online softmax (wave-local state; all 16 lanes of the group agree)
    const float m_new = fmaxf(m_run, s);
    const float alpha = __builtin_amdgcn_exp2f(
        1.44269504f * (m_run - m_new));
    const float p = __builtin_amdgcn_exp2f(1.44269504f * (s - m_new));
    l_run = l_run * alpha + p;
    ushort8 vv8 = *(const ushort8*)(rows.vb + roff + dchunk);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[j] = fmaf(acc[j], alpha, p * bf16_to_f32(vv8[j]));
    }
    m_run = m_new;
  }

  // combine the 4 row-slots of each wave, then the 4 waves: 16 partial
  // (m, l, o[128]) states -> LDS, block-combined by wave 0
  __shared__ float sm[16], sl[16], so[16][128];
  const int slot = wave * 4 + tsub;
  if ((lane & 15) == 0) {
    sm[slot] = m_run;
    sl[slot] = l_run;
  }
  #pragma unroll
  for (int j = 0; j < 8; ++j) so[slot][dchunk + j] = acc[j];
  __syncthreads();

  if (wave == 0) {
    float m_t = -3.0e38f;
    #pragma unroll
    for (int i = 0; i < 16; ++i) m_t = fmaxf(m_t, sm[i]);
    float l_t = 0.f;
    float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float w = __builtin_amdgcn_exp2f(1.44269504f * (sm[i] - m_t));
      l_t += sl[i] * w;
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        out[j] = fmaf(so[i][dchunk + j], w, out[j]);
      }
    }
    epilogue(m_t, l_t, out, lane, dchunk);
  }
}

// Pass 2 of the split (flash-decode) variants, dense and paged: combines
// the SPLIT partials of every (b, hq). Defined in decode_attn.hip.
extern "C" void decode_attn_merge_launch(const void* ml, const void* oacc,
                                         void* o, int BHq, int split,
                                         hipStream_t stream);

// ---- rope + cache append of ONE position -----------------------------------
// One wave for head h of qkv row b ([B, (Hq+2*Hkv)*128] packed wqkv output):
// q and k heads are rotated (half-split pairing, same convention as
// rope_fwdbwd_kernel) with table row `pos`, q goes to qout [B, Hq, 128],
// the roped k and the raw v go to row `kv_row` of kc / vc [rows, Hkv, 128].
__device__ __forceinline__ void decode_rope_append(
    const unsigned short* __restrict__ qkv, unsigned short* __restrict__ qout,
    unsigned short* __restrict__ kc, unsigned short* __restrict__ vc,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int b, int h, int Hq, int Hkv, int pos, long kv_row) {
  const int lane = threadIdx.x;  // 0..63: one rotation pair (lane, lane+64)
  const unsigned short* src = qkv + ((long)b * (Hq + 2 * Hkv) + h) * HD;
  if (h < Hq + Hkv) {  // q or k head: rotate
    const float x1 = bf16_to_f32(src[lane]);
    const float x2 = bf16_to_f32(src[lane + 64]);
    const float c = cos_t[(long)pos * 64 + lane];
    const float s = sin_t[(long)pos * 64 + lane];
    const unsigned short y1 = f32_to_bf16(fmaf(x1, c, -s * x2));
    const unsigned short y2 = f32_to_bf16(fmaf(x2, c, s * x1));
    unsigned short* dst =
        (h < Hq) ? qout + ((long)b * Hq + h) * HD
                 : kc + (kv_row * Hkv + (h - Hq)) * HD;
    dst[lane] = y1;
    dst[lane + 64] = y2;
  } else {  // v head: plain copy into the cache
    unsigned short* dst = vc + (kv_row * Hkv + (h - Hq - Hkv)) * HD;
    dst[lane] = src[lane];
    dst[lane + 64] = src[lane + 64];
  }
}
