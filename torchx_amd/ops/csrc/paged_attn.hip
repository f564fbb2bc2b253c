// Paged (block-table) counterparts of the decode kernels in
// decode_attn.hip, bf16, GQA, HD = 128.
//
//   kpool / vpool  [num_pages, P, Hkv, 128]   P a power of two, 16..256
//   block_table    int32 [B, M]   logical page j of sequence b lives in
//                                 physical page block_table[b][j]
//   pos            int32 [B]      row b attends pos[b]+1 rows, appends at
//                                 pos[b]
//
// Logical row t of sequence b is pool[bt[b][t / P]][t % P][hkv][:]. Only
// the addressing differs from the dense kernels: the row-to-lane
// assignment (16 lanes per row, wave w owns t = t0 + 4w + tsub + 16i),
// the split count, the per-row chunk and the online-softmax / merge
// arithmetic are the same expressions in the same order, so the output
// is bit-identical to decode_attn_kernel / decode_attn_split_kernel on
// the same logical cache.
//
// No table content can produce an out-of-bounds access: every physical
// page id is clamped to [0, num_pages), L to [0, M*P], the append
// position to [0, M*P) (and to the rope table), and all pool offsets are
// 64-bit.
#include "common.h"

#define HD 128

// Per-wave partial state over this lane's rows t = t_begin + 16*i < t_end.
// The loop body is decode_attn_kernel's, with the row pointer looked up
// through the table; the table entry is reloaded only when t / P changes
// (the 16 lanes of a row read the same entry).
__device__ __forceinline__ void paged_rows(
    const unsigned short* __restrict__ kpool,
    const unsigned short* __restrict__ vpool,
    const int* __restrict__ bt_row,  // this sequence's table row [M]
    int num_pages, int logP, long row_stride, long head_off,
    int t_begin, int t_end, const float (&qv)[8], float& m_run, float& l_run,
    float (&acc)[8]) {
  const int pmask = (1 << logP) - 1;
  int cur_j = -1;
  long page_base = 0;  // first row of the current physical page
  for (int t = t_begin; t < t_end; t += 16) {
    const int j = t >> logP;
    if (j != cur_j) {
      const int pg = min(max(bt_row[j], 0), num_pages - 1);
      page_base = (long)pg << logP;
      cur_j = j;
    }
    const long roff = (page_base + (t & pmask)) * row_stride + head_off;
    const unsigned short* kr = kpool + roff;
    ushort8 kv8 = *(const ushort8*)kr;
    float s = 0.f;
    #pragma unroll
    for (int j2 = 0; j2 < 8; ++j2) s = fmaf(qv[j2], bf16_to_f32(kv8[j2]), s);
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
    const unsigned short* vr = vpool + roff;
    ushort8 vv8 = *(const ushort8*)vr;
    #pragma unroll
    for (int j2 = 0; j2 < 8; ++j2) {
      acc[j2] = fmaf(acc[j2], alpha, p * bf16_to_f32(vv8[j2]));
    }
    m_run = m_new;
  }
}

__device__ __forceinline__ int paged_len(const int* __restrict__ pos, int b,
                                         int M, int logP) {
  // L = pos + 1 clamped to [0, M*P]; compare before adding so a garbage
  // pos cannot overflow
  const int cap = M << logP;
  const int p = pos[b];
  return p < 0 ? 0 : (p >= cap ? cap : p + 1);
}

__global__ void __launch_bounds__(256)
paged_decode_attn_kernel(const unsigned short* __restrict__ q,  // [B,Hq,128]
                         const unsigned short* __restrict__ kpool,
                         const unsigned short* __restrict__ vpool,
                         unsigned short* __restrict__ o,        // [B,Hq,128]
                         const int* __restrict__ bt,            // [B, M]
                         const int* __restrict__ pos,           // [B]
                         int B, int Hq, int Hkv, int num_pages, int logP,
                         int M, float scale) {
  const int b = blockIdx.x / Hq;
  const int hq = blockIdx.x % Hq;
  const int L = paged_len(pos, b, M, logP);
  const int hkv = hq / (Hq / Hkv);

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int tsub = lane >> 4;        // wave's row slot 0..3
  const int dchunk = (lane & 15) * 8;  // this lane's 8 d's

  const unsigned short* qp = q + ((long)b * Hq + hq) * HD + dchunk;
  float qv[8];
  {
    ushort8 v = *(const ushort8*)qp;
    #pragma unroll
    for (int j = 0; j < 8; ++j) qv[j] = bf16_to_f32(v[j]) * scale;
  }

  const long row_stride = (long)Hkv * HD;
  float m_run = -3.0e38f, l_run = 0.f;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  paged_rows(kpool, vpool, bt + (long)b * M, num_pages, logP, row_stride,
             (long)hkv * HD + dchunk, 4 * wave + tsub, L, qv, m_run, l_run,
             acc);

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
    const float inv = (l_t > 0.f) ? 1.0f / l_t : 0.f;
    if (tsub == 0) {  // 16 lanes cover all 128 d
      unsigned short* op = o + ((long)b * Hq + hq) * HD + dchunk;
      ushort8 ov;
      #pragma unroll
      for (int j = 0; j < 8; ++j) ov[j] = f32_to_bf16(out[j] * inv);
      *(ushort8*)op = ov;
    }
  }
}

// ---- split-K (flash-decode) variant ---------------------------------------
// Pass 1: the cache length is split across gridDim.y blocks exactly as in
// decode_attn_split_kernel (chunk = ceil(L / split) per row), each block
// writing an UNNORMALIZED (m, l, o[128]) partial to f32 scratch.
__global__ void __launch_bounds__(256)
paged_decode_attn_split_kernel(const unsigned short* __restrict__ q,
                               const unsigned short* __restrict__ kpool,
                               const unsigned short* __restrict__ vpool,
                               float* __restrict__ ml,    // [B*Hq, SPLIT, 2]
                               float* __restrict__ oacc,  // [B*Hq, SPLIT, 128]
                               const int* __restrict__ bt,
                               const int* __restrict__ pos,
                               int B, int Hq, int Hkv, int num_pages,
                               int logP, int M, float scale) {
  const int bq = blockIdx.x;
  const int b = bq / Hq;
  const int hq = bq % Hq;
  const int L = paged_len(pos, b, M, logP);
  const int hkv = hq / (Hq / Hkv);
  const int split = gridDim.y;
  const int chunk = (L + split - 1) / split;
  const int t0 = blockIdx.y * chunk;
  const int t1 = min(L, t0 + chunk);

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int tsub = lane >> 4;
  const int dchunk = (lane & 15) * 8;

  const unsigned short* qp = q + ((long)b * Hq + hq) * HD + dchunk;
  float qv[8];
  {
    ushort8 v = *(const ushort8*)qp;
    #pragma unroll
    for (int j = 0; j < 8; ++j) qv[j] = bf16_to_f32(v[j]) * scale;
  }

  const long row_stride = (long)Hkv * HD;
  float m_run = -3.0e38f, l_run = 0.f;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  paged_rows(kpool, vpool, bt + (long)b * M, num_pages, logP, row_stride,
             (long)hkv * HD + dchunk, t0 + 4 * wave + tsub, t1, qv, m_run,
             l_run, acc);

  // block-combine the 16 (wave, row-slot) partials, wave 0 writes scratch
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
      for (int j = 0; j < 8; ++j)
        out[j] = fmaf(so[i][dchunk + j], w, out[j]);
    }
    const long pbase = ((long)bq * split + blockIdx.y);
    if (lane == 0) {
      ml[pbase * 2] = m_t;       // m = -inf, l = 0 for an empty slice
      ml[pbase * 2 + 1] = l_t;
    }
    if (tsub == 0) {
      #pragma unroll
      for (int j = 0; j < 8; ++j) oacc[pbase * HD + dchunk + j] = out[j];
    }
  }
}

// pass 2: a copy of decode_attn_merge_kernel (that one is only reachable
// through the dense split launcher): one 128-thread block per (b, hq);
// thread d combines SPLIT partials and writes the normalized bf16 element.
__global__ void __launch_bounds__(128)
paged_decode_attn_merge_kernel(const float* __restrict__ ml,
                               const float* __restrict__ oacc,
                               unsigned short* __restrict__ o,  // [B,Hq,128]
                               int split) {
  const int bq = blockIdx.x;
  const int d = threadIdx.x;
  float m_t = -3.0e38f;
  for (int s = 0; s < split; ++s)
    m_t = fmaxf(m_t, ml[((long)bq * split + s) * 2]);
  float l_t = 0.f, out = 0.f;
  for (int s = 0; s < split; ++s) {
    const long p = (long)bq * split + s;
    const float w = __builtin_amdgcn_exp2f(1.44269504f * (ml[p * 2] - m_t));
    l_t += ml[p * 2 + 1] * w;
    out = fmaf(oacc[p * HD + d], w, out);
  }
  const float inv = (l_t > 0.f) ? 1.0f / l_t : 0.f;
  o[(long)bq * HD + d] = f32_to_bf16(out * inv);
}

// split == 1 -> single pass (ml / oacc unused); else split + merge.
extern "C" void paged_decode_attn_launch(
    const void* q, const void* kpool, const void* vpool, void* ml,
    void* oacc, void* o, const void* bt, const void* pos, int B, int Hq,
    int Hkv, int num_pages, int logP, int M, int split, float scale,
    hipStream_t stream) {
  if (split <= 1) {
    hipLaunchKernelGGL(paged_decode_attn_kernel, dim3(B * Hq), dim3(256), 0,
                       stream, (const unsigned short*)q,
                       (const unsigned short*)kpool,
                       (const unsigned short*)vpool, (unsigned short*)o,
                       (const int*)bt, (const int*)pos, B, Hq, Hkv,
                       num_pages, logP, M, scale);
    return;
  }
  hipLaunchKernelGGL(paged_decode_attn_split_kernel, dim3(B * Hq, split),
                     dim3(256), 0, stream, (const unsigned short*)q,
                     (const unsigned short*)kpool,
                     (const unsigned short*)vpool, (float*)ml, (float*)oacc,
                     (const int*)bt, (const int*)pos, B, Hq, Hkv, num_pages,
                     logP, M, scale);
  hipLaunchKernelGGL(paged_decode_attn_merge_kernel, dim3(B * Hq), dim3(128),
                     0, stream, (const float*)ml, (const float*)oacc,
                     (unsigned short*)o, split);
}

// Fused decode rope + paged cache append: decode_rope_cache_kernel with
// the destination row computed through the table,
//   slot = bt[b][pos / P] * P + pos % P.
// Same rotation arithmetic, so the roped q and the stored K/V rows are
// bit-identical to the dense kernel's. One wave per head.
__global__ void __launch_bounds__(64)
paged_decode_rope_cache_kernel(const unsigned short* __restrict__ qkv,
                               unsigned short* __restrict__ qout,  // [B,Hq,128]
                               unsigned short* __restrict__ kpool,
                               unsigned short* __restrict__ vpool,
                               const int* __restrict__ bt,      // [B, M]
                               const float* __restrict__ cos_t,  // [S, 64]
                               const float* __restrict__ sin_t,
                               const int* __restrict__ pos_dev,  // [B]
                               int B, int Hq, int Hkv, int num_pages,
                               int logP, int M, int rope_rows) {
  const int nh = Hq + 2 * Hkv;
  const int b = blockIdx.x / nh;
  const int h = blockIdx.x % nh;
  // append position clamped to [0, M*P) and to the rope table
  const int cap = min(M << logP, rope_rows);
  const int pos = min(max(pos_dev[b], 0), cap - 1);
  const int pg = min(max(bt[(long)b * M + (pos >> logP)], 0), num_pages - 1);
  const long slot = ((long)pg << logP) + (pos & ((1 << logP) - 1));
  const int lane = threadIdx.x;  // 0..63: one rotation pair (lane, lane+64)
  const unsigned short* src = qkv + ((long)b * nh + h) * HD;
  if (h < Hq + Hkv) {  // q or k head: rotate
    const float x1 = bf16_to_f32(src[lane]);
    const float x2 = bf16_to_f32(src[lane + 64]);
    const float c = cos_t[(long)pos * 64 + lane];
    const float s = sin_t[(long)pos * 64 + lane];
    const unsigned short y1 = f32_to_bf16(fmaf(x1, c, -s * x2));
    const unsigned short y2 = f32_to_bf16(fmaf(x2, c, s * x1));
    unsigned short* dst =
        (h < Hq) ? qout + ((long)b * Hq + h) * HD
                 : kpool + (slot * Hkv + (h - Hq)) * HD;
    dst[lane] = y1;
    dst[lane + 64] = y2;
  } else {  // v head: plain copy into the pool
    unsigned short* dst = vpool + (slot * Hkv + (h - Hq - Hkv)) * HD;
    dst[lane] = src[lane];
    dst[lane + 64] = src[lane + 64];
  }
}

extern "C" void paged_decode_rope_cache_launch(
    const void* qkv, void* qout, void* kpool, void* vpool, const void* bt,
    const void* cos_t, const void* sin_t, const void* pos_dev, int B, int Hq,
    int Hkv, int num_pages, int logP, int M, int rope_rows,
    hipStream_t stream) {
  hipLaunchKernelGGL(paged_decode_rope_cache_kernel,
                     dim3(B * (Hq + 2 * Hkv)), dim3(64), 0, stream,
                     (const unsigned short*)qkv, (unsigned short*)qout,
                     (unsigned short*)kpool, (unsigned short*)vpool,
                     (const int*)bt, (const float*)cos_t,
                     (const float*)sin_t, (const int*)pos_dev, B, Hq, Hkv,
                     num_pages, logP, M, rope_rows);
}

// Fused rope + page append for a packed prefill: qkv [T, (Hq+2*Hkv)*128]
// is the wqkv output of T tokens of any mix of sequences; token t sits at
// logical position pos[t] and its K/V row goes to physical pool row
// slot[t] (= page * P + pos % P, worked out once per forward pass from the
// block table). Writes the roped q [T, Hq, 128], the roped k and the raw v.
// One dispatch for the split, the three contiguous copies, the two ropes
// and the two index_copy_ of the unfused path; the rotation is
// rope_fwdbwd_kernel's expression, so q and the stored rows are
// bit-identical to it.
//
// 8 lanes per (token, head): lane i8 owns the rotation pairs
// (8*i8 + j, 64 + 8*i8 + j), j = 0..7 — two 16-byte loads, two 16-byte
// stores, and 2 x 2 float4 of the tables. pos is clamped to the rope
// table, slot to [0, num_pages * P), offsets are 64-bit.
__global__ void __launch_bounds__(256)
paged_prefill_rope_cache_kernel(const unsigned short* __restrict__ qkv,
                                unsigned short* __restrict__ qout,  // [T,Hq,128]
                                unsigned short* __restrict__ kpool,
                                unsigned short* __restrict__ vpool,
                                const float* __restrict__ cos_t,  // [S, 64]
                                const float* __restrict__ sin_t,
                                const int* __restrict__ pos_dev,   // [T]
                                const int* __restrict__ slot_dev,  // [T]
                                long T, int Hq, int Hkv, long pool_rows,
                                int rope_rows) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int nh = Hq + 2 * Hkv;
  const long n = T * nh * 8;
  for (long i = grid_stride_begin(); i < n; i += grid_stride()) {
    const int i8 = (int)(i & 7);
    const long th = i >> 3;
    const long t = th / nh;
    const int h = (int)(th - t * nh);
    const unsigned short* src = qkv + th * HD + i8 * 8;
    ushort8 u1 = *(const ushort8*)src;
    ushort8 u2 = *(const ushort8*)(src + 64);
    unsigned short* dst;
    if (h < Hq) {
      dst = qout + (t * Hq + h) * HD;
    } else {
      const long slot = min(max((long)slot_dev[t], 0L), pool_rows - 1);
      dst = (h < Hq + Hkv) ? kpool + (slot * Hkv + (h - Hq)) * HD
                           : vpool + (slot * Hkv + (h - Hq - Hkv)) * HD;
    }
    dst += i8 * 8;
    if (h < Hq + Hkv) {  // q or k head: rotate
      const int pos = min(max(pos_dev[t], 0), rope_rows - 1);
      const float* cp = cos_t + (long)pos * 64 + i8 * 8;
      const float* sp = sin_t + (long)pos * 64 + i8 * 8;
      const f4 c0 = *(const f4*)cp, c1 = *(const f4*)(cp + 4);
      const f4 s0 = *(const f4*)sp, s1 = *(const f4*)(sp + 4);
      ushort8 o1, o2;
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = j < 4 ? c0[j & 3] : c1[j & 3];
        const float s = j < 4 ? s0[j & 3] : s1[j & 3];
        const float x1 = bf16_to_f32(u1[j]);
        const float x2 = bf16_to_f32(u2[j]);
        o1[j] = f32_to_bf16(fmaf(x1, c, -s * x2));
        o2[j] = f32_to_bf16(fmaf(x2, c, s * x1));
      }
      u1 = o1;
      u2 = o2;
    }
    *(ushort8*)dst = u1;
    *(ushort8*)(dst + 64) = u2;
  }
}

extern "C" void paged_prefill_rope_cache_launch(
    const void* qkv, void* qout, void* kpool, void* vpool, const void* cos_t,
    const void* sin_t, const void* pos_dev, const void* slot_dev, long T,
    int Hq, int Hkv, long pool_rows, int rope_rows, hipStream_t stream) {
  const long n = T * (Hq + 2 * Hkv) * 8;
  long grid = (n + 255) / 256;
  if (grid > 65535 * 8) grid = 65535 * 8;
  hipLaunchKernelGGL(paged_prefill_rope_cache_kernel, dim3((unsigned)grid),
                     dim3(256), 0, stream, (const unsigned short*)qkv,
                     (unsigned short*)qout, (unsigned short*)kpool,
                     (unsigned short*)vpool, (const float*)cos_t,
                     (const float*)sin_t, (const int*)pos_dev,
                     (const int*)slot_dev, T, Hq, Hkv, pool_rows, rope_rows);
}
