// Paged (block-table) counterparts of the decode kernels in
// decode_attn.hip, bf16, GQA, HD = 128.
//
//   kpool / vpool  [num_pages, P, Hkv, 128]   P a power of two, 16..256
//   block_table    int32 [B, M]   logical page j of sequence b lives in
//                                 physical page block_table[b][j]
//   pos            int32 [B]      row b attends pos[b]+1 rows, appends at
//                                 pos[b]
//
// Logical row t of sequence b is pool[bt[b][t / P]][t % P][hkv][:]. The
// kernels run decode_attn_block (decode_core.h) with the paged row source
// in place of the dense one, with the same split count and per-row chunk,
// so the output is bit-identical to decode_attn_kernel /
// decode_attn_split_kernel on the same logical cache. The bounds argument
// is next to PagedRows.
#include "decode_core.h"

__device__ __forceinline__ int paged_len(const int* __restrict__ pos, int b,
                                         int M, int logP) {
  // L = pos + 1 clamped to [0, M*P]; compare before adding so a garbage
  // pos cannot overflow
  const int cap = M << logP;
  const int p = pos[b];
  return p < 0 ? 0 : (p >= cap ? cap : p + 1);
}

__device__ __forceinline__ PagedRows paged_rows(
    const unsigned short* __restrict__ kpool,
    const unsigned short* __restrict__ vpool, const int* __restrict__ bt_row,
    int hkv, int Hkv, int num_pages, int logP) {
  const long head_off = (long)hkv * HD;
  return PagedRows{kpool + head_off, vpool + head_off, bt_row,
                   (long)Hkv * HD, num_pages, logP};
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
  const long bq = (long)b * Hq + hq;
  decode_attn_block(q + bq * HD,
                    paged_rows(kpool, vpool, bt + (long)b * M,
                               hq / (Hq / Hkv), Hkv, num_pages, logP),
                    0, L, scale, StoreOutput{o + bq * HD});
}

// ---- split-K (flash-decode) variant ---------------------------------------
// Pass 1: the cache length is split across gridDim.y blocks exactly as in
// decode_attn_split_kernel (chunk = ceil(L / split) per row), each block
// writing an UNNORMALIZED (m, l, o[128]) partial to f32 scratch. Pass 2 is
// decode_attn_merge_kernel.
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
  const int split = gridDim.y;
  const int chunk = (L + split - 1) / split;
  const int t0 = blockIdx.y * chunk;
  const int t1 = min(L, t0 + chunk);
  const long pbase = (long)bq * split + blockIdx.y;
  decode_attn_block(q + (long)bq * HD,
                    paged_rows(kpool, vpool, bt + (long)b * M,
                               hq / (Hq / Hkv), Hkv, num_pages, logP),
                    t0, t1, scale,
                    StorePartial{ml + pbase * 2, oacc + pbase * HD});
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
  decode_attn_merge_launch(ml, oacc, o, B * Hq, split, stream);
}

// Fused decode rope + paged cache append: decode_rope_cache_kernel with
// the destination row computed through the table,
//   slot = bt[b][pos / P] * P + pos % P.
// Same rotation (decode_rope_append), so the roped q and the stored K/V
// rows are bit-identical to the dense kernel's. One wave per head.
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
  decode_rope_append(qkv, qout, kpool, vpool, cos_t, sin_t, b, h, Hq, Hkv,
                     pos, slot);
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
