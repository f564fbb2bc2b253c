// Paged (block-table) counterparts of the fp8 KV-cache kernels in
// decode_attn_fp8kv.hip, HD = 128, GQA: the pools PagedBatcher decodes
// over with kv_cache="fp8".
//
//   k8pool / v8pool  [num_pages, P, Hkv, 128] e4m3   P a power of two, 16..256
//   kspool / vspool  [num_pages, P, Hkv] fp32        value = k8 * ks
//   block_table      int32 [B, M]   logical page j of sequence b lives in
//                                   physical page block_table[b][j]
//   pos              int32 [B]      row b attends pos[b]+1 rows, appends at
//                                   pos[b]
//
// Logical row t of sequence b is pool[bt[b][t / P]][t % P][hkv]. The three
// kernels run the bodies of decode_fp8kv_core.h, so for the same split
// count the attention output is bit-identical to decode_attn_fp8kv_kernel on
// the same logical cache, and both quantisers store the bytes and scales of
// the dense ones. A fourth kernel is the packed-token rope + quantising
// append of the ragged prefill pass; the prefill attention over these pools
// is in attention.hip (paged_prefill_attn_fp8kv_kernel).
//
// Attention: decode_attn_fp8kv_block over PagedRows8. Work split, lane map,
// loop structure, arithmetic, combine and merge are the dense kernel's;
// only the K/V/scale addresses differ, each group's four table entries
// loaded in front of its 16 pool loads. No table content can address
// outside the pools: see the bounds argument at PagedRows8; the quantisers
// clamp in the same way.
#include "decode_fp8kv_core.h"

// grid.x = B * Hkv * NG with NG = G / HB head groups per kv head; grid.y =
// split; chunk = ceil(L / split) per row, as in the dense kernel.
template <int G, bool SPLIT>
__global__ void __launch_bounds__(256)
paged_decode_attn_fp8kv_kernel(
    const unsigned short* __restrict__ q,       // [B,Hq,128]
    const unsigned char* __restrict__ k8pool,   // [num_pages,P,Hkv,128]
    const unsigned char* __restrict__ v8pool,
    const float* __restrict__ kspool,           // [num_pages,P,Hkv]
    const float* __restrict__ vspool,
    unsigned short* __restrict__ o,             // [B,Hq,128]
    float* __restrict__ ml,                     // [B*Hq, split, 2]
    float* __restrict__ oacc,                   // [B*Hq, split, 128]
    const int* __restrict__ bt,                 // [B, M]
    const int* __restrict__ pos,                // [B]
    int Hkv, int num_pages, int logP, int M, float scale) {
  constexpr int HB = G < 4 ? G : 4;
  constexpr int NG = G / HB;
  const int grp = blockIdx.x % NG;
  const int hkv = (blockIdx.x / NG) % Hkv;
  const int b = blockIdx.x / (NG * Hkv);
  const int Hq = Hkv * G;
  const int L = paged_len(pos, b, M, logP);
  const int split = SPLIT ? (int)gridDim.y : 1;
  const int chunk = (L + split - 1) / split;
  const int t0 = SPLIT ? (int)blockIdx.y * chunk : 0;
  const int t1 = min(L, t0 + chunk);
  const long bq0 = (long)b * Hq + (long)hkv * G + grp * HB;
  PagedRows8 rows;
  rows.kb = k8pool + (long)hkv * HD;
  rows.vb = v8pool + (long)hkv * HD;
  rows.ksb = kspool + hkv;
  rows.vsb = vspool + hkv;
  rows.bt_row = bt + (long)b * M;
  rows.Hkv = Hkv;
  rows.M = M;
  rows.num_pages = num_pages;
  rows.logP = logP;
  decode_attn_fp8kv_block<HB, SPLIT, true>(q + bq0 * HD, rows, t0, t1, scale,
                                           o, ml, oacc, bq0, split,
                                           (int)blockIdx.y);
}

template <int G, bool SPLIT>
static void paged_fp8kv_launch_one(const void* q, const void* k8pool,
                                   const void* v8pool, const void* kspool,
                                   const void* vspool, void* o, void* ml,
                                   void* oacc, const void* bt,
                                   const void* pos, int B, int Hkv,
                                   int num_pages, int logP, int M, int split,
                                   float scale, hipStream_t stream) {
  constexpr int NG = G / (G < 4 ? G : 4);
  hipLaunchKernelGGL((paged_decode_attn_fp8kv_kernel<G, SPLIT>),
                     dim3(B * Hkv * NG, split), dim3(256), 0, stream,
                     (const unsigned short*)q, (const unsigned char*)k8pool,
                     (const unsigned char*)v8pool, (const float*)kspool,
                     (const float*)vspool, (unsigned short*)o, (float*)ml,
                     (float*)oacc, (const int*)bt, (const int*)pos, Hkv,
                     num_pages, logP, M, scale);
}

// G = Hq / Hkv must be 1, 2, 4 or 8 (checked by the binding). split == 1 is
// the single-pass kernel (ml / oacc unused); split > 1 writes partials and
// runs decode_attn_merge_launch.
extern "C" void paged_decode_attn_fp8kv_launch(
    const void* q, const void* k8pool, const void* v8pool, const void* kspool,
    const void* vspool, void* o, void* ml, void* oacc, const void* bt,
    const void* pos, int B, int Hq, int Hkv, int num_pages, int logP, int M,
    int split, float scale, hipStream_t stream) {
  const bool sp = split > 1;
  decltype(&paged_fp8kv_launch_one<1, false>) fn;
  switch (Hq / Hkv) {
    case 1:
      fn = sp ? paged_fp8kv_launch_one<1, true>
              : paged_fp8kv_launch_one<1, false>;
      break;
    case 2:
      fn = sp ? paged_fp8kv_launch_one<2, true>
              : paged_fp8kv_launch_one<2, false>;
      break;
    case 4:
      fn = sp ? paged_fp8kv_launch_one<4, true>
              : paged_fp8kv_launch_one<4, false>;
      break;
    default:
      fn = sp ? paged_fp8kv_launch_one<8, true>
              : paged_fp8kv_launch_one<8, false>;
      break;
  }
  fn(q, k8pool, v8pool, kspool, vspool, o, ml, oacc, bt, pos, B, Hkv,
     num_pages, logP, M, split, scale, stream);
  if (sp) decode_attn_merge_launch(ml, oacc, o, B * Hq, split, stream);
}

// Pool row of logical row t of the sequence whose table row is bt_row: the
// table index clamped to [0, M-1], the page id to [0, num_pages).
__device__ __forceinline__ long paged_slot(const int* __restrict__ bt_row,
                                           int t, int M, int num_pages,
                                           int logP) {
  const int j = min(max(t >> logP, 0), M - 1);
  const int pg = min(max(bt_row[j], 0), num_pages - 1);
  return ((long)pg << logP) + (t & ((1 << logP) - 1));
}

// ---- decode side: rope + quantising append through the table ---------------
// decode_rope_cache_fp8kv_kernel with the destination row
//   slot = bt[b][pos >> logP] * P + (pos & (P-1)),
// pos int32 [B], clamped to [0, M*P) and to the rope table. One wave per
// head of the packed qkv row.
__global__ void __launch_bounds__(64)
paged_decode_rope_cache_fp8kv_kernel(
    const unsigned short* __restrict__ qkv, unsigned short* __restrict__ qout,
    unsigned char* __restrict__ k8pool, unsigned char* __restrict__ v8pool,
    float* __restrict__ kspool, float* __restrict__ vspool,
    const int* __restrict__ bt,        // [B, M]
    const float* __restrict__ cos_t,   // [R, 64]
    const float* __restrict__ sin_t,
    const int* __restrict__ pos_dev,   // [B]
    int B, int Hq, int Hkv, int num_pages, int logP, int M, int rope_rows) {
  const int nh = Hq + 2 * Hkv;
  const int b = blockIdx.x / nh;
  const int h = blockIdx.x % nh;
  const int cap = min(M << logP, rope_rows);
  const int pos = min(max(pos_dev[b], 0), cap - 1);
  const long slot = paged_slot(bt + (long)b * M, pos, M, num_pages, logP);
  decode_rope_quant_append(qkv, qout, k8pool, v8pool, kspool, vspool, cos_t,
                           sin_t, b, h, Hq, Hkv, pos, slot);
}

extern "C" void paged_decode_rope_cache_fp8kv_launch(
    const void* qkv, void* qout, void* k8pool, void* v8pool, void* kspool,
    void* vspool, const void* bt, const void* cos_t, const void* sin_t,
    const void* pos_dev, int B, int Hq, int Hkv, int num_pages, int logP,
    int M, int rope_rows, hipStream_t stream) {
  hipLaunchKernelGGL(paged_decode_rope_cache_fp8kv_kernel,
                     dim3(B * (Hq + 2 * Hkv)), dim3(64), 0, stream,
                     (const unsigned short*)qkv, (unsigned short*)qout,
                     (unsigned char*)k8pool, (unsigned char*)v8pool,
                     (float*)kspool, (float*)vspool, (const int*)bt,
                     (const float*)cos_t, (const float*)sin_t,
                     (const int*)pos_dev, B, Hq, Hkv, num_pages, logP, M,
                     rope_rows);
}

// ---- ragged prefill side: rope + quantising append for packed tokens -------
// paged_prefill_rope_cache_kernel (paged_attn.hip) for fp8 pools: qkv
// [T, (Hq+2*Hkv)*128], token t at logical position pos[t], its K/V row at
// physical pool row slot[t]. Same lane map (8 lanes per (token, head), lane
// i8 owns the rotation pairs (8*i8 + j, 64 + 8*i8 + j)) and the same
// rotation expression, so q is that kernel's q bit for bit. A k head is
// roped and rounded to bf16, a v head taken raw; the row's amax is an
// 8-lane butterfly over the lane's 16 elements, and the 16 bytes go out as
// two 8-byte stores, lane 0 of the 8 adding the scale: quantize_kv_rows of
// the row the bf16 kernel would store. pos is clamped to the rope table,
// slot to [0, num_pages * P), offsets are 64-bit.
__global__ void __launch_bounds__(256)
paged_prefill_rope_cache_fp8kv_kernel(
    const unsigned short* __restrict__ qkv,
    unsigned short* __restrict__ qout,  // [T,Hq,128]
    unsigned char* __restrict__ k8pool, unsigned char* __restrict__ v8pool,
    float* __restrict__ kspool, float* __restrict__ vspool,
    const float* __restrict__ cos_t,   // [R, 64]
    const float* __restrict__ sin_t,
    const int* __restrict__ pos_dev,   // [T]
    const int* __restrict__ slot_dev,  // [T]
    long T, int Hq, int Hkv, long pool_rows, int rope_rows) {
  const int nh = Hq + 2 * Hkv;
  const long n = T * nh * 8;  // whole 8-lane groups enter and leave together
  for (long i = grid_stride_begin(); i < n; i += grid_stride()) {
    const int i8 = (int)(i & 7);
    const long th = i >> 3;
    const long t = th / nh;
    const int h = (int)(th - t * nh);
    const unsigned short* src = qkv + th * HD + i8 * 8;
    ushort8 u1 = *(const ushort8*)src;
    ushort8 u2 = *(const ushort8*)(src + 64);
    if (h < Hq + Hkv) {  // q or k head: rotate, round to bf16
      const int pos = min(max(pos_dev[t], 0), rope_rows - 1);
      const float* cp = cos_t + (long)pos * 64 + i8 * 8;
      const float* sp = sin_t + (long)pos * 64 + i8 * 8;
      const f32x4 c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4);
      const f32x4 s0 = *(const f32x4*)sp, s1 = *(const f32x4*)(sp + 4);
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
    if (h < Hq) {
      unsigned short* dst = qout + (t * Hq + h) * HD + i8 * 8;
      *(ushort8*)dst = u1;
      *(ushort8*)(dst + 64) = u2;
      continue;
    }
    float x1[8], x2[8];
    float amax = 0.f;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      x1[j] = bf16_to_f32(u1[j]);
      x2[j] = bf16_to_f32(u2[j]);
      amax = fmaxf(amax, fmaxf(fabsf(x1[j]), fabsf(x2[j])));
    }
    #pragma unroll
    for (int off = 4; off >= 1; off >>= 1)
      amax = fmaxf(amax, __shfl_xor(amax, off, 8));
    const float scale = kv_row_scale(amax);
    const bool is_k = h < Hq + Hkv;
    const long slot = min(max((long)slot_dev[t], 0L), pool_rows - 1);
    const long drow = slot * Hkv + (is_k ? h - Hq : h - Hq - Hkv);
    unsigned char* dst = (is_k ? k8pool : v8pool) + drow * HD + i8 * 8;
    *(uint2_v*)dst = kv_quant_pack8(x1, scale);
    *(uint2_v*)(dst + 64) = kv_quant_pack8(x2, scale);
    if (i8 == 0) (is_k ? kspool : vspool)[drow] = scale;
  }
}

extern "C" void paged_prefill_rope_cache_fp8kv_launch(
    const void* qkv, void* qout, void* k8pool, void* v8pool, void* kspool,
    void* vspool, const void* cos_t, const void* sin_t, const void* pos_dev,
    const void* slot_dev, long T, int Hq, int Hkv, long pool_rows,
    int rope_rows, hipStream_t stream) {
  const long n = T * (Hq + 2 * Hkv) * 8;
  long grid = (n + 255) / 256;
  if (grid > 65535 * 8) grid = 65535 * 8;
  hipLaunchKernelGGL(paged_prefill_rope_cache_fp8kv_kernel,
                     dim3((unsigned)grid), dim3(256), 0, stream,
                     (const unsigned short*)qkv, (unsigned short*)qout,
                     (unsigned char*)k8pool, (unsigned char*)v8pool,
                     (float*)kspool, (float*)vspool, (const float*)cos_t,
                     (const float*)sin_t, (const int*)pos_dev,
                     (const int*)slot_dev, T, Hq, Hkv, pool_rows, rope_rows);
}

// ---- prefill side: quantise S rows of K and V into the pages ---------------
// kv_quantize_store_kernel with the destination row found through the
// table per item: logical rows start .. start+S-1 of sequence b go to the
// pages of table row b. 16 lanes per (row, kv head) item, 16 items per
// block, blockIdx.y picks K or V: one launch in place of the arange, the
// table gather and the two index_copy_ of a bf16 pool's store_prefix. The
// 16 lanes of an item read the same table entry. The binding checks
// start + S <= M * P; the table index and the page id are clamped anyway.
__global__ void __launch_bounds__(256)
paged_kv_quantize_store_kernel(
    const unsigned short* __restrict__ k,  // [B,S,Hkv,128]
    const unsigned short* __restrict__ v, unsigned char* __restrict__ k8pool,
    unsigned char* __restrict__ v8pool, float* __restrict__ kspool,
    float* __restrict__ vspool,
    const int* __restrict__ bt,  // [B, M]
    long n_items, int S, int Hkv, int num_pages, int logP, int M, int start) {
  const unsigned short* __restrict__ src = blockIdx.y ? v : k;
  unsigned char* __restrict__ dst8 = blockIdx.y ? v8pool : k8pool;
  float* __restrict__ dsts = blockIdx.y ? vspool : kspool;
  const int dl = threadIdx.x & 15;
  const long item = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = item < n_items;
  const long it = live ? item : n_items - 1;  // whole 16-lane groups agree
  const long h = it % Hkv;
  const long bs = it / Hkv;
  const int s = (int)(bs % S);
  const long b = bs / S;
  const long drow =
      paged_slot(bt + b * M, start + s, M, num_pages, logP) * Hkv + h;
  kv_quantize_item(src, it, dst8, dsts, drow, dl, live);
}

extern "C" void paged_kv_quantize_store_launch(
    const void* k, const void* v, void* k8pool, void* v8pool, void* kspool,
    void* vspool, const void* bt, int B, int S, int Hkv, int num_pages,
    int logP, int M, int start, hipStream_t stream) {
  const long n_items = (long)B * S * Hkv;
  hipLaunchKernelGGL(paged_kv_quantize_store_kernel,
                     dim3((unsigned)((n_items + 15) / 16), 2), dim3(256), 0,
                     stream, (const unsigned short*)k,
                     (const unsigned short*)v, (unsigned char*)k8pool,
                     (unsigned char*)v8pool, (float*)kspool, (float*)vspool,
                     (const int*)bt, n_items, S, Hkv, num_pages, logP, M,
                     start);
}
