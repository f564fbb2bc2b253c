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
// the dense ones.
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
