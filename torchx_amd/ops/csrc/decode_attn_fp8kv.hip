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
#include "decode_fp8kv_core.h"

// ---- prefill side: quantise and store S rows of K and V ---------------------
// 16 lanes per (row, kv head) run kv_quantize_item. A block holds 16 items;
// blockIdx.y picks K or V.
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

  kv_quantize_item(src, it, dst8, dsts, drow, dl, live);
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
// [B]); one wave per head of the packed qkv row runs
// decode_rope_quant_append into cache row b * T + pos. `pos` is clamped to
// [0, T) and to the rope table.
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
  int pos = pos_dev ? pos_dev[per_row ? b : 0] : pos_host;
  pos = min(max(pos, 0), min(T, rope_rows) - 1);
  decode_rope_quant_append(qkv, qout, k8, v8, ks, vs, cos_t, sin_t, b, h, Hq,
                           Hkv, pos, (long)b * T + pos);
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
// The block body, the row sources and the quantise helpers are in
// decode_fp8kv_core.h, shared with paged_attn_fp8kv.hip.

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
      q + bq0 * HD,
      DenseRows8{k8 + row0 * HD, v8 + row0 * HD, ks + row0, vs + row0, Hkv},
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
