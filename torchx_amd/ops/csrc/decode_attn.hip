// Single-position (decode) attention over a dense KV cache, bf16, GQA,
// HD = 128 — the serving-side counterpart of the training flash kernels.
//
//   o[b,hq,:] = softmax(scale * q[b,hq,:] . K[b,:L,hkv,:]^T) . V[b,:L,hkv,:]
//
// The block body (row loop, online softmax, LDS combine) is
// decode_attn_block in decode_core.h; the kernels here give it the dense
// row source and an epilogue. HBM-bound by the K/V cache stream
// (L x 512 B per (b, hkv), shared by the GQA group via L2).
#include "decode_core.h"

// L from the host, or len + 1 from a device int32: a scalar, or [B] with
// per_row (ragged / continuous batching)
__device__ __forceinline__ int dense_len(const int* __restrict__ len_dev,
                                         int per_row, int b, int L_host) {
  return len_dev ? (len_dev[per_row ? b : 0] + 1) : L_host;
}

__device__ __forceinline__ DenseRows dense_rows(
    const unsigned short* __restrict__ kc,  // [B, T, Hkv, 128]
    const unsigned short* __restrict__ vc, int b, int hkv, int Hkv, int T) {
  const long row_stride = (long)Hkv * HD;
  const long base = (long)b * T * row_stride + (long)hkv * HD;
  return DenseRows{kc + base, vc + base, row_stride};
}

__global__ void __launch_bounds__(256)
decode_attn_kernel(const unsigned short* __restrict__ q,   // [B, Hq, 128]
                   const unsigned short* __restrict__ kc,  // [B, T, Hkv, 128]
                   const unsigned short* __restrict__ vc,  // [B, T, Hkv, 128]
                   unsigned short* __restrict__ o,         // [B, Hq, 128]
                   const int* __restrict__ len_dev,  // optional: L = len+1
                   int B, int Hq, int Hkv, int T, int L_host, int per_row,
                   float scale) {
  const int b = blockIdx.x / Hq;
  const int hq = blockIdx.x % Hq;
  const int L = dense_len(len_dev, per_row, b, L_host);
  const long bq = (long)b * Hq + hq;
  decode_attn_block(q + bq * HD, dense_rows(kc, vc, b, hq / (Hq / Hkv), Hkv, T),
                    0, L, scale, StoreOutput{o + bq * HD});
}

extern "C" void decode_attn_launch(const void* q, const void* kc,
                                   const void* vc, void* o,
                                   const void* len_dev, int B, int Hq,
                                   int Hkv, int T, int L, int per_row,
                                   float scale, hipStream_t stream) {
  hipLaunchKernelGGL(decode_attn_kernel, dim3(B * Hq), dim3(256), 0, stream,
                     (const unsigned short*)q, (const unsigned short*)kc,
                     (const unsigned short*)vc, (unsigned short*)o,
                     (const int*)len_dev, B, Hq, Hkv, T, L, per_row, scale);
}

// Fused decode-side rope + cache append: consumes the packed wqkv output
// [B, (Hq+2*Hkv)*128] for ONE position, ropes q and k, writes the roped k
// and the raw v into the caches at row `pos`, and emits q contiguous
// [B, Hq, 128] for decode_attn (decode_rope_append in decode_core.h).
// Replaces ~6 tiny kernels (2x rope, 2x index_copy, split copies) per layer
// per token; one wave per head, latency-floor bound.
// `pos` comes from the host (eager) or a device int32 scalar (hipGraph).
__global__ void __launch_bounds__(64)
decode_rope_cache_kernel(const unsigned short* __restrict__ qkv,
                         unsigned short* __restrict__ qout,  // [B, Hq, 128]
                         unsigned short* __restrict__ kc,    // [B,T,Hkv,128]
                         unsigned short* __restrict__ vc,
                         const float* __restrict__ cos_t,    // [S, 64]
                         const float* __restrict__ sin_t,
                         const int* __restrict__ pos_dev,
                         int B, int Hq, int Hkv, int T, int pos_host,
                         int per_row) {
  const int nh = Hq + 2 * Hkv;
  const int b = blockIdx.x / nh;
  const int h = blockIdx.x % nh;
  const int pos = pos_dev ? pos_dev[per_row ? b : 0] : pos_host;
  decode_rope_append(qkv, qout, kc, vc, cos_t, sin_t, b, h, Hq, Hkv, pos,
                     (long)b * T + pos);
}

extern "C" void decode_rope_cache_launch(const void* qkv, void* qout,
                                         void* kc, void* vc,
                                         const void* cos_t, const void* sin_t,
                                         const void* pos_dev, int B, int Hq,
                                         int Hkv, int T, int pos_host,
                                         int per_row, hipStream_t stream) {
  hipLaunchKernelGGL(decode_rope_cache_kernel, dim3(B * (Hq + 2 * Hkv)),
                     dim3(64), 0, stream, (const unsigned short*)qkv,
                     (unsigned short*)qout, (unsigned short*)kc,
                     (unsigned short*)vc, (const float*)cos_t,
                     (const float*)sin_t, (const int*)pos_dev, B, Hq, Hkv, T,
                     pos_host, per_row);
}

// ---- split-K (flash-decode) variant ---------------------------------------
// At decode batch 4 the single-pass kernel launches only B*Hq = 128 blocks
// on 256 CUs — half the chip idles and each block serially streams its
// whole K/V slice (~25 us/layer measured). Pass 1 splits the cache length
// across gridDim.y blocks, each producing an UNNORMALIZED partial
// (m, l, o[128]) in f32 scratch; pass 2 (one small block per (b, hq))
// combines the partials exactly like the in-block wave merge.
__global__ void __launch_bounds__(256)
decode_attn_split_kernel(const unsigned short* __restrict__ q,
                         const unsigned short* __restrict__ kc,
                         const unsigned short* __restrict__ vc,
                         float* __restrict__ ml,    // [B*Hq, SPLIT, 2]
                         float* __restrict__ oacc,  // [B*Hq, SPLIT, 128]
                         const int* __restrict__ len_dev,
                         int B, int Hq, int Hkv, int T, int L_host,
                         int per_row, float scale) {
  const int bq = blockIdx.x;
  const int b = bq / Hq;
  const int hq = bq % Hq;
  const int L = dense_len(len_dev, per_row, b, L_host);
  const int split = gridDim.y;
  const int chunk = (L + split - 1) / split;
  const int t0 = blockIdx.y * chunk;
  const int t1 = min(L, t0 + chunk);
  const long pbase = (long)bq * split + blockIdx.y;
  decode_attn_block(q + (long)bq * HD,
                    dense_rows(kc, vc, b, hq / (Hq / Hkv), Hkv, T), t0, t1,
                    scale, StorePartial{ml + pbase * 2, oacc + pbase * HD});
}

// pass 2: one 128-thread block per (b, hq); thread d combines SPLIT
// partials and writes the normalized bf16 output element.
__global__ void __launch_bounds__(128)
decode_attn_merge_kernel(const float* __restrict__ ml,
                         const float* __restrict__ oacc,
                         unsigned short* __restrict__ o,  // [B, Hq, 128]
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

extern "C" void decode_attn_merge_launch(const void* ml, const void* oacc,
                                         void* o, int BHq, int split,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(decode_attn_merge_kernel, dim3(BHq), dim3(128), 0,
                     stream, (const float*)ml, (const float*)oacc,
                     (unsigned short*)o, split);
}

extern "C" void decode_attn_split_launch(const void* q, const void* kc,
                                         const void* vc, void* ml,
                                         void* oacc, void* o,
                                         const void* len_dev, int B, int Hq,
                                         int Hkv, int T, int L, int split,
                                         int per_row, float scale,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(decode_attn_split_kernel, dim3(B * Hq, split),
                     dim3(256), 0, stream, (const unsigned short*)q,
                     (const unsigned short*)kc, (const unsigned short*)vc,
                     (float*)ml, (float*)oacc, (const int*)len_dev, B, Hq,
                     Hkv, T, L, per_row, scale);
  decode_attn_merge_launch(ml, oacc, o, B * Hq, split, stream);
}
