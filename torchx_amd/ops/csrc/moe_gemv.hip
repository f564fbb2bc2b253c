// Device-routed MoE decode MLP: grouped expert GEMVs that read the top-k
// routing from device memory, so the MLP half of a Mixtral decode step is
// two dispatches and no host round trip.
//
//   A  moe_gemv_swiglu_kernel        h[b, j]  = swiglu(x[b] @ wgu_e^T)
//   B  moe_gemv_down_combine_kernel  out[b]   = sum_e c * (h[b, j_e] @ wdown_e^T)
//
// for every (token b, slot j) with e = idx[b, j], c = cw[b, j].
// x [B, H], idx [B, k] int64 (torch.topk), cw [B, k], B <= 8, k <= 8;
// E <= 16 experts, each its own wgu_e [2I, H] and wdown_e [H, I] tensor;
// H % 512 == 0, I % 512 == 0. The E base pointers travel by value in the
// kernel arguments (ExpertPtrs): a wave indexes them with a wave-uniform
// expert number, which is a scalar load from the kernarg segment — no
// device pointer table, no copy, no lifetime question.
//
// Routing prologue (once per wave, wave-uniform, lives in SGPRs): lane l
// loads idx[l] for l < B*k — one vector load — and clamps it to [0, E),
// so no routing content can address outside a weight. A ballot of
// "my entry == e" is then the 64-bit (token, slot) pair mask of expert e:
// token b owns bits [b*k, b*k + k). From it come the 8-bit token mask,
// m_e = popcount(mask), which selects the M-templated body by a uniform
// switch, and per token the slot j (first set bit of its k bits). Token m
// of the body is the m-th set bit of the mask; its row is addressed
// directly, there is no gather.
//
// Arithmetic contract — the fused path is bit-identical to the per-expert
// loop decode_linear_swiglu -> decode_linear -> out[rows] += ye * coef:
//   - gate/up/down dot products accumulate exactly as in gemv.hip: lane
//     owns k = lane*8 + 512*chunk, 4-chunk main loop and 1-chunk tail,
//     fdot2 over j2 = 0..3 per chunk in order, 6-step shfl_xor butterfly
//     (32 down to 1); every (token, row) chain is independent of M;
//   - h  = bf16(g * (1 / (1 + exp2(-1.44269504 g))) * u);
//   - ye = bf16(acc);
//   - t  = bf16(f32(ye) * f32(c));
//   - the running output starts at +0 and is updated
//     o = bf16(f32(o) + f32(t)) over the experts in ascending order,
//     which is what the bf16 `out[rows] += ye * coef[:, None]` of the loop
//     computes;
//   - fp contraction is off in this file, so no rounding is fused away.
#include "common.h"

// no fused multiply-add may swallow a rounding of the contract
#pragma clang fp contract(off)

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct ExpertPtrs {
  const unsigned short* p[16];
};

__device__ __forceinline__ float moe_dot2(ushort8 a, ushort8 b, float acc,
                                          int j2) {
  return __builtin_amdgcn_fdot2_f32_bf16(((const bf16x2*)&a)[j2],
                                         ((const bf16x2*)&b)[j2], acc,
                                         false);
}

// round-to-nearest-even with torch's NaN result, for the combine steps
// that stand for torch bf16 arithmetic
__device__ __forceinline__ unsigned short f32_to_bf16_nan(float f) {
  return f != f ? (unsigned short)0x7fc0 : f32_to_bf16(f);
}

// This lane's clamped routing entry; -1 on lanes past the B*k entries.
__device__ __forceinline__ int moe_lane_expert(const long* __restrict__ idx,
                                               int lane, int BK, int E) {
  if (lane >= BK) return -1;
  const long v = idx[lane];
  return (int)(v < 0 ? 0 : (v >= E ? E - 1 : v));
}

// 8-bit token mask of a (token, slot) pair mask.
__device__ __forceinline__ unsigned moe_token_mask(unsigned long pm, int k) {
  const unsigned long kmask = (1ul << k) - 1;
  unsigned tmask = 0;
  #pragma unroll
  for (int b = 0; b < 8; ++b)
    if ((pm >> (b * k)) & kmask) tmask |= 1u << b;
  return tmask;
}

// Tokens (ascending) and their (token, slot) pair index for one expert.
template <int M>
__device__ __forceinline__ void moe_tokens(unsigned long pm, unsigned tmask,
                                           int k, int (&tok)[M],
                                           int (&pair)[M]) {
  const unsigned long kmask = (1ul << k) - 1;
  #pragma unroll
  for (int m = 0; m < M; ++m) {
    tok[m] = __builtin_ctz(tmask);
    tmask &= tmask - 1;
    const unsigned long seg = (pm >> (tok[m] * k)) & kmask;
    pair[m] = tok[m] * k + __builtin_ctzl(seg);
  }
}

// ---- kernel A ---------------------------------------------------------------
// gemv_swiglu_bf16_kernel's body on the expert's tokens: gate row n and up
// row n + I of wgu_e against the x rows tok[0..M).
template <int M>
__device__ __forceinline__ void moe_swiglu_body(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w,
    unsigned short* __restrict__ h, unsigned long pm, unsigned tmask, int k,
    int n, int I, int K, int lane) {
  int tok[M], pair[M];
  moe_tokens<M>(pm, tmask, k, tok, pair);
  const unsigned short* xr[M];
  #pragma unroll
  for (int m = 0; m < M; ++m) xr[m] = x + (long)tok[m] * K;

  float acc[M][2];
  #pragma unroll
  for (int m = 0; m < M; ++m) acc[m][0] = acc[m][1] = 0.f;

  int kc = lane * 8;
  for (; kc + 512 * 3 < K; kc += 512 * 4) {
    ushort8 xf[M][4];
    #pragma unroll
    for (int u = 0; u < 4; ++u)
      #pragma unroll
      for (int m = 0; m < M; ++m)
        xf[m][u] = *(const ushort8*)(xr[m] + kc + 512 * u);
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned short* wr = w + (long)(n + r * I) * K + kc;
      ushort8 wf[4];
      #pragma unroll
      for (int u = 0; u < 4; ++u) wf[u] = *(const ushort8*)(wr + 512 * u);
      #pragma unroll
      for (int u = 0; u < 4; ++u)
        #pragma unroll
        for (int j2 = 0; j2 < 4; ++j2)
          #pragma unroll
          for (int m = 0; m < M; ++m)
            acc[m][r] = moe_dot2(xf[m][u], wf[u], acc[m][r], j2);
    }
  }
  for (; kc < K; kc += 512) {
    ushort8 xf[M];
    #pragma unroll
    for (int m = 0; m < M; ++m) xf[m] = *(const ushort8*)(xr[m] + kc);
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      ushort8 wf = *(const ushort8*)(w + (long)(n + r * I) * K + kc);
      #pragma unroll
      for (int j2 = 0; j2 < 4; ++j2)
        #pragma unroll
        for (int m = 0; m < M; ++m)
          acc[m][r] = moe_dot2(xf[m], wf, acc[m][r], j2);
    }
  }

  #pragma unroll
  for (int m = 0; m < M; ++m)
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      float v = acc[m][r];
      #pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      acc[m][r] = v;
    }
  if (lane == 0) {
    #pragma unroll
    for (int m = 0; m < M; ++m) {
      const float g = acc[m][0], u = acc[m][1];
      const float sig =
          1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * g));
      h[(long)pair[m] * I + n] = f32_to_bf16(g * sig * u);
    }
  }
}

// grid (I/4, E), 256 threads; wave w of block (bx, e) owns gate row
// 4*bx + w of expert e. No barrier anywhere, so a wave may leave alone.
__global__ void __launch_bounds__(256)
moe_gemv_swiglu_kernel(const unsigned short* __restrict__ x,   // [B, H]
                       const long* __restrict__ idx,           // [B, k]
                       ExpertPtrs wgu,                         // E x [2I, H]
                       unsigned short* __restrict__ h,         // [B, k, I]
                       int B, int k, int E, int I, int H) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.y;
  const int n = blockIdx.x * 4 + wave;
  const int mine = moe_lane_expert(idx, lane, B * k, E);
  const unsigned long pm = __ballot(mine == e);
  if (pm == 0 || n >= I) return;  // idle expert: before any weight load
  const unsigned tmask = moe_token_mask(pm, k);
  const unsigned short* __restrict__ w = wgu.p[e];
  switch (__builtin_popcount(tmask)) {
    #define MOE_A_CASE(MM)                                                  \
      case MM:                                                              \
        moe_swiglu_body<MM>(x, w, h, pm, tmask, k, n, I, H, lane);          \
        break;
    MOE_A_CASE(1) MOE_A_CASE(2) MOE_A_CASE(3) MOE_A_CASE(4)
    MOE_A_CASE(5) MOE_A_CASE(6) MOE_A_CASE(7) MOE_A_CASE(8)
    #undef MOE_A_CASE
    default: break;
  }
}

// ---- kernel B ---------------------------------------------------------------
// gemv_bf16_kernel's body (RPW = 2) for one expert: rows n0, n0 + 1 of
// wdown_e against the h rows of the expert's (token, slot) pairs, then the
// ordered bf16 fold into the lanes' running outputs: lane tok + 8 r holds
// out[tok, n0 + r]. After the butterfly every lane has the reduced value,
// so the update is a select — no runtime-indexed registers.
template <int M>
__device__ __forceinline__ unsigned short moe_down_body(
    const unsigned short* __restrict__ h, const unsigned short* __restrict__ w,
    unsigned long pm, unsigned tmask, int k, unsigned cwv, int n0, int K,
    int lane, unsigned short o) {
  int tok[M], pair[M];
  moe_tokens<M>(pm, tmask, k, tok, pair);
  const unsigned short* xr[M];
  #pragma unroll
  for (int m = 0; m < M; ++m) xr[m] = h + (long)pair[m] * K;

  float acc[M][2];
  #pragma unroll
  for (int m = 0; m < M; ++m) acc[m][0] = acc[m][1] = 0.f;

  int kc = lane * 8;
  for (; kc + 512 * 3 < K; kc += 512 * 4) {
    ushort8 xf[M][4];
    #pragma unroll
    for (int u = 0; u < 4; ++u)
      #pragma unroll
      for (int m = 0; m < M; ++m)
        xf[m][u] = *(const ushort8*)(xr[m] + kc + 512 * u);
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned short* wr = w + (long)(n0 + r) * K + kc;
      ushort8 wf[4];
      #pragma unroll
      for (int u = 0; u < 4; ++u) wf[u] = *(const ushort8*)(wr + 512 * u);
      #pragma unroll
      for (int u = 0; u < 4; ++u)
        #pragma unroll
        for (int j2 = 0; j2 < 4; ++j2)
          #pragma unroll
          for (int m = 0; m < M; ++m)
            acc[m][r] = moe_dot2(xf[m][u], wf[u], acc[m][r], j2);
    }
  }
  for (; kc < K; kc += 512) {
    ushort8 xf[M];
    #pragma unroll
    for (int m = 0; m < M; ++m) xf[m] = *(const ushort8*)(xr[m] + kc);
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      ushort8 wf = *(const ushort8*)(w + (long)(n0 + r) * K + kc);
      #pragma unroll
      for (int j2 = 0; j2 < 4; ++j2)
        #pragma unroll
        for (int m = 0; m < M; ++m)
          acc[m][r] = moe_dot2(xf[m], wf, acc[m][r], j2);
    }
  }

  #pragma unroll
  for (int m = 0; m < M; ++m) {
    // c = cw[tok, slot]: lane `pair` loaded it in the prologue
    const float c = bf16_to_f32(
        (unsigned short)__builtin_amdgcn_readlane((int)cwv, pair[m]));
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      float v = acc[m][r];
      #pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      const float ye = bf16_to_f32(f32_to_bf16(v));
      const float t = bf16_to_f32(f32_to_bf16_nan(ye * c));
      const unsigned short on = f32_to_bf16_nan(bf16_to_f32(o) + t);
      o = lane == tok[m] + 8 * r ? on : o;
    }
  }
  return o;
}

// grid H/8, 256 threads; a wave owns output rows n0, n0 + 1 for all tokens
// and walks the experts in ascending order.
__global__ void __launch_bounds__(256)
moe_gemv_down_combine_kernel(const unsigned short* __restrict__ h,   // [B,k,I]
                             const long* __restrict__ idx,           // [B, k]
                             const unsigned short* __restrict__ cw,  // [B, k]
                             ExpertPtrs wdown,                       // E x [H, I]
                             unsigned short* __restrict__ out,       // [B, H]
                             int B, int k, int E, int I, int H) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * 2;
  if (n0 >= H) return;
  const int mine = moe_lane_expert(idx, lane, B * k, E);
  const unsigned cwv = lane < B * k ? cw[lane] : 0;
  unsigned short o = 0;  // +0, as torch.zeros_like
  for (int e = 0; e < E; ++e) {
    const unsigned long pm = __ballot(mine == e);
    if (pm == 0) continue;  // idle expert: none of its weight is read
    const unsigned tmask = moe_token_mask(pm, k);
    const unsigned short* __restrict__ w = wdown.p[e];
    switch (__builtin_popcount(tmask)) {
      #define MOE_B_CASE(MM)                                                \
        case MM:                                                            \
          o = moe_down_body<MM>(h, w, pm, tmask, k, cwv, n0, I, lane, o);   \
          break;
      MOE_B_CASE(1) MOE_B_CASE(2) MOE_B_CASE(3) MOE_B_CASE(4)
      MOE_B_CASE(5) MOE_B_CASE(6) MOE_B_CASE(7) MOE_B_CASE(8)
      #undef MOE_B_CASE
      default: break;
    }
  }
  const int b = lane & 7, r = lane >> 3;
  if (r < 2 && b < B) out[(long)b * H + n0 + r] = o;
}

// ---- launchers --------------------------------------------------------------
static ExpertPtrs moe_pack(const void* const* w, int E) {
  ExpertPtrs p;
  for (int e = 0; e < 16; ++e)
    p.p[e] = (const unsigned short*)w[e < E ? e : 0];
  return p;
}

// callers guard 1 <= B, k <= 8, 1 <= E <= 16, H % 512 == I % 512 == 0
extern "C" void moe_gemv_swiglu_launch(const void* x, const void* idx,
                                       const void* const* wgu, void* h, int B,
                                       int k, int E, int I, int H,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(moe_gemv_swiglu_kernel, dim3(I / 4, E), dim3(256), 0,
                     stream, (const unsigned short*)x, (const long*)idx,
                     moe_pack(wgu, E), (unsigned short*)h, B, k, E, I, H);
}

extern "C" void moe_gemv_down_combine_launch(const void* h, const void* idx,
                                             const void* cw,
                                             const void* const* wdown,
                                             void* out, int B, int k, int E,
                                             int I, int H,
                                             hipStream_t stream) {
  hipLaunchKernelGGL(moe_gemv_down_combine_kernel, dim3(H / 8), dim3(256), 0,
                     stream, (const unsigned short*)h, (const long*)idx,
                     (const unsigned short*)cw, moe_pack(wdown, E),
                     (unsigned short*)out, B, k, E, I, H);
}
