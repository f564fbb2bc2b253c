// W8A16 device-routed MoE decode MLP: moe_gemv.hip's two grouped expert
// kernels on fp8 e4m3 expert weights with one fp32 scale per weight row
// (ops.Fp8Weight), so the Mixtral decode MLP streams half the bytes.
//
//   A  moe_gemv_swiglu_fp8w_kernel        h[b, j] = swiglu(x[b] @ wgu_e^T)
//   B  moe_gemv_down_combine_fp8w_kernel  out[b]  = sum_e c * (h[b, j_e] @ wdown_e^T)
//
// for every (token b, slot j) with e = idx[b, j], c = cw[b, j], where
// wgu_e = scale_e[:, None] * w8_e. x [B, H] bf16, idx [B, k] int64, cw
// [B, k] bf16, B <= 8, k <= 8; E <= 16 experts, each its own w8 [2I, H] /
// [H, I] e4m3 tensor and scale [2I] / [H] fp32 tensor; H % 1024 == 0 and
// I % 1024 == 0, so no wave is partial. The experts' w8 and scale base
// pointers travel by value in the kernel arguments (two 16-entry structs)
// and are indexed by the wave-uniform expert number: scalar loads from
// the kernarg segment, as in moe_gemv.hip.
//
// The routing prologue is moe_gemv.hip's: one vector load of idx per lane,
// clamped to [0, E); a ballot gives the (token, slot) pair mask of an
// expert, from it the token mask, m_e = popcount, and a uniform switch
// selects the body instantiated for M = 1..8. Token rows are addressed
// directly, there is no gather.
//
// Arithmetic contract — bit-identical to the per-expert loop wherever the
// loop runs gemv_fp8.hip's dot2 kernels:
//   - every (token, row) dot product is gemv_fp8.hip's fp8_rows_dot chain:
//     a lane owns k = 16 lane + 1024 chunk, the main loop takes 2 chunks
//     with all weight loads of the iteration issued before the first
//     convert, a 1-chunk tail follows; 16 weights are 8 converts
//     (v_cvt_scalef32_pk_bf16_fp8, scale operand 1.0, sel = false, true)
//     into v_dot2c_f32_bf16 in the order d = 0..3, sel = 0, 1 (byte order:
//     see gemv_fp8.hip); a 6-step shfl_xor butterfly (32 down to 1)
//     reduces the wave; the row scale multiplies the reduced fp32 sum
//     once. The chain depends neither on M nor on the rows per wave;
//   - h  = bf16(g * (1 / (1 + exp2(-1.44269504 g))) * u), g and u scaled;
//   - ye = bf16(scale * acc);
//   - t  = bf16(f32(ye) * f32(c));
//   - o  = bf16(f32(o) + f32(t)) from +0 over the experts in ascending
//     order, with torch's NaN result, as in moe_gemv.hip;
//   - fp contraction is off in this file.
//
// Groups of 6 to 8 tokens per expert also run on the dot2 body (VALU-bound
// there, and rare at decode batch sizes); a grouped MFMA variant is not
// part of this file.
#include "common.h"

// no fused multiply-add may swallow a rounding of the contract
#pragma clang fp contract(off)

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int MOE8_CHUNK = 1024;  // k per wave load instruction
// Kernel B's default output rows per wave. Measured at the 8x7B shape
// (H 4096, I 14336, tools/moe_probe.py, profiles/README.md r14a), 2 against
// 4 rows: 22.2 / 63.8 / 101.7 us against 27.8 / 75.4 / 118.4 us at
// B = 1 / 4 / 8.
constexpr int MOE8_DOWN_ROWS = 2;

struct ExpertW8 {
  const unsigned char* p[16];
};
struct ExpertScale {
  const float* p[16];
};

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

// x fragment of one chunk: xf[m][0] = elements 0..7 of the lane's 16,
// xf[m][1] = elements 8..15
template <int M>
__device__ __forceinline__ void moe_load_x16(
    ushort8 (&xf)[M][2], const unsigned short* const (&xr)[M], int kc) {
  #pragma unroll
  for (int m = 0; m < M; ++m) {
    xf[m][0] = *(const ushort8*)(xr[m] + kc);
    xf[m][1] = *(const ushort8*)(xr[m] + kc + 8);
  }
}

// gemv_fp8.hip's mac16: 16 weights of one row against the M x fragments
template <int M>
__device__ __forceinline__ void moe_mac16(float (&acc)[M], const uint4_v w,
                                          const ushort8 (&xf)[M][2]) {
  #pragma unroll
  for (int d = 0; d < 4; ++d) {
    // the builtin wants sel as a literal
    const bf16x2 wp[2] = {
        __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[d], 1.0f, false),
        __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[d], 1.0f, true)};
    #pragma unroll
    for (int sel = 0; sel < 2; ++sel) {
      const int p = 2 * d + sel;  // the lane's bf16 pair these weights meet
      #pragma unroll
      for (int m = 0; m < M; ++m)
        acc[m] = __builtin_amdgcn_fdot2_f32_bf16(
            ((const bf16x2*)&xf[m][p >> 2])[p & 3], wp[sel], acc[m], false);
    }
  }
}

// gemv_fp8.hip's fp8_rows_dot on row pointers: acc[r][m] = sum_k
// xr[m][k] * wr[r][k], wave-reduced (every lane holds the sum).
template <int M, int ROWS>
__device__ __forceinline__ void moe_fp8_rows_dot(
    float (&acc)[ROWS][M], const unsigned short* const (&xr)[M],
    const unsigned char* const (&wr)[ROWS], int K, int lane) {
  #pragma unroll
  for (int r = 0; r < ROWS; ++r)
    #pragma unroll
    for (int m = 0; m < M; ++m) acc[r][m] = 0.f;

  int kc = lane * 16;  // this lane's first k within a chunk
  for (; kc + MOE8_CHUNK < K; kc += 2 * MOE8_CHUNK) {  // 2 chunks
    uint4_v wf[ROWS][2];
    #pragma unroll
    for (int r = 0; r < ROWS; ++r)
      #pragma unroll
      for (int u = 0; u < 2; ++u)
        wf[r][u] = *(const uint4_v*)(wr[r] + kc + MOE8_CHUNK * u);
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      ushort8 xf[M][2];
      moe_load_x16<M>(xf, xr, kc + MOE8_CHUNK * u);
      #pragma unroll
      for (int r = 0; r < ROWS; ++r) moe_mac16<M>(acc[r], wf[r][u], xf);
    }
  }
  for (; kc < K; kc += MOE8_CHUNK) {  // 1-chunk tail
    uint4_v wf[ROWS];
    #pragma unroll
    for (int r = 0; r < ROWS; ++r)
      wf[r] = *(const uint4_v*)(wr[r] + kc);
    ushort8 xf[M][2];
    moe_load_x16<M>(xf, xr, kc);
    #pragma unroll
    for (int r = 0; r < ROWS; ++r) moe_mac16<M>(acc[r], wf[r], xf);
  }

  #pragma unroll
  for (int r = 0; r < ROWS; ++r)
    #pragma unroll
    for (int m = 0; m < M; ++m) {
      float v = acc[r][m];
      #pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      acc[r][m] = v;
    }
}

// ---- kernel A ---------------------------------------------------------------
// gemv_swiglu_fp8w_kernel's body on the expert's tokens: gate rows n0,
// n0 + 1 and up rows n0 + I, n0 + 1 + I of w8_e (four row streams per
// wave) against the x rows tok[0..M).
template <int M>
__device__ __forceinline__ void moe_swiglu_fp8w_body(
    const unsigned short* __restrict__ x, const unsigned char* __restrict__ w,
    const float* __restrict__ scale, unsigned short* __restrict__ h,
    unsigned long pm, unsigned tmask, int k, int n0, int I, int K, int lane) {
  int tok[M], pair[M];
  moe_tokens<M>(pm, tmask, k, tok, pair);
  const unsigned short* xr[M];
  #pragma unroll
  for (int m = 0; m < M; ++m) xr[m] = x + (long)tok[m] * K;
  // gate rows first, then their up rows
  const unsigned char* wr[4] = {
      w + (long)n0 * K, w + (long)(n0 + 1) * K,
      w + (long)(n0 + I) * K, w + (long)(n0 + 1 + I) * K};

  float acc[4][M];
  moe_fp8_rows_dot<M, 4>(acc, xr, wr, K, lane);

  if (lane == 0) {
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float sg = scale[n0 + r], su = scale[n0 + r + I];
      #pragma unroll
      for (int m = 0; m < M; ++m) {
        const float g = acc[r][m] * sg, u = acc[2 + r][m] * su;
        const float sig =
            1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * g));
        h[(long)pair[m] * I + n0 + r] = f32_to_bf16(g * sig * u);
      }
    }
  }
}

// grid (I/8, E), 256 threads; wave w of block (bx, e) owns gate rows
// 8*bx + 2*w, + 1 of expert e. No barrier anywhere, so a wave may leave
// alone.
__global__ void __launch_bounds__(256)
moe_gemv_swiglu_fp8w_kernel(const unsigned short* __restrict__ x,  // [B, H]
                            const long* __restrict__ idx,          // [B, k]
                            ExpertW8 wgu,                          // E x [2I, H]
                            ExpertScale sgu,                       // E x [2I]
                            unsigned short* __restrict__ h,        // [B, k, I]
                            int B, int k, int E, int I, int H) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.y;
  const int n0 = (blockIdx.x * 4 + wave) * 2;
  const int mine = moe_lane_expert(idx, lane, B * k, E);
  const unsigned long pm = __ballot(mine == e);
  if (pm == 0 || n0 >= I) return;  // idle expert: before any weight load
  const unsigned tmask = moe_token_mask(pm, k);
  const unsigned char* __restrict__ w = wgu.p[e];
  const float* __restrict__ s = sgu.p[e];
  switch (__builtin_popcount(tmask)) {
    #define MOE8_A_CASE(MM)                                                 \
      case MM:                                                              \
        moe_swiglu_fp8w_body<MM>(x, w, s, h, pm, tmask, k, n0, I, H, lane); \
        break;
    MOE8_A_CASE(1) MOE8_A_CASE(2) MOE8_A_CASE(3) MOE8_A_CASE(4)
    MOE8_A_CASE(5) MOE8_A_CASE(6) MOE8_A_CASE(7) MOE8_A_CASE(8)
    #undef MOE8_A_CASE
    default: break;
  }
}

// ---- kernel B ---------------------------------------------------------------
// gemv_fp8w_kernel's body for one expert: rows n0 .. n0 + ROWS - 1 of w8_e
// against the h rows of the expert's (token, slot) pairs, then the ordered
// bf16 fold into the lanes' running outputs: lane tok + 8 r holds
// out[tok, n0 + r]. After the butterfly every lane has the reduced value,
// so the update is a select — no runtime-indexed registers.
template <int M, int ROWS>
__device__ __forceinline__ unsigned short moe_down_fp8w_body(
    const unsigned short* __restrict__ h, const unsigned char* __restrict__ w,
    const float* __restrict__ scale, unsigned long pm, unsigned tmask, int k,
    unsigned cwv, int n0, int K, int lane, unsigned short o) {
  int tok[M], pair[M];
  moe_tokens<M>(pm, tmask, k, tok, pair);
  const unsigned short* xr[M];
  #pragma unroll
  for (int m = 0; m < M; ++m) xr[m] = h + (long)pair[m] * K;
  const unsigned char* wr[ROWS];
  #pragma unroll
  for (int r = 0; r < ROWS; ++r) wr[r] = w + (long)(n0 + r) * K;

  float acc[ROWS][M];
  moe_fp8_rows_dot<M, ROWS>(acc, xr, wr, K, lane);

  #pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const float s = scale[n0 + r];
    #pragma unroll
    for (int m = 0; m < M; ++m) {
      // c = cw[tok, slot]: lane `pair` loaded it in the prologue
      const float c = bf16_to_f32(
          (unsigned short)__builtin_amdgcn_readlane((int)cwv, pair[m]));
      const float ye = bf16_to_f32(f32_to_bf16(acc[r][m] * s));
      const float t = bf16_to_f32(f32_to_bf16_nan(ye * c));
      const unsigned short on = f32_to_bf16_nan(bf16_to_f32(o) + t);
      o = lane == tok[m] + 8 * r ? on : o;
    }
  }
  return o;
}

// grid H/(4 ROWS), 256 threads; a wave owns output rows n0 .. n0 + ROWS - 1
// for all tokens and walks the experts in ascending order.
template <int ROWS>
__global__ void __launch_bounds__(256)
moe_gemv_down_combine_fp8w_kernel(
    const unsigned short* __restrict__ h,   // [B, k, I]
    const long* __restrict__ idx,           // [B, k]
    const unsigned short* __restrict__ cw,  // [B, k]
    ExpertW8 wdown,                         // E x [H, I]
    ExpertScale sdown,                      // E x [H]
    unsigned short* __restrict__ out,       // [B, H]
    int B, int k, int E, int I, int H) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  if (n0 >= H) return;
  const int mine = moe_lane_expert(idx, lane, B * k, E);
  const unsigned cwv = lane < B * k ? cw[lane] : 0;
  unsigned short o = 0;  // +0, as torch.zeros_like
  for (int e = 0; e < E; ++e) {
    const unsigned long pm = __ballot(mine == e);
    if (pm == 0) continue;  // idle expert: none of its weight is read
    const unsigned tmask = moe_token_mask(pm, k);
    const unsigned char* __restrict__ w = wdown.p[e];
    const float* __restrict__ s = sdown.p[e];
    switch (__builtin_popcount(tmask)) {
      #define MOE8_B_CASE(MM)                                               \
        case MM:                                                            \
          o = moe_down_fp8w_body<MM, ROWS>(h, w, s, pm, tmask, k, cwv, n0,  \
                                           I, lane, o);                     \
          break;
      MOE8_B_CASE(1) MOE8_B_CASE(2) MOE8_B_CASE(3) MOE8_B_CASE(4)
      MOE8_B_CASE(5) MOE8_B_CASE(6) MOE8_B_CASE(7) MOE8_B_CASE(8)
      #undef MOE8_B_CASE
      default: break;
    }
  }
  const int b = lane & 7, r = lane >> 3;
  if (r < ROWS && b < B) out[(long)b * H + n0 + r] = o;
}

// ---- launchers --------------------------------------------------------------
static ExpertW8 moe8_pack_w(const void* const* w, int E) {
  ExpertW8 p;
  for (int e = 0; e < 16; ++e)
    p.p[e] = (const unsigned char*)w[e < E ? e : 0];
  return p;
}

static ExpertScale moe8_pack_s(const void* const* s, int E) {
  ExpertScale p;
  for (int e = 0; e < 16; ++e) p.p[e] = (const float*)s[e < E ? e : 0];
  return p;
}

// callers guard 1 <= B, k <= 8, 1 <= E <= 16, H % 1024 == I % 1024 == 0
extern "C" void moe_gemv_swiglu_fp8w_launch(const void* x, const void* idx,
                                            const void* const* w8,
                                            const void* const* scale, void* h,
                                            int B, int k, int E, int I, int H,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(moe_gemv_swiglu_fp8w_kernel, dim3(I / 8, E), dim3(256),
                     0, stream, (const unsigned short*)x, (const long*)idx,
                     moe8_pack_w(w8, E), moe8_pack_s(scale, E),
                     (unsigned short*)h, B, k, E, I, H);
}

template <int ROWS>
static void moe8_down_launch_rows(const void* h, const void* idx,
                                  const void* cw, const void* const* w8,
                                  const void* const* scale, void* out, int B,
                                  int k, int E, int I, int H,
                                  hipStream_t stream) {
  hipLaunchKernelGGL((moe_gemv_down_combine_fp8w_kernel<ROWS>),
                     dim3(H / (4 * ROWS)), dim3(256), 0, stream,
                     (const unsigned short*)h, (const long*)idx,
                     (const unsigned short*)cw, moe8_pack_w(w8, E),
                     moe8_pack_s(scale, E), (unsigned short*)out, B, k, E, I,
                     H);
}

// rows = 2 or 4 forces the output rows per wave (tools/moe_probe.py), 0
// takes the default
extern "C" void moe_gemv_down_combine_fp8w_launch(
    const void* h, const void* idx, const void* cw, const void* const* w8,
    const void* const* scale, void* out, int B, int k, int E, int I, int H,
    int rows, hipStream_t stream) {
  if (rows == 0) rows = MOE8_DOWN_ROWS;
  if (rows == 4)
    moe8_down_launch_rows<4>(h, idx, cw, w8, scale, out, B, k, E, I, H,
                             stream);
  else
    moe8_down_launch_rows<2>(h, idx, cw, w8, scale, out, B, k, E, I, H,
                             stream);
}
