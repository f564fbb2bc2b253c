// W8A16 skinny-M GEMV for the decode path: fp8 e4m3 weights with one fp32
// scale per output row, bf16 activations, bf16 output.
//
//   out[m, n] = bf16(scale[n] * sum_k x[m, k] * w8[n, k])
//
// with M <= 8, K % 1024 == 0, w8 row-major [N, K] (OCP e4m3,
// torch.float8_e4m3fn). gemv.hip is W-stream bound and already reads
// every bf16 weight byte once; this kernel halves the bytes.
//
// Layout. 256-thread blocks (4 waves), a wave owns ROWS = 4 weight rows
// (2 for small problems, see gemv_fp8w_launch) and marches K in 1024-element chunks: a lane loads 16 B = 16 weights,
// the wave's load instruction covers 1 KB of one row. The lane's x
// fragment for a chunk is 16 bf16 = two 16-B loads per token (L2-resident
// as in gemv.hip) and is shared by the wave's rows. The main loop takes 2
// chunks at a time and issues all ROWS * 2 weight loads (128 B per lane,
// what gemv.hip keeps in flight with 2 rows x 4 chunks of bf16) before the
// first MAC; a 1-chunk tail follows when K % 2048 != 0. x costs 8 VGPRs
// per (token, chunk), twice gemv.hip's, which is why the unroll is 2 and
// not 4: at M = 8 the two chunks of x are 128 VGPRs.
//
// Convert and byte order. v_cvt_scalef32_pk_bf16_fp8 turns one 16-bit half
// of a weight dword into a packed bf16 pair in one VALU op, and the pair
// feeds v_dot2c_f32_bf16 directly. Every e4m3 value is exact in bf16, so
// the convert (scale operand 1.0) rounds nothing. Memory is little
// endian: dword d (0..3) of the lane's 16 B holds the weights
// k0 + 4d .. k0 + 4d + 3 in bytes 0..3, k0 = chunk base + 16 * lane.
//   sel = false: byte 0 -> pair.x (low bf16), byte 1 -> pair.y
//                = weights k0 + 4d, k0 + 4d + 1 = bf16 pair 2d of the lane
//   sel = true:  byte 2 -> pair.x, byte 3 -> pair.y
//                = weights k0 + 4d + 2, k0 + 4d + 3 = bf16 pair 2d + 1
// x pair p (0..7) of the lane is the elements k0 + 2p, k0 + 2p + 1, low
// half first: pairs 0..3 lie in the first 16-B x load, 4..7 in the second.
// So weight pair (d, sel) meets x pair p = 2d + sel, element for element.
//
// The row scale is applied once, in fp32, to the wave-reduced sum: putting
// it into the convert would round every scaled weight to bf16 again.
//
// VALU budget: per weight byte (1 + M) / 2 ops (one convert and M dot2 per
// two weights) against M / 4 in gemv.hip.
#include "common.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int FP8_ROWS = 4;      // weight rows per wave
constexpr int FP8_CHUNK = 1024;  // k per wave load instruction

// x fragment of one chunk: xf[m][0] = elements 0..7 of the lane's 16,
// xf[m][1] = elements 8..15
template <int M>
__device__ __forceinline__ void load_x16(ushort8 (&xf)[M][2],
                                         const unsigned short* __restrict__ x,
                                         int K, int kc) {
  #pragma unroll
  for (int m = 0; m < M; ++m) {
    const unsigned short* xr = x + (long)m * K + kc;
    xf[m][0] = *(const ushort8*)xr;
    xf[m][1] = *(const ushort8*)(xr + 8);
  }
}

// 16 weights of one row against the M x fragments: 8 converts, 8 M dot2
template <int M>
__device__ __forceinline__ void mac16(float (&acc)[M], const uint4_v w,
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

// acc[r][m] = sum_k x[m, k] * w8[row[r], k], wave-reduced (every lane holds
// the sum). The rows are whatever the caller names: consecutive rows for
// the plain kernel, gate rows and their up rows for the SwiGLU one.
template <int M, int ROWS>
__device__ __forceinline__ void fp8_rows_dot(
    float (&acc)[ROWS][M], const unsigned short* __restrict__ x,
    const unsigned char* __restrict__ w, const int (&row)[ROWS], int K,
    int lane) {
  const unsigned char* wr[ROWS];
  #pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    wr[r] = w + (long)row[r] * K;
    #pragma unroll
    for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
  }

  int kc = lane * 16;  // this lane's first k within a chunk
  for (; kc + FP8_CHUNK < K; kc += 2 * FP8_CHUNK) {  // 2 chunks
    uint4_v wf[ROWS][2];
    #pragma unroll
    for (int r = 0; r < ROWS; ++r)
      #pragma unroll
      for (int u = 0; u < 2; ++u)
        wf[r][u] = *(const uint4_v*)(wr[r] + kc + FP8_CHUNK * u);
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      ushort8 xf[M][2];
      load_x16<M>(xf, x, K, kc + FP8_CHUNK * u);
      #pragma unroll
      for (int r = 0; r < ROWS; ++r) mac16<M>(acc[r], wf[r][u], xf);
    }
  }
  for (; kc < K; kc += FP8_CHUNK) {  // 1-chunk tail
    uint4_v wf[ROWS];
    #pragma unroll
    for (int r = 0; r < ROWS; ++r)
      wf[r] = *(const uint4_v*)(wr[r] + kc);
    ushort8 xf[M][2];
    load_x16<M>(xf, x, K, kc);
    #pragma unroll
    for (int r = 0; r < ROWS; ++r) mac16<M>(acc[r], wf[r], xf);
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

// A wave whose rows all lie past N leaves before any load (no barrier in
// the kernel). A partial wave streams row N - 1 in place of each missing
// row, so that the load batch stays branch-free, and stores only its valid
// rows.
template <int M, int ROWS>
__global__ void __launch_bounds__(256)
gemv_fp8w_kernel(const unsigned short* __restrict__ x,  // [M, K] bf16
                 const unsigned char* __restrict__ w,   // [N, K] e4m3
                 const float* __restrict__ scale,       // [N]
                 unsigned short* __restrict__ out,      // [M, N] bf16
                 int N, int K) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  if (n0 >= N) return;

  int row[ROWS];
  #pragma unroll
  for (int r = 0; r < ROWS; ++r) row[r] = min(n0 + r, N - 1);
  float acc[ROWS][M];
  fp8_rows_dot<M, ROWS>(acc, x, w, row, K, lane);

  if (lane == 0) {
    #pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (n0 + r >= N) break;
      const float s = scale[n0 + r];
      #pragma unroll
      for (int m = 0; m < M; ++m)
        out[(long)m * N + n0 + r] = f32_to_bf16(acc[r][m] * s);
    }
  }
}

// Fused wgu GEMV + SwiGLU: w is the packed [gate; up] = [2I, K]. A wave
// owns two gate rows n0, n0 + 1 and their up rows n0 + I, n0 + 1 + I (the
// same four row streams per wave as the plain kernel) and writes
// silu(g) * u with g, u the scaled dot products.
template <int M>
__global__ void __launch_bounds__(256)
gemv_swiglu_fp8w_kernel(const unsigned short* __restrict__ x,  // [M, K]
                        const unsigned char* __restrict__ w,   // [2I, K]
                        const float* __restrict__ scale,       // [2I]
                        unsigned short* __restrict__ out,      // [M, I]
                        int I, int K) {
  constexpr int G = FP8_ROWS / 2;  // gate rows per wave
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * G;
  if (n0 >= I) return;

  int row[FP8_ROWS];  // gate rows first, then their up rows
  #pragma unroll
  for (int r = 0; r < G; ++r) {
    row[r] = min(n0 + r, I - 1);
    row[G + r] = row[r] + I;
  }
  float acc[FP8_ROWS][M];
  fp8_rows_dot<M, FP8_ROWS>(acc, x, w, row, K, lane);

  if (lane == 0) {
    #pragma unroll
    for (int r = 0; r < G; ++r) {
      if (n0 + r >= I) break;
      const float sg = scale[n0 + r], su = scale[n0 + r + I];
      #pragma unroll
      for (int m = 0; m < M; ++m) {
        const float g = acc[r][m] * sg, u = acc[G + r][m] * su;
        const float sig =
            1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * g));
        out[(long)m * I + n0 + r] = f32_to_bf16(g * sig * u);
      }
    }
  }
}

template <int ROWS>
static void gemv_fp8w_launch_rows(const void* x, const void* w,
                                  const void* scale, void* o, int M, int N,
                                  int K, hipStream_t stream) {
  const int blocks = (N + 4 * ROWS - 1) / (4 * ROWS);
  switch (M) {
    #define GF8_CASE(MM)                                                    \
      case MM:                                                              \
        hipLaunchKernelGGL((gemv_fp8w_kernel<MM, ROWS>), dim3(blocks),      \
                           dim3(256), 0, stream, (const unsigned short*)x,  \
                           (const unsigned char*)w, (const float*)scale,    \
                           (unsigned short*)o, N, K);                       \
        break;
    GF8_CASE(1) GF8_CASE(2) GF8_CASE(3) GF8_CASE(4)
    GF8_CASE(5) GF8_CASE(6) GF8_CASE(7) GF8_CASE(8)
    #undef GF8_CASE
    default: break;  // caller guards M <= 8
  }
}

extern "C" void gemv_fp8w_launch(const void* x, const void* w,
                                 const void* scale, void* o, int M, int N,
                                 int K, hipStream_t stream) {
  // 4 rows per wave leave N <= 8192 with at most 2 waves per SIMD, and at
  // K <= 8192 a wave runs at most 4 main-loop iterations: nothing hides
  // its start-up and drain. 2 rows per wave (64 B per lane in flight,
  // twice the waves) measured 15-45% faster there (wo, wqkv); long rows
  // (wdown, K = 14336) and large N keep 4.
  if (N <= 8192 && K <= 8192)
    gemv_fp8w_launch_rows<2>(x, w, scale, o, M, N, K, stream);
  else
    gemv_fp8w_launch_rows<FP8_ROWS>(x, w, scale, o, M, N, K, stream);
}

extern "C" void gemv_swiglu_fp8w_launch(const void* x, const void* w,
                                        const void* scale, void* o, int M,
                                        int I, int K, hipStream_t stream) {
  const int blocks = (I + 2 * FP8_ROWS - 1) / (2 * FP8_ROWS);
  switch (M) {
    #define GSF8_CASE(MM)                                                   \
      case MM:                                                              \
        hipLaunchKernelGGL((gemv_swiglu_fp8w_kernel<MM>), dim3(blocks),     \
                           dim3(256), 0, stream, (const unsigned short*)x,  \
                           (const unsigned char*)w, (const float*)scale,    \
                           (unsigned short*)o, I, K);                       \
        break;
    GSF8_CASE(1) GSF8_CASE(2) GSF8_CASE(3) GSF8_CASE(4)
    GSF8_CASE(5) GSF8_CASE(6) GSF8_CASE(7) GSF8_CASE(8)
    #undef GSF8_CASE
    default: break;
  }
}
