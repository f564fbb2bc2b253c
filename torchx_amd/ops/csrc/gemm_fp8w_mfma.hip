// W8A16 decode GEMM on the matrix cores, for 1 <= M <= 32 tokens: fp8 e4m3
// weights with one fp32 scale per output row, bf16 activations, bf16 output.
//
//   out[m, n] = bf16(scale[n] * sum_k x[m, k] * w8[n, k])
//
// with K % 1024 == 0 and w8 row-major [N, K] (OCP e4m3), the contract of
// gemv_fp8.hip. That kernel pays (1 + M) / 2 VALU ops per weight byte and
// is VALU-bound from M = 5; here the MACs go to v_mfma_f32_16x16x32_bf16
// and the VALU is left with the converts, 1 op per 2 weights whatever M is.
//
// Operand maps. In lane l, i = l & 15 and g = l >> 4. The weights are the A
// operand (16 rows x 32 k), x is B (32 k x 16 tokens), C is 16 rows x 16
// tokens: A holds row i at the instruction's k 8g .. 8g+7, B holds token i
// at the same k, C holds token i and rows 4g .. 4g+3 in registers 0 .. 3.
// The sum over k is order-free as long as A and B name the same k in the
// same slot, so which 8 k of memory a slot holds is free. Of a wave's 64 k
// per step, lane (i, g) feeds two MFMAs: half h takes k 32h + 8g .. + 7 of
// weight row i (8 B = 2 dwords) and of token i (16 B).
//
// Loads and the lane exchange. Loading those bytes straight into lane
// (i, g) puts 16 different rows into every 16 consecutive lanes, 8 or 16 B
// each. That form was built first and measured (profiles/README.md r13a):
// its time grew with the number of distinct x rows, 16.1 us at M = 9 to
// 32.8 us at M = 32 on wdown, the mark of a load path that pays per row
// touched, not per byte. So the loads are issued row-major instead: lane
// l = 4r + p loads row (or token) r, piece p, so that 4 consecutive lanes
// cover 32 contiguous weight bytes or 64 contiguous x bytes, and
// one ds_bpermute_b32 per dword (a register exchange through the LDS
// crossbar, no LDS memory) hands lane (i, g) the dword of lane 4i + g.
// Per half h: the weight load is 8 B at byte 32h + 8p of the wave's 64,
// the x load 16 B at element 32h + 8p. The same rows at M = 9 .. 32 then
// take 13.2 .. 17.2 us.
// Byte order is gemv_fp8.hip's: v_cvt_scalef32_pk_bf16_fp8 with sel = false
// gives bytes 0, 1 of a dword as (pair.x, pair.y), sel = true bytes 2, 3,
// so the two dwords become 8 consecutive k in order, the order of the x
// load. Every e4m3 value is exact in bf16 (scale operand 1.0), and the row
// scale is applied once to the finished fp32 sum.
//
// Work split. A 256-thread block owns RT tiles of 16 rows and its four
// waves split K: in each 256-element k step wave w takes [k + 64w, +64), so
// a wave covers 64 contiguous bytes of each of 16 rows and the block 256
// contiguous bytes per row. The loop takes 4 steps (1024 k, exact since
// K % 1024 == 0, no tail) and issues all 8 RT weight loads, 64 or 128 B per
// lane, before the first convert. A step's B fragments are loaded once and
// shared by the row tiles; MT token tiles of 16 reuse each converted A
// fragment. x comes from L2 at 2 MT / RT bytes per weight byte.
//
// Edges. Rows at or past N stream row N - 1, token columns at or past M
// read row M - 1 of x; neither is stored. MFMA column i of C depends on
// column i of B alone, so a padding column cannot reach a live one.
//
// Epilogue. Every wave writes its C registers to LDS, one __syncthreads,
// then the four partial sums are added in the fixed order wave 0, 1, 2, 3
// (no atomics: the result is the same on every run), scaled, put through
// SwiGLU where it applies, and stored as bf16.
// LDS layout: red[wave][tile][j][lane] fp32, tile = rt * MT + mt, j the C
// register: 4 * RT * MT * 4 * 64 * 4 B = 4 KiB .. 16 KiB. A wave's write of
// register j and the reducing wave's read of (wave, tile, j) both touch 64
// consecutive dwords, lane l at dword l: consecutive banks, conflict-free.
#include "common.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mbf16x8 __attribute__((ext_vector_type(8)));

constexpr int MF_STEP = 256;   // k per block step, 64 per wave
constexpr int MF_UNROLL = 4;   // steps per loop iteration: 1024 k

// dwords d0, d1 = 8 consecutive fp8 weights -> the 8 bf16 of an A operand
__device__ __forceinline__ mbf16x8 cvt8(unsigned d0, unsigned d1) {
  // the builtin wants sel as a literal
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
  mbf16x8 a;
  a[0] = p0[0]; a[1] = p0[1]; a[2] = p1[0]; a[3] = p1[1];
  a[4] = p2[0]; a[5] = p2[1]; a[6] = p3[0]; a[7] = p3[1];
  return a;
}

// SWIGLU = false: w is [N, K], the block owns rows n0 .. n0 + 16 RT - 1 and
// out is [M, N]. SWIGLU = true (RT = 2): w is the packed [gate; up] =
// [2N, K], tile 0 is the gate rows n0 .. n0 + 15 and tile 1 their up rows
// N + n0 .., out is [M, N]; g and u of one (token, row) land in the same
// lane and C register, so silu(g) * u needs no exchange.
template <int RT, int MT, bool SWIGLU>
__global__ void __launch_bounds__(256)
gemm_fp8w_mfma_kernel(const unsigned short* __restrict__ x,  // [M, K] bf16
                      const unsigned char* __restrict__ w,   // e4m3
                      const float* __restrict__ scale,
                      unsigned short* __restrict__ out,      // [M, N] bf16
                      int M, int N, int K) {
  static_assert(!SWIGLU || RT == 2, "SwiGLU pairs a gate and an up tile");
  constexpr int T = RT * MT;
  __shared__ float red[4 * T * 4 * 64];

  const int n0 = blockIdx.x * (SWIGLU ? 16 : 16 * RT);
  if (n0 >= N) return;  // the whole block, before any load and the barrier
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int i = lane & 15, g = lane >> 4;  // MFMA position
  const int r = lane >> 2, p = lane & 3;   // load position: row, piece
  const int pull = (4 * i + g) * 4;        // ds_bpermute address of lane 4i+g
  const int koff = 64 * wave + 8 * p;      // the lane's first k within a step

  const unsigned char* wr[RT];
  #pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int row = SWIGLU ? min(n0 + r, N - 1) + t * N
                           : min(n0 + 16 * t + r, N - 1);
    wr[t] = w + (long)row * K + koff;
  }
  const unsigned short* xr[MT];
  #pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xr[mt] = x + (long)min(16 * mt + r, M - 1) * K + koff;

  f32x4 acc[RT][MT];
  #pragma unroll
  for (int t = 0; t < RT; ++t)
    #pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k = 0; k < K; k += MF_UNROLL * MF_STEP) {
    uint2_v wf[RT][MF_UNROLL][2];
    #pragma unroll
    for (int t = 0; t < RT; ++t)
      #pragma unroll
      for (int s = 0; s < MF_UNROLL; ++s)
        #pragma unroll
        for (int h = 0; h < 2; ++h)
          wf[t][s][h] = *(const uint2_v*)(wr[t] + k + MF_STEP * s + 32 * h);
    #pragma unroll
    for (int s = 0; s < MF_UNROLL; ++s) {
      mbf16x8 xf[MT][2];
      #pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint4_v v = *(const uint4_v*)(xr[mt] + k + MF_STEP * s + 32 * h);
          #pragma unroll
          for (int c = 0; c < 4; ++c)
            v[c] = __builtin_amdgcn_ds_bpermute(pull, v[c]);
          xf[mt][h] = __builtin_bit_cast(mbf16x8, v);
        }
      #pragma unroll
      for (int t = 0; t < RT; ++t)
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
          const mbf16x8 a =
              cvt8(__builtin_amdgcn_ds_bpermute(pull, wf[t][s][h][0]),
                   __builtin_amdgcn_ds_bpermute(pull, wf[t][s][h][1]));
          #pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, xf[mt][h], acc[t][mt], 0, 0, 0);
        }
    }
  }

  #pragma unroll
  for (int t = 0; t < RT; ++t)
    #pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        red[((wave * T + t * MT + mt) * 4 + j) * 64 + lane] = acc[t][mt][j];
  __syncthreads();

  // sum of the four waves' partials of tile (t, mt), register j, this lane
  auto total = [&](int t, int mt, int j) {
    float v = red[((t * MT + mt) * 4 + j) * 64 + lane];
    #pragma unroll
    for (int wv = 1; wv < 4; ++wv)
      v += red[((wv * T + t * MT + mt) * 4 + j) * 64 + lane];
    return v;
  };

  // Wave-uniform split of the output tiles over the waves; the lane keeps
  // its C position: token 16 mt + i, rows nb .. nb + 3.
  constexpr int UNITS = SWIGLU ? MT : T;
  #pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    if ((u & 3) != wave) continue;
    const int t = SWIGLU ? 0 : u / MT, mt = SWIGLU ? u : u % MT;
    const int tok = 16 * mt + i;
    const int nb = n0 + 16 * t + 4 * g;
    if (tok >= M || nb >= N) continue;
    unsigned short o[4];
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = min(nb + j, N - 1);
      float v = total(t, mt, j) * scale[n];
      if (SWIGLU) {
        const float up = total(1, mt, j) * scale[N + n];
        const float sig =
            1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * v));
        v = v * sig * up;
      }
      o[j] = f32_to_bf16(v);
    }
    unsigned short* op = out + (long)tok * N + nb;
    if ((N & 3) == 0) {  // nb % 4 == 0: all four rows are live, 8-B aligned
      uint2_v pk;
      pk[0] = o[0] | ((unsigned)o[1] << 16);
      pk[1] = o[2] | ((unsigned)o[3] << 16);
      *(uint2_v*)op = pk;
    } else {
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        if (nb + j < N) op[j] = o[j];
    }
  }
}

template <int RT, int MT, bool SWIGLU>
static void mfma_launch(const void* x, const void* w, const void* scale,
                        void* o, int M, int N, int K, hipStream_t stream) {
  const int rows = SWIGLU ? 16 : 16 * RT;
  hipLaunchKernelGGL((gemm_fp8w_mfma_kernel<RT, MT, SWIGLU>),
                     dim3((N + rows - 1) / rows), dim3(256), 0, stream,
                     (const unsigned short*)x, (const unsigned char*)w,
                     (const float*)scale, (unsigned short*)o, M, N, K);
}

// rt = 1 or 2 forces the row-tile count (the probe's knob), 0 takes the
// rule below. The caller guards 1 <= M <= 32.
extern "C" void gemm_fp8w_mfma_launch(const void* x, const void* w,
                                      const void* scale, void* o, int M,
                                      int N, int K, int rt,
                                      hipStream_t stream) {
  // 2 row tiles halve the x reads per weight byte but leave N / 32 blocks:
  // 128 on 256 CUs at N = 4096, where 1 tile measured 30-35% faster (wo
  // 4.7 against 7.1 us, wdown 13.2 against 19.5 us at M = 9). At N = 6144
  // (wqkv, 192 blocks) 1 tile is 3-7% faster up to M = 16 (8.4 against
  // 8.9 us at M = 9) and 2 tiles 20% faster at M = 32 (9.2 against
  // 11.5 us), where MT = 2 doubles the x reads. Larger N fills the CUs
  // with either and takes 2, the shape of the SwiGLU kernel.
  if (rt == 0) rt = N <= 4096 || (N <= 8192 && M <= 16) ? 1 : 2;
  if (rt == 1) {
    if (M <= 16) mfma_launch<1, 1, false>(x, w, scale, o, M, N, K, stream);
    else mfma_launch<1, 2, false>(x, w, scale, o, M, N, K, stream);
  } else {
    if (M <= 16) mfma_launch<2, 1, false>(x, w, scale, o, M, N, K, stream);
    else mfma_launch<2, 2, false>(x, w, scale, o, M, N, K, stream);
  }
}

extern "C" void gemm_swiglu_fp8w_mfma_launch(const void* x, const void* w,
                                             const void* scale, void* o,
                                             int M, int I, int K,
                                             hipStream_t stream) {
  if (M <= 16) mfma_launch<2, 1, true>(x, w, scale, o, M, I, K, stream);
  else mfma_launch<2, 2, true>(x, w, scale, o, M, I, K, stream);
}
