// Fused MoE decode router: (residual add + RMSNorm +) gate GEMV + top-k +
// softmax in one dispatch, bf16 I/O, fp32 logits.
//
//   s = bf16(x + res), y = rmsnorm(s) * w           (NORM instances only)
//   l[e] = sum_i y[i] * wr[e, i]                    fp32, e < E <= 16
//   idx[0..k) = the k largest l, value descending, ties to the LOWER e
//   cw[j] = bf16(exp(l_j - l_0) / sum_j exp(l_j - l_0))
//
// One 256-thread block per token row with rmsnorm_res_fwd_kernel's
// thread->element map (thread t owns elements (it*256 + t)*8 .. +7), its
// expressions, block_reduce<4> and rsqrtf, so s and y are that kernel's
// bits. The dot products use the thread's own y elements after the bf16
// rounding (what a GEMM on y would read): the normed row makes no trip
// through memory or LDS between the norm and the routing.
//
// A thread's 16-byte pieces of wr[e] do not depend on x, so the first
// expert group's loads are issued at the top and land under the
// sum-of-squares reduction. Experts are taken in groups of G = 8 (H <=
// 4096) or 4, G * ITERS <= 16 loads and <= 64 VGPRs in flight: one group
// at E = 8, H = 4096.
//
// Per expert: fdot2 chain over it ascending, pairs ascending; 6-step wave
// butterfly; wave partials to LDS part[4][16]; lane e of wave 0 adds them
// in the order wave 0, 1, 2, 3. No atomics, nothing shared between rows: a
// row's result does not depend on the batch it is in.
//
// Top-k in wave 0 by lane exchange: lane e < E holds a 64-bit key
// (order-preserving image of the fp32 logit + 1) << 6 | (63 - e), all other
// lanes and already selected ones the dead key 0 (below every live key,
// -inf and NaN included); k rounds of a 16-lane butterfly max. A live key
// always exists while fewer than k <= E experts are taken, so the k results
// are distinct and in [0, E) for any input.
#include "common.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float route_dot2(ushort8 a, ushort8 b, float acc,
                                            int j2) {
  return __builtin_amdgcn_fdot2_f32_bf16(((const bf16x2*)&a)[j2],
                                         ((const bf16x2*)&b)[j2], acc,
                                         false);
}

// fp32 -> u32 whose unsigned order is the float order (-0 counts as +0)
__device__ __forceinline__ unsigned int route_ord(float f) {
  unsigned int u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float route_unord(unsigned int o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

template <int ITERS> struct RouteGroup {
  static constexpr int G = ITERS <= 2 ? 8 : 4;  // divides 16
};

template <int ITERS, bool NORM>
__global__ void __launch_bounds__(256)
moe_route_kernel(const unsigned short* __restrict__ x,    // NORM: [B, H]
                 const unsigned short* __restrict__ res,  // NORM: [B, H]/null
                 const unsigned short* __restrict__ w,    // NORM: [H]
                 const unsigned short* __restrict__ wr,   // [E, H]
                 unsigned short* __restrict__ s_out,      // NORM, res: [B, H]
                 unsigned short* __restrict__ y,  // NORM: out, else in [B, H]
                 long* __restrict__ idx,                  // [B, k]
                 unsigned short* __restrict__ cw,         // [B, k]
                 int H, int E, int k, float eps) {
  constexpr int G = RouteGroup<ITERS>::G;
  __shared__ float red[4];
  __shared__ float part[4][16];
  const long row = blockIdx.x;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  unsigned short* yr = y + row * (long)H;

  // the thread's pieces of the expert rows e0 .. e0+G-1. A group is taken
  // whole, without a branch per expert, so that its loads, dot chains and
  // butterflies interleave; a row past E-1 re-reads row E-1 (in bounds,
  // from cache) and its logit is never looked at.
  ushort8 wv[G][ITERS];
  auto load_group = [&](int e0) {
    #pragma unroll
    for (int g = 0; g < G; ++g) {
      const unsigned short* we = wr + (long)min(e0 + g, E - 1) * H;
      #pragma unroll
      for (int it = 0; it < ITERS; ++it)
        wv[g][it] = *(const ushort8*)(we + (it * 256 + threadIdx.x) * 8);
    }
  };
  load_group(0);

  ushort8 yv[ITERS];  // the thread's y elements, bf16
  if (NORM) {
    const unsigned short* xr = x + row * (long)H;
    float xs[ITERS][8];
    float acc = 0.f;
    #pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      int i = (it * 256 + threadIdx.x) * 8;
      ushort8 v = *(const ushort8*)(xr + i);
      ushort8 rv;
      if (res) rv = *(const ushort8*)(res + row * (long)H + i);
      ushort8 sv;
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_to_f32(v[j]);
        if (res) {
          f += bf16_to_f32(rv[j]);
          sv[j] = f32_to_bf16(f);
          f = bf16_to_f32(sv[j]);  // norm sees the bf16-rounded stream
        }
        xs[it][j] = f;
        acc = fmaf(f, f, acc);
      }
      if (res) *(ushort8*)(s_out + row * (long)H + i) = sv;
    }
    float total = block_reduce<4>(acc, red,
        [] __device__ (float a, float b) { return a + b; });
    float r = rsqrtf(total / (float)H + eps);

    #pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      int i = (it * 256 + threadIdx.x) * 8;
      ushort8 wn = *(const ushort8*)(w + i);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        yv[it][j] = f32_to_bf16(xs[it][j] * r * bf16_to_f32(wn[j]));
      }
      *(ushort8*)(yr + i) = yv[it];
    }
  } else {
    #pragma unroll
    for (int it = 0; it < ITERS; ++it)
      yv[it] = *(const ushort8*)(yr + (it * 256 + threadIdx.x) * 8);
  }

  // gate GEMV: this thread's share of every logit, wave-reduced
  for (int e0 = 0;;) {
    float a[G];
    #pragma unroll
    for (int g = 0; g < G; ++g) {
      a[g] = 0.f;
      #pragma unroll
      for (int it = 0; it < ITERS; ++it)
        #pragma unroll
        for (int j2 = 0; j2 < 4; ++j2)
          a[g] = route_dot2(yv[it], wv[g][it], a[g], j2);
    }
    #pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
      #pragma unroll
      for (int g = 0; g < G; ++g) a[g] += __shfl_xor(a[g], off, 64);
    if (lane == 0) {
      #pragma unroll
      for (int g = 0; g < G; ++g) part[wave][e0 + g] = a[g];  // e0+g <= 15
    }
    e0 += G;
    if (e0 >= E) break;
    load_group(e0);
  }
  __syncthreads();
  if (wave != 0) return;

  // wave 0: logits, k rounds of a 16-lane arg-max, softmax over the k
  unsigned long long key = 0ull;  // dead
  if (lane < E) {
    float l = part[0][lane];
    l += part[1][lane];
    l += part[2][lane];
    l += part[3][lane];
    key = (((unsigned long long)route_ord(l) + 1ull) << 6)
        | (unsigned long long)(63 - lane);
  }
  float l0 = 0.f, lj = 0.f;
  int ej = 0;
  for (int j = 0; j < k; ++j) {
    unsigned long long m = key;
    #pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
      unsigned long long o = __shfl_xor(m, off, 64);
      m = o > m ? o : m;
    }
    const int e = 63 - (int)(m & 63ull);
    const float l = route_unord((unsigned int)((m >> 6) - 1ull));
    if (j == 0) l0 = l;
    if (lane == j) { ej = e; lj = l; }
    if (lane == e) key = 0ull;
  }
  float p = lane < k ? expf(lj - l0) : 0.f;
  float sum = p;
  #pragma unroll
  for (int off = 4; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane < k) {
    idx[row * k + lane] = (long)ej;
    cw[row * k + lane] = f32_to_bf16(p / sum);
  }
}

// x/res/w/s_out null -> the norm-less instance (y is the input)
extern "C" void moe_route_launch(const void* x, const void* res,
                                 const void* w, const void* wr, void* s_out,
                                 void* y, void* idx, void* cw, long B, int H,
                                 int E, int k, float eps, bool norm,
                                 hipStream_t stream) {
  #define ROUTE_LAUNCH(N, NORM)                                              \
    hipLaunchKernelGGL((moe_route_kernel<N, NORM>), dim3(B), dim3(256), 0,   \
                       stream, (const unsigned short*)x,                     \
                       (const unsigned short*)res, (const unsigned short*)w, \
                       (const unsigned short*)wr, (unsigned short*)s_out,    \
                       (unsigned short*)y, (long*)idx, (unsigned short*)cw,  \
                       H, E, k, eps)
  #define ROUTE_CASE(N)                                                      \
    case N:                                                                  \
      if (norm) ROUTE_LAUNCH(N, true); else ROUTE_LAUNCH(N, false);          \
      break;
  switch (H / 2048) {
    ROUTE_CASE(1)
    ROUTE_CASE(2)
    ROUTE_CASE(3)
    ROUTE_CASE(4)
    default: break;  // binding guards H
  }
  #undef ROUTE_CASE
  #undef ROUTE_LAUNCH
}
