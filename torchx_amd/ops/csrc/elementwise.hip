// Element-wise hot ops: RoPE (fwd/bwd) and SwiGLU (fwd/bwd), bf16.
//
// Memory-bound: everything is vectorized (8 bf16 = 16 B per lane load) per
// the CDNA4 guide (scalar bf16 loads are ~2-2.5x slower).  RoPE uses
// host-precomputed f32 cos/sin tables (on-device trig would turn this
// VALU-bound).
//
// Replaces what the reference (meta-pytorch/torchx) delegates to stock
// PyTorch ops in its launched apps.
#include "common.h"

// ---------------------------------------------------------------------------
// RoPE, rotate-half (Llama) pairing: (i, i + D/2), D = head_dim.
// x: [rows, D] bf16 where rows = B*S*H, layout [B, S, H, D];
// cos/sin: [S, D/2] f32; pos_of_row = (row / H) % S.
// sign=+1 forward, -1 backward (inverse rotation).
// Each thread: 4 pairs (4 bf16 from each half = 8 B loads).
// ---------------------------------------------------------------------------
__global__ void rope_fwdbwd_kernel(
    const unsigned short* __restrict__ x,
    unsigned short* __restrict__ y,
    const float* __restrict__ cos_t,   // [S, D/2]
    const float* __restrict__ sin_t,   // [S, D/2]
    long np4,      // (rows * D/2) / 4
    int half_d,    // D/2, multiple of 4
    int heads,     // H
    int seq_len,   // S
    float sign) {
  typedef unsigned short us4 __attribute__((ext_vector_type(4)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  for (long p4 = grid_stride_begin(); p4 < np4; p4 += grid_stride()) {
    long p = p4 * 4;
    long row = p / half_d;
    int i = (int)(p % half_d);
    int pos = (int)((row / heads) % seq_len);
    const long base = row * (2L * half_d);
    us4 u1 = *(const us4*)(x + base + i);
    us4 u2 = *(const us4*)(x + base + half_d + i);
    f4 c = *(const f4*)(cos_t + (long)pos * half_d + i);
    f4 s = *(const f4*)(sin_t + (long)pos * half_d + i);
    us4 o1, o2;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x1 = bf16_to_f32(u1[j]);
      float x2 = bf16_to_f32(u2[j]);
      float y1 = fmaf(x1, c[j], -sign * s[j] * x2);
      float y2 = fmaf(x2, c[j], sign * s[j] * x1);
      o1[j] = f32_to_bf16(y1);
      o2[j] = f32_to_bf16(y2);
    }
    *(us4*)(y + base + i) = o1;
    *(us4*)(y + base + half_d + i) = o2;
  }
}

extern "C" void rope_launch(
    const void* x, void* y, const void* cos_t, const void* sin_t,
    long rows, int head_dim, int heads, int seq_len, float sign,
    hipStream_t stream) {
  const int half_d = head_dim / 2;
  const long np4 = rows * half_d / 4;
  const int block = 256;
  int grid = (int)((np4 + block - 1) / block);
  if (grid > 65535 * 8) grid = 65535 * 8;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rope_fwdbwd_kernel, dim3(grid), dim3(block), 0, stream,
                     (const unsigned short*)x, (unsigned short*)y,
                     (const float*)cos_t, (const float*)sin_t, np4, half_d,
                     heads, seq_len, sign);
}

// ---------------------------------------------------------------------------
// SwiGLU: out = silu(g) * u   (all bf16, flat n elements, n % 8 == 0)
// ---------------------------------------------------------------------------
__global__ void swiglu_fwd_kernel(
    const unsigned short* __restrict__ g,
    const unsigned short* __restrict__ u,
    unsigned short* __restrict__ out,
    long n8) {
  for (long i8 = grid_stride_begin(); i8 < n8; i8 += grid_stride()) {
    long i = i8 * 8;
    ushort8 gv = *(const ushort8*)(g + i);
    ushort8 uv = *(const ushort8*)(u + i);
    ushort8 ov;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gf = bf16_to_f32(gv[j]);
      float uf = bf16_to_f32(uv[j]);
      float sig =
          1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * gf));
      ov[j] = f32_to_bf16(gf * sig * uf);
    }
    *(ushort8*)(out + i) = ov;
  }
}

__global__ void swiglu_bwd_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ g,
    const unsigned short* __restrict__ u,
    unsigned short* __restrict__ dg,
    unsigned short* __restrict__ du,
    long n8) {
  for (long i8 = grid_stride_begin(); i8 < n8; i8 += grid_stride()) {
    long i = i8 * 8;
    ushort8 dov = *(const ushort8*)(dout + i);
    ushort8 gv = *(const ushort8*)(g + i);
    ushort8 uv = *(const ushort8*)(u + i);
    ushort8 dgv, duv;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float dof = bf16_to_f32(dov[j]);
      float gf = bf16_to_f32(gv[j]);
      float uf = bf16_to_f32(uv[j]);
      float sig =
          1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * gf));
      float silu = gf * sig;
      float dsilu = sig * (1.0f + gf * (1.0f - sig));
      dgv[j] = f32_to_bf16(dof * uf * dsilu);
      duv[j] = f32_to_bf16(dof * silu);
    }
    *(ushort8*)(dg + i) = dgv;
    *(ushort8*)(du + i) = duv;
  }
}

extern "C" void swiglu_fwd_launch(const void* g, const void* u, void* out,
                                  long n, hipStream_t stream) {
  const long n8 = n / 8;
  const int block = 256;
  long grid = (n8 + block - 1) / block;
  if (grid > 65535 * 8) grid = 65535 * 8;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3((int)grid), dim3(block), 0,
                     stream, (const unsigned short*)g,
                     (const unsigned short*)u, (unsigned short*)out, n8);
}

extern "C" void swiglu_bwd_launch(const void* dout, const void* g,
                                  const void* u, void* dg, void* du, long n,
                                  hipStream_t stream) {
  const long n8 = n / 8;
  const int block = 256;
  long grid = (n8 + block - 1) / block;
  if (grid > 65535 * 8) grid = 65535 * 8;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3((int)grid), dim3(block), 0,
                     stream, (const unsigned short*)dout,
                     (const unsigned short*)g, (const unsigned short*)u,
                     (unsigned short*)dg, (unsigned short*)du, n8);
}

// ---------------------------------------------------------------------------
// Strided in-place-capable RoPE over the fused qkv buffer: rows = B*S, each
// row is [q: Hq*128 | k: Hkv*128 | v: Hkv*128] at row_stride elements.
// Rotates the first (Hq+Hkv) heads; the v region is untouched (pass y == x
// for in-place, e.g. on the dqkv gradient buffer).
// ---------------------------------------------------------------------------
__global__ void rope_qkv_kernel(
    const unsigned short* __restrict__ x,
    unsigned short* __restrict__ y,
    const float* __restrict__ cos_t,   // [S, 64]
    const float* __restrict__ sin_t,
    long np4,        // rows * nh * 16  (4-pair groups, half_d = 64)
    int nh,          // Hq + Hkv
    long row_stride, // elements per row
    int seq_len,
    float sign) {
  typedef unsigned short us4 __attribute__((ext_vector_type(4)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int half_d = 64;
  // 2D grid: x covers (head, pair-group) with shifts/masks only, y strides
  // rows — the old flat grid-stride form paid a 64-bit div/mod (by nh=40,
  // not a power of two) on every thread
  const long hp4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (hp4 >= (long)nh * 16) return;
  const int h = (int)(hp4 >> 4);
  const int i = (int)(hp4 & 15) * 4;
  const long rows = np4 / ((long)nh * 16);
  for (long row = blockIdx.y; row < rows; row += gridDim.y) {
    const int pos = (int)(row % seq_len);
    const long base = row * row_stride + (long)h * 128;
    us4 u1 = *(const us4*)(x + base + i);
    us4 u2 = *(const us4*)(x + base + half_d + i);
    f4 c = *(const f4*)(cos_t + (long)pos * half_d + i);
    f4 s = *(const f4*)(sin_t + (long)pos * half_d + i);
    us4 o1, o2;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x1 = bf16_to_f32(u1[j]);
      float x2 = bf16_to_f32(u2[j]);
      o1[j] = f32_to_bf16(fmaf(x1, c[j], -sign * s[j] * x2));
      o2[j] = f32_to_bf16(fmaf(x2, c[j], sign * s[j] * x1));
    }
    *(us4*)(y + base + i) = o1;
    *(us4*)(y + base + half_d + i) = o2;
  }
}

extern "C" void rope_qkv_launch(
    const void* x, void* y, const void* cos_t, const void* sin_t,
    long rows, int nh, long row_stride, int seq_len, float sign,
    hipStream_t stream) {
  const long np4 = rows * nh * 16;
  const int block = 256;
  const int gx = (int)(((long)nh * 16 + block - 1) / block);
  const int gy = (int)((rows < 65535) ? (rows > 0 ? rows : 1) : 65535);
  hipLaunchKernelGGL(rope_qkv_kernel, dim3(gx, gy), dim3(block), 0,
                     stream, (const unsigned short*)x, (unsigned short*)y,
                     (const float*)cos_t, (const float*)sin_t, np4, nh,
                     row_stride, seq_len, sign);
}

// ---------------------------------------------------------------------------
// SwiGLU over the packed gate-up buffer gu = [rows, 2I]: out = silu(g)*u
// with g = gu[:, :I], u = gu[:, I:].  Avoids the two .contiguous() copies
// of the chunked views and the torch.cat in backward.
// ---------------------------------------------------------------------------
// 2D grid (cols x rows): the old 1D grid-stride form spent a 64-bit
// integer division (p / i8, i8 = I/8 = 1792 for llama) on EVERY thread —
// ~25% over the HBM roofline on a pure streaming kernel.
__global__ void swiglu_gu_fwd_kernel(
    const unsigned short* __restrict__ gu,
    unsigned short* __restrict__ out,
    long rows,
    long i8) {   // I / 8
  const long c8 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c8 >= i8) return;
  for (long row = blockIdx.y; row < rows; row += gridDim.y) {
    const long base = row * 2 * i8 * 8 + c8 * 8;
    ushort8 gv = *(const ushort8*)(gu + base);
    ushort8 uv = *(const ushort8*)(gu + base + i8 * 8);
    ushort8 ov;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gf = bf16_to_f32(gv[j]);
      float uf = bf16_to_f32(uv[j]);
      float sig =
          1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * gf));
      ov[j] = f32_to_bf16(gf * sig * uf);
    }
    *(ushort8*)(out + (row * i8 + c8) * 8) = ov;
  }
}

// dgate/dup of 8 packed elements: the per-element arithmetic of the packed
// SwiGLU backward, shared by the plain kernel and the one that also writes
// the transposed copy so that both produce the same bits.
__device__ __forceinline__ void swiglu_gu_bwd8(
    const ushort8& dov, const ushort8& gv, const ushort8& uv,
    ushort8& dgv, ushort8& duv) {
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    float dof = bf16_to_f32(dov[j]);
    float gf = bf16_to_f32(gv[j]);
    float uf = bf16_to_f32(uv[j]);
    float sig =
        1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504f * gf));
    float silu = gf * sig;
    dgv[j] = f32_to_bf16(dof * uf * sig * (1.0f + gf * (1.0f - sig)));
    duv[j] = f32_to_bf16(dof * silu);
  }
}

__global__ void swiglu_gu_bwd_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ gu,
    unsigned short* __restrict__ dgu,
    long rows, long i8) {
  const long c8 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c8 >= i8) return;
  for (long row = blockIdx.y; row < rows; row += gridDim.y) {
    const long base = row * 2 * i8 * 8 + c8 * 8;
    ushort8 dov = *(const ushort8*)(dout + (row * i8 + c8) * 8);
    ushort8 gv = *(const ushort8*)(gu + base);
    ushort8 uv = *(const ushort8*)(gu + base + i8 * 8);
    ushort8 dgv, duv;
    swiglu_gu_bwd8(dov, gv, uv, dgv, duv);
    *(ushort8*)(dgu + base) = dgv;
    *(ushort8*)(dgu + base + i8 * 8) = duv;
  }
}

extern "C" void swiglu_gu_fwd_launch(const void* gu, void* out, long rows,
                                     long I, hipStream_t stream) {
  const long i8 = I / 8;
  const int block = 256;
  const int gx = (int)((i8 + block - 1) / block);
  const int gy = (int)((rows < 65535) ? (rows > 0 ? rows : 1) : 65535);
  hipLaunchKernelGGL(swiglu_gu_fwd_kernel, dim3(gx, gy), dim3(block), 0,
                     stream, (const unsigned short*)gu, (unsigned short*)out,
                     rows, i8);
}

extern "C" void swiglu_gu_bwd_launch(const void* dout, const void* gu,
                                     void* dgu, long rows, long I,
                                     hipStream_t stream) {
  const long i8 = I / 8;
  const int block = 256;
  const int gx = (int)((i8 + block - 1) / block);
  const int gy = (int)((rows < 65535) ? (rows > 0 ? rows : 1) : 65535);
  hipLaunchKernelGGL(swiglu_gu_bwd_kernel, dim3(gx, gy), dim3(block), 0,
                     stream, (const unsigned short*)dout,
                     (const unsigned short*)gu, (unsigned short*)dgu, rows,
                     i8);
}

// ---------------------------------------------------------------------------
// bf16 2D transpose: in [R, C] -> out [C, R].  64x64 LDS tiles, 8-wide
// vector loads AND stores (both global streams coalesced; the strided
// direction goes through LDS).  Feeds the dgrad-NT path: dx = dy @ Wt^T
// runs ~15% faster than dy @ W on these shapes, and torch's strided copy
// for .t().contiguous() is several times slower than this.
// R, C must be multiples of 64 (all transformer weight dims are).
// ---------------------------------------------------------------------------
#define TP 64

// Block -> 64x64 tile for the kernels that write tiles transposed: TGROUP
// consecutive blocks take TGROUP consecutive row tiles of one column tile,
// then the next column tile of the same rows (the last group may be
// shorter).  The 128-B segments those blocks write to one output row then
// form a 4-KB run in flight together, and the next blocks read on along the
// same 2048 input rows.  Against column tiles fastest: swiglu_gu_bwd_t
// -15%; transpose_bf16 -4% to -9% on the activation and wqkv/wo/wgu
// shapes at 16384 tokens, +3% on wdown's [4096, 14336] (two groups only).
#define TGROUP 32

__device__ __forceinline__ void tile_of_block(int bid, int nrow, int ncol,
                                              int& rt, int& ct) {
  const int grp = bid / (TGROUP * ncol);
  const int rem = bid - grp * (TGROUP * ncol);
  const int glen = min(TGROUP, nrow - grp * TGROUP);
  rt = grp * TGROUP + rem % glen;
  ct = rem / glen;
}

__global__ void __launch_bounds__(256)
transpose_bf16_kernel(const unsigned short* __restrict__ in,
                      unsigned short* __restrict__ out, int R, int C) {
  // +1 short of row padding: store-pass lanes hit rows 8 apart, and
  // 8*(64+1) shorts staggers them 4 banks apart -> conflict-free
  // (any even padding aliases: 8*(64+p)*2B % 128B == 0 for p in {0,2,4,8})
  __shared__ unsigned short tile[TP][TP + 1];
  int rt, ct;
  tile_of_block((int)blockIdx.x, R / TP, C / TP, rt, ct);
  const int tile_r = rt * TP;  // input row of this tile
  const int tile_c = ct * TP;  // input col of this tile

  // load: 256 threads x 8 = 2048 elems/pass, 2 passes for 64x64
  #pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = pass * 2048 + threadIdx.x * 8;
    const int r = idx / TP;        // 0..63
    const int c = idx % TP;        // multiple of 8
    ushort8 v = *(const ushort8*)(in + (long)(tile_r + r) * C + tile_c + c);
    #pragma unroll
    for (int j = 0; j < 8; ++j) tile[r][c + j] = v[j];
  }
  __syncthreads();
  // store: thread writes out rows (= input cols) 8-wide
  #pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = pass * 2048 + threadIdx.x * 8;
    const int oc = idx / TP;       // output row = input col, 0..63
    const int orr = idx % TP;      // output col base = input row
    ushort8 v;
    #pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[orr + j][oc];
    *(ushort8*)(out + (long)(tile_c + oc) * R + tile_r + orr) = v;
  }
}

// ---------------------------------------------------------------------------
// Packed SwiGLU backward that also writes its result transposed:
// dgu [rows, 2I] as swiglu_gu_bwd_kernel (same bits), and dguT [2I, rows]
// = dgu^T, the operand the wgu wgrad wants (dW = dguT @ xT^T runs as a BLAS
// TN GEMM, both operands contiguous along the reduction dimension).  The
// stand-alone transpose would read dgu back (2I*rows*2 B); here the tile is
// still in registers.
//
// One block = 64 rows x 64 columns of I, gate and up halves both.  The
// natural rows go out as 16-B stores straight from registers (128-B
// segments per row and half).  The same values are parked in two LDS tiles
// laid out as transpose_bf16_kernel's, [64][64+1] shorts (16,640 B in all),
// and read back column-wise for the transposed 16-B stores (128-B segments
// per dguT row).
// Banks (32 dword banks for 2-byte accesses, conflicts per 32-lane half):
//  - park: a half covers 4 tile rows x 8 column groups; columns 8 apart are
//    4 banks apart, and the 65-short row pitch puts rows r and r+1 on the
//    same banks for even r (2 distinct dwords per bank: 2-way, which a
//    2-byte LDS store hides behind its own issue cycles) and rows r, r+2
//    one bank apart;
//  - read back: a half covers 4 adjacent columns x 8 row groups; rows 8
//    apart are 8*65 shorts = 260 dwords = 4 banks apart, adjacent columns
//    share a dword (broadcast) or sit on the next bank: conflict-free.
// Block order: tile_of_block's groups of 32 row tiles.  With column tiles
// fastest this kernel measured 0.74 ms at rows=16384, I=14336; grouped,
// 0.63 ms, which is the ~5.2 TB/s the plain swiglu_gu_bwd_kernel streams at
// (that kernel plus a stand-alone transpose: 0.87 ms).
// rows and I must be multiples of 64, (rows/64)*(I/64) < 2^31.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
swiglu_gu_bwd_t_kernel(const unsigned short* __restrict__ dout,
                       const unsigned short* __restrict__ gu,
                       unsigned short* __restrict__ dgu,
                       unsigned short* __restrict__ dguT,
                       long rows, long I) {
  __shared__ unsigned short tg[TP][TP + 1];
  __shared__ unsigned short tu[TP][TP + 1];
  int rt, ct;
  tile_of_block((int)blockIdx.x, (int)(rows / TP), (int)(I / TP), rt, ct);
  const long tile_r = (long)rt * TP;  // first row of this tile
  const long tile_c = (long)ct * TP;  // first column (within I)

  #pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = pass * 2048 + threadIdx.x * 8;
    const int r = idx / TP;        // 0..63
    const int c = idx % TP;        // multiple of 8
    const long row = tile_r + r;
    const long base = row * 2 * I + tile_c + c;
    ushort8 dov = *(const ushort8*)(dout + row * I + tile_c + c);
    ushort8 gv = *(const ushort8*)(gu + base);
    ushort8 uv = *(const ushort8*)(gu + base + I);
    ushort8 dgv, duv;
    swiglu_gu_bwd8(dov, gv, uv, dgv, duv);
    *(ushort8*)(dgu + base) = dgv;
    *(ushort8*)(dgu + base + I) = duv;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      tg[r][c + j] = dgv[j];
      tu[r][c + j] = duv[j];
    }
  }
  __syncthreads();
  #pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = pass * 2048 + threadIdx.x * 8;
    const int oc = idx / TP;       // dguT row within the tile = column
    const int orr = idx % TP;      // dguT column base = row
    ushort8 vg, vu;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      vg[j] = tg[orr + j][oc];
      vu[j] = tu[orr + j][oc];
    }
    const long o = (tile_c + oc) * rows + tile_r + orr;
    *(ushort8*)(dguT + o) = vg;
    *(ushort8*)(dguT + o + I * rows) = vu;
  }
}

extern "C" void swiglu_gu_bwd_t_launch(const void* dout, const void* gu,
                                       void* dgu, void* dguT, long rows,
                                       long I, hipStream_t stream) {
  hipLaunchKernelGGL(swiglu_gu_bwd_t_kernel,
                     dim3((unsigned)((I / TP) * (rows / TP))), dim3(256), 0,
                     stream, (const unsigned short*)dout,
                     (const unsigned short*)gu, (unsigned short*)dgu,
                     (unsigned short*)dguT, rows, I);
}

extern "C" void transpose_bf16_launch(const void* in, void* out, long R,
                                      long C, hipStream_t stream) {
  hipLaunchKernelGGL(transpose_bf16_kernel,
                     dim3((unsigned)((C / TP) * (R / TP))), dim3(256), 0,
                     stream, (const unsigned short*)in, (unsigned short*)out,
                     (int)R, (int)C);
}
