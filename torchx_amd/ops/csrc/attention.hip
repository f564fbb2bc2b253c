// Flash-style fused attention (forward + backward) for CDNA4 / gfx950.
//
// MFMA tiling with v_mfma_f32_32x32x16_bf16 (2xK gfx950 form), online
// softmax, causal masking, GQA.  Head dim fixed at 128 (Llama-3/Mixtral).
// Layouts are BSHD: q [B,S,Hq,128], k/v [B,S,Hkv,128], all bf16; lse/delta
// [B,Hq,S] f32.
//
// Design (the measured ladder is in profiles/README.md; idioms follow the
// CDNA4 guide's attention appendix):
//  * "swapped QK^T": S^T = mfma(A=K, B=Q) so each lane owns ONE q row's
//    scores -> softmax fully in-register (exp2 domain, v_cvt_pk_bf16_f32
//    fragment packing, defer-max rescale skip), one shfl_xor(32) partner
//    exchange, no cross-lane LDS reduction.
//  * KV tiles of 64 rows; K/V arrive by async global_load_lds into
//    XOR-swizzled natural images; the transposed operands (V^T / Q^T /
//    dO^T / K^T) are read straight off those images with hardware
//    transpose reads (nat_tr_frag), so no transposed image is built.
//  * T1 XCD swizzle: blocks streaming the same (batch, kv-head) tensors
//    land on one XCD so the stream is L2-resident (the kernels are
//    otherwise HBM-bound at ~128 FLOP/B).
//  * Forward block size is 4 waves at every length.
//  * paged_prefill_attn_kernel: the 4-wave forward over a block-table KV
//    cache, for a chunk of query rows behind an already cached prefix;
//    paged_prefill_attn_ragged_kernel: the same block work over a packed
//    batch of chunks of different lengths (host-built tile list).
//  * Backward is FA2-style without atomics: preprocess delta =
//    rowsum(dO*O); ONE dK+dV kernel, 4 waves at one wave per SIMD, in
//    which a wave accumulates both dK and dV for its 32 kv rows (S, P and
//    dP computed once) and exports the scaled bf16 dS (the 8-wave kernel
//    with separate dV / dK waves, which computes the same bits, remains
//    selectable); a dQ kernel (grid over q tiles) that is a streamed GEMM
//    dS.K over that export (the dQ kernel that recomputes dS itself
//    remains selectable).
//
// MFMA fragment maps used (verified against rocm CK xdlops_gemm.hpp and the
// CDNA4 guide; C/D map from the guide):
//   A[m=32, k=16]: lane l holds A[l&31][(l>>5)*8 + j], j=0..7  (bf16x8)
//   B[k=16, n=32]: lane l holds B[(l>>5)*8 + j][l&31]
//   C[m=32, n=32]: lane l holds C[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31], r=0..15
#include "common.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>

typedef __bf16 mbf16x8 __attribute__((ext_vector_type(8)));

#define HD 128           // head dim
#define QBLK 32          // q rows per wave
#define KBLK 32          // kv rows per tile
#define NWAVES 4         // waves per block
#define BLOCK_Q (QBLK * NWAVES)  // q rows per block (fwd / dq)
#define BLOCK_K (KBLK * NWAVES)  // kv rows per block (dkv)

__device__ __forceinline__ f32x16 mfma32(mbf16x8 a, mbf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// v_cvt_pk_bf16_f32: 2 f32 -> packed 2x bf16 (RNE) in ONE instruction
// (no builtin on gfx950 — guide T12 recipe; the manual RNE pack is ~6 VALU
// ops per value and dominated the softmax)
__device__ __forceinline__ unsigned int pack_bf16x2(float a, float b) {
  unsigned int r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// C-layout row index of accumulator register r for this lane-half.
__device__ __forceinline__ int c_row(int r, int half) {
  return (r & 3) + 8 * (r >> 2) + 4 * half;
}

// Build the two k-slice MFMA fragments (slice s covers k in [16s, 16s+16))
// from 16 f32 values held in C-layout.  Lane-half exchange via shfl_xor(32).
__device__ __forceinline__ void cvals_to_frags(const float* p, bool hi,
                                               mbf16x8* f0, mbf16x8* f1) {
  unsigned int w[2][4];
  #pragma unroll
  for (int s = 0; s < 2; ++s) {
    unsigned int a01 = pack_bf16x2(p[8 * s + 0], p[8 * s + 1]);
    unsigned int a23 = pack_bf16x2(p[8 * s + 2], p[8 * s + 3]);
    unsigned int a45 = pack_bf16x2(p[8 * s + 4], p[8 * s + 5]);
    unsigned int a67 = pack_bf16x2(p[8 * s + 6], p[8 * s + 7]);
    unsigned int x01 = __shfl_xor((int)a01, 32, 64);
    unsigned int x23 = __shfl_xor((int)a23, 32, 64);
    unsigned int x45 = __shfl_xor((int)a45, 32, 64);
    unsigned int x67 = __shfl_xor((int)a67, 32, 64);
    w[s][0] = hi ? x45 : a01;
    w[s][1] = hi ? x67 : a23;
    w[s][2] = hi ? a45 : x01;
    w[s][3] = hi ? a67 : x23;
  }
  uint4_v u0 = {w[0][0], w[0][1], w[0][2], w[0][3]};
  uint4_v u1 = {w[1][0], w[1][1], w[1][2], w[1][3]};
  *f0 = __builtin_bit_cast(mbf16x8, u0);
  *f1 = __builtin_bit_cast(mbf16x8, u1);
}

// ---------------------------------------------------------------------------
// Forward v2 (guide Appendix B ladder): KVBLK=64, double-buffered K tiles
// arriving by async global_load_lds into an XOR-swizzled LDS image (T2+T3),
// V reg-staged and transposed AFTER the barrier (T14 async-STAGE split),
// exp2-domain online softmax (v_exp_f32 native).
// ---------------------------------------------------------------------------

#define FKV 64                      // kv rows per staged tile
#define KIMG_BYTES (FKV * 256)      // [64 rows][256 B], byte ^= (row&15)<<4
#define LOG2E 1.44269504088896340736f
#define LN2 0.69314718055994530942f

// K fragment from the swizzled K image: row k = sub*32 + (lane&31),
// d-slice c -> 16 B at [32c + (lane>>5)*16] ^ swizzle.
__device__ __forceinline__ mbf16x8 kimg_frag(const char* kimg, int sub, int c) {
  const int lane = threadIdx.x & 63;
  const int row = sub * 32 + (lane & 31);
  const int byte = (c * 32 + ((lane >> 5) * 16)) ^ ((row & 15) << 4);
  return *(const mbf16x8*)(kimg + row * 256 + byte);
}

// ---------------------------------------------------------------------------
// T10 hardware transpose read: assemble the MFMA fragment of the
// TRANSPOSED tile — lane holds 8 elements (rows ks*16+(lane>>5)*8+j
// of the NATURAL 64-row image, at its own column dt*32+(lane&31)) — with
// two ds_read_tr16_b64 per fragment, straight off the XOR-swizzled natural
// image, so no kernel builds a transposed LDS image.  Per-16-lane-cluster
// semantics (probe-verified, tools/probe_tr_read.py): lane j addresses the
// 4-bf16 chunk
// (row r0 + (j>>2), cols cbase + 4*(j&3)); lane i receives the 4 rows at
// column cbase + i, packed low-to-high.
// ---------------------------------------------------------------------------
typedef short short4_v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) short4_v* lds_s4p;

__device__ __forceinline__ mbf16x8 nat_tr_frag(const char* nat, int ks,
                                               int dt) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 15;
  const int r_lo = ks * 16 + ((lane >> 5) * 8) + (j >> 2);
  const int r_hi = r_lo + 4;
  const int d0 = dt * 32 + ((lane >> 4) & 1) * 16 + 4 * (j & 3);
  const int g16 = (d0 >> 3) << 4;
  const int off = (d0 & 7) * 2;
  const int b_lo = r_lo * 256 + ((g16 ^ ((r_lo & 15) << 4)) | off);
  const int b_hi = r_hi * 256 + ((g16 ^ ((r_hi & 15) << 4)) | off);
  short4_v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s4p)(nat + b_lo));
  short4_v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s4p)(nat + b_hi));
  uint2_v ul = __builtin_bit_cast(uint2_v, lo);
  uint2_v uh = __builtin_bit_cast(uint2_v, hi);
  uint4_v u = {ul[0], ul[1], uh[0], uh[1]};
  return __builtin_bit_cast(mbf16x8, u);
}

// Async-stage one 64-row K tile: 16 global_load_lds_dwordx4 per block
// (16/NW per wave), source-permuted so the lane-linear LDS image lands
// swizzled (T2 note: swizzle moves to the SOURCE with glds staging).
// Rows beyond S clamp to S-1 (values masked in softmax).
template <int NW = 4, int TFKV = FKV>
__device__ __forceinline__ void stage_k_glds(
    const unsigned short* __restrict__ kb, long kv0, long stride_elems,
    int S, char* kimg) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  #pragma unroll
  for (int j = 0; j < (TFKV / 4) / NW; ++j) {
    const int i = wave * ((TFKV / 4) / NW) + j;
    const int row = i * 4 + (lane >> 4);
    const int colbyte = ((lane & 15) * 16) ^ ((row & 15) << 4);
    long srow = kv0 + row;
    if (srow >= S) srow = S - 1;
    const char* src = (const char*)(kb + srow * stride_elems) + colbyte;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(kimg + i * 1024),
        16, 0, 0);
  }
}

// stage_k_glds with (wave, lane) as parameters, so that a caller can hand in
// an opaque copy of the lane id and keep the per-piece lane constants out of
// its loop-carried registers.
template <int NW = 4, int TFKV = FKV>
__device__ __forceinline__ void stage_k_glds_at(
    const unsigned short* __restrict__ kb, long kv0, long stride_elems,
    int S, char* kimg, int wave, int lane) {
  #pragma unroll
  for (int j = 0; j < (TFKV / 4) / NW; ++j) {
    const int i = wave * ((TFKV / 4) / NW) + j;
    const int row = i * 4 + (lane >> 4);
    const int colbyte = ((lane & 15) * 16) ^ ((row & 15) << 4);
    long srow = kv0 + row;
    if (srow >= S) srow = S - 1;
    const char* src = (const char*)(kb + srow * stride_elems) + colbyte;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(kimg + i * 1024),
        16, 0, 0);
  }
}


// T1 XCD-aware block swizzle: the dispatcher hands consecutive blockIdx to
// consecutive XCDs (each with its own 4 MB L2).  Group the G*nqt blocks
// that read the same (b, hkv) K/V stream onto ONE XCD so K/V go L2-resident
// after the first touch (these kernels are otherwise HBM-bound at
// AI ~= 128 FLOP/B).  Falls back to the linear map when B*Hkv % 8 != 0.
__device__ __forceinline__ void map_block_fwd(int B, int Hq, int Hkv,
                                              int nqt, int G,
                                              int* b, int* hq, int* qt) {
  int bid = blockIdx.x;
  if (((B * Hkv) & 7) == 0) {
    const int gsz = G * nqt;
    const int xcd = bid & 7, slot = bid >> 3;
    const int g = (slot / gsz) * 8 + xcd;
    *b = g / Hkv;
    const int r = slot % gsz;
    *hq = (g % Hkv) * G + r / nqt;
    *qt = r % nqt;
  } else {
    *b = bid / (Hq * nqt);
    bid -= *b * Hq * nqt;
    *hq = bid / nqt;
    *qt = bid % nqt;
  }
}

// Balanced map of the dense forward (attn_fwd_kernel; the dQ kernels keep
// map_block_fwd).  Under the causal mask q tile qt costs ~qt+1 units, and
// map_block_fwd walks each head with qt ascending, so an XCD's last
// dispatched blocks are its heaviest and the kernel ends on their tail.
//
// A unit is a (b, kv head, q tile) and owns G = Hq / Hkv blocks, one per q
// head of the group; with xcd = bid & 7, slot = bid >> 3 the blocks of a
// unit are adjacent in dispatch order and sit on one XCD.
//   B*Hkv % 8 == 0: XCD x owns the ns = B*Hkv/8 streams x, x+8, ... — the
//     streams map_block_fwd gives it, so a K/V stream still lives in one
//     L2.  Its unit u = slot / G is stream u % ns at tile u / ns counted
//     from the heaviest end: tiles descend, interleaved over the XCD's
//     streams.  The grid is exactly B*Hq*nqt.
//   otherwise: unit = (slot / G) * 8 + xcd over all B*Hkv*nqt units, tile
//     unit / (B*Hkv) from the heaviest end, stream unit % (B*Hkv); the grid
//     is rounded up to whole rounds of 8 units (attn_fwd_launch) and a block
//     of a unit past the end returns false: it must leave before any
//     barrier.
// heavy = 0 keeps the unit layout with tiles ascending (A/B of the two
// steps).  Every (b, hq, qt) is produced exactly once for every shape.
__device__ __forceinline__ bool map_block_fwd_balanced(int B, int Hq, int Hkv,
                                                       int nqt, int G,
                                                       int heavy, int* b,
                                                       int* hq, int* qt) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int u = slot / G;
  const int nstream = B * Hkv;
  int g, t;
  if ((nstream & 7) == 0) {
    const int ns = nstream >> 3;
    g = (u % ns) * 8 + xcd;
    t = u / ns;
  } else {
    const int unit = u * 8 + xcd;
    if (unit >= nstream * nqt) return false;
    g = unit % nstream;
    t = unit / nstream;
  }
  *b = g / Hkv;
  *hq = (g % Hkv) * G + slot % G;
  *qt = heavy ? nqt - 1 - t : t;
  return true;
}

// Forward O epilogue: normalise this lane's q row of O^T and store it as
// bf16 at `ob` (the row's d = 0), 8 bytes per store.
__device__ __forceinline__ void fwd_store_o(const f32x16 (&acc_o)[4],
                                            float l_run, bool hi,
                                            unsigned short* ob) {
  const float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
  #pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    #pragma unroll
    for (int g = 0; g < 4; ++g) {
      // regs 4g..4g+3 are consecutive d: d = dt*32 + 8g + 4*hi + (0..3)
      bf16x4_raw w;
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = (short)f32_to_bf16(acc_o[dt][4 * g + j] * inv_l);
      }
      *(bf16x4_raw*)(ob + dt * 32 + 8 * g + 4 * (hi ? 1 : 0)) = w;
    }
  }
}

__global__ void __launch_bounds__(256, 2)
attn_fwd_kernel(const unsigned short* __restrict__ q,
                const unsigned short* __restrict__ k,
                const unsigned short* __restrict__ v,
                unsigned short* __restrict__ o,
                float* __restrict__ lse,  // [B,Hq,S]
                int B, int S, int Hq, int Hkv, float scale, int causal,
                long q_rs, long kv_rs,    // per-seq-row element strides
                int map) {  // 0 map_block_fwd, 1 balanced, 2 adjacent
  // K and V natural 2-rings (glds); the PV A-operand (V^T) is read off
  // the natural V image with hardware transpose reads (T10) — no V^T
  // build, 64 KiB LDS -> true 2 blocks/CU.
  __shared__ __align__(16) char smem[4 * KIMG_BYTES];

  const int BQ = BLOCK_Q;
  const int nqt = (S + BQ - 1) / BQ;
  const int G = Hq / Hkv;
  int b, hq, qt;
  if (map == 0) {
    map_block_fwd(B, Hq, Hkv, nqt, G, &b, &hq, &qt);
  } else if (!map_block_fwd_balanced(B, Hq, Hkv, nqt, G, map == 1, &b, &hq,
                                     &qt)) {
    return;  // block-uniform: a padding unit of the rounded-up grid
  }
  const int hkv = hq / G;

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const bool hi = lane >= 32;
  const int qr = lane & 31;

  const long q_seq_stride = q_rs;
  const long kv_seq_stride = kv_rs;
  const unsigned short* qb = q + (long)b * S * q_seq_stride + (long)hq * HD;
  const unsigned short* kb = k + (long)b * S * kv_seq_stride + (long)hkv * HD;
  const unsigned short* vb = v + (long)b * S * kv_seq_stride + (long)hkv * HD;

  const int q0_blk = qt * BQ;
  const int qw0 = q0_blk + wave * QBLK;       // wave's first q row
  const long q_row = qw0 + qr;                 // this lane's q row
  const bool wave_active = qw0 < S;

  // Q fragments in registers: chunk c covers d in [16c, 16c+16)
  mbf16x8 qfrag[8];
  {
    const long row = (q_row < S) ? q_row : (S - 1);
    const unsigned short* qp = qb + row * q_seq_stride + (hi ? 8 : 0);
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      qfrag[c] = __builtin_bit_cast(mbf16x8, *(const ushort8*)(qp + c * 16));
    }
  }

  f32x16 acc_o[4] = {};
  float m_run = -3.0e38f, l_run = 0.f;   // m in exp2 domain
  const float sc2 = scale * LOG2E;

  const int kv_limit = causal ? min(S, q0_blk + BQ) : S;
  const int ntiles = (kv_limit + FKV - 1) / FKV;
  const int qw_max = min(qw0 + QBLK - 1, S - 1);

  char* k0 = smem;                       // K tile t   (cur)
  char* k1 = smem + KIMG_BYTES;          // K tile t+1 (in flight)
  char* vcur = smem + 2 * KIMG_BYTES;    // V natural cur
  char* vnxt = smem + 3 * KIMG_BYTES;    // V natural nxt

  // prologue: glds K0 + V0 natural
  stage_k_glds<4>(kb, 0, kv_seq_stride, S, k0);
  stage_k_glds<4>(vb, 0, kv_seq_stride, S, vcur);
  asm volatile("s_waitcnt vmcnt(0)");
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * FKV;
    const bool has_next = (t + 1) < ntiles;
    if (has_next) {
      // issue next K/V glds BEFORE compute (T14: their latency hides
      // under this tile's MFMAs; the stream is L2-resident anyway)
      stage_k_glds<4>(kb, kv0 + FKV, kv_seq_stride, S, k1);
      stage_k_glds<4>(vb, kv0 + FKV, kv_seq_stride, S, vnxt);
    }

    const bool needed = wave_active && (!causal || kv0 <= qw_max);
    if (needed) {
      // S^T[k, q] = K . Q^T over both 32-row k sub-tiles (T5: setprio
      // keeps the MFMA pipe fed while the other wave issues memory ops)
      f32x16 acc0 = {}, acc1 = {};
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int c = 0; c < 8; ++c) {
        acc0 = mfma32(kimg_frag(k0, 0, c), qfrag[c], acc0);
        acc1 = mfma32(kimg_frag(k0, 1, c), qfrag[c], acc1);
      }
      __builtin_amdgcn_s_setprio(0);

      float sv[32];
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv[r] = acc0[r] * sc2;
        sv[16 + r] = acc1[r] * sc2;
      }
      const bool mask_tile =
          (causal && kv0 + FKV - 1 > qw0) || (kv0 + FKV > S) || (q_row >= S);
      if (mask_tile) {
        #pragma unroll
        for (int r = 0; r < 32; ++r) {
          const long kg = kv0 + (r >> 4) * 32 + c_row(r & 15, hi);
          if (kg >= S || q_row >= S || (causal && kg > q_row)) {
            sv[r] = -3.0e38f;
          }
        }
      }

      // online softmax, exp2 domain (lane owns q row; partner lane+32
      // holds the other 16 k's of each sub-tile).  T13 defer-max: skip the
      // O-wide rescale while per-tile max growth stays under THR2
      // (P bounded by 2^THR2 ~= e^8, bf16-accum tolerates; the previous
      // tile's PV is complete before this decision — the safe order).
      float m_tile = sv[0];
      #pragma unroll
      for (int r = 1; r < 32; ++r) m_tile = fmaxf(m_tile, sv[r]);
      m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32, 64));
      const float THR2 = 11.54f;  // 8 * log2(e)
      if (!__all(m_tile - m_run <= THR2)) {
        const float m_new = fmaxf(m_run, m_tile);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
        m_run = m_new;
        #pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          #pragma unroll
          for (int r = 0; r < 16; ++r) acc_o[dt][r] *= alpha;
        }
      }

      float row_sum = 0.f;
      #pragma unroll
      for (int r = 0; r < 32; ++r) {
        sv[r] = __builtin_amdgcn_exp2f(sv[r] - m_run);  // sv becomes P
        row_sum += sv[r];
      }
      row_sum += __shfl_xor(row_sum, 32, 64);
      l_run += row_sum;

      mbf16x8 pf[4];
      cvals_to_frags(sv, hi, &pf[0], &pf[1]);
      cvals_to_frags(sv + 16, hi, &pf[2], &pf[3]);

      // O^T[d, q] += V^T . P  (A = V^T by hardware transpose read off
      // the natural V image, T10)
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          acc_o[dt] = mfma32(nat_tr_frag(vcur, ks, dt), pf[ks], acc_o[dt]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (has_next) {
      asm volatile("s_waitcnt vmcnt(0)");  // own K/V glds landed
      __syncthreads();   // everyone done reading cur; nxt visible
      char* tk = k0; k0 = k1; k1 = tk;
      char* tv = vcur; vcur = vnxt; vnxt = tv;
    }
  }

  if (!wave_active || q_row >= S) return;

  fwd_store_o(acc_o, l_run, hi, o + (((long)b * S + q_row) * Hq + hq) * HD);
  if (!hi) {
    // lse stays in the natural-log domain for the backward kernels
    lse[((long)b * Hq + hq) * S + q_row] = (m_run + __log2f(l_run)) * LN2;
  }
}

// ---------------------------------------------------------------------------
// Paged prefill: a chunk of S query rows at logical positions
// ctx[b] .. ctx[b]+S-1 over a block-table KV cache that already holds
// L = ctx[b] + S rows (the chunk's own K/V are stored before the launch).
//
//   q            [B, S, Hq, 128] bf16
//   kpool/vpool  [num_pages, P, Hkv, 128] bf16, P a power of two, 16..256
//   bt           int32 [B, M]; logical row t of sequence b is
//                pool[bt[b][t / P]][t % P][hkv][:]
//   ctx          int32 [B]
//   o            [B, S, Hq, 128] bf16       (no lse: inference only)
//
// This is attn_fwd_kernel (causal) with two changes. (1) The staging
// source row goes through the table. A wave stages the 16 consecutive,
// 16-aligned logical rows [kv0 + 16w, +16) of a tile, which lie in ONE
// page for every P >= 16, so a tile costs each lane one table entry; rows
// at or past L read row L-1 (as the dense kernel clamps to S-1) through
// the entry of page (L-1)/P fetched once. The entry for the tile after
// next is fetched while the next tile's loads are issued, so no K/V load
// waits on a table load of its own iteration. (2) The causal diagonal is
// shifted by ctx: q row i sees keys t <= ctx + i.
//
// The LDS images, the tile sequence, the MFMA order and the softmax are
// the dense kernel's expressions in the dense kernel's order. Hence, for
// ctx[b] % 128 == 0, row i of the output is bit-identical to row
// ctx[b] + i of attn_fwd_kernel (causal) over the gathered dense
// sequence of length ctx[b] + S: the block holds the same 128 q rows, its
// waves the same 32, and every wave walks the same tiles. For any other
// ctx the grouping of q rows into waves differs, the __all of the
// defer-max decision sees other rows, and only the tolerance against an
// fp32 reference holds.
//
// No table or ctx content can address outside the pools or the table:
// ctx is clamped to [0, M*P] and L to [1, M*P], table indices are taken
// from rows < L (so < M), every entry read is clamped to [0, num_pages),
// and pool offsets are 64-bit.
// ---------------------------------------------------------------------------

// Table entry of the page holding the wave's 16-row staging group of the
// tile at kv0 (the row is clamped into the sequence, so the index is < M).
// The raw entry is carried to the iteration that uses it and clamped
// there (paged_page_base), so nothing waits on this load where it issues.
__device__ __forceinline__ int paged_group_entry(
    const int* __restrict__ bt_row, int kv0, int L, int logP) {
  const int wave = threadIdx.x / 64;
  const int g0 = min(kv0 + wave * (FKV / 4), L - 1);
  return bt_row[g0 >> logP];
}

// Physical first row of a page, the table entry clamped to [0, num_pages).
__device__ __forceinline__ long paged_page_base(int entry, int num_pages,
                                                int logP) {
  return (long)min(max(entry, 0), num_pages - 1) << logP;
}

// stage_k_glds<4> with the source row looked up: same lane -> (row,
// colbyte) map, same LDS image.  `pb` points at this kv head's column of
// pool row 0; `grp_base` is the page base of this tile's group, `last_row`
// the physical row of logical row L-1.
__device__ __forceinline__ void stage_paged_glds(
    const unsigned short* __restrict__ pb, int kv0, long stride_elems,
    int L, int pmask, long grp_base, long last_row, char* img) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  #pragma unroll
  for (int j = 0; j < (FKV / 4) / 4; ++j) {
    const int i = wave * ((FKV / 4) / 4) + j;
    const int row = i * 4 + (lane >> 4);
    const int colbyte = ((lane & 15) * 16) ^ ((row & 15) << 4);
    const int t = kv0 + row;
    long srow = grp_base + (t & pmask);
    if (t >= L) srow = last_row;
    const char* src = (const char*)(pb + srow * stride_elems) + colbyte;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(img + i * 1024),
        16, 0, 0);
  }
}

// One block's work, shared by the [B, S] kernel and the ragged one: q tile
// `qt` (128 rows) of one (sequence, q head). `qb` / `ob` point at the
// sequence's first chunk row of that head, `kb` / `vb` at the kv head's
// column of pool row 0, `bt_row` at the sequence's table row; the chunk
// has S rows behind `ctx_b` cached ones. All four waves run every barrier.
__device__ __forceinline__ void paged_prefill_tile(
    const unsigned short* __restrict__ qb,
    const unsigned short* __restrict__ kb,
    const unsigned short* __restrict__ vb,
    unsigned short* __restrict__ ob,
    const int* __restrict__ bt_row, int ctx_b, int S, int qt, int Hq,
    int Hkv, int num_pages, int logP, int M, float scale, char* smem) {
  const int BQ = 4 * QBLK;

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const bool hi = lane >= 32;
  const int qr = lane & 31;

  // cached rows before the chunk, and the sequence length; compare before
  // adding so a garbage ctx cannot overflow
  const int cap = M << logP;
  const int c0 = min(max(ctx_b, 0), cap);
  const int L = (S > cap - c0) ? cap : c0 + S;
  const int pmask = (1 << logP) - 1;

  const long q_seq_stride = (long)Hq * HD;
  const long kv_seq_stride = (long)Hkv * HD;

  const int q0_blk = qt * BQ;
  const int qw0 = q0_blk + wave * QBLK;       // wave's first q row
  const long q_row = qw0 + qr;                 // this lane's q row
  const bool wave_active = qw0 < S;

  // Q fragments in registers: chunk c covers d in [16c, 16c+16)
  mbf16x8 qfrag[8];
  {
    const long row = (q_row < S) ? q_row : (S - 1);
    const unsigned short* qp = qb + row * q_seq_stride + (hi ? 8 : 0);
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      qfrag[c] = __builtin_bit_cast(mbf16x8, *(const ushort8*)(qp + c * 16));
    }
  }

  f32x16 acc_o[4] = {};
  float m_run = -3.0e38f, l_run = 0.f;   // m in exp2 domain
  const float sc2 = scale * LOG2E;

  const int kv_limit = min(L, c0 + q0_blk + BQ);
  const int ntiles = (kv_limit + FKV - 1) / FKV;
  const int qw_max = min(qw0 + QBLK - 1, S - 1);

  char* k0 = smem;                       // K tile t   (cur)
  char* k1 = smem + KIMG_BYTES;          // K tile t+1 (in flight)
  char* vcur = smem + 2 * KIMG_BYTES;    // V natural cur
  char* vnxt = smem + 3 * KIMG_BYTES;    // V natural nxt

  // physical row of logical row L-1 (where rows past the end read)
  const long last_row =
      paged_page_base(bt_row[(L - 1) >> logP], num_pages, logP) +
      ((L - 1) & pmask);

  // prologue: glds K0 + V0 natural; table entry of tile 1
  int ent_nxt = paged_group_entry(bt_row, FKV, L, logP);
  {
    const long base0 = paged_page_base(
        paged_group_entry(bt_row, 0, L, logP), num_pages, logP);
    stage_paged_glds(kb, 0, kv_seq_stride, L, pmask, base0, last_row, k0);
    stage_paged_glds(vb, 0, kv_seq_stride, L, pmask, base0, last_row, vcur);
  }
  asm volatile("s_waitcnt vmcnt(0)");
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * FKV;
    const bool has_next = (t + 1) < ntiles;
    if (has_next) {
      // issue next K/V glds BEFORE compute (T14), through the entry
      // fetched one iteration ago; the entry of tile t+2 goes out with
      // them and is first looked at in the next iteration
      const long base = paged_page_base(ent_nxt, num_pages, logP);
      ent_nxt = paged_group_entry(bt_row, kv0 + 2 * FKV, L, logP);
      stage_paged_glds(kb, kv0 + FKV, kv_seq_stride, L, pmask, base,
                       last_row, k1);
      stage_paged_glds(vb, kv0 + FKV, kv_seq_stride, L, pmask, base,
                       last_row, vnxt);
    }

    const bool needed = wave_active && (kv0 <= c0 + qw_max);
    if (needed) {
      // S^T[k, q] = K . Q^T over both 32-row k sub-tiles (T5)
      f32x16 acc0 = {}, acc1 = {};
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int c = 0; c < 8; ++c) {
        acc0 = mfma32(kimg_frag(k0, 0, c), qfrag[c], acc0);
        acc1 = mfma32(kimg_frag(k0, 1, c), qfrag[c], acc1);
      }
      __builtin_amdgcn_s_setprio(0);

      float sv[32];
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv[r] = acc0[r] * sc2;
        sv[16 + r] = acc1[r] * sc2;
      }
      const bool mask_tile =
          (kv0 + FKV - 1 > c0 + qw0) || (kv0 + FKV > L) || (q_row >= S);
      if (mask_tile) {
        #pragma unroll
        for (int r = 0; r < 32; ++r) {
          const long kg = kv0 + (r >> 4) * 32 + c_row(r & 15, hi);
          if (kg >= L || q_row >= S || kg > c0 + q_row) {
            sv[r] = -3.0e38f;
          }
        }
      }

      // online softmax, exp2 domain, T13 defer-max (see attn_fwd_kernel)
      float m_tile = sv[0];
      #pragma unroll
      for (int r = 1; r < 32; ++r) m_tile = fmaxf(m_tile, sv[r]);
      m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32, 64));
      const float THR2 = 11.54f;  // 8 * log2(e)
      if (!__all(m_tile - m_run <= THR2)) {
        const float m_new = fmaxf(m_run, m_tile);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
        m_run = m_new;
        #pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          #pragma unroll
          for (int r = 0; r < 16; ++r) acc_o[dt][r] *= alpha;
        }
      }

      float row_sum = 0.f;
      #pragma unroll
      for (int r = 0; r < 32; ++r) {
        sv[r] = __builtin_amdgcn_exp2f(sv[r] - m_run);  // sv becomes P
        row_sum += sv[r];
      }
      row_sum += __shfl_xor(row_sum, 32, 64);
      l_run += row_sum;

      mbf16x8 pf[4];
      cvals_to_frags(sv, hi, &pf[0], &pf[1]);
      cvals_to_frags(sv + 16, hi, &pf[2], &pf[3]);

      // O^T[d, q] += V^T . P  (hardware transpose read, T10)
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          acc_o[dt] = mfma32(nat_tr_frag(vcur, ks, dt), pf[ks], acc_o[dt]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (has_next) {
      asm volatile("s_waitcnt vmcnt(0)");  // own K/V glds landed
      __syncthreads();   // everyone done reading cur; nxt visible
      char* tk = k0; k0 = k1; k1 = tk;
      char* tv = vcur; vcur = vnxt; vnxt = tv;
    }
  }

  if (!wave_active || q_row >= S) return;

  fwd_store_o(acc_o, l_run, hi, ob + q_row * q_seq_stride);
}

__global__ void __launch_bounds__(256, 2)
paged_prefill_attn_kernel(const unsigned short* __restrict__ q,
                          const unsigned short* __restrict__ kpool,
                          const unsigned short* __restrict__ vpool,
                          unsigned short* __restrict__ o,
                          const int* __restrict__ bt,   // [B, M]
                          const int* __restrict__ ctx,  // [B]
                          int B, int S, int Hq, int Hkv, int num_pages,
                          int logP, int M, float scale) {
  __shared__ __align__(16) char smem[4 * KIMG_BYTES];

  const int nqt = (S + 4 * QBLK - 1) / (4 * QBLK);
  const int G = Hq / Hkv;
  int b, hq, qt;
  map_block_fwd(B, Hq, Hkv, nqt, G, &b, &hq, &qt);
  const int hkv = hq / G;
  const long seq_off = ((long)b * S * Hq + hq) * HD;
  paged_prefill_tile(q + seq_off, kpool + (long)hkv * HD,
                     vpool + (long)hkv * HD, o + seq_off, bt + (long)b * M,
                     ctx[b], S, qt, Hq, Hkv, num_pages, logP, M, scale, smem);
}

// ---------------------------------------------------------------------------
// Ragged paged prefill: the same block work over a PACKED q [T, Hq, 128]
// holding the chunks of B sequences of different lengths back to back.
//
//   tiles  int4 [ntiles], built on the host from the lengths: (sequence b,
//          q tile qt of that sequence, cu[b] = its first packed row, S_b =
//          its chunk length). Tile qt of sequence b covers packed rows
//          cu[b] + 128*qt .. +127, cut at S_b: a tile never holds rows of
//          two sequences.
//   bt     int32 [B, M], ctx int32 [B]: row b is sequence b's.
//
// A block is paged_prefill_tile on (q + cu[b] rows, S_b, ctx[b], qt), the
// very call the [B, S] kernel makes for a batch holding sequence b alone,
// so sequence b's output is bit-identical to that kernel's at every ctx.
//
// Block map. A unit is a (tile, kv head) pair, unit = tile * Hkv + hkv,
// and owns G = Hq / Hkv blocks, one per q head of the group. The
// dispatcher deals consecutive blockIdx to consecutive XCDs, so with
// xcd = bid & 7, slot = bid >> 3 the blocks of unit (slot / G) * 8 + xcd
// all sit on one XCD and read its K/V stream through one L2. The grid is
// rounded up to whole rounds of 8 units; blocks of a unit past the end
// leave as a whole before any barrier. With Hkv % 8 == 0 every tile of a
// (sequence, kv head) lands on XCD hkv & 7, as in map_block_fwd; with a
// smaller Hkv the tiles of one stream spread over 8 / Hkv XCDs (no equal
// group size exists to deal whole streams to XCDs when lengths differ).
// Units are walked in tile-list order, which the host chooses.
//
// Tile contents are clamped (b to [0, B), cu to [0, T), S_b to
// [1, T - cu], qt to a tile of the chunk), so no list can address outside
// q, o or the table; the pools are guarded as in the [B, S] kernel.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 2)
paged_prefill_attn_ragged_kernel(
    const unsigned short* __restrict__ q,      // [T, Hq, 128]
    const unsigned short* __restrict__ kpool,
    const unsigned short* __restrict__ vpool,
    unsigned short* __restrict__ o,            // [T, Hq, 128]
    const int* __restrict__ bt,                // [B, M]
    const int* __restrict__ ctx,               // [B]
    const int4* __restrict__ tiles,            // [ntiles]
    int ntiles, int B, int T, int Hq, int Hkv, int num_pages, int logP,
    int M, float scale) {
  __shared__ __align__(16) char smem[4 * KIMG_BYTES];

  const int G = Hq / Hkv;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int unit = (slot / G) * 8 + xcd;
  if (unit >= ntiles * Hkv) return;  // block-uniform: the padding units
  const int hkv = unit % Hkv;
  const int hq = hkv * G + slot % G;
  const int4 td = tiles[unit / Hkv];
  const int b = min(max(td.x, 0), B - 1);
  const int cu = min(max(td.z, 0), T - 1);
  const int S = min(max(td.w, 1), T - cu);
  const int qt = min(max(td.y, 0), (S - 1) / (4 * QBLK));
  const long seq_off = ((long)cu * Hq + hq) * HD;
  paged_prefill_tile(q + seq_off, kpool + (long)hkv * HD,
                     vpool + (long)hkv * HD, o + seq_off, bt + (long)b * M,
                     ctx[b], S, qt, Hq, Hkv, num_pages, logP, M, scale, smem);
}

// ---------------------------------------------------------------------------
// Backward preprocess: delta[b,h,s] = rowsum(dO * O)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
attn_bwd_pre_kernel(const unsigned short* __restrict__ dout,
                    const unsigned short* __restrict__ o,
                    float* __restrict__ delta,  // [B,Hq,S]
                    long rows,  // B*S*Hq
                    int S, int Hq) {
  // 16 lanes per row x 8 elems (16-B loads; the 1-row-per-wave version's
  // 4-B loads ran 3x off roofline); 4 rows per wave, 16 per block
  const long row = (long)blockIdx.x * 16 + threadIdx.x / 16;
  if (row >= rows) return;
  const int sl = threadIdx.x & 15;
  const unsigned short* dp = dout + row * HD + sl * 8;
  const unsigned short* op = o + row * HD + sl * 8;
  ushort8 dv = *(const ushort8*)dp;
  ushort8 ov = *(const ushort8*)op;
  float acc = 0.f;
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc = fmaf(bf16_to_f32(dv[j]), bf16_to_f32(ov[j]), acc);
  }
  // reduce across the 16-lane group
  #pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    acc += __shfl_down(acc, off, 16);  // width 16: stay within the group
  }
  if (sl == 0) {
    const long b = row / ((long)S * Hq);
    const long s = (row / Hq) % S;
    const long h = row % Hq;
    delta[(b * Hq + h) * S + s] = acc;
  }
}

// ---------------------------------------------------------------------------
// dS scratch (dkv kernel -> streamed dQ kernel).  One 2 KiB image per
// 32q x 32k sub-tile: the scaled bf16 dS^T, natural [k 0..31][q 0..31], 64 B
// per k row.  Images are ordered [b][hq][q/128][k/32][(q/32)&3] so the walk
// of one dQ block (128 q rows, ascending k) reads one contiguous run, 8 KiB
// per 32 k rows.  Addressing uses global sub-tile coordinates only (never
// the dkv kernel's staged-tile size).  Under a causal mask q block qt keeps
// its k sub-tiles 0 .. 4*qt+3 only (the lower triangle of 128x32 groups).
// ---------------------------------------------------------------------------
#define DS_IMG_BYTES 2048

// first 8 KiB group of q block qt within one (b, hq) plane
__host__ __device__ __forceinline__ long ds_qt_base(int qt, int nqt,
                                                    int causal) {
  return causal ? 2L * qt * (qt + 1) : 4L * qt * nqt;
}

extern "C" long attn_bwd_ds_bytes(int B, int S, int Hq, int causal) {
  const int nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  return (long)B * Hq * ds_qt_base(nqt, nqt, causal) * 4 * DS_IMG_BYTES;
}

// ---------------------------------------------------------------------------
// Backward dQ (recompute form): grid over q tiles; inner loop over kv tiles.
// dQ[q,d] = scale * sum_k (P*(dP - delta))[q,k] * K[k,d]
// ---------------------------------------------------------------------------
template <int TFKV>
__global__ void __launch_bounds__(256, 2)
attn_bwd_dq_kernel(const unsigned short* __restrict__ q,
                   const unsigned short* __restrict__ k,
                   const unsigned short* __restrict__ v,
                   const unsigned short* __restrict__ dout,
                   const float* __restrict__ lse,
                   const float* __restrict__ delta,
                   unsigned short* __restrict__ dq,
                   int B, int S, int Hq, int Hkv, float scale, int causal,
                   long q_rs, long kv_rs, long dq_rs) {
  // v3 (T10): KV tiles of 64; K and V natural images arrive by async
  // global_load_lds (2-deep rings, swizzled); the dQ-accumulate A-operand
  // (K^T) is read straight off the natural K image with hardware
  // transpose reads — no K^T build, no rot image.  64 KiB LDS -> true
  // 2 blocks/CU.
  __shared__ __align__(16) char smem[4 * (TFKV * 256)];
  char* kcur = smem;
  char* knxt = smem + TFKV * 256;
  char* vcur = smem + 2 * (TFKV * 256);
  char* vnxt = smem + 3 * (TFKV * 256);

  const int nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  const int G = Hq / Hkv;
  int b, hq, qt;
  map_block_fwd(B, Hq, Hkv, nqt, G, &b, &hq, &qt);
  const int hkv = hq / G;

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const bool hi = lane >= 32;
  const int qr = lane & 31;

  const long q_seq_stride = q_rs;
  const long kv_seq_stride = kv_rs;
  const unsigned short* qb = q + (long)b * S * q_seq_stride + (long)hq * HD;
  const unsigned short* kb = k + (long)b * S * kv_seq_stride + (long)hkv * HD;
  const unsigned short* vb = v + (long)b * S * kv_seq_stride + (long)hkv * HD;
  const unsigned short* dob =
      dout + ((long)b * S) * ((long)Hq * HD) + (long)hq * HD;  // dense

  const int q0_blk = qt * BLOCK_Q;
  const int qw0 = q0_blk + wave * QBLK;
  const long q_row = qw0 + qr;
  const bool wave_active = qw0 < S;
  const bool row_valid = q_row < S;

  mbf16x8 qfrag[8];
  float my_lse2 = 0.f, my_delta = 0.f;
  const long qrow_safe = row_valid ? q_row : (S - 1);
  const unsigned short* dop =
      dob + qrow_safe * ((long)Hq * HD) + (hi ? 8 : 0);
  {
    const unsigned short* qp = qb + qrow_safe * q_seq_stride + (hi ? 8 : 0);
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      qfrag[c] = __builtin_bit_cast(mbf16x8, *(const ushort8*)(qp + c * 16));
    }
    if (row_valid) {
      my_lse2 = lse[((long)b * Hq + hq) * S + q_row] * LOG2E;
      my_delta = delta[((long)b * Hq + hq) * S + q_row];
    }
  }

  f32x16 acc_dq[4] = {};
  const float sc2 = scale * LOG2E;

  const int kv_limit = causal ? min(S, q0_blk + BLOCK_Q) : S;
  const int ntiles = (kv_limit + TFKV - 1) / TFKV;
  const int qw_max = min(qw0 + QBLK - 1, S - 1);

  stage_k_glds<4, TFKV>(kb, 0, kv_seq_stride, S, kcur);
  stage_k_glds<4, TFKV>(vb, 0, kv_seq_stride, S, vcur);
  asm volatile("s_waitcnt vmcnt(0)");
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * TFKV;
    const bool has_next = (t + 1) < ntiles;
    if (has_next) {
      // next tile's glds issue BEFORE compute; with the XCD swizzle the
      // K/V stream is L2-resident, one tile of cover is plenty
      stage_k_glds<4, TFKV>(kb, kv0 + TFKV, kv_seq_stride, S, knxt);
      stage_k_glds<4, TFKV>(vb, kv0 + TFKV, kv_seq_stride, S, vnxt);
    }

    const bool needed = wave_active && (!causal || kv0 <= qw_max);
    if (needed) {
      // dO fragments re-read each tile (L2-hot; keeping them resident
      // costs 32 VGPR across the staging phase and spills)
      mbf16x8 dofrag[8];
      #pragma unroll
      for (int c = 0; c < 8; ++c) {
        dofrag[c] =
            __builtin_bit_cast(mbf16x8, *(const ushort8*)(dop + c * 16));
      }
      // two 32-row k sub-tiles fully sequentially (no running max to
      // couple them -> half the live accumulators of a fused pass; the
      // loop must NOT unroll or both subs' accumulators go live at once)
      #pragma clang loop unroll(disable)
      for (int sb = 0; sb < TFKV / 32; ++sb) {
        if (causal && kv0 + 32 * sb > qw_max) break;  // rest fully masked
        f32x16 acc_s = {}, acc_dp = {};
        #pragma unroll
        for (int c = 0; c < 8; ++c) {
          acc_s = mfma32(kimg_frag(kcur, sb, c), qfrag[c], acc_s);
          acc_dp = mfma32(kimg_frag(vcur, sb, c), dofrag[c], acc_dp);
        }
        const int k0 = kv0 + 32 * sb;
        const bool mask_tile =
            (causal && k0 + 31 > qw0) || (k0 + 32 > S) || !row_valid;
        float ds[16];
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s2 = acc_s[r] * sc2;
          if (mask_tile) {
            const long kg = k0 + c_row(r, hi);
            if (kg >= S || !row_valid || (causal && kg > q_row)) {
              s2 = -3.0e38f;
            }
          }
          const float pr = __builtin_amdgcn_exp2f(s2 - my_lse2);
          ds[r] = scale * pr * (acc_dp[r] - my_delta);
        }
        mbf16x8 df0, df1;
        cvals_to_frags(ds, hi, &df0, &df1);
        // dQ^T[d, q] += K^T . dS^T; K^T fragments by hardware transpose
        // read from the natural K image (T10)
        #pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          acc_dq[dt] =
              mfma32(nat_tr_frag(kcur, 2 * sb, dt), df0, acc_dq[dt]);
          acc_dq[dt] =
              mfma32(nat_tr_frag(kcur, 2 * sb + 1, dt), df1, acc_dq[dt]);
        }
      }
    }

    if (has_next) {
      asm volatile("s_waitcnt vmcnt(0)");
      __syncthreads();   // all waves done reading cur; nxt glds visible
      char* tk = kcur; kcur = knxt; knxt = tk;
      char* tv = vcur; vcur = vnxt; vnxt = tv;
    }
  }

  if (!wave_active || !row_valid) return;
  unsigned short* dqb =
      dq + ((long)b * S + q_row) * dq_rs + (long)hq * HD;
  #pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    #pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4_raw w;
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = (short)f32_to_bf16(acc_dq[dt][4 * g + j]);
      }
      *(bf16x4_raw*)(dqb + dt * 32 + 8 * g + 4 * (hi ? 1 : 0)) = w;
    }
  }
}

// ---------------------------------------------------------------------------
// Backward dQ (streamed form): dQ[q,d] = sum_k dS[q,k] * K[k,d] over the dS
// images the dkv kernel exported.  One product: no Q, dO, V, lse, delta,
// exp2 or mask.  Same grid, XCD grouping, k order and MFMA sequence as the
// recompute kernel (dQ^T[d,q] += K^T . dS^T, k ascending in 16-row slices),
// so the two forms differ only by how the bf16 dS fragments were produced.
//
// K tiles of 64 rows arrive by global_load_lds into the usual swizzled
// natural image (block-shared, 2-ring, one barrier per tile) and are read
// with nat_tr_frag.  dS is WAVE-PRIVATE: wave w stages only the images of
// its own 32 q rows (2 x 1 KiB glds per 32 k rows, lane-linear, no source
// permutation), so its own vmcnt(0) orders them and a wave never stages a
// sub-tile it does not consume — the set read here (k0 < S, and k0 <= qw0
// under the causal mask) is a subset of what the dkv kernel writes.
//
// Bank conflicts of the dS reads: ds_read_b64_tr_b16 banks over 2 groups of
// 32 lanes, 64 banks x 4 B.  A group is two 16-lane clusters (q 0..15 and
// q 16..31 of the same 4 k rows); lane j of a cluster addresses the 8-B
// chunk (k row j>>2, q chunk j&3), so the group covers 4 consecutive 64-B k
// rows completely = 256 contiguous bytes starting at a multiple of 256 —
// every bank exactly once, no swizzle needed for a 64-B-row image.
// LDS issue: per 32 k rows 8 MFMAs take 16 K + 4 dS transpose reads, 2.5
// per MFMA.
// ---------------------------------------------------------------------------
__device__ __forceinline__ mbf16x8 ds_tr_frag(const char* img, int ks) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 15;
  const int r_lo = ks * 16 + ((lane >> 5) * 8) + (j >> 2);
  const int cb = ((lane >> 4) & 1) * 32 + (j & 3) * 8;
  short4_v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s4p)(img + r_lo * 64 + cb));
  short4_v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s4p)(img + (r_lo + 4) * 64 + cb));
  uint2_v ul = __builtin_bit_cast(uint2_v, lo);
  uint2_v uh = __builtin_bit_cast(uint2_v, hi);
  uint4_v u = {ul[0], ul[1], uh[0], uh[1]};
  return __builtin_bit_cast(mbf16x8, u);
}

__global__ void __launch_bounds__(256, 2)
attn_bwd_dq_stream_kernel(const unsigned short* __restrict__ k,
                          const char* __restrict__ ds,
                          unsigned short* __restrict__ dq,
                          int B, int S, int Hq, int Hkv, int causal,
                          long kv_rs, long dq_rs, int heavy_first) {
  // K 2-ring (32 KiB) + dS 2-ring [buf][wave][2 images] (32 KiB) = 64 KiB
  __shared__ __align__(16) char smem[2 * KIMG_BYTES + 16 * DS_IMG_BYTES];

  const int nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  const int G = Hq / Hkv;
  int b, hq, qt;
  map_block_fwd(B, Hq, Hkv, nqt, G, &b, &hq, &qt);
  if (heavy_first) qt = nqt - 1 - qt;
  const int hkv = hq / G;

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const bool hi = lane >= 32;

  char* kcur = smem;
  char* knxt = smem + KIMG_BYTES;
  char* dcur = smem + 2 * KIMG_BYTES + wave * (2 * DS_IMG_BYTES);
  char* dnxt = dcur + 8 * DS_IMG_BYTES;

  const unsigned short* kb = k + (long)b * S * kv_rs + (long)hkv * HD;
  const int q0_blk = qt * BLOCK_Q;
  const int qw0 = q0_blk + wave * QBLK;
  const long q_row = qw0 + (lane & 31);
  const bool wave_active = qw0 < S;
  // start of the last 32-row k sub-tile this wave consumes (-1: none)
  const int k_last =
      !wave_active ? -1 : (causal ? qw0 : ((S - 1) / KBLK) * KBLK);
  // this wave's images: [k/32] stride 8 KiB, lane-linear within an image
  const char* ds_w =
      ds + ((((long)b * Hq + hq) * ds_qt_base(nqt, nqt, causal) +
             ds_qt_base(qt, nqt, causal)) * 4 + wave) * DS_IMG_BYTES +
      lane * 16;

  auto stage_ds = [&](int kv0, char* dst) {
    #pragma unroll
    for (int sb = 0; sb < FKV / 32; ++sb) {
      const int k0 = kv0 + 32 * sb;
      if (k0 <= k_last) {
        const char* src = ds_w + (long)(k0 / KBLK) * (4 * DS_IMG_BYTES);
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) unsigned int*)(
                  src + i * 1024),
              (__attribute__((address_space(3))) unsigned int*)(
                  dst + sb * DS_IMG_BYTES + i * 1024),
              16, 0, 0);
        }
      }
    }
  };

  f32x16 acc_dq[4] = {};

  const int kv_limit = causal ? min(S, q0_blk + BLOCK_Q) : S;
  const int ntiles = (kv_limit + FKV - 1) / FKV;

  stage_k_glds<4, FKV>(kb, 0, kv_rs, S, kcur);
  stage_ds(0, dcur);
  asm volatile("s_waitcnt vmcnt(0)");
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * FKV;
    const bool has_next = (t + 1) < ntiles;
    if (has_next) {
      stage_k_glds<4, FKV>(kb, kv0 + FKV, kv_rs, S, knxt);
      stage_ds(kv0 + FKV, dnxt);
    }

    if (kv0 <= k_last) {
      #pragma unroll
      for (int sb = 0; sb < FKV / 32; ++sb) {
        if (kv0 + 32 * sb > k_last) break;
        const mbf16x8 df0 = ds_tr_frag(dcur + sb * DS_IMG_BYTES, 0);
        const mbf16x8 df1 = ds_tr_frag(dcur + sb * DS_IMG_BYTES, 1);
        #pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          acc_dq[dt] =
              mfma32(nat_tr_frag(kcur, 2 * sb, dt), df0, acc_dq[dt]);
          acc_dq[dt] =
              mfma32(nat_tr_frag(kcur, 2 * sb + 1, dt), df1, acc_dq[dt]);
        }
      }
    }

    if (has_next) {
      asm volatile("s_waitcnt vmcnt(0)");  // own K pieces + own dS landed
      __syncthreads();   // all waves done reading cur K; nxt K visible
      char* tk = kcur; kcur = knxt; knxt = tk;
      char* td = dcur; dcur = dnxt; dnxt = td;
    }
  }

  if (!wave_active || q_row >= S) return;
  unsigned short* dqb = dq + ((long)b * S + q_row) * dq_rs + (long)hq * HD;
  #pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    #pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4_raw w;
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = (short)f32_to_bf16(acc_dq[dt][4 * g + j]);
      }
      *(bf16x4_raw*)(dqb + dt * 32 + 8 * g + 4 * (hi ? 1 : 0)) = w;
    }
  }
}

// ---------------------------------------------------------------------------
// Backward dK/dV: grid over kv blocks of 128 rows (wave owns 32); inner loop
// over GQA group heads x q tiles.  No atomics: each (b, hkv, kv-row) is
// owned by exactly one wave.  Split into a dV pass and a dK pass so each
// kernel fits 2 waves/SIMD (the combined kernel needed 316 regs -> 1
// wave/SIMD with zero latency hiding; the S^T recompute in the second pass
// costs 8 extra MFMAs/tile but doubles occupancy).
// ---------------------------------------------------------------------------
// 512-thread (8-wave) staging variants: same image formats as the 4-wave
// helpers, work split across twice the threads.
template <int TFKV = FKV>
__device__ __forceinline__ void stage_k_glds8(
    const unsigned short* __restrict__ kb, long kv0, long stride_elems,
    int S, char* kimg) {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  #pragma unroll
  for (int j = 0; j < TFKV / 32; ++j) {
    const int i = wave * (TFKV / 32) + j;
    const int row = i * 4 + (lane >> 4);
    const int colbyte = ((lane & 15) * 16) ^ ((row & 15) << 4);
    long srow = kv0 + row;
    if (srow >= S) srow = S - 1;
    const char* src = (const char*)(kb + srow * stride_elems) + colbyte;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(kimg + i * 1024),
        16, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// Backward dK+dV, one 8-wave kernel.  Waves w and w+4 own the SAME 32 kv
// rows of a 128-row block: w accumulates dV, w+4 accumulates dK — so the
// Q/dO streams are staged ONCE for both outputs (the two-pass version
// streamed them 2-3x).  C-layouts are flipped vs the fwd kernel (swapped
// operand order): each lane owns one q COLUMN, so lse/delta are direct
// per-lane global loads (no LDS staging).  Four staged images per tile —
// Q nat (S^T chain B-op), dO nat (dP^T chain B-op), Q^T (dK accumulate
// B-op), dO^T (dV accumulate B-op) — double-buffered in 128 KiB LDS, one
// barrier per tile.
// ---------------------------------------------------------------------------

template <int TFKV>
__global__ void __launch_bounds__(512, 2)
attn_bwd_dkv_kernel(const unsigned short* __restrict__ q,
                    const unsigned short* __restrict__ k,
                    const unsigned short* __restrict__ v,
                    const unsigned short* __restrict__ dout,
                    const float* __restrict__ lse,
                    const float* __restrict__ delta,
                    unsigned short* __restrict__ dk,
                    unsigned short* __restrict__ dv,
                    char* __restrict__ ds,  // dS scratch, or null
                    int B, int S, int Hq, int Hkv, float scale, int causal,
                    long q_rs, long kv_rs, long dout_rs, long out_rs) {
  // T10: the accumulate B-operands (Q^T / dO^T) are hardware transpose
  // reads off the natural images — no Q^T/dO^T builds, half the LDS
  // (64 KiB + lse) -> 2 blocks/CU.
  // TFKV=64: 64 KiB LDS -> 2 blocks/CU; TFKV=128: 128 KiB, 1 block but
  // half the barriers/loop iterations (A/B via TORCHX_AMD_DKV_FKV)
  __shared__ __align__(16) char smem[4 * (TFKV * 256)];
  __shared__ float lse_buf[2][TFKV], del_buf[2][TFKV];
  char* qn_c = smem;                       // Q natural cur
  char* don_c = smem + TFKV * 256;         // dO natural cur
  char* qn_n = smem + 2 * (TFKV * 256);
  char* don_n = smem + 3 * (TFKV * 256);

  const int nkt = (S + BLOCK_K - 1) / BLOCK_K;
  const int G = Hq / Hkv;
  int b, hkv, kt;
  {
    int bid = blockIdx.x;
    if (((B * Hkv) & 7) == 0) {
      const int xcd = bid & 7, slot = bid >> 3;
      const int g = (slot / nkt) * 8 + xcd;
      b = g / Hkv;
      hkv = g % Hkv;
      kt = slot % nkt;
    } else {
      b = bid / (Hkv * nkt);
      bid -= b * Hkv * nkt;
      hkv = bid / nkt;
      kt = bid % nkt;
    }
  }

  const int wave = threadIdx.x / 64;
  const bool is_dk = wave >= 4;
  const int lane = threadIdx.x & 63;
  const bool hi = lane >= 32;
  const int kr = lane & 31;

  const long q_seq_stride = q_rs;
  const long kv_seq_stride = kv_rs;
  const unsigned short* kb = k + (long)b * S * kv_seq_stride + (long)hkv * HD;
  const unsigned short* vb = v + (long)b * S * kv_seq_stride + (long)hkv * HD;

  const int kv0_blk = kt * BLOCK_K;
  const int kw0 = kv0_blk + (wave & 3) * KBLK;  // this wave's 32 kv rows
  const long k_row = kw0 + kr;
  const bool wave_active = kw0 < S;
  const bool krow_valid = k_row < S;

  // K resident in all waves; V resident in the dK waves
  mbf16x8 kfrag[8], vfrag[8];
  {
    const long row = krow_valid ? k_row : (S - 1);
    const unsigned short* kp = kb + row * kv_seq_stride + (hi ? 8 : 0);
    const unsigned short* vp = vb + row * kv_seq_stride + (hi ? 8 : 0);
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      kfrag[c] = __builtin_bit_cast(mbf16x8, *(const ushort8*)(kp + c * 16));
      if (is_dk) {
        vfrag[c] =
            __builtin_bit_cast(mbf16x8, *(const ushort8*)(vp + c * 16));
      }
    }
  }

  f32x16 acc[4] = {};
  const float sc2 = scale * LOG2E;

  const int t0 = causal ? (kv0_blk / TFKV) : 0;
  const int nt = (S + TFKV - 1) / TFKV;
  const int nt_eff = nt - t0;
  const int total = G * nt_eff;

  // dS export (dK waves only): this lane's 16 B slot inside an image — k
  // row kr, q octet hi (f0) / 2 + hi (f1) — plus the wave's k sub-tile
  const bool ds_on = is_dk && ds != nullptr;
  const int ds_nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  const long ds_plane = ds_qt_base(ds_nqt, ds_nqt, causal);
  const long ds_lane = (long)(kw0 / KBLK) * (4 * DS_IMG_BYTES) + kr * 64 +
                       (hi ? 16 : 0);

  auto head_q = [&](int gh) {
    return q + (long)b * S * q_seq_stride + (long)(hkv * G + gh) * HD;
  };
  auto head_do = [&](int gh) {
    return dout + (long)b * S * dout_rs + (long)(hkv * G + gh) * HD;
  };
  auto stage_lse = [&](int gh, int t, int buf) {
    const int hq_ = hkv * G + gh;
    const int q0_ = t * TFKV;
    if (threadIdx.x < TFKV) {
      const float* lse_b = lse + ((long)b * Hq + hq_) * S;
      const int qg = q0_ + threadIdx.x;
      lse_buf[buf][threadIdx.x] = (qg < S) ? lse_b[qg] * LOG2E : 0.f;
    } else if (threadIdx.x < 2 * TFKV) {
      const float* del_b = delta + ((long)b * Hq + hq_) * S;
      const int qg = q0_ + (threadIdx.x - TFKV);
      del_buf[buf][threadIdx.x - TFKV] = (qg < S) ? del_b[qg] : 0.f;
    }
  };

  // prologue: tile (gh=0, t=t0) — glds the natural images
  stage_k_glds8<TFKV>(head_q(0), (long)t0 * TFKV, q_seq_stride, S, qn_c);
  stage_k_glds8<TFKV>(head_do(0), (long)t0 * TFKV, dout_rs, S, don_c);
  asm volatile("s_waitcnt vmcnt(0)");
  stage_lse(0, t0, 0);
  __syncthreads();

  const float* lse_cur = lse_buf[0];
  const float* del_cur = del_buf[0];
  int lse_nxt = 1;
  for (int idx = 0; idx < total; ++idx) {
    const int gh = idx / nt_eff;
    const int t = t0 + idx % nt_eff;
    const int q0 = t * TFKV;
    const int hq = hkv * G + gh;
    const bool has_next = (idx + 1) < total;
    const int ngh = (idx + 1) / nt_eff;
    const long nrow0 = (long)(t0 + (idx + 1) % nt_eff) * TFKV;
    if (has_next) {
      // async glds issue BEFORE compute (their latency hides under the
      // MFMAs; the address temporaries are consumed by the instruction
      // immediately so this does not raise register pressure).  The
      // reg-staged tr loads stay in the tail: their 32 data registers
      // across the compute phase are what spilled.
      stage_k_glds8<TFKV>(head_q(ngh), nrow0, q_seq_stride, S, qn_n);
      stage_k_glds8<TFKV>(head_do(ngh), nrow0, dout_rs, S, don_n);
    }

    const bool needed =
        wave_active && (!causal || q0 + TFKV - 1 >= kw0);
    int n_ds = 0;   // dS stores issued behind this tile's glds pieces
    if (needed) {
      char* ds_head = ds + ((long)b * Hq + hq) * ds_plane * (4 * DS_IMG_BYTES)
                      + ds_lane;
      #pragma clang loop unroll(disable)
      for (int sb = 0; sb < TFKV / 32; ++sb) {
        if (causal && q0 + 32 * sb + 32 <= kw0) continue;  // fully masked
        // S[q, k own] (lane owns the k column; q rows via c_row so the
        // contraction dim of the accumulate MFMAs is the C-row dim);
        // dP[q, k own] for the dK waves
        f32x16 acc_s = {}, acc_dp = {};
        #pragma unroll
        for (int c = 0; c < 8; ++c) {
          acc_s = mfma32(kimg_frag(qn_c, sb, c), kfrag[c], acc_s);
          if (is_dk) {
            acc_dp = mfma32(kimg_frag(don_c, sb, c), vfrag[c], acc_dp);
          }
        }

        const int qs0 = q0 + 32 * sb;
        // causal masking only bites when SOME (q, k) pair in this
        // 32q x 32k(own) tile has k > q, i.e. qs0 < kw0 + 32; interior
        // tiles (q strictly above every owned k) skip the 16-row mask
        // VALU entirely (it used to run on EVERY causal tile)
        const bool mask_tile = (causal && qs0 < kw0 + 32)
                               || (qs0 + 32 > S) || !krow_valid;
        float cv[16];
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = 32 * sb + c_row(r, hi);  // q offset within tile
          float s2 = acc_s[r] * sc2;
          if (mask_tile) {
            const long qg = q0 + ql;
            if (qg >= S || !krow_valid || (causal && k_row > qg)) {
              s2 = -3.0e38f;
            }
          }
          const float pr =
              __builtin_amdgcn_exp2f(s2 - lse_cur[ql]);
          cv[r] = is_dk ? scale * pr * (acc_dp[r] - del_cur[ql]) : pr;
        }

        mbf16x8 f0, f1;
        cvals_to_frags(cv, hi, &f0, &f1);

        // dV[k,d] += P^T . dO ; dK[k,d] += dS^T . Q — B fragments by
        // hardware transpose read from the natural images (T10)
        const char* acc_img = is_dk ? qn_c : don_c;
        #pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          acc[dt] =
              mfma32(f0, nat_tr_frag(acc_img, 2 * sb, dt), acc[dt]);
          acc[dt] =
              mfma32(f1, nat_tr_frag(acc_img, 2 * sb + 1, dt), acc[dt]);
          if (dt == 0) {
            // export the scaled dS^T sub-tile whole (masked elements are
            // exact zeros); sub-tiles that start past the last q row are
            // not stored.  2 x 16 B per lane, 2 KiB contiguous per wave.
            // Placement: the compiler puts a vmcnt(0) in front of the
            // first transpose read of every sub-tile (it cannot prove
            // the read clear of the glds pieces in flight), so the
            // stores go right BEHIND that wait and have a whole sub-tile
            // of MFMAs before the next one; the sched_barrier keeps them
            // from being hoisted above it.
            __builtin_amdgcn_sched_barrier(0);
            if (ds_on && qs0 < S) {
              char* p = ds_head +
                        (ds_qt_base(qs0 / BLOCK_Q, ds_nqt, causal) * 4 +
                         ((qs0 / QBLK) & 3)) * DS_IMG_BYTES;
              *(uint4_v*)p = __builtin_bit_cast(uint4_v, f0);
              *(uint4_v*)(p + 32) = __builtin_bit_cast(uint4_v, f1);
              n_ds = 2;
            }
          }
        }
      }
    }

    if (has_next) {
      // own glds of the nxt tiles done.  vmcnt counts stores too, in issue
      // order: when this tile exported, its last two stores are younger
      // than every glds piece, so the wait may leave those two in flight
      if (n_ds) {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      stage_lse(ngh, t0 + (idx + 1) % nt_eff, lse_nxt);
      __syncthreads();   // ONE barrier per tile publishes everything
      lse_cur = lse_buf[lse_nxt];
      del_cur = del_buf[lse_nxt];
      lse_nxt ^= 1;
      char* tp;
      tp = qn_c; qn_c = qn_n; qn_n = tp;
      tp = don_c; don_c = don_n; don_n = tp;
    }
  }

  // store via LDS transpose (8-B global writes); wave-private f32 region
  unsigned short* out = is_dk ? dk : dv;
  __syncthreads();
  float* tr = (float*)smem + wave * (32 * 36);
  if (wave_active) {
    #pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      __syncthreads();
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        tr[c_row(r, hi) * 36 + kr] = acc[dt][r];
      }
      __syncthreads();
      #pragma unroll
      for (int rep = 0; rep < 4; ++rep) {
        const int kk = kr;
        const int d0 = (hi ? 16 : 0) + rep * 4;
        if (kw0 + kk < S) {
          bf16x4_raw w;
          #pragma unroll
          for (int j = 0; j < 4; ++j) {
            w[j] = (short)f32_to_bf16(tr[kk * 36 + d0 + j]);
          }
          *(bf16x4_raw*)(out + ((long)b * S + kw0 + kk) * out_rs +
                         (long)hkv * HD + dt * 32 + d0) = w;
        }
      }
    }
  } else {
    #pragma unroll
    for (int i = 0; i < 8; ++i) __syncthreads();
  }
}

// cvals_to_frags over already packed bf16 pairs, with the lane-half
// exchange done by v_permlane32_swap (gfx950): swap(a, b) trades a's upper
// 32 lanes for b's lower 32, so (a01, a45) -> (w0, w2) and (a23, a67) ->
// (w1, w3) in one VALU op each — the same words the shfl_xor + select form
// builds, without its eight trips through the LDS pipe.
__device__ __forceinline__ void packed_to_frags_swap(const unsigned int* a,
                                                     mbf16x8* f0,
                                                     mbf16x8* f1) {
  // a[4 * s + i] = pack(p[8 * s + 2 * i], p[8 * s + 2 * i + 1])
  unsigned int w[2][4];
  #pragma unroll
  for (int s = 0; s < 2; ++s) {
    auto e0 = __builtin_amdgcn_permlane32_swap(a[4 * s + 0], a[4 * s + 2],
                                               false, false);
    auto e1 = __builtin_amdgcn_permlane32_swap(a[4 * s + 1], a[4 * s + 3],
                                               false, false);
    w[s][0] = e0[0];
    w[s][1] = e1[0];
    w[s][2] = e0[1];
    w[s][3] = e1[1];
  }
  uint4_v u0 = {w[0][0], w[0][1], w[0][2], w[0][3]};
  uint4_v u1 = {w[1][0], w[1][1], w[1][2], w[1][3]};
  *f0 = __builtin_bit_cast(mbf16x8, u0);
  *f1 = __builtin_bit_cast(mbf16x8, u1);
}

// ---------------------------------------------------------------------------
// Backward dK+dV, merged roles: one 4-wave kernel at ONE wave per SIMD (the
// 512-register budget of gfx950: 256 VGPR + 256 AGPR).  Wave w owns kv rows
// [kt*128 + 32w, +32) and accumulates BOTH dV and dK, so S^T, P and dP are
// computed once per sub-tile (32 MFMAs where the split kernel's wave pair
// issues 40; one mask/exp2 pass instead of two; 16 Q/dO fragment reads
// instead of 24).  Every expression, and the order of every accumulation,
// is the split kernel's, so dk, dv and the exported dS are bit-identical.
//
// At one wave per SIMD nothing hides a latency for free, so the tile body
// is a hand-staged software pipeline over single 32-q sub-tiles: LDS reads
// are issued in groups ahead of their MFMAs, and the S/dP chain of the
// next sub-tile and the dV/dK accumulation of the previous one run chunk
// by chunk under the mask/exp2 VALU of the current one (see the stage
// list in the loop).  The block mapping, the staged
// images, the lse/delta double buffer, the dS image layout and the
// epilogue are the split kernel's.  The next tile's lse/delta value is
// loaded into one register at the loop head, next to the glds issue, and
// written to LDS at the tile end.
// ---------------------------------------------------------------------------
template <int TFKV>
__global__ void __launch_bounds__(256, 1)
attn_bwd_dkv_merged_kernel(const unsigned short* __restrict__ q,
                           const unsigned short* __restrict__ k,
                           const unsigned short* __restrict__ v,
                           const unsigned short* __restrict__ dout,
                           const float* __restrict__ lse,
                           const float* __restrict__ delta,
                           unsigned short* __restrict__ dk,
                           unsigned short* __restrict__ dv,
                           char* __restrict__ ds,  // dS scratch, or null
                           int B, int S, int Hq, int Hkv, float scale,
                           int causal, long q_rs, long kv_rs, long dout_rs,
                           long out_rs) {
  constexpr int NS = TFKV / 32;  // 32-q sub-tiles per staged tile
  __shared__ __align__(16) char smem[4 * (TFKV * 256)];
  __shared__ __align__(16) float lse_buf[2][TFKV], del_buf[2][TFKV];
  char* qn_c = smem;                       // Q natural cur
  char* don_c = smem + TFKV * 256;         // dO natural cur
  char* qn_n = smem + 2 * (TFKV * 256);
  char* don_n = smem + 3 * (TFKV * 256);

  const int nkt = (S + BLOCK_K - 1) / BLOCK_K;
  const int G = Hq / Hkv;
  int b, hkv, kt;
  {
    int bid = blockIdx.x;
    if (((B * Hkv) & 7) == 0) {
      const int xcd = bid & 7, slot = bid >> 3;
      const int g = (slot / nkt) * 8 + xcd;
      b = g / Hkv;
      hkv = g % Hkv;
      kt = slot % nkt;
    } else {
      b = bid / (Hkv * nkt);
      bid -= b * Hkv * nkt;
      hkv = bid / nkt;
      kt = bid % nkt;
    }
  }

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  const bool hi = lane >= 32;
  const int kr = lane & 31;

  const long q_seq_stride = q_rs;
  const long kv_seq_stride = kv_rs;
  const unsigned short* kb = k + (long)b * S * kv_seq_stride + (long)hkv * HD;
  const unsigned short* vb = v + (long)b * S * kv_seq_stride + (long)hkv * HD;

  const int kv0_blk = kt * BLOCK_K;
  const int kw0 = kv0_blk + wave * KBLK;  // this wave's 32 kv rows
  const long k_row = kw0 + kr;
  const bool wave_active = kw0 < S;
  const bool krow_valid = k_row < S;

  // K and V rows of this wave stay resident
  mbf16x8 kfrag[8], vfrag[8];
  {
    const long row = krow_valid ? k_row : (S - 1);
    const unsigned short* kp = kb + row * kv_seq_stride + (hi ? 8 : 0);
    const unsigned short* vp = vb + row * kv_seq_stride + (hi ? 8 : 0);
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      kfrag[c] = __builtin_bit_cast(mbf16x8, *(const ushort8*)(kp + c * 16));
      vfrag[c] = __builtin_bit_cast(mbf16x8, *(const ushort8*)(vp + c * 16));
    }
  }

  f32x16 accv[4] = {}, acck[4] = {};
  const float sc2 = scale * LOG2E;

  const int t0 = causal ? (kv0_blk / TFKV) : 0;
  const int nt = (S + TFKV - 1) / TFKV;
  const int nt_eff = nt - t0;
  const int total = G * nt_eff;

  // dS export: this lane's 16 B slot inside an image — k row kr, q octet
  // hi (f0) / 2 + hi (f1) — plus the wave's k sub-tile
  const bool ds_on = ds != nullptr;
  const int ds_nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  const long ds_plane = ds_qt_base(ds_nqt, ds_nqt, causal);
  const long ds_lane = (long)(kw0 / KBLK) * (4 * DS_IMG_BYTES) + kr * 64 +
                       (hi ? 16 : 0);

  auto head_q = [&](int gh) {
    return q + (long)b * S * q_seq_stride + (long)(hkv * G + gh) * HD;
  };
  auto head_do = [&](int gh) {
    return dout + (long)b * S * dout_rs + (long)(hkv * G + gh) * HD;
  };
  // lse (threads [0, TFKV)) / delta (threads [TFKV, 2*TFKV)) value of tile
  // (gh, t) for this thread, and its slot in the LDS buffers
  auto load_lse = [&](int gh, int t) -> float {
    const int hq_ = hkv * G + gh;
    const int q0_ = t * TFKV;
    float x = 0.f;
    if (threadIdx.x < TFKV) {
      const float* lse_b = lse + ((long)b * Hq + hq_) * S;
      const int qg = q0_ + threadIdx.x;
      x = (qg < S) ? lse_b[qg] : 0.f;
    } else if (threadIdx.x < 2 * TFKV) {
      const float* del_b = delta + ((long)b * Hq + hq_) * S;
      const int qg = q0_ + (threadIdx.x - TFKV);
      x = (qg < S) ? del_b[qg] : 0.f;
    }
    return x;
  };
  // (the lse value is scaled here, not at the load: an ALU use of the
  // loaded register at the loop head would wait for the load and, with
  // it, for every glds piece issued in front of it)
  auto store_lse = [&](int buf, float x) {
    if (threadIdx.x < TFKV) {
      lse_buf[buf][threadIdx.x] = x * LOG2E;
    } else if (threadIdx.x < 2 * TFKV) {
      del_buf[buf][threadIdx.x - TFKV] = x;
    }
  };

  // prologue: tile (gh=0, t=t0) — glds the natural images
  stage_k_glds<4, TFKV>(head_q(0), (long)t0 * TFKV, q_seq_stride, S, qn_c);
  stage_k_glds<4, TFKV>(head_do(0), (long)t0 * TFKV, dout_rs, S, don_c);
  asm volatile("s_waitcnt vmcnt(0)");
  store_lse(0, load_lse(0, t0));
  __syncthreads();

  int lse_nxt = 1;   // lse/delta buffer of the next tile; cur is the other
  // The accumulators are untouched from the tile head to step 1.  Naming
  // them there, in their own register file, keeps the allocator from
  // parking them elsewhere for that stretch and moving all 128 back.
  auto pin_acc = [&]() __attribute__((always_inline)) {
    asm volatile("" : "+a"(accv[0]), "+a"(accv[1]), "+a"(accv[2]),
                      "+a"(accv[3]), "+a"(acck[0]), "+a"(acck[1]),
                      "+a"(acck[2]), "+a"(acck[3]));
  };
  for (int idx = 0; idx < total; ++idx) {
    const int gh = idx / nt_eff;
    const int t = t0 + idx % nt_eff;
    const int q0 = t * TFKV;
    const int hq = hkv * G + gh;
    const bool has_next = (idx + 1) < total;
    const int ngh = (idx + 1) / nt_eff;
    const int ntile = t0 + (idx + 1) % nt_eff;
    float lse_reg = 0.f;
    // opaque copy of the lane id: what the tile derives from it (glds
    // source offsets, LDS read addresses) is recomputed per tile — hoisted
    // out of the tile loop those lane constants would be spilled around it
    int lane_t = lane;
    asm volatile("" : "+v"(lane_t));
    pin_acc();
    if (has_next) {
      // async glds issue BEFORE compute: their latency hides under the
      // S/dP chain and the softmax of the first sub-tile.  The next
      // tile's lse/delta value rides along in ONE register, so the
      // barrier at the tile end does not wait on a fresh global load.
      stage_k_glds_at<4, TFKV>(head_q(ngh), (long)ntile * TFKV, q_seq_stride,
                               S, qn_n, wave, lane_t);
      stage_k_glds_at<4, TFKV>(head_do(ngh), (long)ntile * TFKV, dout_rs, S,
                               don_n, wave, lane_t);
      lse_reg = load_lse(ngh, ntile);
    }

    // first sub-tile of this tile that is not fully masked for the wave's
    // kv rows (uniform); NS when the wave has nothing to do in the tile
    int sb0 = 0;
    if (causal && kw0 > q0) sb0 = (kw0 - q0) / 32;
    if (!wave_active || sb0 > NS) sb0 = NS;
    sb0 = __builtin_amdgcn_readfirstlane(sb0);

    int n_ds = 0;   // dS stores issued behind this tile's glds pieces
    char* ds_head = ds + ((long)b * Hq + hq) * ds_plane * (4 * DS_IMG_BYTES)
                    + ds_lane;

    // The tile body is a software pipeline over single 32-q sub-tiles,
    // rotated so that the mask/exp2/pack VALU of sub-tile sb always has
    // MFMAs under it.  Step sb runs 16 chunks, pinned by sched_barriers;
    // chunk r holds
    //   - MFMA r of the S/dP chain of sub-tile sb+1 (even r: S, odd r: dP),
    //   - MFMA r of the dV/dK accumulation of sub-tile sb-1,
    //   - the VALU of C-value r of sub-tile sb,
    // and, in every second chunk, the LDS reads of the next chunk pair
    // (Q/dO fragments, transpose-read fragments, lse/delta), so that only
    // a window of them is live.  Carried from
    // step to step: S/dP of the next sub-tile (ns, ndp) and the P/dS
    // fragments of the previous one (p0, p1, d0, d1).  The pipeline drains
    // at the tile boundary: the chain of sub-tile 0 and the accumulation of
    // the last sub-tile run bare, in front of the tile's one barrier.
    //
    // LDS addresses.  For a fixed lane every read of the tile body differs
    // from a lane constant by a compile-time byte offset: a sub-tile step
    // adds a multiple of 32 rows, so the (row & 15) << 4 swizzle term does
    // not move, and the dO image sits TFKV * 256 B behind the Q image.
    // Twelve addresses (8 d-slices of kimg_frag, 4 d-tiles of nat_tr_frag)
    // are derived per tile from the opaque copy of the lane id, and every
    // read is one ds_read at base + immediate.
    const int hi_t = lane_t >> 5;
    const int img_off = (int)(qn_c - smem);   // Q image; dO at + DO_OFF
    constexpr int DO_OFF = TFKV * 256;
    int a_kf[8], a_tr[4];
    {
      // kimg_frag(img, sub, c) = img + sub * 8192 + (kb ^ 32c)
      const int kb = (lane_t & 31) * 256 +
                     ((hi_t * 16) ^ ((lane_t & 15) << 4));
      #pragma unroll
      for (int c = 0; c < 8; ++c) a_kf[c] = img_off + (kb ^ (c * 32));
      // nat_tr_frag(img, ks, dt): low rows at img + ks * 4096 + (tb ^ 64dt),
      // high rows (+4: swizzle bit 6 flips) at + 1024 + (tb ^ 64(dt ^ 1))
      const int j = lane_t & 15;
      const int rl = hi_t * 8 + (j >> 2);
      const int g16 = ((lane_t >> 4) & 1) * 32 + ((j & 3) >> 1) * 16;
      const int tb = rl * 256 + ((g16 ^ (rl << 4)) | ((j & 1) * 8));
      #pragma unroll
      for (int dt = 0; dt < 4; ++dt) a_tr[dt] = img_off + (tb ^ (dt * 64));
    }
    const float* lse_l = &lse_buf[lse_nxt ^ 1][hi_t * 4];
    const float* del_l = &del_buf[lse_nxt ^ 1][hi_t * 4];
    // Q (o = 1) / dO (o = 0) fragment of sub-tile sb, d-slice c
    auto kf_read = [&](int o, int sb, int c)
        __attribute__((always_inline)) {
      return *(const mbf16x8*)(smem + a_kf[c] +
                               ((o ? 0 : DO_OFF) + sb * 8192));
    };
    // B fragment of accumulate MFMA i of sub-tile sb, by hardware transpose
    // read from the natural images (T10).  i = 4 * dt + 2 * k-slice + o:
    // o = 0 reads dO (for dV += P^T . dO), o = 1 reads Q (dK += dS^T . Q)
    auto acc_frag = [&](int sb, int i) __attribute__((always_inline)) {
      const int dt = i >> 2;
      const int imm = ((i & 1) ? 0 : DO_OFF) +
                      (2 * sb + ((i >> 1) & 1)) * 4096;
      short4_v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s4p)(smem + a_tr[dt] + imm));
      short4_v hh = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s4p)(smem + a_tr[dt ^ 1] + (imm + 1024)));
      uint2_v ul = __builtin_bit_cast(uint2_v, lo);
      uint2_v uh = __builtin_bit_cast(uint2_v, hh);
      uint4_v u = {ul[0], ul[1], uh[0], uh[1]};
      return __builtin_bit_cast(mbf16x8, u);
    };
    // accumulate MFMA i: per accumulator the order is p0 then p1, d0 then
    // d1, as in the split kernel
    auto acc_mfma = [&](int i, const mbf16x8& f, const mbf16x8& p0,
                        const mbf16x8& p1, const mbf16x8& d0,
                        const mbf16x8& d1) {
      const int dt = i >> 2;
      if (i & 1) {
        acck[dt] = mfma32((i & 2) ? d1 : d0, f, acck[dt]);
      } else {
        accv[dt] = mfma32((i & 2) ? p1 : p0, f, accv[dt]);
      }
    };
    // export the scaled dS^T sub-tile whole (masked elements are exact
    // zeros; sub-tiles that start past the last q row are not stored):
    // 2 x 16 B per lane, 2 KiB contiguous per wave
    auto export_ds = [&](int sb, const mbf16x8& d0, const mbf16x8& d1) {
      const int qs0 = q0 + 32 * sb;
      if (ds_on && sb >= sb0 && qs0 < S) {
        char* p = ds_head +
                  (ds_qt_base(qs0 / BLOCK_Q, ds_nqt, causal) * 4 +
                   ((qs0 / QBLK) & 3)) * DS_IMG_BYTES;
        *(uint4_v*)p = __builtin_bit_cast(uint4_v, d0);
        *(uint4_v*)(p + 32) = __builtin_bit_cast(uint4_v, d1);
        n_ds = 2;
      }
    };

    if (sb0 < NS) {
      // In the diagonal tile of a causal head the sub-tiles in front of
      // sb0 are fully masked for this wave; they run all the same (p and
      // dS come out as exact zeros, which leave the accumulators as they
      // are) and only their export is skipped: the tile ends at a barrier
      // behind wave 0, whose sb0 is 0 there, so skipping them would not
      // end it sooner.
      f32x16 ns, ndp;            // S / dP of the sub-tile the next step owns
      mbf16x8 p0, p1, d0, d1;    // P / dS fragments of the previous sub-tile

      // one pipeline step; has_prev / has_next say whether an accumulation
      // and a chain ride under this sub-tile's VALU
      auto step_body = [&](int sb, auto has_prev, auto has_next,
                           auto masked)
          __attribute__((always_inline)) {
        constexpr bool HP = decltype(has_prev)::value;
        constexpr bool HN = decltype(has_next)::value;
        const f32x16 cs = ns, cdp = ndp;
        mbf16x8 qf[8], of[8];   // chain fragments of sb+1
        mbf16x8 tf[16];         // accumulate fragments of sb-1
        f32x4 lv[4], dl[4];
        // stage A: the reads of the first chunk pair (C-layout rows
        // 8j + 4*hi + 0..3 of lse/delta are 16 B runs), and the export of
        // the previous sub-tile's dS
        if (HN) {
          qf[0] = kf_read(1, sb + 1, 0);
          of[0] = kf_read(0, sb + 1, 0);
        }
        lv[0] = *(const f32x4*)(lse_l + 32 * sb);
        dl[0] = *(const f32x4*)(del_l + 32 * sb);
        if (HP) {
          tf[0] = acc_frag(sb - 1, 0);
          tf[1] = acc_frag(sb - 1, 1);
          export_ds(sb - 1, d0, d1);
        }
        __builtin_amdgcn_sched_barrier(0);

        // The compiler waits for LDS data with lgkmcnt(0) only, so a wait
        // drains every read in flight.  The reads therefore go out once
        // per PAIR of chunks, for the next pair, right behind the pair's
        // first MFMA — the one place where the wait for this pair's own
        // operands sits — and have two chunks (four MFMAs) to land.
        auto pair_reads = [&](int r) __attribute__((always_inline)) {
          const int n = r + 2;   // first chunk of the next pair
          if (n < 16) {
            if (HN) {
              qf[n >> 1] = kf_read(1, sb + 1, n >> 1);
              of[n >> 1] = kf_read(0, sb + 1, n >> 1);
            }
            if (HP) {
              tf[n] = acc_frag(sb - 1, n);
              tf[n + 1] = acc_frag(sb - 1, n + 1);
            }
            if (!(n & 3)) {
              lv[n >> 2] = *(const f32x4*)(lse_l + 32 * sb + 2 * n);
              dl[n >> 2] = *(const f32x4*)(del_l + 32 * sb + 2 * n);
            }
          }
        };
        float cp[16], cd[16];
        unsigned int pp[8], pd[8];   // packed bf16 pairs of cp / cd
        f32x16 s_n = {}, dp_n = {};
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (HN) {
            if (r & 1) {
              dp_n = mfma32(of[r >> 1], vfrag[r >> 1], dp_n);
            } else {
              s_n = mfma32(qf[r >> 1], kfrag[r >> 1], s_n);
              __builtin_amdgcn_sched_barrier(0);
              pair_reads(r);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          if (HP) {
            acc_mfma(r, tf[r], p0, p1, d0, d1);
            if (!HN && !(r & 1)) {
              __builtin_amdgcn_sched_barrier(0);
              pair_reads(r);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          {
            // the split kernel rounds s*sc2 before it subtracts lse (its
            // mask select sits between the two): no fused multiply-add
            // here either, or dS and P differ in the last bit
            #pragma clang fp contract(off)
            const int ql = 32 * sb + c_row(r, hi);  // q offset in tile
            float s2 = cs[r] * sc2;
            if (decltype(masked)::value) {
              const long qg = q0 + ql;
              if (qg >= S || !krow_valid || (causal && k_row > qg)) {
                s2 = -3.0e38f;
              }
            }
            const float pr =
                __builtin_amdgcn_exp2f(s2 - lv[r >> 2][r & 3]);
            cp[r] = pr;
            cd[r] = scale * pr * (cdp[r] - dl[r >> 2][r & 3]);
          }
          // The pack is inline asm, which the compiler's hazard pass does
          // not look into: packed straight behind its v_exp_f32 it reads
          // the register before the transcendental unit has written it
          // (seen on the GPU: the low lanes got the exp2 argument).  So P
          // is packed one chunk pair late, behind a sched_barrier; dS
          // comes out of an ordinary multiply and is packed at once.
          if (r & 1) {
            if (r >= 3) pp[(r >> 1) - 1] = pack_bf16x2(cp[r - 3], cp[r - 2]);
            pd[r >> 1] = pack_bf16x2(cd[r - 1], cd[r]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (HN) {
          ns = s_n;
          ndp = dp_n;
        }
        packed_to_frags_swap(pd, &d0, &d1);
        __builtin_amdgcn_sched_barrier(0);
        pp[7] = pack_bf16x2(cp[14], cp[15]);
        packed_to_frags_swap(pp, &p0, &p1);
        __builtin_amdgcn_sched_barrier(0);
      };
      auto step = [&](int sb, auto has_prev, auto has_next)
          __attribute__((always_inline)) {
        const int qs0 = q0 + 32 * sb;
        // causal masking only bites when SOME (q, k) pair in this
        // 32q x 32k(own) tile has k > q, i.e. qs0 < kw0 + 32.  The gate is
        // a wave-uniform branch around the WHOLE step, so the MFMAs and
        // the VALU stay in one block either way
        // (kw0 + 32 > S says "some lane's kv row is past S" for the whole
        // wave: the test must not be per lane, or the lanes would split
        // over both instances and run the step's MFMAs twice)
        const bool mask_tile = (causal && qs0 < kw0 + 32)
                               || (qs0 + 32 > S) || (kw0 + KBLK > S);
        pin_acc();
        if (mask_tile) {
          step_body(sb, has_prev, has_next, std::true_type{});
        } else {
          step_body(sb, has_prev, has_next, std::false_type{});
        }
      };

      pin_acc();
      // fill: the chain of sub-tile 0 runs bare.  S[q, k own] and
      // dP[q, k own]: the lane owns the k column; q rows via c_row so the
      // contraction dim of the accumulate MFMAs is the C-row dim
      {
        mbf16x8 qf[8], of[8];
        #pragma unroll
        for (int c = 0; c < 2; ++c) {
          qf[c] = kf_read(1, 0, c);
          of[c] = kf_read(0, 0, c);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 s = {}, dp = {};
        #pragma unroll
        for (int c = 0; c < 8; ++c) {
          s = mfma32(qf[c], kfrag[c], s);
          if (!(c & 1) && c + 2 < 8) {
            // behind the wait of this group of four: the next group's
            __builtin_amdgcn_sched_barrier(0);
            #pragma unroll
            for (int n = c + 2; n < c + 4; ++n) {
              qf[n] = kf_read(1, 0, n);
              of[n] = kf_read(0, 0, n);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          dp = mfma32(of[c], vfrag[c], dp);
        }
        ns = s;
        ndp = dp;
        __builtin_amdgcn_sched_barrier(0);
      }
      pin_acc();
      step(0, std::false_type{}, std::true_type{});
      #pragma unroll
      for (int sb = 1; sb < NS - 1; ++sb) {
        step(sb, std::true_type{}, std::true_type{});
      }
      step(NS - 1, std::true_type{}, std::false_type{});
      // drain: the accumulation of the last sub-tile runs bare, its
      // fragment reads in groups of four, one group ahead
      {
        mbf16x8 tf[16];
        #pragma unroll
        for (int i = 0; i < 4; ++i) tf[i] = acc_frag(NS - 1, i);
        export_ds(NS - 1, d0, d1);
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int i = 0; i < 16; ++i) {
          acc_mfma(i, tf[i], p0, p1, d0, d1);
          __builtin_amdgcn_sched_barrier(0);
          if (!(i & 3) && i + 4 < 16) {
            #pragma unroll
            for (int n = i + 4; n < i + 8; ++n) tf[n] = acc_frag(NS - 1, n);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }

    if (has_next) {
      // own glds of the nxt tiles (and the lse/delta register) done.
      // vmcnt counts stores too, in issue order: when this tile exported,
      // its last two stores are younger than every load, so the wait may
      // leave those two in flight
      if (n_ds) {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // (the compiler still guards lse_reg with a vmcnt(0) of its own in
      // front of this write — it cannot count the conditional stores —
      // so for now the two stores are drained here after all; they have
      // had the 12 MFMAs behind the export to complete)
      store_lse(lse_nxt, lse_reg);
      // ONE barrier per tile publishes everything: a bare s_barrier
      // behind lgkmcnt(0) (the lse/delta write above), without the fence
      // of a __syncthreads, which drains vmcnt to 0 by itself
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      lse_nxt ^= 1;
      char* tp;
      tp = qn_c; qn_c = qn_n; qn_n = tp;
      tp = don_c; don_c = don_n; don_n = tp;
    }
  }

  // store via LDS transpose (8-B global writes); wave-private f32 region,
  // once per output
  __syncthreads();
  float* tr = (float*)smem + wave * (32 * 36);
  if (wave_active) {
    #pragma unroll
    for (int o = 0; o < 2; ++o) {
      unsigned short* out = o ? dk : dv;
      #pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        __syncthreads();
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          tr[c_row(r, hi) * 36 + kr] = o ? acck[dt][r] : accv[dt][r];
        }
        __syncthreads();
        #pragma unroll
        for (int rep = 0; rep < 4; ++rep) {
          const int kk = kr;
          const int d0 = (hi ? 16 : 0) + rep * 4;
          if (kw0 + kk < S) {
            bf16x4_raw w;
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
              w[j] = (short)f32_to_bf16(tr[kk * 36 + d0 + j]);
            }
            *(bf16x4_raw*)(out + ((long)b * S + kw0 + kk) * out_rs +
                           (long)hkv * HD + dt * 32 + d0) = w;
          }
        }
      }
    }
  } else {
    #pragma unroll
    for (int i = 0; i < 16; ++i) __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
// Block map of attn_fwd_kernel: 0 = map_block_fwd ("legacy"),
// 1 = balanced (unit-adjacent, heaviest first), 2 = unit-adjacent with
// tiles ascending.  Initial value from TORCHX_AMD_FWD_MAP, read once; the
// setter switches it at run time so one process can run all of them.
#define ATTN_FWD_MAP_DEFAULT 1
static int g_fwd_map = -1;

extern "C" int attn_fwd_map_get() {
  if (g_fwd_map < 0) {
    const char* e = getenv("TORCHX_AMD_FWD_MAP");
    g_fwd_map = !e ? ATTN_FWD_MAP_DEFAULT
              : strcmp(e, "legacy") == 0 ? 0
              : strcmp(e, "balanced") == 0 ? 1
              : strcmp(e, "adjacent") == 0 ? 2 : ATTN_FWD_MAP_DEFAULT;
  }
  return g_fwd_map;
}

extern "C" void attn_fwd_map_set(int map) {
  g_fwd_map = (map >= 0 && map <= 2) ? map : ATTN_FWD_MAP_DEFAULT;
}

extern "C" void attn_fwd_launch(const void* q, const void* k, const void* v,
                                void* o, void* lse, int B, int S, int Hq,
                                int Hkv, float scale, int causal,
                                long q_rs, long kv_rs, hipStream_t stream) {
  const int nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  const int map = attn_fwd_map_get();
  // the balanced maps' fallback rounds the grid up to whole rounds of 8
  // units of G blocks (map_block_fwd_balanced)
  long grid = (long)B * Hq * nqt;
  if (map != 0 && ((B * Hkv) & 7) != 0) {
    grid = ((long)B * Hkv * nqt + 7) / 8 * 8 * (Hq / Hkv);
  }
  hipLaunchKernelGGL(attn_fwd_kernel, dim3((unsigned)grid), dim3(256), 0,
                     stream, (const unsigned short*)q,
                     (const unsigned short*)k, (const unsigned short*)v,
                     (unsigned short*)o, (float*)lse, B, S, Hq, Hkv, scale,
                     causal, q_rs, kv_rs, map);
}

extern "C" void paged_prefill_attn_launch(
    const void* q, const void* kpool, const void* vpool, void* o,
    const void* bt, const void* ctx, int B, int S, int Hq, int Hkv,
    int num_pages, int logP, int M, float scale, hipStream_t stream) {
  const int nqt = (S + 4 * QBLK - 1) / (4 * QBLK);
  hipLaunchKernelGGL(paged_prefill_attn_kernel, dim3(B * Hq * nqt), dim3(256),
                     0, stream, (const unsigned short*)q,
                     (const unsigned short*)kpool,
                     (const unsigned short*)vpool, (unsigned short*)o,
                     (const int*)bt, (const int*)ctx, B, S, Hq, Hkv,
                     num_pages, logP, M, scale);
}

extern "C" void paged_prefill_attn_ragged_launch(
    const void* q, const void* kpool, const void* vpool, void* o,
    const void* bt, const void* ctx, const void* tiles, int ntiles, int B,
    int T, int Hq, int Hkv, int num_pages, int logP, int M, float scale,
    hipStream_t stream) {
  // whole rounds of 8 units, G blocks each (see the kernel's block map)
  const long units = (long)ntiles * Hkv;
  const long grid = (units + 7) / 8 * 8 * (Hq / Hkv);
  hipLaunchKernelGGL(paged_prefill_attn_ragged_kernel, dim3((unsigned)grid),
                     dim3(256), 0, stream, (const unsigned short*)q,
                     (const unsigned short*)kpool,
                     (const unsigned short*)vpool, (unsigned short*)o,
                     (const int*)bt, (const int*)ctx, (const int4*)tiles,
                     ntiles, B, T, Hq, Hkv, num_pages, logP, M, scale);
}

// dK/dV implementation of the backward: 1 = merged (one wave accumulates
// both outputs), 0 = split (the 8-wave dV/dK role pairs, kept as the
// comparison build).  Initial value from TORCHX_AMD_DKV_IMPL, read once;
// the setter switches it at run time so one process can run both.
static int g_dkv_merged = -1;

extern "C" int attn_bwd_dkv_impl_get() {
  if (g_dkv_merged < 0) {
    const char* e = getenv("TORCHX_AMD_DKV_IMPL");
    g_dkv_merged = (e && strcmp(e, "split") == 0) ? 0 : 1;
  }
  return g_dkv_merged;
}

extern "C" void attn_bwd_dkv_impl_set(int merged) {
  g_dkv_merged = merged ? 1 : 0;
}

// ds: the dS scratch (attn_bwd_ds_bytes) selects the streamed dQ kernel;
// null selects the recompute dQ kernel and the dkv kernel exports nothing.
// Order pre -> dkv -> dq: the streamed dQ consumes what dkv wrote.
extern "C" void attn_bwd_launch(const void* q, const void* k, const void* v,
                                const void* o, const void* dout,
                                const void* lse, void* delta, void* dq,
                                void* dk, void* dv, void* ds, int B, int S,
                                int Hq, int Hkv, float scale, int causal,
                                long q_rs, long kv_rs, long dqkv_q_rs,
                                long dqkv_kv_rs, hipStream_t stream) {
  const long rows = (long)B * S * Hq;
  hipLaunchKernelGGL(attn_bwd_pre_kernel, dim3((int)((rows + 15) / 16)),
                     dim3(256), 0, stream, (const unsigned short*)dout,
                     (const unsigned short*)o, (float*)delta, rows, S, Hq);
  const int nkt = (S + BLOCK_K - 1) / BLOCK_K;
  const long dout_rs = (long)Hq * HD;
  // 128-row q tiles measured +4% over 64 (fewer barriers/iterations beat
  // the 2-blocks/CU the 64-row variant's smaller LDS allows)
  static int dkv_fkv = -1;
  if (dkv_fkv < 0) {
    const char* e = getenv("TORCHX_AMD_DKV_FKV");
    dkv_fkv = (e && atoi(e) == 64) ? 64 : 128;
  }
  // the merged and the split (8-wave) kernels take the same arguments
  auto launch_dkv = [&](auto kernel, int threads) {
    hipLaunchKernelGGL(kernel, dim3(B * Hkv * nkt), dim3(threads), 0, stream,
                       (const unsigned short*)q, (const unsigned short*)k,
                       (const unsigned short*)v, (const unsigned short*)dout,
                       (const float*)lse, (const float*)delta,
                       (unsigned short*)dk, (unsigned short*)dv, (char*)ds,
                       B, S, Hq, Hkv, scale, causal, q_rs, kv_rs, dout_rs,
                       dqkv_kv_rs);
  };
  const bool dkv128 = dkv_fkv == 128 && S % 128 == 0;
  if (attn_bwd_dkv_impl_get() == 1) {
    if (dkv128) launch_dkv(attn_bwd_dkv_merged_kernel<128>, 256);
    else launch_dkv(attn_bwd_dkv_merged_kernel<64>, 256);
  } else {
    if (dkv128) launch_dkv(attn_bwd_dkv_kernel<128>, 512);
    else launch_dkv(attn_bwd_dkv_kernel<64>, 512);
  }
  const int nqt = (S + BLOCK_Q - 1) / BLOCK_Q;
  if (ds != nullptr) {
    // the longest (last) q tiles launch first: measured -0.8% on the whole
    // backward at S=8192 and level at S=4096 against ascending order;
    // TORCHX_AMD_DQ_HEAVY_FIRST=0 restores ascending for re-measurement
    static int heavy_first = -1;
    if (heavy_first < 0) {
      const char* e = getenv("TORCHX_AMD_DQ_HEAVY_FIRST");
      heavy_first = (e && atoi(e) == 0) ? 0 : 1;
    }
    hipLaunchKernelGGL(attn_bwd_dq_stream_kernel, dim3(B * Hq * nqt),
                       dim3(256), 0, stream, (const unsigned short*)k,
                       (const char*)ds, (unsigned short*)dq, B, S, Hq, Hkv,
                       causal, kv_rs, dqkv_q_rs, heavy_first);
    return;
  }
  static int dq_fkv = -1;
  if (dq_fkv < 0) {
    const char* e = getenv("TORCHX_AMD_DQ_FKV");
    dq_fkv = (e && atoi(e) == 128) ? 128 : 64;
  }
  auto launch_dq = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B * Hq * nqt), dim3(256), 0, stream,
                       (const unsigned short*)q, (const unsigned short*)k,
                       (const unsigned short*)v, (const unsigned short*)dout,
                       (const float*)lse, (const float*)delta,
                       (unsigned short*)dq, B, S, Hq, Hkv, scale, causal,
                       q_rs, kv_rs, dqkv_q_rs);
  };
  if (dq_fkv == 128 && S % 128 == 0) launch_dq(attn_bwd_dq_kernel<128>);
  else launch_dq(attn_bwd_dq_kernel<64>);
}
