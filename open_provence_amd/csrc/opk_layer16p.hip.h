// opk_layer16p.hip.h -- the whole-layer kernel as WAVE PAIRS (hidden = 256, single-pass operands), 16x16x32 MFMAs
#pragma once

#include "opk_layer32.hip.h"  // Layer32Params

namespace opk {

// ----------------------------------------------------------------------------------------------
// One launch per layer, the arithmetic of rowgemm_kernel<.., RP_MLP, ..> (opk_rowgemm.hip.h):
//   x += o Wo^T ; LayerNorm ; x += GeGLU(LN(x) Wi^T) Wo^T with h on chip ; LayerNorm ; the next layer's q / k / v^T
// Why another form (round 6).  Every phase of this launch is bound by instruction ISSUE and by the board's POWER limit, not by
// HBM (with every HBM stream removed the 8 x 16 form is 6 % shorter: profiles/r06_exp_stagger_memfree.txt) and not by the
// matrix pipe (busy 40 % of the cycles; the chip holds 1.8 - 1.95 of its 2.4 GHz under these kernels, 2.17 on all-zero data).
// What the forms so far pay per 16 cycles of matrix work:
//   8 waves x 16 rows (two waves per SIMD):  one MFMA + ONE 1 KiB weight-fragment read from LDS (a fragment serves one MFMA)
//                                            + 1.7 vector instructions of GeGLU + ~1.5 of moves / waits / nops;
//   4 waves x 32 rows (one wave per SIMD, 512 registers): half the fragment reads, but nothing fills the wave's own stalls.
// Two waves per SIMD AND 32 rows per wave needs ~300 of the 256 registers -- because a wave holds all 256 output features
// of its rows (128 accumulators).  Here the two waves of a pair SHARE one 32-row tile and split the OUTPUT FEATURES of every
// contraction:
//   wave (pw, hf), pw = row tile 0..3 of the 128-row block, hf = half 0 / 1
//   attention-output projection, MLP output projection:  output tiles 4 hf .. 4 hf + 3 of 8     (64 accumulators)
//   Wi:  tile 2 t + hf of pair step t (16 h-columns + their gates)                              (16 accumulators, x 2 for the pipeline)
//   next q / k / v^T:  tile 2 it + hf of pair step it
// A weight fragment (16 features x 32 k, 1 KiB) is read from LDS by ONE wave and multiplied against BOTH 16-row halves of the
// tile: half the LDS reads per flop of the 8 x 16 form at the same two waves per SIMD.  (The same split on 32x32x16 MFMAs
// -- half the MFMA instructions again -- was built first and measured: 12 % fewer cycles, but that shape draws so much more
// power per flop that the chip clocks 8 % lower under it: profiles/r06_pair_kernel_steps.txt.)  What a wave lacks of its rows
// comes from its partner through LDS: the other half of each h fragment (8 bytes per lane and 16 rows per pair step, consumed
// one step later so that the block's single barrier per step orders it), and after each LayerNorm the partner's normalised
// fragments (8 KiB per wave), the row statistics combined from the halves' (mean, M2) by the parallel-variance formula.
//
// Register layout (v_mfma_f32_16x16x32): lane = (n16 = lane % 16, g = lane / 16); the wave's rows are m0 + 16 mf + n16, mf = 0, 1.
//   "swapped" products (weights = X operand, token rows = Y): D[fh][mf] of a 32-feature tile: lane (n16, g) holds slots
//   16 fh + 4 g + r (r = 0..3) of row 16 mf + n16.  l16p_source_row() permutes the weight rows so that a lane's 8 slots of a
//   tile are the 8 consecutive k = 32 T + 8 g + (0..7) it needs as the Y operand of the next contraction (k-pair T), a GeGLU
//   input beside its gate (fh = 0 / 1), or a RoPE pair (d, d + 32).  Operand layouts in memory are the other kernels' own:
//   o, q, k as 1 KiB pieces [row/16][C/32][plane][16 (k%32/8) + row%16][8] (= one Y fragment), v^T as
//   [head][row/32][plane][4][16 kg + d'][8 keys]; x as fp32 rows, or TILED between two launches of this kernel (XIN_T / XOUT_T:
//   the 32 x 32 values of a row tile x feature tile as four 1 KiB pieces [2 mf + fh][lane][4 floats], so that every load / store
//   moves one contiguous KiB -- rows cost 16 bytes per lane in 16 different cache lines per instruction).
// K order: a wave multiplies its OWN four k-pairs first, then its partner's: a feature's summation order depends on the
// feature only, never on where a row sits in the block.
// ----------------------------------------------------------------------------------------------

enum Layer16pPack { L16_RESID = 0, L16_GEGLU = 1, L16_QKV = 2 };

// source row of slot m (0..31; fh = m / 16, rho = m % 16 = 4 g + r) of 32-row tile T of a weight matrix
__host__ __device__ inline int l16p_source_row(int mode, int T, int m, int H, int I) {
  const int fh = m >> 4, rho = m & 15, g = rho >> 2, r = rho & 3;
  if (mode == L16_RESID) return 32 * T + 8 * g + 4 * fh + r;
  if (mode == L16_GEGLU) {  // tile 2t + hf: h columns 32 t + 8 g + 4 hf + r (fh = 0) and their gates (fh = 1)
    const int col = 32 * (T >> 1) + 8 * g + 4 * (T & 1) + r;
    return fh ? I + col : col;
  }
  const int per = H / 32;  // tiles in each of q, k, v
  if (T < 2 * per) {       // q / k: 16 d of a head (fh = 0) and their RoPE partners d + 32 (fh = 1)
    const int blk = T / per, cc = T % per;
    return blk * H + (cc >> 1) * HEAD_DIM + 16 * (cc & 1) + 4 * g + r + 32 * fh;
  }
  // v (tokens x features orientation): column rho of fragment fh is feature slot (piece n = 2 (cv & 1) + fh, d' = rho) of the
  // transposed layout, in the d order of rowgemm_source_row (the attention output then is lane-contiguous)
  const int cv = T - 2 * per;
  return 2 * H + (cv >> 1) * HEAD_DIM + 32 * (cv & 1) + 8 * (rho >> 2) + 4 * fh + (rho & 3);
}

#ifdef OPK_PACK_KERNELS
// one plane.  chunk-major: dst[T][kp][fh][lane][8], k-major: dst[kp][T][fh][lane][8]; lane (rho, gk) holds k = 32 kp + 8 gk + e
__global__ void pack_layer16p_kernel(const float* __restrict__ src, int n_rows, int K, int mode, int kmajor, int H, int I,
                                     u16* __restrict__ dst, int f16) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n_rows * K) return;
  const int KP = K / 32, NTL = n_rows / 32;
  size_t t = idx;
  const int e = (int)(t & 7); t >>= 3;
  const int l = (int)(t & 63); t >>= 6;
  const int fh = (int)(t & 1); t >>= 1;
  int T, kp;
  if (kmajor) {
    T = (int)(t % NTL);
    kp = (int)(t / NTL);
  } else {
    kp = (int)(t % KP);
    T = (int)(t / KP);
  }
  const int row = l16p_source_row(mode, T, 16 * fh + (l & 15), H, I);
  const float v = src[(size_t)row * K + 32 * kp + 8 * (l >> 4) + e];
  dst[idx] = f16 ? f2h(v) : f2bf(v);
}
#endif

template <bool H16>
__device__ __forceinline__ uint32_t pack2x(float a, float b) {
  if constexpr (H16) return pack_f16x2(a, b);
  else return pack_bf16x2(a, b);
}

__device__ __forceinline__ void lds_write_frag(uint32_t lds_addr, const bf16x8& v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(lds_addr), "v"(v) : "memory");
}
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lds_write_u2(uint32_t lds_addr, uint32_t lo, uint32_t hi) {  // (an ext-vector operand: a 64-bit register pair)
  const u32x2 v = {lo, hi};
  asm volatile("ds_write_b64 %0, %1" ::"v"(lds_addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write_f2(uint32_t lds_addr, const f32x2& v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(lds_addr), "v"(v) : "memory");
}
__device__ __forceinline__ f32x2 lds_read_f2(uint32_t lds_addr) {
  f32x2 v;
  asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_addr) : "memory");
  return v;
}
// s_barrier with the compiler fenced on both sides: the bare builtin is "no memory" to the optimizer, which then moves LDS
// reads, plain loads and the LDS-DMA intrinsic across it (seen: nondeterministic q / k / v^T of one row half until a
// sequence point was added in front of the second LayerNorm -- profiles/r06_pair_kernel_steps.txt)
__device__ __forceinline__ void block_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
template <int N>
__device__ __forceinline__ void lds_wait3(bf16x8& a, bf16x8& b, bf16x8& c) {
  asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(N));
}
__device__ __forceinline__ void store_stream8(void* dst, const uint2& v) {
  typedef unsigned int u32x2_nt __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store(u32x2_nt{v.x, v.y}, reinterpret_cast<u32x2_nt*>(dst));
}

// A stream of NSTEPS steps of NF (2 or 3) weight fragments each; fragment j of step s is at LDS byte offset Off::at(s, j)
// from address register Off::base(s, j) of `addr` (a wave's fragments sit behind up to NB wave-dependent bases); requested
// DEPTH steps ahead into DEPTH + 1 rotating register sets, waited for by count (frag_stream2 of opk_common.hip.h).
template <int NSTEPS, int NF, int DEPTH, class Off, int NB, class Body>
__device__ __forceinline__ void frag_stream_m(const uint32_t (&addr)[NB], Body&& body) {
  static_assert(NF == 2 || NF == 3, "two or three fragments per step");
  constexpr int SETS = DEPTH + 1;
  bf16x8 w[SETS][NF];
  auto read_group = [&](auto step_tag) {
    constexpr int s = decltype(step_tag)::value;
    static_for<NF>([&](auto j_tag) {
      constexpr int j = decltype(j_tag)::value;
      w[s % SETS][j] = lds_read_frag<Off::at(s, j)>(addr[Off::base(s, j)]);
    });
  };
  static_for<(DEPTH + 1 < NSTEPS ? DEPTH + 1 : NSTEPS)>([&](auto t) { read_group(t); });
  static_for<NSTEPS>([&](auto t) {
    constexpr int s = decltype(t)::value;
    constexpr int set = s % SETS;
    constexpr int ahead = (NSTEPS - 1 - s) < DEPTH ? (NSTEPS - 1 - s) : DEPTH;
    if constexpr (NF == 2) lds_wait2<2 * ahead>(w[set][0], w[set][1]);
    else lds_wait3<3 * ahead>(w[set][0], w[set][1], w[set][2]);
    body(t, w[set]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (s + DEPTH + 1 < NSTEPS) read_group(std::integral_constant<int, s + DEPTH + 1>{});
  });
}

// NT = hidden / 32 (8).  QKV: the next layer's q / k / v^T follow (false: the last layer).  H16: fp16 operands (kernel set "f16").
template <int NT, bool QKV, bool H16, bool XIN_T = false, bool XOUT_T = false>
__global__ __launch_bounds__(512, 2) void layer16p_kernel(Layer32Params p) {
  constexpr bool HOUT = false;
#include "opk_layer16p_body.inc"
}

// A forward with a hidden-state request (QKV only): the same launch, whose new residual rows also go, in token order, to the
// entry of the request (Layer32Params::hid_out; padding rows skipped) beside the residual stream's own store.  The body is
// shared text, so that layer16p_kernel's instantiations compile exactly as before.
template <int NT, bool QKV, bool H16, bool XIN_T = false, bool XOUT_T = false>
__global__ __launch_bounds__(512, 2) void layer16p_hout_kernel(Layer32Params p) {
  constexpr bool HOUT = true;
#include "opk_layer16p_body.inc"
}

}  // namespace opk
