// opk_assemble.hip.h -- op_assemble_rows: the `prefix + query + middle + context + suffix` rows of a prepared request,
// laid out on the device from a resident corpus of fragment token ids.  Memory-bound and tiny next to a forward: plain
// C++ copies, a wave per row segment, 16-byte stores (and loads, where the source lines up) inside a copy, element
// accesses at its ends.  No LDS, no atomics.  Every index the kernel reads from device memory -- the row plan, the
// offsets -- is held inside the buffers' sizes before it addresses anything: a store lands in the row's own
// [cu[row], cu[row + 1]) within [0, total), a load inside its source buffer, whatever the plan holds.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace opk {

constexpr int ASSEMBLE_MAX_PIECE = 8;  // = OP_ASSEMBLE_MAX_PIECE: ids per template piece
constexpr int ASSEMBLE_SEGMENTS = 3;   // waves per row: the pieces + the query, the first context copy, the second
constexpr int ASSEMBLE_PLAN_WORDS = 4; // int32 words per row of the plan: query, first_frag, n_frag, clip

struct AssemblePieces {  // by value in the kernel's arguments
  int32_t prefix[ASSEMBLE_MAX_PIECE], middle[ASSEMBLE_MAX_PIECE], suffix[ASSEMBLE_MAX_PIECE];
  int32_t n_prefix, n_middle, n_suffix;
};

// One wave copies src[s0, s0 + len) to dst[d0, d0 + len), cut to what lies inside src[0, n_src) and dst[0, d_hi) (d0 >= 0).
// Element stores up to the first 16-byte boundary of dst, int4 stores from there (one int4 load when the source lines up
// with them, four element loads otherwise), element stores for the last len % 4.
__device__ __forceinline__ void assemble_copy_run(const int32_t* __restrict__ src, int s0, int len, int n_src, int32_t* __restrict__ dst,
                                                  long long d0, int d_hi, int lane) {
  if (s0 < 0 || s0 >= n_src || d0 < 0 || d0 >= (long long)d_hi) return;
  if (len > n_src - s0) len = n_src - s0;
  if ((long long)len > (long long)d_hi - d0) len = (int)((long long)d_hi - d0);
  if (len <= 0) return;
  const int32_t* s = src + (size_t)s0;
  int32_t* d = dst + (size_t)d0;
  const uintptr_t d_addr = reinterpret_cast<uintptr_t>(d);
  int head = len;  // (a dst that is not 4-byte aligned never meets a 16-byte boundary: element stores throughout)
  if ((d_addr & 3) == 0) {
    head = (int)(((16 - (d_addr & 15)) & 15) >> 2);
    if (head > len) head = len;
  }
  for (int i = lane; i < head; i += 64) d[i] = s[i];
  const int n_vec = (len - head) >> 2;
  const bool src_wide = (reinterpret_cast<uintptr_t>(s + head) & 15) == 0;
  for (int v = lane; v < n_vec; v += 64) {
    const int p = head + 4 * v;
    int4 x;
    if (src_wide) {
      x = *reinterpret_cast<const int4*>(s + p);
    } else {
      x.x = s[p], x.y = s[p + 1], x.z = s[p + 2], x.w = s[p + 3];
    }
    *reinterpret_cast<int4*>(d + p) = x;
  }
  for (int i = head + 4 * n_vec + lane; i < len; i += 64) d[i] = s[i];
}

// A wave per (row, segment), 4 waves per block.  Segment 0: prefix, query, middle and -- behind the context -- suffix.
// Segment 1: the context, or for a clipped row the first `clip` tokens of its first fragment.  Segment 2: a clipped row's
// further fragments.  A row's fragments are consecutive in the corpus, so each segment is one contiguous copy.  A row with
// n_frag = 0 has no context; with clip = -1 it has no suffix either (a pair whose second sequence is empty).
__global__ __launch_bounds__(256) void assemble_rows_kernel(const int32_t* __restrict__ corpus, const int32_t* __restrict__ frag_off, int n_frag,
                                                            int n_corpus, const int32_t* __restrict__ query_ids,
                                                            const int32_t* __restrict__ q_off, int n_queries, int n_query_tokens,
                                                            AssemblePieces pc, const int32_t* __restrict__ plan,
                                                            const int32_t* __restrict__ cu, int n_rows, int total, int32_t* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63);
  const long long wave = (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6);
  const int row = (int)(wave / ASSEMBLE_SEGMENTS);
  const int seg = (int)(wave - (long long)row * ASSEMBLE_SEGMENTS);
  if (row >= n_rows) return;
  int lo = cu[row], hi = cu[row + 1];
  if (lo < 0) lo = 0;
  if (hi > total) hi = total;
  if (hi <= lo) return;
  const int32_t* pr = plan + (size_t)row * ASSEMBLE_PLAN_WORDS;
  const int query = pr[0], first = pr[1], n = pr[2], clip = pr[3];
  if (query < 0 || query >= n_queries || first < 0 || n < 0 || first > n_frag - n) return;
  int q0 = q_off[query], q1 = q_off[query + 1];
  if (q0 < 0) q0 = 0;
  if (q1 > n_query_tokens) q1 = n_query_tokens;
  const int q_len = q1 > q0 ? q1 - q0 : 0;
  const int head_len = pc.n_prefix + q_len + pc.n_middle;
  const int n_suffix = (n == 0 && clip < 0) ? 0 : pc.n_suffix;  // a row without context may end behind `middle`

  // the context: [a0, a0 + a_len) then [b0, b0 + b_len) of the corpus
  int a0 = 0, a_len = 0, b0 = 0, b_len = 0;
  if (n > 0) {
    a0 = frag_off[first];
    const int first_end = frag_off[first + 1], last_end = frag_off[first + n];
    if (clip > 0) {
      a_len = first_end - a0 < clip ? first_end - a0 : clip;
      b0 = first_end;
      b_len = last_end - first_end;
    } else {
      a_len = last_end - a0;
    }
    if (a_len < 0) a_len = 0;
    if (b_len < 0) b_len = 0;
  }

  if (seg == 0) {
    const long long ctx_len = (long long)a_len + b_len;
    for (int i = lane; i < head_len + n_suffix; i += 64) {
      int value;
      long long at = i;  // position within the row
      if (i < pc.n_prefix) {
        value = pc.prefix[i];
      } else if (i < pc.n_prefix + q_len) {
        value = query_ids[(size_t)q0 + (size_t)(i - pc.n_prefix)];
      } else if (i < head_len) {
        value = pc.middle[i - pc.n_prefix - q_len];
      } else {
        value = pc.suffix[i - head_len], at += ctx_len;
      }
      if (at < (long long)(hi - lo)) out[(size_t)lo + (size_t)at] = value;
    }
  } else if (seg == 1) {
    assemble_copy_run(corpus, a0, a_len, n_corpus, out, (long long)lo + head_len, hi, lane);
  } else if (b_len > 0) {
    assemble_copy_run(corpus, b0, b_len, n_corpus, out, (long long)lo + head_len + a_len, hi, lane);
  }
}

}  // namespace opk
