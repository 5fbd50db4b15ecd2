// opk_decide.hip.h -- the last host stages of a prepared request on the device: op_planned_fragment_means (the mean
// keep-probability of every fragment of every row, its token range derived from the row plan op_assemble_rows laid the row out
// from), op_located_fragment_means (the same with the context looked up in the assembled row first, as the reference looks it
// up: at most head_len x n_ctx id compares per row) and op_sentence_decisions (per context: the sentences' averages over their
// fragments, the threshold, the title rule).
// Tiny next to a forward: plain C++, vector stores only, no LDS, no atomics.  Every index the kernels read from device memory
// -- the row plan, the offsets, the slot table, the instance table -- is held inside the buffers' sizes before it addresses
// anything, as in opk_assemble.hip.h: a load lands inside its source buffer, a store inside the output, whatever the tables hold.
// Every loop is bounded by a length from the plan, clamped; nothing waits on memory another thread writes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opk_pairwise.hip.h"

namespace opk {

constexpr int DECIDE_PLAN_WORDS = 4;      // = ASSEMBLE_PLAN_WORDS: query, first_frag, n_frag, clip
constexpr int DECIDE_INSTANCE_WORDS = 6;  // = OP_DECISIONS_INSTANCE_WORDS: slot_begin, slot_end, sent_out_begin, n_sentences, item_sent_base, title_index

struct PlannedMeansParams {  // by value in the kernel's arguments
  const float* keep_prob;     // [total]
  const int32_t* frag_off;    // [n_frag + 1]
  const int32_t* frag_shift;  // [n_frag]
  const int32_t* q_off;       // [n_queries + 1]
  const int32_t* plan;        // [n_rows][4]
  const int32_t* cu;          // [n_rows + 1]
  const int32_t* slot_off;    // [n_rows + 1]
  float* mean_out;            // [n_slots]
  int32_t* slot_frag_out;     // [n_slots]
  int n_frag, n_queries, n_query_tokens, n_rows, total, n_slots;
  int n_prefix, n_middle;
};

// A wave per row, a lane per fragment (lane, lane + 64, ...).  Fragment j of the row = fragment f = first_frag + j of the corpus:
// its tokens start behind prefix + query + middle and the fragments before it (the first one cut to `clip` ids when clip > 0),
// the range is shifted left by frag_shift[f] (the title tokens in front of its sentence) and clamped to the row -- the
// arithmetic of pipeline.fragment_token_ranges -- and averaged as segment_mean_kernel averages: numpy's float32 pairwise sum,
// divided in float64, rounded to float32; 1.0 for an empty range.
__global__ __launch_bounds__(256) void planned_fragment_means_kernel(PlannedMeansParams p) {
  const int lane = (int)(threadIdx.x & 63);
  const long long wave = (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6);
  if (wave >= (long long)p.n_rows) return;
  const int row = (int)wave;
  int lo = p.cu[row], hi = p.cu[row + 1];
  if (lo < 0) lo = 0;
  if (hi > p.total) hi = p.total;
  const int row_len = hi > lo ? hi - lo : 0;
  const int32_t* pr = p.plan + (size_t)row * DECIDE_PLAN_WORDS;
  const int query = pr[0], first = pr[1], n = pr[2], clip = pr[3];
  if (query < 0 || query >= p.n_queries || first < 0 || n <= 0 || first > p.n_frag - n) return;
  int q0 = p.q_off[query], q1 = p.q_off[query + 1];
  if (q0 < 0) q0 = 0;
  if (q1 > p.n_query_tokens) q1 = p.n_query_tokens;
  const int q_len = q1 > q0 ? q1 - q0 : 0;
  const long long head_len = (long long)p.n_prefix + q_len + p.n_middle;
  const long long slot0 = p.slot_off[row];
  const long long first_off = p.frag_off[first], first_end = p.frag_off[first + 1];
  const long long first_len = clip > 0 ? (long long)clip : first_end - first_off;
  for (int j = lane; j < n; j += 64) {
    const long long slot = slot0 + j;
    if (slot < 0 || slot >= (long long)p.n_slots) continue;
    const int f = first + j;
    const long long f0 = p.frag_off[f], f1 = p.frag_off[f + 1];
    const long long len = j == 0 ? first_len : f1 - f0;
    // (fragments are consecutive in the corpus: those before fragment j hold first_len + frag_off[f] - frag_off[first + 1] ids)
    long long start = head_len + (j == 0 ? 0 : first_len + (f0 - first_end));
    long long end = start + len;
    const long long shift = p.frag_shift[f];
    start -= shift;
    end -= shift;
    if (start < 0) start = 0;
    if (end > (long long)row_len) end = row_len;
    float value = 1.0f;
    if (end > start) {
      const int count = (int)(end - start);
      const float sum = np_pairwise_sum_f32(p.keep_prob + (size_t)lo + (size_t)start, count);
      value = (float)((double)sum / (double)count);
    }
    p.mean_out[slot] = value;
    p.slot_frag_out[slot] = f;
  }
}

struct LocatedMeansParams {  // by value in the kernel's arguments
  PlannedMeansParams planned;
  const int32_t* ids;     // [total]: the rows op_assemble_rows laid out from the same plan
  int32_t* ctx_start_out; // [n_rows]
};

// op_located_fragment_means: planned_fragment_means_kernel with the context LOOKED UP in the row, as the reference does
// (pipeline.prepare_block_inputs: _find_subsequence(ids, ctx)) -- the first place at or left of head_len = prefix + query + middle
// where the row's whole context (n_ctx ids: the row's fragments end to end, the first one `clip` long when clip > 0, held to
// row_len - head_len) occurs.  It is left of head_len when the context also occurs in prefix + query + middle, or in those
// followed by the start of its own copy; head_len itself always matches.  A wave per row.  The search: lane-per-candidate over
// idx = 0 .. head_len - 1 in ascending passes of 64; a lane whose first id matches compares on until a mismatch; a ballot picks
// the lowest matching lane of the pass, and the first pass with a match ends the search (the branch is uniform across the wave:
// it tests the ballot).  Work per row: at most head_len x n_ctx compares.  Every read is ids[lo + k] with k < head_len + n_ctx <=
// row_len, inside the row's own [cu[row], cu[row + 1]) within [0, total).  ctx_start_out[row] = the place found; a row the
// plain kernel skips, or one without context ids, gets head_len (0 ids for a query that is not the request's) and no slots.
// The fragments' ranges, shift, clamp and mean are then the plain kernel's with head_len replaced by the place found.
__global__ __launch_bounds__(256) void located_fragment_means_kernel(LocatedMeansParams lp) {
  const PlannedMeansParams& p = lp.planned;
  const int lane = (int)(threadIdx.x & 63);
  const long long wave = (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6);
  if (wave >= (long long)p.n_rows) return;
  const int row = (int)wave;
  int lo = p.cu[row], hi = p.cu[row + 1];
  if (lo < 0) lo = 0;
  if (hi > p.total) hi = p.total;
  const int row_len = hi > lo ? hi - lo : 0;
  const int32_t* pr = p.plan + (size_t)row * DECIDE_PLAN_WORDS;
  const int query = pr[0], first = pr[1], n = pr[2], clip = pr[3];
  int q_len = 0;
  if (query >= 0 && query < p.n_queries) {
    int q0 = p.q_off[query], q1 = p.q_off[query + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > p.n_query_tokens) q1 = p.n_query_tokens;
    q_len = q1 > q0 ? q1 - q0 : 0;
  }
  const long long head_sum = (long long)p.n_prefix + q_len + p.n_middle;
  const int head_len = head_sum < (long long)INT32_MAX ? (int)head_sum : INT32_MAX;
  const bool planned = query >= 0 && query < p.n_queries && first >= 0 && n > 0 && first <= p.n_frag - n;
  long long first_off = 0, first_end = 0, first_len = 0;
  int n_ctx = 0;
  if (planned) {
    first_off = p.frag_off[first], first_end = p.frag_off[first + 1];
    first_len = clip > 0 ? (long long)clip : first_end - first_off;
    long long ctx = first_len + ((long long)p.frag_off[first + n] - first_end);
    if (ctx > (long long)row_len - head_len) ctx = (long long)row_len - head_len;
    n_ctx = ctx > 0 ? (int)ctx : 0;
  }
  int found = head_len;
  if (n_ctx > 0) {
    const int32_t* rid = lp.ids + (size_t)lo;
    const int32_t* ctx = rid + head_len;  // (head_len + n_ctx <= row_len)
    const int32_t ctx0 = ctx[0];
    for (int base = 0; base < head_len; base += 64) {
      const int idx = base + lane;
      bool match = idx < head_len && rid[idx] == ctx0;
      if (match) {
        for (int j = 1; j < n_ctx; ++j) {  // (idx + j < head_len + n_ctx)
          if (rid[idx + j] != ctx[j]) {
            match = false;
            break;
          }
        }
      }
      const unsigned long long hits = __ballot(match);
      if (hits != 0ull) {
        found = base + __builtin_ctzll(hits);
        break;
      }
    }
  }
  if (lane == 0) lp.ctx_start_out[row] = found;
  if (n_ctx <= 0) return;
  const long long slot0 = p.slot_off[row];
  for (int j = lane; j < n; j += 64) {
    const long long slot = slot0 + j;
    if (slot < 0 || slot >= (long long)p.n_slots) continue;
    const int f = first + j;
    const long long f0 = p.frag_off[f], f1 = p.frag_off[f + 1];
    const long long len = j == 0 ? first_len : f1 - f0;
    long long start = (long long)found + (j == 0 ? 0 : first_len + (f0 - first_end));
    long long end = start + len;
    const long long shift = p.frag_shift[f];
    start -= shift;
    end -= shift;
    if (start < 0) start = 0;
    if (end > (long long)row_len) end = row_len;
    float value = 1.0f;
    if (end > start) {
      const int count = (int)(end - start);
      const float sum = np_pairwise_sum_f32(p.keep_prob + (size_t)lo + (size_t)start, count);
      value = (float)((double)sum / (double)count);
    }
    p.mean_out[slot] = value;
    p.slot_frag_out[slot] = f;
  }
}

struct DecisionsParams {  // by value in the kernel's arguments
  const int32_t* instances;  // [n_instances][6]
  const float* mean;         // [n_slots]
  const int32_t* slot_frag;  // [n_slots]
  const int32_t* frag_sent;  // [n_frag]
  double* avg_out;           // [n_out]
  uint8_t* keep_out;         // [n_out]
  double threshold;
  int n_instances, n_slots, n_frag, n_out;
};

// the corpus-wide sentence number of the fragment in `slot`; -1 where the slot names no fragment of the corpus
__device__ __forceinline__ int decide_slot_sentence(const DecisionsParams& p, int slot) {
  const int f = p.slot_frag[slot];
  return (f >= 0 && f < p.n_frag) ? p.frag_sent[f] : -1;
}

// One thread per context instance, sequential: the instance's slots are in fragment order and a sentence's fragments are
// consecutive there (the corpus is eligible: sentence_index does not decrease), so one walk over the slots meets every
// sentence's run once.  Per sentence: no value -> 0.0, one -> itself, more -> their float64 pairwise sum / n (numpy's order),
// then Python's max(0.0, min(avg, 1.0)) operand for operand (a NaN average comes out as 0.0), keep = avg > threshold; at the
// end the title rule.
__global__ __launch_bounds__(64) void sentence_decisions_kernel(DecisionsParams p) {
  const int inst = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (inst >= p.n_instances) return;
  const int32_t* in = p.instances + (size_t)inst * DECIDE_INSTANCE_WORDS;
  int slot = in[0], slot_end = in[1];
  const int out0 = in[2], n_sent = in[3], sent_base = in[4], title = in[5];
  if (slot < 0) slot = 0;
  if (slot_end > p.n_slots) slot_end = p.n_slots;
  if (out0 < 0 || n_sent <= 0 || out0 > p.n_out - n_sent) return;
  bool any = false;
  for (int k = 0; k < n_sent; ++k) {
    const long long want = (long long)sent_base + k;
    while (slot < slot_end && (long long)decide_slot_sentence(p, slot) < want) ++slot;  // (slots of no sentence of this walk)
    const int run = slot;
    while (slot < slot_end && (long long)decide_slot_sentence(p, slot) == want) ++slot;
    const int n = slot - run;
    double avg = 0.0;
    if (n == 1) avg = (double)p.mean[run];
    else if (n > 1) avg = np_pairwise_sum_f64(p.mean + run, n) / (double)n;
    const double capped = (1.0 < avg) ? 1.0 : avg;         // min(avg, 1.0): 1.0 only where it is smaller
    const double clamped = (capped > 0.0) ? capped : 0.0;  // max(0.0, capped): capped only where it is larger (NaN, -0.0 -> 0.0)
    const bool keep = clamped > p.threshold;
    any = any || keep;
    p.avg_out[(size_t)out0 + k] = clamped;
    p.keep_out[(size_t)out0 + k] = keep ? 1 : 0;
  }
  if (any && title >= 0 && title < n_sent) p.keep_out[(size_t)out0 + title] = 1;
}

}  // namespace opk
