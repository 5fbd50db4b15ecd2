// opk_loss.hip.h -- the evaluation losses of the reference's inference file on the device (op_loss): logits that a forward
// left on the device -> one fp32 scalar, optionally with the unreduced terms.  Four kinds (LOSS_*), one shape of kernel:
// every term is evaluated in fp64 from the fp32 inputs in its stable form, a thread adds its terms in the order it meets
// them, a block adds its threads in a fixed tree and writes ONE partial to the scratch block, and loss_finish_kernel (one
// block) adds the partials in index order, divides once in fp64 and rounds once to fp32.  No floating-point atomics and a
// grid that depends on the sizes only: the same inputs give the same bits on every call.  This is a side pass of a few
// hundred thousand terms at most, so the fp64 device maths functions are affordable; plain C++, no LDS beyond the block
// reduction.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace opk {

constexpr int LOSS_TOKEN_CE = 0, LOSS_RANK_BCE = 1, LOSS_RANK_CE = 2, LOSS_RANK_MSE = 3;  // = enum op_loss_kind
constexpr int LOSS_MAX_BLOCKS = 256;  // the grid's cap: blocks stride over rows beyond it
constexpr int LOSS_THREADS = 256;
constexpr uint32_t LOSS_NONE = 0xffffffffu;

// What loss_finish_kernel leaves (copied to the host for an op_loss_report).
struct LossResult {
  double sum;           // of the terms that count
  long long count;      // how many do
  long long bad_value;  // the label at bad_index
  uint32_t bad_index;   // linear index into labels of the first label outside 0 <= y < C (not ignore_index); LOSS_NONE = none
  uint32_t status;      // bit 0: there is one
  float loss;
  uint32_t reserved;
};
// The handle's scratch block: one partial per block of the first launch, then the result.  5.2 KB whatever the batch.
struct LossScratch {
  double sum[LOSS_MAX_BLOCKS];
  long long count[LOSS_MAX_BLOCKS];
  uint32_t bad[LOSS_MAX_BLOCKS];
  LossResult result;
};

struct LossParams {
  const float* logits;  // token kind: packed [total_tokens][2]; ranking kinds: [n_rows][channels]
  const void* labels;   // token kind: [n_rows][width]; BCE / CE: [n_rows]; MSE: [n_rows][channels]
  const int32_t* cu;    // token kind: [n_rows + 1]
  float* terms;         // nullable
  int n_rows, width, channels, total_tokens;
  long long ignore_index;
};

// sum / count / first offender of one block -> scratch[blockIdx.x].  Called by every thread of a 256-thread block.  The
// butterfly adds the same pairs in every lane (IEEE addition commutes), the four wave totals are added in wave order.
__device__ __forceinline__ void loss_block_partial(double sum, long long count, uint32_t bad, LossScratch* __restrict__ scratch) {
  __shared__ double wave_sum[LOSS_THREADS / 64];
  __shared__ long long wave_count[LOSS_THREADS / 64];
  __shared__ uint32_t wave_bad[LOSS_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off);
    count += __shfl_xor(count, off);
    bad = min(bad, (uint32_t)__shfl_xor((int)bad, off));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wave_sum[wave] = sum;
    wave_count[wave] = count;
    wave_bad[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < LOSS_THREADS / 64; ++w) {
      sum += wave_sum[w];
      count += wave_count[w];
      bad = min(bad, wave_bad[w]);
    }
    scratch->sum[blockIdx.x] = sum;
    scratch->count[blockIdx.x] = count;
    scratch->bad[blockIdx.x] = bad;
  }
}

// softplus(d) = log(1 + e^d) without overflow or cancellation: the 2-class cross entropy with d = z_other - z_label, and
// the tail of the binary one
__device__ __forceinline__ double loss_softplus(double d) { return fmax(d, 0.0) + log1p(exp(-fabs(d))); }

// LOSS_TOKEN_CE.  One wave per row at a time (4 rows per block step, blocks stride over the rows): token t of row r is
// packed position cu[r] + j and reads labels[r][j]; labels at j >= len[r] are never read.  Row bounds are held inside
// [0, total_tokens) and j inside the label row whatever cu holds.  Every packed position of a row gets its term when
// p.terms is given: +0.0 for an ignored or out-of-range label.
template <typename LabelT>
__global__ __launch_bounds__(LOSS_THREADS) void loss_token_ce_kernel(LossParams p, LossScratch* __restrict__ scratch) {
  const LabelT* __restrict__ labels = static_cast<const LabelT*>(p.labels);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sum = 0.0;
  long long count = 0;
  uint32_t bad = LOSS_NONE;
  for (long long r = (long long)blockIdx.x * (LOSS_THREADS / 64) + wave; r < p.n_rows; r += (long long)gridDim.x * (LOSS_THREADS / 64)) {
    const int start = max(p.cu[r], 0), end = min(p.cu[r + 1], p.total_tokens);
    const size_t base = (size_t)r * (size_t)p.width;
    for (int t = start + lane; t < end; t += 64) {
      const int j = t - start;
      float term32 = 0.0f;
      if (j < p.width) {
        const long long y = (long long)labels[base + (size_t)j];
        if (y != p.ignore_index) {
          if ((unsigned long long)y < 2ull) {
            const double z0 = (double)p.logits[2 * (size_t)t], z1 = (double)p.logits[2 * (size_t)t + 1];
            const double term = loss_softplus(y ? z0 - z1 : z1 - z0);
            sum += term;
            ++count;
            term32 = (float)term;
          } else {
            bad = min(bad, (uint32_t)(base + (size_t)j));  // (the caller keeps n_rows * width below 2^31)
          }
        }
      }
      if (p.terms) p.terms[t] = term32;
    }
  }
  loss_block_partial(sum, count, bad, scratch);
}

// LOSS_RANK_BCE: one thread per row, max(z, 0) - z y + log1p(exp(-|z|)) (BCEWithLogitsLoss), left to right: at z = 80,
// y = 1 the first two cancel exactly and the tail is the term.  (A template like the others, so that the header can be
// included by the C ABI unit for its structs without defining a kernel there.)
template <typename Unused = void>
__global__ __launch_bounds__(LOSS_THREADS) void loss_rank_bce_kernel(LossParams p, LossScratch* __restrict__ scratch) {
  const float* __restrict__ labels = static_cast<const float*>(p.labels);
  double sum = 0.0;
  long long count = 0;
  for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < p.n_rows; i += (long long)gridDim.x * LOSS_THREADS) {
    const double z = (double)p.logits[i], y = (double)labels[i];
    const double term = fmax(z, 0.0) - z * y + log1p(exp(-fabs(z)));
    sum += term;
    ++count;
    if (p.terms) p.terms[i] = (float)term;
  }
  loss_block_partial(sum, count, LOSS_NONE, scratch);
}

// LOSS_RANK_CE: one thread per row of C >= 2 logits, log-sum-exp after subtracting the maximum, as
// log1p(sum over c != argmax of exp(z_c - max)) + (max - z_y); for C = 2 that is loss_softplus(z_other - z_y) term by term.
template <typename LabelT>
__global__ __launch_bounds__(LOSS_THREADS) void loss_rank_ce_kernel(LossParams p, LossScratch* __restrict__ scratch) {
  const LabelT* __restrict__ labels = static_cast<const LabelT*>(p.labels);
  const int C = p.channels;
  double sum = 0.0;
  long long count = 0;
  uint32_t bad = LOSS_NONE;
  for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < p.n_rows; i += (long long)gridDim.x * LOSS_THREADS) {
    const long long y = (long long)labels[i];
    float term32 = 0.0f;
    if (y != p.ignore_index) {
      if ((unsigned long long)y < (unsigned long long)C) {
        const float* __restrict__ z = p.logits + (size_t)i * (size_t)C;
        float top = z[0];
        int at = 0;  // the first maximum: its own exp(0) is the 1 of log1p, so a sum of 1 + 4e-35 keeps its tail
        for (int c = 1; c < C; ++c)
          if (z[c] > top) top = z[c], at = c;
        double rest = 0.0;
        for (int c = 0; c < C; ++c)
          if (c != at) rest += exp((double)z[c] - (double)top);
        const double term = log1p(rest) + ((double)top - (double)z[y]);
        sum += term;
        ++count;
        term32 = (float)term;
      } else {
        bad = min(bad, (uint32_t)i);
      }
    }
    if (p.terms) p.terms[i] = term32;
  }
  loss_block_partial(sum, count, bad, scratch);
}

// LOSS_RANK_MSE: one thread per element of [n_rows][C], (z - y)^2.
template <typename Unused = void>
__global__ __launch_bounds__(LOSS_THREADS) void loss_rank_mse_kernel(LossParams p, LossScratch* __restrict__ scratch) {
  const float* __restrict__ labels = static_cast<const float*>(p.labels);
  const long long n = (long long)p.n_rows * (long long)p.channels;
  double sum = 0.0;
  long long count = 0;
  for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * LOSS_THREADS) {
    const double d = (double)p.logits[i] - (double)labels[i];
    const double term = d * d;
    sum += term;
    ++count;
    if (p.terms) p.terms[i] = (float)term;
  }
  loss_block_partial(sum, count, LOSS_NONE, scratch);
}

// The second launch, one block: the n_partials partials in index order, one fp64 division (0.0 / 0 = NaN for an empty
// count, as torch's mean), one rounding.  A label out of range makes the loss NaN and is reported with its value.
// LabelT = float: the kind has no integer labels.
template <typename LabelT>
__global__ __launch_bounds__(64) void loss_finish_kernel(LossScratch* __restrict__ scratch, int n_partials, const LabelT* __restrict__ labels,
                                                         float* __restrict__ loss_out) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  long long count = 0;
  uint32_t bad = LOSS_NONE;
  for (int i = 0; i < n_partials; ++i) {
    sum += scratch->sum[i];
    count += scratch->count[i];
    bad = min(bad, scratch->bad[i]);
  }
  float loss = (float)(sum / (double)count);
  LossResult res;
  res.sum = sum;
  res.count = count;
  res.bad_value = 0;
  res.bad_index = bad;
  res.status = 0;
  res.reserved = 0;
  if (bad != LOSS_NONE) {
    res.status = 1;
    res.bad_value = (long long)labels[bad];
    loss = __int_as_float(0x7fc00000);
  }
  res.loss = loss;
  scratch->result = res;
  *loss_out = loss;
}

}  // namespace opk

namespace opl {

// op_launch_loss.hip: the two launches of one op_loss call on st.  labels_dtype as enum op_int_dtype / OP_LABELS_F32, already
// checked against the kind; false when there is no kernel for the pair.  n_rows == 0 launches the finishing step only.
bool launch_loss(hipStream_t st, int kind, int labels_dtype, const opk::LossParams& p, opk::LossScratch* scratch, float* loss_dev);

}  // namespace opl
