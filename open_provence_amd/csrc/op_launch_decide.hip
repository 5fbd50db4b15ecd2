// op_launch_decide.hip -- launches of op_planned_fragment_means', op_located_fragment_means' and op_sentence_decisions' kernels
// (opk_decide.hip.h).
#include "op_internal.h"
#include "opk_decide.hip.h"

namespace opl {
using namespace opk;

static_assert(DECIDE_INSTANCE_WORDS == OP_DECISIONS_INSTANCE_WORDS, "the public header and opk_decide.hip.h disagree on an instance's words");

static PlannedMeansParams planned_means_params(const op_assemble_request& rows, const op_planned_means_request& req) {
  PlannedMeansParams p = {};
  p.keep_prob = req.keep_prob_dev, p.frag_off = rows.frag_off_dev, p.frag_shift = req.frag_shift_dev, p.q_off = rows.q_off_dev;
  p.plan = rows.plan_dev, p.cu = rows.cu_seqlens_dev, p.slot_off = req.slot_off_dev;
  p.mean_out = req.mean_out_dev, p.slot_frag_out = req.slot_frag_out_dev;
  p.n_frag = rows.n_frag, p.n_queries = rows.n_queries, p.n_query_tokens = rows.q_off_host[rows.n_queries];
  p.n_rows = rows.n_rows, p.total = rows.total_tokens, p.n_slots = req.n_slots;
  p.n_prefix = rows.n_prefix, p.n_middle = rows.n_middle;
  return p;
}

void launch_planned_fragment_means(hipStream_t st, const op_assemble_request& rows, const op_planned_means_request& req) {
  const PlannedMeansParams p = planned_means_params(rows, req);
  hipLaunchKernelGGL(planned_fragment_means_kernel, dim3((unsigned)((rows.n_rows + 3) / 4)), dim3(256), 0, st, p);
}

void launch_located_fragment_means(hipStream_t st, const op_assemble_request& rows, const op_planned_means_request& req, const int32_t* ids,
                                   int32_t* ctx_start_out) {
  LocatedMeansParams p = {};
  p.planned = planned_means_params(rows, req);
  p.ids = ids, p.ctx_start_out = ctx_start_out;
  hipLaunchKernelGGL(located_fragment_means_kernel, dim3((unsigned)((rows.n_rows + 3) / 4)), dim3(256), 0, st, p);
}

void launch_sentence_decisions(hipStream_t st, const op_decisions_request& req) {
  DecisionsParams p = {};
  p.instances = req.instances_dev, p.mean = req.mean_dev, p.slot_frag = req.slot_frag_dev, p.frag_sent = req.frag_sent_dev;
  p.avg_out = req.avg_out_dev, p.keep_out = req.keep_out_dev, p.threshold = req.threshold;
  p.n_instances = req.n_instances, p.n_slots = req.n_slots, p.n_frag = req.n_frag, p.n_out = req.n_out;
  hipLaunchKernelGGL(sentence_decisions_kernel, dim3((unsigned)((req.n_instances + 63) / 64)), dim3(64), 0, st, p);
}

}  // namespace opl
