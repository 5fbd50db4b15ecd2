// locate_check.cpp -- a stand-alone driver of the host check of op_located_fragment_means in open_provence_amd/csrc/op_plan.h
// (check_located_means) for tests/test_lookup_model.py: no HIP, no device.  It builds a well-formed request, breaks it one field
// at a time and prints `label code message` per attempt ("-" for no message); the expectations live in the test.  The host
// arrays are heap blocks of exactly their size, so a check that reads past one is a sanitizer report; the device pointers are a
// fake address that a host check must never follow.
#include <cstdio>
#include <functional>
#include <vector>

#include "../../open_provence_amd/csrc/op_plan.h"

namespace {

const int32_t* const FAKE_I32 = reinterpret_cast<const int32_t*>(0x1000);
float* const FAKE_F32 = reinterpret_cast<float*>(0x1000);

void report(const char* label, const opp::Refusal& r) { std::printf("%s %d %s\n", label, r.code, r.text[0] ? r.text : "-"); }

// 4 fragments of 3, 2, 4 and 1 ids, queries of 2 and 0 ids, one-id pieces; row 0 = query 0 with fragments 0, 1 (10 ids), row 1 =
// query 1 with fragment 2 clipped to 3 ids and fragment 3 (7 ids); the rows' fragments take slots 1 .. 5 of 5; 17 ids, 2 places.
struct Located {
  std::vector<int32_t> frag_off{0, 3, 5, 9, 10}, q_off{0, 2, 2}, plan{0, 0, 2, 0, 1, 2, 2, 3}, cu{0, 10, 17}, slot_off{1, 3, 5};
  int32_t piece[1] = {7};
  op_assemble_request rows{};
  op_planned_means_request req{};
  const int32_t* ids = FAKE_I32;
  int32_t* ctx_start_out = const_cast<int32_t*>(FAKE_I32);
  void bind() {
    rows.struct_bytes = sizeof(op_assemble_request);
    rows.n_frag = 4, rows.n_queries = 2, rows.n_rows = 2, rows.total_tokens = 17;
    rows.n_prefix = rows.n_middle = rows.n_suffix = 1;
    rows.prefix = rows.middle = rows.suffix = piece;
    rows.corpus_dev = rows.query_ids_dev = nullptr;  // (not read by this call)
    rows.frag_off_dev = rows.q_off_dev = rows.plan_dev = rows.cu_seqlens_dev = FAKE_I32;
    rows.frag_off_host = frag_off.data(), rows.q_off_host = q_off.data(), rows.plan_host = plan.data(), rows.cu_seqlens_host = cu.data();
    req.struct_bytes = sizeof(op_planned_means_request);
    req.n_slots = 5;
    req.keep_prob_dev = FAKE_F32, req.frag_shift_dev = FAKE_I32, req.slot_off_dev = FAKE_I32, req.slot_off_host = slot_off.data();
    req.mean_out_dev = FAKE_F32, req.slot_frag_out_dev = const_cast<int32_t*>(FAKE_I32);
  }
};

void located_case(const char* label, const std::function<void(Located&)>& spoil) {
  Located m;
  m.bind();
  spoil(m);
  report(label, opp::check_located_means(&m.rows, &m.req, m.ids, m.ctx_start_out));
}

void no_rows(Located& m) {
  m.rows.n_rows = 0, m.rows.total_tokens = 0;
  m.rows.plan_host = m.rows.cu_seqlens_host = m.req.slot_off_host = nullptr;  // (nothing to read without rows)
}

}  // namespace

int main() {
  located_case("well_formed", [](Located&) {});
  located_case("no_rows", no_rows);
  located_case("no_rows_null_buffers", [](Located& m) {
    no_rows(m);
    m.ids = nullptr, m.ctx_start_out = nullptr;
  });
  // the two buffers of the lookup
  located_case("null_ids", [](Located& m) { m.ids = nullptr; });
  located_case("null_ctx_start_out", [](Located& m) { m.ctx_start_out = nullptr; });
  located_case("null_both", [](Located& m) { m.ids = nullptr, m.ctx_start_out = nullptr; });
  // everything check_planned_means checks, under this call's name
  report("null_rows", opp::check_located_means(nullptr, nullptr, FAKE_I32, const_cast<int32_t*>(FAKE_I32)));
  {
    Located m;
    m.bind();
    report("null_request", opp::check_located_means(&m.rows, nullptr, m.ids, m.ctx_start_out));
  }
  located_case("rows_struct_bytes", [](Located& m) { m.rows.struct_bytes = 8; });
  located_case("struct_bytes", [](Located& m) { m.req.struct_bytes += 8; });
  located_case("negative_rows", [](Located& m) { m.rows.n_rows = -1; });
  located_case("negative_slots", [](Located& m) { m.req.n_slots = -1; });
  located_case("negative_total", [](Located& m) { m.rows.total_tokens = -17; });
  located_case("negative_frag", [](Located& m) { m.rows.n_frag = -4; });
  located_case("negative_queries", [](Located& m) { m.rows.n_queries = -2; });
  located_case("long_prefix", [](Located& m) { m.rows.n_prefix = OP_ASSEMBLE_MAX_PIECE + 1; });
  located_case("negative_middle", [](Located& m) { m.rows.n_middle = -1; });
  located_case("null_plan_host", [](Located& m) { m.rows.plan_host = nullptr; });
  located_case("null_plan_dev", [](Located& m) { m.rows.plan_dev = nullptr; });
  located_case("null_cu_host", [](Located& m) { m.rows.cu_seqlens_host = nullptr; });
  located_case("null_cu_dev", [](Located& m) { m.rows.cu_seqlens_dev = nullptr; });
  located_case("null_frag_off_host", [](Located& m) { m.rows.frag_off_host = nullptr; });
  located_case("null_frag_off_dev", [](Located& m) { m.rows.frag_off_dev = nullptr; });
  located_case("null_q_off_host", [](Located& m) { m.rows.q_off_host = nullptr; });
  located_case("null_q_off_dev", [](Located& m) { m.rows.q_off_dev = nullptr; });
  located_case("null_slot_off_host", [](Located& m) { m.req.slot_off_host = nullptr; });
  located_case("null_slot_off_dev", [](Located& m) { m.req.slot_off_dev = nullptr; });
  located_case("null_frag_shift", [](Located& m) { m.req.frag_shift_dev = nullptr; });
  located_case("null_keep_prob", [](Located& m) { m.req.keep_prob_dev = nullptr; });
  located_case("null_mean_out", [](Located& m) { m.req.mean_out_dev = nullptr; });
  located_case("null_slot_frag_out", [](Located& m) { m.req.slot_frag_out_dev = nullptr; });
  located_case("query_outside", [](Located& m) { m.plan[4] = 2; });
  located_case("negative_query", [](Located& m) { m.plan[0] = -1; });
  located_case("fragments_past_the_corpus", [](Located& m) { m.plan[4 + 2] = 3; });
  located_case("negative_first_fragment", [](Located& m) { m.plan[1] = -1; });
  located_case("negative_fragment_count", [](Located& m) { m.plan[2] = -2; });
  located_case("clip_beyond_the_fragment", [](Located& m) { m.plan[4 + 3] = 5; });
  located_case("negative_clip", [](Located& m) { m.plan[3] = -1; });
  located_case("frag_off_decreases", [](Located& m) { m.frag_off[1] = 6; });
  located_case("q_off_decreases", [](Located& m) { m.q_off[2] = 1; });
  located_case("offsets_from_1", [](Located& m) { m.q_off[0] = 1; });
  located_case("cu_start", [](Located& m) { m.cu[0] = 1; });
  located_case("cu_end", [](Located& m) { m.cu[2] = 18; });
  located_case("cu_decreases", [](Located& m) { m.cu[1] = 18; });
  located_case("slot_off_negative", [](Located& m) { m.slot_off[0] = -1; });
  located_case("slot_off_not_prefix_sums", [](Located& m) { m.slot_off[2] = 4; });
  located_case("slot_off_past_the_outputs", [](Located& m) { m.slot_off = {2, 4, 6}; });
  return 0;
}
