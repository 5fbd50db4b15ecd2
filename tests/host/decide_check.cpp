// decide_check.cpp -- a stand-alone driver of the two host checks of prepared requests in open_provence_amd/csrc/op_plan.h
// (check_planned_means, check_decisions) for tests/test_decision_model.py: no HIP, no device.  It builds a well-formed pair of
// requests, breaks them one way at a time and prints `label code message` per attempt ("-" for no message); the expectations
// live in the test.  The host arrays are heap blocks of exactly their size, so a check that reads past one is a sanitizer report;
// the device pointers are a fake address that a host check must never follow.
#include <cstdio>
#include <functional>
#include <vector>

#include "../../open_provence_amd/csrc/op_plan.h"

namespace {

const int32_t* const FAKE_I32 = reinterpret_cast<const int32_t*>(0x1000);
float* const FAKE_F32 = reinterpret_cast<float*>(0x1000);

void report(const char* label, const opp::Refusal& r) { std::printf("%s %d %s\n", label, r.code, r.text[0] ? r.text : "-"); }

// 4 fragments of 3, 2, 4 and 1 ids, queries of 2 and 0 ids, one-id pieces; row 0 = query 0 with fragments 0, 1 (10 ids), row 1 =
// query 1 with fragment 2 clipped to 3 ids and fragment 3 (7 ids); the rows' fragments take slots 1 .. 5 of 5.
struct Means {
  std::vector<int32_t> frag_off{0, 3, 5, 9, 10}, q_off{0, 2, 2}, plan{0, 0, 2, 0, 1, 2, 2, 3}, cu{0, 10, 17}, slot_off{1, 3, 5};
  int32_t piece[1] = {7};
  op_assemble_request rows{};
  op_planned_means_request req{};
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

void means_case(const char* label, const std::function<void(Means&)>& spoil) {
  Means m;
  m.bind();
  spoil(m);
  report(label, opp::check_planned_means(&m.rows, &m.req));
}

// 2 instances over 5 slots and 4 fragments: sentences 0 .. 3 and 3 .. 5 of the outputs
struct Decisions {
  std::vector<int32_t> instances{0, 3, 0, 3, 0, 2, 3, 5, 3, 2, 3, -1};
  op_decisions_request req{};
  void bind() {
    req.struct_bytes = sizeof(op_decisions_request);
    req.n_instances = 2, req.n_slots = 5, req.n_frag = 4, req.n_out = 5;
    req.threshold = 0.5;
    req.instances_dev = FAKE_I32, req.instances_host = instances.data();
    req.mean_dev = FAKE_F32, req.slot_frag_dev = FAKE_I32, req.frag_sent_dev = FAKE_I32;
    req.avg_out_dev = reinterpret_cast<double*>(0x1000), req.keep_out_dev = reinterpret_cast<uint8_t*>(0x1000);
  }
};

void decisions_case(const char* label, const std::function<void(Decisions&)>& spoil) {
  Decisions d;
  d.bind();
  spoil(d);
  report(label, opp::check_decisions(&d.req));
}

}  // namespace

int main() {
  means_case("means:well_formed", [](Means&) {});
  means_case("means:no_rows", [](Means& m) {
    m.rows.n_rows = 0, m.rows.total_tokens = 0;
    m.rows.plan_host = m.rows.cu_seqlens_host = m.req.slot_off_host = nullptr;  // (nothing to read without rows)
  });
  report("means:null_rows", opp::check_planned_means(nullptr, nullptr));
  {
    Means m;
    m.bind();
    report("means:null_request", opp::check_planned_means(&m.rows, nullptr));
  }
  means_case("means:rows_struct_bytes", [](Means& m) { m.rows.struct_bytes = 8; });
  means_case("means:struct_bytes", [](Means& m) { m.req.struct_bytes += 8; });
  means_case("means:negative_rows", [](Means& m) { m.rows.n_rows = -1; });
  means_case("means:negative_slots", [](Means& m) { m.req.n_slots = -1; });
  means_case("means:negative_total", [](Means& m) { m.rows.total_tokens = -17; });
  means_case("means:null_plan_host", [](Means& m) { m.rows.plan_host = nullptr; });
  means_case("means:null_plan_dev", [](Means& m) { m.rows.plan_dev = nullptr; });
  means_case("means:null_cu_host", [](Means& m) { m.rows.cu_seqlens_host = nullptr; });
  means_case("means:null_frag_off_host", [](Means& m) { m.rows.frag_off_host = nullptr; });
  means_case("means:null_q_off_dev", [](Means& m) { m.rows.q_off_dev = nullptr; });
  means_case("means:null_slot_off_host", [](Means& m) { m.req.slot_off_host = nullptr; });
  means_case("means:null_slot_off_dev", [](Means& m) { m.req.slot_off_dev = nullptr; });
  means_case("means:null_frag_shift", [](Means& m) { m.req.frag_shift_dev = nullptr; });
  means_case("means:null_keep_prob", [](Means& m) { m.req.keep_prob_dev = nullptr; });
  means_case("means:null_mean_out", [](Means& m) { m.req.mean_out_dev = nullptr; });
  means_case("means:null_slot_frag_out", [](Means& m) { m.req.slot_frag_out_dev = nullptr; });
  means_case("means:query_outside", [](Means& m) { m.plan[4] = 2; });
  means_case("means:negative_query", [](Means& m) { m.plan[0] = -1; });
  means_case("means:fragments_past_the_corpus", [](Means& m) { m.plan[4 + 2] = 3; });
  means_case("means:negative_first_fragment", [](Means& m) { m.plan[1] = -1; });
  means_case("means:negative_fragment_count", [](Means& m) { m.plan[2] = -2; });
  means_case("means:clip_beyond_the_fragment", [](Means& m) { m.plan[4 + 3] = 5; });
  means_case("means:negative_clip", [](Means& m) { m.plan[3] = -1; });
  means_case("means:frag_off_decreases", [](Means& m) { m.frag_off[1] = 6; });
  means_case("means:q_off_decreases", [](Means& m) { m.q_off[2] = 1; });
  means_case("means:offsets_from_1", [](Means& m) { m.q_off[0] = 1; });
  means_case("means:cu_start", [](Means& m) { m.cu[0] = 1; });
  means_case("means:cu_end", [](Means& m) { m.cu[2] = 18; });
  means_case("means:cu_decreases", [](Means& m) { m.cu[1] = 18; });
  means_case("means:slot_off_negative", [](Means& m) { m.slot_off[0] = -1; });
  means_case("means:slot_off_not_prefix_sums", [](Means& m) { m.slot_off[2] = 4; });
  means_case("means:slot_off_past_the_outputs", [](Means& m) { m.slot_off = {2, 4, 6}; });

  decisions_case("decisions:well_formed", [](Decisions&) {});
  decisions_case("decisions:no_instances", [](Decisions& d) {
    d.req.n_instances = d.req.n_out = 0;
    d.req.instances_host = d.req.instances_dev = nullptr;
    d.req.avg_out_dev = nullptr, d.req.keep_out_dev = nullptr;
  });
  report("decisions:null_request", opp::check_decisions(nullptr));
  decisions_case("decisions:struct_bytes", [](Decisions& d) { d.req.struct_bytes = 4; });
  decisions_case("decisions:negative_instances", [](Decisions& d) { d.req.n_instances = -1; });
  decisions_case("decisions:negative_slots", [](Decisions& d) { d.req.n_slots = -5; });
  decisions_case("decisions:negative_frag", [](Decisions& d) { d.req.n_frag = -1; });
  decisions_case("decisions:negative_out", [](Decisions& d) { d.req.n_out = -1; });
  decisions_case("decisions:null_instances_dev", [](Decisions& d) { d.req.instances_dev = nullptr; });
  decisions_case("decisions:null_instances_host", [](Decisions& d) { d.req.instances_host = nullptr; });
  decisions_case("decisions:null_mean", [](Decisions& d) { d.req.mean_dev = nullptr; });
  decisions_case("decisions:null_slot_frag", [](Decisions& d) { d.req.slot_frag_dev = nullptr; });
  decisions_case("decisions:null_frag_sent", [](Decisions& d) { d.req.frag_sent_dev = nullptr; });
  decisions_case("decisions:null_avg_out", [](Decisions& d) { d.req.avg_out_dev = nullptr; });
  decisions_case("decisions:null_keep_out", [](Decisions& d) { d.req.keep_out_dev = nullptr; });
  decisions_case("decisions:slots_past_the_buffer", [](Decisions& d) { d.instances[6 + 1] = 6; });
  decisions_case("decisions:negative_slot", [](Decisions& d) { d.instances[0] = -1; });
  decisions_case("decisions:slots_backwards", [](Decisions& d) { d.instances[6 + 0] = 5, d.instances[6 + 1] = 3; });
  decisions_case("decisions:sentences_past_the_outputs", [](Decisions& d) { d.instances[6 + 3] = 3; });
  decisions_case("decisions:sentences_overlap", [](Decisions& d) { d.instances[6 + 2] = 2; });
  decisions_case("decisions:negative_sentences", [](Decisions& d) { d.instances[3] = -1; });
  decisions_case("decisions:outputs_not_tiled", [](Decisions& d) { d.req.n_out = 6; });
  decisions_case("decisions:negative_sent_base", [](Decisions& d) { d.instances[4] = -1; });
  decisions_case("decisions:title_past_the_sentences", [](Decisions& d) { d.instances[5] = 3; });
  decisions_case("decisions:title_below_minus_one", [](Decisions& d) { d.instances[6 + 5] = -2; });
  return 0;
}
