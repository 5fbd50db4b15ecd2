// plan_check.cpp -- a stand-alone driver of open_provence_amd/csrc/op_plan.h for tests/test_plan_host.py: no HIP, no device.
// It reads one query per line from stdin and answers each with one line on stdout; the expectations live in the test.
//   avail  H I flags f16_unfit                                  -> the available sets of that shape
//   select H I flags req*6 any_lo*4 not_f16 f16_unfit f8_off forced_set forced_mask -> eff*6 set mlp_layers
//   cand   H I flags default_set                                -> the calibration candidates in order
//   search n_layers tol flags reference default n_cand cand.. n_rules (set mask|* err rc).. -> the result and the measure calls
//   maxdiff n got*n ref*n                                       -> max |got - ref|, +inf when not finite
//   chunks chunk_rows n len..                                  -> capacity, then (s1 rows max_len) per chunk
//   plan   heads cus flags n len..                              -> waves_g items_g items_l
//   items  waves n len..                                        -> work items
//   layout H I rows_pad n_seqs f32                              -> total bytes, then (name kind offset bytes) per region
//   cu     total max_seqlen max_pos n cu[0..n]                  -> code and message of check_cu_seqlens
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../open_provence_amd/csrc/op_plan.h"

namespace {

opp::SelectState state_of(int H, int I, unsigned flags) {
  opp::SelectState s;
  const opp::Paths p = opp::paths_of(H, I, flags);
  const opp::Packs k = opp::packs_of(p, H, flags);
  s.row_path = p.row;
  s.panel_path = p.panel;
  s.f8_packs = k.f8;
  s.h16_packs = k.h16;
  s.f32_packs = k.f32;
  s.flags = flags;
  return s;
}

std::vector<int32_t> read_cu(std::istream& in, int* max_len) {
  int n = 0;
  in >> n;
  std::vector<int32_t> cu(1, 0);
  *max_len = 0;
  for (int i = 0; i < n; ++i) {
    int len = 0;
    in >> len;
    cu.push_back(cu.back() + len);
    *max_len = std::max(*max_len, len);
  }
  return cu;
}

struct Rule {
  int set;
  bool any_mask;
  uint64_t mask;
  float err;
  int rc;
};

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "avail") {
      int H, I, unfit;
      unsigned flags;
      in >> H >> I >> flags >> unfit;
      opp::SelectState s = state_of(H, I, flags);
      s.f16_unfit = unfit != 0;
      for (int set = -1; set <= OP_KS_COUNT; ++set)
        if (opp::set_available(s, set)) printf("%d ", set);
      printf("\n");
    } else if (what == "select") {
      int H, I, v;
      unsigned flags;
      in >> H >> I >> flags;
      opp::SelectState s = state_of(H, I, flags);
      in >> s.req.wqkv >> s.req.qk >> s.req.pv >> s.req.attn_out >> s.req.wi >> s.req.mlp_out;
      const int fam[4] = {OP_FAM_WQKV, OP_FAM_ATTN_OUT, OP_FAM_WI, OP_FAM_MLP_OUT};
      for (int f : fam) {
        in >> v;
        s.any_lo[f] = v != 0;
      }
      in >> v, s.not_f16 = v != 0;
      in >> v, s.f16_unfit = v != 0;
      in >> v, s.f8_off = v != 0;
      in >> s.forced_set >> std::hex >> s.forced_mlp_layers >> std::dec;
      const opp::Selection r = opp::select(s);
      printf("%d %d %d %d %d %d %d %" PRIx64 "\n", r.eff.wqkv, r.eff.qk, r.eff.pv, r.eff.attn_out, r.eff.wi, r.eff.mlp_out, r.set, r.mlp_layers);
    } else if (what == "cand") {
      int H, I, def;
      unsigned flags;
      in >> H >> I >> flags >> def;
      for (int set : opp::calibration_candidates(state_of(H, I, flags), def)) printf("%d ", set);
      printf("\n");
    } else if (what == "search") {
      int n_layers, reference, def, n_cand, n_rules;
      float tol;
      unsigned flags;
      in >> n_layers >> tol >> flags >> reference >> def >> n_cand;
      std::vector<int> cand(n_cand);
      for (int& c : cand) in >> c;
      in >> n_rules;
      std::vector<Rule> rules(n_rules);
      for (Rule& r : rules) {
        std::string mask, err;
        in >> r.set >> mask >> err >> r.rc;
        r.any_mask = mask == "*";
        r.mask = r.any_mask ? 0 : strtoull(mask.c_str(), nullptr, 16);
        r.err = strtof(err.c_str(), nullptr);
      }
      std::ostringstream calls;
      auto measure = [&](int set, uint64_t mask) -> opp::Measurement {
        calls << " " << set << ":" << std::hex << mask << std::dec;
        for (int pass = 0; pass < 2; ++pass)
          for (const Rule& r : rules)
            if (r.set == set && (pass == 0 ? (!r.any_mask && r.mask == mask) : r.any_mask)) return {r.rc, r.err};
        return {OP_ERR_INVALID, 0.f};  // a call the test did not script
      };
      const opp::SearchResult r = opp::calibration_search(cand, reference, def, tol, flags, n_layers, measure);
      printf("%d %d %" PRIx64 " %.9g %.9g %d", r.rc, r.chosen, r.mlp_layers, r.default_err, r.mlp_layers_err, r.n_candidates);
      for (int c = 0; c < r.n_candidates; ++c) printf(" %d=%.9g", r.candidate_set[c], r.candidate_err[c]);
      printf(" |%s\n", calls.str().c_str());
    } else if (what == "maxdiff") {
      int n = 0;
      in >> n;
      std::vector<float> got(n), ref(n);
      std::string v;
      for (float& g : got) in >> v, g = strtof(v.c_str(), nullptr);
      for (float& r : ref) in >> v, r = strtof(v.c_str(), nullptr);
      printf("%.9g\n", opp::max_diff(got, ref));
    } else if (what == "chunks") {
      int chunk_rows, max_len = 0;
      in >> chunk_rows;
      const std::vector<int32_t> cu = read_cu(in, &max_len);
      const int n = (int)cu.size() - 1;
      const int cap = opp::chunk_row_capacity(chunk_rows, n, cu[n], max_len);
      printf("%d", cap);
      for (int s0 = 0; s0 < n;) {
        int rows = -1, longest = -1;
        const int s1 = opp::next_chunk(cu.data(), s0, n, cap, &rows, &longest);
        printf(" %d %d %d", s1, rows, longest);
        if (s1 <= s0) break;  // (the test sees the missing sequences)
        s0 = s1;
      }
      printf("\n");
    } else if (what == "plan") {
      int heads, cus, max_len = 0;
      unsigned flags;
      in >> heads >> cus >> flags;
      const std::vector<int32_t> cu = read_cu(in, &max_len);
      const opp::AttnPlan p = opp::attention_plan(cu.data(), 0, (int)cu.size() - 1, max_len, heads, cus, flags);
      printf("%d %d %d\n", p.waves_g, p.items_g, p.items_l);
    } else if (what == "items") {
      int waves, max_len = 0;
      in >> waves;
      const std::vector<int32_t> cu = read_cu(in, &max_len);
      printf("%d\n", opp::count_items(cu.data(), 0, (int)cu.size() - 1, waves));
    } else if (what == "layout") {
      int H, I, rows_pad, n_seqs, f32;
      in >> H >> I >> rows_pad >> n_seqs >> f32;
      const opp::Layout lay = opp::workspace_layout(H, I, rows_pad, n_seqs, f32 != 0);
      printf("%zu", lay.bytes);
      for (int i = 0; i < lay.n; ++i) printf(" %s %d %zu %zu", lay.regions[i].name, lay.regions[i].kind, lay.regions[i].offset, lay.regions[i].bytes);
      printf("\n");
    } else if (what == "cu") {
      int total, max_seqlen, max_pos, n;
      in >> total >> max_seqlen >> max_pos >> n;
      std::vector<int32_t> cu(n + 1);
      for (int32_t& c : cu) in >> c;
      const opp::Refusal r = opp::check_cu_seqlens(cu.data(), n, total, max_seqlen, max_pos);
      printf("%d %s\n", r.code, r.text);
    } else {
      printf("? %s\n", what.c_str());
    }
  }
  return 0;
}
