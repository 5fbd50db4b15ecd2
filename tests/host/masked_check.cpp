// masked_check.cpp -- a stand-alone driver of the host checks of op_forward_masked_native in open_provence_amd/csrc/op_plan.h
// (check_masked_args, check_masked_native_handle, masked_native_layout) for tests/test_masked_native_host.py: no HIP, no device.
// It prints `label code message` per attempt ("-" for no message), then `layout ...` lines; the expectations live in the test.
#include <cstdio>

#include "../../open_provence_amd/csrc/op_plan.h"

namespace {

void report(const char* label, const opp::Refusal& r) { std::printf("%s %d %s\n", label, r.code, r.text[0] ? r.text : "-"); }

struct Args {
  bool has_report = true;
  uint32_t report_bytes = sizeof(op_masked_report);
  int n_rows = 3, width = 200;
  bool ids = true, mask = true, prune = true, rank = true, workspace = true;
  opp::Refusal check() const {
    return opp::check_masked_args("op_forward_masked_native", has_report, report_bytes, n_rows, width, ids, mask, prune, rank, workspace);
  }
};

void layout(int hidden, int chunk_rows, int n_rows, int width, size_t forward_bytes) {
  const opp::MaskedNativeLayout l = opp::masked_native_layout(hidden, chunk_rows, n_rows, width, forward_bytes);
  std::printf("layout %d %d %d %d %zu : %zu %zu %zu %zu %zu %zu\n", hidden, chunk_rows, n_rows, width, forward_bytes, l.cu, l.status, l.key_row,
              l.vmean, l.forward, l.bytes);
}

}  // namespace

int main() {
  Args a;
  report("well_formed", a.check());
  a = Args{}, a.has_report = false;
  report("null_report", a.check());
  a = Args{}, a.report_bytes = 8;
  report("report_struct_bytes", a.check());
  a = Args{}, a.n_rows = -1;
  report("negative_rows", a.check());
  a = Args{}, a.width = -5;
  report("negative_width", a.check());
  a = Args{}, a.n_rows = 1 << 16, a.width = 1 << 15;  // = 2^31
  report("too_many_cells", a.check());
  a = Args{}, a.n_rows = 1 << 16, a.width = (1 << 15) - 1;  // below 2^31
  report("cells_below_the_limit", a.check());
  a = Args{}, a.ids = false;
  report("null_ids", a.check());
  a = Args{}, a.mask = false;
  report("null_mask", a.check());
  a = Args{}, a.prune = false;
  report("null_prune", a.check());
  a = Args{}, a.rank = false;
  report("null_rank", a.check());
  a = Args{}, a.workspace = false;
  report("null_workspace", a.check());
  // the order: the report before the sizes, the sizes before the buffers, ids first among those
  a = Args{}, a.has_report = false, a.n_rows = -1, a.ids = false;
  report("order_report_first", a.check());
  a = Args{}, a.n_rows = -1, a.width = -1, a.ids = false;
  report("order_rows_before_width", a.check());
  a = Args{}, a.ids = a.mask = a.prune = a.rank = a.workspace = false;
  report("order_ids_first", a.check());
  // an empty batch needs no buffer
  a = Args{}, a.n_rows = 0, a.ids = a.mask = a.prune = a.rank = a.workspace = false;
  report("empty_rows", a.check());
  a = Args{}, a.width = 0, a.ids = a.mask = a.prune = a.rank = a.workspace = false;
  report("empty_width", a.check());

  // the handle's fitness: (width, max_pos, row_path, panel_path, set)
  report("row_path", opp::check_masked_native_handle(200, 2048, true, false, OP_KS_F16));
  report("panel_path", opp::check_masked_native_handle(2048, 2048, false, true, OP_KS_BF16X3));
  report("cleared_operands", opp::check_masked_native_handle(1, 2048, true, false, -1));
  report("too_wide", opp::check_masked_native_handle(2049, 2048, true, false, OP_KS_F16));
  report("tiled_path", opp::check_masked_native_handle(200, 2048, false, false, OP_KS_BF16X3));
  report("set_fp32", opp::check_masked_native_handle(200, 2048, true, false, OP_KS_F32));
  report("order_width_first", opp::check_masked_native_handle(4096, 2048, false, false, OP_KS_F32));
  report("order_path_before_set", opp::check_masked_native_handle(200, 2048, false, false, OP_KS_F32));

  layout(256, 0, 3, 200, 1000);
  layout(512, 256, 31, 200, 4096);
  layout(128, 0, 1, 1, 256);
  layout(256, 131072, 1000, 512, 123456);
  return 0;
}
