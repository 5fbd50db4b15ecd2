// op_select.hip -- C ABI: which kernel set a handle runs.  The device side of the selection (resolve_policy / pin; the
// decisions themselves are op_plan.h's), op_weights_ready, the pinning entry points, the MLP layer mask, op_calibrate.
#include "op_handle.h"

namespace {
// what selection reads from the handle (the device flags: resolve_policy)
opp::SelectState select_state(const op_handle* h) {
  opp::SelectState s;
  s.req = h->req;
  s.f16_unfit = h->f16_unfit;
  s.row_path = h->row_path;
  s.panel_path = h->panel_path;
  s.f8_packs = h->f8_packs;
  s.h16_packs = h->h16_packs;
  s.f32_packs = h->f32_packs;
  s.f8_off = h->f8_off;
  s.flags = h->cfg.flags;
  s.forced_set = h->forced_set;
  s.forced_mlp_layers = h->forced_mlp_layers;
  return s;
}
}  // namespace

namespace oph {

// The weights' flags from the device, the selection (opp::select), the result into the handle.
int resolve_policy(op_handle* h) {
  if (h->resolved) return OP_OK;
  // [OP_FAM_COUNT]: some GEMM weight is not exactly an fp16 value; [+ 2]: some weight TENSOR sits on fp16's subnormal grid
  // (note_f16_fit in opk_common.hip.h): the "f16 + fp8" sets cannot represent it
  int any_lo[OP_FAM_COUNT + 3] = {0};
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  OP_HIP(h, hipMemcpy(any_lo, h->any_lo_dev, sizeof(any_lo), hipMemcpyDeviceToHost));
  h->f16_unfit = any_lo[OP_FAM_COUNT + 2] != 0;
  opp::SelectState s = select_state(h);
  for (int f = 0; f < OP_FAM_COUNT; ++f) s.any_lo[f] = any_lo[f] != 0;
  s.not_f16 = any_lo[OP_FAM_COUNT] != 0;
  const opp::Selection sel = opp::select(s);
  h->eff = sel.eff;
  h->set = sel.set;
  h->ks = &opp::set_row(sel.set);
  h->mlp_layers = sel.mlp_layers;
  h->resolved = true;
  return OP_OK;
}

// run kernel set `set` with layer mask `mlp_layers` from now on where the handle can (-1: the default selection)
int pin(op_handle* h, int set, uint64_t mlp_layers) {
  h->forced_set = set;
  h->forced_mlp_layers = mlp_layers;
  h->resolved = false;
  return resolve_policy(h);
}

}  // namespace oph

namespace {

// deterministic calibration batch: 24 rows of min(512, max_pos) tokens + 14 ragged rows, ids uniform over the vocabulary
// (specials avoided as bench.py does: [1000, V - 1000) when the vocabulary is that large)
void synthetic_calibration_rows(const op_handle* h, std::vector<int32_t>& ids, std::vector<int32_t>& cu) {
  const int full = std::min(512, h->max_pos);
  // (the forward fuzz on calibrated sets finds its worst rows among the 1-3 token ones: several of them are in)
  const int ragged[14] = {1, 2, 2, 3, 5, 9, 17, 33, 64, 96, 130, 257, 333, 511};
  std::vector<int> lens(24, full);
  for (int r : ragged) lens.push_back(std::min(r, h->max_pos));
  const int lo = h->V > 4000 ? 1000 : 0, span = h->V > 4000 ? h->V - 2000 : h->V;
  uint64_t state = 0x9E3779B97F4A7C15ull;
  cu.assign(1, 0);
  ids.clear();
  for (int len : lens) {
    for (int i = 0; i < len; ++i) {
      state += 0x9E3779B97F4A7C15ull;  // splitmix64
      uint64_t z = state;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      ids.push_back(lo + (int32_t)(z % (uint64_t)span));
    }
    cu.push_back((int32_t)ids.size());
  }
}

// op_calibrate's visit to a handle.  While it lasts nothing is profiled or captured; when it ends, on whichever way out, both
// come back -- and so does what was pinned before the call, unless the call got as far as pinning its own answer (keep_pin).
struct CalibrationVisit {
  op_handle* const h;
  const bool profiling;
  float* const capture;
  const bool f8_off;
  const int forced_set;
  const uint64_t forced_mlp_layers;
  bool pin_kept = false;

  explicit CalibrationVisit(op_handle* h_)
      : h(h_), profiling(h_->profiling), capture(h_->capture), f8_off(h_->f8_off), forced_set(h_->forced_set), forced_mlp_layers(h_->forced_mlp_layers) {
    h->profiling = false;
    h->capture = nullptr;
  }
  CalibrationVisit(const CalibrationVisit&) = delete;
  void keep_pin() { pin_kept = true; }
  int restore_pin() {
    pin_kept = true;
    h->f8_off = f8_off;
    return pin(h, forced_set, forced_mlp_layers);
  }
  ~CalibrationVisit() {
    h->profiling = profiling;
    h->capture = capture;
    if (!pin_kept) (void)restore_pin();
  }
};

}  // namespace

extern "C" {

int op_weights_ready(op_handle* h) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_weights_ready: NULL handle");
  if (h->missing.empty()) return resolve_policy(h);
  std::string msg = "missing weights:";
  size_t shown = 0;
  for (const auto& m : h->missing) {
    if (shown++ == 8) {
      msg += " ...";
      break;
    }
    msg += " " + m;
  }
  msg += " (" + std::to_string(h->missing.size()) + " total)";
  return fail(h, OP_ERR_STATE, "%s", msg.c_str());
}

int op_set_compact_operands(op_handle* h, int enabled, int* changed) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_set_compact_operands: NULL handle");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  const int before = h->set;
  h->f8_off = enabled == 0;
  // (switching off: a pinned / calibrated compact set goes too)
  rc = enabled ? pin(h, h->forced_set, h->forced_mlp_layers) : pin(h, -1);
  if (changed) *changed = (rc == OP_OK && h->set != before) ? 1 : 0;
  return rc;
}

int op_select_kernel_set(op_handle* h, int kernel_set) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_select_kernel_set: NULL handle");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  if (kernel_set == OP_KS_F32 && !h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_select_kernel_set: kernel set %d (\"fp32\") needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS",
                kernel_set);
  if (kernel_set != OP_KS_AUTO && !opp::set_available(select_state(h), kernel_set))
    return fail(h, OP_ERR_UNSUPPORTED, "op_select_kernel_set: kernel set %d cannot run on this handle (shape, flags or weights)", kernel_set);
  return pin(h, kernel_set == OP_KS_AUTO ? -1 : kernel_set);  // (the coverage follows the arithmetic: coverage_prepare)
}

int op_mlp_correction_layers(op_handle* h, uint64_t* layer_mask) {
  if (!h || !layer_mask) return fail(h, OP_ERR_INVALID, "op_mlp_correction_layers: NULL argument");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  *layer_mask = mlp_by_layer(*h->ks) ? (h->mlp_layers & opp::all_layers_mask(h->cfg.num_layers)) : 0ull;
  return OP_OK;
}

int op_select_mlp_correction_layers(op_handle* h, uint64_t layer_mask) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_select_mlp_correction_layers: NULL handle");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  if (h->forced_set != OP_KS_F16_MLP_F8 && h->forced_set != OP_KS_F16_MLP_F8_W)
    return fail(h, OP_ERR_STATE, "op_select_mlp_correction_layers: pin kernel set %d or %d first (op_select_kernel_set / op_calibrate)", OP_KS_F16_MLP_F8_W,
                OP_KS_F16_MLP_F8);
  if (h->cfg.num_layers > 64) return fail(h, OP_ERR_UNSUPPORTED, "op_select_mlp_correction_layers: more than 64 layers");
  return pin(h, h->forced_set, layer_mask);
}

int op_calibrate(op_handle* h, float tolerance, const int32_t* ids_host, const int32_t* cu_seqlens_host, int n_seqs,
                 op_calibration* report) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_calibrate: NULL handle");
  if (report && report->struct_bytes != sizeof(op_calibration))
    return fail(h, OP_ERR_INVALID, "op_calibrate: op_calibration.struct_bytes=%u, library expects %zu", report->struct_bytes, sizeof(op_calibration));
  if (!(tolerance >= 0.f)) return fail(h, OP_ERR_INVALID, "op_calibrate: tolerance must be >= 0");
  if ((ids_host == nullptr) != (cu_seqlens_host == nullptr) || (ids_host && n_seqs <= 0))
    return fail(h, OP_ERR_INVALID, "op_calibrate: ids_host / cu_seqlens_host / n_seqs must be given together");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  // the caller's batch is checked BEFORE the handle's state is touched: a refused call leaves a pinned set where it was
  if (ids_host) {
    const opp::Refusal bad = opp::check_calibration_batch(ids_host, cu_seqlens_host, n_seqs, h->cfg.max_position_embeddings, h->cfg.vocab_size);
    if (bad.code != OP_OK) return fail(h, bad);
  }
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  h->cov_clear = true;  // whatever set comes out, it has seen no real row
  CalibrationVisit visit(h);

  // the default selection and its (hi, lo) bf16 realisation = the reference of the comparison
  OP_TRY(pin(h, -1));
  const int default_set = h->set;
  h->f8_off = true;
  OP_TRY(pin(h, -1));
  // OP_CAL_REFERENCE_F32 on a handle with the fp32 packs: kernel set "fp32" is the reference, the (hi, lo) bf16 set a candidate
  // like any other (where it is cheaper than the default)
  const bool ref_f32 = report && (report->flags & OP_CAL_REFERENCE_F32) != 0 && h->set >= 0 && opp::set_available(select_state(h), OP_KS_F32);
  const int reference_set = ref_f32 ? (int)OP_KS_F32 : h->set;
  h->f8_off = visit.f8_off;
  OP_TRY(pin(h, -1));

  op_calibration rep;
  memset(&rep, 0, sizeof(rep));
  rep.struct_bytes = sizeof(rep);
  rep.tolerance = tolerance;
  rep.reference_set = reference_set;
  rep.default_set = default_set;
  rep.chosen_set = default_set;
  rep.flags = report ? report->flags : 0u;
  auto finish = [&]() -> int {
    if (report) *report = rep;
    return OP_OK;
  };
  // nothing to measure: whatever was pinned before the call stays pinned
  auto finish_unchanged = [&]() -> int {
    OP_TRY(visit.restore_pin());
    rep.chosen_set = h->set;
    return finish();
  };
  if (default_set < 0 || reference_set < 0) return finish_unchanged();  // a custom policy on the all-terms kernels: nothing cheaper is defined
  const std::vector<int> cand = opp::calibration_candidates(select_state(h), default_set);
  if (cand.empty() && !ref_f32) return finish_unchanged();  // (fp32 reference: the default itself is still measured against it)

  std::vector<int32_t> ids, cu;
  if (ids_host) {
    cu.assign(cu_seqlens_host, cu_seqlens_host + n_seqs + 1);
    ids.assign(ids_host, ids_host + cu[n_seqs]);
  } else {
    synthetic_calibration_rows(h, ids, cu);
    n_seqs = (int)cu.size() - 1;
  }
  const int total = cu[n_seqs];
  int max_len = 0;
  for (int s = 0; s < n_seqs; ++s) max_len = std::max(max_len, cu[s + 1] - cu[s]);
  rep.n_rows = n_seqs;
  rep.n_tokens = total;

  size_t ws_bytes = op_workspace_bytes(h, n_seqs, total, max_len);
  // the largest workspace of the sets that run: the fp32 set's (its planes follow everybody's regions)
  if (ref_f32) ws_bytes = std::max(ws_bytes, forward_layout(h, n_seqs, total, max_len, true).bytes);
  const size_t n_prune = (size_t)total * 2, n_rank = (size_t)n_seqs * h->nl;
  int32_t *ids_dev = nullptr, *cu_dev = nullptr;
  float* out_dev = nullptr;
  void* ws_dev = nullptr;
  hipStream_t st = nullptr;
  auto release = [&]() {
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(ids_dev);
    (void)hipFree(cu_dev);
    (void)hipFree(out_dev);
    (void)hipFree(ws_dev);
  };
  hipError_t e = hipMalloc((void**)&ids_dev, ids.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&cu_dev, cu.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&out_dev, (n_prune + n_rank) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&ws_dev, ws_bytes + 256);
  if (e == hipSuccess) e = hipStreamCreate(&st);
  if (e == hipSuccess) e = hipMemcpy(ids_dev, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(cu_dev, cu.data(), cu.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    release();
    return fail(h, OP_ERR_HIP, "op_calibrate: staging failed: %s", hipGetErrorString(e));
  }
  void* ws_aligned = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(ws_dev) + 255) / 256 * 256);
  std::vector<float> ref(n_prune + n_rank), got(n_prune + n_rank);
  auto run = [&](int set, std::vector<float>& out, uint64_t mlp_layers) -> int {
    OP_TRY(pin(h, set, mlp_layers));
    OP_TRY(op_forward_packed(h, ids_dev, cu_dev, cu.data(), n_seqs, total, max_len, out_dev, out_dev + n_prune, nullptr, ws_aligned,
                             ws_bytes, st));
    OP_HIP(h, hipStreamSynchronize(st));
    OP_HIP(h, hipMemcpy(out.data(), out_dev, out.size() * sizeof(float), hipMemcpyDeviceToHost));
    return OP_OK;
  };
  bool have_ref = false;  // the search's first measurement is the reference's own run
  auto measure = [&](int set, uint64_t mlp_layers) -> opp::Measurement {
    const bool is_ref = !have_ref;
    have_ref = true;
    const int run_rc = run(set, is_ref ? ref : got, mlp_layers);
    if (run_rc != OP_OK) return {run_rc, INFINITY};
    if (!is_ref) return {OP_OK, opp::max_diff(got, ref)};
    bool ref_finite = true;
    for (float v : ref) ref_finite = ref_finite && std::isfinite(v);
    return {OP_OK, ref_finite ? 0.f : INFINITY};
  };
  const opp::SearchResult found = opp::calibration_search(cand, reference_set, default_set, tolerance, rep.flags, h->cfg.num_layers, measure);
  release();

  // what the search chose runs from now on (after an error: the default selection)
  visit.keep_pin();
  const uint64_t all_layers = opp::all_layers_mask(h->cfg.num_layers);
  const int rc2 = found.chosen >= 0 ? pin(h, found.chosen, found.mlp_layers | ~all_layers) : pin(h, -1);
  if (found.rc != OP_OK) return found.rc;
  if (rc2 != OP_OK) return rc2;
  rep.default_err = found.default_err;
  rep.n_candidates = found.n_candidates;
  std::copy(found.candidate_set, found.candidate_set + 16, rep.candidate_set);
  std::copy(found.candidate_err, found.candidate_err + 16, rep.candidate_err);
  rep.mlp_layers_err = found.mlp_layers_err;
  rep.chosen_set = h->set;
  rep.mlp_layers = mlp_by_layer(*h->ks) ? (h->mlp_layers & all_layers) : 0ull;
  return finish();
}

int op_effective_policy(op_handle* h, uint8_t* terms_out, int* kernel_set) {
  if (!h || !terms_out || !kernel_set) return fail(h, OP_ERR_INVALID, "op_effective_policy: NULL argument");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  terms_out[OP_FAM_WQKV] = (uint8_t)h->eff.wqkv;
  terms_out[OP_FAM_QK] = (uint8_t)h->eff.qk;
  terms_out[OP_FAM_PV] = (uint8_t)h->eff.pv;
  terms_out[OP_FAM_ATTN_OUT] = (uint8_t)h->eff.attn_out;
  terms_out[OP_FAM_WI] = (uint8_t)h->eff.wi;
  terms_out[OP_FAM_MLP_OUT] = (uint8_t)h->eff.mlp_out;
  *kernel_set = h->set;
  return OP_OK;
}

}  // extern "C"
