// op_services.hip -- C ABI: the small services around a forward, each a check of its arguments and one launch through its
// launch unit: the padded [B, L] boundary (pack / unpack), op_loss, the running audit (coverage, gather, compare),
// op_segment_means, op_assemble_rows, the planned / located fragment means, op_sentence_decisions.
#include "op_handle.h"
#include "opk_padded.hip.h"
#include "opk_segment_mean.hip.h"

extern "C" {

int op_segment_means(op_handle* h, const float* keep_prob_dev, int n_values, const int32_t* seg_dev, int n_seg,
                     float* out_dev, void* hip_stream) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_segment_means: NULL handle");
  if (n_seg < 0 || n_values < 0 || (n_seg > 0 && (!keep_prob_dev || !seg_dev || !out_dev)))
    return fail(h, OP_ERR_INVALID, "op_segment_means: NULL buffer or negative count");
  if (n_seg == 0) return OP_OK;
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)((n_seg + 127) / 128)), dim3(128), 0, (hipStream_t)hip_stream,
                     keep_prob_dev, seg_dev, n_seg, n_values, out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_pack_padded(op_handle* h, const void* ids_dev, int ids_dtype, const void* mask_dev, int mask_dtype, int n_rows, int width,
                   int32_t* ids_packed_dev, int32_t* cu_seqlens_dev, int32_t* cu_seqlens_host, op_padded_report* report,
                   void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!report) return fail(h, OP_ERR_INVALID, "op_pack_padded: report is NULL");
  if (report->struct_bytes != sizeof(op_padded_report))
    return fail(h, OP_ERR_INVALID, "op_pack_padded: op_padded_report.struct_bytes is %u, expected %zu", report->struct_bytes,
                sizeof(op_padded_report));
  if (ids_dtype != OP_INT_I32 && ids_dtype != OP_INT_I64)
    return fail(h, OP_ERR_INVALID, "op_pack_padded: ids_dtype %d is neither OP_INT_I32 nor OP_INT_I64", ids_dtype);
  if (mask_dev && mask_dtype != OP_INT_I32 && mask_dtype != OP_INT_I64 && mask_dtype != OP_INT_U8)
    return fail(h, OP_ERR_INVALID, "op_pack_padded: unknown mask_dtype %d", mask_dtype);
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "op_pack_padded: negative n_rows %d", n_rows);
  if (width < 0) return fail(h, OP_ERR_INVALID, "op_pack_padded: negative width %d", width);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  if (cells > (int64_t)INT32_MAX)  // (the first offender of each check is a 32-bit linear index)
    return fail(h, OP_ERR_INVALID, "op_pack_padded: n_rows * width = %lld exceeds 2^31 - 1", (long long)cells);
  if (!cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_pack_padded: cu_seqlens_dev is NULL");
  if (!cu_seqlens_host) return fail(h, OP_ERR_INVALID, "op_pack_padded: cu_seqlens_host is NULL");
  if (cells > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_pack_padded: ids_dev is NULL");
  if (cells > 0 && !ids_packed_dev) return fail(h, OP_ERR_INVALID, "op_pack_padded: ids_packed_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_pack_padded: NULL handle");
  report->total_tokens = report->max_seqlen = report->status = 0;
  report->mask_row = report->mask_col = report->id_row = report->id_col = -1;
  report->id_value = 0;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(h, OP_ERR_STATE, "op_pack_padded: the stream is being captured (the call synchronises it to read the batch's size back)");
  if (cells == 0) {  // nothing to launch: every row is empty
    OP_HIP(h, hipMemsetAsync(cu_seqlens_dev, 0, ((size_t)n_rows + 1) * sizeof(int32_t), stream));
    std::fill(cu_seqlens_host, cu_seqlens_host + n_rows + 1, 0);
    return OP_OK;
  }
  if (!h->pad_status) OP_TRY(dev_alloc(h, &h->pad_status, (size_t)opk::PAD_ST_WORDS));
  const size_t n_cu = (size_t)n_rows + 1, words = n_cu + opk::PAD_ST_WORDS;
  if (h->pad_host_words < words) {
    if (h->pad_host) (void)hipHostFree(h->pad_host);
    h->pad_host = nullptr;
    h->pad_host_words = 0;
    void* p = nullptr;
    const size_t grown = std::max<size_t>(words, 4096);
    hipError_t e = hipHostMalloc(&p, grown * sizeof(int32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", grown * sizeof(int32_t), hipGetErrorString(e));
    h->pad_host = reinterpret_cast<int32_t*>(p);
    h->pad_host_words = grown;
  }
  OP_HIP(h, hipMemsetAsync(h->pad_status, 0xff, 2 * sizeof(uint32_t), stream));  // the two atomicMin words = PAD_ST_NONE
  if (!opl::launch_padded_pack(stream, ids_dev, ids_dtype, mask_dev, mask_dtype, n_rows, width, h->V, ids_packed_dev, cu_seqlens_dev,
                               h->pad_status))
    return fail(h, OP_ERR_UNSUPPORTED, "op_pack_padded: no kernel for ids_dtype %d / mask_dtype %d", ids_dtype, mask_dtype);
  OP_HIP(h, hipGetLastError());
  uint32_t* st_host = reinterpret_cast<uint32_t*>(h->pad_host + n_cu);
  OP_HIP(h, hipMemcpyAsync(h->pad_host, cu_seqlens_dev, n_cu * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipMemcpyAsync(st_host, h->pad_status, opk::PAD_ST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));  // the one synchronisation: the forward's grids need T and the longest row
  std::memcpy(cu_seqlens_host, h->pad_host, n_cu * sizeof(int32_t));
  report->total_tokens = (int32_t)st_host[opk::PAD_ST_TOTAL];
  report->max_seqlen = (int32_t)st_host[opk::PAD_ST_MAXLEN];
  const uint32_t bad_mask = st_host[opk::PAD_ST_MASK], bad_id = st_host[opk::PAD_ST_ID];
  if (bad_mask != opk::PAD_ST_NONE) {
    report->status |= 1;
    report->mask_row = (int32_t)(bad_mask / (uint32_t)width);
    report->mask_col = (int32_t)(bad_mask % (uint32_t)width);
  }
  if (bad_id != opk::PAD_ST_NONE) {
    report->status |= 2;
    report->id_row = (int32_t)(bad_id / (uint32_t)width);
    report->id_col = (int32_t)(bad_id % (uint32_t)width);
    report->id_value = (int64_t)((uint64_t)st_host[opk::PAD_ST_IDVAL] | ((uint64_t)st_host[opk::PAD_ST_IDVAL + 1] << 32));
  }
  if (report->status == 0) return OP_OK;
  char mask_text[160] = "", id_text[200] = "";
  if (report->status & 1)
    snprintf(mask_text, sizeof(mask_text), "the attention mask is not ones-then-zeros at row %d, column %d", report->mask_row, report->mask_col);
  if (report->status & 2)
    snprintf(id_text, sizeof(id_text), "token id %lld at row %d, column %d is outside the embedding table (vocab_size %d)",
             (long long)report->id_value, report->id_row, report->id_col, h->V);
  return fail(h, OP_ERR_INVALID, "op_pack_padded: %s%s%s", mask_text, report->status == 3 ? "; " : "", id_text);
}

int op_unpack_padded(op_handle* h, const float* packed_dev, const int32_t* cu_seqlens_dev, int n_rows, int width, int channels,
                     float* padded_dev, void* hip_stream) {
  if (channels != 1 && channels != 2) return fail(h, OP_ERR_INVALID, "op_unpack_padded: channels is %d, expected 1 or 2", channels);
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "op_unpack_padded: negative n_rows %d", n_rows);
  if (width < 0) return fail(h, OP_ERR_INVALID, "op_unpack_padded: negative width %d", width);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  if (cells > (int64_t)INT32_MAX)
    return fail(h, OP_ERR_INVALID, "op_unpack_padded: n_rows * width = %lld exceeds 2^31 - 1", (long long)cells);
  if (cells > 0 && !packed_dev) return fail(h, OP_ERR_INVALID, "op_unpack_padded: packed_dev is NULL");
  if (cells > 0 && !cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_unpack_padded: cu_seqlens_dev is NULL");
  if (cells > 0 && !padded_dev) return fail(h, OP_ERR_INVALID, "op_unpack_padded: padded_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_unpack_padded: NULL handle");
  if (cells == 0) return OP_OK;
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  if (!opl::launch_padded_scatter(reinterpret_cast<hipStream_t>(hip_stream), packed_dev, cu_seqlens_dev, n_rows, width, channels, padded_dev))
    return fail(h, OP_ERR_UNSUPPORTED, "op_unpack_padded: no kernel for %d channels", channels);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_loss(op_handle* h, const op_loss_request* req, float* loss_dev, op_loss_report* report, void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!req) return fail(h, OP_ERR_INVALID, "op_loss: request is NULL");
  if (req->struct_bytes != sizeof(op_loss_request))
    return fail(h, OP_ERR_INVALID, "op_loss: op_loss_request.struct_bytes is %u, expected %zu", req->struct_bytes, sizeof(op_loss_request));
  if (report && report->struct_bytes != sizeof(op_loss_report))
    return fail(h, OP_ERR_INVALID, "op_loss: op_loss_report.struct_bytes is %u, expected %zu", report->struct_bytes, sizeof(op_loss_report));
  const int kind = req->kind, dtype = req->labels_dtype;
  if (kind < OP_LOSS_TOKEN_CE || kind > OP_LOSS_RANK_MSE) return fail(h, OP_ERR_INVALID, "op_loss: unknown kind %d", kind);
  if (dtype != OP_INT_I32 && dtype != OP_INT_I64 && dtype != OP_INT_U8 && dtype != OP_LABELS_F32)
    return fail(h, OP_ERR_INVALID, "op_loss: unknown labels_dtype %d", dtype);
  const bool token = kind == OP_LOSS_TOKEN_CE, integer = token || kind == OP_LOSS_RANK_CE;
  if (integer ? (dtype != OP_INT_I32 && dtype != OP_INT_I64) : dtype != OP_LABELS_F32)
    return fail(h, OP_ERR_INVALID, "op_loss: labels_dtype %d does not fit kind %d (%s)", dtype, kind,
                integer ? "OP_INT_I32 or OP_INT_I64" : "OP_LABELS_F32");
  if (req->n_rows < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative n_rows %d", req->n_rows);
  if (req->channels < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative channels %d", req->channels);
  if (token && req->width < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative width %d", req->width);
  if (token && req->total_tokens < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative total_tokens %d", req->total_tokens);
  if (token && req->channels != 2) return fail(h, OP_ERR_INVALID, "op_loss: channels is %d, OP_LOSS_TOKEN_CE takes 2", req->channels);
  if (kind == OP_LOSS_RANK_BCE && req->channels != 1)
    return fail(h, OP_ERR_INVALID, "op_loss: channels is %d, OP_LOSS_RANK_BCE takes 1", req->channels);
  if (kind == OP_LOSS_RANK_CE && req->channels < 2)
    return fail(h, OP_ERR_INVALID, "op_loss: channels is %d, OP_LOSS_RANK_CE takes at least 2", req->channels);
  const int64_t label_cells = (int64_t)req->n_rows * (int64_t)(token ? req->width : kind == OP_LOSS_RANK_MSE ? req->channels : 1);
  const int64_t logit_rows = token ? (int64_t)req->total_tokens : (int64_t)req->n_rows;
  if (token && label_cells > (int64_t)INT32_MAX)  // (the first offender is a 32-bit linear index)
    return fail(h, OP_ERR_INVALID, "op_loss: n_rows * width = %lld exceeds 2^31 - 1", (long long)label_cells);
  if (!token && (int64_t)req->n_rows * (int64_t)req->channels > (int64_t)INT32_MAX)
    return fail(h, OP_ERR_INVALID, "op_loss: n_rows * channels = %lld exceeds 2^31 - 1", (long long)req->n_rows * req->channels);
  if (token && (int64_t)req->total_tokens > label_cells)
    return fail(h, OP_ERR_INVALID, "op_loss: total_tokens %d exceeds n_rows * width = %lld", req->total_tokens, (long long)label_cells);
  if (!loss_dev) return fail(h, OP_ERR_INVALID, "op_loss: loss_dev is NULL");
  if (logit_rows * req->channels > 0 && !req->logits_dev) return fail(h, OP_ERR_INVALID, "op_loss: logits_dev is NULL");
  if (label_cells > 0 && !req->labels_dev) return fail(h, OP_ERR_INVALID, "op_loss: labels_dev is NULL");
  if (token && req->n_rows > 0 && !req->cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_loss: cu_seqlens_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_loss: NULL handle");
  if (report) {
    report->status = 0;
    report->bad_row = report->bad_col = -1;
    report->bad_value = report->count = 0;
    report->sum = 0.0;
    report->loss = 0.0f;
    report->reserved = 0;
  }

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  if (report) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
    if (capturing != hipStreamCaptureStatusNone)
      return fail(h, OP_ERR_STATE, "op_loss: the stream is being captured (a call with a report synchronises it to read the result back)");
    if (!h->loss_host) {
      void* p = nullptr;
      hipError_t e = hipHostMalloc(&p, sizeof(opk::LossResult), hipHostMallocDefault);
      if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", sizeof(opk::LossResult), hipGetErrorString(e));
      h->loss_host = reinterpret_cast<opk::LossResult*>(p);
    }
  }
  opk::LossParams lp;
  lp.logits = req->logits_dev;
  lp.labels = req->labels_dev;
  lp.cu = token ? req->cu_seqlens_dev : nullptr;
  lp.terms = req->terms_dev;
  lp.n_rows = req->n_rows;
  lp.width = token ? req->width : 0;
  lp.channels = req->channels;
  lp.total_tokens = token ? req->total_tokens : 0;
  lp.ignore_index = (long long)req->ignore_index;
  if (!opl::launch_loss(stream, kind, dtype, lp, h->loss_scratch, loss_dev))
    return fail(h, OP_ERR_UNSUPPORTED, "op_loss: no kernel for kind %d / labels_dtype %d", kind, dtype);
  OP_HIP(h, hipGetLastError());
  if (!report) return OP_OK;
  OP_HIP(h, hipMemcpyAsync(h->loss_host, &h->loss_scratch->result, sizeof(opk::LossResult), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));  // the one synchronisation: the caller asked for the result on the host
  const opk::LossResult& res = *h->loss_host;
  report->count = (int64_t)res.count;
  report->sum = res.sum;
  report->loss = res.loss;
  if (res.status == 0) return OP_OK;
  report->status = 1;
  report->bad_value = (int64_t)res.bad_value;
  report->bad_row = token ? (int32_t)(res.bad_index / (uint32_t)req->width) : (int32_t)res.bad_index;
  report->bad_col = token ? (int32_t)(res.bad_index % (uint32_t)req->width) : 0;
  return fail(h, OP_ERR_INVALID, "op_loss: label %lld at row %d, column %d is outside 0 <= label < %d and is not ignore_index (%lld)",
              (long long)report->bad_value, report->bad_row, report->bad_col, req->channels, (long long)req->ignore_index);
}

// The coverage belongs to one arithmetic: the kernel set (and the layer mask of sets 8 / 9) it was collected under.  It is
// emptied lazily, on the stream of the call that next looks at it -- after op_coverage_reset / op_calibrate / op_load_weight
// of the embedding table, and whenever the handle runs another arithmetic than the one the coverage belongs to.  So
// op_select_kernel_set enqueues nothing (the default audit mode never pays for a feature it does not use), and an audit's
// detour through the reference set and back finds the coverage as it left it.
static int coverage_prepare(op_handle* h, hipStream_t stream) {
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  const int set = h->resolved ? h->set : -2;
  const uint64_t mlp = (h->resolved && mlp_by_layer(*h->ks)) ? h->mlp_layers : 0ull;
  if (h->cov_clear || set != h->cov_set || mlp != h->cov_mlp_layers) {
    OP_HIP(h, hipMemsetAsync(h->cov_bits, 0, (((size_t)h->V + 31) / 32) * sizeof(uint32_t), stream));
    OP_HIP(h, hipMemsetAsync(h->cov_state, 0, opl::COV_WORDS * sizeof(uint32_t), stream));
    h->cov_clear = false;
    h->cov_set = set;
    h->cov_mlp_layers = mlp;
  }
  return OP_OK;
}

int op_coverage_scan(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                     int32_t* row_novel_dev, op_coverage_report* report, void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!report) return fail(h, OP_ERR_INVALID, "op_coverage_scan: report is NULL");
  if (report->struct_bytes != sizeof(op_coverage_report))
    return fail(h, OP_ERR_INVALID, "op_coverage_scan: op_coverage_report.struct_bytes is %u, expected %zu", report->struct_bytes,
                sizeof(op_coverage_report));
  if (n_seqs < 0) return fail(h, OP_ERR_INVALID, "op_coverage_scan: negative n_seqs %d", n_seqs);
  if (total_tokens < 0) return fail(h, OP_ERR_INVALID, "op_coverage_scan: negative total_tokens %d", total_tokens);
  if (n_seqs > 0 && !cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_coverage_scan: cu_seqlens_dev is NULL");
  if (n_seqs > 0 && !row_novel_dev) return fail(h, OP_ERR_INVALID, "op_coverage_scan: row_novel_dev is NULL");
  if (n_seqs > 0 && total_tokens > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_coverage_scan: ids_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_coverage_scan: NULL handle");
  report->novel_tokens = report->longest_row_tokens = report->max_audited_tokens = 0;
  report->longest_row = -1;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(h, OP_ERR_STATE, "op_coverage_scan: the stream is being captured (the call synchronises it to read the report back)");
  if (!h->cov_host) {
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, opl::COV_WORDS * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", opl::COV_WORDS * sizeof(uint32_t), hipGetErrorString(e));
    h->cov_host = reinterpret_cast<uint32_t*>(p);
  }
  OP_TRY(coverage_prepare(h, stream));
  OP_HIP(h, hipMemsetAsync(h->cov_state + opl::COV_NOVEL, 0, (opl::COV_WORDS - opl::COV_NOVEL) * sizeof(uint32_t), stream));
  if (n_seqs > 0) {
    opl::launch_coverage_scan(stream, ids_dev, cu_seqlens_dev, n_seqs, total_tokens, h->V, h->cov_bits, row_novel_dev, h->cov_state);
    OP_HIP(h, hipGetLastError());
  }
  OP_HIP(h, hipMemcpyAsync(h->cov_host, h->cov_state, opl::COV_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));  // the one synchronisation: the caller decides on the host whether to audit
  report->max_audited_tokens = (int32_t)h->cov_host[opl::COV_MAXLEN];
  report->novel_tokens = (int32_t)h->cov_host[opl::COV_NOVEL];
  if (n_seqs > 0) {
    report->longest_row_tokens = (int32_t)h->cov_host[opl::COV_LONGEST + 1];
    report->longest_row = (int32_t)~h->cov_host[opl::COV_LONGEST];
  }
  return OP_OK;
}

// the checks commit, gather and compare share: a packed batch and a list of its rows
static int check_row_list(op_handle* h, const char* who, const void* cu_seqlens_dev, int n_seqs, int total_tokens, const void* rows_dev,
                          int n_rows) {
  if (n_seqs < 0) return fail(h, OP_ERR_INVALID, "%s: negative n_seqs %d", who, n_seqs);
  if (total_tokens < 0) return fail(h, OP_ERR_INVALID, "%s: negative total_tokens %d", who, total_tokens);
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "%s: negative n_rows %d", who, n_rows);
  if (n_rows > 0 && !cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "%s: cu_seqlens_dev is NULL", who);
  if (n_rows > 0 && !rows_dev) return fail(h, OP_ERR_INVALID, "%s: rows_dev is NULL", who);
  return OP_OK;
}

int op_coverage_commit(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                       const int32_t* rows_dev, int n_rows, void* hip_stream) {
  OP_TRY(check_row_list(h, "op_coverage_commit", cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows));
  if (n_rows > 0 && total_tokens > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_coverage_commit: ids_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_coverage_commit: NULL handle");
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  OP_TRY(coverage_prepare(h, stream));
  if (n_rows == 0) return OP_OK;
  opl::launch_coverage_commit(stream, ids_dev, cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows, h->V, h->cov_bits, h->cov_state);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_coverage_reset(op_handle* h) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_coverage_reset: NULL handle");
  h->cov_clear = true;
  return OP_OK;
}

int op_gather_rows(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                   const int32_t* rows_dev, int n_rows, int32_t* sub_ids_dev, int32_t* sub_cu_dev, void* hip_stream) {
  OP_TRY(check_row_list(h, "op_gather_rows", cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows));
  if (!sub_cu_dev) return fail(h, OP_ERR_INVALID, "op_gather_rows: sub_cu_dev is NULL");
  if (n_rows > 0 && total_tokens > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_gather_rows: ids_dev is NULL");
  if (n_rows > 0 && total_tokens > 0 && !sub_ids_dev) return fail(h, OP_ERR_INVALID, "op_gather_rows: sub_ids_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_gather_rows: NULL handle");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  if (n_rows == 0) {
    OP_HIP(h, hipMemsetAsync(sub_cu_dev, 0, sizeof(int32_t), stream));
    return OP_OK;
  }
  opl::launch_gather_rows(stream, ids_dev, cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows, sub_ids_dev, sub_cu_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_audit_compare(op_handle* h, const float* prune_dev, const float* rank_dev, const int32_t* cu_seqlens_dev, int n_seqs,
                     int total_tokens, const int32_t* rows_dev, int n_rows, const float* sub_prune_dev, const float* sub_rank_dev,
                     const int32_t* sub_cu_dev, float* err_dev, void* hip_stream) {
  OP_TRY(check_row_list(h, "op_audit_compare", cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows));
  if (!err_dev) return fail(h, OP_ERR_INVALID, "op_audit_compare: err_dev is NULL");
  if (n_rows > 0 && total_tokens > 0 && (!prune_dev || !sub_prune_dev)) return fail(h, OP_ERR_INVALID, "op_audit_compare: prune_dev / sub_prune_dev is NULL");
  if (n_rows > 0 && (!rank_dev || !sub_rank_dev)) return fail(h, OP_ERR_INVALID, "op_audit_compare: rank_dev / sub_rank_dev is NULL");
  if (n_rows > 0 && !sub_cu_dev) return fail(h, OP_ERR_INVALID, "op_audit_compare: sub_cu_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_audit_compare: NULL handle");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  OP_HIP(h, hipMemsetAsync(err_dev, 0, sizeof(float), stream));  // +0.0: the kernel's atomicMax starts from it
  if (n_rows == 0) return OP_OK;
  opl::launch_audit_compare(stream, prune_dev, rank_dev, cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows, sub_prune_dev, sub_rank_dev,
                            sub_cu_dev, h->nl, err_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_assemble_rows(op_handle* h, const op_assemble_request* req, int32_t* ids_dev, void* hip_stream) {
  // (the request's own fields first, on the host copies: nothing is enqueued before the last check)
  if (!req) return fail(h, OP_ERR_INVALID, "op_assemble_rows: request is NULL");
  if (req->struct_bytes != sizeof(op_assemble_request))
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: op_assemble_request.struct_bytes is %u, expected %zu", req->struct_bytes,
                sizeof(op_assemble_request));
  if (req->n_frag < 0 || req->n_queries < 0 || req->n_rows < 0 || req->total_tokens < 0)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: negative count (n_frag %d, n_queries %d, n_rows %d, total_tokens %d)", req->n_frag,
                req->n_queries, req->n_rows, req->total_tokens);
  const int32_t* const pieces[3] = {req->prefix, req->middle, req->suffix};
  const int n_pieces[3] = {req->n_prefix, req->n_middle, req->n_suffix};
  static const char* const piece_names[3] = {"prefix", "middle", "suffix"};
  for (int i = 0; i < 3; ++i) {
    if (n_pieces[i] < 0 || n_pieces[i] > OP_ASSEMBLE_MAX_PIECE)
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: %s holds %d ids, expected 0 .. %d", piece_names[i], n_pieces[i], OP_ASSEMBLE_MAX_PIECE);
    if (n_pieces[i] > 0 && !pieces[i]) return fail(h, OP_ERR_INVALID, "op_assemble_rows: %s is NULL", piece_names[i]);
  }
  if (req->n_rows == 0) {
    if (req->total_tokens != 0) return fail(h, OP_ERR_INVALID, "op_assemble_rows: no rows but total_tokens is %d", req->total_tokens);
    if (!h) return fail(nullptr, OP_ERR_INVALID, "op_assemble_rows: NULL handle");
    return OP_OK;
  }
  if (!req->plan_dev || !req->plan_host || !req->cu_seqlens_dev || !req->cu_seqlens_host || !req->q_off_dev || !req->q_off_host ||
      !req->frag_off_dev || !req->frag_off_host)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: a plan, cu_seqlens or offset buffer is NULL");
  if (req->q_off_host[0] != 0 || req->frag_off_host[0] != 0)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: offsets do not start at 0");
  for (int q = 0; q < req->n_queries; ++q)
    if (req->q_off_host[q + 1] < req->q_off_host[q]) return fail(h, OP_ERR_INVALID, "op_assemble_rows: q_off decreases at query %d", q);
  const int n_query_tokens = req->q_off_host[req->n_queries], n_corpus = req->frag_off_host[req->n_frag];
  if (n_corpus < 0) return fail(h, OP_ERR_INVALID, "op_assemble_rows: frag_off ends at %d", n_corpus);
  if (req->cu_seqlens_host[0] != 0) return fail(h, OP_ERR_INVALID, "op_assemble_rows: cu_seqlens_host[0] is %d", req->cu_seqlens_host[0]);
  bool any_query = false, any_ctx = false;
  int64_t at = 0;
  for (int r = 0; r < req->n_rows; ++r) {
    const int32_t* pr = req->plan_host + (size_t)r * 4;
    const int query = pr[0], first = pr[1], n = pr[2], clip = pr[3];
    if (query < 0 || query >= req->n_queries) return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d names query %d of %d", r, query, req->n_queries);
    if (first < 0 || n < 0 || first > req->n_frag - n)
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d takes fragments %d .. %d + %d of %d", r, first, first, n, req->n_frag);
    int64_t ctx = 0;
    if (n > 0) {
      const int32_t* fo = req->frag_off_host + first;
      if (fo[0] < 0 || fo[1] < fo[0] || fo[n] < fo[1] || fo[n] > n_corpus)
        return fail(h, OP_ERR_INVALID, "op_assemble_rows: frag_off decreases or leaves the corpus at row %d", r);
      if (clip < 0 || clip > fo[1] - fo[0])
        return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d clips its first fragment of %d ids to %d", r, fo[1] - fo[0], clip);
      ctx = clip > 0 ? (int64_t)clip + (fo[n] - fo[1]) : (int64_t)(fo[n] - fo[0]);
    } else if (clip != 0 && clip != -1) {
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d has clip %d and no fragment", r, clip);
    }
    const int row_suffix = (n == 0 && clip == -1) ? 0 : n_pieces[2];
    const int q_len = req->q_off_host[query + 1] - req->q_off_host[query];
    any_query |= q_len > 0;
    any_ctx |= ctx > 0;
    at += (int64_t)n_pieces[0] + q_len + n_pieces[1] + ctx + row_suffix;
    if (at > (int64_t)INT32_MAX || (int64_t)req->cu_seqlens_host[r + 1] != at)
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: cu_seqlens_host[%d] is %d, the plan's rows end at %lld", r + 1,
                  req->cu_seqlens_host[r + 1], (long long)at);
  }
  if (at != (int64_t)req->total_tokens)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: the plan's rows hold %lld ids, total_tokens is %d", (long long)at, req->total_tokens);
  if (at > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_assemble_rows: ids_dev is NULL");
  if (any_query && !req->query_ids_dev) return fail(h, OP_ERR_INVALID, "op_assemble_rows: query_ids_dev is NULL");
  if (any_ctx && !req->corpus_dev) return fail(h, OP_ERR_INVALID, "op_assemble_rows: corpus_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_assemble_rows: NULL handle");
  if (at == 0) return OP_OK;
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_assemble_rows(reinterpret_cast<hipStream_t>(hip_stream), req->corpus_dev, req->frag_off_dev, req->n_frag, n_corpus,
                            req->query_ids_dev, req->q_off_dev, req->n_queries, n_query_tokens, pieces, n_pieces, req->plan_dev,
                            req->cu_seqlens_dev, req->n_rows, req->total_tokens, ids_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_planned_fragment_means(op_handle* h, const op_assemble_request* rows, const op_planned_means_request* req, void* hip_stream) {
  // (the requests first, on the host copies -- opp::check_planned_means: nothing is enqueued before the last check)
  const opp::Refusal refused = opp::check_planned_means(rows, req);
  if (refused.code != OP_OK) return fail(h, refused);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_planned_fragment_means: NULL handle");
  if (rows->n_rows == 0 || req->slot_off_host[rows->n_rows] == req->slot_off_host[0]) return OP_OK;  // (no fragment in any row)
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_planned_fragment_means(reinterpret_cast<hipStream_t>(hip_stream), *rows, *req);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_located_fragment_means(op_handle* h, const op_assemble_request* rows, const op_planned_means_request* req, const int32_t* ids_dev,
                              int32_t* ctx_start_out_dev, void* hip_stream) {
  const opp::Refusal refused = opp::check_located_means(rows, req, ids_dev, ctx_start_out_dev);
  if (refused.code != OP_OK) return fail(h, refused);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_located_fragment_means: NULL handle");
  if (rows->n_rows == 0) return OP_OK;  // (a row without fragments still gets its ctx_start)
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_located_fragment_means(reinterpret_cast<hipStream_t>(hip_stream), *rows, *req, ids_dev, ctx_start_out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_sentence_decisions(op_handle* h, const op_decisions_request* req, void* hip_stream) {
  const opp::Refusal refused = opp::check_decisions(req);
  if (refused.code != OP_OK) return fail(h, refused);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_sentence_decisions: NULL handle");
  if (req->n_instances == 0) return OP_OK;  // (n_out is 0 too: the instances tile the outputs)
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_sentence_decisions(reinterpret_cast<hipStream_t>(hip_stream), *req);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

}  // extern "C"
