// op_forward_masked.hip -- C ABI: op_forward_masked / op_masked_workspace_bytes, the forward under an arbitrary [n_rows][width]
// attention mask.  No kernel of its own: the call checks its arguments, carves its workspace, runs the id check with the dense
// cu_seqlens (op_launch_f32_masked.hip) and hands a dense batch with its key mask to the forward unit (forward_packed_impl with
// a MaskedReq: kernel set "fp32", the masked attention and heads swapped in).  op_forward_masked_native /
// op_masked_native_workspace_bytes: the same call on the handle's selected kernel set (MaskedReq::native; row and panel path).
#include "op_handle.h"

struct MaskedWorkspace {
  int32_t* cu;       // [n_rows + 1] = r * width
  uint32_t* status;  // the id check's word (opk::MASKED_ST_NONE: clear)
  float* vmean;      // [n_rows][H]
  char* forward;     // a forward workspace of kernel set "fp32" for n_rows sequences of `width` tokens
  size_t forward_bytes, bytes;
};

// (the regions in the order they are first written)
static void carve_masked(const op_handle* h, char* base, int n_rows, int width, MaskedWorkspace& ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up_sz(bytes, 256);
    return p;
  };
  ws.cu = reinterpret_cast<int32_t*>(take(((size_t)n_rows + 1) * 4));
  ws.status = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t)));
  ws.vmean = reinterpret_cast<float*>(take((size_t)n_rows * (size_t)h->H * sizeof(float)));
  ws.forward_bytes = forward_layout(h, n_rows, n_rows * width, width, /*f32=*/true).bytes;
  ws.forward = take(ws.forward_bytes);
  ws.bytes = off;
}

// op_forward_masked_native's regions (opp::masked_native_layout) over `base`
struct MaskedNativeWorkspace {
  int32_t* cu;
  uint32_t* status;
  uint8_t* key_row;
  float* vmean;
  char* forward;
  size_t forward_bytes, bytes;
};
static void carve_masked_native(const op_handle* h, char* base, int n_rows, int width, MaskedNativeWorkspace& ws) {
  ws.forward_bytes = forward_layout(h, n_rows, n_rows * width, width, /*f32=*/false).bytes;
  const opp::MaskedNativeLayout l = opp::masked_native_layout(h->H, h->chunk_rows, n_rows, width, ws.forward_bytes);
  ws.cu = reinterpret_cast<int32_t*>(base + l.cu);
  ws.status = reinterpret_cast<uint32_t*>(base + l.status);
  ws.key_row = reinterpret_cast<uint8_t*>(base + l.key_row);
  ws.vmean = reinterpret_cast<float*>(base + l.vmean);
  ws.forward = base + l.forward;
  ws.bytes = l.bytes;
}

// The id check of a dense batch on `stream` (synchronised once; a second time to read an offender's value): the dense cu_seqlens
// into cu_dev, the first id outside the table into the report.  `fn`: the entry point the refusal names.
static int masked_id_check(op_handle* h, const char* fn, const int32_t* ids_dev, int n_rows, int width, int32_t* cu_dev, uint32_t* status_dev,
                           op_masked_report* report, hipStream_t stream) {
  OP_HIP(h, hipMemsetAsync(status_dev, 0xff, sizeof(uint32_t), stream));
  opl::launch_masked_prepare(stream, ids_dev, n_rows, width, h->V, cu_dev, status_dev);
  OP_HIP(h, hipGetLastError());
  uint32_t bad = opk::MASKED_ST_NONE;
  OP_HIP(h, hipMemcpyAsync(&bad, status_dev, sizeof(bad), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));
  if (bad == opk::MASKED_ST_NONE) return OP_OK;
  int32_t value = 0;
  OP_HIP(h, hipMemcpyAsync(&value, ids_dev + bad, sizeof(value), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));
  report->status = 2;
  report->id_row = (int32_t)(bad / (uint32_t)width);
  report->id_col = (int32_t)(bad % (uint32_t)width);
  report->id_value = value;
  return fail(h, OP_ERR_INVALID, "%s: token id %lld at row %d, column %d is outside the embedding table (vocab_size %d)", fn,
              (long long)report->id_value, report->id_row, report->id_col, h->V);
}

extern "C" {

size_t op_masked_native_workspace_bytes(const op_handle* h, int n_rows, int width) {
  if (!h || n_rows < 0 || width < 0 || (int64_t)n_rows * (int64_t)width > (int64_t)INT32_MAX) return 0;
  MaskedNativeWorkspace ws;
  carve_masked_native(h, nullptr, n_rows, width, ws);
  return ws.bytes;
}

int op_forward_masked_native(op_handle* h, const int32_t* ids_dev, const uint8_t* mask_dev, int n_rows, int width, void* workspace,
                             size_t workspace_bytes, float* prune_out, float* rank_out, op_masked_report* report, void* hip_stream) {
  const char* const fn = "op_forward_masked_native";
  // (the arguments' own fields first: none of them needs the handle)
  const opp::Refusal bad_args = opp::check_masked_args(fn, report != nullptr, report ? report->struct_bytes : 0u, n_rows, width, ids_dev != nullptr,
                                                       mask_dev != nullptr, prune_out != nullptr, rank_out != nullptr, workspace != nullptr);
  if (bad_args.code != OP_OK) return fail(h, bad_args);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "%s: NULL handle", fn);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  report->status = 0;
  report->id_row = report->id_col = -1;
  report->id_value = 0;
  opp::Refusal unfit = opp::check_masked_native_handle(width, h->max_pos, h->row_path, h->panel_path, h->set);
  if (unfit.code != OP_OK) return fail(h, unfit);
  if (cells == 0) return OP_OK;
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;
  unfit = opp::check_masked_native_handle(width, h->max_pos, h->row_path, h->panel_path, h->set);  // (the selection may have been made just now)
  if (unfit.code != OP_OK) return fail(h, unfit);
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(h, OP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  MaskedNativeWorkspace ws;
  carve_masked_native(h, reinterpret_cast<char*>(workspace), n_rows, width, ws);
  if (workspace_bytes < ws.bytes) return fail(h, OP_ERR_WORKSPACE, "workspace has %zu bytes, need %zu", workspace_bytes, ws.bytes);

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(h, OP_ERR_STATE, "%s: the stream is being captured (the call synchronises it to read the id check back)", fn);
  // the dense cu_seqlens and the id check; its word comes back before the forward is enqueued: the embedding kernels only clamp
  OP_TRY(masked_id_check(h, fn, ids_dev, n_rows, width, ws.cu, ws.status, report, stream));

  std::vector<int32_t> cu_host((size_t)n_rows + 1);
  for (int r = 0; r <= n_rows; ++r) cu_host[(size_t)r] = r * width;
  PackedBatch b;
  b.ids_dev = ids_dev, b.cu_dev = ws.cu, b.cu_host = cu_host.data();
  b.n_seqs = n_rows, b.total_tokens = (int)cells, b.max_seqlen = width;
  b.prune_out = prune_out, b.rank_out = rank_out;
  b.workspace = ws.forward, b.workspace_bytes = ws.forward_bytes, b.stream = stream;
  MaskedReq msk;
  msk.key_ok = mask_dev;
  msk.vmean = ws.vmean;
  msk.cu_host = cu_host.data();
  msk.native = true;
  msk.key_row = ws.key_row;
  return forward_packed_impl(h, b, nullptr, &msk);
}

size_t op_masked_workspace_bytes(const op_handle* h, int n_rows, int width) {
  if (!h || n_rows < 0 || width < 0 || (int64_t)n_rows * (int64_t)width > (int64_t)INT32_MAX) return 0;
  MaskedWorkspace ws;
  carve_masked(h, nullptr, n_rows, width, ws);
  return ws.bytes;
}

int op_forward_masked(op_handle* h, const int32_t* ids_dev, const uint8_t* mask_dev, int n_rows, int width, void* workspace,
                      size_t workspace_bytes, float* prune_out, float* rank_out, op_masked_report* report, void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!report) return fail(h, OP_ERR_INVALID, "op_forward_masked: report is NULL");
  if (report->struct_bytes != sizeof(op_masked_report))
    return fail(h, OP_ERR_INVALID, "op_forward_masked: op_masked_report.struct_bytes is %u, expected %zu", report->struct_bytes,
                sizeof(op_masked_report));
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "op_forward_masked: negative n_rows %d", n_rows);
  if (width < 0) return fail(h, OP_ERR_INVALID, "op_forward_masked: negative width %d", width);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  if (cells > (int64_t)INT32_MAX)  // (tokens and the first offending id are 32-bit linear indices)
    return fail(h, OP_ERR_INVALID, "op_forward_masked: n_rows * width = %lld exceeds 2^31 - 1", (long long)cells);
  if (cells > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_forward_masked: ids_dev is NULL");
  if (cells > 0 && !mask_dev) return fail(h, OP_ERR_INVALID, "op_forward_masked: mask_dev is NULL");
  if (cells > 0 && !prune_out) return fail(h, OP_ERR_INVALID, "op_forward_masked: prune_logits_dev is NULL");
  if (cells > 0 && !rank_out) return fail(h, OP_ERR_INVALID, "op_forward_masked: rank_logits_dev is NULL");
  if (cells > 0 && !workspace) return fail(h, OP_ERR_INVALID, "op_forward_masked: workspace_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_forward_masked: NULL handle");
  report->status = 0;
  report->id_row = report->id_col = -1;
  report->id_value = 0;
  if (width > h->max_pos)
    return fail(h, OP_ERR_INVALID, "op_forward_masked: width %d exceeds max_position_embeddings %d", width, h->max_pos);
  if (!h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_forward_masked: the pass needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS");
  if (cells == 0) return OP_OK;
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(h, OP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  MaskedWorkspace ws;
  carve_masked(h, reinterpret_cast<char*>(workspace), n_rows, width, ws);
  if (workspace_bytes < ws.bytes) return fail(h, OP_ERR_WORKSPACE, "workspace has %zu bytes, need %zu", workspace_bytes, ws.bytes);

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(h, OP_ERR_STATE, "op_forward_masked: the stream is being captured (the call synchronises it to read the id check back)");

  // the dense cu_seqlens and the id check; its word comes back before the forward is enqueued: the embedding kernel only clamps
  OP_TRY(masked_id_check(h, "op_forward_masked", ids_dev, n_rows, width, ws.cu, ws.status, report, stream));

  std::vector<int32_t> cu_host((size_t)n_rows + 1);
  for (int r = 0; r <= n_rows; ++r) cu_host[(size_t)r] = r * width;
  PackedBatch b;
  b.ids_dev = ids_dev, b.cu_dev = ws.cu, b.cu_host = cu_host.data();
  b.n_seqs = n_rows, b.total_tokens = (int)cells, b.max_seqlen = width;
  b.prune_out = prune_out, b.rank_out = rank_out;
  b.workspace = ws.forward, b.workspace_bytes = ws.forward_bytes, b.stream = stream;
  MaskedReq msk;
  msk.key_ok = mask_dev;
  msk.vmean = ws.vmean;
  msk.cu_host = cu_host.data();
  return forward_packed_impl(h, b, nullptr, &msk);
}

}  // extern "C"
