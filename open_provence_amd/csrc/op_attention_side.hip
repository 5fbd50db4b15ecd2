// op_attention_side.hip -- C ABI: op_attention_probs / op_attention_rows, the side passes over one layer's input hidden state,
// and their workspace.  No kernel of its own: the row map comes from the forward unit (launch_side_row_map), the rest from the
// fp32 and attention-probability launch units.
#include "op_handle.h"

// ---- op_attention_probs: the softmax probabilities of one layer, a side pass over that layer's input hidden state ----------
struct AttnProbsWorkspace {
  int32_t *roff, *row_seq, *row_pos, *row_tok;
  float *x, *ln, *q, *k;
  size_t bytes;
};

// (the regions in the order they are first written: row maps, the gathered state, LayerNorm(attn_norm), q and k)
static void carve_attention(const op_handle* h, char* base, int cap_rows_pad, int n_seqs, AttnProbsWorkspace& ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up_sz(bytes, 256);
    return p;
  };
  const size_t R = (size_t)cap_rows_pad, plane = R * (size_t)h->H * sizeof(float);
  ws.roff = reinterpret_cast<int32_t*>(take(((size_t)n_seqs + 1) * 4));
  ws.row_seq = reinterpret_cast<int32_t*>(take(R * 4));
  ws.row_pos = reinterpret_cast<int32_t*>(take(R * 4));
  ws.row_tok = reinterpret_cast<int32_t*>(take(R * 4));
  ws.x = reinterpret_cast<float*>(take(plane));
  ws.ln = reinterpret_cast<float*>(take(plane));
  ws.q = reinterpret_cast<float*>(take(plane));
  ws.k = reinterpret_cast<float*>(take(plane));
  ws.bytes = off;
}

extern "C" size_t op_attention_workspace_bytes(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen) {
  if (!h || n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return 0;
  const int cap_pad = align_up(chunk_row_capacity(h, n_seqs, total_tokens, max_seqlen) + 64, 256);  // (as op_workspace_bytes)
  AttnProbsWorkspace ws;
  carve_attention(h, nullptr, cap_pad, n_seqs, ws);
  return ws.bytes;
}

// The part op_attention_probs and op_attention_rows share, after their own checks: workspace, chunks of sequences as the forward
// takes them, and per chunk the row map, the state's rows, LayerNorm(attn_norm), q | k with RoPE; `tail(ws, s0, ns, is_global)`
// then enqueues the call's own kernel over the chunk's q and k.
template <typename Tail>
static int attention_side_pass(op_handle* h, const char* what, const PackedBatch& b, int li, const float* hidden_dev, Tail&& tail) {
  if (!b.cu_dev || !b.workspace) return fail(h, OP_ERR_INVALID, "%s: NULL buffer", what);
  if ((reinterpret_cast<uintptr_t>(b.workspace) & 255) != 0) return fail(h, OP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  const size_t need = op_attention_workspace_bytes(h, b.n_seqs, b.total_tokens, b.max_seqlen);
  if (b.workspace_bytes < need) return fail(h, OP_ERR_WORKSPACE, "workspace has %zu bytes, need %zu", b.workspace_bytes, need);

  std::vector<int32_t> cu_copy;
  const int32_t* cu = nullptr;
  OP_TRY(host_cu_seqlens(h, b, cu_copy, &cu));

  const int H = h->H;
  const hipStream_t stream = b.stream;
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  const float* attn_norm = li != 0 ? h->layers[li].attn_norm : nullptr;  // layer 0: the identity, as in the forward
  const int cap = chunk_row_capacity(h, b.n_seqs, b.total_tokens, b.max_seqlen);
  AttnProbsWorkspace ws;
  carve_attention(h, reinterpret_cast<char*>(b.workspace), align_up(cap + 64, 256), b.n_seqs, ws);

  int s0 = 0;
  while (s0 < b.n_seqs) {  // chunks of sequences, as the forward takes them
    int rows = 0, max_len = 0;
    const int s1 = opp::next_chunk(cu, s0, b.n_seqs, cap, &rows, &max_len);
    if (rows > cap) return fail(h, OP_ERR_WORKSPACE, "internal: chunk of %d rows exceeds capacity %d", rows, cap);
    const int ns = s1 - s0;
    const int r_pad = align_up(std::max(rows, 1), GEMM_BM);
    // row map; the state's rows (zero rows where the map holds no token); LayerNorm; q | k with RoPE, q scaled
    launch_side_row_map(stream, b.cu_dev, s0, ns, r_pad, ws.roff, ws.row_seq, ws.row_pos, ws.row_tok);
    opl::launch_attn_probs_gather(stream, hidden_dev, ws.row_tok, H, r_pad, ws.x);
    if (attn_norm) opl::launch_f32_ln(stream, ws.x, attn_norm, h->cfg.norm_eps, H, r_pad, ws.ln);
    F32GemmParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.a = attn_norm ? ws.ln : ws.x;
    gp.w = reinterpret_cast<const float*>(h->layers[li].pack[W_QKV][PF_F32]);
    gp.K = H;
    gp.n_tiles = 2 * H / GEMM_BN;  // the q and k column tiles only
    gp.m_tiles = r_pad / GEMM_BM;
    gp.o0 = ws.q;
    gp.o1 = ws.k;
    gp.ld_out = H;
    gp.hidden = H;
    gp.inter = h->I;
    gp.row_pos = ws.row_pos;
    gp.rope_cos = h->rope_cos[is_global ? 1 : 0];
    gp.rope_sin = h->rope_sin[is_global ? 1 : 0];
    gp.max_pos = h->max_pos;
    if (!opl::launch_f32_gemm(stream, gp, F32_EPI_QKV)) return fail(h, OP_ERR_UNSUPPORTED, "internal: no fp32 GEMM epilogue %d", F32_EPI_QKV);
    tail(ws, s0, ns, is_global);
    OP_HIP(h, hipGetLastError());
    s0 = s1;
  }
  return OP_OK;
}

extern "C" {

int op_attention_probs(op_handle* h, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs, int total_tokens, int max_seqlen,
                       const op_attention_request* req, void* workspace, size_t workspace_bytes, void* hip_stream) {
  // (the request's own fields first: none of them needs the handle)
  if (!req) return fail(h, OP_ERR_INVALID, "op_attention_probs: the request is NULL");
  if (req->struct_bytes != sizeof(op_attention_request))
    return fail(h, OP_ERR_INVALID, "op_attention_probs: op_attention_request.struct_bytes is %u, expected %zu", req->struct_bytes,
                sizeof(op_attention_request));
  if (req->dtype != OP_HIDDEN_F32) return fail(h, OP_ERR_INVALID, "op_attention_probs: dtype %d is not OP_HIDDEN_F32", req->dtype);
  if (n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return fail(h, OP_ERR_INVALID, "op_attention_probs: negative size");
  const bool empty = n_seqs == 0 || total_tokens == 0;
  if (req->pad_width < 0 || req->pad_width < max_seqlen || (!empty && req->pad_width == 0))
    return fail(h, OP_ERR_INVALID, "op_attention_probs: pad_width %d below max_seqlen %d", req->pad_width, max_seqlen);
  if (!empty && !req->hidden_dev) return fail(h, OP_ERR_INVALID, "op_attention_probs: hidden_dev is NULL");
  if (!empty && !req->out_dev) return fail(h, OP_ERR_INVALID, "op_attention_probs: out_dev is NULL");
  if ((size_t)n_seqs * (size_t)req->pad_width > (size_t)INT32_MAX)  // (output rows are 32-bit indices inside a sequence's matrices)
    return fail(h, OP_ERR_INVALID, "op_attention_probs: %zu output rows per head exceed 2^31 - 1", (size_t)n_seqs * (size_t)req->pad_width);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_attention_probs: NULL handle");
  if (req->layer < 0 || req->layer >= h->N)
    return fail(h, OP_ERR_INVALID, "op_attention_probs: layer %d outside 0 .. %d", req->layer, h->N - 1);
  if (!h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_attention_probs: the pass needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS");
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  const int width = req->pad_width;
  const size_t mat_elems = (size_t)h->nh * (size_t)width * (size_t)width;  // one sequence
  float* out = reinterpret_cast<float*>(req->out_dev);
  if (n_seqs == 0 || width == 0) return OP_OK;
  if (total_tokens == 0) {  // only empty sequences: every row is padding
    OP_HIP(h, hipMemsetAsync(out, 0, (size_t)n_seqs * mat_elems * sizeof(float), stream));
    return OP_OK;
  }
  PackedBatch b;
  b.cu_dev = cu_dev, b.cu_host = cu_host_in, b.n_seqs = n_seqs, b.total_tokens = total_tokens, b.max_seqlen = max_seqlen;
  b.workspace = workspace, b.workspace_bytes = workspace_bytes, b.stream = stream;
  return attention_side_pass(h, "op_attention_probs", b, req->layer, req->hidden_dev,
                             [&](const AttnProbsWorkspace& ws, int s0, int ns, bool is_global) {
                               AttnProbsParams ap;
                               ap.q = ws.q;
                               ap.k = ws.k;
                               ap.out = out;
                               ap.cu = cu_dev;
                               ap.s0 = s0;
                               ap.roff = ws.roff;
                               ap.H = h->H;
                               ap.num_heads = h->nh;
                               ap.window = is_global ? -1 : h->cfg.local_attention / 2;
                               ap.width = width;
                               ap.wide = (width % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
                               opl::launch_attn_probs(stream, ap, ns);
                             });
}

// ---- op_attention_rows: one query row per sequence of op_attention_probs' matrices, per head or as the mean over heads --------
int op_attention_rows(op_handle* h, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs, int total_tokens, int max_seqlen,
                      const op_attention_rows_request* req, void* workspace, size_t workspace_bytes, void* hip_stream) {
  // (the request's own fields first: none of them needs the handle)
  if (!req) return fail(h, OP_ERR_INVALID, "op_attention_rows: the request is NULL");
  if (req->struct_bytes != sizeof(op_attention_rows_request))
    return fail(h, OP_ERR_INVALID, "op_attention_rows: op_attention_rows_request.struct_bytes is %u, expected %zu", req->struct_bytes,
                sizeof(op_attention_rows_request));
  if (req->reduce_heads != 0 && req->reduce_heads != 1)
    return fail(h, OP_ERR_INVALID, "op_attention_rows: reduce_heads %d is neither 0 nor 1", req->reduce_heads);
  if (n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return fail(h, OP_ERR_INVALID, "op_attention_rows: negative size");
  const bool empty = n_seqs == 0 || total_tokens == 0;
  if (req->pad_width < 0 || req->pad_width < max_seqlen || (!empty && req->pad_width == 0))
    return fail(h, OP_ERR_INVALID, "op_attention_rows: pad_width %d below max_seqlen %d", req->pad_width, max_seqlen);
  if (!empty && !req->hidden_dev) return fail(h, OP_ERR_INVALID, "op_attention_rows: hidden_dev is NULL");
  if (!empty && !req->out_dev) return fail(h, OP_ERR_INVALID, "op_attention_rows: out_dev is NULL");
  if (req->query_pos_host && !req->query_pos_dev)
    return fail(h, OP_ERR_INVALID, "op_attention_rows: query_pos_host without query_pos_dev");
  if (req->query_pos_host)
    for (int s = 0; s < n_seqs; ++s)
      if (req->query_pos_host[s] < 0)
        return fail(h, OP_ERR_INVALID, "op_attention_rows: query position %d of sequence %d is negative", req->query_pos_host[s], s);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_attention_rows: NULL handle");
  if (req->layer < 0 || req->layer >= h->N)
    return fail(h, OP_ERR_INVALID, "op_attention_rows: layer %d outside 0 .. %d", req->layer, h->N - 1);
  if (!h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_attention_rows: the pass needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS");
  const bool head_mean = req->reduce_heads != 0;
  if (head_mean && h->nh > AR_MAX_HEADS)
    return fail(h, OP_ERR_UNSUPPORTED, "op_attention_rows: reduce_heads with %d heads (at most %d)", h->nh, AR_MAX_HEADS);
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  const int width = req->pad_width;
  const size_t row_elems = (head_mean ? (size_t)1 : (size_t)h->nh) * (size_t)width;  // one sequence
  float* out = req->out_dev;
  if (n_seqs == 0 || width == 0) return OP_OK;
  if (total_tokens == 0) {  // only empty sequences: no position lies inside one
    OP_HIP(h, hipMemsetAsync(out, 0, (size_t)n_seqs * row_elems * sizeof(float), stream));
    return OP_OK;
  }
  PackedBatch b;
  b.cu_dev = cu_dev, b.cu_host = cu_host_in, b.n_seqs = n_seqs, b.total_tokens = total_tokens, b.max_seqlen = max_seqlen;
  b.workspace = workspace, b.workspace_bytes = workspace_bytes, b.stream = stream;
  return attention_side_pass(h, "op_attention_rows", b, req->layer, req->hidden_dev,
                             [&](const AttnProbsWorkspace& ws, int s0, int ns, bool is_global) {
                               AttnRowsParams ar;
                               ar.q = ws.q;
                               ar.k = ws.k;
                               ar.out = out;
                               ar.cu = cu_dev;
                               ar.qpos = req->query_pos_dev;
                               ar.s0 = s0;
                               ar.roff = ws.roff;
                               ar.H = h->H;
                               ar.num_heads = h->nh;
                               ar.window = is_global ? -1 : h->cfg.local_attention / 2;
                               ar.width = width;
                               opl::launch_attn_rows(stream, ar, ns, head_mean);
                             });
}

}  // extern "C"
