// op_api.hip -- C ABI of libopenprovence_hip.so (see include/open_provence_hip.h for the contract and
// the reference interfaces each entry point replaces): the handle's lifecycle and introspection -- create / destroy, errors,
// profiling, the debug hooks, the workspace's size and layout.  Host side only.  The other units of the C ABI (op_handle.h):
// op_weights.hip (weight loading and packing), op_select.hip (kernel-set selection, calibration), op_forward.hip +
// op_forward_layers.hip (the launch sequence of a forward), op_attention_side.hip, op_services.hip.
#include "op_handle.h"
#include "opk_clock_probe.hip.h"

namespace {

thread_local std::string g_last_error;

const char* kProfileNames[PK_COUNT] = {"rowmap",        "embed_ln",      "layer_norm",    "gemm_qk_rope", "gemm_v_t",
                                       "attn_global",   "attn_local",    "gemm_attn_out", "gemm_wi_geglu",
                                       "gemm_mlp_out",  "final_ln_prune", "rank_head",    "capture",
                                       "rowgemm_ln_qkv_rope", "rowgemm_attn_out", "rowgemm_ln_wi_geglu",
                                       "kstream_mlp_out", "fused_attnout_ln_wi_geglu", "fused_mlpout_ln_qkv_rope",
                                       "clear_lo_planes", "fused_layer_attnout_mlp_qkv", "gemm_qkv_rope"};

}  // namespace

namespace oph {

int fail(op_handle* h, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  g_last_error = buf;
  return code;
}

int fail(op_handle* h, const opp::Refusal& r) { return fail(h, r.code, "%s", r.text); }

// RoPE tables by HF's recipe (modeling_modernbert.py:117-163), reproduced to the bit in inv_freq: HF computes
// 1.0 / (theta ** (arange(0, 64, 2, fp32) / 64)) in fp32, which rounds TWICE -- an fp32 power, then an fp32 reciprocal.  The
// power is taken in double and rounded to fp32 (torch's fp32 pow agrees with the correctly rounded one on all 32 exponents at
// theta 10000 and 160000), then divided in fp32.  Rounding once, (float)(1.0 / pow(theta, e)), is one ulp off in 10 / 8 of the
// 32 entries at those thetas, and the angle's error grows with the position: 1.2e-4 in the table at position 8191.
// angle = fp32(pos) * inv_freq in fp32; cos / sin of that fp32 angle, correctly rounded (torch's cosf is within 6e-8 of it).
// tests/test_rope_tables.py holds the tables to torch's within 2^-23 through op_debug_rope_tables.
void build_rope_host(float theta, int max_pos, std::vector<float>& cs, std::vector<float>& sn) {
  cs.resize((size_t)max_pos * ROPE_HALF);
  sn.resize((size_t)max_pos * ROPE_HALF);
  float inv_freq[ROPE_HALF];
  for (int k = 0; k < ROPE_HALF; ++k) {
    const float expo = (float)(2 * k) / (float)HEAD_DIM;
    inv_freq[k] = 1.0f / (float)std::pow((double)theta, (double)expo);
  }
  for (int p = 0; p < max_pos; ++p) {
    for (int k = 0; k < ROPE_HALF; ++k) {
      const float ang = (float)p * inv_freq[k];
      cs[(size_t)p * ROPE_HALF + k] = (float)std::cos((double)ang);
      sn[(size_t)p * ROPE_HALF + k] = (float)std::sin((double)ang);
    }
  }
}

int drain_profile(op_handle* h) {
  for (auto& ev : h->events) {
    OP_HIP(h, hipEventSynchronize(ev.stop));
    float ms = 0.f;
    OP_HIP(h, hipEventElapsedTime(&ms, ev.start, ev.stop));
    h->prof_ms[ev.kind] += ms;
    h->prof_launches[ev.kind] += 1;
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
  }
  h->events.clear();
  return OP_OK;
}

}  // namespace oph

extern "C" {

int op_abi_version(void) { return OP_ABI_VERSION; }

const char* op_last_error(const op_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

const char* op_profile_kind_name(int kind) { return (kind >= 0 && kind < PK_COUNT) ? kProfileNames[kind] : "?"; }

int op_device_count(int* count) {
  if (!count) return fail(nullptr, OP_ERR_INVALID, "op_device_count: count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(nullptr, OP_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  }
  *count = n;
  return OP_OK;
}

int op_create(const op_config* cfg, op_handle** out) {
  if (!cfg || !out) return fail(nullptr, OP_ERR_INVALID, "op_create: NULL argument");
  *out = nullptr;
  if (cfg->struct_bytes != sizeof(op_config))
    return fail(nullptr, OP_ERR_INVALID, "op_create: op_config.struct_bytes=%u, library expects %zu (ABI mismatch)",
                cfg->struct_bytes, sizeof(op_config));
  const int H = cfg->hidden_size, I = cfg->intermediate_size, N = cfg->num_layers, nh = cfg->num_heads;
  if (H <= 0 || I <= 0 || N <= 0 || nh <= 0 || cfg->vocab_size <= 0 || cfg->num_labels <= 0)
    return fail(nullptr, OP_ERR_INVALID, "op_create: non-positive dimension");
  if (N > OP_MAX_LAYERS) return fail(nullptr, OP_ERR_UNSUPPORTED, "num_layers %d > %d", N, OP_MAX_LAYERS);
  if (H % nh != 0 || H / nh != HEAD_DIM)
    return fail(nullptr, OP_ERR_UNSUPPORTED, "head_dim must be 64 (hidden_size %d / num_heads %d)", H, nh);
  if (H % GEMM_BN != 0 || H > 1024)
    return fail(nullptr, OP_ERR_UNSUPPORTED, "hidden_size %d must be a multiple of 128 and <= 1024", H);
  if (I % 64 != 0) return fail(nullptr, OP_ERR_UNSUPPORTED, "intermediate_size %d must be a multiple of 64", I);
  if (cfg->num_labels > 64) return fail(nullptr, OP_ERR_UNSUPPORTED, "num_labels %d > 64", cfg->num_labels);
  Policy req;
  switch (cfg->precision) {
    case OP_PRECISION_BF16X3: req = opl::kPolicies[0]; break;
    case OP_PRECISION_BF16X2: req = opl::kPolicies[1]; break;
    case OP_PRECISION_BF16: req = opl::kPolicies[2]; break;
    case OP_PRECISION_CUSTOM:
      for (int f = 0; f < OP_FAM_COUNT; ++f)
        if (cfg->terms[f] > 3) return fail(nullptr, OP_ERR_INVALID, "terms[%d] = %d is not a term mask (0..3)", f, cfg->terms[f]);
      req = Policy{cfg->terms[OP_FAM_WQKV], cfg->terms[OP_FAM_QK], cfg->terms[OP_FAM_PV], cfg->terms[OP_FAM_ATTN_OUT],
                   cfg->terms[OP_FAM_WI], cfg->terms[OP_FAM_MLP_OUT]};
      break;
    default: return fail(nullptr, OP_ERR_INVALID, "unknown precision %d", cfg->precision);
  }
  if (cfg->pooling != OP_POOL_CLS && cfg->pooling != OP_POOL_MEAN)
    return fail(nullptr, OP_ERR_INVALID, "unknown pooling %d", cfg->pooling);
  if (cfg->local_attention < 0 || cfg->max_position_embeddings <= 0)
    return fail(nullptr, OP_ERR_INVALID, "bad local_attention / max_position_embeddings");

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, OP_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (cfg->device_id < 0 || cfg->device_id >= ndev)
    return fail(nullptr, OP_ERR_INVALID, "device_id %d out of range (count %d)", cfg->device_id, ndev);

  op_handle* h = new (std::nothrow) op_handle();
  if (!h) return fail(nullptr, OP_ERR_NOMEM, "out of host memory");
  h->cfg = *cfg;
  h->H = H;
  h->I = I;
  h->N = N;
  h->nh = nh;
  h->V = cfg->vocab_size;
  h->nl = cfg->num_labels;
  h->max_pos = cfg->max_position_embeddings;
  h->req = h->eff = req;
  h->chunk_rows = cfg->chunk_rows > 0 ? align_up(cfg->chunk_rows, ROW_ALIGN) : 262144;  // grids must cover the chip several times over
  h->layers.resize(N);
  // the dispatch path of this shape (opp::paths_of)
  const opp::Paths paths = opp::paths_of(H, I, (unsigned)cfg->flags);
  h->row_path = paths.row;
  h->panel_path = paths.panel;

#define OP_CREATE_TRY(expr)  \
  do {                       \
    int _rc = (expr);        \
    if (_rc != OP_OK) {      \
      g_last_error = h->err; \
      op_destroy(h);         \
      return _rc;            \
    }                        \
  } while (0)
#define OP_CREATE_HIP(expr)                                                                  \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      int _rc = fail(h, OP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));          \
      op_destroy(h);                                                                         \
      return _rc;                                                                            \
    }                                                                                        \
  } while (0)

  OP_CREATE_HIP(hipSetDevice(cfg->device_id));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device_id) == hipSuccess && prop.multiProcessorCount > 0)
      h->n_cus = prop.multiProcessorCount;
  }
  const size_t HH = (size_t)H * H;
  OP_CREATE_TRY(dev_alloc(h, &h->any_lo_dev, OP_FAM_COUNT + 3));  // + the fp16-fit flags of the "f16 + fp8" packs (note_f16_fit)
  OP_CREATE_HIP(hipMemset(h->any_lo_dev, 0, (OP_FAM_COUNT + 3) * sizeof(int)));
  OP_CREATE_TRY(dev_alloc(h, &h->f16_fit_dev, 2));
  OP_CREATE_HIP(hipMemset(h->f16_fit_dev, 0, 2 * sizeof(float)));
  // the weight packs this shape and these flags build (opp::packs_of)
  const opp::Packs packs = opp::packs_of(paths, H, (unsigned)cfg->flags);
  h->f8_packs = packs.f8;
  h->h16_packs = packs.h16;
  h->f32_packs = packs.f32;
  OP_CREATE_TRY(dev_alloc(h, &h->emb, (size_t)h->V * H));
  OP_CREATE_TRY(dev_alloc(h, &h->emb_norm, H));
  OP_CREATE_TRY(dev_alloc(h, &h->final_norm, H));
  OP_CREATE_TRY(dev_alloc(h, &h->dense_t, HH));
  OP_CREATE_TRY(dev_alloc(h, &h->head_norm, H));
  OP_CREATE_TRY(dev_alloc(h, &h->cls_w, (size_t)h->nl * H));
  OP_CREATE_TRY(dev_alloc(h, &h->cls_b, h->nl));
  OP_CREATE_TRY(dev_alloc(h, &h->prune_w, (size_t)2 * H));
  OP_CREATE_TRY(dev_alloc(h, &h->prune_b, 2));
  h->missing = {"model.embeddings.tok_embeddings.weight", "model.embeddings.norm.weight", "model.final_norm.weight",
                "head.dense.weight", "head.norm.weight", "classifier.weight", "classifier.bias",
                "pruning_head.classifier.weight", "pruning_head.classifier.bias"};
  for (int i = 0; i < N; ++i) {
    LayerWeights& lw = h->layers[i];
    const std::string pre = "model.layers." + std::to_string(i) + ".";
    if (i != 0) {
      OP_CREATE_TRY(dev_alloc(h, &lw.attn_norm, H));
      h->missing.push_back(pre + "attn_norm.weight");
    }
    OP_CREATE_TRY(dev_alloc(h, &lw.mlp_norm, H));
    // the GEMM weights in every format this handle's path and flags build (pack_exists); fp16 + e4m3: 4 bytes per weight element
    for (const AllocStep& step : kAllocOrder)
      for (Weight w : step.order)
        for (int f = 0; f < step.n_fmt; ++f) {
          const PackFmt pf = step.fmt[f];
          if (kPackElems[w][pf] && pack_exists(pf, h->row_path, h->panel_path, h->f8_packs, h->h16_packs, h->f32_packs, H))
            OP_CREATE_TRY(dev_alloc(h, &lw.pack[w][pf], weight_elems(w, H, I) * kPackElems[w][pf]));
        }
    h->missing.push_back(pre + "mlp_norm.weight");
    for (const WeightDesc& wd : kWeights) h->missing.push_back(pre + wd.tail);
  }
  OP_CREATE_TRY(dev_alloc(h, &h->cov_bits, ((size_t)h->V + 31) / 32));
  OP_CREATE_TRY(dev_alloc(h, &h->cov_state, (size_t)opl::COV_WORDS));
  OP_CREATE_TRY(dev_alloc(h, &h->loss_scratch, 1));  // (here, not on first use: op_loss without a report may be captured)
  for (int t = 0; t < 2; ++t) {
    std::vector<float> cs, sn;
    build_rope_host(t == 1 ? cfg->global_rope_theta : cfg->local_rope_theta, h->max_pos, cs, sn);
    OP_CREATE_TRY(dev_alloc(h, &h->rope_cos[t], cs.size()));
    OP_CREATE_TRY(dev_alloc(h, &h->rope_sin[t], sn.size()));
    OP_CREATE_HIP(hipMemcpy(h->rope_cos[t], cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    OP_CREATE_HIP(hipMemcpy(h->rope_sin[t], sn.data(), sn.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  *out = h;
  return OP_OK;
}

void op_destroy(op_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device_id);
  for (auto& ev : h->events) {
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
  }
  for (void* p : h->allocations) (void)hipFree(p);
  if (h->pad_host) (void)hipHostFree(h->pad_host);
  if (h->cov_host) (void)hipHostFree(h->cov_host);
  if (h->loss_host) (void)hipHostFree(h->loss_host);
  delete h;
}

size_t op_workspace_bytes(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen) {
  if (!h || n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return 0;
  return forward_layout(h, n_seqs, total_tokens, max_seqlen, h->set == OP_KS_F32).bytes;
}

int op_debug_workspace_layout(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen, op_workspace_region* entries,
                              int max_entries) {
  if (!h || n_seqs < 0 || total_tokens < 0 || max_seqlen < 0 || max_entries < 0 || (!entries && max_entries > 0)) return OP_ERR_INVALID;
  const opp::Layout lay = forward_layout(h, n_seqs, total_tokens, max_seqlen, h->set == OP_KS_F32);  // (as op_workspace_bytes)
  for (int i = 0; i < lay.n && i < max_entries; ++i)
    entries[i] = op_workspace_region{lay.regions[i].name, (uint64_t)lay.regions[i].offset, (uint64_t)lay.regions[i].bytes, (int32_t)lay.regions[i].kind};
  return lay.n;
}

int op_debug_rope_tables(const op_handle* h, int global_table, float theta, int max_pos, float* cos_host, float* sin_host) {
  if (max_pos <= 0 || !cos_host || !sin_host) return OP_ERR_INVALID;
  const size_t count = (size_t)max_pos * ROPE_HALF;
  if (!h) {  // no handle, no device: the tables op_create would build for this theta
    if (!(theta > 0.f)) return OP_ERR_INVALID;
    std::vector<float> cs, sn;
    build_rope_host(theta, max_pos, cs, sn);
    std::copy(cs.begin(), cs.end(), cos_host);
    std::copy(sn.begin(), sn.end(), sin_host);
    return OP_OK;
  }
  const int t = global_table ? 1 : 0;
  if (max_pos != h->max_pos || !h->rope_cos[t] || !h->rope_sin[t]) return OP_ERR_INVALID;
  if (hipSetDevice(h->cfg.device_id) != hipSuccess) return OP_ERR_HIP;
  if (hipMemcpy(cos_host, h->rope_cos[t], count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return OP_ERR_HIP;
  if (hipMemcpy(sin_host, h->rope_sin[t], count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return OP_ERR_HIP;
  return OP_OK;
}

int op_debug_primitive(op_handle* h, int kind, int mode, const void* in_dev, size_t n, void* out_dev, void* hip_stream) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_debug_primitive: NULL handle");
  const int group = opl::probe_group_size(kind);
  if (group == 0 || (mode != 0 && mode != 1)) return fail(h, OP_ERR_INVALID, "op_debug_primitive: unknown kind %d or mode %d", kind, mode);
  if (n % (size_t)group != 0) return fail(h, OP_ERR_INVALID, "op_debug_primitive: n = %zu is not a multiple of kind %d's group of %d", n, kind, group);
  if (n > ((size_t)1 << 31)) return fail(h, OP_ERR_INVALID, "op_debug_primitive: n = %zu is beyond 2^31 elements", n);
  if (n == 0) return OP_OK;
  if (!in_dev || !out_dev) return fail(h, OP_ERR_INVALID, "op_debug_primitive: NULL buffer");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_probe((hipStream_t)hip_stream, kind, mode, in_dev, n, out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_debug_capture_hidden(op_handle* h, float* hidden_dev) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_debug_capture_hidden: NULL handle");
  h->capture = hidden_dev;
  return OP_OK;
}

int op_profile_enable(op_handle* h, int enabled) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_profile_enable: NULL handle");
  h->profiling = enabled != 0;
  return OP_OK;
}

int op_debug_clock_probe(op_handle* h, int spin_us, unsigned long long* out_dev, void* hip_stream) {
  if (!h || !out_dev || spin_us <= 0) return fail(h, OP_ERR_INVALID, "op_debug_clock_probe: bad argument");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (unsigned long long)spin_us * 100ull, out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_profile_reset(op_handle* h) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_profile_reset: NULL handle");
  int rc = drain_profile(h);
  for (int k = 0; k < PK_COUNT; ++k) {
    h->prof_ms[k] = 0;
    h->prof_launches[k] = 0;
  }
  return rc;
}

int op_profile_read(op_handle* h, op_profile_entry* entries, int max_entries) {
  if (!h || (!entries && max_entries > 0)) return fail(h, OP_ERR_INVALID, "op_profile_read: NULL argument");
  int rc = drain_profile(h);
  if (rc != OP_OK) return rc;
  int n = 0;
  for (int k = 0; k < PK_COUNT && n < max_entries; ++k) {
    if (h->prof_launches[k] == 0) continue;
    entries[n].kind = k;
    entries[n].launches = h->prof_launches[k];
    entries[n].total_ms = h->prof_ms[k];
    ++n;
  }
  return n;
}

}  // extern "C"
