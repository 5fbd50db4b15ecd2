// op_weights.hip -- C ABI: op_load_weight, and every packed form of a GEMM weight (WeightPacker).  The one unit that compiles
// the pack kernels of the kernel families (OPK_PACK_KERNELS) and the conversion / split / transpose / fit kernels (opk_load.hip.h).
#define OPK_PACK_KERNELS 1
#include "op_handle.h"
#include "opk_load.hip.h"

namespace {

void erase_missing(op_handle* h, const std::string& name) {
  auto it = std::find(h->missing.begin(), h->missing.end(), name);
  if (it != h->missing.end()) h->missing.erase(it);
}

// Every packed form of one GEMM weight tensor (op_load_weight), on the null stream: one method per packing kernel.
struct WeightPacker {
  op_handle* h;
  const WeightDesc& wd;
  const float* f32;  // the tensor as fp32 [d0][d1]
  int d0, d1;
  // A requested policy without the hi x lo(weight) term stores zeros in the lo plane (so that any kernel set gives
  // that policy's numerics); `any_lo` records whether the tensor had a non-zero lo element at all.
  int zero_lo;
  int* any_lo;

  size_t count() const { return (size_t)d0 * d1; }
  dim3 grid(size_t n) const { return dim3((unsigned)((n + 255) / 256)); }
  // the fp16 + e4m3 packs raise this flag (any_lo_dev[OP_FAM_COUNT]) for a weight they cannot hold exactly
  int* not_f16() const { return h->any_lo_dev + OP_FAM_COUNT; }

  // panel-major: [panel][k-step][plane][16 fragments][512], rows permuted per consumer (panel_source_row); f16: fp16 values
  void panels(u16* dst, int f16) const {
    int tile0 = 0;
    for (const PanelSeg& sg : wd.panel) {
      const int n_tiles = (sg.th * h->H + sg.ti * h->I) / 256;
      if (n_tiles)
        hipLaunchKernelGGL(pack_panel_kernel, grid((size_t)n_tiles * 256 * d1), dim3(256), 0, 0, f32, n_tiles, d1, sg.epi, h->H, h->I,
                           dst + (size_t)tile0 * 256 * d1 * 2, f16 ? 1 : zero_lo, any_lo, f16);
      tile0 += n_tiles;
    }
  }
  // the fp16 slabs + e4m3 slabs of the same panels
  void panels_f8(u16* dst16, u16* dst8) const {
    const size_t lo_off = count();  // bytes of the whole tensor's e4m3(w) slabs: the lo(w) slabs follow
    int tile0 = 0;
    for (const PanelSeg& sg : wd.panel) {
      const int n_tiles = (sg.th * h->H + sg.ti * h->I) / 256;
      if (n_tiles)
        hipLaunchKernelGGL(pack_panel_f8_kernel, grid((size_t)n_tiles * 256 * d1), dim3(256), 0, 0, f32, n_tiles, d1, sg.epi, h->H, h->I,
                           dst16 + (size_t)tile0 * 256 * d1, dst8 + (size_t)tile0 * 256 * d1 / 2, lo_off, zero_lo, not_f16(), h->f16_fit_dev);
      tile0 += n_tiles;
    }
  }
  // row path: chunk-major (pack_rowgemm_kernel) or k-streamed (pack_kstream_kernel); f16: fp16 values in the hi plane
  void rows(u16* dst, int f16) const {
    if (wd.row_mode == ROW_PACK_KSTREAM)
      hipLaunchKernelGGL(pack_kstream_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, 1, dst, f16 ? 1 : zero_lo, any_lo, f16);
    else
      hipLaunchKernelGGL(pack_rowgemm_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.row_mode, h->H, h->I, dst, f16 ? 1 : zero_lo,
                         any_lo, f16);
  }
  void rows_f8(u16* dst_a, u16* dst_b) const {
    if (wd.row_mode == ROW_PACK_KSTREAM)
      hipLaunchKernelGGL(pack_kstream_f8_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, 1, dst_a, dst_b, zero_lo, not_f16(), h->f16_fit_dev);
    else
      hipLaunchKernelGGL(pack_rowgemm_f8_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.row_mode, h->H, h->I, dst_a, zero_lo, not_f16(),
                         h->f16_fit_dev);
  }
  // after the one fp16 + e4m3 pack of the tensor: its energy, then the tensor's verdict (f16_unfit) from what the pack lost
  void close_f16_fit() const {
    hipLaunchKernelGGL(weight_energy_kernel, dim3(256), dim3(256), 0, 0, f32, count(), h->f16_fit_dev);
    hipLaunchKernelGGL(f16_fit_close_tensor_kernel, dim3(1), dim3(1), 0, 0, not_f16(), h->f16_fit_dev);
  }

  void run(u16* const* pk) const {  // pk[PF_COUNT]: the layer's packs of this weight
    if (pk[PF_HI])
      hipLaunchKernelGGL(split_planes_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.geglu ? h->I : 0, pk[PF_HI], pk[PF_LO], zero_lo,
                         any_lo);
    if (h->panel_path) {
      if (pk[PF_PANEL16]) {
        panels_f8(pk[PF_PANEL16], pk[PF_PANEL8]);
        close_f16_fit();
      }
      panels(pk[PF_PK], 0);
      if (pk[PF_PK16]) panels(pk[PF_PK16], 1);
    } else if (h->row_path) {
      rows(pk[PF_PK], 0);
      if (pk[PF_PK16]) rows(pk[PF_PK16], 1);
      if (pk[PF_ROW_F8A]) {
        rows_f8(pk[PF_ROW_F8A], pk[PF_ROW_F8B]);
        close_f16_fit();
      }
      if (pk[PF_L32])  // (hi plane; that kernel runs only when the lo planes are zero)
        hipLaunchKernelGGL(pack_layer32_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.l32_mode, wd.kmajor, h->H, h->I, pk[PF_L32]);
      for (PackFmt pf : {PF_PAIR, PF_PAIR16})
        if (pk[pf])
          hipLaunchKernelGGL(pack_layer16p_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.l32_mode, wd.kmajor, h->H, h->I, pk[pf],
                             pf == PF_PAIR16 ? 1 : 0);
    }
  }
};

}  // namespace

extern "C" {

int op_load_weight(op_handle* h, const char* name_c, const void* data, int dtype, const int64_t* shape, int ndim) {
  if (!h || !name_c || !data || !shape) return fail(h, OP_ERR_INVALID, "op_load_weight: NULL argument");
  if (dtype != OP_DTYPE_F32 && dtype != OP_DTYPE_BF16 && dtype != OP_DTYPE_F16)
    return fail(h, OP_ERR_INVALID, "op_load_weight(%s): unknown dtype %d", name_c, dtype);
  if (ndim < 1 || ndim > 2) return fail(h, OP_ERR_INVALID, "op_load_weight(%s): ndim %d not in {1,2}", name_c, ndim);
  std::string name(name_c);
  const std::string legacy_prefix = "ranking_model.";
  if (name.compare(0, legacy_prefix.size(), legacy_prefix) == 0) name = name.substr(legacy_prefix.size());
  const int64_t d0 = shape[0], d1 = ndim == 2 ? shape[1] : 1;
  const int H = h->H, I = h->I;

  bool transpose = false;
  float* dst_f32 = nullptr;
  const WeightDesc* wd = nullptr;  // a GEMM weight ...
  u16* const* packs = nullptr;     // ... and the layer's packs of it
  int64_t want0 = 0, want1 = 1;
  auto expect = [&](int64_t a, int64_t b) {
    want0 = a;
    want1 = b;
  };

  if (name == "model.embeddings.tok_embeddings.weight") {
    dst_f32 = h->emb; expect(h->V, H);
    h->cov_clear = true;  // (the audited ids were audited against the old table)
  } else if (name == "model.embeddings.norm.weight") {
    dst_f32 = h->emb_norm; expect(H, 1);
  } else if (name == "model.final_norm.weight") {
    dst_f32 = h->final_norm; expect(H, 1);
  } else if (name == "head.dense.weight") {
    dst_f32 = h->dense_t; transpose = true; expect(H, H);
  } else if (name == "head.norm.weight") {
    dst_f32 = h->head_norm; expect(H, 1);
  } else if (name == "classifier.weight") {
    dst_f32 = h->cls_w; expect(h->nl, H);
  } else if (name == "classifier.bias") {
    dst_f32 = h->cls_b; expect(h->nl, 1);
  } else if (name == "pruning_head.classifier.weight") {
    dst_f32 = h->prune_w; expect(2, H);
  } else if (name == "pruning_head.classifier.bias") {
    dst_f32 = h->prune_b; expect(2, 1);
  } else {
    int li = -1;
    char tail[64] = {0};
    if (sscanf(name.c_str(), "model.layers.%d.%63s", &li, tail) != 2 || li < 0 || li >= h->N)
      return fail(h, OP_ERR_INVALID, "op_load_weight: unknown tensor name '%s'", name_c);
    LayerWeights& lw = h->layers[li];
    const std::string t(tail);
    if (t == "attn_norm.weight" && li != 0) {
      dst_f32 = lw.attn_norm; expect(H, 1);
    } else if (t == "mlp_norm.weight") {
      dst_f32 = lw.mlp_norm; expect(H, 1);
    } else {
      for (int w = 0; w < W_COUNT; ++w)
        if (t == kWeights[w].tail) {
          wd = &kWeights[w];
          packs = lw.pack[w];
          expect((int64_t)weight_rows((Weight)w, H, I), (int64_t)weight_cols((Weight)w, H, I));
        }
      if (!wd) return fail(h, OP_ERR_INVALID, "op_load_weight: unknown tensor name '%s'", name_c);
    }
  }
  if (d0 != want0 || d1 != want1)
    return fail(h, OP_ERR_INVALID, "op_load_weight(%s): shape [%lld, %lld] but the model needs [%lld, %lld]", name_c,
                (long long)d0, (long long)d1, (long long)want0, (long long)want1);

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  const size_t count = (size_t)d0 * (size_t)d1;
  const size_t esz = dtype == OP_DTYPE_F32 ? 4 : 2;
  void* raw = nullptr;
  float* f32 = nullptr;
  OP_HIP(h, hipMalloc(&raw, count * esz));
  hipError_t e = hipMemcpy(raw, data, count * esz, hipMemcpyDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&f32, count * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(raw);
    return fail(h, OP_ERR_HIP, "op_load_weight(%s): staging failed: %s", name_c, hipGetErrorString(e));
  }
  const unsigned blocks = (unsigned)((count + 255) / 256);
  hipLaunchKernelGGL(convert_to_f32_kernel, dim3(blocks), dim3(256), 0, 0, raw, dtype, count, f32);
  if (wd) {
    const int req_mask[OP_FAM_COUNT] = {h->req.wqkv, h->req.qk, h->req.pv, h->req.attn_out, h->req.wi, h->req.mlp_out};
    h->resolved = false;
    // a kernel set pinned by op_select_kernel_set or measured by op_calibrate belongs to the weights it was chosen on: new
    // GEMM weights start from the default selection again (and from the compact formats, if op_set_compact_operands left them)
    h->forced_set = -1;
    h->forced_mlp_layers = ~0ull;
    h->f8_off = false;
    WeightPacker{h, *wd, f32, (int)d0, (int)d1, (req_mask[wd->family] & OP_TERM_RIGHT_LO) ? 0 : 1, h->any_lo_dev + wd->family}.run(packs);
    // kernel set "fp32": the tensor as it is
    if (packs[PF_F32]) e = hipMemcpyAsync(packs[PF_F32], f32, count * sizeof(float), hipMemcpyDeviceToDevice, 0);
  } else if (transpose) {
    hipLaunchKernelGGL(transpose_f32_kernel, dim3(blocks), dim3(256), 0, 0, f32, (int)d0, (int)d1, dst_f32);
  } else {
    e = hipMemcpyAsync(dst_f32, f32, count * sizeof(float), hipMemcpyDeviceToDevice, 0);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(0);
  (void)hipFree(raw);
  (void)hipFree(f32);
  if (e != hipSuccess) return fail(h, OP_ERR_HIP, "op_load_weight(%s): %s", name_c, hipGetErrorString(e));
  erase_missing(h, name);
  return OP_OK;
}

}  // extern "C"
