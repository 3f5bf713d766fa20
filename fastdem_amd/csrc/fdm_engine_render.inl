// fdm_engine_render.inl — host side of the layer -> RGBA image stage (kernels: fdm_render.hpp).
// Part of fdm_engine_post.hip (one of the library's five translation units, fdm_engine_host.hpp).

namespace {
int check_render(fdm_engine* e, const char* layer, const fdm_image_config* cfg, Layer** l) {
  if (cfg->normalize < 0 || cfg->normalize > 2) return fail(FDM_ERR_INVALID, "image config: normalize out of range");
  if (cfg->colormap < 0 || cfg->colormap > 2) return fail(FDM_ERR_INVALID, "image config: colormap out of range");
  if (int rc = resolve_pending(e)) return rc;
  *l = find_layer(e, layer);
  if (!*l || (*l)->pending) return fail(FDM_ERR_NO_LAYER, std::string("no layer ") + layer);
  return FDM_OK;
}
// Everything up to the finished image in e->d_image, enqueue-only.  `range_on_device`: the normalisation range is in
// e->d_render->range (every mode but FIXED_RANGE).
int enqueue_render(fdm_engine* e, const Layer* l, const fdm_image_config* cfg, bool* range_on_device) {
  if (e->ncell == 0 || e->ncell > (size_t(1) << 31)) return fail(FDM_ERR_INVALID, "map too large to render");
  if (int rc_grow = grow_device(e, &e->d_image, &e->image_cap, e->ncell, e->ncell)) return rc_grow;
  if (!e->d_render) HIPCK(hipMalloc(reinterpret_cast<void**>(&e->d_render), sizeof(RenderState)));
  const float* src = lptr(e, *l);
  const int stride = lstride(e, *l);
  const unsigned ncell = unsigned(e->ncell);
  RenderState* rs = e->d_render;
  *range_on_device = cfg->normalize != kNormFixed;
  if (*range_on_device) {
    // a block takes 256 cells per round: enough blocks to fill the chip several times over, few enough that the merge of
    // the block tables (at most 256 atomics each) stays small beside the pass
    const unsigned blocks = std::min(2048u, (ncell + 255u) / 256u);
    HIPCK(hipMemsetAsync(rs, 0, sizeof(RenderState), e->stream));
    hipLaunchKernelGGL(k_render_hist<0>, dim3(blocks), dim3(256), 0, e->stream, src, stride, ncell, rs);
    hipLaunchKernelGGL(k_render_pick<0>, dim3(1), dim3(256), 0, e->stream, rs, int(cfg->normalize));
    if (cfg->normalize == kNormPercentile) {
      hipLaunchKernelGGL(k_render_hist<1>, dim3(blocks), dim3(256), 0, e->stream, src, stride, ncell, rs);
      hipLaunchKernelGGL(k_render_pick<1>, dim3(1), dim3(256), 0, e->stream, rs, int(cfg->normalize));
      hipLaunchKernelGGL(k_render_hist<2>, dim3(blocks), dim3(256), 0, e->stream, src, stride, ncell, rs);
      hipLaunchKernelGGL(k_render_pick<2>, dim3(1), dim3(256), 0, e->stream, rs, int(cfg->normalize));
      hipLaunchKernelGGL(k_render_hist<3>, dim3(blocks), dim3(256), 0, e->stream, src, stride, ncell, rs);
      hipLaunchKernelGGL(k_render_pick<3>, dim3(1), dim3(256), 0, e->stream, rs, int(cfg->normalize));
    }
  }
  RenderParams Q{};
  Q.s_rows = e->G.s_rows; Q.s_cols = e->G.s_cols;
  Q.stride = stride;
  Q.slot = int(e->scan_no & 3);
  // (a tiled engine stores a window of the buffer and keeps start index 0: the window is the image)
  Q.use_start = cfg->align_to_world && e->G.s_rows == e->G.rows && e->G.s_cols == e->G.cols;
  Q.normalize = cfg->normalize; Q.colormap = cfg->colormap;
  Q.fixed_min = cfg->fixed_min; Q.fixed_max = cfg->fixed_max;
  const dim3 grid(unsigned((Q.s_cols + kRenderTile - 1) / kRenderTile), unsigned((Q.s_rows + kRenderTile - 1) / kRenderTile));
  hipLaunchKernelGGL(k_render_colour, grid, dim3(256), 0, e->stream, Q, src, e->d_state, rs, e->d_image);
  HIPCK(hipGetLastError());
  return FDM_OK;
}
}  // namespace

extern "C" {

void fdm_default_image_config(fdm_image_config* cfg) {  // PngExportConfig{} (io/png.hpp:29-38)
  if (!cfg) return;
  cfg->normalize = kNormPercentile;
  cfg->colormap = kMapViridis;
  cfg->align_to_world = 1;
  cfg->fixed_min = -2.0f;
  cfg->fixed_max = 2.0f;
}

int fdm_engine_render_layer_device(fdm_engine* e, const char* layer, const fdm_image_config* cfg, void** d_rgba,
                                   int32_t* width, int32_t* height, float range2[2]) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !layer || !cfg || !d_rgba) return fail(FDM_ERR_INVALID, "null argument");
  HIPCK(hipSetDevice(e->device));
  *d_rgba = nullptr;
  Layer* l = nullptr;
  if (int rc = check_render(e, layer, cfg, &l)) return rc;
  bool on_device = false;
  if (int rc = enqueue_render(e, l, cfg, &on_device)) return rc;
  if (width) *width = e->G.s_cols;
  if (height) *height = e->G.s_rows;
  *d_rgba = e->d_image;
  if (range2) {
    if (on_device) {
      HIPCK(hipMemcpyAsync(range2, e->d_render->range, 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
      if (int rc_sync = sync_all(e)) return rc_sync;
    } else {
      range2[0] = cfg->fixed_min; range2[1] = cfg->fixed_max;
    }
  }
  return FDM_OK;
}

int fdm_engine_render_layer(fdm_engine* e, const char* layer, const fdm_image_config* cfg, void* host_rgba,
                            uint64_t cap_bytes, int32_t* width, int32_t* height, float range2[2]) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !layer || !cfg) return fail(FDM_ERR_INVALID, "null argument");
  HIPCK(hipSetDevice(e->device));
  Layer* l = nullptr;
  if (int rc = check_render(e, layer, cfg, &l)) return rc;
  if (width) *width = e->G.s_cols;
  if (height) *height = e->G.s_rows;
  const uint64_t bytes = uint64_t(e->ncell) * 4u;
  if (!host_rgba || cap_bytes < bytes) return FDM_OK;  // the caller learns the size first: nothing is rendered
  bool on_device = false;
  if (int rc = enqueue_render(e, l, cfg, &on_device)) return rc;
  HIPCK(hipMemcpyAsync(host_rgba, e->d_image, bytes, hipMemcpyDeviceToHost, e->stream));
  float range[2] = {cfg->fixed_min, cfg->fixed_max};
  if (on_device && range2)
    HIPCK(hipMemcpyAsync(range, e->d_render->range, sizeof(range), hipMemcpyDeviceToHost, e->stream));
  if (int rc_sync = sync_all(e)) return rc_sync;
  if (range2) { range2[0] = range[0]; range2[1] = range[1]; }
  return FDM_OK;
}

}  // extern "C"
