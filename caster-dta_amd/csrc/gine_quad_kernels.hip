// gine_quad_kernels.hip -- the GINE layer kernels of gine_quad_tile.h for the layer shapes of the shipped models
// (GineShapesShipped), and quad::gine_fwd / quad::gine_bwd: this table first, then the two of the wider shapes
// (gine_quad_wide_kernels.hip, gine_quad_wide64_kernels.hip).
#include "gine_quad_tile.h"

namespace quad {

int gine_bwd(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
             const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
             const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
             const float* mask, gvp::RngArgs rng, const float* g_out, float* g_x, float* slab, int max_workgroups,
             int* rows, int* row_len, hipStream_t st, const float* agg_in, const uint16_t* pos_in,
             float* g_edge, float* g_self, float* g_eattr, int eattr_accum) {
  GineQArgs a = gine_bwd_args(x, ntypes, eattr, etypes, rowptr, eperm, esrc, edst, N, w, slope, mask, rng, g_out, g_x, slab,
                              agg_in, pos_in, g_edge, g_self, g_eattr, eattr_accum);
  const int rc = gine_bwd_in<GineShapesShipped>(cin, chid, cout, nt, net, ed, a, max_workgroups, rows, row_len, st);
  if (rc != CGVP_ERR_UNSUPPORTED_DIMS) return rc;
  for (auto* next : {gine_bwd_wide, gine_bwd_wide64}) {
    const int r = next(cin, chid, cout, nt, net, ed, x, ntypes, eattr, etypes, rowptr, eperm, esrc, edst, N, w, slope, mask,
                       rng, g_out, g_x, slab, max_workgroups, rows, row_len, st, agg_in, pos_in, g_edge, g_self, g_eattr,
                       eattr_accum);
    if (r != CGVP_ERR_UNSUPPORTED_DIMS) return r;
  }
  return CGVP_ERR_UNSUPPORTED_DIMS;
}

// Forward on tiles for the compiled layer shapes; returns 1 when the shape is not compiled (the fine-grained
// cgvp_gine_conv_fwd then uses the generic one-wave-per-atom kernel; the whole passes refuse the configuration).
int gine_fwd(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
             const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
             const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
             const float* mask, gvp::RngArgs rng, float* out, float* agg_out, uint16_t* pos_out, hipStream_t st) {
  GineFArgs a{x, ntypes, eattr, etypes, rowptr, eperm, esrc, edst, N, w->eps, w->we, w->be, w->w0, w->b0,
              w->w1, w->b1, slope, mask, rng, out, agg_out, pos_out};
  const int rc = gine_fwd_in<GineShapesShipped>(cin, chid, cout, nt, net, ed, a, st);
  if (rc != 1) return rc;
  for (auto* next : {gine_fwd_wide, gine_fwd_wide64}) {
    const int r = next(cin, chid, cout, nt, net, ed, x, ntypes, eattr, etypes, rowptr, eperm, esrc, edst, N, w, slope, mask,
                       rng, out, agg_out, pos_out, st);
    if (r != 1) return r;
  }
  return 1;
}

bool gine_shape_compiled(int cin, int chid, int cout, int nt, int net, int ed) {
  const auto yes = [](auto) { return 1; };
  return for_gine_shape(GineShapesShipped{}, cin, chid, cout, nt, net, ed, 0, yes) ||
         for_gine_shape(GineShapesWide{}, cin, chid, cout, nt, net, ed, 0, yes) ||
         for_gine_shape(GineShapesWide64{}, cin, chid, cout, nt, net, ed, 0, yes);
}

// slab row of the largest compiled layer (cgvp_gine_bwd_workspace_floats)
int gine_max_slab_row() {
  constexpr int a = gine_max_layer_floats(GineShapesShipped{}), b = gine_max_layer_floats(GineShapesWide{}),
                c = gine_max_layer_floats(GineShapesWide64{});
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

}  // namespace quad

#ifdef CGVP_STAMPS
extern "C" int cgvp_debug_set_stamp_buffer_gine(unsigned long long* buf) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf_gine), &buf, sizeof(buf));
}
#endif
