// gine_quad_wide64_kernels.hip -- the GINE layer kernels of gine_quad_tile.h for the layers of hidden / output width 64
// behind 52, 32 or 64 input columns (GineShapesWide64): what quad::gine_fwd / quad::gine_bwd try last.
#include "gine_quad_tile.h"

CGVP_GINE_TABLE_ENTRY_POINTS(wide64, GineShapesWide64)
