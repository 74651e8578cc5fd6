// gine_quad_wide_kernels.hip -- the GINE layer kernels of gine_quad_tile.h for the new shapes of width 16 / 32
// (GineShapesWide): what quad::gine_fwd / quad::gine_bwd (gine_quad_kernels.hip) try after the shipped shapes.
#include "gine_quad_tile.h"

CGVP_GINE_TABLE_ENTRY_POINTS(wide, GineShapesWide)
