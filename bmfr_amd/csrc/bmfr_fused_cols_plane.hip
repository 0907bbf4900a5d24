// bmfr_fused_cols_plane.hip -- the column-split K1 (half tmp_data) reading the
// previous-frame pixel positions from the caller's plane
// (bmfr_frame_inputs.prev_pixel) instead of projecting, compiled apart from
// the projecting kernels.
#define BMFR_COLS_PLANE 1
#include "bmfr_fused_cols.hip"
