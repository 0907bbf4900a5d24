// bmfr_fused_cols_f32_plane.hip -- the column-split K1 for f32 tmp_data
// reading the previous-frame pixel positions from the caller's plane
// (bmfr_frame_inputs.prev_pixel).
#define BMFR_COLS_F32 1
#define BMFR_COLS_PLANE 1
#include "bmfr_fused_cols.hip"
