// bmfr_fused_plane.hip -- the row-split K1 (f32 tmp_data, exact fit) reading
// the previous-frame pixel positions from the caller's plane
// (bmfr_frame_inputs.prev_pixel) instead of projecting, compiled apart from
// the projecting kernels.
#define BMFR_ROWS_PLANE 1
#include "bmfr_fused.hip"
