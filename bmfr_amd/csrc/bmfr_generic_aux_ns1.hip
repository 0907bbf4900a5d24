// bmfr_generic_aux_ns1.hip -- the generic-feature K1 of lists that name caller-supplied planes,
// FEATURES_NOT_SCALED = 1 (bmfr_generic.h).
#define BMFR_GENERIC_AUX_NS 1
#include "bmfr_generic.h"
