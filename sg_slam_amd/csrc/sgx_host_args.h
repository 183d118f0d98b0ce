// sgx_host_args.h — host only: C-ABI values (include/sgx.h) as the by-value kernel argument structs (sgx_types.h)
#pragma once
#include "sgx_types.h"
#include "../../include/sgx.h"
#include <string.h>

static inline SgxCam to_cam(const sgx_camera *c) { SgxCam k; k.fx = c->fx; k.fy = c->fy; k.cx = c->cx; k.cy = c->cy; k.bf = c->bf; k.minX = c->min_x; k.maxX = c->max_x; k.minY = c->min_y; k.maxY = c->max_y; return k; }

// a per-level table (scale factors, sigma^2, ...) of nlevels <= 12 entries, zero-padded
static inline SgxScales to_scales(const float *table, int nlevels)
{
    SgxScales s; memset(&s, 0, sizeof s);
    for (int i = 0; i < nlevels; i++) s.s[i] = table[i];
    return s;
}
