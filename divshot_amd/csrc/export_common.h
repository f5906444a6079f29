// export_common.h — what the export and ingestion entry points (pack.hip, reduced.hip, knn.hip) share: one definition each.
#pragma once
#include <initializer_list>
#include "dvs_device.h"

static inline bool dvs_off16(const void* p) { return ((uintptr_t)p & 15u) != 0; }
// an entry point's argument check, true = refuse with DVS_ERR_INVALID before anything is launched: a required pointer is null or off a
// 16-byte boundary, an optional (nullable) one is off it, or the shN layout is not one of the two
static inline bool dvs_bad_args(std::initializer_list<const void*> required, std::initializer_list<const void*> optional = {},
                                int shn_layout = DVS_SHN_ROWS) {
    for (const void* p : required) if (!p || dvs_off16(p)) return true;
    for (const void* p : optional) if (dvs_off16(p)) return true;
    return shn_layout != DVS_SHN_ROWS && shn_layout != DVS_SHN_TILED;
}

// q = rot / |rot| of the repository's (w, x, y, z), as dvs_pack_compressed, dvs_pack_splat32 and the reduced format define it: the squares summed
// as ((w^2 + x^2) + y^2) + z^2 (dvs_pack_spz: w^2 last, see spz_rot), IEEE sqrt and divisions; a squared norm of 0 or not finite gives (1, 0, 0, 0)
__device__ __forceinline__ void dvs_unit_quat(const float4 r, float q[4]) {
    const float ss = ((r.x * r.x + r.y * r.y) + r.z * r.z) + r.w * r.w;
    if (!(ss > 0.0f) || !(ss < __builtin_inff())) { q[0] = 1.0f; q[1] = q[2] = q[3] = 0.0f; return; }
    const float len = dvs_sqrt_rn(ss);
    q[0] = r.x / len; q[1] = r.y / len; q[2] = r.z / len; q[3] = r.w / len;
}
