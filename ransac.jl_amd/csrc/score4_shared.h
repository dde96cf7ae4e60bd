// score4_shared.h -- what two or more units of the v4 score path need: score4.hip (the kernel and its launch), boxes32.hip (the
// binary32 twins of an ordering, once per cloud), unpermute4.hip (the mask lists -> subset order) and score4_diag.hip (the diag
// build's audits and probes).  What only the kernel uses stays in score4.hip.
#pragma once

#include "rh_internal.h"
#include "score4_device.h"

namespace {

typedef float rh_f32x4 __attribute__((ext_vector_type(4)));
typedef float rh_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long rh_u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t rh_u32x4 __attribute__((ext_vector_type(4)));

// the groupings (rh_internal.h holds their one statement and what ties them to the k-d tree's nodes)
constexpr int S4_TG = RH_G2_TG;          // groups per tile (8, measured in round 4 -- the per-chunk work of stage 1 paid once per 8 box tests,
                                         // fuller batches: cfg3 0.0906 -> 0.0959 ms, cfg2 0.078 -> 0.104, cfg5 0.384 -> 0.375; R = 4 with it: worse still)
constexpr int S4_STG = RH_S4_STG;        // groups per super-tile (st_cull_kernel): 4 tiles = 1024 points of the k-d leaf order

static __device__ __forceinline__ bool is_nan_bits(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7fffffffu) > 0x7f800000u;
}

template <int KIND> struct S4Fields { static constexpr int NBOX = KIND == RH_PLANE ? 8 : (KIND == RH_SPHERE ? 5 : (KIND == RH_CYLINDER ? 10 : 11)); };

// may a plane candidate (fields 5-7 of its culling record: the cells its inliers' normals can lie in) meet a group / super-tile
// whose points' normals lie in the cells of gm?  (score4_device.h, normal cells)
static __device__ __forceinline__ bool nsig_meet(const float (&B)[rh4::RH_BOX_FIELDS], const rh_u32x4 gm)
{
    return (((__builtin_bit_cast(uint32_t, B[5]) & gm.x) | (__builtin_bit_cast(uint32_t, B[6]) & gm.y)) | (__builtin_bit_cast(uint32_t, B[7]) & gm.z)) != 0u;
}

inline int cdiv4(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace
