// scene_xform.hpp -- moving a triangle: the arithmetic mirt_transform (csrc/scene_host.cpp) and mirt_scene_transform
// (scene_kernels.hip) share, so that a host mirror and the device scene hold the same bits.
//
// Each vertex becomes rot * v + translate: GLM's column-major mat3 * vec3 in its written order (type_mat3x3.inl: per row the three
// products, summed left to right -- mirt_math.hpp: mat3_mul_vec), then one add per component; no contraction (both translation
// units are built with -ffp-contract=off).  Draw() does the same to its ray direction.  The normal is recomputed as
// Triangle::ComputeNormal does after every change of the vertices (TestModel.h:26-31, :172-191; LoadSTL.cpp:78):
// normalize(cross(v2 - v0, v1 - v0)) -- a triangle with two equal vertices gets the NaN normal it gets there.  The colour stays.
#pragma once

#include "../csrc/mirt_math.hpp"

namespace mirt {

MIRT_HD void transform_tri(float *t15, const float *rot9, v3 tr)
{
    const v3 v0 = add3(mat3_mul_vec(rot9, ld3(t15)), tr);
    const v3 v1 = add3(mat3_mul_vec(rot9, ld3(t15 + 3)), tr);
    const v3 v2 = add3(mat3_mul_vec(rot9, ld3(t15 + 6)), tr);
    st3(t15, v0); st3(t15 + 3, v1); st3(t15 + 6, v2);
    st3(t15 + 9, normalize3(cross3(sub3(v2, v0), sub3(v1, v0))));
}

}  // namespace mirt
