// x0_predict.h - the predicted clean image of one element, x0 = fl(fl(cx*x) - fl(ce*eps)), and the row of the coefficient table a batch row
// reads (LatentDiffusion.x0_threshold_table: cx, ce, kx, k0 per time-step value).  ONE body for pf_x0_threshold (x0_threshold.hip), which
// bounds this x0, and pf_x0_predict (steer.hip), which writes it out for the steering reward: the two cannot drift apart.
#pragma once
#include "noise.h"

namespace pf {

// table row of batch row `row`: t[row * t_stride] clamped into [0, n_table - 1], four floats per row
__device__ __forceinline__ const float* x0_table_row(const int64_t* t, int32_t t_stride, const float* table, int32_t n_table, unsigned row) {
  int64_t tv = t[(size_t)row * t_stride];
  tv = tv < 0 ? 0 : (tv > n_table - 1 ? n_table - 1 : tv);
  return table + 4 * tv;
}
// every operation individually rounded (noise.h): the same bits in every kernel that inlines it, whatever the width of its accesses
__device__ __forceinline__ float x0_of(float cx, float ce, float x, float e) { return sub_rn(mul_rn(cx, x), mul_rn(ce, e)); }

}  // namespace pf
