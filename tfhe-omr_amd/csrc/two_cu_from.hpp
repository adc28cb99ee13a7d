// two_cu_from.hip's kernels, as cooperative-launch pointers for detect.hip (launch_br2xy). Arguments: the
// production kernel's (br2y_kernel / br2x_kernel), then const uint64_t *acc0 (device, canonical u64
// [n][2][N2]).
#pragma once

namespace omr {

const void *br2y_from_kernel_ptr();
const void *br2x_from_kernel_ptr();

}  // namespace omr
