// Instantiates emit_fields' walk form (csum_walk.h: csum_kernel with the form WFields) for fixed-stride batches.
#include "csum_walk.h"

namespace smolcsum {
template hipError_t launch_walk_fields<true>(int, const KParams&, uint32_t, hipStream_t);
}  // namespace smolcsum
