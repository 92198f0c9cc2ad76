// Dispatches a batched call to the walk kernel instantiation for its mode and batch form, copy-emit to
// copy_kernel's launcher (csum_copy.hip) where the number has a COPY row (and, in the experiments build,
// instantiates the walk kernel's MODE_COPY forms: launch_walk<MODE_COPY, ...>).
#include "csum_walk.h"

namespace smolcsum {

// instantiated in csum_walk_{data,emit,verify}_{fixed,desc}.hip and csum_walk_nhc.hip
extern template hipError_t launch_walk<MODE_DATA, true>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk<MODE_DATA, false>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk<MODE_EMIT, true>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk<MODE_EMIT, false>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk<MODE_VERIFY, true>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk<MODE_VERIFY, false>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk_nhc<MODE_EMIT, true>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk_nhc<MODE_EMIT, false>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk_nhc<MODE_VERIFY, true>(int, int, const KParams&, uint32_t, hipStream_t);
extern template hipError_t launch_walk_nhc<MODE_VERIFY, false>(int, int, const KParams&, uint32_t, hipStream_t);

hipError_t launch_csum(int mode, int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s) {
    const bool implicit = p.desc == nullptr;
    if (p.addrs) {  // 6LoWPAN NHC UDP
        if (mode == MODE_EMIT)
            return implicit ? launch_walk_nhc<MODE_EMIT, true>(shape, var, p, max_blocks, s)
                            : launch_walk_nhc<MODE_EMIT, false>(shape, var, p, max_blocks, s);
        if (mode == MODE_VERIFY)
            return implicit ? launch_walk_nhc<MODE_VERIFY, true>(shape, var, p, max_blocks, s)
                            : launch_walk_nhc<MODE_VERIFY, false>(shape, var, p, max_blocks, s);
        return hipErrorInvalidValue;
    }
    switch (mode) {
        case MODE_DATA:
            return implicit ? launch_walk<MODE_DATA, true>(shape, var, p, max_blocks, s)
                            : launch_walk<MODE_DATA, false>(shape, var, p, max_blocks, s);
        case MODE_EMIT:
            return implicit ? launch_walk<MODE_EMIT, true>(shape, var, p, max_blocks, s)
                            : launch_walk<MODE_EMIT, false>(shape, var, p, max_blocks, s);
        case MODE_COPY: {
            // a COPY row's number (17 / 21 are the product's) runs copy_kernel; any other the walk kernel's
            // MODE_COPY form of it (the registry's V_WALK_COPY rows 1, 8, 11, 16: the round-1 / 2 designs,
            // in the experiments build only)
            const Variant* row = find_variant(var);
            if (row && row->family == F_COPY) return launch_copy_kernel(shape, var, p, max_blocks, s);
            return implicit ? launch_walk<MODE_COPY, true>(shape, var, p, max_blocks, s)
                            : launch_walk<MODE_COPY, false>(shape, var, p, max_blocks, s);
        }
        default:
            return implicit ? launch_walk<MODE_VERIFY, true>(shape, var, p, max_blocks, s)
                            : launch_walk<MODE_VERIFY, false>(shape, var, p, max_blocks, s);
    }
}

}  // namespace smolcsum
