// Dispatches a batched call to the walk kernel instantiation for its mode and batch form (and, in the
// experiments build, instantiates the walk kernel's MODE_COPY forms: launch_walk<MODE_COPY, ...>).
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

// variant 17: the class-split copy-emit kernel (csum_copy.hip)
hipError_t launch_copy_v17(int shape, const KParams& p, uint32_t max_blocks, hipStream_t s);
// variant 21: variant 17 with the first body round's loads ahead of round 1's stores (csum_copy.hip)
hipError_t launch_copy_v21(int shape, const KParams& p, uint32_t max_blocks, hipStream_t s);
#ifdef SMOL_EXP
// variants 30 / 22: 21 with non-temporal body stores / and source loads (csum_copy.hip)
hipError_t launch_copy_nt(int var, const KParams& p, uint32_t max_blocks, hipStream_t s);
#endif

// 17 / 21 (copy_kernel) are the product's; the walk kernel's MODE_COPY forms (the registry's V_WALK_COPY
// rows 1, 8, 11, 16: the round-1 / 2 designs) are in the experiments build only.
template <bool IMPLICIT>
hipError_t launch_copy(int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s) {
    switch (var) {
        case 17: return launch_copy_v17(shape, p, max_blocks, s);
        case 21: return launch_copy_v21(shape, p, max_blocks, s);
#ifdef SMOL_EXP
        case 30:
        case 98:
        case 102:
        case 22: return launch_copy_nt(var, p, max_blocks, s);
#endif
        default: return launch_walk<MODE_COPY, IMPLICIT>(shape, var, p, max_blocks, s);
    }
}

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
        case MODE_COPY:
            return implicit ? launch_copy<true>(shape, var, p, max_blocks, s) : launch_copy<false>(shape, var, p, max_blocks, s);
        default:
            return implicit ? launch_walk<MODE_VERIFY, true>(shape, var, p, max_blocks, s)
                            : launch_walk<MODE_VERIFY, false>(shape, var, p, max_blocks, s);
    }
}

}  // namespace smolcsum
