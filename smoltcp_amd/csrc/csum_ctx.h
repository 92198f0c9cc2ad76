// The engine's context and what both ABI files (csum_api.cpp, csum_tools.cpp) need around it (internal).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/smolcsum.h"
#include "csum_dispatch.h"

namespace smolcsum {

// Grid cap meaning "one work item per group" (no persistent loop): on MI355X many small
// workgroups dispatched by the hardware beat a persistent grid (tools/sweep.py, C2: verify
// 0.244 ms vs 0.27 ms at 8 blocks per CU).
constexpr uint32_t kNaturalGrid = 0x7fffffffu;

// The context's entry buffer: the field entries and per-8-record flags of one chunk of kStageChunk records
// (as 16-B entries: kRouteChunk), allocated with the context (no allocation in a batched call).  It has two
// users, the staged descriptor emit and the fixed-stride route; a use on another stream than the previous
// one first waits for that one.
struct EntryBuffer {
    uint64_t* entries = nullptr;
    uint32_t* flags = nullptr;
    hipStream_t stream = nullptr;  // of the last use
    bool used = false;             // the entries have been used at all
    bool recorded = false;         // `done` was recorded after their last use
    hipEvent_t done = nullptr;

    // Before a use on stream s.  The staged descriptor emit records `done` after every call; the
    // fixed-stride route does not (a record per call sits between the emit and the next kernel of a
    // single-stream caller, the common case), so the event is recorded here, on the previous stream, when a
    // call on a different stream arrives: after everything that stream holds by now, the last use of the
    // entries included.  If that record fails (the stream is gone), the device is synchronised instead.
    hipError_t acquire(hipStream_t s) {
        if (!used || stream == s) return hipSuccess;
        if (!recorded) {
            if (hipEventRecord(done, stream) != hipSuccess) {
                (void)hipGetLastError();
                used = false;  // nothing is in flight after this
                return hipDeviceSynchronize();
            }
            recorded = true;
        }
        return hipStreamWaitEvent(s, done, 0);
    }
    // The use on stream s is the last one from here on; `recorded`: the caller recorded `done` after it.
    void release(hipStream_t s, bool was_recorded) {
        stream = s;
        used = true;
        recorded = was_recorded;
    }
};

}  // namespace smolcsum

struct smol_csum_ctx {
    int device = 0;
    int num_cu = 0;
    uint32_t max_blocks = smolcsum::kNaturalGrid;  // grid cap (kNaturalGrid: one work item per group)
    int shape = -1;               // -1 automatic, else CFG_*
    int variant = -1;             // kernel variant (-1 automatic; variants.def)
    uint8_t* dummy = nullptr;     // 256 zero bytes on the device (target of loads with nothing to read)
    int tile_records = 32;        // tile kernel: records per wavefront tile (32 or 64)
    bool max_blocks_set = false;  // grid cap given explicitly (tooling)
    int xcd_remap = -1;           // walk kernel: each XCD's blocks take a contiguous range of records
                                  // (-1: automatic, xcd_remap_auto; 0 / 1: forced, tooling)
    uint64_t launch_records = 0;  // records per kernel launch (0: the whole batch in one launch)
    smolcsum::EntryBuffer scratch;  // staged emit (the registry's V_STAGED variants) and the route below
    // the two-launch route of fixed-stride whole-segment emit (csum_api.cpp run_one): -1 automatic, 0 always
    // one launch, 1 the pair wherever it is legal (smol_csum_tool_set_emit_route); records per launch pair (at
    // most kRouteChunk, the entries the buffer holds); whether the last emit took the pair
    int emit_route = -1;
    uint64_t route_chunk = smolcsum::kRouteChunk;
    bool last_route = false;
    // descriptor-batch emit chooses between the staged form (kDwalkEmitStaged) and the in-place one
    // (kDwalkEmit) from the previous staged call's wavefront flags (a sample of the first kSample copied to
    // host memory): staged while at least half of the sampled wavefronts staged, else in place, probing with
    // the staged form again every kReprobe calls
    uint32_t* sample_host = nullptr;  // pinned
    hipEvent_t sample_ev = nullptr;
    bool sample_pending = false;
    int desc_staged = 1;              // 1: the staged form (also before any sample), 0: in place
    uint32_t since_probe = 0;
    int fields_kernel = smolcsum::FK_AUTO;  // emit_fields: FK_AUTO, or a forced form (smol_csum_tool_set_fields_kernel)
    bool vcopy_nt = false;            // verify_copy: non-temporal body stores (smol_csum_tool_set_vcopy_stores)
};

namespace smolcsum {

inline thread_local std::string g_last_error;  // smol_csum_last_error: one per thread, for both ABI files

inline int hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return SMOL_EHIP;
}

struct DeviceGuard {  // run on ctx->device, restore the caller's current device afterwards
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int now = -1;
        if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
    }
};

inline int check_batch(const smol_csum_batch_t* b, const void* d_buf) {
    if (!b) return SMOL_EINVAL;
    if (b->n == 0) return SMOL_OK;
    if (!d_buf) return SMOL_EINVAL;
    if ((b->flags & ~(SMOL_REC_IPHDR_ONLY | SMOL_BATCH_FIELD_STORES)) != 0 || b->reserved[0] != 0 ||
        b->reserved[1] != 0)
        return SMOL_EINVAL;
    if (b->desc) {
        if (((uintptr_t)b->desc & 15u) != 0) return SMOL_EINVAL;
    } else if (b->len > SMOL_MAX_RECORD_LEN) {
        return SMOL_ERANGE;
    }
    return SMOL_OK;
}

inline uint32_t cu_count(const smol_csum_ctx_t* ctx) { return (uint32_t)(ctx->num_cu > 0 ? ctx->num_cu : 256); }

// launch() on the context's device; `what` names it in the error message.
template <class F>
int on_device(const smol_csum_ctx_t* ctx, const char* what, F&& launch) {
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const hipError_t e = launch();
    return e == hipSuccess ? SMOL_OK : hip_fail(e, what);
}

}  // namespace smolcsum
