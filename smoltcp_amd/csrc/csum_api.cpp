// C ABI of the checksum engine: scalar host mirrors of smoltcp::wire::checksum and the batched
// device entry points (include/smolcsum.h), plus the tooling entry points
// (include/smolcsum_tools.h).  No exception crosses this boundary; every batched call either
// launches HIP kernels or returns an error — there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "../../include/smolcsum.h"
#include "../../include/smolcsum_tools.h"
#include "csum_dispatch.h"

using namespace smolcsum;

struct smol_csum_ctx {
    int device;
    int num_cu;
    uint32_t max_blocks;  // grid cap (kNaturalGrid: one work item per group)
    int shape;            // -1 automatic, else CFG_*
    int variant;          // kernel variant (-1 automatic; variants.def)
    uint8_t* dummy;       // 256 zero bytes on the device (target of loads with nothing to read)
    int tile_records;     // tile kernel: records per wavefront tile (32 or 64)
    bool max_blocks_set;  // grid cap given explicitly (tooling)
    int xcd_remap;        // walk kernel: each XCD's blocks take a contiguous range of records
                          // (-1: automatic, xcd_remap_auto; 0 / 1: forced, tooling)
    uint64_t launch_records;  // records per kernel launch (0: the whole batch in one launch)
    // staged emit (the registry's V_STAGED variants): the field entries and per-8-record flags of one
    // chunk of kStageChunk records, allocated with the context (no allocation in a batched call);
    // stage_stream / stage_done order a use of the entries on another stream after the previous one
    // (order_scratch below): stage_used says the entries have been used at all, stage_recorded that
    // stage_done was recorded after their last use
    uint64_t* stage;
    uint32_t* stage_flags;
    void* stage_stream;
    bool stage_used;
    bool stage_recorded;
    hipEvent_t stage_done;
    // the two-launch route of fixed-stride whole-segment emit (run()): -1 automatic, 0 always one launch,
    // 1 the pair wherever it is legal (smol_csum_tool_set_emit_route); records per launch pair (at most
    // kRouteChunk, the entries the buffer holds); whether the last emit took the pair
    int emit_route;
    uint64_t route_chunk;
    bool last_route;
    // descriptor-batch emit chooses between the staged form (kDwalkEmitStaged) and the in-place one
    // (kDwalkEmit) from the
    // previous staged call's wavefront flags (a sample of the first kSample copied to host memory):
    // staged while at least half of the sampled wavefronts staged, else in place, probing with the
    // staged form again every kReprobe calls
    uint32_t* sample_host;    // pinned
    hipEvent_t sample_ev;
    bool sample_pending;
    int desc_staged;          // 1: the staged form (also before any sample), 0: in place
    uint32_t since_probe;
    int fields_kernel;        // emit_fields: FK_AUTO, or a forced form (smol_csum_tool_set_fields_kernel)
    bool vcopy_nt;            // verify_copy: non-temporal body stores (smol_csum_tool_set_vcopy_stores)
};

namespace {
constexpr uint32_t kSample = 256;   // wavefront flags (8 records each) sampled per staged call
constexpr uint32_t kReprobe = 64;   // in-place calls between two staged probes
}

namespace smolcsum {

uint32_t resident_blocks(const void* kernel, uint32_t num_cu, uint32_t max_blocks) {
    if (num_cu == 0) return max_blocks;  // explicit grid cap (smol_csum_tool_set_max_blocks)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1)
        per_cu = 1;
    const uint64_t cap = (uint64_t)per_cu * num_cu;
    return (uint32_t)(cap < max_blocks ? cap : max_blocks);
}

}  // namespace smolcsum

namespace {

thread_local std::string g_last_error;

int hip_fail(hipError_t e, const char* what) {
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

bool caps_valid(const smol_checksum_caps_t* c) {
    if (!c) return false;
    const uint8_t v[5] = {c->ipv4, c->udp, c->tcp, c->icmpv4, c->icmpv6};
    for (uint8_t x : v)
        if (x > SMOL_CHECKSUM_NONE) return false;
    return c->reserved[0] == 0 && c->reserved[1] == 0 && c->reserved[2] == 0;
}

// Grid cap meaning "one work item per group" (no persistent loop): on MI355X many small
// workgroups dispatched by the hardware beat a persistent grid (tools/sweep.py, C2: verify
// 0.244 ms vs 0.27 ms at 8 blocks per CU).
constexpr uint32_t kNaturalGrid = 0x7fffffffu;

int check_batch(const smol_csum_batch_t* b, const void* d_buf) {
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

// What a batched call with caps checks first, in this order: the context and the caps, then the batch.
// False: the call ends here with *rc (an error, or SMOL_OK for an empty batch).
bool begin_call(const smol_csum_ctx_t* ctx, const smol_checksum_caps_t* caps, const smol_csum_batch_t* b,
                const void* d_buf, int* rc) {
    *rc = !ctx || !caps_valid(caps) ? SMOL_EINVAL : check_batch(b, d_buf);
    return *rc == SMOL_OK && b->n != 0;
}

// The same for a call over fragment groups: no groups is SMOL_OK whatever the batch holds, groups over an
// empty batch are an error.
bool begin_group_call(const smol_csum_ctx_t* ctx, const smol_checksum_caps_t* caps, const smol_csum_batch_t* b,
                      const void* d_buf, const smol_csum_frag_group_t* d_groups, uint64_t n_groups, int* rc) {
    *rc = !ctx || !caps_valid(caps) ? SMOL_EINVAL : check_batch(b, d_buf);
    if (*rc != SMOL_OK || n_groups == 0) return false;
    if (b->n == 0 || !d_groups || ((uintptr_t)d_groups & 15u) != 0) *rc = SMOL_EINVAL;
    return *rc == SMOL_OK;
}

uint32_t cu_count(const smol_csum_ctx_t* ctx) { return (uint32_t)(ctx->num_cu > 0 ? ctx->num_cu : 256); }

// Zeroed launch parameters with what every batched call takes from its arguments: the batch form, the
// record kind, the caps (none: smol_csum_batch_data) and the dummy line.
KParams base_params(const smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                    const smol_checksum_caps_t* caps) {
    KParams p;
    std::memset(&p, 0, sizeof p);
    p.buf = const_cast<uint8_t*>(d_buf);  // (only emit and copy_emit store there)
    p.desc = b->desc;
    p.n = b->n;
    p.stride = b->stride;
    p.len = b->len;
    p.kind = b->kind | ((b->flags & SMOL_REC_IPHDR_ONLY) ? KIND_IPHDR_ONLY : 0u);
    if (caps) {
        p.caps_ipv4 = caps->ipv4;
        p.caps_udp = caps->udp;
        p.caps_tcp = caps->tcp;
        p.caps_icmpv4 = caps->icmpv4;
        p.caps_icmpv6 = caps->icmpv6;
    }
    p.dummy = ctx->dummy;
    return p;
}

// launch() on the context's device; `what` names it in the error message.
template <class F>
int on_device(const smol_csum_ctx_t* ctx, const char* what, F&& launch) {
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const hipError_t e = launch();
    return e == hipSuccess ? SMOL_OK : hip_fail(e, what);
}

// launch_records: a batch larger than that goes out as consecutive launches on the stream, each over the
// next launch_records records.  launch(i0, q) launches the records from i0 on, q being p over them (n, and
// desc or buf advanced); the caller's per-record arrays advance by i0.  Stops at the first failure.
template <class F>
hipError_t for_launches(const smol_csum_ctx_t* ctx, const smol_csum_batch_t* b, const KParams& p, F&& launch) {
    const uint64_t per = ctx->launch_records && ctx->launch_records < b->n ? ctx->launch_records : b->n;
    for (uint64_t i0 = 0; i0 < b->n; i0 += per) {
        KParams q = p;
        q.n = b->n - i0 < per ? b->n - i0 : per;
        if (b->desc) q.desc = b->desc + i0;
        else q.buf = p.buf + i0 * b->stride;
        const hipError_t e = launch(i0, q);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

PickCtx pick_ctx(const smol_csum_ctx_t* ctx) { return {ctx->variant, ctx->shape, ctx->desc_staged}; }

const char* family_kernel(int family) {
    switch (family) {
        case F_TILE: case F_STRIPE: return "csum_tile_kernel";
        case F_XWALK: return "xwalk_kernel";
        case F_DWALK: return "dwalk_kernel";
        case F_COPY: return "copy_kernel";
        case F_XCOPY: return "xcopy_kernel";
        default: return "csum_kernel";
    }
}

// The automatic descriptor-batch emit (nothing forced, IP records, 2-B-field mode not asked).
bool has_desc_auto(const smol_csum_ctx_t* ctx, const smol_csum_batch_t* b, const uint8_t* d_addrs) {
    return b->desc && !d_addrs && ctx->variant < 0 && !(b->flags & SMOL_BATCH_FIELD_STORES);
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// Before the context's entry buffer is used on stream s: a use on another stream than the previous one
// first waits for that one.  The staged descriptor emit records stage_done after every call; the
// fixed-stride route does not (a record per call sits between the emit and the next kernel of a
// single-stream caller, the common case), so the event is recorded here, on the previous stream, when a
// call on a different stream arrives: after everything that stream holds by now, the last use of the
// entries included.  If that record fails (the stream is gone), the device is synchronised instead.
hipError_t order_scratch(smol_csum_ctx_t* ctx, void* stream) {
    if (!ctx->stage_used || ctx->stage_stream == stream) return hipSuccess;
    if (!ctx->stage_recorded) {
        if (hipEventRecord(ctx->stage_done, (hipStream_t)ctx->stage_stream) != hipSuccess) {
            (void)hipGetLastError();
            ctx->stage_used = false;  // nothing is in flight after this
            return hipDeviceSynchronize();
        }
        ctx->stage_recorded = true;
    }
    return hipStreamWaitEvent((hipStream_t)stream, ctx->stage_done, 0);
}

// The automatic route's range, from the interleaved on / off sweeps (profiles/
// emit_route_sweep.jsonl): the record lengths and batch sizes at which the pair beat the one-launch form
// by more than the spread of repeated runs, IPv4/UDP and the IPv6 mix.  Below 1473 B the pair loses
// (1024 B: -12 %), and at 1922 B (4 records per wavefront) too; below 2^20 records the second launch's
// fill and tail cost more than the stores save (2^18: -2 %, 2^19: even), and from 2^22 records on the chunk
// pairs lose to one long launch (2^22: -2.9 %; C5's 2^27: -2.7 %).
constexpr uint32_t kRouteMinLen = 1473, kRouteMaxLen = 1921;
constexpr uint64_t kRouteMinRecords = 1ull << 20, kRouteMaxRecords = 1ull << 21;

// Whether a picked emit runs as the two-launch route (stage 1: the fields-sink form of the picked kernel
// into the context's entries; pass 2: csum_segpass.hip).  Only what pick_kernel chose by itself for a
// plain fixed-stride batch, and never under capture: a captured emit keeps one launch and touches
// neither the entries nor an event.
bool takes_route(const smol_csum_ctx_t* ctx, int mode, const smol_csum_batch_t* b, const Pick& k, const uint8_t* d_addrs,
                 hipStream_t s) {
    if (mode != MODE_EMIT || ctx->emit_route == 0 || ctx->variant >= 0 || b->desc || d_addrs ||
        (b->flags & SMOL_BATCH_FIELD_STORES) || k.family != F_XWALK ||
        (k.variant != kXwalkEmitWT && k.variant != kXwalkEmitNt))
        return false;
    if (ctx->emit_route < 0 &&
        (b->n < kRouteMinRecords || b->n > kRouteMaxRecords || b->len < kRouteMinLen || b->len > kRouteMaxLen))
        return false;
    return !capturing(s);
}

// Before a descriptor-batch emit: take the last staged call's sample when it has arrived (a
// non-blocking event query), and probe with the staged form every kReprobe in-place calls.
void update_desc_choice(smol_csum_ctx_t* ctx, hipStream_t s) {
    if (capturing(s)) return;  // a captured graph keeps the choice it was captured with
    if (ctx->sample_pending && hipEventQuery(ctx->sample_ev) == hipSuccess) {
        ctx->sample_pending = false;
        uint32_t n = ctx->sample_host[kSample], staged = 0;
        for (uint32_t i = 0; i < n && i < kSample; ++i) staged += ctx->sample_host[i] != 0u;
        ctx->desc_staged = n == 0 || 2 * staged >= n ? 1 : 0;
        ctx->since_probe = 0;
    }
    if (!ctx->desc_staged && !ctx->sample_pending && ++ctx->since_probe >= kReprobe) ctx->desc_staged = 1;
}

// After a staged descriptor-batch emit of n records: copy the first wavefront flags to host memory.
void sample_desc_choice(smol_csum_ctx_t* ctx, uint64_t n, hipStream_t s) {
    if (capturing(s) || ctx->sample_pending) return;
    const uint32_t waves = (uint32_t)((n + 7) / 8 < kSample ? (n + 7) / 8 : kSample);
    ctx->sample_host[kSample] = waves;
    if (hipMemcpyAsync(ctx->sample_host, ctx->stage_flags, waves * sizeof(uint32_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipEventRecord(ctx->sample_ev, s) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    ctx->sample_pending = true;
}

int run(smol_csum_ctx_t* ctx, int mode, uint8_t* d_buf, const smol_csum_batch_t* b,
        const smol_checksum_caps_t* caps, uint16_t* d_out, uint8_t* d_status, void* stream,
        const uint8_t* d_src = nullptr, const smol_csum_copy_t* d_copy = nullptr,
        const uint8_t* d_addrs = nullptr) {
    KParams p = base_params(ctx, d_buf, b, caps);
    p.src = d_src;
    p.copy = d_copy;
    if (d_addrs) p.kind = KIND_NHC_UDP;
    p.addrs = d_addrs;
    p.out16 = d_out;
    p.status = d_status;
    p.num_cu = ctx->max_blocks_set ? 0u : cu_count(ctx);
    p.xcd_remap = ctx->xcd_remap >= 0 ? (uint32_t)ctx->xcd_remap : (uint32_t)xcd_remap_auto(mode, b);
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const hipStream_t s = (hipStream_t)stream;
    // A batch larger than launch_records records goes out as consecutive launches on the stream,
    // each over the next launch_records records (the per-record arrays advance with them).
    const uint64_t per = ctx->launch_records ? ctx->launch_records : b->n;
    if (per < b->n) {
        for (uint64_t i0 = 0; i0 < b->n; i0 += per) {
            smol_csum_batch_t sub = *b;
            sub.n = b->n - i0 < per ? b->n - i0 : per;
            uint8_t* buf = d_buf;
            if (b->desc) sub.desc = b->desc + i0;
            else buf = d_buf + i0 * b->stride;
            const uint64_t keep = ctx->launch_records;
            ctx->launch_records = 0;
            const int rc = run(ctx, mode, buf, &sub, caps, d_out ? d_out + i0 : nullptr, d_status ? d_status + i0 : nullptr,
                               stream, d_src, d_copy ? d_copy + i0 : nullptr, d_addrs ? d_addrs + 32 * i0 : nullptr);
            ctx->launch_records = keep;
            if (rc != SMOL_OK) return rc;
        }
        return SMOL_OK;
    }
    const bool desc_auto = mode == MODE_EMIT && has_desc_auto(ctx, b, d_addrs);
    if (desc_auto) update_desc_choice(ctx, s);
    const Pick k = pick_kernel(pick_ctx(ctx), mode, b, p);
    if (mode == MODE_EMIT) ctx->last_route = false;
    if (takes_route(ctx, mode, b, k, d_addrs, s)) {
        // route_chunk records at a time through the context's entries: each chunk's fields launch followed
        // by its segment pass, in stream order
        hipError_t e = order_scratch(ctx, stream);
        if (e != hipSuccess) return hip_fail(e, "ordering the entry buffer (emit route)");
        ctx->stage_stream = stream;
        ctx->stage_used = true;
        ctx->stage_recorded = false;
        for (uint64_t i0 = 0; i0 < b->n; i0 += ctx->route_chunk) {
            KParams q = p;
            q.n = b->n - i0 < ctx->route_chunk ? b->n - i0 : ctx->route_chunk;
            q.buf = d_buf + i0 * b->stride;
            if (d_status) q.status = d_status + i0;
            q.fields = reinterpret_cast<smol_csum_fields_t*>(ctx->stage);
            e = launch_xwalk_route(k.variant, q, s);
            if (e != hipSuccess) return hip_fail(e, "checksum kernel launch (emit route)");
        }
        ctx->last_route = true;
        return SMOL_OK;
    }
    if (mode == MODE_EMIT && variant_is(k.variant, V_STAGED)) {
        // staged emit: kStageChunk records at a time through the context's entries, each chunk's staging
        // launch followed by its segment pass.  A call on another stream than the previous staged emit
        // first waits for that one (the entries are the context's).
        const hipError_t ew = order_scratch(ctx, stream);
        if (ew != hipSuccess) return hip_fail(ew, "hipStreamWaitEvent (staged emit)");
        for (uint64_t i0 = 0; i0 < b->n; i0 += kStageChunk) {
            KParams q = p;
            q.n = b->n - i0 < kStageChunk ? b->n - i0 : kStageChunk;
            if (b->desc) q.desc = b->desc + i0;
            else q.buf = d_buf + i0 * b->stride;
            if (d_status) q.status = d_status + i0;
            q.stage = ctx->stage;
            q.stage_flags = ctx->stage_flags;
            const hipError_t e = k.family == F_DWALK ? launch_dwalk(mode, k.variant, q, s) : launch_xwalk(mode, k.variant, q, s);
            if (e != hipSuccess) return hip_fail(e, "checksum kernel launch");
        }
        if (desc_auto) sample_desc_choice(ctx, b->n < kStageChunk ? b->n : kStageChunk, s);
        hipError_t er = hipEventRecord(ctx->stage_done, s);  // (after the sample's copy: it reads the flags)
        if (er != hipSuccess) return hip_fail(er, "hipEventRecord (staged emit)");
        ctx->stage_stream = stream;
        ctx->stage_used = true;
        ctx->stage_recorded = true;
        return SMOL_OK;
    }
    hipError_t e = hipSuccess;
    switch (k.family) {
        case F_XCOPY: e = launch_xcopy(k.variant, p, s); break;
        case F_DWALK: e = launch_dwalk(mode, k.variant, p, s); break;
        case F_XWALK: e = launch_xwalk(mode, k.variant, p, s); break;
        case F_STRIPE: e = launch_stripe(mode, p, s); break;
        case F_TILE:
            e = launch_tile(mode, k.shape, find_variant(k.variant)->tile_loads, ctx->tile_records, p, ctx->max_blocks, s);
            break;
        default: e = launch_csum(mode, k.shape, k.variant, p, ctx->max_blocks, s); break;  // walk / copy kernels
    }
    if (e != hipSuccess) return hip_fail(e, mode == MODE_COPY ? "copy-emit kernel launch" : "checksum kernel launch");
    return SMOL_OK;
}

}  // namespace

extern "C" {

// The scalar host mirrors (smol_csum_data, _combine, _pseudo_header*) are in csum_scalar.cpp.

// ---- context ---------------------------------------------------------------------------------

int smol_csum_ctx_create(int device, smol_csum_ctx_t** out) {
    if (!out) return SMOL_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        g_last_error = "no HIP device";
        return SMOL_ENODEV;
    }
    if (device < 0 || device >= count) return SMOL_ENODEV;
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute");
    DeviceGuard guard(device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    uint8_t* dummy = nullptr;
    e = hipMalloc(&dummy, 256);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    e = hipMemset(dummy, 0, 256);
    if (e != hipSuccess) {
        (void)hipFree(dummy);
        return hip_fail(e, "hipMemset");
    }
    uint64_t* stage = nullptr;
    uint32_t* flags = nullptr;
    hipEvent_t done = nullptr;
    e = hipMalloc(&stage, kStageChunk * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&flags, (kStageChunk / 8 + 64) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
    uint32_t* sample = nullptr;
    hipEvent_t sev = nullptr;
    if (e == hipSuccess) e = hipHostMalloc(&sample, (kSample + 1) * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sev, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(dummy);
        if (stage) (void)hipFree(stage);
        if (flags) (void)hipFree(flags);
        if (sample) (void)hipHostFree(sample);
        return hip_fail(e, "context allocation");
    }
    auto* c = new (std::nothrow) smol_csum_ctx;
    if (!c) {
        (void)hipFree(dummy);
        (void)hipFree(stage);
        (void)hipFree(flags);
        (void)hipEventDestroy(done);
        (void)hipHostFree(sample);
        (void)hipEventDestroy(sev);
        return SMOL_ENOMEM;
    }
    c->dummy = dummy;
    c->stage = stage;
    c->stage_flags = flags;
    c->stage_stream = nullptr;
    c->stage_used = false;
    c->stage_recorded = false;
    c->emit_route = -1;
    c->route_chunk = kRouteChunk;
    c->last_route = false;
    c->stage_done = done;
    c->sample_host = sample;
    c->sample_ev = sev;
    c->sample_pending = false;
    c->desc_staged = 1;
    c->since_probe = 0;
    c->fields_kernel = FK_AUTO;
    c->vcopy_nt = false;
    c->tile_records = 32;
    c->max_blocks_set = false;
    c->xcd_remap = -1;
    c->launch_records = 0;
    c->device = device;
    c->num_cu = cus;
    c->max_blocks = kNaturalGrid;
    c->shape = -1;
    c->variant = -1;
    *out = c;
    return SMOL_OK;
}

int smol_csum_ctx_destroy(smol_csum_ctx_t* ctx) {
    if (!ctx) return SMOL_OK;
    {
        DeviceGuard guard(ctx->device);
        (void)hipFree(ctx->dummy);
        (void)hipFree(ctx->stage);
        (void)hipFree(ctx->stage_flags);
        (void)hipEventDestroy(ctx->stage_done);
        if (ctx->sample_pending) (void)hipEventSynchronize(ctx->sample_ev);
        (void)hipHostFree(ctx->sample_host);
        (void)hipEventDestroy(ctx->sample_ev);
    }
    delete ctx;
    return SMOL_OK;
}

// ---- batched device entry points -------------------------------------------------------------

int smol_csum_batch_data(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                         uint16_t* d_out, void* stream) {
    if (!ctx) return SMOL_EINVAL;
    int rc = check_batch(b, d_buf);
    if (rc != SMOL_OK || b->n == 0) return rc;
    if (!d_out) return SMOL_EINVAL;
    return run(ctx, MODE_DATA, const_cast<uint8_t*>(d_buf), b, nullptr, d_out, nullptr, stream);
}

int smol_csum_batch_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                         const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    return run(ctx, MODE_EMIT, d_buf, b, caps, nullptr, d_status, stream);
}

int smol_csum_batch_verify(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                           const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_status) return SMOL_EINVAL;
    return run(ctx, MODE_VERIFY, const_cast<uint8_t*>(d_buf), b, caps, nullptr, d_status, stream);
}

int smol_csum_batch_copy_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                              const uint8_t* d_src, const smol_csum_copy_t* d_copy,
                              const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_src || !d_copy || ((uintptr_t)d_copy & 15u) != 0) return SMOL_EINVAL;
    return run(ctx, MODE_COPY, d_buf, b, caps, nullptr, d_status, stream, d_src, d_copy);
}

// Emit with the fields sink (include/smolcsum.h): every record's entry to d_fields, nothing into d_buf.
// Uses none of the context's scratch or events, so calls on different streams are independent.
int smol_csum_batch_emit_fields(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                const smol_checksum_caps_t* caps, smol_csum_fields_t* d_fields, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_fields || ((uintptr_t)d_fields & 15u) != 0) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);  // (the fields sink stores nothing in d_buf)
    p.num_cu = ctx->max_blocks_set ? 0u : cu_count(ctx);
    const hipStream_t s = (hipStream_t)stream;
    return on_device(ctx, "emit_fields kernel launch", [&] {
        return for_launches(ctx, b, p, [&](uint64_t i0, KParams q) {
            q.fields = d_fields + i0;
            switch (pick_fields(ctx->fields_kernel, b, q)) {
                case FK_XWALK: return launch_xwalk_fields(q, s);
                case FK_DWALK: return launch_dwalk_fields(q, s);
                default: break;
            }
            // the walk kernel on variant 5's shape (kWalkVerify: the line grid)
            return b->desc ? launch_walk_fields<false>(auto_shape(b->len, true, kWalkVerify), q, ctx->max_blocks, s)
                           : launch_walk_fields<true>(auto_shape(b->len, false, kWalkVerify), q, ctx->max_blocks, s);
        });
    });
}

// Verify with the payloads delivered in the same pass (include/smolcsum.h).  Uses none of the context's
// scratch or events, so calls on different streams are independent.
int smol_csum_batch_verify_copy(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                const smol_checksum_caps_t* caps, uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                                uint8_t* d_status, smol_csum_span_t* d_spans, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_dst || !d_slots || !d_status || !d_spans || ((uintptr_t)d_slots & 15u) != 0 || ((uintptr_t)d_spans & 7u) != 0)
        return SMOL_EINVAL;
    const KParams p = base_params(ctx, d_buf, b, caps);
    const hipStream_t s = (hipStream_t)stream;
    const int shape = ctx->shape >= 0 ? ctx->shape : vcopy_shape(b->len, b->desc != nullptr);
    return on_device(ctx, "verify_copy kernel launch", [&] {
        return for_launches(ctx, b, p, [&](uint64_t i0, KParams q) {
            q.status = d_status + i0;
            const VCopyArgs v = {d_dst, d_slots + i0, d_spans + i0};
            return launch_vcopy(shape, ctx->vcopy_nt, q, v, ctx->max_blocks, s);
        });
    });
}

// ---- IPv4 fragment groups ---------------------------------------------------------------------

static int run_frag(smol_csum_ctx_t* ctx, int mode, uint8_t* d_buf, const smol_csum_batch_t* b,
                    const smol_csum_frag_group_t* d_groups, uint64_t n_groups, const smol_checksum_caps_t* caps,
                    uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_group_call(ctx, caps, b, d_buf, d_groups, n_groups, &rc)) return rc;
    if (mode == MODE_VERIFY && !d_status) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    return on_device(ctx, "fragment kernel launch", [&] { return launch_frag(mode, p, d_groups, n_groups, (hipStream_t)stream); });
}

int smol_csum_batch_emit_frag(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                              const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                              const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    return run_frag(ctx, MODE_EMIT, d_buf, b, d_groups, n_groups, caps, d_status, stream);
}

int smol_csum_batch_verify_frag(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    return run_frag(ctx, MODE_VERIFY, const_cast<uint8_t*>(d_buf), b, d_groups, n_groups, caps, d_status, stream);
}

// verify_frag with the fragment payloads put together in each group's slot in the same pass
// (include/smolcsum.h).  Uses none of the context's scratch or events, so calls on different streams are
// independent.
int smol_csum_batch_verify_reassemble(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                      const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                      const smol_checksum_caps_t* caps, uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                                      uint8_t* d_status, smol_csum_dgram_t* d_dgrams, void* stream) {
    int rc;
    if (!begin_group_call(ctx, caps, b, d_buf, d_groups, n_groups, &rc)) return rc;
    if (!d_dst || !d_slots || !d_status || !d_dgrams || ((uintptr_t)d_slots & 15u) != 0 || ((uintptr_t)d_dgrams & 15u) != 0)
        return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    const FragCopyArgs v = {d_dst, d_slots, d_dgrams};
    return on_device(ctx, "verify_reassemble kernel launch",
                     [&] { return launch_fragcopy(p, d_groups, n_groups, v, (hipStream_t)stream); });
}

// Emit with every whole IPv4 datagram cut into frames in its place of d_dst in the same pass
// (include/smolcsum.h).  Uses none of the context's scratch or events, so calls on different streams are
// independent.
int smol_csum_batch_fragment_emit(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                  const smol_checksum_caps_t* caps, uint8_t* d_dst, const smol_csum_fragplan_t* d_plans,
                                  uint32_t frame_stride, smol_csum_fragout_t* d_out, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_dst || !d_plans || !d_out || ((uintptr_t)d_plans & 15u) != 0 || ((uintptr_t)d_out & 15u) != 0) return SMOL_EINVAL;
    const KParams p = base_params(ctx, d_buf, b, caps);
    const FragCutArgs v = {d_dst, d_plans, frame_stride, d_out};
    return on_device(ctx, "fragment_emit kernel launch", [&] { return launch_fragcut(p, v, (hipStream_t)stream); });
}

// ---- 6LoWPAN NHC UDP --------------------------------------------------------------------------

int smol_csum_batch_nhc_udp_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                                 const smol_ipv6_addr_pair_t* d_addrs, const smol_checksum_caps_t* caps,
                                 uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_addrs || ((uintptr_t)d_addrs & 3u) != 0) return SMOL_EINVAL;
    return run(ctx, MODE_EMIT, d_buf, b, caps, nullptr, d_status, stream, nullptr, nullptr,
               reinterpret_cast<const uint8_t*>(d_addrs));
}

int smol_csum_batch_nhc_udp_verify(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                   const smol_ipv6_addr_pair_t* d_addrs, const smol_checksum_caps_t* caps,
                                   uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_status || !d_addrs || ((uintptr_t)d_addrs & 3u) != 0) return SMOL_EINVAL;
    return run(ctx, MODE_VERIFY, const_cast<uint8_t*>(d_buf), b, caps, nullptr, d_status, stream, nullptr,
               nullptr, reinterpret_cast<const uint8_t*>(d_addrs));
}

const char* smol_csum_last_error(void) { return g_last_error.c_str(); }

int smol_csum_abi_version(void) { return SMOLCSUM_ABI_VERSION; }

// ---- tooling (include/smolcsum_tools.h) -------------------------------------------------------

int smol_csum_tool_synth(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                         int profile, uint64_t seed, void* stream) {
    if (!ctx || profile < 0 || profile > SMOL_SYNTH_RANDOM) return SMOL_EINVAL;
    int rc = check_batch(b, d_buf);
    if (rc != SMOL_OK || b->n == 0) return rc;
    SynthParams p{d_buf, b->desc, b->n, b->stride, b->len, (uint32_t)profile, seed};
    return on_device(ctx, "synth kernel launch", [&] {
        return launch_synth(p, ctx->max_blocks, (hipStream_t)stream);
    });
}

int smol_csum_tool_corrupt(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                           uint32_t every, uint64_t seed, void* stream) {
    if (!ctx || every == 0) return SMOL_EINVAL;
    int rc = check_batch(b, d_buf);
    if (rc != SMOL_OK || b->n == 0) return rc;
    SynthParams p{d_buf, b->desc, b->n, b->stride, b->len, 0u, seed};
    return on_device(ctx, "corrupt kernel launch", [&] {
        return launch_corrupt(p, every, (hipStream_t)stream);
    });
}

int smol_csum_tool_set_shape(smol_csum_ctx_t* ctx, int shape) {
    if (!ctx || shape < -1 || shape >= CFG_COUNT) return SMOL_EINVAL;
    ctx->shape = shape;
    return SMOL_OK;
}

int smol_csum_tool_variant_built(int variant) { return variant_built(variant) ? 1 : 0; }

int smol_csum_tool_set_variant(smol_csum_ctx_t* ctx, int variant) {
    if (!ctx || !variant_built(variant)) return SMOL_EINVAL;
    ctx->variant = variant;
    return SMOL_OK;
}

int smol_csum_tool_set_tile(smol_csum_ctx_t* ctx, int records) {
    if (!ctx || (records != 32 && records != 64)) return SMOL_EINVAL;
    ctx->tile_records = records;
    return SMOL_OK;
}

int smol_csum_tool_set_max_blocks(smol_csum_ctx_t* ctx, uint32_t max_blocks) {
    if (!ctx) return SMOL_EINVAL;
    ctx->max_blocks = max_blocks ? max_blocks : kNaturalGrid;
    ctx->max_blocks_set = max_blocks != 0;
    return SMOL_OK;
}

int smol_csum_tool_set_xcd_remap(smol_csum_ctx_t* ctx, int on) {
    if (!ctx || on < -1) return SMOL_EINVAL;
    ctx->xcd_remap = on;
    return SMOL_OK;
}

int smol_csum_tool_set_launch_records(smol_csum_ctx_t* ctx, uint64_t records) {
    if (!ctx) return SMOL_EINVAL;
    ctx->launch_records = records;
    return SMOL_OK;
}

int smol_csum_tool_set_fields_kernel(smol_csum_ctx_t* ctx, int kernel) {
    if (!ctx || kernel < FK_AUTO || kernel > FK_DWALK) return SMOL_EINVAL;
    ctx->fields_kernel = kernel;
    return SMOL_OK;
}

int smol_csum_tool_set_emit_route(smol_csum_ctx_t* ctx, int route) {
    if (!ctx || route < -1 || route > 1) return SMOL_EINVAL;
    ctx->emit_route = route;
    return SMOL_OK;
}

int smol_csum_tool_last_route(const smol_csum_ctx_t* ctx) { return ctx ? (ctx->last_route ? 1 : 0) : SMOL_EINVAL; }

int smol_csum_tool_set_route_chunk(smol_csum_ctx_t* ctx, uint64_t records) {
    if (!ctx || records > kRouteChunk) return SMOL_EINVAL;
    ctx->route_chunk = records ? records : kRouteChunk;
    return SMOL_OK;
}

int smol_csum_tool_set_vcopy_stores(smol_csum_ctx_t* ctx, int nt) {
    if (!ctx || (nt != 0 && nt != 1)) return SMOL_EINVAL;
    ctx->vcopy_nt = nt == 1;
    return SMOL_OK;
}

int smol_csum_tool_stream_read(smol_csum_ctx_t* ctx, const uint8_t* d_buf, uint64_t bytes,
                               uint32_t* d_sink, void* stream) {
    if (!ctx || !d_buf || !d_sink || (bytes & 15u) || ((uintptr_t)d_buf & 15u)) return SMOL_EINVAL;
    return on_device(ctx, "stream-read kernel launch", [&] {
        return launch_stream_read(d_buf, bytes, d_sink, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_field_probe(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, uint64_t stride,
                               uint32_t f1, uint32_t f2, void* stream) {
    if (!ctx || !d_buf || (bytes & 15u) || ((uintptr_t)d_buf & 15u) || stride == 0 || f1 == ~0u) return SMOL_EINVAL;
    return on_device(ctx, "field-probe kernel launch", [&] {
        return launch_field_probe(d_buf, bytes, stride, f1, f2, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_field_probe_list(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, const uint64_t* d_addrs,
                                    const uint32_t* d_piece_first, int flags, void* stream) {
    if (!ctx || !d_buf || !d_addrs || !d_piece_first || (bytes & 15u) || ((uintptr_t)d_buf & 15u) || (flags & ~1))
        return SMOL_EINVAL;
    return on_device(ctx, "field-probe kernel launch", [&] {
        return launch_field_probe_list(d_buf, bytes, d_addrs, d_piece_first, flags & 1, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_segment_probe(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, const uint32_t* d_bitmap, int flags,
                                 void* stream) {
    if (!ctx || !d_buf || !d_bitmap || (bytes & 15u) || ((uintptr_t)d_buf & 15u) || ((uintptr_t)d_bitmap & 15u) ||
        (flags & ~1))
        return SMOL_EINVAL;
    return on_device(ctx, "segment-probe kernel launch", [&] {
        return launch_segment_probe(d_buf, bytes, d_bitmap, flags & 1, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_field_scatter(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, const uint64_t* d_addrs,
                                 const uint16_t* d_vals, uint64_t n, int flags, void* stream) {
    if (!ctx || !d_buf || (n && (!d_addrs || !d_vals)) || (flags & ~15) || n > (0xFFFFFFull << 8)) return SMOL_EINVAL;
    return on_device(ctx, "field-scatter kernel launch", [&] {
        return launch_field_scatter(d_buf, bytes, d_addrs, d_vals, n, flags & 15, (hipStream_t)stream);
    });
}

int smol_csum_tool_auto_shape(uint32_t len, int has_desc) {
    // the walk kernel's verify shape (descriptor batches: kWalkVerifyDesc, which serves them when the
    // descriptor walk does not: NHC, data, forced variants)
    return auto_shape(len, has_desc != 0, walk_variant(MODE_VERIFY, has_desc != 0));
}

const char* smol_csum_tool_kernel_name(const smol_csum_ctx_t* ctx, int op, int has_desc) {
    // Without the batch this cannot see its record length: it answers for a batch that no
    // length-dependent kernel serves (descriptor batches exactly; fixed-stride batches the walk kernel's
    // lengths).  smol_csum_tool_kernel_for takes the batch.
    if (!ctx || op < MODE_DATA || op > MODE_COPY) return "";
    smol_csum_batch_t b;
    std::memset(&b, 0, sizeof b);
    b.n = 1;
    b.len = b.stride = 64;
    b.desc = has_desc ? reinterpret_cast<const smol_csum_desc_t*>(ctx->dummy) : nullptr;
    return smol_csum_tool_kernel_for(ctx, op, &b);
}

int smol_csum_tool_pick(int variant, int shape, int desc_staged, int op, const smol_csum_batch_t* b, int nhc, int out[3]) {
    if (!b || !out || op < MODE_DATA || op > MODE_COPY || !variant_built(variant) || shape < -1 || shape >= CFG_COUNT)
        return SMOL_EINVAL;
    KParams p;  // what the dispatch reads of the launch parameters: the batch form (nothing dereferenced)
    std::memset(&p, 0, sizeof p);
    p.desc = b->desc;
    p.n = b->n;
    p.stride = b->stride;
    p.len = b->len;
    p.addrs = nhc ? reinterpret_cast<const uint8_t*>(b) : nullptr;  // (only marks an NHC batch)
    const Pick k = pick_kernel(PickCtx{variant, shape, desc_staged}, op, b, p);
    out[0] = k.family;
    out[1] = k.variant;
    out[2] = k.shape;
    return SMOL_OK;
}

const char* smol_csum_tool_kernel_for(const smol_csum_ctx_t* ctx, int op, const smol_csum_batch_t* b) {
    int k[3];
    if (!ctx || smol_csum_tool_pick(ctx->variant, ctx->shape, ctx->desc_staged, op, b, 0, k) != SMOL_OK) return "";
    return family_kernel(k[0]);
}

int smol_csum_tool_variant_info(int variant, int out[4]) {
    const Variant* r = find_variant(variant);
    if (!r || !out) return SMOL_EINVAL;
    out[0] = r->family;
    out[1] = r->flags;
    out[2] = r->built() ? 1 : 0;
    out[3] = r->exp_only ? 1 : 0;
    return SMOL_OK;
}

int smol_csum_tool_form(int variant, int op, int out[13]) {
    if (!out || (op != MODE_EMIT && op != MODE_VERIFY)) return SMOL_EINVAL;
    const bool emit = op == MODE_EMIT;
    auto xw = [&](auto f) {
        const int v[13] = {F_XWALK, f.NOSTORE, f.SEG, f.PERSIST, f.NTS,   f.HALF,  f.STAGE,
                           f.HINT,  f.WPE,     f.WV,  f.STEPS,   f.ONLY_R, f.MAX_LEN == ~0u ? 0 : (int)f.MAX_LEN};
        std::memcpy(out, v, sizeof v);
    };
    if (emit ? with_xwalk_form<true>(variant, xw) : with_xwalk_form<false>(variant, xw)) return SMOL_OK;
    bool none = true;
    auto dw = [&](auto f) {
        const int v[13] = {F_DWALK, f.NOSTORE, f.GROUPS, f.SEGF, f.SEGPASS};
        std::memcpy(out, v, sizeof v);
        none = f.NONE;
    };
    const bool d = emit ? with_dwalk_form<true>(variant, dw) : with_dwalk_form<false>(variant, dw);
    return d && !none ? SMOL_OK : SMOL_EINVAL;
}

int smol_csum_tool_walk_launch(int variant, int op, int implicit, int nhc, int shape, int out[4]) {
    if (!out || op < MODE_DATA || op > MODE_COPY || shape < 0 || shape >= CFG_COUNT) return SMOL_EINVAL;
    if (nhc && op != MODE_EMIT && op != MODE_VERIFY) return SMOL_EINVAL;
    const int kern = nhc ? KERN_WALK_NHC : KERN_WALK;
    auto note = [&](auto, auto num, auto g, auto u) {
        const int v[4] = {kern, decltype(num)::value, decltype(g)::value, decltype(u)::value};
        std::memcpy(out, v, sizeof v);
    };
    auto batch_form = [&](auto mode, auto is_nhc) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool NHC = decltype(is_nhc)::value;
        return implicit ? with_walk_kernel<MODE, true, NHC>(variant, shape, note)
                        : with_walk_kernel<MODE, false, NHC>(variant, shape, note);
    };
    using std::integral_constant;
    bool ok = false;
    if (op == MODE_COPY && with_copy_kernel(variant, shape, [&](auto, auto num, auto g, auto u, auto, auto) {
            const int v[4] = {KERN_COPY, decltype(num)::value, decltype(g)::value, decltype(u)::value};
            std::memcpy(out, v, sizeof v);
        }))
        return SMOL_OK;  // a COPY row: copy_kernel's launcher, whatever the batch form
    if (nhc) {
        ok = op == MODE_EMIT ? batch_form(integral_constant<int, MODE_EMIT>{}, std::true_type{})
                             : batch_form(integral_constant<int, MODE_VERIFY>{}, std::true_type{});
    } else {
        switch (op) {
            case MODE_DATA: ok = batch_form(integral_constant<int, MODE_DATA>{}, std::false_type{}); break;
            case MODE_EMIT: ok = batch_form(integral_constant<int, MODE_EMIT>{}, std::false_type{}); break;
            case MODE_VERIFY: ok = batch_form(integral_constant<int, MODE_VERIFY>{}, std::false_type{}); break;
            default: ok = batch_form(integral_constant<int, MODE_COPY>{}, std::false_type{}); break;
        }
    }
    return ok ? SMOL_OK : SMOL_EINVAL;
}

uint32_t smol_csum_tool_last_launch(void) { return g_last_launch.load(std::memory_order_relaxed); }

}  // extern "C"
