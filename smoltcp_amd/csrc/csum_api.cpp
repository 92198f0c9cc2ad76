// C ABI of the checksum engine (include/smolcsum.h): the context and the batched device entry points.  The
// scalar host mirrors of smoltcp::wire::checksum are in csum_scalar.cpp, the tooling entry points
// (include/smolcsum_tools.h) in csum_tools.cpp.  No exception crosses this boundary; every batched call either
// launches HIP kernels or returns an error — there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/smolcsum.h"
#include "csum_ctx.h"

using namespace smolcsum;

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

bool caps_valid(const smol_checksum_caps_t* c) {
    if (!c) return false;
    const uint8_t v[5] = {c->ipv4, c->udp, c->tcp, c->icmpv4, c->icmpv6};
    for (uint8_t x : v)
        if (x > SMOL_CHECKSUM_NONE) return false;
    return c->reserved[0] == 0 && c->reserved[1] == 0 && c->reserved[2] == 0;
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

// Zeroed launch parameters with what every batched call takes from its arguments: the batch form, the
// record kind, the caps (none: smol_csum_batch_data) and the dummy line.  The entry points add their own
// per-record arrays.
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

PickCtx pick_ctx(const smol_csum_ctx_t* ctx) { return {ctx->variant, ctx->shape, ctx->desc_staged}; }

// The automatic descriptor-batch emit (nothing forced, IP records, 2-B-field mode not asked).
bool has_desc_auto(const smol_csum_ctx_t* ctx, const smol_csum_batch_t* b, const KParams& p) {
    return b->desc && !p.addrs && ctx->variant < 0 && !(b->flags & SMOL_BATCH_FIELD_STORES);
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
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
bool takes_route(const smol_csum_ctx_t* ctx, int mode, const smol_csum_batch_t* b, const Pick& k, const KParams& p,
                 hipStream_t s) {
    if (mode != MODE_EMIT || ctx->emit_route == 0 || ctx->variant >= 0 || b->desc || p.addrs ||
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
    if (hipMemcpyAsync(ctx->sample_host, ctx->scratch.flags, waves * sizeof(uint32_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipEventRecord(ctx->sample_ev, s) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    ctx->sample_pending = true;
}

// One data / emit / verify / copy-emit call over the batch b, p being its launch parameters (run() below
// cuts them): the choice of kernel for this batch, then its launches on stream s.
int run_one(smol_csum_ctx_t* ctx, int mode, const smol_csum_batch_t* b, KParams p, hipStream_t s) {
    p.xcd_remap = ctx->xcd_remap >= 0 ? (uint32_t)ctx->xcd_remap : (uint32_t)xcd_remap_auto(mode, b);
    const bool desc_auto = mode == MODE_EMIT && has_desc_auto(ctx, b, p);
    if (desc_auto) update_desc_choice(ctx, s);
    const Pick k = pick_kernel(pick_ctx(ctx), mode, b, p);
    EntryBuffer& scratch = ctx->scratch;
    if (mode == MODE_EMIT) ctx->last_route = false;
    if (takes_route(ctx, mode, b, k, p, s)) {
        // route_chunk records at a time through the context's entries: each chunk's fields launch followed
        // by its segment pass, in stream order.  No event is recorded after them (EntryBuffer::acquire), so
        // the use is noted before the launches.
        hipError_t e = scratch.acquire(s);
        if (e != hipSuccess) return hip_fail(e, "ordering the entry buffer (emit route)");
        scratch.release(s, false);
        e = for_chunks(p, ctx->route_chunk, [&](uint64_t, KParams q) {
            q.fields = reinterpret_cast<smol_csum_fields_t*>(scratch.entries);
            return launch_xwalk_route(k.variant, q, s);
        });
        if (e != hipSuccess) return hip_fail(e, "checksum kernel launch (emit route)");
        ctx->last_route = true;
        return SMOL_OK;
    }
    if (mode == MODE_EMIT && variant_is(k.variant, V_STAGED)) {
        // staged emit: kStageChunk records at a time through the context's entries, each chunk's staging
        // launch followed by its segment pass; `done` is recorded after every call
        hipError_t e = scratch.acquire(s);
        if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent (staged emit)");
        e = for_chunks(p, kStageChunk, [&](uint64_t, KParams q) {
            q.stage = scratch.entries;
            q.stage_flags = scratch.flags;
            return k.family == F_DWALK ? launch_dwalk(mode, k.variant, q, s) : launch_xwalk(mode, k.variant, q, s);
        });
        if (e != hipSuccess) return hip_fail(e, "checksum kernel launch");
        if (desc_auto) sample_desc_choice(ctx, b->n < kStageChunk ? b->n : kStageChunk, s);
        e = hipEventRecord(scratch.done, s);  // (after the sample's copy: it reads the flags)
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord (staged emit)");
        scratch.release(s, true);
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

// A batch larger than launch_records records goes out as consecutive calls on the stream, each over the
// next launch_records records and each with its own choice of kernel (run_one).
int run(smol_csum_ctx_t* ctx, int mode, const smol_csum_batch_t* b, KParams p, void* stream) {
    p.num_cu = ctx->max_blocks_set ? 0u : cu_count(ctx);
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    return for_chunks(p, ctx->launch_records, [&](uint64_t, const KParams& q) {
        smol_csum_batch_t sub = *b;
        sub.n = q.n;
        sub.desc = q.desc;
        return run_one(ctx, mode, &sub, q, (hipStream_t)stream);
    });
}

// Null-safe; what smol_csum_ctx_create has allocated so far, or everything.
void free_resources(smol_csum_ctx_t* ctx) {
    if (!ctx) return;
    {
        DeviceGuard guard(ctx->device);
        (void)hipFree(ctx->dummy);
        (void)hipFree(ctx->scratch.entries);
        (void)hipFree(ctx->scratch.flags);
        if (ctx->scratch.done) (void)hipEventDestroy(ctx->scratch.done);
        if (ctx->sample_pending) (void)hipEventSynchronize(ctx->sample_ev);
        (void)hipHostFree(ctx->sample_host);
        if (ctx->sample_ev) (void)hipEventDestroy(ctx->sample_ev);
    }
    delete ctx;
}

}  // namespace

extern "C" {

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
    auto* c = new (std::nothrow) smol_csum_ctx;
    if (!c) return SMOL_ENOMEM;
    c->device = device;
    c->num_cu = cus;
    const char* what = "hipMalloc";
    e = hipMalloc(&c->dummy, 256);
    if (e == hipSuccess) {
        what = "hipMemset";
        e = hipMemset(c->dummy, 0, 256);
    }
    if (e == hipSuccess) {
        what = "context allocation";
        e = hipMalloc(&c->scratch.entries, kStageChunk * sizeof(uint64_t));
    }
    if (e == hipSuccess) e = hipMalloc(&c->scratch.flags, (kStageChunk / 8 + 64) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->scratch.done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(&c->sample_host, (kSample + 1) * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->sample_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        free_resources(c);
        return hip_fail(e, what);
    }
    *out = c;
    return SMOL_OK;
}

int smol_csum_ctx_destroy(smol_csum_ctx_t* ctx) {
    free_resources(ctx);
    return SMOL_OK;
}

// ---- batched device entry points -------------------------------------------------------------

int smol_csum_batch_data(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                         uint16_t* d_out, void* stream) {
    if (!ctx) return SMOL_EINVAL;
    int rc = check_batch(b, d_buf);
    if (rc != SMOL_OK || b->n == 0) return rc;
    if (!d_out) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, nullptr);
    p.out16 = d_out;
    return run(ctx, MODE_DATA, b, p, stream);
}

int smol_csum_batch_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                         const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    return run(ctx, MODE_EMIT, b, p, stream);
}

int smol_csum_batch_verify(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                           const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_status) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    return run(ctx, MODE_VERIFY, b, p, stream);
}

int smol_csum_batch_copy_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                              const uint8_t* d_src, const smol_csum_copy_t* d_copy,
                              const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_src || !d_copy || ((uintptr_t)d_copy & 15u) != 0) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    p.src = d_src;
    p.copy = d_copy;
    return run(ctx, MODE_COPY, b, p, stream);
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
    p.fields = d_fields;
    const hipStream_t s = (hipStream_t)stream;
    return on_device(ctx, "emit_fields kernel launch", [&] {
        return for_chunks(p, ctx->launch_records, [&](uint64_t, const KParams& q) {
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
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    const hipStream_t s = (hipStream_t)stream;
    const int shape = ctx->shape >= 0 ? ctx->shape : vcopy_shape(b->len, b->desc != nullptr);
    return on_device(ctx, "verify_copy kernel launch", [&] {
        return for_chunks(p, ctx->launch_records, [&](uint64_t i0, const KParams& q) {
            const VCopyArgs v = {d_dst, d_slots + i0, d_spans + i0};
            return launch_vcopy(shape, ctx->vcopy_nt, q, v, ctx->max_blocks, s);
        });
    });
}

// The responders' configuration (NULL: none): false when a reserved byte is set; *bcast is the interface's
// IPv4 broadcast address as a big-endian word, 0 without one.
static bool responder_cfg(const smol_csum_echo_cfg_t* cfg, uint32_t* bcast) {
    *bcast = 0;
    if (!cfg) return true;
    if (cfg->reserved[0] | cfg->reserved[1] | cfg->reserved[2] | cfg->reserved[3]) return false;
    *bcast = (uint32_t)cfg->bcast_v4[0] << 24 | (uint32_t)cfg->bcast_v4[1] << 16 | (uint32_t)cfg->bcast_v4[2] << 8 |
             (uint32_t)cfg->bcast_v4[3];
    return true;
}

// Verify with the replies to the batch's echo requests written in the same pass (include/smolcsum.h).  Uses
// none of the context's scratch or events, so calls on different streams are independent.
int smol_csum_batch_verify_echo_reply(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                      const smol_checksum_caps_t* caps, const smol_csum_echo_cfg_t* cfg,
                                      uint8_t* d_dst, const smol_csum_slot_t* d_slots, uint8_t* d_status,
                                      smol_csum_echo_t* d_echo, void* stream) {
    int rc;
    const bool work = begin_call(ctx, caps, b, d_buf, &rc);
    if (rc != SMOL_OK) return rc;
    uint32_t bcast;
    if (!responder_cfg(cfg, &bcast)) return SMOL_EINVAL;
    if (!work) return rc;
    if (!d_dst || !d_slots || !d_status || !d_echo || ((uintptr_t)d_slots & 15u) != 0 || ((uintptr_t)d_echo & 7u) != 0)
        return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    const hipStream_t s = (hipStream_t)stream;
    const int shape = ctx->shape >= 0 ? ctx->shape : echo_shape(b->len, b->desc != nullptr);
    return on_device(ctx, "verify_echo_reply kernel launch", [&] {
        return for_chunks(p, ctx->launch_records, [&](uint64_t i0, const KParams& q) {
            const EchoArgs v = {d_dst, d_slots + i0, d_echo + i0, bcast};
            return launch_echo(shape, q, v, ctx->max_blocks, s);
        });
    });
}

// Verify with the ICMP errors for the batch's refused datagrams written in the same pass (include/smolcsum.h).
// Uses none of the context's scratch or events, so calls on different streams are independent.
int smol_csum_batch_verify_unreach_reply(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                         const smol_checksum_caps_t* caps, const smol_csum_echo_cfg_t* cfg,
                                         const uint8_t* d_udp_open, uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                                         uint8_t* d_status, smol_csum_unreach_t* d_unr, void* stream) {
    int rc;
    const bool work = begin_call(ctx, caps, b, d_buf, &rc);
    if (rc != SMOL_OK) return rc;
    uint32_t bcast;
    if (!responder_cfg(cfg, &bcast)) return SMOL_EINVAL;
    if (!work) return rc;
    if (!d_dst || !d_slots || !d_status || !d_unr || ((uintptr_t)d_slots & 15u) != 0 || ((uintptr_t)d_unr & 7u) != 0)
        return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    const hipStream_t s = (hipStream_t)stream;
    const int shape = ctx->shape >= 0 ? ctx->shape : unreach_shape(b->len, b->desc != nullptr);
    return on_device(ctx, "verify_unreach_reply kernel launch", [&] {
        return for_chunks(p, ctx->launch_records, [&](uint64_t i0, const KParams& q) {
            const UnreachArgs v = {d_dst, d_slots + i0, d_unr + i0, d_udp_open, bcast};
            return launch_unreach(shape, q, v, ctx->max_blocks, s);
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

// Every send's header template and payload range cut into MSS-sized frames in its place of d_dst, checksums
// filled in the same pass (include/smolcsum.h).  Uses none of the context's scratch or events, so calls on
// different streams are independent.
int smol_csum_batch_tcp_segment_emit(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                     const smol_checksum_caps_t* caps, const uint8_t* d_src, uint8_t* d_dst,
                                     const smol_csum_tcpplan_t* d_plans, uint32_t frame_stride,
                                     smol_csum_tcpout_t* d_out, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_src || !d_dst || !d_plans || !d_out || ((uintptr_t)d_plans & 15u) != 0 || ((uintptr_t)d_out & 15u) != 0)
        return SMOL_EINVAL;
    const KParams p = base_params(ctx, d_buf, b, caps);
    const TcpCutArgs v = {d_src, d_dst, d_plans, frame_stride, d_out};
    return on_device(ctx, "tcp_segment_emit kernel launch", [&] { return launch_tcpcut(p, v, (hipStream_t)stream); });
}

// Verify with every TCP segment's payload delivered to its sequence number's place in its connection's
// receive ring in the same pass (include/smolcsum.h).  Uses none of the context's scratch or events, so calls
// on different streams are independent.
int smol_csum_batch_verify_tcp_assemble(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                        const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                        const smol_checksum_caps_t* caps, uint8_t* d_dst, const smol_csum_tcpwin_t* d_wins,
                                        uint8_t* d_status, smol_csum_tcpseg_t* d_segs, smol_csum_tcpflow_t* d_flows,
                                        void* stream) {
    int rc;
    if (!begin_group_call(ctx, caps, b, d_buf, d_groups, n_groups, &rc)) return rc;
    if (!d_dst || !d_wins || !d_status || !d_segs || !d_flows || ((uintptr_t)d_wins & 15u) != 0 ||
        ((uintptr_t)d_segs & 15u) != 0 || ((uintptr_t)d_flows & 15u) != 0)
        return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    const TcpAsmArgs v = {d_dst, d_wins, d_segs, d_flows};
    return on_device(ctx, "verify_tcp_assemble kernel launch",
                     [&] { return launch_tcpasm(p, d_groups, n_groups, v, ctx->max_blocks, (hipStream_t)stream); });
}

// Verify with every UDP datagram's payload delivered to the place its socket's PacketBuffer::enqueue gives it,
// metadata entries written, in the same pass (include/smolcsum.h).  Uses none of the context's scratch or
// events, so calls on different streams are independent.
int smol_csum_batch_verify_udp_enqueue(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                       const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                       const smol_checksum_caps_t* caps, uint8_t* d_dst, const smol_csum_udpsock_t* d_socks,
                                       smol_csum_udpmeta_t* d_meta, uint8_t* d_status, smol_csum_udprx_t* d_rx,
                                       smol_csum_udpsockout_t* d_out, void* stream) {
    int rc;
    if (!begin_group_call(ctx, caps, b, d_buf, d_groups, n_groups, &rc)) return rc;
    if (!d_dst || !d_socks || !d_meta || !d_status || !d_rx || !d_out || ((uintptr_t)d_socks & 15u) != 0 ||
        ((uintptr_t)d_meta & 15u) != 0 || ((uintptr_t)d_rx & 15u) != 0 || ((uintptr_t)d_out & 15u) != 0)
        return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.status = d_status;
    const UdpRxArgs v = {d_dst, d_socks, d_meta, d_rx, d_out};
    return on_device(ctx, "verify_udp_enqueue kernel launch",
                     [&] { return launch_udprx(p, d_groups, n_groups, v, ctx->max_blocks, (hipStream_t)stream); });
}

// Every socket's transmit PacketBuffer dequeued and its datagrams written out as frames, headers built on the
// device, checksums filled in the pass that copies the payload (include/smolcsum.h).  No batch: the sockets'
// buffers are the input.  Uses none of the context's scratch or events, so calls on different streams are
// independent.
int smol_csum_batch_udp_dequeue_emit(smol_csum_ctx_t* ctx, const uint8_t* d_src, const smol_csum_udptxsock_t* d_socks,
                                     uint64_t n_groups, const smol_csum_udpmeta_t* d_meta, const smol_checksum_caps_t* caps,
                                     uint8_t* d_dst, uint32_t frame_stride, smol_csum_udptx_t* d_tx,
                                     smol_csum_udptxout_t* d_out, void* stream) {
    if (!ctx || !caps_valid(caps)) return SMOL_EINVAL;
    if (n_groups == 0) return SMOL_OK;
    if (!d_src || !d_socks || !d_meta || !d_dst || !d_tx || !d_out || ((uintptr_t)d_socks & 15u) != 0 ||
        ((uintptr_t)d_meta & 15u) != 0 || ((uintptr_t)d_tx & 15u) != 0 || ((uintptr_t)d_out & 15u) != 0)
        return SMOL_EINVAL;
    const UdpTxArgs v = {d_src, d_socks, d_meta, d_dst, d_tx, d_out, ctx->dummy, frame_stride, caps->ipv4, caps->udp};
    return on_device(ctx, "udp_dequeue_emit kernel launch",
                     [&] { return launch_udptx(v, n_groups, ctx->max_blocks, (hipStream_t)stream); });
}

// ---- 6LoWPAN NHC UDP --------------------------------------------------------------------------

int smol_csum_batch_nhc_udp_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                                 const smol_ipv6_addr_pair_t* d_addrs, const smol_checksum_caps_t* caps,
                                 uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_addrs || ((uintptr_t)d_addrs & 3u) != 0) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.kind = KIND_NHC_UDP;
    p.addrs = reinterpret_cast<const uint8_t*>(d_addrs);
    p.status = d_status;
    return run(ctx, MODE_EMIT, b, p, stream);
}

int smol_csum_batch_nhc_udp_verify(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* b,
                                   const smol_ipv6_addr_pair_t* d_addrs, const smol_checksum_caps_t* caps,
                                   uint8_t* d_status, void* stream) {
    int rc;
    if (!begin_call(ctx, caps, b, d_buf, &rc)) return rc;
    if (!d_status || !d_addrs || ((uintptr_t)d_addrs & 3u) != 0) return SMOL_EINVAL;
    KParams p = base_params(ctx, d_buf, b, caps);
    p.kind = KIND_NHC_UDP;
    p.addrs = reinterpret_cast<const uint8_t*>(d_addrs);
    p.status = d_status;
    return run(ctx, MODE_VERIFY, b, p, stream);
}

const char* smol_csum_last_error(void) { return g_last_error.c_str(); }

int smol_csum_abi_version(void) { return SMOLCSUM_ABI_VERSION; }

}  // extern "C"
