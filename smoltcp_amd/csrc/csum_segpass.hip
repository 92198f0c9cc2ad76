// The segment pass of the two-launch fixed-stride emit (the route of csum_api.cpp run_one(): stage 1 is
// xwalk_kernel<MODE_EMIT, R, XFields> writing every record's emit_fields entry into the context's scratch,
// this pass writes the records).  seg_pass4_kernel (csum_dwalk.hip) serves the staged descriptor emit with
// one record per lane group and three dependent loads (flag, entry, segment); here stage 1 writes every
// entry (no flags), the stride is fixed, and a lane group keeps several records in flight:
//  - a group of 4 lanes x 16 B takes K consecutive records: first the K entries and the entry before the
//    first (the neighbour the rule asks about at a group seam; inside the group it is a register), all
//    requested together; then csum_segrule.h decides per record, and the segments of all K records are
//    requested together before any is patched or stored: two memory round trips per K records;
//  - whole segments are patched and stored write-through and non-temporal (sc0 sc1 nt, seg_pass4_kernel's
//    policy, written as the instruction: a vector store); a record the rule gives no segments stores every
//    field as a 2-B store by the group's lane 0;
//  - lane 0 writes the status byte the entry carries when the caller asked for status.
// Only segments the rule returned are loaded, so no load or store leaves the batch.
//
// Measured and dropped (C2, kernel traces; this form: 0.0607 ms, seg_pass4_kernel
// 0.0557 ms):
//  - address speculation, that is the two segments covering record bytes [0, 128 - a0 % 64) requested
//    together with the entries, one round trip: 0.0788 ms.  The pass is bound by the lines it moves (2
//    segment reads per record instead of the 1.25 it needs), not by its round trips;
//  - a wavefront's 64 records dealt so that each entry load instruction takes 16 consecutive entries
//    (group g: records 16 k + g), the neighbour's field end by a shuffle: 0.0647 ms.
#include "csum_dispatch.h"
#include "csum_segrule.h"
#include "csum_walk.h"

namespace smolcsum {

namespace segpass {
constexpr int K = 4;                  // records per lane group
constexpr int GROUPS = 64;            // lane groups per workgroup (256 threads)
constexpr int PER_BLOCK = K * GROUPS; // records per workgroup
}  // namespace segpass

__global__ __launch_bounds__(256) void seg_pass_fields_kernel(KParams p) {
    using namespace segpass;
    const uint64_t r0 = ((uint64_t)blockIdx.x * GROUPS + (threadIdx.x >> 2)) * K;
    const uint32_t l = threadIdx.x & 3u;
    if (r0 >= p.n) return;
    const uint32_t cnt = (uint32_t)(p.n - r0 < (uint64_t)K ? p.n - r0 : (uint64_t)K);
    const uint32_t len = p.len;
    const uint64_t stride = p.stride;
    const uint64_t base = (uint64_t)p.buf;
    const uint64_t total = (p.n - 1) * stride + len;  // the batch's bytes
    const uint64_t ent = (uint64_t)p.fields;

    // ---- the entries (unconditional, so that they issue back to back: a record past the batch's last
    // loads the last one's again; record 0's neighbour entry is its own and not used) ----
    u32x4 e[K + 1];
    e[0] = __builtin_nontemporal_load((const GMEM u32x4*)(ent + 16 * (r0 != 0 ? r0 - 1 : 0)));
#pragma unroll
    for (int k = 0; k < K; ++k)
        e[k + 1] = __builtin_nontemporal_load((const GMEM u32x4*)(ent + 16 * (r0 + ((uint32_t)k < cnt ? (uint32_t)k : cnt - 1))));

    // ---- decide; every segment load of the group's records ----
    SegRule d[K];
    u32x4 xa[K], xb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t r = r0 + (uint64_t)k;
        const uint64_t a0 = base + r * stride;
        const u32x4 en = e[k + 1], ep = e[k];
        const uint32_t off[3] = {en.x & 0xffffu, en.x >> 16, en.y & 0xffffu};
        const uint32_t poff[3] = {ep.x & 0xffffu, ep.x >> 16, ep.y & 0xffffu};
        d[k] = SegRule{SEGRULE_2B, SEGRULE_2B};
        if ((uint32_t)k < cnt)
            d[k] = seg_rule((uint32_t)(a0 & 63u), len, stride, off, r != 0 ? segrule_field_end(poff) : SEGRULE_NO_PREV, a0 - base,
                            total - (a0 - base));
        xa[k] = xb[k] = u32x4{0u, 0u, 0u, 0u};
        if (d[k].a != SEGRULE_2B) {
            xa[k] = *(const GMEM u32x4*)(a0 + (int64_t)d[k].a + 16 * l);
            if (d[k].b != d[k].a) xb[k] = *(const GMEM u32x4*)(a0 + (int64_t)d[k].b + 16 * l);
        }
    }

    // ---- patch, store ----
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if ((uint32_t)k >= cnt) break;
        const uint64_t r = r0 + (uint64_t)k;
        const uint64_t a0 = base + r * stride;
        const u32x4 en = e[k + 1];
        const uint32_t off[3] = {en.x & 0xffffu, en.x >> 16, en.y & 0xffffu};
        const uint32_t val[3] = {en.y >> 16, en.z & 0xffffu, en.z >> 16};
        if (p.status && l == 0) ((gu8)p.status)[r] = (uint8_t)en.w;
        if (d[k].a == SEGRULE_2B) {
            if (l == 0) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (off[i] != SEGRULE_NO_FIELD) store_be16((gu8)a0 + off[i], val[i]);
            }
            continue;
        }
        // this lane's 16 bytes of a segment with the field bytes that fall into them patched in
        // (selects, no branches: byte q of the lane's 16 is byte q % 4 of word q / 4)
        auto patch = [&](u32x4 x, uint64_t w) {
            uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // the byte's index in the lane's 16 (past 15 when it lies before or after them)
                    const uint32_t q = off[i] == SEGRULE_NO_FIELD ? 16u : (uint32_t)(a0 + off[i] + (uint32_t)j - w);
                    const uint32_t sh = 8u * (q & 3u);
                    const uint32_t by = (j ? val[i] : val[i] >> 8) & 0xffu;
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c) xs[c] = (q >> 2) == c ? (xs[c] & ~(0xffu << sh)) | (by << sh) : xs[c];
                }
            }
            return u32x4{xs[0], xs[1], xs[2], xs[3]};
        };
        const uint64_t wa = a0 + (int64_t)d[k].a + 16 * l, wb = a0 + (int64_t)d[k].b + 16 * l;
        const u32x4 ya = patch(xa[k], wa);
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(wa), "v"(ya) : "memory");
        if (d[k].b != d[k].a) {
            const u32x4 yb = patch(xb[k], wb);
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(wb), "v"(yb) : "memory");
        }
    }
}

hipError_t launch_seg_pass_fields(const KParams& p, hipStream_t s) {
    if (!p.fields || p.desc || p.n == 0) return hipErrorInvalidValue;
    const uint64_t blocks = (p.n + segpass::PER_BLOCK - 1) / segpass::PER_BLOCK;
    if (blocks > kMaxGridBlocks) return hipErrorInvalidValue;  // (a chunk of the route is far smaller)
    hipLaunchKernelGGL(seg_pass_fields_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace smolcsum
