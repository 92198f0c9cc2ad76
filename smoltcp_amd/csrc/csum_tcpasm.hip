// Verify + delivery of TCP segments into their connections' receive rings
// (smol_csum_batch_verify_tcp_assemble, include/smolcsum.h): vcopy_kernel's pass over a record (csum_vcopy.hip)
// with the destination taken from the segment's own sequence number, one workgroup per connection.
//
// On receive the reference sums a segment in TcpRepr::parse (src/wire/tcp.rs:917-919), and
// TcpSocket::process then tests it against the receive window, trims it and copies it into the ring
// (src/socket/tcp.rs:1705-1783, 2205-2241; rx_buffer.write_unallocated, src/storage/ring_buffer.rs:321-338):
// two passes over the payload, and the place is known only from the header.  Here every 16-B chunk of a
// frame is loaded once; the registers are summed as verify sums them and the same registers feed the stores.
//
// One 256-thread workgroup per group (fragcopy_kernel's shape, csum_fraggroup.h's group_valid, lds_sync and
// wave reductions), grid-stride over groups.
//   1. Record j goes to wave j mod 4.  The wave streams it with csum_deliver.h's pieces for G = 64 (load_step,
//      Record::parse, sum_step, store_step, finish): step 0's 128-B header window goes to the wave's LDS
//      window, parse_geometry<false> parses it, every chunk is loaded once and summed once, finish_gates
//      (MODE_VERIFY) writes the status byte and leaves it in LDS.  This file's own: the delivered range is the
//      payload trimmed to the window (csum_tcpwin.h), and the destination is one or two pieces of the ring, so
//      a record is stored into two Dests from the same registers, each piece with its own funnel shift (the
//      second is empty unless the range wraps).  The copy waits for no verdict.
//   2. Barrier (all threads, whatever the group streamed).  Thread j holds record j's window range and class
//      (delivered, counted) from LDS and scans the group's ranges once: a counted record that meets a
//      delivered, not counted one is redelivered; contig_len is the smallest of 0 and the counted ends that
//      no counted range continues (start <= x < end), which is where the union's front stops.  One workgroup
//      reduction, whatever the count.
//   3. When anything is redelivered: an agent-scope release fence in front of a barrier completes the first
//      pass's stores, then the waves stream those records again, copy only.
//   4. Thread j writes record j's segment entry, thread 0 the flow entry.
//
// Every barrier is reached by all 256 threads: an invalid group is skipped by the whole workgroup before the
// first one, and the redelivery barrier is taken on a value every thread reads from LDS.
#include "csum_deliver.h"
#include "csum_fraggroup.h"
#include "csum_tcpwin.h"

namespace smolcsum {
namespace tcpasm {

using namespace deliver;
using namespace fraggroup;

// Chunks per lane and step.  The kernel is bound by the latency of a record's chain (load, parse, rule, sum,
// gates), one record per wave at a time, so resident waves count for more than a frame in one step: U = 1
// compiles to 72 VGPRs and 7 waves per SIMD with no scratch, U = 2 to 103 VGPRs and 4 waves, which took 1.3 to
// 1.6 times as long.  A 1514-B frame is two steps.
constexpr int U = 1;
constexpr uint32_t STEP = 64 * U;
constexpr uint32_t MAXS = SMOL_MAX_FLOW_SEGMENTS;
static_assert(MAXS <= 256, "thread j holds record j");
static_assert(sizeof(smol_csum_tcpwin_t) == 32 && sizeof(smol_csum_tcpseg_t) == 16 && sizeof(smol_csum_tcpflow_t) == 16,
              "entry layouts");

// a record's class in the group phase
constexpr uint32_t CLS_NONE = 0, CLS_DELIVERED = 1, CLS_COUNTED = 2;

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}

// The ring pieces of a record's delivered range, which starts at record offset src.
struct Pieces {
    Dest a, b;
};
__device__ __forceinline__ Pieces pieces_of(const TcpWinRule& w, uint64_t ring, uint64_t a0, uint32_t head, uint32_t src) {
    Pieces q;
    q.a = dest_of(a0, head, src, ring + w.pos0, w.len0);
    q.b = dest_of(a0, head, src + w.len0, ring, w.len1);
    return q;
}

template <bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void tcpasm_kernel(
    KParams p, const smol_csum_frag_group_t* groups, uint64_t ngroups, TcpAsmArgs v) {
    __shared__ u32x4 win[4][WIN_CH];
    __shared__ Geom geo[4];
    // record j of the group: its sequence number, window range, first delivered byte's record offset,
    // payload offset | SMOL_SEG_* << 16, status byte and class
    __shared__ uint32_t s_seq[MAXS], s_woff[MAXS], s_len[MAXS], s_src[MAXS], s_info[MAXS], s_stat[MAXS];
    __shared__ uint8_t s_cls[MAXS];
    __shared__ uint32_t s_red[4][4];  // the four waves' values of the group reduction
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
        const uint64_t first = groups[gi].first;
        const uint32_t count = groups[gi].count;
        const u32x4 w0 = *(gcv4)((uint64_t)v.wins + 32ull * gi);        // dst_offset, ring_len, ring_pos
        const u32x4 w1 = *(gcv4)((uint64_t)v.wins + 32ull * gi + 16u);  // window_start, window_len, reserved
        const uint32_t ring_len = w0.z, ring_pos = w0.w, wstart = w1.x, wlen = w1.y;
        const bool win_ok = (w1.z | w1.w) == 0 && wlen <= ring_len && (ring_len ? ring_pos < ring_len : ring_pos == 0);
        // an invalid group: its entry, indexed by group, is zero.  The whole workgroup leaves here.
        if (!group_valid(p, groups[gi]) || !win_ok) {
            if (tid == 0) *(GMEM u32x4*)((uint64_t)v.flows + 16ull * gi) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }
        const uint64_t ring = (uint64_t)v.dst + ((uint64_t)w0.x | ((uint64_t)w0.y << 32));

        // ---- 1. one pass over the wave's records: the status byte, and the delivery ----
        // (Issuing the first step of the wave's NEXT record before the current one is used, as fragcopy_kernel
        // does, measured no faster with U = 2 and spilled: 1.4461 ms against 1.4449 on 2^14 flows of 45,
        // DESIGN.md §6.)
        for (uint32_t j = wave; j < count; j += 4) {
            const uint64_t r = first + j;
            const Record rec(rec_at<IMPLICIT, false>(p, r), &win[wave][0], geo[wave]);
            const uint32_t nch = rec.nch;

            u32x4 c[U], xh;
            load_step<64, U>(rec.base, nch, 0u, true, lane, dummy, c, xh);
            const int s1 = rec.parse<64, U>(c, lane);
            const Geom& g = rec.g;

            // the TCP payload span (verify_copy's rule), the window rule and the ring pieces
            uint32_t off = 0, seq = 0, fl = 0;
            TcpWinRule w = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
            if (!(g.st & (SMOL_ST_MALFORMED | SMOL_ST_UNSUPPORTED)) && g.proto == P_TCP) {
                const uint32_t thl = (rec.rd(g.l4_off + 12) >> 4) * 4;
                off = g.l4_off + thl;
                seq = rec.rd(g.l4_off + 4) << 24 | rec.rd(g.l4_off + 5) << 16 | rec.rd(g.l4_off + 6) << 8 | rec.rd(g.l4_off + 7);
                const bool syn_rst = (rec.rd(g.l4_off + 13) & 0x06u) != 0;
                w = tcpwin_rule(seq, g.l4_len - thl, wstart, wlen, ring_pos, ring_len);
                fl = SMOL_SEG_TCP | (w.in_window ? SMOL_SEG_IN_WINDOW : 0u) | (w.in_window && !syn_rst ? SMOL_SEG_COPIED : 0u);
            }
            const bool st = (fl & SMOL_SEG_COPIED) && w.len > 0;  // (wave-uniform)
            const Pieces q = pieces_of(w, ring, rec.rr.a0, rec.head, off + w.trim);

            uint32_t acc = 0;
            for (uint32_t i0 = 0; i0 < nch; i0 += STEP) {
                if (i0) load_step<64, U>(rec.base, nch, i0, st, lane, dummy, c, xh);
                acc = sum_step<64, U>(c, i0, rec, s1, lane, acc);
                if (st) store_step<64, U>(c, xh, i0, nch, lane, q.a, q.b);
            }

            finish<64>(p, rec, acc, r, lane, &s_stat[j]);
            if (lane == 0) {
                s_seq[j] = seq;
                s_woff[j] = w.win_off;
                s_len[j] = w.len;
                s_src[j] = off + w.trim;
                s_info[j] = (off & 0xffffu) | fl << 16;
                s_cls[j] = (uint8_t)(!st ? CLS_NONE : (s_stat[j] & SMOL_ST_ACCEPT) ? CLS_COUNTED : CLS_DELIVERED);
            }
            wave_lds_sync();  // the window is rewritten by the wave's next record
        }
        lds_sync();  // (all threads, whatever the group streamed) every record's range, verdict and class

        // ---- 2. the group: who is redelivered, and how far the counted ranges reach from the front ----
        uint32_t wo = 0, end = 0, info = 0;
        bool counted = false, redel = false, ext = false, ext0 = false;
        if (tid < count) {
            wo = s_woff[tid];
            end = wo + s_len[tid];
            info = s_info[tid];
            counted = s_cls[tid] == CLS_COUNTED;
            for (uint32_t i = 0; i < count; ++i) {
                const uint32_t ci = s_cls[i];
                if (ci == CLS_NONE) continue;
                const uint32_t a = s_woff[i], b = a + s_len[i];
                if (ci == CLS_COUNTED) {
                    ext0 = ext0 || a == 0;
                    ext = ext || (a <= end && end < b);
                } else if (counted && a < end && wo < b) {
                    redel = true;
                }
            }
            if (redel) {
                info |= SMOL_SEG_REDELIVERED << 16;
                s_info[tid] = info;
            }
        }
        {
            const uint32_t wC = wave_sum(counted ? 1u : 0u), wR = wave_sum(redel ? 1u : 0u);
            const uint32_t wM = wave_min(counted && !ext ? end : ~0u);
            if (lane == 0) {
                s_red[wave][0] = wC;
                s_red[wave][1] = wR;
                s_red[wave][2] = wM;
                if (tid == 0) s_red[0][3] = ext0 ? 1u : 0u;  // (thread 0 always holds a record: count >= 1)
            }
        }
        lds_sync();  // (all threads)
        const uint32_t n_counted = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
        const uint32_t n_redel = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
        const uint32_t front = min(min(s_red[0][2], s_red[1][2]), min(s_red[2][2], s_red[3][2]));
        const uint32_t contig = s_red[0][3] ? front : 0u;

        // ---- 3. redelivery: the counted records that met a record that is not counted, copy only ----
        if (n_redel) {  // (the same value in every thread)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the first pass's stores are complete ...
            __syncthreads();                                    // ... in every wave, before the second ones issue
            for (uint32_t j = wave; j < count; j += 4) {
                if (!((s_info[j] >> 16) & SMOL_SEG_REDELIVERED)) continue;
                const Record rec(rec_at<IMPLICIT, false>(p, first + j), &win[wave][0], geo[wave]);  // (its grid only)
                TcpWinRule w = {1u, s_woff[j], s_len[j], 0u, 0u, 0u, 0u};
                tcpwin_split(w, ring_pos, ring_len);
                const Pieces q = pieces_of(w, ring, rec.rr.a0, rec.head, s_src[j]);
                for (uint32_t i0 = 0; i0 < rec.nch; i0 += STEP) {
                    u32x4 c[U], xh;
                    load_step<64, U>(rec.base, rec.nch, i0, true, lane, dummy, c, xh);
                    store_step<64, U>(c, xh, i0, rec.nch, lane, q.a, q.b);
                }
            }
        }

        // ---- 4. the segment entries and the flow entry ----
        if (tid < count) {  // smol_csum_tcpseg_t: seq, win_off, len, off | flags | reserved
            const u32x4 e = {s_seq[tid], wo, end - wo, info};
            *(GMEM u32x4*)((uint64_t)v.segs + 16ull * (first + tid)) = e;
        }
        if (tid == 0)  // smol_csum_tcpflow_t: contig_len, counted, redelivered, valid | reserved
            *(GMEM u32x4*)((uint64_t)v.flows + 16ull * gi) = u32x4{contig, n_counted, n_redel, 1u};
        lds_sync();  // (all threads) the next group's records rewrite the arrays
    }
}

}  // namespace tcpasm

hipError_t launch_tcpasm(const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups, const TcpAsmArgs& v,
                         uint32_t max_blocks, hipStream_t s) {
    const uint32_t blocks = grid_blocks(ngroups, max_blocks);
    note_launch(KERN_TCPASM, 0, 64, tcpasm::U);
    if (p.desc == nullptr) hipLaunchKernelGGL((tcpasm::tcpasm_kernel<true>), dim3(blocks), dim3(256), 0, s, p, groups, ngroups, v);
    else hipLaunchKernelGGL((tcpasm::tcpasm_kernel<false>), dim3(blocks), dim3(256), 0, s, p, groups, ngroups, v);
    return hipGetLastError();
}

}  // namespace smolcsum
