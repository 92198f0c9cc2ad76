// Verify + delivery of UDP datagrams into their sockets' receive buffers
// (smol_csum_batch_verify_udp_enqueue, include/smolcsum.h): tcpasm_kernel's pass over a record (csum_tcpasm.hip)
// with the destination taken from the socket's PacketBuffer, one workgroup per socket.
//
// On receive the reference sums a datagram in UdpRepr::parse (src/wire/udp.rs:250-257), and UdpSocket::process
// then asks rx_buffer.enqueue(size, metadata) for a place and copies the payload there
// (src/socket/udp.rs:492-529, src/storage/packet_buffer.rs:80-118): two passes over the payload.  The place
// depends on the sizes of every datagram the socket took earlier in the poll, and those on their verdicts.
//
// One 256-thread workgroup per group (tcpasm_kernel's shape, csum_fraggroup.h's group_valid, lds_sync and wave
// reductions), grid-stride over groups; record j goes to wave j mod 4.
//   0. Header pre-pass.  The wave loads the 128-B window of each of its records, eight records at a time (eight
//      lanes a record), parse_geometry<false> parses it, and the record's candidate bit, size, payload offset,
//      addresses and source port go to LDS.  After a barrier thread 0 runs the enqueue rule (csum_pktbuf.h)
//      over ALL candidates in order: the speculative layout, every record's speculative ring_off in LDS.  At
//      most 256 serial iterations, all in LDS.
//   1. The wave streams each of its records once, with csum_deliver.h's pieces for G = 64 (load_step,
//      Record::parse, sum_step, store_step, finish): every 16-B chunk is loaded once and summed as verify sums
//      it; for a candidate the speculative layout enqueues the same registers are stored to its speculative
//      place, one Dest.  The copy waits for no verdict.  finish_gates (MODE_VERIFY) writes
//      the status byte and leaves it in LDS.
//   2. Barrier.  Thread 0 runs the rule again over the ACCEPTED candidates: the accepted layout, every record's
//      final place, flags and meta_idx, the PADDING entries and the group entry.  An ENQUEUED record with
//      len > 0 is RESTORED when step 1 did not store it or its final place differs from its speculative one.
//   3. Only when something is RESTORED (a value every thread reads from LDS): an agent-scope release fence in
//      front of a barrier completes step 1's stores, then the waves stream those records again, copy only.
//   4. Thread j writes record j's entry and, for an ENQUEUED record, its PACKET metadata entry.
//
// Why a record that kept its place is never clobbered.  One run of the rule hands out pairwise disjoint
// ranges of the ring's free space, so speculative ranges are pairwise disjoint and so are accepted ranges.
// Let B be ENQUEUED and not RESTORED: step 1 stored it and its accepted range IS its speculative range.  Every
// other store of step 1 goes to another record's speculative range, disjoint from B's speculative range.
// Every store of step 3 goes to another record's accepted range, disjoint from B's accepted range.  A
// RESTORED record's range is written in step 3, after every store of step 1 is complete (the fence and the
// barrier), and only step-3 stores of other accepted ranges follow, which are disjoint from it.  Bytes that
// lie in a speculative range and in no accepted range may keep a speculative byte: they are free ring space.
// Occupied bytes and padding are in no range of either layout.
//
// Every barrier is reached by all 256 threads: an invalid group is skipped by the whole workgroup before the
// first one, and the restore barrier is taken on a value every thread reads from LDS.
#include "csum_deliver.h"
#include "csum_fraggroup.h"
#include "csum_pktbuf.h"

namespace smolcsum {
namespace udprx {

using namespace deliver;
using namespace fraggroup;

// Chunks per lane and step: tcpasm_kernel's U = 1 (the kernel is bound by the latency of a record's chain,
// so resident waves count for more than a frame in one step).  A 1514-B frame is two steps.
constexpr int U = 1;
constexpr uint32_t STEP = 64 * U;
constexpr uint32_t MAXD = SMOL_MAX_SOCKET_DGRAMS;
constexpr uint32_t PRE = 8;  // records a wave parses at a time in the header pre-pass: 8 lanes each
constexpr uint32_t NONE = ~0u;  // s_size: no candidate; s_spec: the speculative layout does not enqueue it
static_assert(MAXD <= 256 && MAXD == MAXF, "thread j holds record j; group_valid's bound");
static_assert(sizeof(smol_csum_udpsock_t) == 48 && sizeof(smol_csum_udpmeta_t) == 48 && sizeof(smol_csum_udprx_t) == 16 &&
                  sizeof(smol_csum_udpsockout_t) == 32,
              "entry layouts");

template <bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void udprx_kernel(
    KParams p, const smol_csum_frag_group_t* groups, uint64_t ngroups, UdpRxArgs v) {
    __shared__ u32x4 win[4][WIN_CH];
    __shared__ u32x4 pre[4][PRE][WIN_CH + 1];  // the pre-pass's windows, 144 B apart: slot i's dwords start at bank 4 i
    __shared__ Geom geo[4];
    // record j of the group: its size (NONE: no candidate), payload offset | source port << 16, family, the
    // address words of its IP header (source first), speculative and final ring_off, metadata index, SMOL_URX_*
    // and status byte
    __shared__ uint32_t s_size[MAXD], s_offp[MAXD], s_addr[MAXD][8], s_spec[MAXD], s_ring[MAXD], s_midx[MAXD], s_stat[MAXD];
    __shared__ uint8_t s_fam[MAXD], s_fl[MAXD];
    __shared__ uint32_t s_nrest;
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
        const uint64_t first = groups[gi].first;
        const uint32_t count = groups[gi].count;
        const u32x4 k0 = *(gcv4)((uint64_t)v.socks + 48ull * gi);        // dst_offset, meta_first
        const u32x4 k1 = *(gcv4)((uint64_t)v.socks + 48ull * gi + 16u);  // payload_cap, _read, _len, meta_cap
        const u32x4 k2 = *(gcv4)((uint64_t)v.socks + 48ull * gi + 32u);  // meta_read, meta_len, port | reserved
        const uint32_t P = k1.x, M = k1.w, port = k2.z & 0xffffu;
        const PktBufState s0 = {k1.y, k1.z, k2.x, k2.y};
        const bool sock_ok = (k2.z >> 16) == 0 && k2.w == 0 && pktbuf_state_valid(P, M, s0);
        // an invalid group: its entry, indexed by group, is zero.  The whole workgroup leaves here.
        if (!group_valid(p, groups[gi]) || !sock_ok) {
            if (tid < 2) *(GMEM u32x4*)((uint64_t)v.out + 32ull * gi + 16u * tid) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }
        const uint64_t ring = (uint64_t)v.dst + ((uint64_t)k0.x | ((uint64_t)k0.y << 32));
        const uint64_t meta = (uint64_t)v.meta + 48ull * ((uint64_t)k0.z | ((uint64_t)k0.w << 32));

        // ---- 0. the header pre-pass: who is a candidate, and of what size ----
        // Eight of the wave's records at a time: lanes 8 i .. 8 i + 7 load record slot i's window, one chunk each,
        // and then all parse it (the same values in the eight lanes, no lane idle behind a branch), so a round
        // costs one load round trip and one parse for eight records.
        for (uint32_t j0 = wave; j0 < count; j0 += 4 * PRE) {
            const uint32_t slot = (uint32_t)lane >> 3, cl = (uint32_t)lane & 7u;
            const uint32_t j = j0 + 4 * slot;
            const bool have = j < count;
            const RecRef rr = rec_at<IMPLICIT, false>(p, first + (have ? j : j0));
            const uint64_t base = rr.a0 & ~15ull;
            const uint32_t head = (uint32_t)(rr.a0 - base);
            const uint32_t nch = n_chunks<false>(rr);
            u32x4* w8 = &pre[wave][slot][0];
            const uint8_t* wb = reinterpret_cast<const uint8_t*>(w8);
            if (have && cl < nch) w8[cl] = ld16<false>((gcv4)(base + 16ull * cl));
            wave_lds_sync();
            if (have) {
                auto rd = [&](uint32_t o) -> uint32_t {
                    const uint32_t x = head + o;
                    if (x < (uint32_t)WIN) return (uint32_t)wb[x];
                    return ld_byte_sync(rr.a0 + o);
                };
                const Geom g = parse_geometry<false>(rd, rr.len, rr.kind, false);
                // the UDP payload span (verify_copy's rule: UdpPacket::payload, udp.rs:153-157) and the port half
                // of UdpSocket::accepts
                bool cand = !(g.st & (SMOL_ST_MALFORMED | SMOL_ST_UNSUPPORTED)) && g.proto == P_UDP;
                if (cand) cand = (rd(g.l4_off + 2) << 8 | rd(g.l4_off + 3)) == port;
                if (cand) {
                    const uint32_t off = g.l4_off + 8;
                    if (cl == 0) {
                        s_size[j] = g.span_end - off;
                        s_offp[j] = (off & 0xffffu) | (rd(g.l4_off) << 8 | rd(g.l4_off + 1)) << 16;
                        s_fam[j] = (uint8_t)g.fam;
                    }
                    if (cl < g.addr_words / 2) {  // (the addresses lie inside the window: addr_off <= 26)
                        const uint32_t o = head + g.addr_off + 4u * cl;
                        s_addr[j][cl] = (uint32_t)wb[o] | (uint32_t)wb[o + 1] << 8 | (uint32_t)wb[o + 2] << 16 | (uint32_t)wb[o + 3] << 24;
                    }
                } else if (cl == 0) {
                    s_size[j] = NONE;
                }
            }
            wave_lds_sync();  // the windows are rewritten by the wave's next round
        }
        lds_sync();  // (all threads) every record's candidate bit and size
        if (tid == 0) {  // the speculative layout: the rule over all candidates
            PktBufState s = s0;
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t size = s_size[j];
                uint32_t at = NONE;
                if (size != NONE) {
                    const PktBufStep e = pktbuf_enqueue(P, M, s, size);
                    if (e.res & PKTBUF_OK) at = e.ring_off;
                }
                s_spec[j] = at;
            }
        }
        lds_sync();  // (all threads)

        // ---- 1. one pass over the wave's records: the status byte, and the speculative delivery ----
        for (uint32_t j = wave; j < count; j += 4) {
            const uint64_t r = first + j;
            const Record rec(rec_at<IMPLICIT, false>(p, r), &win[wave][0], geo[wave]);
            const uint32_t nch = rec.nch;
            const uint32_t size = s_size[j], spec = s_spec[j];
            const bool st = size != NONE && size > 0 && spec != NONE;  // (wave-uniform)

            u32x4 c[U], xh;
            load_step<64, U>(rec.base, nch, 0u, st, lane, dummy, c, xh);
            const int s1 = rec.parse<64, U>(c, lane);
            const Dest q = dest_of(rec.rr.a0, rec.head, st ? s_offp[j] & 0xffffu : 0u, ring + (st ? spec : 0u), st ? size : 0u);

            uint32_t acc = 0;
            for (uint32_t i0 = 0; i0 < nch; i0 += STEP) {
                if (i0) load_step<64, U>(rec.base, nch, i0, st, lane, dummy, c, xh);
                acc = sum_step<64, U>(c, i0, rec, s1, lane, acc);
                if (st) store_step<64, U>(c, xh, i0, nch, lane, q);
            }

            finish<64>(p, rec, acc, r, lane, &s_stat[j]);
            wave_lds_sync();  // the window is rewritten by the wave's next record
        }
        lds_sync();  // (all threads, whatever the group streamed) every record's verdict

        // ---- 2. the accepted layout: the rule over the accepted candidates ----
        if (tid == 0) {
            PktBufState s = s0;
            uint32_t n_enq = 0, n_full = 0, n_rest = 0;
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t size = s_size[j];
                uint32_t fl = 0, at = 0, mi = 0;
                if (size != NONE) {
                    fl = SMOL_URX_UDP;
                    if (s_stat[j] & SMOL_ST_ACCEPT) {
                        const PktBufStep e = pktbuf_enqueue(P, M, s, size);
                        if (e.res & PKTBUF_PADDED) {  // smol_csum_udpmeta_t: size, and kind in byte 11
                            const uint64_t a = meta + 48ull * e.pad_idx;
                            *(GMEM u32x4*)a = u32x4{e.pad_size, 0u, SMOL_UMETA_PADDING << 24, 0u};
                            *(GMEM u32x4*)(a + 16u) = u32x4{0u, 0u, 0u, 0u};
                            *(GMEM u32x4*)(a + 32u) = u32x4{0u, 0u, 0u, 0u};
                            fl |= SMOL_URX_PADDED;
                        }
                        if (e.res & PKTBUF_OK) {
                            fl |= SMOL_URX_ENQUEUED;
                            at = e.ring_off;
                            mi = e.meta_idx;
                            ++n_enq;
                            if (size > 0 && s_spec[j] != at) {  // (not stored in step 1: s_spec is NONE)
                                fl |= SMOL_URX_RESTORED;
                                ++n_rest;
                            }
                        } else {
                            fl |= SMOL_URX_FULL;
                            ++n_full;
                        }
                    }
                }
                s_fl[j] = (uint8_t)fl;
                s_ring[j] = at;
                s_midx[j] = mi;
            }
            s_nrest = n_rest;
            // smol_csum_udpsockout_t: the state after the poll, the counts, valid | reserved
            *(GMEM u32x4*)((uint64_t)v.out + 32ull * gi) = u32x4{s.pr, s.pl, s.mr, s.ml};
            *(GMEM u32x4*)((uint64_t)v.out + 32ull * gi + 16u) = u32x4{n_enq, n_full, n_rest, 1u};
        }
        lds_sync();  // (all threads)

        // ---- 3. restore: the enqueued records whose final place step 1 did not fill, copy only ----
        if (s_nrest) {  // (the same value in every thread)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the first pass's stores are complete ...
            __syncthreads();                                    // ... in every wave, before the second ones issue
            for (uint32_t j = wave; j < count; j += 4) {
                if (!(s_fl[j] & SMOL_URX_RESTORED)) continue;
                const Record rec(rec_at<IMPLICIT, false>(p, first + j), &win[wave][0], geo[wave]);  // (its grid only)
                const Dest q = dest_of(rec.rr.a0, rec.head, s_offp[j] & 0xffffu, ring + s_ring[j], s_size[j]);
                for (uint32_t i0 = 0; i0 < rec.nch; i0 += STEP) {
                    u32x4 c[U], xh;
                    load_step<64, U>(rec.base, rec.nch, i0, true, lane, dummy, c, xh);
                    store_step<64, U>(c, xh, i0, rec.nch, lane, q);
                }
            }
        }

        // ---- 4. the record entries and the PACKET metadata entries ----
        if (tid < count) {
            const uint32_t size = s_size[tid], fl = s_fl[tid];
            u32x4 e = {0u, 0u, 0u, 0u};  // smol_csum_udprx_t: ring_off, len, meta_idx, off | flags | reserved
            if (size != NONE) e = u32x4{s_ring[tid], size, s_midx[tid], (s_offp[tid] & 0xffffu) | fl << 16};
            *(GMEM u32x4*)((uint64_t)v.rx + 16ull * (first + tid)) = e;
            if (fl & SMOL_URX_ENQUEUED) {
                // smol_csum_udpmeta_t: size, record, src_port | family | kind, reserved; remote_addr; local_addr
                const uint64_t a = meta + 48ull * s_midx[tid];
                const uint32_t fam = s_fam[tid];
                const uint32_t* w = s_addr[tid];
                *(GMEM u32x4*)a = u32x4{size, (uint32_t)(first + tid), (s_offp[tid] >> 16) | fam << 16 | SMOL_UMETA_PACKET << 24, 0u};
                if (fam == 4) {
                    *(GMEM u32x4*)(a + 16u) = u32x4{w[0], 0u, 0u, 0u};
                    *(GMEM u32x4*)(a + 32u) = u32x4{w[1], 0u, 0u, 0u};
                } else {
                    *(GMEM u32x4*)(a + 16u) = u32x4{w[0], w[1], w[2], w[3]};
                    *(GMEM u32x4*)(a + 32u) = u32x4{w[4], w[5], w[6], w[7]};
                }
            }
        }
        lds_sync();  // (all threads) the next group's records rewrite the arrays
    }
}

}  // namespace udprx

hipError_t launch_udprx(const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups, const UdpRxArgs& v,
                        uint32_t max_blocks, hipStream_t s) {
    const uint32_t blocks = grid_blocks(ngroups, max_blocks);
    note_launch(KERN_UDPRX, 0, 64, udprx::U);
    if (p.desc == nullptr) hipLaunchKernelGGL((udprx::udprx_kernel<true>), dim3(blocks), dim3(256), 0, s, p, groups, ngroups, v);
    else hipLaunchKernelGGL((udprx::udprx_kernel<false>), dim3(blocks), dim3(256), 0, s, p, groups, ngroups, v);
    return hipGetLastError();
}

}  // namespace smolcsum
