// Verify + reassembly of IPv4 fragment groups (smol_csum_batch_verify_reassemble, include/smolcsum.h):
// frag_kernel's verify (csum_frag.hip) with every fragment's payload delivered to its place in the
// datagram's slot of d_dst in the same pass.
//
// On receive the reference reads a fragmented datagram twice: PacketAssembler::add copies every
// fragment's payload into the assembler's buffer (src/iface/fragmentation.rs:139-151, called from
// src/iface/interface/ipv4.rs:131), and once assemble() returns the payload the L4 Repr::parse sums all
// of it (udp.rs:250-257, tcp.rs:917-919, icmpv4.rs:404-407).  Here every 16-B chunk of a payload is
// loaded once: the registers are summed as frag_kernel sums them and the same registers feed the
// stores.
//
// One 256-thread workgroup per group.
//   1.-3. csum_fraggroup.h's, as in frag_kernel: thread j parses fragment j's IPv4 header into the
//      datagram map in LDS, the workgroup checks the group contract, and the L4 header is read through
//      the map.  The wave reductions of frag_kernel become workgroup reductions: per-wave values meet
//      in LDS.
//   4. the fragments are dealt to the four wavefronts (fragment j to wave j mod 4).  A wavefront
//      streams its fragment as a vcopy::Piece (csum_walk.h), U chunks per lane and step, all loads of a
//      step issued first, and the first step of its NEXT fragment is issued before the current one is
//      used, so a lane has up to 2 U chunks (and the two successor chunks) in flight.
//      * Sum: each chunk as frag_kernel sums it (edges masked, UDP capped at span_end); a fragment's sum
//        becomes its data() value, the wave adds those up, and the four waves' values meet in LDS:
//        the one's-complement sum does not depend on the order, so the verdict is verify_frag's.
//      * Copy: the piece's destination is the fragment's place in the slot.  Two fragments of a
//        datagram meet at a multiple of 8, inside a destination chunk that two wavefronts write: each
//        writes its bytes of it (store_edge).  No byte of d_dst is read.
//   5. thread j writes fragment j's status byte (frag_kernel's), thread 0 the group's smol_csum_dgram_t.
// The cap is tested before the first store: a group that does not fit still streams for its status.
// The copy waits for no verdict, neither the L4 checksum's nor a fragment header's.
//
// Every barrier is reached by all 256 threads: an invalid group is skipped by the whole workgroup
// before the first one, and broken / raw / unsupported / too-large groups take every barrier with
// nothing to stream.
#include "csum_fraggroup.h"

namespace smolcsum {
namespace fragcopy {

using namespace fraggroup;
using Piece = vcopy::Piece<true>;  // a group over its cap is summed, not delivered

constexpr int U = 2;           // chunks per lane and step: a 1480-B fragment is one step
constexpr uint32_t STEP = 64 * U;
static_assert(MAXF <= 256, "thread j parses fragment j");

template <bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void fragcopy_kernel(
    KParams p, const smol_csum_frag_group_t* groups, uint64_t ngroups, FragCopyArgs v) {
    __shared__ uint64_t s_addr[MAXF];  // the datagram map (DgMap)
    __shared__ uint32_t s_start[MAXF], s_end[MAXF];
    __shared__ uint8_t s_bits[MAXF];
    // the four waves' values of each workgroup reduction (one array per reduction: no reuse inside a group)
    __shared__ uint32_t s_r1[4][6], s_r2[4][2], s_r4[4];
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
        const uint64_t first = groups[gi].first;
        const uint32_t count = groups[gi].count;
        // an invalid group: its entry, indexed by group, is zero.  The whole workgroup leaves here.
        if (!group_valid(p, groups[gi])) {
            if (tid == 0) *(GMEM u32x4*)((uint64_t)v.dgrams + 16ull * gi) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }

        // ---- 1. the fragments' IPv4 headers ----
        const Key k0 = group_key<IMPLICIT>(p, first);
        bool bad = !k0.ok, raw = false, ip_drop = false;
        uint32_t T = 0, sumlen = 0, lastn = 0;
        if (tid < count) {
            const FragHdr h = frag_header<false, IMPLICIT>(p, first + tid, k0);
            raw = h.raw;
            bad = bad || h.bad;
            T = h.T;
            sumlen = h.sumlen;
            lastn = h.lastn;
            ip_drop = !(h.bits & 4u);
            s_addr[tid] = h.addr;
            s_start[tid] = h.start;
            s_end[tid] = h.end;
            s_bits[tid] = (uint8_t)h.bits;
        }
        {
            const uint32_t wT = wave_max(T), wS = wave_sum(sumlen), wL = wave_sum(lastn);
            const bool wB = wave_any(bad), wR = wave_any(raw), wI = wave_any(ip_drop);
            if (lane == 0) {
                s_r1[wave][0] = wT;
                s_r1[wave][1] = wS;
                s_r1[wave][2] = wL;
                s_r1[wave][3] = wB;
                s_r1[wave][4] = wR;
                s_r1[wave][5] = wI;
            }
        }
        lds_sync();  // (all threads) the map and the first reduction
        T = max(max(s_r1[0][0], s_r1[1][0]), max(s_r1[2][0], s_r1[3][0]));
        sumlen = s_r1[0][1] + s_r1[1][1] + s_r1[2][1] + s_r1[3][1];
        lastn = s_r1[0][2] + s_r1[1][2] + s_r1[2][2] + s_r1[3][2];
        bad = (s_r1[0][3] | s_r1[1][3] | s_r1[2][3] | s_r1[3][3]) != 0;
        raw = (s_r1[0][4] | s_r1[1][4] | s_r1[2][4] | s_r1[3][4]) != 0;
        const bool all_ip = (s_r1[0][5] | s_r1[1][5] | s_r1[2][5] | s_r1[3][5]) == 0;

        // ---- 2. the group contract ----
        const DgMap map = {s_addr, s_start, s_end, s_bits, count, dummy};
        bool broken = bad || lastn != 1 || sumlen != T;
        {
            Row row = {false, 0u};
            if (!broken && tid < count) row = contract_row(map, tid, T);
            const bool wB = wave_any(row.broken);
            const uint32_t wZ = wave_sum(row.zero);
            if (lane == 0) {
                s_r2[wave][0] = wB;
                s_r2[wave][1] = wZ;
            }
        }
        lds_sync();  // (all threads)
        broken = broken || (s_r2[0][0] | s_r2[1][0] | s_r2[2][0] | s_r2[3][0]) != 0 ||
                 s_r2[0][1] + s_r2[1][1] + s_r2[2][1] + s_r2[3][1] != 1;

        // ---- 3. the L4 header through the datagram map (every thread: the values are the workgroup's) ----
        const L4Hdr l4 = l4_header<false>(map, k0, broken, raw, T);
        const uint32_t span_end = l4.span_end;

        // ---- 4. one pass over the payloads: data() per fragment slice, and the delivery ----
        const u32x4 sl = *(gcv4)((uint64_t)v.slots + 16ull * gi);  // dst_offset, cap, reserved
        const bool do_sum = l4.proto != P_NONE;
        const bool do_copy = !broken && T <= sl.z;  // the cap test, before the first store
        const uint64_t Dslot = (uint64_t)v.dst + ((uint64_t)sl.x | ((uint64_t)sl.y << 32));

        auto setup = [&](uint32_t j) -> Piece {
            const uint32_t lo = s_start[j], hi = s_end[j];
            const uint32_t he = min(hi, span_end);
            return Piece(s_addr[j], Dslot + lo, do_sum && he > lo ? he - lo : 0u, do_copy ? hi - lo : 0u);
        };

        uint32_t Dw = 0;  // the wave's sum of data() values
        if (do_sum || do_copy) {
            uint32_t j = wave;
            Piece cur = {};
            u32x4 c[U], xh;
            if (j < count) {
                cur = setup(j);
                vcopy::piece_load<U>(cur, 0u, lane, dummy, c, xh);
            }
            while (j < count) {
                const uint32_t jn = j + 4;
                Piece nxt = {};
                u32x4 cn[U], xn;
                if (jn < count) {  // the next fragment's first step, in flight under this one's work
                    nxt = setup(jn);
                    vcopy::piece_load<U>(nxt, 0u, lane, dummy, cn, xn);
                }
                uint32_t acc = 0;
                vcopy::piece_use<U>(cur, 0u, lane, c, xh, acc, vcopy::NoHold{});
                for (uint32_t i0 = STEP; i0 < cur.nk; i0 += STEP) {
                    vcopy::piece_load<U>(cur, i0, lane, dummy, c, xh);
                    vcopy::piece_use<U>(cur, i0, lane, c, xh, acc, vcopy::NoHold{});
                }
                if (cur.sum_len) {
                    const uint32_t S = fold32(wave_sum(acc));
                    Dw += cur.odd() ? S : bswap16(S);  // data() of the slice (csum_device.h)
                }
                cur = nxt;
#pragma unroll
                for (int u = 0; u < U; ++u) c[u] = cn[u];
                xh = xn;
                j = jn;
            }
        }
        if (lane == 0) s_r4[wave] = Dw;
        lds_sync();  // (all threads, whatever the group streamed)

        Verdict verdict = {1, 1, 0};
        if (do_sum) {
            const uint32_t dat = fold32(s_r4[0] + s_r4[1] + s_r4[2] + s_r4[3]);
            verdict = l4_verdict(l4_sum(p, k0, l4, T, dat), l4.proto, map.byte(l4.fo) << 8 | map.byte(l4.fo + 1));
        }

        // ---- 5. status bytes (frag_kernel's) and the datagram entry ----
        if (tid < count) ((gu8)p.status)[first + tid] = (uint8_t)frag_status<false>(s_bits[tid], l4.st, verdict, all_ip);
        if (tid == 0) {  // smol_csum_dgram_t: len, l4_len, l4_off | protocol | copied, reserved
            u32x4 e = {0u, 0u, 0u, 0u};
            if (!broken) {
                e.x = T;
                e.y = l4.l4_len;
                e.z = l4.l4_off | (l4.key_proto << 16) | ((do_copy ? 1u : 0u) << 24);
            }
            *(GMEM u32x4*)((uint64_t)v.dgrams + 16ull * gi) = e;
        }
        lds_sync();  // (all threads) the next group's phase 1 rewrites the map
    }
}

}  // namespace fragcopy

hipError_t launch_fragcopy(const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups,
                           const FragCopyArgs& v, hipStream_t s) {
    const uint32_t blocks = grid_blocks(ngroups, kMaxGridBlocks);
    note_launch(KERN_FRAGCOPY, 0, 64, fragcopy::U);
    if (p.desc == nullptr) hipLaunchKernelGGL((fragcopy::fragcopy_kernel<true>), dim3(blocks), dim3(256), 0, s, p, groups, ngroups, v);
    else hipLaunchKernelGGL((fragcopy::fragcopy_kernel<false>), dim3(blocks), dim3(256), 0, s, p, groups, ngroups, v);
    return hipGetLastError();
}

}  // namespace smolcsum
