// IPv4 fragment groups: smol_csum_batch_emit_frag / smol_csum_batch_verify_frag (include/smolcsum.h).
//
// One wavefront per group of fragments.  What a group is, its contract, the L4 header through the
// datagram map, the gates and the status byte are csum_fraggroup.h's, shared with fragcopy_kernel; this
// file deals the fragments to the lanes, reduces over the wave, and sums:
//
//   1.-3. lane j takes fragments j, j + 64, ...; the group's values are wave reductions;
//   4. the 64 lanes sum each fragment's payload slice as aligned 16-byte chunks (v_sad_u16, the
//      bytes outside the slice and, on emit, the checksum fields masked), and every fragment's sum
//      becomes its data() value;
//   5. lane 0 writes the field bytes where the map puts them; every lane writes its fragments'
//      status bytes.
//
// This is the rare path (fragmented datagrams), written for exactness, not for the HBM roofline:
// one wavefront walks a datagram's fragments one after the other.
#include "csum_fraggroup.h"

namespace smolcsum {
namespace frag {

using namespace fraggroup;

// Zero byte x (absolute address) of the 16-byte chunk at ca, if it lies there.
__device__ __forceinline__ void mask_byte(u32x4& c, uint64_t ca, uint64_t x) {
    if (x < ca || x >= ca + 16) return;
    const uint32_t o = (uint32_t)(x - ca), m = ~(0xffu << (8 * (o & 3)));
    switch (o >> 2) {
        case 0: c.x &= m; break;
        case 1: c.y &= m; break;
        case 2: c.z &= m; break;
        default: c.w &= m; break;
    }
}

template <int MODE, bool IMPLICIT>
__global__ __launch_bounds__(64) void frag_kernel(KParams p, const smol_csum_frag_group_t* groups, uint64_t ngroups) {
    constexpr bool EMIT = MODE == MODE_EMIT;
    __shared__ uint64_t s_addr[MAXF];  // the datagram map (DgMap)
    __shared__ uint32_t s_start[MAXF], s_end[MAXF];
    __shared__ uint8_t s_bits[MAXF];
    const int lane = (int)threadIdx.x;

    for (uint64_t gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
        const uint64_t first = groups[gi].first;
        const uint32_t count = groups[gi].count;
        if (!group_valid(p, groups[gi])) continue;

        // ---- 1. the fragments' IPv4 headers ----
        const Key k0 = group_key<IMPLICIT>(p, first);
        bool bad = !k0.ok, raw = false;
        uint32_t T = 0, sumlen = 0, lastn = 0;
        for (uint32_t j = (uint32_t)lane; j < count; j += 64) {
            const FragHdr h = frag_header<EMIT, IMPLICIT>(p, first + j, k0);
            raw = raw || h.raw;
            bad = bad || h.bad;
            T = max(T, h.T);
            sumlen += h.sumlen;
            lastn += h.lastn;
            s_addr[j] = h.addr;
            s_start[j] = h.start;
            s_end[j] = h.end;
            s_bits[j] = (uint8_t)h.bits;
        }
        lds_sync();
        T = wave_max(T);
        sumlen = wave_sum(sumlen);
        lastn = wave_sum(lastn);
        bad = wave_any(bad);
        raw = wave_any(raw);

        // ---- 2. the group contract ----
        const DgMap map = {s_addr, s_start, s_end, s_bits, count, (uint64_t)p.dummy};
        bool broken = bad || lastn != 1 || sumlen != T;
        uint32_t zeros = 0;
        for (uint32_t j = (uint32_t)lane; !broken && j < count; j += 64) {
            const Row row = contract_row(map, j, T);
            zeros += row.zero;
            if (row.broken) broken = true;
        }
        broken = wave_any(broken) || wave_sum(zeros) != 1;

        // ---- 3. the L4 header through the datagram map ----
        const L4Hdr l4 = l4_header<EMIT>(map, k0, broken, raw, T);
        const uint32_t proto = l4.proto, st = l4.st, span_end = l4.span_end, fo = l4.fo, in_hl = l4.in_hl;

        // ---- 4. the payload sum: data() per fragment slice, one's-complement sum over slices ----
        Verdict verdict = {1, 1, 0};
        if (proto != P_NONE) {
            const uint64_t f0 = EMIT ? map.addr_of(fo) : 0, f1 = EMIT ? map.addr_of(fo + 1) : 0;
            const uint64_t i0 = in_hl ? map.addr_of(18) : 0, i1 = in_hl ? map.addr_of(19) : 0;
            uint32_t D = 0;
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t lo = s_start[j], hi = min(s_end[j], span_end);
                if (hi <= lo) continue;
                const uint64_t A = s_addr[j], B = A + (hi - lo);
                const uint64_t base = A & ~15ull;
                const uint32_t nch = (uint32_t)(((B + 15) >> 4) - (base >> 4));
                uint32_t acc = 0;
                for (uint32_t k = (uint32_t)lane; k < nch; k += 64) {
                    const uint64_t ca = base + 16ull * k;
                    u32x4 c = *(gcv4)ca;
                    const int a = (int)((int64_t)A - (int64_t)ca), b = (int)((int64_t)B - (int64_t)ca);
                    c.x = mask_dword(c.x, a, b);
                    c.y = mask_dword(c.y, a - 4, b - 4);
                    c.z = mask_dword(c.z, a - 8, b - 8);
                    c.w = mask_dword(c.w, a - 12, b - 12);
                    if (EMIT) {  // the reference zeroes the fields before summing
                        mask_byte(c, ca, f0);
                        mask_byte(c, ca, f1);
                        if (in_hl) {
                            mask_byte(c, ca, i0);
                            mask_byte(c, ca, i1);
                        }
                    }
                    acc = add_words(c.x, add_words(c.y, add_words(c.z, add_words(c.w, acc))));
                }
                const uint32_t S = fold32(wave_sum(acc));
                D += (A & 1u) ? S : bswap16(S);  // data() of the slice (csum_device.h)
            }
            uint32_t dat = fold32(D);
            uint32_t vin = 0;
            if (EMIT && in_hl) {
                // Icmpv4Repr::emit writes the embedded IPv4 header under the same caps first
                // (icmpv4.rs:520-543); its field is a BE word at even datagram offset 18
                uint32_t hin = 0;
                for (uint32_t w = 0; w < in_hl / 2; ++w)
                    if (w != 5) hin += map.byte(8 + 2 * w) << 8 | map.byte(9 + 2 * w);
                vin = caps_tx(p.caps_ipv4) ? (~fold32(hin) & 0xffffu) : 0u;
                dat = fold32(dat + vin);
            }
            const L4Sum sum = l4_sum(p, k0, l4, T, dat);
            if (EMIT) {
                if (lane == 0) {
                    uint32_t c = ~sum.comb & 0xffffu;
                    if (proto == P_UDP && c == 0) c = 0xffffu;  // udp.rs:207
                    const uint32_t v = (proto == P_IGMP || caps_tx(sum.gate)) ? c : 0u;
                    ((gu8)f0)[0] = (uint8_t)(v >> 8);
                    ((gu8)f1)[0] = (uint8_t)v;
                    if (in_hl) {
                        ((gu8)i0)[0] = (uint8_t)(vin >> 8);
                        ((gu8)i1)[0] = (uint8_t)vin;
                    }
                }
            } else {
                verdict = l4_verdict(sum, proto, map.byte(fo) << 8 | map.byte(fo + 1));
            }
        }

        // ---- 5. status bytes ----
        bool all_ip = true;
        if (!EMIT)
            for (uint32_t j = (uint32_t)lane; j < count; j += 64) all_ip = all_ip && (s_bits[j] & 4u);
        all_ip = !wave_any(!all_ip);
        for (uint32_t j = (uint32_t)lane; j < count; j += 64) {
            const uint32_t s = frag_status<EMIT>(s_bits[j], st, verdict, all_ip);
            if (p.status) ((gu8)p.status)[first + j] = (uint8_t)s;
        }
        lds_sync();  // the next group's phase 1 rewrites the map
    }
}

}  // namespace frag

hipError_t launch_frag(int mode, const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups,
                       hipStream_t s) {
    const uint32_t blocks = grid_blocks(ngroups, kMaxGridBlocks);
    const bool implicit = p.desc == nullptr;
    if (mode == MODE_EMIT) {
        if (implicit) hipLaunchKernelGGL((frag::frag_kernel<MODE_EMIT, true>), dim3(blocks), dim3(64), 0, s, p, groups, ngroups);
        else hipLaunchKernelGGL((frag::frag_kernel<MODE_EMIT, false>), dim3(blocks), dim3(64), 0, s, p, groups, ngroups);
    } else {
        if (implicit) hipLaunchKernelGGL((frag::frag_kernel<MODE_VERIFY, true>), dim3(blocks), dim3(64), 0, s, p, groups, ngroups);
        else hipLaunchKernelGGL((frag::frag_kernel<MODE_VERIFY, false>), dim3(blocks), dim3(64), 0, s, p, groups, ngroups);
    }
    return hipGetLastError();
}

}  // namespace smolcsum
