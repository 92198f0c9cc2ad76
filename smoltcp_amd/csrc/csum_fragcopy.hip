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
//   1.-3. as frag_kernel: thread j parses fragment j's IPv4 header into the datagram map in LDS, the
//      workgroup checks the group contract, and the L4 header is read through the map.  The wave
//      reductions of frag_kernel become workgroup reductions: per-wave values meet in LDS.
//   4. the fragments are dealt to the four wavefronts (fragment j to wave j mod 4).  A wavefront
//      streams its fragment as 16-B chunks on the source's grid, U per lane and step, all loads of a
//      step issued first, and the first step of its NEXT fragment is issued before the current one is
//      used, so a lane has up to 2 U chunks (and the two successor chunks) in flight.
//      * Sum: each chunk as frag_kernel sums it (edges masked, UDP capped at span_end); a fragment's sum
//        becomes its data() value, the wave adds those up, and the four waves' values meet in LDS:
//        the one's-complement sum does not depend on the order, so the verdict is verify_frag's.
//      * Copy: destination chunks lie on d_dst's 16-B grid.  Destination chunk k of a fragment
//        (fragment-payload bytes [16 k - dh, 16 k - dh + 16), dh = destination address mod 16) is
//        funnel16 of chunk slot k and its successor, taken from the next lane (DPP / bpermute, next4);
//        lane 63 takes it from its own next register and for its last chunk of a step from one extra
//        16-B load.  When dh is larger than the source's offset in its first chunk, the slots start
//        one chunk early (slot 0 reads the dummy line: none of its bytes is used).  Chunks entirely
//        inside the payload go out as one dwordx4 store, a fragment's first and last chunk byte-masked
//        (store_edge): two fragments of a datagram meet at a multiple of 8, inside a destination
//        chunk that two wavefronts write.  No byte of d_dst is read.
//   5. thread j writes fragment j's status byte (frag_kernel's), thread 0 the group's smol_csum_dgram_t.
// The cap is tested before the first store: a group that does not fit still streams for its status.
// The copy waits for no verdict, neither the L4 checksum's nor a fragment header's.
//
// Every barrier is reached by all 256 threads: an invalid group is skipped by the whole workgroup
// before the first one, and broken / raw / unsupported / too-large groups take every barrier with
// nothing to stream.
#include "csum_walk.h"

namespace smolcsum {
namespace fragcopy {

constexpr uint32_t MAXF = SMOL_MAX_FRAGMENTS;
constexpr int U = 2;           // chunks per lane and step: a 1480-B fragment is one step
constexpr uint32_t STEP = 64 * U;
static_assert(MAXF <= 256, "thread j parses fragment j");

__device__ __forceinline__ uint32_t rb(uint64_t a) { return *(gcu8)a; }
__device__ __forceinline__ uint32_t rb16(uint64_t a) { return (rb(a) << 8) | rb(a + 1); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}
__device__ __forceinline__ bool wave_any(bool b) { return __ballot(b) != 0; }

__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One fragment's stream (the same for every lane of the wave).
struct Piece {
    uint64_t base;     // chunk-grid origin: the payload address rounded down to 16
    uint64_t D;        // destination address of the payload's first byte
    uint32_t head;     // payload address - base
    uint32_t nch;      // source chunks that hold a byte of the streamed range
    uint32_t lead;     // 1: the chunk slots start one chunk before base (slot k holds chunk k - lead)
    uint32_t nk;       // chunk slots: nch + lead
    uint32_t sh;       // funnel shift: (head - dh) mod 16
    uint32_t dh;       // D mod 16
    uint32_t sum_len;  // payload bytes summed (0: none)
    uint32_t copy_len; // payload bytes delivered (0: none)
    uint32_t odd;      // the payload starts at an odd address
};

template <bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void fragcopy_kernel(
    KParams p, const smol_csum_frag_group_t* groups, uint64_t ngroups, FragCopyArgs v) {
    using vcopy::next4;
    using vcopy::store_edge;
    using vcopy::sum_chunk;
    __shared__ uint64_t s_addr[MAXF];  // payload start address of fragment j
    __shared__ uint32_t s_start[MAXF], s_end[MAXF];
    __shared__ uint8_t s_bits[MAXF];   // bit 0 check_len ok, 1 MF, 2 IP gate passed, 3 header valid
    // the four waves' values of each workgroup reduction (one array per reduction: no reuse inside a group)
    __shared__ uint32_t s_r1[4][6], s_r2[4][2], s_r4[4];
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
        const uint64_t first = groups[gi].first;
        const uint32_t count = groups[gi].count;
        // an invalid group (outside the batch, count 0 or > SMOL_MAX_FRAGMENTS, reserved != 0): none of its
        // records is read or written; its entry, indexed by group, is zero.  The whole workgroup leaves here.
        if (first >= p.n || count == 0 || count > MAXF || count > p.n - first || groups[gi].reserved != 0) {
            if (tid == 0) *(GMEM u32x4*)((uint64_t)v.dgrams + 16ull * gi) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }

        // ---- 1. the fragments' IPv4 headers (frag_kernel, MODE_VERIFY) ----
        auto rec = [&](uint32_t j, uint64_t& a0, uint32_t& len, uint32_t& kind) {
            const uint64_t r = first + j;
            if (IMPLICIT) {
                a0 = (uint64_t)p.buf + r * p.stride;
                len = p.len;
                kind = p.kind;
            } else {
                const u32x4 d = *(gcv4)((uint64_t)p.desc + 16 * r);
                a0 = (uint64_t)p.buf + ((uint64_t)d.x | ((uint64_t)d.y << 32));
                len = d.z;
                kind = desc_kind(d.w);
            }
        };
        // fragment 0's reassembly key (ipv4.rs get_key: ident, src, dst, protocol)
        uint64_t k0a = 0;
        bool k0ok = false;
        {
            uint64_t a0;
            uint32_t len, kind;
            rec(0, a0, len, kind);
            kind &= 0xffu;
            const uint32_t io = kind == SMOL_KIND_ETH ? 14u : 0u;
            if ((kind == SMOL_KIND_IP || kind == SMOL_KIND_ETH) && len >= io + 20) {
                k0a = a0 + io;
                k0ok = true;
            }
        }
        bool bad = !k0ok, raw = false, ip_drop = false;
        uint32_t T = 0, sumlen = 0, lastn = 0;
        if (tid < count) {
            const uint32_t j = tid;
            uint64_t a0;
            uint32_t len, kind;
            rec(j, a0, len, kind);
            raw = (kind & KIND_IPHDR_ONLY) != 0;  // a raw socket's datagram: headers only
            kind &= 0xffu;
            uint32_t io = 0, ok = 0, hl = 0, total = 0, start = 0, end = 0, mf = 0;
            if (kind == SMOL_KIND_ETH) {
                io = 14;
                ok = len >= 14 && rb16(a0 + 12) == 0x0800u;
            } else {
                ok = kind == SMOL_KIND_IP;
            }
            const uint64_t ip = a0 + io;
            if (ok) ok = len - io >= 20 && (rb(ip) >> 4) == 4;
            if (ok) {
                hl = (rb(ip) & 0x0fu) * 4;
                total = rb16(ip + 2);
                const uint32_t lb = len - io;
                ok = !(lb < hl || hl > total || lb < total || hl < 20);  // Ipv4Packet::check_len
            }
            uint32_t bits = 0xcu;  // IP gate / header: passed unless verified and found bad
            if (ok) {
                const uint32_t fl = rb16(ip + 6);
                start = (fl & 0x1fffu) * 8;  // Ipv4Packet::frag_offset, ipv4.rs:319-322
                end = start + total - hl;
                mf = (fl >> 13) & 1u;
                bool same = k0ok && rb(ip + 9) == rb(k0a + 9) && rb16(ip + 4) == rb16(k0a + 4);
                for (uint32_t b = 12; b < 20; ++b) same = same && rb(ip + b) == rb(k0a + b);
                bad = bad || !same || end <= start;
                T = end;
                sumlen = end - start;
                lastn = mf ? 0u : 1u;
                uint32_t hs = 0;
                for (uint32_t w = 0; w < hl / 2; ++w) hs += rb16(ip + 2 * w);
                const uint32_t valid = fold32(hs) == 0xffffu;
                const uint32_t okg = caps_rx(p.caps_ipv4) ? valid : 1u;
                bits = (okg ? 4u : 0u) | (valid ? 8u : 0u);
            } else {
                bad = true;  // no IPv4 header checked: its IP bits stay set, the record is MALFORMED
            }
            ip_drop = !(bits & 4u);
            s_addr[j] = ip + hl;
            s_start[j] = start;
            s_end[j] = end;
            s_bits[j] = (uint8_t)(bits | (mf << 1) | (ok ? 1u : 0u));
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
        bool broken = bad || lastn != 1 || sumlen != T;
        {
            bool mine = false;
            uint32_t zeros = 0;
            if (!broken && tid < count) {
                const uint32_t sj = s_start[tid], ej = s_end[tid];
                uint32_t starts = 0, next = 0;
                for (uint32_t i = 0; i < count; ++i) {
                    starts += s_start[i] == sj;
                    next += s_start[i] == ej;
                }
                zeros = sj == 0;
                mine = starts != 1 || (ej != T && next != 1) || (!(s_bits[tid] & 2u) && ej != T);
            }
            const bool wB = wave_any(mine);
            const uint32_t wZ = wave_sum(zeros);
            if (lane == 0) {
                s_r2[wave][0] = wB;
                s_r2[wave][1] = wZ;
            }
        }
        lds_sync();  // (all threads)
        broken = broken || (s_r2[0][0] | s_r2[1][0] | s_r2[2][0] | s_r2[3][0]) != 0 ||
                 s_r2[0][1] + s_r2[1][1] + s_r2[2][1] + s_r2[3][1] != 1;

        // ---- 3. the L4 header through the datagram map (every thread: the values are the workgroup's) ----
        auto dg_addr = [&](uint32_t o) -> uint64_t {
            for (uint32_t i = 0; i < count; ++i)
                if (s_start[i] <= o && o < s_end[i]) return s_addr[i] + (o - s_start[i]);
            return dummy;  // (a usable group covers [0, T): not reached)
        };
        auto dg = [&](uint32_t o) -> uint32_t { return rb(dg_addr(o)); };
        uint32_t proto = P_NONE, st = 0, span_end = 0, fo = 0, key_proto = 0, l4_off = 0, l4_len = 0;
        if (broken) {
            st = SMOL_ST_MALFORMED;
        } else {
            key_proto = rb(k0a + 9);
            if (raw) {
                st = SMOL_ST_UNSUPPORTED;
            } else if (key_proto == P_UDP) {
                fo = 6;
                const uint32_t ul = T >= 8 ? (dg(4) << 8 | dg(5)) : 0u;
                if (T < 8 || T < ul || ul < 8) st = SMOL_ST_MALFORMED;
                else if ((dg(2) | dg(3)) == 0) st = SMOL_ST_MALFORMED;  // udp.rs:246-248
                span_end = ul;
                if (!st) {  // UdpPacket::payload, udp.rs:153-157
                    l4_off = 8;
                    l4_len = ul - 8;
                }
            } else if (key_proto == P_TCP) {
                fo = 16;
                const uint32_t thl = T >= 20 ? (dg(12) >> 4) * 4 : 0u;
                if (T < 20 || T < thl || thl < 20) st = SMOL_ST_MALFORMED;
                else if ((dg(0) | dg(1)) == 0 || (dg(2) | dg(3)) == 0) st = SMOL_ST_MALFORMED;  // tcp.rs:910-915
                span_end = T;
                if (!st) {  // TcpPacket::payload, tcp.rs:419-423
                    l4_off = thl;
                    l4_len = T - thl;
                }
            } else if (key_proto == P_ICMP4 || key_proto == P_IGMP) {
                fo = 2;
                if (T < 8) st = SMOL_ST_MALFORMED;
                span_end = T;
            } else {
                st = SMOL_ST_UNSUPPORTED;
            }
            if (!st) proto = key_proto;
        }

        // ---- 4. one pass over the payloads: data() per fragment slice, and the delivery ----
        const u32x4 sl = *(gcv4)((uint64_t)v.slots + 16ull * gi);  // dst_offset, cap, reserved
        const bool do_sum = proto != P_NONE;
        const bool do_copy = !broken && T <= sl.z;  // the cap test, before the first store
        const uint64_t Dslot = (uint64_t)v.dst + ((uint64_t)sl.x | ((uint64_t)sl.y << 32));

        auto setup = [&](uint32_t j) -> Piece {
            Piece q;
            const uint32_t lo = s_start[j], hi = s_end[j];
            const uint64_t A = s_addr[j];
            const uint32_t he = min(hi, span_end);
            q.sum_len = do_sum && he > lo ? he - lo : 0u;
            q.copy_len = do_copy ? hi - lo : 0u;
            const uint32_t L = max(q.sum_len, q.copy_len);
            q.base = A & ~15ull;
            q.head = (uint32_t)(A - q.base);
            q.nch = L ? (uint32_t)(((A + L + 15) >> 4) - (q.base >> 4)) : 0u;
            q.D = Dslot + lo;
            q.dh = (uint32_t)(q.D & 15u);
            q.sh = (q.head - q.dh) & 15u;
            q.lead = q.copy_len && q.head < q.dh ? 1u : 0u;
            q.nk = q.nch + q.lead;
            q.odd = (uint32_t)(A & 1u);
            return q;
        };
        // one step: chunk slots [i0, i0 + STEP), and for lane 63 the slot after them
        auto load = [&](const Piece& q, uint32_t i0, u32x4 (&c)[U], u32x4& xh) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * 64 + lane) - q.lead;  // (slot 0 of a lead: wraps, >= nch)
                c[u] = ld16<false>((gcv4)(k < q.nch ? q.base + 16ull * k : dummy));
            }
            const uint32_t kx = i0 + STEP - q.lead;
            xh = ld16<false>((gcv4)(q.copy_len && lane == 63 && kx < q.nch ? q.base + 16ull * kx : dummy));
        };
        auto use = [&](const Piece& q, uint32_t i0, const u32x4 (&c)[U], const u32x4& xh, uint32_t& acc) {
            if (q.sum_len) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t k = i0 + (uint32_t)(u * 64 + lane) - q.lead;
                    if (k < q.nch) acc = sum_chunk(c[u], (int)(16u * k) - (int)q.head, (int)q.sum_len, acc);
                }
            }
            if (q.copy_len) {  // (the wave's lanes together: the exchange below needs all of them)
                u32x4 ncur = next4<64>(c[0], lane);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const u32x4 nnext = u + 1 < U ? next4<64>(c[u + 1 < U ? u + 1 : u], lane) : xh;
                    const u32x4 hi = lane == 63 ? nnext : ncur;
                    ncur = nnext;
                    const uint32_t k = i0 + (uint32_t)(u * 64 + lane);
                    const int pos = (int)(16u * k) - (int)q.dh;  // payload-relative start of destination chunk k
                    const int lo = -pos, end = (int)q.copy_len - pos;
                    if (k < q.nk && end > 0 && lo < 16) {
                        const u32x4 m = funnel16(c[u], hi, q.sh);
                        const gu8 dst = (gu8)(q.D + (uint64_t)(int64_t)pos);
                        if (lo <= 0 && end >= 16) *(GMEM u32x4*)dst = m;
                        else store_edge(dst, m, lo, end);
                    }
                }
            }
        };

        uint32_t Dw = 0;  // the wave's sum of data() values
        if (do_sum || do_copy) {
            uint32_t j = wave;
            Piece cur = {};
            u32x4 c[U], xh;
            if (j < count) {
                cur = setup(j);
                load(cur, 0u, c, xh);
            }
            while (j < count) {
                const uint32_t jn = j + 4;
                Piece nxt = {};
                u32x4 cn[U], xn;
                if (jn < count) {  // the next fragment's first step, in flight under this one's work
                    nxt = setup(jn);
                    load(nxt, 0u, cn, xn);
                }
                uint32_t acc = 0;
                use(cur, 0u, c, xh, acc);
                for (uint32_t i0 = STEP; i0 < cur.nk; i0 += STEP) {
                    load(cur, i0, c, xh);
                    use(cur, i0, c, xh, acc);
                }
                if (cur.sum_len) {
                    const uint32_t S = fold32(wave_sum(acc));
                    Dw += cur.odd ? S : bswap16(S);  // data() of the slice (csum_device.h)
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

        uint32_t l4_valid = 1, l4_ok = 1, partial = 0;
        if (do_sum) {
            const uint32_t dat = fold32(s_r4[0] + s_r4[1] + s_r4[2] + s_r4[3]);
            uint32_t ph = 0, psum = 0;
            const bool pseudo = proto == P_UDP || proto == P_TCP;
            if (pseudo) {
                for (uint32_t b = 12; b < 20; b += 2) psum += rb16(k0a + b);
                ph = fold32(psum + proto + ((proto == P_UDP ? span_end : T) & 0xffffu));  // pseudo_header_v4
            }
            const uint32_t comb = pseudo ? fold32(ph + dat) : dat;
            const uint32_t gate = proto == P_UDP ? p.caps_udp : proto == P_TCP ? p.caps_tcp
                                : proto == P_ICMP4 ? p.caps_icmpv4 : (uint32_t)SMOL_CHECKSUM_NONE;
            const uint32_t field = dg(fo) << 8 | dg(fo + 1);
            l4_valid = comb == 0xffffu;
            if (proto == P_UDP && field == 0) l4_valid = 1;  // udp.rs:138-140
            if (pseudo) partial = ph == field;
            l4_ok = caps_rx(gate) ? l4_valid : 1u;
        }

        // ---- 5. status bytes (frag_kernel's) and the datagram entry ----
        const bool mal = (st & SMOL_ST_MALFORMED) != 0;
        if (tid < count) {
            const uint32_t bits = s_bits[tid];
            const uint32_t s = st | ((bits & 4u) ? SMOL_ST_IP_OK : 0u) | ((bits & 8u) ? SMOL_ST_IP_VALID : 0u) |
                               ((bits & 1u) ? 0u : (uint32_t)SMOL_ST_MALFORMED) |
                               (l4_ok ? SMOL_ST_L4_OK : 0u) | (l4_valid ? SMOL_ST_L4_VALID : 0u) |
                               (partial ? SMOL_ST_L4_PARTIAL : 0u) | ((all_ip && l4_ok && !mal) ? SMOL_ST_ACCEPT : 0u);
            ((gu8)p.status)[first + tid] = (uint8_t)s;
        }
        if (tid == 0) {  // smol_csum_dgram_t: len, l4_len, l4_off | protocol | copied, reserved
            u32x4 e = {0u, 0u, 0u, 0u};
            if (!broken) {
                e.x = T;
                e.y = l4_len;
                e.z = l4_off | (key_proto << 16) | ((do_copy ? 1u : 0u) << 24);
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
