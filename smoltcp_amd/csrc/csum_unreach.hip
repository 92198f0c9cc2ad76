// Fused verify + ICMP error responder (smol_csum_batch_verify_unreach_reply): echo_kernel (csum_echo.hip)
// with the two sums ending at different bytes, a port map and a longer head.
//
// The reference refuses a UDP datagram to a closed port (process_udp, src/iface/interface/udp.rs:49-77), an
// IPv4 packet of an unhandled protocol (ipv4.rs:240-250) and an IPv6 packet with an unrecognised next header
// (process_nxt_hdr, ipv6.rs:352-364) with an ICMP error that quotes the IP header, emitted again, and the first
// 528 / 1192 bytes of the IP payload: UdpRepr::parse sums the datagram, Icmpv4Repr::emit / Icmpv6Repr::emit
// copy the slice (icmpv4.rs:519-531, icmpv6.rs:740-755) and fill_checksum sums the copy.  Here every 16-B chunk
// of a record is loaded once.
//
// echo_kernel's form: a group of G lanes owns a record, its chunks on the record's own 16-B grid, G * U of them
// per step, step 0 holding the 128-B header window in LDS for parse_geometry (emit = false: verify's parse);
// the copy of the data to its place behind the frame's head is vcopy_kernel's copy of a payload.
// * Three regions from one starting byte.  The verdict sums record bytes [0, s1) (s1: verify's span end, 0 when
//   it sums nothing of the record), the reply [off, e2) (off: the IP payload's first byte, e2 = off + dlen).
//   Each lane keeps two accumulators over disjoint bytes: [0, min(s1, e2)) and [min, max).  The first belongs to
//   both sums, the second to the one that ends later: that owner is one comparison per record.  The ends are
//   byte-exact (sum_range masks the edge chunks), so an odd UDP length pads the verdict's sum with a zero byte
//   while the reply's runs on, and for the protocol / next-header forms (s1 = 0) the whole data is the reply's.
//   The verdict's sum goes to finish_gates (MODE_VERIFY) unchanged.  The reply's leaves out the header bytes
//   [0, off), which the lanes sum again from the LDS window, as finish_gates does for the verdict: plain u32
//   sums, nothing is subtracted from a folded value, so 0x0000 and 0xffff stay apart.
// * The port map.  One dependent byte load after the parse, for well-formed UDP records only.
// * Head.  The rule and the head's bytes with zero checksum fields are csum_unreach.h's, read from the LDS
//   window.  The group's lanes share the word sums of the two IPv4 headers and of the ICMP message; then lane j
//   builds the aligned dwords j, j + G, .. of the destination range [D, D + head_len) (up to 27 of them) and
//   stores them byte-masked, so no byte of d_dst is read and none outside the frame is written.
// * Entry.  Lane 0 writes the record's 8-byte smol_csum_unreach_t; SEND comes from the status byte finish_gates
//   hands back.
// The cap is tested before the first store.  The copy does not wait for the verdict.
#include "csum_unreach.h"
#include "csum_walk.h"

namespace smolcsum {

namespace unreach {

constexpr int WIN = 128;  // the header window: 16-B grid, Grid<false>
constexpr int WIN_CH = WIN / 16;

// The request as csum_unreach.h reads it: addresses, MACs and the TTL / hop limit from the LDS window (record
// byte o at w[o]; all of them lie in front of byte 54), the rest in registers.
struct WinReq {
    const uint8_t* w;
    uint32_t kind_, ver_, ip_, plen_, proto_, hbh_;
    __device__ __forceinline__ uint32_t kind() const { return kind_; }
    __device__ __forceinline__ uint32_t ver() const { return ver_; }
    __device__ __forceinline__ uint32_t plen() const { return plen_; }
    __device__ __forceinline__ uint32_t proto() const { return proto_; }
    __device__ __forceinline__ bool hbh() const { return hbh_ != 0; }
    __device__ __forceinline__ uint32_t hop() const { return w[ip_ + (ver_ == 4 ? 8u : 7u)]; }
    __device__ __forceinline__ uint32_t mac_dst(uint32_t j) const { return w[j]; }
    __device__ __forceinline__ uint32_t mac_src(uint32_t j) const { return w[6 + j]; }
    __device__ __forceinline__ uint32_t ethertype(uint32_t j) const { return w[12 + j]; }
    __device__ __forceinline__ uint32_t src(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 12u : 8u) + j]; }
    __device__ __forceinline__ uint32_t dst(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 16u : 24u) + j]; }
};

// What the rule left of a record, in LDS beside its geometry: unreach_rule's result, the IP payload's offset
// (0 unless REFUSED) and length P, and the protocol / next header reached | hbh << 8.
struct Fact {
    uint32_t rv, off, plen, proto, dlo, dhi, cap;  // (dlo, dhi, cap: the record's slot)
};

// Aligned-word sum of the chunk's bytes inside the record range [lo, hi) (pos: chunk start relative to the
// record start): sum_chunk with a lower bound.
__device__ __forceinline__ uint32_t sum_range(const u32x4& c, int pos, int lo, int hi, uint32_t acc) {
    if (pos >= hi || pos + 16 <= lo) return acc;
    if (pos < lo || pos + 16 > hi) return sum_masked_words(c, lo - pos, hi - pos, acc);
    return add_words(c.x, add_words(c.y, add_words(c.z, add_words(c.w, acc))));
}

}  // namespace unreach

template <int G, int U, bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void unreach_kernel(KParams p, UnreachArgs v) {
    using namespace unreach;
    using vcopy::next4;
    using vcopy::store_edge;
    constexpr int GPB = 256 / G;
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "group size");
    static_assert(G * U >= WIN_CH, "step 0 holds the window");
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ Geom geo[GPB];
    __shared__ Fact fct[GPB];

    const int lane = (int)(threadIdx.x % G);
    const int gib = (int)(threadIdx.x / G);
    const uint64_t ngroups = (uint64_t)gridDim.x * GPB;
    u32x4* wn = &win[gib][0];
    const uint8_t* winb = reinterpret_cast<const uint8_t*>(wn);
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t r = (uint64_t)blockIdx.x * GPB + gib; r < p.n; r += ngroups) {
        const RecRef rr = rec_at<IMPLICIT, false>(p, r);
        const u32x4 sl = *(gcv4)((uint64_t)v.slots + 16ull * r);  // dst_offset, cap, reserved
        const uint64_t base = rr.a0 & ~15ull;
        const uint32_t head = (uint32_t)(rr.a0 - base);
        const uint32_t nch = n_chunks<false>(rr);

        // one step: chunks [i0, i0 + G * U), and for the group's last lane the chunk after them
        u32x4 c[U], xh;
        auto load = [&](uint32_t i0, bool next) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                c[u] = ld16<false>((gcv4)(k < nch ? base + 16ull * k : dummy));
            }
            const uint32_t kx = i0 + (uint32_t)(U * G);
            xh = ld16<false>((gcv4)(next && lane == G - 1 && kx < nch ? base + 16ull * kx : dummy));
        };
        load(0u, true);
#pragma unroll
        for (int u = 0; u * G < WIN_CH; ++u) {
            const uint32_t k = (uint32_t)(u * G + lane);
            if (k < (uint32_t)WIN_CH && k < nch) wn[k] = c[u];
        }
        wave_lds_sync();
        // record byte o: the LDS window, else global memory (behind a long Hop-by-Hop header)
        auto rd = [&](uint32_t o) -> uint32_t {
            const uint32_t x = head + o;
            if (x < (uint32_t)WIN) return (uint32_t)winb[x];
            return ld_byte_sync(rr.a0 + o);
        };
        {
            const Geom g0 = parse_geometry<false>(rd, rr.len, rr.kind, false);
            if (lane == 0) geo[gib] = g0;
        }
        wave_lds_sync();
        const Geom& g = geo[gib];
        const bool l4 = g.proto != P_NONE && !(g.st & SMOL_ST_MALFORMED);
        const int s1 = l4 ? (int)g.span_end : 0;

        // the refusal (process_udp udp.rs:49-77, ipv4.rs:240-250, process_nxt_hdr ipv6.rs:352-364), the address
        // rule and the frame's geometry
        // (its result goes to LDS next to the geometry and is read back behind the stream, where the frame's
        // geometry is worked out again: held in registers across the stream it spilled 12 to 40 bytes in half of
        // the instantiations)
        if (lane == 0) {
            uint32_t rv = 0, off = 0, plen = 0, proto = 0, hbh = 0;
            if (g.fam != 0 && !(rr.kind & KIND_IPHDR_ONLY) && !(g.st & SMOL_ST_MALFORMED)) {
                // an unsupported record that got past the fragment test (which leaves l4_off 0) is one of an
                // unknown protocol / next header; a UDP record is looked up in the port map
                bool cand = (g.st & SMOL_ST_UNSUPPORTED) && g.l4_off != 0, closed = false;
                if (!g.st && g.proto == P_UDP && v.udp_open) {
                    const uint32_t dp = rd(g.l4_off + 2) << 8 | rd(g.l4_off + 3);
                    closed = ((ld_byte_sync((uint64_t)v.udp_open + (dp >> 3)) >> (dp & 7u)) & 1u) == 0;
                    cand = closed;
                }
                if (cand) {
                    if (g.fam == 4) {
                        proto = rd(g.ip_off + 9);
                        off = g.l4_off;
                        plen = g.l4_len;
                    } else {
                        const uint32_t nh = rd(g.ip_off + 6);
                        hbh = nh == 0;
                        proto = hbh ? rd(g.ip_off + 40) : nh;
                        off = g.ip_off + 40;
                        plen = rd(g.ip_off + 4) << 8 | rd(g.ip_off + 5);
                    }
                    rv = unreach_rule(WinReq{winb + head, rr.kind & 0xffu, g.fam, g.ip_off, plen, proto, hbh}, v.bcast_v4, closed);
                }
            }
            Fact f;  // off: 0 unless REFUSED
            f.rv = rv, f.off = rv ? off : 0u, f.plen = plen, f.proto = proto | hbh << 8;
            f.dlo = sl.x, f.dhi = sl.y, f.cap = sl.z;
            fct[gib] = f;
        }
        wave_lds_sync();
        // the record as the rule left it: the flags, the frame's lengths, the cap test (before the first store)
        auto frame = [&](uint32_t& fl, uint32_t& off, uint32_t& hl, uint32_t& dlen, bool& written) {
            const Fact& f = fct[gib];
            fl = unreach_flags(f.rv);
            off = f.off;
            const bool answered = (fl & SMOL_UNR_ANSWERED) != 0;
            hl = answered ? unreach_head_len(rr.kind & 0xffu, g.fam) : 0u;
            dlen = answered ? unreach_dlen(g.fam, f.plen) : 0u;
            written = answered && hl + dlen <= f.cap;
        };
        bool st;
        uint64_t Dd;  // where the data goes
        uint32_t sh, dlen;
        int dk0, lo2, hi2;
        {
            uint32_t fl, off, hl;
            bool written;
            frame(fl, off, hl, dlen, written);
            st = written && dlen > 0;
            Dd = (uint64_t)v.dst + ((uint64_t)fct[gib].dlo | ((uint64_t)fct[gib].dhi << 32)) + hl;
            sh = (uint32_t)((rr.a0 + off - Dd) & 15u);
            // destination chunk of record chunk k: data-relative position 16 k + dk0
            dk0 = (int)sh - (int)head - (int)off;
            // the two sums: [0, s1) and [off, e2); the accumulators part where the first of them ends
            const int e2 = (fl & SMOL_UNR_ANSWERED) ? (int)(off + dlen) : 0;
            lo2 = s1 < e2 ? s1 : e2, hi2 = s1 < e2 ? e2 : s1;
        }

        uint32_t acc = 0, accx = 0;
        for (uint32_t i0 = 0; i0 < nch; i0 += (uint32_t)(G * U)) {
            if (i0) load(i0, st);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                if (k < nch) {
                    const int pos = (int)(16u * k) - (int)head;
                    acc = sum_range(c[u], pos, 0, lo2, acc);
                    accx = sum_range(c[u], pos, lo2, hi2, accx);
                }
            }
            if (st) {  // (the group's lanes together: the exchange below needs all of them)
                u32x4 ncur = next4<G>(c[0], lane);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const u32x4 nnext = u + 1 < U ? next4<G>(c[u + 1 < U ? u + 1 : u], lane) : xh;
                    const u32x4 hi = lane == G - 1 ? nnext : ncur;
                    ncur = nnext;
                    const uint32_t k = i0 + (uint32_t)(u * G + lane);
                    const int pos = (int)(16u * k) + dk0;
                    const int lo = -pos, end = (int)dlen - pos;
                    if (k < nch && end > 0 && lo < 16) {
                        const u32x4 m = funnel16(c[u], hi, sh);
                        const gu8 dst = (gu8)(Dd + (uint64_t)(int64_t)pos);
                        if (lo <= 0 && end >= 16) *(GMEM u32x4*)dst = m;
                        else store_edge(dst, m, lo, end);
                    }
                }
            }
        }

        uint32_t stv = 0;  // lane 0: the status byte
        // (the second accumulator is the sum's that ends later: the verdict's when hi2 is its end)
        finish_gates<G, MODE_VERIFY, false, decltype(rd)>(p, g, hi2 == s1 ? acc + accx : acc, rd, winb, head, rr.a0, r, lane,
                                                          nullptr, ~0ull, ~0ull, 0, nullptr, &stv);
        uint32_t fl, off, hl;
        bool written;
        frame(fl, off, hl, dlen, written);
        const uint64_t D = (uint64_t)v.dst + ((uint64_t)fct[gib].dlo | ((uint64_t)fct[gib].dhi << 32));
        if (fl & SMOL_UNR_ANSWERED) {  // (the group's lanes together)
            const uint32_t rv = fct[gib].rv;
            const WinReq q = {winb + head, rr.kind & 0xffu, g.fam, g.ip_off, fct[gib].plen, fct[gib].proto & 0xffu, 0u};
            const bool v6 = q.ver_ == 6, odd = (rr.a0 & 1u) != 0;
            const uint32_t e = q.kind_ == SMOL_KIND_ETH ? 14u : 0u, iph = v6 ? 40u : 20u;
            // the data's aligned-word sum: this lane's part of [0, e2) less its part of the header bytes [0, off)
            // (off is even: record offset 2 i is the low byte of an aligned word for an even record start)
            uint32_t mine = hi2 == s1 ? acc : acc + accx;
            for (uint32_t i = lane; 2 * i < off; i += G) {
                const uint32_t b0 = winb[head + 2 * i], b1 = winb[head + 2 * i + 1];
                mine -= odd ? ((b0 << 8) + b1) : (b0 + (b1 << 8));
            }
            const uint32_t f = fold32(group_sum<G>(mine));
            const uint32_t dat = odd ? f : bswap16(f);  // the big-endian word sum of the data, folded
            // both IPv4 header checksums (Ipv4Repr::emit twice under the same caps)
            uint32_t ipck = 0, inck = 0;
            if (!v6 && caps_tx(p.caps_ipv4)) {
                ipck = ~fold32(group_sum<G>(unreach_head_words(q, rv, e, 10u, (uint32_t)lane, (uint32_t)G))) & 0xffffu;
                inck = ~fold32(group_sum<G>(unreach_head_words(q, rv, e + 28u, 10u, (uint32_t)lane, (uint32_t)G))) & 0xffffu;
            }
            // the ICMP sum: the message's head words (the quoted header with its final checksum), the data, and
            // over IPv6 the pseudo-header: the reply's addresses, its length and next header
            uint32_t hw = unreach_head_words(q, rv, e + iph, (8u + iph) / 2u, (uint32_t)lane, (uint32_t)G);
            if (v6) hw += unreach_head_words(q, rv, e + 8u, 16u, (uint32_t)lane, (uint32_t)G);
            if (lane == 0) hw += dat + inck + (v6 ? (uint32_t)P_ICMP6 + 48u + dlen : 0u);
            const uint32_t tot = group_sum<G>(hw);
            const uint32_t l4ck = caps_tx(v6 ? p.caps_icmpv6 : p.caps_icmpv4) ? (~fold32(tot) & 0xffffu) : 0u;
            if (written) {
                const uint32_t ipo = unreach_ipck_off(q.kind_, q.ver_), l4o = unreach_l4ck_off(q.kind_, q.ver_);
                const uint32_t ino = unreach_inck_off(q.kind_, q.ver_);
                const uint32_t a = (uint32_t)(D & 3u);
                const uint32_t ndw = (a + hl + 3u) / 4u;
                for (uint32_t j = lane; j < ndw; j += G) {
                    uint32_t w = 0, keep = 0;
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint32_t i = 4u * j + b - a;  // head byte (wraps below 0: >= hl)
                        if (i < hl) {
                            uint32_t x = unreach_head_byte(q, rv, i);
                            if (i == ipo) x = ipck >> 8;
                            else if (i == ipo + 1) x = ipck & 0xffu;
                            else if (i == l4o) x = l4ck >> 8;
                            else if (i == l4o + 1) x = l4ck & 0xffu;
                            else if (i == ino) x = inck >> 8;
                            else if (i == ino + 1) x = inck & 0xffu;
                            w |= x << (8u * b);
                            keep |= 0xffu << (8u * b);
                        }
                    }
                    store_dword_masked((gu8)(D - a + 4ull * j), w, keep);
                }
            }
        }
        if (lane == 0) {  // smol_csum_unreach_t: frame_len, data_off, head_len, flags
            if (written) fl |= SMOL_UNR_WRITTEN | ((stv & SMOL_ST_ACCEPT) ? SMOL_UNR_SEND : 0u);
            const uint64_t e = (uint64_t)(hl + dlen) | ((uint64_t)(off & 0xffffu) << 32) | ((uint64_t)hl << 48) | ((uint64_t)fl << 56);
            *(GMEM uint64_t*)((uint64_t)v.unr + 8ull * r) = e;
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

template <bool IMPLICIT, int G, int U>
hipError_t launch_unreach_one(const KParams& p, const UnreachArgs& v, uint32_t max_blocks, hipStream_t s) {
    constexpr uint32_t GPB = 256 / G;
    const uint64_t want = (p.n + GPB - 1) / GPB;
    const uint32_t blocks = grid_blocks(want, max_blocks);
    note_launch(KERN_UNREACH, 0, G, U);
    hipLaunchKernelGGL((unreach_kernel<G, U, IMPLICIT>), dim3(blocks), dim3(256), 0, s, p, v);
    return hipGetLastError();
}

// Shapes: the whole-segment set of the shape mapper (8 x 6, 8 x 7, 16 x 3, 16 x 4, 32 x 4, 64 x 4).
hipError_t launch_unreach(int shape, const KParams& p, const UnreachArgs& v, uint32_t max_blocks, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    const bool im = p.desc == nullptr;
    with_walk_shape<S_SEG6>(shape, [&](auto g, auto u) {
        constexpr int G = decltype(g)::value, U = decltype(u)::value;
        e = im ? launch_unreach_one<true, G, U>(p, v, max_blocks, s) : launch_unreach_one<false, G, U>(p, v, max_blocks, s);
    });
    return e;
}

}  // namespace smolcsum
