// Fused verify + ICMP echo responder (smol_csum_batch_verify_echo_reply): vcopy_kernel (csum_vcopy.hip)
// with a second sum and a fresh head.
//
// The reference's responder parses an echo request (Icmpv4Repr::parse / Icmpv6Repr::parse sum the whole
// message, src/iface/interface/ipv4.rs:320-371, ipv6.rs:399-416), builds an EchoReply around the same data
// and, on dispatch, copies the data (icmpv4.rs:506-517, icmpv6.rs:814-822) and sums it again (fill_checksum):
// two reads, one write and two sums over bytes that differ in the type byte and the checksum field.  Here
// every 16-B chunk of a record is loaded once.
//
// A group of G lanes owns a record, its chunks on the record's own 16-B grid, G * U of them per step, step 0
// holding the 128-B header window in LDS for parse_geometry (emit = false: verify's parse) — vcopy_kernel's
// form, and the copy of the data to its place behind the reply's head is vcopy_kernel's copy of a payload
// (funnel16 of a chunk and its successor, whole chunks as dwordx4 stores, the two edges byte-masked).
// * Two sums.  Each lane keeps two accumulators: the record bytes in front of the echo data, [0, data_off),
//   and the data, [data_off, span_end).  Their sum is verify's accumulator and goes to finish_gates
//   (MODE_VERIFY) unchanged, which writes the status byte.  The data's accumulator alone, with the reply's
//   own first words (type / code, a zero checksum, ident, sequence number; ICMPv6: the pseudo-header over
//   the swapped addresses and the reply's length) added, gives the reply's checksum: nothing is subtracted
//   from a folded sum, so 0x0000 and 0xffff stay apart and the value is fill_checksum's.  Each lane folds
//   its partial sum to the big-endian form before the group's reduction (one group_sum more than verify).
// * Head.  The rule (answered or not, the head's bytes with zero checksum fields) is csum_echo.h's, read
//   from the LDS window.  After the reduction every lane holds both checksums; lane j builds the j-th
//   aligned dword of the destination range [D, D + head_len) and stores it byte-masked, so no byte of d_dst
//   is read and none outside the frame is written.
// * Entry.  Lane 0 writes the record's 8-byte smol_csum_echo_t; SEND comes from the status byte
//   finish_gates hands back.
// The cap is tested before the first store.  The copy does not wait for the verdict.
#include "csum_echo.h"
#include "csum_walk.h"

namespace smolcsum {

namespace echo {

constexpr int WIN = 128;  // the header window: 16-B grid, Grid<false>
constexpr int WIN_CH = WIN / 16;

// The request as csum_echo.h reads it: addresses and MACs from the LDS window (record byte o at w[o]; all
// of them lie in front of byte 54), the message's bytes 4..7 in a register (they may lie past the window).
struct WinReq {
    const uint8_t* w;
    uint32_t kind_, ver_, ip_, dlen_, idseq_;
    __device__ __forceinline__ uint32_t kind() const { return kind_; }
    __device__ __forceinline__ uint32_t ver() const { return ver_; }
    __device__ __forceinline__ uint32_t dlen() const { return dlen_; }
    __device__ __forceinline__ uint32_t mac_dst(uint32_t j) const { return w[j]; }
    __device__ __forceinline__ uint32_t mac_src(uint32_t j) const { return w[6 + j]; }
    __device__ __forceinline__ uint32_t ethertype(uint32_t j) const { return w[12 + j]; }
    __device__ __forceinline__ uint32_t src(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 12u : 8u) + j]; }
    __device__ __forceinline__ uint32_t dst(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 16u : 24u) + j]; }
    __device__ __forceinline__ uint32_t idseq(uint32_t j) const { return (idseq_ >> (24u - 8u * j)) & 0xffu; }
};

// Aligned-word sum of the chunk's bytes inside the record range [lo, hi) (pos: chunk start relative to the
// record start): sum_chunk with a lower bound.
__device__ __forceinline__ uint32_t sum_range(const u32x4& c, int pos, int lo, int hi, uint32_t acc) {
    if (pos >= hi || pos + 16 <= lo) return acc;
    if (pos < lo || pos + 16 > hi) return sum_masked_words(c, lo - pos, hi - pos, acc);
    return add_words(c.x, add_words(c.y, add_words(c.z, add_words(c.w, acc))));
}

}  // namespace echo

template <int G, int U, bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void echo_kernel(KParams p, EchoArgs v) {
    using namespace echo;
    using vcopy::next4;
    using vcopy::store_edge;
    constexpr int GPB = 256 / G;
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "group size");
    static_assert(G * U >= WIN_CH, "step 0 holds the window");
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ Geom geo[GPB];

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

        // the request (Icmpv4Repr::parse icmpv4.rs:410, Icmpv6Repr::parse icmpv6.rs:689), the address rule
        // and the reply's geometry
        // (built where it is used, before and after the stream, so that nothing of it stays in registers)
        auto request = [&](uint32_t dlen, uint32_t idseq) { return WinReq{winb + head, rr.kind & 0xffu, g.fam, g.ip_off, dlen, idseq}; };
        uint32_t fl = 0, off = 0, plen = 0, hl = 0;
        if (!(g.st & (SMOL_ST_MALFORMED | SMOL_ST_UNSUPPORTED)) && (g.proto == P_ICMP4 || g.proto == P_ICMP6)) {
            const uint32_t t = rd(g.l4_off), code = rd(g.l4_off + 1);
            if (t == (g.proto == P_ICMP4 ? 8u : 128u) && code == 0u) {
                off = g.l4_off + 8;
                plen = g.l4_len - 8;
                fl = echo_rule(request(plen, 0u), v.bcast_v4);
                if (fl & SMOL_ECHO_ANSWERED) hl = echo_head_len(rr.kind & 0xffu, g.fam);
            }
        }
        const bool answered = (fl & SMOL_ECHO_ANSWERED) != 0;
        const bool written = answered && hl + plen <= sl.z;  // the cap test, before the first store
        const bool st = written && plen > 0;
        const uint64_t D = (uint64_t)v.dst + ((uint64_t)sl.x | ((uint64_t)sl.y << 32));
        const uint64_t Dd = D + hl;  // where the data goes
        const uint32_t sh = (uint32_t)((rr.a0 + off - Dd) & 15u);
        // destination chunk of record chunk k: data-relative position 16 k + dk0
        const int dk0 = (int)sh - (int)head - (int)off;
        // the two sums part at the data's first byte (no request: everything in the first)
        const int split = fl ? (int)off : s1;

        uint32_t acc = 0, accd = 0;
        for (uint32_t i0 = 0; i0 < nch; i0 += (uint32_t)(G * U)) {
            if (i0) load(i0, st);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                if (k < nch) {
                    const int pos = (int)(16u * k) - (int)head;
                    acc = sum_range(c[u], pos, 0, split, acc);
                    accd = sum_range(c[u], pos, split, s1, accd);
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
                    const int lo = -pos, end = (int)plen - pos;
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
        finish_gates<G, MODE_VERIFY, false, decltype(rd)>(p, g, acc + accd, rd, winb, head, rr.a0, r, lane, nullptr,
                                                          ~0ull, ~0ull, 0, nullptr, &stv);
        if (answered) {  // (the group's lanes together)
            // the reply's ICMP sum, big-endian words: this lane's data bytes (an aligned-word sum from an odd
            // address is the big-endian one, from an even address its byte swap: data_off is even), its share
            // of the pseudo-header's address words, and on lane 0 the words that are no record bytes
            const uint32_t f = fold32(accd);
            uint32_t mine = (rr.a0 & 1u) ? f : bswap16(f);
            const WinReq q = request(plen, rd(off - 4) << 24 | rd(off - 3) << 16 | rd(off - 2) << 8 | rd(off - 1));
            const bool v6 = q.ver_ == 6;
            if (v6) {
                for (uint32_t i = lane; i < 16u; i += G) {
                    const uint32_t o = head + g.addr_off + 2 * i;
                    mine += (winb[o] << 8) | winb[o + 1];
                }
            }
            if (lane == 0) mine += (q.idseq_ >> 16) + (q.idseq_ & 0xffffu) + (v6 ? 0x8100u + (uint32_t)P_ICMP6 + 8u + plen : 0u);
            const uint32_t tot = group_sum<G>(mine);
            const uint32_t l4ck = caps_tx(v6 ? p.caps_icmpv6 : p.caps_icmpv4) ? (~fold32(tot) & 0xffffu) : 0u;
            if (written) {
                const uint32_t e = q.kind_ == SMOL_KIND_ETH ? 14u : 0u;
                const uint32_t ipo = echo_ipck_off(q.kind_, q.ver_), l4o = echo_l4ck_off(q.kind_, q.ver_);
                uint32_t ipck = 0;
                if (!v6 && caps_tx(p.caps_ipv4)) ipck = ~fold32(echo_head_words(q, e, 10u)) & 0xffffu;
                const uint32_t a = (uint32_t)(D & 3u);
                const uint32_t ndw = (a + hl + 3u) / 4u;
                for (uint32_t j = lane; j < ndw; j += G) {
                    uint32_t w = 0, keep = 0;
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint32_t i = 4u * j + b - a;  // head byte (wraps below 0: >= hl)
                        if (i < hl) {
                            uint32_t x = echo_head_byte(q, i);
                            if (i == ipo) x = ipck >> 8;
                            else if (i == ipo + 1) x = ipck & 0xffu;
                            else if (i == l4o) x = l4ck >> 8;
                            else if (i == l4o + 1) x = l4ck & 0xffu;
                            w |= x << (8u * b);
                            keep |= 0xffu << (8u * b);
                        }
                    }
                    store_dword_masked((gu8)(D - a + 4ull * j), w, keep);
                }
            }
        }
        if (lane == 0) {  // smol_csum_echo_t: frame_len, data_off, head_len, flags
            if (written) fl |= SMOL_ECHO_WRITTEN | ((stv & SMOL_ST_ACCEPT) ? SMOL_ECHO_SEND : 0u);
            const uint64_t e = (uint64_t)(answered ? hl + plen : 0u) | ((uint64_t)(off & 0xffffu) << 32) | ((uint64_t)hl << 48) | ((uint64_t)fl << 56);
            *(GMEM uint64_t*)((uint64_t)v.echo + 8ull * r) = e;
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

template <bool IMPLICIT, int G, int U>
hipError_t launch_echo_one(const KParams& p, const EchoArgs& v, uint32_t max_blocks, hipStream_t s) {
    constexpr uint32_t GPB = 256 / G;
    const uint64_t want = (p.n + GPB - 1) / GPB;
    const uint32_t blocks = grid_blocks(want, max_blocks);
    note_launch(KERN_ECHO, 0, G, U);
    hipLaunchKernelGGL((echo_kernel<G, U, IMPLICIT>), dim3(blocks), dim3(256), 0, s, p, v);
    return hipGetLastError();
}

// Shapes: the whole-segment set of the shape mapper (8 x 6, 8 x 7, 16 x 3, 16 x 4, 32 x 4, 64 x 4).
hipError_t launch_echo(int shape, const KParams& p, const EchoArgs& v, uint32_t max_blocks, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    const bool im = p.desc == nullptr;
    with_walk_shape<S_SEG6>(shape, [&](auto g, auto u) {
        constexpr int G = decltype(g)::value, U = decltype(u)::value;
        e = im ? launch_echo_one<true, G, U>(p, v, max_blocks, s) : launch_echo_one<false, G, U>(p, v, max_blocks, s);
    });
    return e;
}

}  // namespace smolcsum
