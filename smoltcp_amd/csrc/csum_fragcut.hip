// Emit + fragmentation of whole IPv4 datagrams (smol_csum_batch_fragment_emit, include/smolcsum.h): the
// mirror of csum_fragcopy.hip.  Each record is one datagram; its frames (Ethernet header if any, a fresh
// IPv4 header, a slice of the payload) are written to the datagram's place in d_dst with every checksum
// filled, in one pass over the payload.
//
// On transmit the reference reads a datagram it must fragment twice: it emits it whole into frag.buffer,
// the L4 fill_checksum summing every byte (src/iface/interface/mod.rs:1263-1331), and then copies it out
// a fragment at a time behind fresh headers (mod.rs:1334-1347, dispatch_ipv4_frag,
// src/iface/interface/ipv4.rs:421-482).  Here every 16-B chunk of the payload is loaded once: the
// registers are summed and the same registers feed the stores.
//
// One wavefront per datagram, four datagrams per 256-thread workgroup; no LDS, no barrier (the frames are
// regular: frame k's payload is [k step, (k + 1) step), so there is no datagram map to share).
// The record gate, the cap / stride test, the result entry and the launcher are csum_cut.h's, shared with
// csum_tcpcut.hip.
//   1. Gate.  The wave parses the record with parse_geometry (cut::gate): the status byte, the L4 span and
//      the offsets of the fields emit writes are emit's by construction.  The cut rules and the cut (count,
//      frame lengths: a cut::Cut) are written here, the cap / stride test (cut::place) follows; a datagram
//      that is not cut or does not fit streams nothing.
//   2. Streaming.  The wave walks the frames in order (vcopy::piece_walk, csum_walk.h).  A frame's payload
//      slice is streamed as a vcopy::Piece, cut::U chunks per lane and step, all loads of a step
//      issued first, and the first step of the NEXT frame is issued before the current one is used.  Each
//      chunk is summed as aligned words (edges masked, UDP capped at its length field: the tail is
//      delivered, not summed) and funnelled onto the destination's 16-B grid.  The shift is per frame: the
//      frame length is 2 or 4 mod 8.
//   3. Frame head.  Lane i < io + 20 holds byte i of the record's headers; per frame it substitutes total
//      length, ident, flags / offset and the header checksum (computed by every lane from the six words
//      that do not change: a 10-word sum) and stores its byte.
//   4. Held-back fields.  The L4 checksum bytes (payload offset 6, 16 or 2) and an ICMPv4 error's embedded
//      header checksum (offset 18) are masked out of the streaming stores.  Once the last frame is summed
//      the wave runs finish_gates (csum_walk.h, emit's own finish, its fields sink in a register) and lane 0
//      writes each value to frame o / step at io + 20 + o % step: every byte of d_dst is written once, and
//      nothing depends on the order of two stores.  step is a multiple of 8 and the offsets are even, so
//      a field never straddles two frames.
// No byte of d_dst is read.
#include "csum_cut.h"

namespace smolcsum {
namespace fragcut {

constexpr int32_t NO_HOLD = -(1 << 30);

// One frame: its payload slice (its bytes below the L4 span's end summed) and what the frame head needs.
struct Frame : cut::Frame {
    uint32_t lo;     // datagram-payload offset of the slice
    int32_t h0, h1;  // slice-relative offsets of the held-back fields (far below 0: none)
    uint32_t more;   // another frame follows (MF)
};

// A held-back field in a destination chunk (at most one: they lie 16 apart): the bytes around it go out.
struct HeldBack {
    int32_t h0, h1;
    __device__ __forceinline__ bool operator()(gu8 dst, const u32x4& m, int pos, int lo, int end) const {
        const int a = max(lo, 0), b = min(end, 16);
        int h = h0 - pos;
        if (!(h + 2 > a && h < b)) h = h1 - pos;
        if (!(h + 2 > a && h < b)) return false;
        vcopy::store_edge(dst, m, a, h);
        vcopy::store_edge(dst, m, h + 2, b);
        return true;
    }
};

template <bool IMPLICIT>
__global__ __launch_bounds__(256) void fragcut_kernel(KParams p, FragCutArgs v) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t dummy = (uint64_t)p.dummy;
    const uint64_t nwaves = 4ull * gridDim.x;

    for (uint64_t r = 4ull * blockIdx.x + wave; r < p.n; r += nwaves) {
        // ---- 1. the gate: emit's parse, the cut, the cap ----
        const cut::Gate gt = cut::gate<IMPLICIT>(p, r);
        const cut::Rd rd = gt.rd;
        const uint64_t a0 = rd.a0;
        const Geom g = gt.g;
        const u32x4 pl = *(gcv4)((uint64_t)v.plans + 16ull * r);  // dst_offset, cap, ip_mtu | ident << 16
        const uint32_t cap = pl.z, mtu = pl.w & 0xffffu, ident = pl.w >> 16;
        const uint32_t io = g.ip_off, l4o = io + 20;
        const uint64_t ip = a0 + io;
        // cut: an IPv4 header that passed check_len (fam 4), IHL 5, not itself a fragment, ip_mtu >= 28
        bool is_cut = g.fam == 4 && g.ip_hl == 20 && mtu >= 28;
        uint32_t total = 20, id0 = 0, fl0 = 0;
        if (is_cut) {
            total = rb16(ip + 2);
            id0 = rb16(ip + 4);
            fl0 = rb16(ip + 6);
            is_cut = (fl0 & 0x3fffu) == 0;
        }
        const uint32_t T = total - 20;
        const uint32_t step = (mtu - 20) & ~7u;  // max_ipv4_fragment_size, phy/mod.rs:297-300
        const bool single = 20 + T <= mtu;        // the iface sends it as it is, mod.rs:1276
        cut::Cut ct = {0u, 0u, 0u};
        if (is_cut) {
            ct.count = single ? 1u : (T + step - 1) / step;
            ct.frame_len = single ? l4o + T : l4o + step;
            ct.last_len = l4o + T - (ct.count - 1) * (single ? 0u : step);
        }
        const cut::Place at = cut::place(ct, v.frame_stride, cap);  // before the first store
        const uint32_t count = ct.count, S = at.S;

        if (at.fits) {
            const bool l4 = g.proto != P_NONE && !(g.st & SMOL_ST_MALFORMED);
            const uint32_t span = l4 ? g.span_end - l4o : 0u;  // payload bytes summed
            const int32_t f1 = l4 ? (int32_t)g.fo : NO_HOLD;
            const int32_t f2 = g.in_off ? (int32_t)(g.in_off - l4o + 10) : NO_HOLD;
            const uint32_t pstep = single ? T : step;  // payload bytes of every frame but the last
            const uint64_t Dbase = (uint64_t)v.dst + ((uint64_t)pl.x | ((uint64_t)pl.y << 32));
            // the frame head: this lane's byte of the record's headers, and the header words no frame changes
            const uint32_t hb = rb(a0 + ((uint32_t)lane < l4o ? (uint32_t)lane : 0u));
            const uint32_t H0 = rb16(ip) + rb16(ip + 8) + rb16(ip + 12) + rb16(ip + 14) + rb16(ip + 16) + rb16(ip + 18);

            auto setup = [&](uint32_t k) -> Frame {
                Frame f;
                f.lo = k * pstep;
                const uint32_t hi = min(f.lo + pstep, T);
                f.F = Dbase + (uint64_t)k * S;
                f.q = vcopy::Piece<false>(a0 + l4o + f.lo, f.F + l4o, span > f.lo ? min(span, hi) - f.lo : 0u, hi - f.lo);
                f.h0 = f1 - (int32_t)f.lo;
                f.h1 = f2 - (int32_t)f.lo;
                f.more = k + 1 < count;
                return f;
            };
            // the io + 20 header bytes of the frame, one byte per lane
            auto head = [&](const Frame& f) {
                const uint32_t tl = 20 + f.q.copy_len;
                const uint32_t idk = single ? id0 : ident;
                const uint32_t flk = single ? fl0 : ((f.more ? 0x2000u : 0u) | (f.lo >> 3));
                const uint32_t cs = caps_tx(p.caps_ipv4) ? (~fold32(H0 + tl + idk + flk) & 0xffffu) : 0u;
                const int j = lane - (int)io;
                const uint32_t b = j == 2 ? tl >> 8 : j == 3 ? tl : j == 4 ? idk >> 8 : j == 5 ? idk
                                 : j == 6 ? flk >> 8 : j == 7 ? flk : j == 10 ? cs >> 8 : j == 11 ? cs : hb;
                if ((uint32_t)lane < l4o) ((gu8)f.F)[lane] = (uint8_t)b;
            };

            uint32_t acc = 0;  // this lane's part of the aligned-word sum over the summed payload bytes
            vcopy::piece_walk<cut::U>(count, lane, dummy, setup, cut::SliceOf{}, [&](const Frame& f, uint32_t, auto stream) {
                head(f);
                stream(acc, HeldBack{f.h0, f.h1});
            });

            // ---- 4. emit's finish over the sums, and the held-back fields ----
            if (l4) {
                // finish_gates takes the lanes' sum over [0, span_end) and removes the header bytes [0, l4_off)
                // itself: add them here, word for word as it removes them
                const bool odd = (a0 & 1u) != 0;
                for (uint32_t i = (uint32_t)lane; 2 * i < l4o; i += 64) {
                    const uint32_t e = rd(2 * i), o = rd(2 * i + 1);
                    acc += odd ? ((e << 8) + o) : (e + (o << 8));
                }
                // (its header window is the record itself here, head 0: the IPv4 header and address words are
                // read from global memory, once per datagram)
                u32x4 e = {0u, 0u, 0u, 0u};  // lane 0: smol_csum_fields_t (off[3], val[3], status)
                finish_gates<64, MODE_EMIT, false, decltype(rd), 0, false, false, false, false, true, true>(
                    p, g, acc, rd, (const uint8_t*)a0, 0u, a0, r, lane, nullptr, ~0ull, ~0ull, 0, &e);
                if (lane == 0) {
                    auto put = [&](int32_t f, uint32_t val) {
                        const uint32_t k = (uint32_t)f / pstep, o = (uint32_t)f % pstep;
                        store_be16((gu8)(Dbase + (uint64_t)k * S + l4o + o), val);
                    };
                    put(f1, e.z & 0xffffu);
                    if (f2 != NO_HOLD) put(f2, e.z >> 16);
                }
            }
        }
        cut::store_result(v.out, r, lane, ct, g.st, at.fits);
    }
}

}  // namespace fragcut

hipError_t launch_fragcut(const KParams& p, const FragCutArgs& v, hipStream_t s) {
    return cut::launch(KERN_FRAGCUT, fragcut::fragcut_kernel<true>, fragcut::fragcut_kernel<false>, p, v, s);
}

}  // namespace smolcsum
