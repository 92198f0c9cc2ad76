// UDP sockets' transmit buffers drained into frames (smol_csum_batch_udp_dequeue_emit, include/smolcsum.h): the
// send-side mirror of csum_udprx.hip.  Each group is one socket's transmit PacketBuffer: a payload ring in d_src
// and a ring of 48-byte metadata entries in d_meta.  The datagrams are dequeued in order and each one is written
// to the socket's place in d_dst as a whole frame: Ethernet header (optional), IPv4 or IPv6 header, UDP header,
// all built here from the socket entry and the metadata entry, both checksums filled, then the payload, in one
// pass over the payload.
//
// In the reference such a burst is repeated UdpSocket::dispatch calls within one poll (src/socket/udp.rs:535-592):
// tx_buffer.dequeue_with skips a padding entry and hands out one contiguous payload
// (src/storage/packet_buffer.rs:169-204), dispatch_ip writes the Ethernet and IP headers
// (src/iface/interface/mod.rs:1245-1268, 1359-1395; src/wire/ipv4.rs:584-611, src/wire/ipv6.rs:628-640),
// UdpRepr::emit copies the payload and fill_checksum sums it again (src/wire/udp.rs:286-309, 194-208).  Here every
// 16-B chunk of a payload is loaded once: the registers are summed and the same registers feed the stores.
//
// One 256-thread workgroup per socket (udprx_kernel's shape), grid-stride over sockets.
//   0. The socket entry (96 B, the same for every thread) and its validity: an invalid group is left by the
//      whole workgroup before the first barrier.
//   1. Thread j loads metadata entry (mr + j) % M into LDS, whole (the rule reads its first 16 bytes, the heads
//      its addresses): at most 2 * max_dgrams entries, because a call dequeues at most max_dgrams PACKET entries
//      and at most one PADDING entry in front of each (a second one is CORRUPT).
//   2. Barrier.  Thread 0 runs the dequeue rule (csum_pktbuf.h pktbuf_front / pktbuf_take) and the placement
//      (OVERSIZE, NOSPACE, the frame offsets) over the entries in LDS: every dequeued datagram's d_tx entry goes
//      to LDS, the group entry to d_out.  At most 256 + padding serial iterations, all in LDS.
//   3. Barrier.  Thread k writes d_tx entry k.  Wave w streams SENT datagrams w, w + 4, ... (an OVERSIZE one takes no turn) with
//      vcopy::piece_walk (csum_walk.h: the cut kernels' pipeline), U chunks per lane and step, the first step of
//      the wave's NEXT frame issued before the current one is used.  The slice's sum is reduced across the wave
//      once it is streamed: the lanes sum aligned little-endian words, so for a slice at an even source address
//      the folded sum is byte-swapped into the header's big-endian words, at an odd one it already is (RFC 1071
//      2(B)).  Then the head, one big-endian word per lane (at most 31): the lane takes its word from the
//      constants, the socket entry or the metadata entry in LDS, one wave reduction over the address words gives
//      the pseudo-header's and the IPv4 header's sums, and the word is stored (one 2-byte store per lane where the
//      frame starts even, two byte stores where it starts odd).  The head goes out after its frame's slice
//      because it carries the slice's sum (tcpcut_kernel's order).
// Stores and cache policy are the cut kernels': plain loads and stores, dwordx4 inside a slice, byte-masked edges,
// nothing read back from d_dst.
#include "csum_fraggroup.h"
#include "csum_pktbuf.h"

namespace smolcsum {
namespace udptx {

using fraggroup::lds_sync;

// Chunks per lane and step: a 1472-B payload (92 or 93 chunks) is one step, as in the cut kernels.
constexpr int U = 2;
constexpr uint32_t MAXD = SMOL_MAX_SOCKET_DGRAMS;
constexpr uint32_t MAXE = 2 * MAXD;  // metadata entries a call can consume
static_assert(MAXD <= 256, "thread k holds d_tx entry k");
static_assert(sizeof(smol_csum_udptxsock_t) == 96 && sizeof(smol_csum_udpmeta_t) == 48 && sizeof(smol_csum_udptx_t) == 16 &&
                  sizeof(smol_csum_udptxout_t) == 32,
              "entry layouts");
static_assert(PKTBUF_KIND_PACKET == SMOL_UMETA_PACKET && PKTBUF_KIND_PADDING == SMOL_UMETA_PADDING, "the rule's entry kinds");

// One SENT datagram as its wave streams it: the payload slice and what the head needs.
struct Frame {
    vcopy::Piece<false> q;  // the slice: all of it summed and delivered
    uint64_t F;             // destination address of the frame's first byte
    uint32_t e;             // LDS index of its metadata entry
    uint32_t size, fam;
};
struct SliceOf {
    __device__ __forceinline__ const vcopy::Piece<false>& operator()(const Frame& f) const { return f.q; }
};

__global__ __launch_bounds__(256) void udptx_kernel(UdpTxArgs v, uint64_t ngroups) {
    __shared__ u32x4 s_ent[MAXE][3];  // metadata entries (mr + j) % M: size, record, port | family | kind; remote; local
    __shared__ u32x4 s_tx[MAXD];      // smol_csum_udptx_t k: frame_off, ring_off, meta_idx, ip_len | flags << 16
    __shared__ uint16_t s_eidx[MAXD]; // ... and the LDS index of its metadata entry
    __shared__ uint16_t s_sent[MAXD]; // the SENT ones among them, in order: their k
    __shared__ uint32_t s_ntx, s_nsent;
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t dummy = (uint64_t)v.dummy;
    const uint32_t S = v.frame_stride;
    const bool udp_tx = caps_tx(v.caps_udp), ip_tx = caps_tx(v.caps_ipv4);

    for (uint64_t gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
        // ---- 0. the socket entry ----
        const uint64_t sock = (uint64_t)v.socks + 96ull * gi;
        const u32x4 a0 = *(gcv4)sock;          // src_offset, meta_first
        const u32x4 a1 = *(gcv4)(sock + 16u);  // dst_offset, tx_first
        const u32x4 a2 = *(gcv4)(sock + 32u);  // payload_cap, _read, _len, meta_cap
        const u32x4 a3 = *(gcv4)(sock + 48u);  // meta_read, meta_len, dst_cap, max_dgrams
        const u32x4 a4 = *(gcv4)(sock + 64u);  // port | ip_mtu << 16, hop_limit | flags << 8 | eth_dst ..
        const u32x4 a5 = *(gcv4)(sock + 80u);  // .. eth_src | reserved
        const uint32_t P = a2.x, M = a2.w, dst_cap = a3.z, maxd = a3.w;
        const uint32_t port = a4.x & 0xffffu, mtu = a4.x >> 16, hop = a4.y & 0xffu, flags = (a4.y >> 8) & 0xffu;
        const PktBufState s0 = {a2.y, a2.z, a3.x, a3.y};
        const bool ok = (a5.x >> 16) == 0 && (a5.y | a5.z | a5.w) == 0 && (flags & ~SMOL_UTXS_ETH) == 0 && maxd >= 1 &&
                        maxd <= MAXD && pktbuf_state_valid(P, M, s0);
        // an invalid group: its entry is zero.  The whole workgroup leaves here.
        if (!ok) {
            if (tid < 2) *(GMEM u32x4*)((uint64_t)v.out + 32ull * gi + 16u * tid) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }
        const uint64_t Sbase = (uint64_t)v.src + ((uint64_t)a0.x | ((uint64_t)a0.y << 32));
        const uint64_t meta = (uint64_t)v.meta + 48ull * ((uint64_t)a0.z | ((uint64_t)a0.w << 32));
        const uint64_t Dbase = (uint64_t)v.dst + ((uint64_t)a1.x | ((uint64_t)a1.y << 32));
        const uint64_t txb = (uint64_t)v.tx + 16ull * ((uint64_t)a1.z | ((uint64_t)a1.w << 32));
        const uint32_t io = (flags & SMOL_UTXS_ETH) ? 14u : 0u;
        // this lane's word of the Ethernet addresses (eth_dst, eth_src: bytes 70 .. 81 of the entry)
        const uint32_t ethw = io && lane < 6 ? rb16(sock + 70u + 2u * (uint32_t)lane) : 0u;

        // ---- 1. the metadata entries the call can consume ----
        const uint32_t nload = min(s0.ml, 2u * maxd);
        for (uint32_t j = tid; j < nload; j += 256u) {
            const uint64_t a = meta + 48ull * pktbuf_wrap(s0.mr, j, M);
            s_ent[j][0] = *(gcv4)a;
            s_ent[j][1] = *(gcv4)(a + 16u);
            s_ent[j][2] = *(gcv4)(a + 32u);
        }
        lds_sync();  // (all threads)

        // ---- 2. the dequeue rule and the placement ----
        if (tid == 0) {
            PktBufState s = s0;
            auto lds_of = [&](uint32_t idx) -> uint32_t { return idx >= s0.mr ? idx - s0.mr : idx + (M - s0.mr); };
            auto at = [&](uint32_t idx) -> PktBufEntry {
                const u32x4 w = s_ent[lds_of(idx)][0];
                return {w.x, w.z >> 24, (w.z >> 16) & 0xffu};
            };
            uint32_t k = 0, sent = 0, over = 0, stop;
            uint64_t next = 0;  // where the next frame starts, relative to dst_offset
            for (;;) {
                if (k == maxd) {
                    stop = SMOL_UTX_STOP_MAX;
                    break;
                }
                const PktBufFront f = pktbuf_front(P, M, s, at);
                if (f.res & (PKTBUF_EMPTY | PKTBUF_CORRUPT)) {
                    stop = (f.res & PKTBUF_EMPTY) ? SMOL_UTX_STOP_EMPTY : SMOL_UTX_STOP_CORRUPT;
                    break;
                }
                const uint64_t ip_len = (f.family == 4u ? 28u : 48u) + (uint64_t)f.size;
                uint32_t fl = (f.res & PKTBUF_PADDED) ? SMOL_UTX_PADDED : 0u, ipl = 0;
                if (ip_len > mtu) {
                    fl |= SMOL_UTX_OVERSIZE;
                    ++over;
                } else {
                    if (next + io + ip_len > dst_cap || (S != 0 && io + ip_len > S)) {
                        stop = SMOL_UTX_STOP_NOSPACE;
                        break;
                    }
                    fl |= SMOL_UTX_SENT;
                    ipl = (uint32_t)ip_len;
                }
                pktbuf_take(P, M, s, f.size);
                s_tx[k] = u32x4{(uint32_t)min(next, (uint64_t)0xffffffffu), f.ring_off, f.meta_idx, ipl | fl << 16};
                s_eidx[k] = (uint16_t)lds_of(f.meta_idx);
                if (fl & SMOL_UTX_SENT) {
                    s_sent[sent] = (uint16_t)k;
                    ++sent;
                    next = S != 0 ? (uint64_t)sent * S : next + io + ip_len;
                }
                ++k;
            }
            s_ntx = k;
            s_nsent = sent;
            // smol_csum_udptxout_t: the state after the call, the counts, bytes, stop | valid << 8
            *(GMEM u32x4*)((uint64_t)v.out + 32ull * gi) = u32x4{s.pr, s.pl, s.mr, s.ml};
            *(GMEM u32x4*)((uint64_t)v.out + 32ull * gi + 16u) =
                u32x4{sent, over, (uint32_t)min(next, (uint64_t)0xffffffffu), stop | 1u << 8};
        }
        lds_sync();  // (all threads)

        // ---- 3. the entries, and the frames ----
        const uint32_t ntx = s_ntx;
        if (tid < ntx) *(GMEM u32x4*)(txb + 16ull * tid) = s_tx[tid];

        auto setup = [&](uint32_t j) -> Frame {
            const uint32_t k = s_sent[wave + 4u * j];
            const u32x4 t = s_tx[k];
            Frame f;
            f.e = s_eidx[k];
            const u32x4 w0 = s_ent[f.e][0];
            f.size = w0.x;
            f.fam = (w0.z >> 16) & 0xffu;
            f.F = Dbase + t.x;
            f.q = vcopy::Piece<false>(Sbase + t.y, f.F + io + (f.fam == 4u ? 28u : 48u), f.size, f.size);
            return f;
        };
        // the frame's head, one big-endian word per lane; pay: the big-endian word sum of its payload
        auto head = [&](const Frame& f, uint32_t pay) {
            const uint8_t* eb = reinterpret_cast<const uint8_t*>(&s_ent[f.e][0]);
            const bool v4 = f.fam == 4u;
            const int iw = lane - (int)(io / 2);   // word index in the IP header
            const int uw = iw - (v4 ? 10 : 20);    // word index in the UDP header
            const uint32_t nw = io / 2 + (v4 ? 14u : 24u);
            // the address words: source = local_addr (entry bytes 32 ..), destination = remote_addr (16 ..)
            const int na = v4 ? 2 : 8, a0w = v4 ? 6 : 4;  // words per address, the first address word
            int ao = -1;
            if (iw >= a0w && iw < a0w + na) ao = 32 + 2 * (iw - a0w);
            else if (iw >= a0w + na && iw < a0w + 2 * na) ao = 16 + 2 * (iw - a0w - na);
            const uint32_t aw = ao >= 0 ? (uint32_t)eb[ao] << 8 | (uint32_t)eb[ao + 1] : 0u;
            const uint32_t A = group_sum<64>(aw);
            const uint32_t dport = (uint32_t)eb[8] | (uint32_t)eb[9] << 8;  // the entry's src_port
            const uint32_t ul = 8u + f.size, ipl = (v4 ? 20u : 0u) + ul;
            uint32_t ucs = 0;
            if (udp_tx) {  // pseudo-header, header, payload; 0 goes out as 0xffff (udp.rs:194-208)
                ucs = ~fold32(A + P_UDP + ul + port + dport + ul + pay) & 0xffffu;
                ucs = ucs ? ucs : 0xffffu;
            }
            const uint32_t ttl = hop << 8 | P_UDP;
            const uint32_t ics = ip_tx ? (~fold32(0x4500u + ipl + 0x4000u + ttl + A) & 0xffffu) : 0u;
            uint32_t w;
            if (iw < 0) w = lane < 6 ? ethw : v4 ? 0x0800u : 0x86DDu;
            else if (uw >= 0) w = uw == 0 ? port : uw == 1 ? dport : uw == 2 ? ul : ucs;
            else if (ao >= 0) w = aw;
            else if (v4) w = iw == 0 ? 0x4500u : iw == 1 ? ipl : iw == 3 ? 0x4000u : iw == 4 ? ttl : iw == 5 ? ics : 0u;
            else w = iw == 0 ? 0x6000u : iw == 2 ? ul : iw == 3 ? (P_UDP << 8 | hop) : 0u;
            if ((uint32_t)lane < nw) store_be16((gu8)(f.F + 2u * (uint32_t)lane), w);
        };

        const uint32_t nsent = s_nsent;
        const uint32_t mine = nsent > wave ? (nsent - wave + 3u) / 4u : 0u;  // this wave's frames
        vcopy::piece_walk<U>(mine, lane, dummy, setup, SliceOf{}, [&](const Frame& f, uint32_t, auto stream) {
            uint32_t acc = 0;     // this lane's part of the aligned-word sum over the payload
            stream(acc, vcopy::NoHold{});
            // (a lane sums at most 65 chunks of a 65507-B payload: no wrap; folded before the wave's sum)
            const uint32_t le = fold32(group_sum<64>(fold32(acc)));
            head(f, f.q.odd() ? le : bswap16(le));
        });
        lds_sync();  // (all threads) the next group's entries rewrite the arrays
    }
}

}  // namespace udptx

hipError_t launch_udptx(const UdpTxArgs& v, uint64_t ngroups, uint32_t max_blocks, hipStream_t s) {
    const uint32_t blocks = grid_blocks(ngroups, max_blocks);
    note_launch(KERN_UDPTX, 0, 64, udptx::U);
    hipLaunchKernelGGL(udptx::udptx_kernel, dim3(blocks), dim3(256), 0, s, v, ngroups);
    return hipGetLastError();
}

}  // namespace smolcsum
