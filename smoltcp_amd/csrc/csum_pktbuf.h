// The enqueue rule of smol_csum_batch_verify_udp_enqueue (include/smolcsum.h): where a UDP socket's
// PacketBuffer puts the next datagram.  Plain host / device functions with no HIP in them, so that the text
// udprx_kernel (csum_udprx.hip) runs is walked on the CPU under the sanitizers (tests/cpp/pktbuf_asan.cpp).
//
// PacketBuffer::enqueue (src/storage/packet_buffer.rs:80-118) over its two RingBuffers
// (src/storage/ring_buffer.rs:76-105 window / contiguous_window / get_idx, :181-211 enqueue_many), statement
// for statement.  State: the capacities P (payload bytes) and M (metadata entries), and
// (pr, pl, mr, ml) = (payload read_at, payload length, metadata read_at, metadata length).  For a datagram
// of `size` bytes:
//   1. P < size or ml == M: Full, nothing changes (packet_buffer.rs:81-83).
//   2. pl == 0: pr = 0 (:87-89, RingBuffer::clear).
//   3. window = P - pl; widx = P ? (pr + pl) % P : 0; contig = min(window, P - widx) (:91-92).
//   4. window < size: Full (:94-95).
//   5. else contig < size: window - contig < size: Full (:97-102); otherwise a PADDING(contig) entry goes to
//      metadata index (mr + ml) % M, ml += 1, pl += contig (:106-109).
//   6. ml == M: Full; the padding stays (the `?` of :113).
//   7. the PACKET entry goes to metadata index (mr + ml) % M, ml += 1; ring_off = (pr + pl) % P, or 0 when
//      P == 0; pl += size (:113-117).
// A delivered payload is one contiguous piece: step 5 leaves contig >= size at the ring's front.
//
// The state the caller hands over obeys pl <= P, ml <= M, pr < P (or pr == 0 with P == 0) and the same for
// mr (the group contract), and every step keeps that.  Under it pr + pl < 2 P and mr + ml < 2 M, so each
// modulo above is one conditional subtraction (pktbuf_wrap): a 64-bit division per datagram is what the
// kernel's serial loop must not pay.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SMOL_PKTBUF_FN __host__ __device__ inline
#else
#define SMOL_PKTBUF_FN inline
#endif

namespace smolcsum {

struct PktBufState {
    uint32_t pr, pl, mr, ml;
};

// What one enqueue did.  res: PKTBUF_OK, PKTBUF_FULL, each with or without PKTBUF_PADDED.
constexpr uint32_t PKTBUF_OK = 1u, PKTBUF_FULL = 2u, PKTBUF_PADDED = 4u;
struct PktBufStep {
    uint32_t res;
    uint32_t ring_off;  // OK: payload-ring index of the datagram's first byte
    uint32_t meta_idx;  // OK: metadata-ring index of its PACKET entry
    uint32_t pad_idx;   // PADDED: metadata-ring index of the PADDING entry
    uint32_t pad_size;  // PADDED: its size (the contiguous window it closes)
};

// (a + b) % n for a < n, b <= n (n > 0); 0 for n == 0: RingBuffer::get_idx.
SMOL_PKTBUF_FN uint32_t pktbuf_wrap(uint32_t a, uint32_t b, uint32_t n) {
    const uint64_t s = (uint64_t)a + b;
    return n == 0 ? 0u : (uint32_t)(s >= n ? s - n : s);
}

SMOL_PKTBUF_FN PktBufStep pktbuf_enqueue(uint32_t P, uint32_t M, PktBufState& s, uint32_t size) {
    PktBufStep r = {PKTBUF_FULL, 0u, 0u, 0u, 0u};
    if (P < size || s.ml == M) return r;                     // 1
    if (s.pl == 0) s.pr = 0;                                 // 2
    const uint32_t window = P - s.pl;                        // 3
    const uint32_t widx = pktbuf_wrap(s.pr, s.pl, P);
    const uint32_t contig = window < P - widx ? window : P - widx;
    if (window < size) return r;                             // 4
    if (contig < size) {                                     // 5
        if (window - contig < size) return r;
        r.res |= PKTBUF_PADDED;
        r.pad_idx = pktbuf_wrap(s.mr, s.ml, M);
        r.pad_size = contig;
        s.ml += 1;
        s.pl += contig;
    }
    if (s.ml == M) return r;                                 // 6
    r.meta_idx = pktbuf_wrap(s.mr, s.ml, M);                 // 7
    s.ml += 1;
    r.ring_off = pktbuf_wrap(s.pr, s.pl, P);
    s.pl += size;
    r.res = (r.res & PKTBUF_PADDED) | PKTBUF_OK;
    return r;
}

// The group contract on a socket's ring state.
SMOL_PKTBUF_FN bool pktbuf_state_valid(uint32_t P, uint32_t M, const PktBufState& s) {
    return s.pl <= P && s.ml <= M && (P ? s.pr < P : s.pr == 0) && (M ? s.mr < M : s.mr == 0);
}

// The dequeue rule of smol_csum_batch_udp_dequeue_emit (include/smolcsum.h): which datagram a UDP socket's
// PacketBuffer hands out next, the text udptx_kernel (csum_udptx.hip) runs and tests/cpp/pktbuf_dequeue_asan.cpp
// walks.
//
// PacketBuffer::dequeue_with (src/storage/packet_buffer.rs:169-204) over the same two RingBuffers
// (src/storage/ring_buffer.rs:145-161 dequeue_one_with, :239-268 dequeue_many_with), statement for statement,
// in two halves, because the closure between them (UdpSocket::dispatch's emit, src/socket/udp.rs:535-592) may
// fail and then the packet stays queued (packet_buffer.rs:199):
//   pktbuf_front   1. dequeue_padding (:156-167): when ml > 0 and the entry at mr is PADDING,
//                     n = min(size, pl, P - pr) (dequeue_many's clamp); pr = (pr + n) % P, or 0 when P == 0;
//                     pl -= n; mr = (mr + 1) % M; ml -= 1.  This happens whatever follows.
//                  2. ml == 0: Empty (:176, dequeue_one_with's Err).
//                  3. the entry at mr must be PACKET, of family 4 or 6, with size <= min(pl, P - pr): the
//                     `unwrap` of :185 and the debug_assert of :191.  Otherwise Corrupt, nothing more changes.
//                     Else the datagram is payload-ring bytes [pr, pr + size), its entry is at mr.
//   pktbuf_take    4. the closure returned Ok: pr = (pr + size) % P; pl -= size; mr = (mr + 1) % M; ml -= 1.
// pktbuf_dequeue is both: PacketBuffer::dequeue (:207-209).  Under the group contract pr + size <= P and
// mr + 1 <= M, so each modulo is pktbuf_wrap's conditional subtraction here too.
constexpr uint32_t PKTBUF_KIND_PACKET = 1u, PKTBUF_KIND_PADDING = 2u;  // SMOL_UMETA_*
// What the rule reads of a metadata entry.
struct PktBufEntry {
    uint32_t size, kind, family;
};
// What one dequeue found.  res: PKTBUF_OK, PKTBUF_EMPTY or PKTBUF_CORRUPT, each with or without PKTBUF_PADDED
// (a PADDING entry was dequeued in front).
constexpr uint32_t PKTBUF_EMPTY = 8u, PKTBUF_CORRUPT = 16u;
struct PktBufFront {
    uint32_t res;
    uint32_t ring_off;  // OK: payload-ring index of the datagram's first byte
    uint32_t meta_idx;  // OK: metadata-ring index of its PACKET entry
    uint32_t size;      // OK: its payload bytes
    uint32_t family;    // OK: 4 or 6
};

// AT: PktBufEntry at(uint32_t metadata-ring index).
template <class AT>
SMOL_PKTBUF_FN PktBufFront pktbuf_front(uint32_t P, uint32_t M, PktBufState& s, const AT& at) {
    PktBufFront r = {0u, 0u, 0u, 0u, 0u};
    if (s.ml > 0) {                                           // 1
        const PktBufEntry e = at(s.mr);
        if (e.kind == PKTBUF_KIND_PADDING) {
            uint32_t n = e.size < s.pl ? e.size : s.pl;
            n = n < P - s.pr ? n : P - s.pr;
            s.pr = pktbuf_wrap(s.pr, n, P);
            s.pl -= n;
            s.mr = pktbuf_wrap(s.mr, 1u, M);
            s.ml -= 1;
            r.res |= PKTBUF_PADDED;
        }
    }
    if (s.ml == 0) {                                          // 2
        r.res |= PKTBUF_EMPTY;
        return r;
    }
    const PktBufEntry e = at(s.mr);                           // 3
    const uint32_t contig = s.pl < P - s.pr ? s.pl : P - s.pr;
    if (e.kind != PKTBUF_KIND_PACKET || (e.family != 4u && e.family != 6u) || e.size > contig) {
        r.res |= PKTBUF_CORRUPT;
        return r;
    }
    r.res |= PKTBUF_OK;
    r.ring_off = s.pr;
    r.meta_idx = s.mr;
    r.size = e.size;
    r.family = e.family;
    return r;
}

SMOL_PKTBUF_FN void pktbuf_take(uint32_t P, uint32_t M, PktBufState& s, uint32_t size) {  // 4
    s.pr = pktbuf_wrap(s.pr, size, P);
    s.pl -= size;
    s.mr = pktbuf_wrap(s.mr, 1u, M);
    s.ml -= 1;
}

template <class AT>
SMOL_PKTBUF_FN PktBufFront pktbuf_dequeue(uint32_t P, uint32_t M, PktBufState& s, const AT& at) {
    const PktBufFront r = pktbuf_front(P, M, s, at);
    if (r.res & PKTBUF_OK) pktbuf_take(P, M, s, r.size);
    return r;
}

}  // namespace smolcsum
