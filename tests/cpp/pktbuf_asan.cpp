// The enqueue rule of smol_csum_batch_verify_udp_enqueue (smoltcp_amd/csrc/csum_pktbuf.h pktbuf_enqueue, the
// function udprx_kernel calls) walked on the CPU over small rings: payload capacities P 0 .. 17, metadata
// capacities M 0 .. 5, every start state the group contract allows (pl 0 .. P, pr 0 .. P - 1, ml 0 .. M,
// mr 0 .. M - 1), datagram sizes 0 .. 18, sequences of up to 4 enqueues.  Every step is compared with a plain
// restatement of PacketBuffer::enqueue over two RingBuffers with the reference's own modulo arithmetic
// (src/storage/packet_buffer.rs:80-118, src/storage/ring_buffer.rs:76-105, 181-211), and against a byte map of
// the ring: a delivered range is contiguous, inside the ring, and was free; padding and payload never overlap.
//
// A step that returns Full without a padding entry changes nothing, so the sequences that continue behind it
// are the sequences that continue from the same state one step earlier, which the walk visits anyway: the
// walk does not descend behind such a step.  Every other sequence of the sweep is walked in full.
//
// Stand-alone (its own main), built with -fsanitize=address,undefined by tests/test_pktbuf_rule_cpu.py.
// Prints "ok <steps walked> <single steps> <digest>": the digest covers the single steps (every P, M, start
// state and size, in sweep order), each step's nine words (res, ring_off, meta_idx, pad_idx, pad_size and the
// state after it) hashed with FNV-1a (64 bit, little-endian bytes), the step hashes folded d = (d ^ h) * prime.
// tests/test_pktbuf_rule_cpu.py recomputes it with tests/udp_enqueue_ref.py over the same sweep.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smoltcp_amd/csrc/csum_pktbuf.h"

using namespace smolcsum;

namespace {

constexpr uint64_t FNV_OFFSET = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;
constexpr int MAXP = 17, MAXM = 5, MAXSIZE = 18, DEPTH = 4;

// RingBuffer's counters (ring_buffer.rs:76-105)
struct Ring {
    uint32_t cap, read_at, length;
    uint32_t window() const { return cap - length; }
    uint32_t get_idx(uint32_t idx) const { return cap > 0 ? (read_at + idx) % cap : 0; }
    uint32_t contiguous_window() const {
        const uint32_t w = window(), e = cap - get_idx(length);
        return w < e ? w : e;
    }
    bool is_full() const { return window() == 0; }
    // enqueue_many (:181-211): the slice's start and its length
    uint32_t enqueue_many(uint32_t size, uint32_t* at) {
        if (length == 0) read_at = 0;
        *at = get_idx(length);
        const uint32_t max_size = contiguous_window();
        if (size > max_size) size = max_size;
        length += size;
        return size;
    }
};

struct Plain {
    Ring meta, pay;
    // PacketBuffer::enqueue (packet_buffer.rs:80-118)
    PktBufStep enqueue(uint32_t size) {
        PktBufStep r = {PKTBUF_FULL, 0, 0, 0, 0};
        if (pay.cap < size || meta.is_full()) return r;
        if (pay.length == 0) pay.read_at = 0;  // payload_ring.clear()
        const uint32_t window = pay.window(), contig = pay.contiguous_window();
        if (window < size) return r;
        if (contig < size) {
            if (window - contig < size) return r;
            r.res |= PKTBUF_PADDED;  // metadata_ring.enqueue_one()?: not full, tested above
            r.pad_idx = meta.get_idx(meta.length);
            r.pad_size = contig;
            meta.length += 1;
            uint32_t at;
            (void)pay.enqueue_many(contig, &at);
        }
        if (meta.is_full()) return r;  // metadata_ring.enqueue_one()?
        r.meta_idx = meta.get_idx(meta.length);
        meta.length += 1;
        const uint32_t got = pay.enqueue_many(size, &r.ring_off);
        if (got != size) {  // debug_assert!(payload_buf.len() == size)
            std::printf("FAIL the restatement's slice is short\n");
            std::exit(1);
        }
        r.res = (r.res & PKTBUF_PADDED) | PKTBUF_OK;
        return r;
    }
};

unsigned long long g_steps = 0, g_singles = 0;
uint64_t g_digest = FNV_OFFSET;

[[noreturn]] void fail(const char* what, int P, int M, const PktBufState& s, int size, int depth) {
    std::printf("FAIL %s: P %d, M %d, state (%u, %u, %u, %u), size %d, depth %d\n", what, P, M, s.pr, s.pl, s.mr, s.ml, size, depth);
    std::exit(1);
}

// owner: one byte per ring byte, 0 free, 1 occupied before the walk, 2 padding, 3 payload
void walk(int P, int M, const PktBufState& s0, const uint8_t* owner0, int depth) {
    for (int size = 0; size <= MAXSIZE; ++size) {
        PktBufState s = s0;
        const PktBufStep e = pktbuf_enqueue((uint32_t)P, (uint32_t)M, s, (uint32_t)size);
        Plain q = {{(uint32_t)M, s0.mr, s0.ml}, {(uint32_t)P, s0.pr, s0.pl}};
        const PktBufStep w = q.enqueue((uint32_t)size);
        ++g_steps;
        if (e.res != w.res || e.ring_off != w.ring_off || e.meta_idx != w.meta_idx || e.pad_idx != w.pad_idx ||
            e.pad_size != w.pad_size)
            fail("step differs from the restatement", P, M, s0, size, depth);
        if (s.pr != q.pay.read_at || s.pl != q.pay.length || s.mr != q.meta.read_at || s.ml != q.meta.length)
            fail("state differs from the restatement", P, M, s0, size, depth);
        if (!pktbuf_state_valid((uint32_t)P, (uint32_t)M, s)) fail("state leaves the contract", P, M, s0, size, depth);
        if (depth == 0) {
            const uint32_t words[9] = {e.res, e.ring_off, e.meta_idx, e.pad_idx, e.pad_size, s.pr, s.pl, s.mr, s.ml};
            uint64_t h = FNV_OFFSET;
            for (uint32_t x : words)
                for (int b = 0; b < 4; ++b) h = (h ^ ((x >> (8 * b)) & 0xffu)) * FNV_PRIME;
            g_digest = (g_digest ^ h) * FNV_PRIME;
            ++g_singles;
        }
        const bool ok = (e.res & PKTBUF_OK) != 0, full = (e.res & PKTBUF_FULL) != 0, padded = (e.res & PKTBUF_PADDED) != 0;
        if (ok == full) fail("neither or both of OK and FULL", P, M, s0, size, depth);
        if (!padded && full) {
            if (std::memcmp(&s, &s0, sizeof s) != 0) fail("a plain Full changed the state", P, M, s0, size, depth);
            continue;  // (see the header comment: nothing new lies behind it)
        }
        uint8_t owner[MAXP + 1];
        std::memcpy(owner, owner0, sizeof owner);
        if (padded) {
            if (e.pad_idx >= (uint32_t)M || e.pad_size == 0) fail("padding entry", P, M, s0, size, depth);
            // the padding closes the ring's end: it starts at the write index and ends at P
            const uint32_t at = (s0.pr + s0.pl) % (uint32_t)P;  // (s0.pl > 0: an empty ring never pads)
            if (at + e.pad_size != (uint32_t)P) fail("padding does not end at the ring's end", P, M, s0, size, depth);
            for (uint32_t i = at; i < at + e.pad_size; ++i) {
                if (owner[i]) fail("padding over a used byte", P, M, s0, size, depth);
                owner[i] = 2;
            }
            if (ok && e.ring_off != 0) fail("a padded datagram does not start at 0", P, M, s0, size, depth);
            if (ok && e.meta_idx != (e.pad_idx + 1) % (uint32_t)M) fail("packet entry not behind its padding", P, M, s0, size, depth);
        }
        if (ok) {
            if (e.meta_idx >= (uint32_t)M) fail("metadata index", P, M, s0, size, depth);
            if ((uint64_t)e.ring_off + (uint32_t)size > (uint32_t)P) fail("range leaves the ring", P, M, s0, size, depth);
            for (uint32_t i = e.ring_off; i < e.ring_off + (uint32_t)size; ++i) {
                if (owner[i]) fail("payload over a used byte", P, M, s0, size, depth);
                owner[i] = 3;
            }
        }
        uint32_t used = 0;
        for (int i = 0; i < P; ++i) used += owner[i] != 0;
        if (used != s.pl) fail("payload_len is not the bytes in use", P, M, s0, size, depth);
        if (depth + 1 < DEPTH) walk(P, M, s, owner, depth + 1);
    }
}

}  // namespace

int main() {
    for (int P = 0; P <= MAXP; ++P)
        for (int M = 0; M <= MAXM; ++M)
            for (int pr = 0; pr < (P ? P : 1); ++pr)
                for (int pl = 0; pl <= P; ++pl)
                    for (int mr = 0; mr < (M ? M : 1); ++mr)
                        for (int ml = 0; ml <= M; ++ml) {
                            const PktBufState s = {(uint32_t)pr, (uint32_t)pl, (uint32_t)mr, (uint32_t)ml};
                            uint8_t owner[MAXP + 1] = {};
                            for (int i = 0; i < pl; ++i) owner[(pr + i) % P] = 1;
                            walk(P, M, s, owner, 0);
                        }
    std::printf("ok %llu %llu %016llx\n", g_steps, g_singles, (unsigned long long)g_digest);
    return 0;
}
