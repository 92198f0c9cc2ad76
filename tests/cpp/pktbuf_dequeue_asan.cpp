// The dequeue rule of smol_csum_batch_udp_dequeue_emit (smoltcp_amd/csrc/csum_pktbuf.h pktbuf_front,
// pktbuf_take, pktbuf_dequeue: the functions udptx_kernel calls) walked on the CPU over small rings: payload
// capacities P 0 .. 17, metadata capacities M 0 .. 5, every start state the group contract allows (pl 0 .. P,
// pr 0 .. P - 1, ml 0 .. M, mr 0 .. M - 1), and for each of them 57 metadata rings: the front entry takes every
// kind (PACKET, PADDING, invalid) and every size 0 .. 18, the entries behind it follow from those two (below),
// so that runs of packets, paddings between packets, padding after padding and invalid entries in every
// position all occur.  Over each ring pktbuf_dequeue runs up to 4 times.  Every step is compared with a plain
// restatement of PacketBuffer::dequeue_with over two RingBuffers with the reference's own modulo arithmetic
// (src/storage/packet_buffer.rs:156-204, src/storage/ring_buffer.rs:145-161, 239-268); a handed-out range must
// lie inside the ring's allocated bytes in one piece; and pktbuf_front alone (the closure failed) must leave the
// packet queued and differ from the full step by pktbuf_take only.
//
// Stand-alone (its own main), built with -fsanitize=address,undefined by tests/test_pktbuf_dequeue_rule_cpu.py.
// Prints "ok <steps walked> <single steps> <digest>": the digest covers the single steps (the first step of
// every run, in sweep order), each step's nine words (res, ring_off, meta_idx, size, family and the state after
// it) hashed with FNV-1a (64 bit, little-endian bytes), the step hashes folded d = (d ^ h) * prime.
// tests/test_pktbuf_dequeue_rule_cpu.py recomputes it with tests/udp_dequeue_ref.py over the same sweep.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../smoltcp_amd/csrc/csum_pktbuf.h"

using namespace smolcsum;

namespace {

constexpr uint64_t FNV_OFFSET = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;
constexpr int MAXP = 17, MAXM = 5, MAXSIZE = 18, DEPTH = 4;

// The ring for (k0, z0): the entry j places behind the front one (ring index (mr + j) % M) has kind code
// (k0 + j * (1 + z0 % 3)) % 3 (0 PACKET, 1 PADDING, 2 invalid), size (z0 + 7 j) % 19, and t = (z0 + j) % 3
// chooses the family of a PACKET entry (4, 6, 4) and the flavour of an invalid one (kind 0, kind 3, a PACKET
// entry of family 5).
PktBufEntry entry_of(int k0, int z0, int j) {
    const int code = (k0 + j * (1 + z0 % 3)) % 3, t = (z0 + j) % 3;
    const uint32_t size = (uint32_t)((z0 + 7 * j) % (MAXSIZE + 1));
    if (code == 0) return {size, PKTBUF_KIND_PACKET, t == 1 ? 6u : 4u};
    if (code == 1) return {size, PKTBUF_KIND_PADDING, 0u};
    return {size, t == 0 ? 0u : t == 1 ? 3u : PKTBUF_KIND_PACKET, 5u};
}

// RingBuffer's counters (ring_buffer.rs:76-105) and the two dequeues the packet buffer uses
struct Ring {
    uint32_t cap, read_at, length;
    // dequeue_one_with's Ok arm (:145-161) / dequeue_many_with with f returning `size` (:239-268): the start
    // and the length of the slice handed out
    uint32_t dequeue_many(uint32_t size, uint32_t* at) {
        const uint32_t cap_left = cap - read_at;
        uint32_t max_size = cap_left < length ? cap_left : length;
        if (size > max_size) size = max_size;
        *at = read_at;
        read_at = cap > 0 ? (read_at + size) % cap : 0;
        length -= size;
        return size;
    }
    void dequeue_one() {
        read_at = (read_at + 1) % cap;  // (length > 0, so cap > 0)
        length -= 1;
    }
};

struct Plain {
    Ring meta, pay;
    PktBufEntry ring[MAXM + 1];
    // PacketBuffer::dequeue_padding (packet_buffer.rs:156-167)
    bool dequeue_padding() {
        if (meta.length == 0 || ring[meta.read_at].kind != PKTBUF_KIND_PADDING) return false;
        uint32_t at;
        (void)pay.dequeue_many(ring[meta.read_at].size, &at);
        meta.dequeue_one();
        return true;
    }
    // PacketBuffer::dequeue_with (:169-204); take: the closure's verdict
    PktBufFront dequeue_with(bool take) {
        PktBufFront r = {0u, 0u, 0u, 0u, 0u};
        if (dequeue_padding()) r.res |= PKTBUF_PADDED;
        if (meta.length == 0) {
            r.res |= PKTBUF_EMPTY;
            return r;
        }
        const PktBufEntry e = ring[meta.read_at];
        const uint32_t cap_left = pay.cap - pay.read_at;
        const uint32_t contig = cap_left < pay.length ? cap_left : pay.length;
        // the unwrap of the header (a padding entry has none), the address family dispatch_ip can send, and
        // debug_assert!(payload_buf.len() == size)
        if (e.kind != PKTBUF_KIND_PACKET || (e.family != 4 && e.family != 6) || e.size > contig) {
            r.res |= PKTBUF_CORRUPT;
            return r;
        }
        r.res |= PKTBUF_OK;
        r.meta_idx = meta.read_at;
        r.size = e.size;
        r.family = e.family;
        r.ring_off = pay.read_at;
        if (take) {
            uint32_t at;
            const uint32_t got = pay.dequeue_many(e.size, &at);
            if (got != e.size || at != r.ring_off) {
                std::printf("FAIL the restatement's slice is short\n");
                std::exit(1);
            }
            meta.dequeue_one();
        }
        return r;
    }
};

unsigned long long g_steps = 0, g_singles = 0;
uint64_t g_digest = FNV_OFFSET;

[[noreturn]] void fail(const char* what, int P, int M, const PktBufState& s, int k0, int z0, int depth) {
    std::printf("FAIL %s: P %d, M %d, state (%u, %u, %u, %u), front kind %d size %d, depth %d\n", what, P, M, s.pr, s.pl, s.mr,
                s.ml, k0, z0, depth);
    std::exit(1);
}

bool same(const PktBufFront& a, const PktBufFront& b) {
    return a.res == b.res && a.ring_off == b.ring_off && a.meta_idx == b.meta_idx && a.size == b.size && a.family == b.family;
}

void run(int P, int M, const PktBufState& s0, int k0, int z0) {
    Plain q = {{(uint32_t)M, s0.mr, s0.ml}, {(uint32_t)P, s0.pr, s0.pl}, {}};
    for (int j = 0; j < M; ++j) q.ring[(s0.mr + (uint32_t)j) % (uint32_t)M] = entry_of(k0, z0, j);
    const auto at = [&](uint32_t idx) -> PktBufEntry {
        if (idx >= (uint32_t)M) fail("entry index outside the ring", P, M, s0, k0, z0, -1);
        return q.ring[idx];
    };
    PktBufState s = s0;
    for (int depth = 0; depth < DEPTH; ++depth) {
        const PktBufState before = s;
        // the closure fails: the padding is gone, the packet stays
        PktBufState sf = before;
        const PktBufFront f = pktbuf_front((uint32_t)P, (uint32_t)M, sf, at);
        Plain qf = q;
        const PktBufFront wf = qf.dequeue_with(false);
        if (!same(f, wf)) fail("front differs from the restatement", P, M, before, k0, z0, depth);
        if (sf.pr != qf.pay.read_at || sf.pl != qf.pay.length || sf.mr != qf.meta.read_at || sf.ml != qf.meta.length)
            fail("front's state differs from the restatement", P, M, before, k0, z0, depth);
        // the whole step
        const PktBufFront e = pktbuf_dequeue((uint32_t)P, (uint32_t)M, s, at);
        const PktBufFront w = q.dequeue_with(true);
        ++g_steps;
        if (!same(e, w) || !same(e, f)) fail("step differs from the restatement", P, M, before, k0, z0, depth);
        if (s.pr != q.pay.read_at || s.pl != q.pay.length || s.mr != q.meta.read_at || s.ml != q.meta.length)
            fail("state differs from the restatement", P, M, before, k0, z0, depth);
        if (!pktbuf_state_valid((uint32_t)P, (uint32_t)M, s)) fail("state leaves the contract", P, M, before, k0, z0, depth);
        if (depth == 0) {
            const uint32_t words[9] = {e.res, e.ring_off, e.meta_idx, e.size, e.family, s.pr, s.pl, s.mr, s.ml};
            uint64_t h = FNV_OFFSET;
            for (uint32_t x : words)
                for (int b = 0; b < 4; ++b) h = (h ^ ((x >> (8 * b)) & 0xffu)) * FNV_PRIME;
            g_digest = (g_digest ^ h) * FNV_PRIME;
            ++g_singles;
        }
        const uint32_t kinds = e.res & (PKTBUF_OK | PKTBUF_EMPTY | PKTBUF_CORRUPT);
        if (kinds != PKTBUF_OK && kinds != PKTBUF_EMPTY && kinds != PKTBUF_CORRUPT)
            fail("not exactly one of OK, EMPTY and CORRUPT", P, M, before, k0, z0, depth);
        if (e.res & PKTBUF_OK) {
            // one piece inside the bytes that were allocated once the padding was gone
            if ((uint64_t)e.ring_off + e.size > (uint32_t)P || e.size > sf.pl || e.ring_off != sf.pr || e.meta_idx != sf.mr)
                fail("range leaves the allocated bytes", P, M, before, k0, z0, depth);
            if (sf.pl - s.pl != e.size || sf.ml - s.ml != 1) fail("take is not the packet", P, M, before, k0, z0, depth);
        } else {
            if (sf.pr != s.pr || sf.pl != s.pl || sf.mr != s.mr || sf.ml != s.ml)
                fail("a stop dequeued more than the padding", P, M, before, k0, z0, depth);
            break;  // EMPTY and CORRUPT repeat themselves
        }
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
                            for (int k0 = 0; k0 < 3; ++k0)
                                for (int z0 = 0; z0 <= MAXSIZE; ++z0) run(P, M, s, k0, z0);
                        }
    std::printf("ok %llu %llu %016llx\n", g_steps, g_singles, (unsigned long long)g_digest);
    return 0;
}
