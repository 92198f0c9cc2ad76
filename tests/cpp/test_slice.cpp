// Cutting a record range out of a batch (smoltcp_amd/csrc/csum_launch.h: slice, for_chunks): every
// per-record array that is set advances to the range's first record, null stays null, and what is not
// indexed by record (stage, stage_flags, dummy, src) is left alone; the chunk loop visits each record once,
// in order, and stops at the first failure.  Host only: pointers are compared, nothing is dereferenced.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smoltcp_amd/csrc/csum_launch.h"

using namespace smolcsum;

static int bad = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            std::printf("line %d: %s\n", __LINE__, #c);      \
            ++bad;                                           \
        }                                                    \
    } while (0)

constexpr uint64_t N = 100, STRIDE = 1564;
static uint8_t buf[N * STRIDE], status[N], src[64], dummy[256], addrs[32 * N];
static smol_csum_desc_t desc[N];
static uint16_t out16[N];
static smol_csum_copy_t copy[N];
static smol_csum_fields_t fields[N];
static uint64_t stage[N];
static uint32_t stage_flags[N];

// both batch forms; `arrays`: every per-record array set, or none
static KParams params(bool with_desc, bool arrays) {
    KParams p;
    std::memset(&p, 0, sizeof p);
    p.buf = buf;
    p.desc = with_desc ? desc : nullptr;
    p.n = N;
    p.stride = STRIDE;
    p.len = 1500;
    p.kind = 2;
    p.caps_udp = 1;
    p.num_cu = 256;
    p.xcd_remap = 1;
    p.dummy = dummy;
    p.src = src;
    p.stage = stage;
    p.stage_flags = stage_flags;
    if (arrays) {
        p.status = status;
        p.out16 = out16;
        p.copy = copy;
        p.addrs = addrs;
        p.fields = fields;
    }
    return p;
}

static void check_slice(bool with_desc, bool arrays) {
    const KParams p = params(with_desc, arrays);
    for (uint64_t i0 : {uint64_t{0}, uint64_t{1}, uint64_t{7}, N - 1}) {
        const uint64_t n = N - i0 < 16 ? N - i0 : 16;
        const KParams q = slice(p, i0, n);
        CHECK(q.n == n);
        // the batch: the descriptors advance when there are any (the offsets they hold are from buf), else buf
        CHECK(q.desc == (with_desc ? desc + i0 : nullptr));
        CHECK(q.buf == (with_desc ? buf : buf + i0 * STRIDE));
        // the per-record arrays: one entry per record, addrs 32 B per record
        CHECK(q.status == (arrays ? status + i0 : nullptr));
        CHECK(q.out16 == (arrays ? out16 + i0 : nullptr));
        CHECK(q.copy == (arrays ? copy + i0 : nullptr));
        CHECK(q.addrs == (arrays ? addrs + 32 * i0 : nullptr));
        CHECK(q.fields == (arrays ? fields + i0 : nullptr));
        // not per record: chunk-relative scratch, the dummy line, the copy source
        CHECK(q.stage == stage && q.stage_flags == stage_flags && q.dummy == dummy && q.src == src);
        // and the scalars
        CHECK(q.stride == STRIDE && q.len == 1500 && q.kind == 2 && q.caps_udp == 1 && q.caps_ipv4 == 0 &&
              q.caps_tcp == 0 && q.caps_icmpv4 == 0 && q.caps_icmpv6 == 0 && q.num_cu == 256 && q.xcd_remap == 1);
    }
}

static void check_chunks(bool with_desc) {
    const KParams p = params(with_desc, true);
    for (uint64_t per : {uint64_t{1}, uint64_t{7}, uint64_t{16}, uint64_t{100}, uint64_t{101}}) {
        std::vector<int> seen(N, 0);
        uint64_t next = 0, calls = 0;
        const int rc = for_chunks(p, per, [&](uint64_t i0, const KParams& q) {
            CHECK(i0 == next);  // in order, nothing skipped
            CHECK(q.n == (N - i0 < per ? N - i0 : per));  // only the last chunk is short
            CHECK(q.status == status + i0 && q.fields == fields + i0);
            CHECK(with_desc ? q.desc == desc + i0 : q.buf == buf + i0 * STRIDE);
            for (uint64_t i = i0; i < i0 + q.n && i < N; ++i) ++seen[i];
            next = i0 + q.n;
            ++calls;
            return 0;
        });
        CHECK(rc == 0 && next == N && calls == (N + per - 1) / per);
        for (uint64_t i = 0; i < N; ++i) CHECK(seen[i] == 1);
    }
    // the first failing callback ends the loop, and its result is the loop's
    uint64_t calls = 0;
    const int rc = for_chunks(p, 7, [&](uint64_t i0, const KParams&) {
        ++calls;
        return i0 == 14 ? 5 : 0;
    });
    CHECK(rc == 5 && calls == 3);
    // 0 records per chunk: the whole batch in one; an empty batch: no call
    calls = 0;
    CHECK(for_chunks(p, 0, [&](uint64_t i0, const KParams& q) { return ++calls, (i0 == 0 && q.n == N) ? 0 : 1; }) == 0);
    CHECK(calls == 1);
    CHECK(for_chunks(slice(p, 0, 0), 7, [&](uint64_t, const KParams&) { return 1; }) == 0);
}

int main() {
    for (bool with_desc : {false, true}) {
        for (bool arrays : {false, true}) check_slice(with_desc, arrays);
        check_chunks(with_desc);
    }
    std::printf(bad ? "FAILED %d\n" : "slices ok\n", bad);
    return bad ? 1 : 0;
}
