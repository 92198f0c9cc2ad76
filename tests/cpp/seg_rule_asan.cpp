// The whole-segment rule of the two-launch emit route (smoltcp_amd/csrc/csum_segrule.h seg_rule, the
// function the segment pass calls) walked on the CPU: batches of 4 records at every start address modulo
// 64, lengths 64 .. 200 and 1500, packed and gapped strides, a probe field at every offset of the record
// in several neighbour patterns.  For every batch: no whole segment leaves the batch or holds a gap byte,
// no segment is written by two records' decisions, no 2-B store of one record lands in a whole segment of
// another, and every field byte is covered exactly once, by a segment or by a 2-B store.
// Stand-alone (its own main), built with -fsanitize=address,undefined by tests/test_seg_rule_cpu.py: the
// per-segment book is a heap block of exactly the batch's segments, so a segment outside the batch is a
// report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../smoltcp_amd/csrc/csum_segrule.h"

using namespace smolcsum;

namespace {

constexpr int N = 4;  // records: the first, two inner ones, the last
constexpr uint32_t NF = SEGRULE_NO_FIELD;

struct Fields {
    uint32_t off[3];
};

unsigned long long g_checked = 0, g_whole = 0, g_two_b = 0;

[[noreturn]] void fail(const char* what, uint32_t base, uint32_t len, uint64_t stride, int rec, uint32_t f) {
    std::printf("FAIL %s: base %% 64 = %u, len %u, stride %llu, record %d, probe field %u\n", what, base, len,
                (unsigned long long)stride, rec, f);
    std::exit(1);
}

// One batch: record i at base + i * stride with fields fs[i].
// seg_writer: which record writes a segment whole (one entry per 64-B segment the batch touches).
void check_batch(uint32_t base, uint32_t len, uint64_t stride, const Fields fs[N], uint32_t probe, std::vector<int>& seg_writer) {
    const uint64_t total = (N - 1) * stride + len;
    const uint64_t first_seg = base / 64;
    std::fill(seg_writer.begin(), seg_writer.end(), -1);
    SegRule d[N];
    for (int i = 0; i < N; ++i) {
        const uint64_t a0 = base + i * stride;
        const uint32_t prev = i == 0 ? SEGRULE_NO_PREV : segrule_field_end(fs[i - 1].off);
        d[i] = seg_rule((uint32_t)(a0 % 64), len, stride, fs[i].off, prev, a0 - base, total - (a0 - base));
        ++g_checked;
        if (d[i].a == SEGRULE_2B) {
            ++g_two_b;
            continue;
        }
        ++g_whole;
        if (segrule_field_end(fs[i].off) == 0) fail("segments for a record without a field", base, len, stride, i, probe);
        if (d[i].b != d[i].a && d[i].b != d[i].a + 64) fail("segments not adjacent", base, len, stride, i, probe);
        for (int w = 0; w < (d[i].b != d[i].a ? 2 : 1); ++w) {
            const int64_t s = (int64_t)a0 + (w ? d[i].b : d[i].a);
            if (s % 64 != 0) fail("segment not aligned", base, len, stride, i, probe);
            if (s < (int64_t)base || (uint64_t)s + 64 > base + total) fail("segment leaves the batch", base, len, stride, i, probe);
            // (a segment inside the batch holds a gap byte unless it lies inside one record, or the records are packed)
            if (stride != len && ((uint64_t)s - base) % stride + 64 > len) fail("segment holds a gap byte", base, len, stride, i, probe);
            int& wr = seg_writer.at((uint64_t)s / 64 - first_seg);
            if (wr != -1) fail("two decisions write one segment", base, len, stride, i, probe);
            wr = i;
        }
    }
    // every field byte is written exactly once: by its own 2-B store and no segment of anybody's, or by
    // exactly one of its own record's segments and no 2-B store
    for (int i = 0; i < N; ++i) {
        const uint64_t a0 = base + i * stride;
        for (int k = 0; k < 3; ++k) {
            if (fs[i].off[k] == NF) continue;
            for (uint32_t j = 0; j < 2; ++j) {
                const uint64_t at = a0 + fs[i].off[k] + j;
                const int wr = seg_writer[at / 64 - first_seg];
                if (d[i].a == SEGRULE_2B) {
                    if (wr != -1) fail("a 2-B store lands in another record's whole segment", base, len, stride, i, probe);
                } else {
                    if (wr != i) fail("a field byte outside its record's segments", base, len, stride, i, probe);
                    const bool in_a = at / 64 == (a0 + d[i].a) / 64, in_b = d[i].b != d[i].a && at / 64 == (a0 + d[i].b) / 64;
                    if (in_a == in_b) fail("a field byte not in exactly one of its segments", base, len, stride, i, probe);
                }
            }
        }
    }
}

void walk(uint32_t len) {
    const uint64_t strides[4] = {len, len + 1ull, len + 36ull, len + 64ull};
    for (uint32_t base = 0; base < 64; ++base)
        for (uint64_t stride : strides) {
            std::vector<int> seg_writer((base + (N - 1) * stride + len + 63) / 64 - base / 64);
            for (uint32_t f = 0; f + 2 <= len; ++f) {
                auto fit = [&](uint32_t o) { return o + 2 <= len ? o : NF; };
                const Fields one = {{f, NF, NF}}, two = {{f, fit(f + 16), NF}}, three = {{fit(f + 16), f, fit(f + 70)}},
                             far = {{f, fit(f + 120), NF}}, tail = {{NF, len - 2, NF}}, head = {{0, NF, NF}},
                             nothing = {{NF, NF, NF}};
                const Fields pats[][N] = {
                    {one, one, one, one},         {two, two, two, two},     {three, three, three, three},
                    {one, tail, one, tail},       {tail, two, head, one},   {nothing, one, nothing, two},
                    {head, head, head, head},     {far, one, far, tail},    {two, nothing, tail, three},
                };
                // (three of the nine patterns per point, every pattern at every third offset and start)
                for (uint32_t k = (f + base) % 3; k < 9; k += 3) check_batch(base, len, stride, pats[k], f, seg_writer);
            }
        }
}

}  // namespace

int main() {
    for (uint32_t len = 64; len <= 200; ++len) walk(len);
    walk(1500);
    if (g_whole == 0 || g_two_b == 0) {
        std::printf("FAIL the walk never reached both answers\n");
        return 1;
    }
    std::printf("ok %llu decisions, %llu whole, %llu 2-B\n", g_checked, g_whole, g_two_b);
    return 0;
}
