// The whole-segment rule of fixed-stride emit, restated on emit_fields entries (the segment pass of the
// two-launch route, csum_segpass.hip).  One host / device function with no HIP in it, so that the rule is
// walked on the CPU (tests/cpp/test_seg_rule.cpp).
//
// Emit writes 2-B fields; HBM takes a plain write for a whole 64-B segment and a read-modify-write for
// anything smaller, so a record's fields go out as the whole aligned segment(s) holding them wherever
// every byte of those segments may be written by this record's decision alone (csum_xwalk.hip states
// the same rule on a wavefront's parsed records: ok_tail / prev_ok):
//  - a record decides for the segments its fields lie in, all or nothing: both whole, or every field as
//    a 2-B store;
//  - its fields must end 64 B or more before its end (ok_tail), so none of its segments reaches its last
//    64 bytes, the next record or a gap;
//  - a segment that starts before the record also holds the previous record's last bytes: whole only for
//    packed records (stride == len; with a gap those bytes are gap bytes and never written), when a
//    previous record exists in the batch and its own fields end 64 B or more before its end (so it
//    writes nothing there, neither a field nor a segment of its own);
//  - no segment starts before the batch's first byte or ends past its last.
// Two records' decisions therefore never write one segment, and no 2-B store of one record lands in a
// whole segment of another.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SMOL_SEGRULE_FN __host__ __device__ inline
#else
#define SMOL_SEGRULE_FN inline
#endif

namespace smolcsum {

constexpr uint32_t SEGRULE_NO_FIELD = 0xffffu;  // an entry's unused slot (SMOL_NO_FIELD)
constexpr uint32_t SEGRULE_NO_PREV = ~0u;       // prev_end: the neighbour's entry is not known
constexpr int32_t SEGRULE_2B = INT32_MIN;       // SegRule::a: every field goes out as a 2-B store

// Record-relative starts of the whole segments (b == a: one segment); a == SEGRULE_2B: none.
struct SegRule {
    int32_t a, b;
};

// The end of an entry's fields in its record (the largest offset + 2; 0: no field).
SMOL_SEGRULE_FN uint32_t segrule_field_end(const uint32_t off[3]) {
    uint32_t hi = 0;
    for (int i = 0; i < 3; ++i)
        if (off[i] != SEGRULE_NO_FIELD && off[i] + 2 > hi) hi = off[i] + 2;
    return hi;
}

// ph: the record's address modulo 64; len, stride: the batch's; off: the entry's field offsets;
// prev_end: segrule_field_end of the previous record's entry (SEGRULE_NO_PREV: not known, which counts
// as a neighbour with a field in its tail); before: the batch's bytes before this record's first
// (0 for record 0); after: the batch's bytes from this record's first to the batch's last (len for the
// last record).  A record without a field gets SEGRULE_2B (and has nothing to store).
SMOL_SEGRULE_FN SegRule seg_rule(uint32_t ph, uint32_t len, uint64_t stride, const uint32_t off[3], uint32_t prev_end,
                                 uint64_t before, uint64_t after) {
    const SegRule two_b = {SEGRULE_2B, SEGRULE_2B};
    uint32_t lo = SEGRULE_NO_FIELD;
    for (int i = 0; i < 3; ++i)
        if (off[i] < lo) lo = off[i];
    const uint32_t hi = segrule_field_end(off);
    if (hi == 0 || (uint64_t)hi + 64 > len) return two_b;  // ok_tail
    const int32_t a = (int32_t)((ph + lo) & ~63u) - (int32_t)ph;
    const int32_t b = (int32_t)((ph + hi - 1) & ~63u) - (int32_t)ph;
    if (b > a + 64) return two_b;  // the fields span more than two adjacent segments
    const bool prev_ok = stride == (uint64_t)len && before >= (uint64_t)len && prev_end != SEGRULE_NO_PREV &&
                         (prev_end == 0 || (uint64_t)prev_end + 64 <= len);
    if (a < 0 && !(prev_ok && (uint64_t)(-a) <= before)) return two_b;
    if ((uint64_t)((int64_t)b + 64) > after || (uint64_t)((int64_t)b + 64) > len) return two_b;
    return SegRule{a, b};
}

}  // namespace smolcsum
