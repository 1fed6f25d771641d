// Stand-alone check of csrc/list_plan.h, the host arithmetic of bj_list_unsatisfied (tests/test_list_plan_host.py builds it with
// the address and undefined-behaviour sanitizers): how a capacity falls across the four kinds against a list written out entry by
// entry, totals[0] as the sum, the rows of a chunk, and the entry slots of the device block at the edges of 64 bits.
#include "list_plan.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

using bj::ListSplit;

// the split by writing the list out: kinds in order, the first `capacity` kept
static void split_by_enumeration(uint64_t capacity, const uint64_t t[5]) {
    std::vector<int> list;
    for (int k = 1; k <= 4; k++) list.insert(list.end(), (size_t)t[k], k);
    const ListSplit s = bj::list_split(capacity, t);
    CHECK(s.total == list.size());
    CHECK(s.total == t[1] + t[2] + t[3] + t[4]);
    const size_t kept = capacity < list.size() ? (size_t)capacity : list.size();
    CHECK(s.kept == kept && s.written[0] == kept);
    uint64_t written[5] = {}, first[5] = {};
    bool seen[5] = {};
    for (size_t i = 0; i < list.size(); i++) {
        if (!seen[list[i]]) first[list[i]] = i, seen[list[i]] = true;
        if (i < kept) written[list[i]]++;
    }
    uint64_t sum = 0;
    for (int k = 1; k <= 4; k++) {
        CHECK(s.written[k] == written[k]);
        if (seen[k]) CHECK(s.first[k] == first[k]);
        if (s.written[k]) CHECK(s.first[k] < kept);   // the entry the host layer looks at is one it has copied
        sum += s.written[k];
    }
    CHECK(sum == s.kept);
}

int main() {
    // every small combination of totals under every capacity around the boundaries between the kinds
    for (uint64_t a = 0; a <= 3; a++)
        for (uint64_t b = 0; b <= 3; b++)
            for (uint64_t c = 0; c <= 2; c++)
                for (uint64_t d = 0; d <= 2; d++) {
                    const uint64_t t[5] = {0, a, b, c, d};
                    for (uint64_t capacity = 0; capacity <= a + b + c + d + 2; capacity++) split_by_enumeration(capacity, t);
                }
    {   // the cut inside kind 2, inside kind 3, and kind 4 only once the capacity reaches it
        const uint64_t t[5] = {0, 5, 7, 2, 3};
        ListSplit s = bj::list_split(6, t);
        CHECK(s.written[1] == 5 && s.written[2] == 1 && s.written[3] == 0 && s.written[4] == 0 && s.kept == 6 && s.total == 17);
        s = bj::list_split(13, t);
        CHECK(s.written[2] == 7 && s.written[3] == 1 && s.written[4] == 0);
        s = bj::list_split(14, t);
        CHECK(s.written[3] == 2 && s.written[4] == 0);
        s = bj::list_split(15, t);
        CHECK(s.written[4] == 1 && s.first[4] == 14);
        s = bj::list_split(UINT64_MAX, t);
        CHECK(s.kept == 17 && s.written[4] == 3);
        s = bj::list_split(0, t);
        CHECK(s.kept == 0 && s.total == 17 && s.written[1] == 0);
    }
    {   // totals near 2^64 saturate instead of wrapping
        const uint64_t t[5] = {0, UINT64_MAX - 1, 5, 0, 0};
        const ListSplit s = bj::list_split(UINT64_MAX, t);
        CHECK(s.total == UINT64_MAX && s.written[1] == UINT64_MAX - 1 && s.written[2] == 1);
    }
    // chunk rows: a multiple of the block, never above the cap or the padded trace, at least the padded capacity below them
    for (unsigned log_n = 0; log_n <= 30; log_n++) {
        const uint64_t n = (uint64_t)1 << log_n;
        for (uint64_t capacity : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)64, (uint64_t)65, (uint64_t)255, (uint64_t)256, (uint64_t)257,
                                  (uint64_t)1000, (uint64_t)16384, (uint64_t)16385, (uint64_t)1 << 40, UINT64_MAX}) {
            const uint64_t m = bj::list_chunk_rows(capacity, n);
            CHECK(m >= bj::LIST_BLOCK && m % bj::LIST_BLOCK == 0 && m <= bj::LIST_CHUNK_MAX);
            CHECK(m <= (n > bj::LIST_BLOCK ? n : bj::LIST_BLOCK));
            if (capacity <= m) CHECK(m - capacity < bj::LIST_BLOCK || m == bj::list_chunk_rows(0, n));   // padded capacity, or the floor
            CHECK(bj::list_chunks(n, m) <= 64 || m == bj::LIST_CHUNK_MAX);
            CHECK(bj::list_chunks(0, m) == 0 && bj::list_chunks(1, m) == 1 && bj::list_chunks(m, m) == 1 && bj::list_chunks(m + 1, m) == 2);
        }
    }
    CHECK(bj::list_chunk_rows(1, 1024) == 256 && bj::list_chunk_rows(65, 1024) == 256 && bj::list_chunk_rows(1000, 1024) == 1024);
    CHECK(bj::list_chunk_rows(64, (uint64_t)1 << 20) == 16384 && bj::list_chunk_rows(5000, 8192) == 5120);
    // entry slots: the capacity, or what n rows can hold
    CHECK(bj::list_entry_slots(0, 1024, 15, 5, 8) == 0);
    CHECK(bj::list_entry_slots(100, 1024, 15, 5, 8) == 100);
    CHECK(bj::list_entry_slots(UINT64_MAX, 1024, 15, 5, 8) == 1024 * (15 + 5 + 8 + 1));
    CHECK(bj::list_entry_slots(UINT64_MAX, 1024, 15, 5, 0) == 1024 * 20);
    CHECK(bj::list_entry_slots(UINT64_MAX, (uint64_t)1 << 30, UINT64_MAX >> 8, 0, 0) == UINT64_MAX);
    CHECK(bj::list_mul_add_sat(0, UINT64_MAX, 7) == 7 && bj::list_mul_add_sat(UINT64_MAX, 1, 1) == UINT64_MAX);
    if (!failures) std::printf("list plan == expected\n");
    return failures ? 1 : 0;
}
