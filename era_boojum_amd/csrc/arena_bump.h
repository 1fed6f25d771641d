// The bump arithmetic of a context's proof workspace, defined once: where a request of `elems` words lands.  The arena is one
// reservation (the total of the proof's workspace plan, workspace_plan.h) bump-allocated from offset 0; a proof that outgrows it
// goes on in overflow slabs, each bump-allocated the same way, and never returns to the arena.  Every start is rounded up to 64
// words (512 bytes).  The high-water mark counts the words the proof in flight has taken: the arena's offset while no slab exists,
// then elems + 64 for every block that lands in a slab.  The library allocates device memory only for "new slab" (ctx.hip); this
// value holds no pointer.  Plain C++17, no HIP: a host program can use it (tests/arena_bump_check.cpp).
#pragma once
#include <cstddef>
#include <vector>

namespace bj {

struct ArenaBump {
    static constexpr size_t ALIGN = 64, MIN_SLAB = (size_t)1 << 25;   // words: 512 bytes, 256 MiB
    size_t arena_words = 0, arena_off = 0;
    std::vector<size_t> slabs;   // words of each overflow slab, in the order they were opened
    size_t slab_off = 0;         // words used in the last slab
    size_t high_water = 0;       // words the proof in flight has taken (arena + slabs)

    enum Where : unsigned { NOTHING, ARENA, LAST_SLAB, NEW_SLAB };
    struct Place {
        Where where;
        size_t offset;       // of the block in the arena or the slab
        size_t slab_words;   // NEW_SLAB: the size of the slab to allocate
    };
    static size_t aligned(size_t off) { return (off + ALIGN - 1) & ~(ALIGN - 1); }

    // Places `elems` words and moves the state behind them.  Outside a proof the arena alone serves: the slabs belong to the
    // proof in flight, and a request that does not fit answers NOTHING and changes nothing.
    Place place(size_t elems, bool in_proof) {
        const size_t start = aligned(arena_off);
        if (slabs.empty() && start + elems <= arena_words) {
            arena_off = start + elems;
            if (arena_off > high_water) high_water = arena_off;
            return {ARENA, start, 0};
        }
        if (!in_proof) return {NOTHING, 0, 0};
        if (!slabs.empty()) {
            const size_t st = aligned(slab_off);
            if (st + elems <= slabs.back()) {
                slab_off = st + elems;
                high_water += elems + ALIGN;
                return {LAST_SLAB, st, 0};
            }
        }
        const size_t slab = elems > MIN_SLAB ? elems : MIN_SLAB;
        slabs.push_back(slab);
        slab_off = elems;
        if (high_water < arena_off) high_water = arena_off;
        high_water += elems + ALIGN;
        return {NEW_SLAB, 0, slab};
    }
    size_t slab_words() const {
        size_t s = 0;
        for (size_t w : slabs) s += w;
        return s;
    }
    void drop_slabs() {
        slabs.clear();
        slab_off = 0;
    }
    void reset() {   // a new proof: the arena keeps its size
        arena_off = high_water = 0;
        drop_slabs();
    }
};

}  // namespace bj
