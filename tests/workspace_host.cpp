// Stand-alone check of torch_nf_amd/csrc/workspace.h (no HIP): a Carver run over NULL (the size query) and over a real
// buffer (the carve) walks the same offsets; regions are aligned as asked and do not overlap; empty regions and
// reserve() cost what they say; 2^40-element walks do not wrap; round_up / is_aligned at their boundaries.  Built and
// run by test_workspace_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../torch_nf_amd/csrc/workspace.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

using namespace tnf;

// one region of a walk: where it starts, where it ends, what alignment was asked for
struct Region {
    int64_t begin, end, align;
};

// The sequence both walks take: mixed element types, alignments 4 / 8 / 16 / 256, sizes that are no multiple of their
// alignment, an empty region, a reserve.  `out` receives each region as offsets from `base`.
static int64_t walk(void* base, Region* out, int* n, bool* null_when_null) {
    Carver c(base);
    char* b = static_cast<char*>(base);
    int k = 0;
    *null_when_null = true;
    auto note = [&](void* p, int64_t count, int64_t size, int64_t align) {
        const int64_t end = c.bytes();
        out[k++] = Region{end - count * size, end, align};
        if (base) CHECK(static_cast<char*>(p) == b + (end - count * size));
        else if (p) *null_when_null = false;
    };
    note(c.take<float>(3, 16), 3, 4, 16);       // 12 bytes
    note(c.take<float>(1, 4), 1, 4, 4);         // packed behind it
    note(c.take<double>(5, 8), 5, 8, 8);        // 16 -> 16
    note(c.take<unsigned>(1, 4), 1, 4, 4);
    note(c.take<char>(7, 256), 7, 1, 256);      // jumps to 256
    note(c.take<float>(0, 256), 0, 4, 256);     // empty: only the alignment
    note(c.take<int>(33, 16), 33, 4, 16);
    const int64_t before = c.bytes();
    c.reserve(100);
    CHECK(c.bytes() == before + 100);
    note(c.take<double>(2, 8), 2, 8, 8);
    CHECK(c.bytes(8) == c.bytes());  // rounding the total does not move the walk
    *n = k;
    return c.bytes(256);
}

int main() {
    // ---- the same walk over NULL and over a buffer ----
    Region q[16], r[16];
    int nq = 0, nr = 0;
    bool nulls = false, unused = false;
    const int64_t need = walk(nullptr, q, &nq, &nulls);
    CHECK(nulls);  // the size query hands out no pointer at all
    void* buf = aligned_alloc(256, (size_t)need);
    CHECK(buf != nullptr);
    const int64_t used = walk(buf, r, &nr, &unused);
    CHECK(used == need);
    CHECK(nq == nr && nq == 8);
    for (int i = 0; i < nq; ++i) {
        CHECK(q[i].begin == r[i].begin && q[i].end == r[i].end);
        CHECK(q[i].begin % q[i].align == 0);
        CHECK(is_aligned(static_cast<char*>(buf) + r[i].begin, r[i].align));
        CHECK(q[i].end <= need);
        if (i > 0) CHECK(q[i].begin >= q[i - 1].end);  // consecutive regions do not overlap
    }
    free(buf);
    // the offsets themselves, so that a change of the walking rule shows here first
    CHECK(q[0].begin == 0 && q[0].end == 12);
    CHECK(q[1].begin == 12 && q[1].end == 16);
    CHECK(q[2].begin == 16 && q[2].end == 56);
    CHECK(q[3].begin == 56 && q[3].end == 60);
    CHECK(q[4].begin == 256 && q[4].end == 263);
    CHECK(q[5].begin == 512 && q[5].end == 512);  // an empty region consumes nothing beyond its alignment
    CHECK(q[6].begin == 512 && q[6].end == 644);
    CHECK(q[7].begin == 744 && q[7].end == 760);  // 644 + the 100 reserved bytes, already a multiple of 8
    CHECK(need == 768);

    // ---- an empty region at an aligned offset consumes nothing at all ----
    {
        Carver c(nullptr);
        c.take<float>(64, 256);
        const int64_t at = c.bytes();
        CHECK(c.take<double>(0, 256) == nullptr);
        CHECK(c.bytes() == at);
        c.reserve(0);
        CHECK(c.bytes() == at);
    }

    // ---- counts near 2^40: the offset is 64-bit throughout ----
    {
        const int64_t big = ((int64_t)1 << 40) + 3;
        Carver c(nullptr);
        CHECK(c.take<float>(big, 256) == nullptr);
        CHECK(c.bytes() == 4 * big);
        CHECK(c.take<double>(big, 256) == nullptr);
        const int64_t second = round_up(4 * big, 256);
        CHECK(c.bytes() == second + 8 * big);
        c.reserve(big);
        CHECK(c.bytes() == second + 9 * big);
        CHECK(c.bytes(256) == round_up(second + 9 * big, 256));
        CHECK(c.bytes(256) > ((int64_t)13 << 40));
    }

    // ---- round_up and is_aligned at 0, 1, align - 1, align, align + 1 ----
    for (int64_t align : {1, 4, 8, 16, 256}) {
        CHECK(round_up(0, align) == 0);
        CHECK(round_up(1, align) == align);
        CHECK(round_up(align - 1, align) == (align == 1 ? 0 : align));
        CHECK(round_up(align, align) == align);
        CHECK(round_up(align + 1, align) == (align == 1 ? 2 : 2 * align));
        CHECK(is_aligned(nullptr, align));
        CHECK(is_aligned(reinterpret_cast<const void*>((uintptr_t)1), align) == (align == 1));
        CHECK(is_aligned(reinterpret_cast<const void*>((uintptr_t)(align - 1)), align) == (align == 1));
        CHECK(is_aligned(reinterpret_cast<const void*>((uintptr_t)align), align));
        CHECK(is_aligned(reinterpret_cast<const void*>((uintptr_t)(align + 1)), align) == (align == 1));
    }

    if (failures) {
        printf("workspace_host: %d check(s) failed\n", failures);
        return 1;
    }
    printf("workspace_host: ok\n");
    return 0;
}
