// Stand-alone program: the host-only part of beam search (zoomearth_amd/csrc/ze_index.cpp: argument and table checks, the divisor
// table, the live-group selection) built with -fsanitize=address,undefined and driven over valid, refused and edge inputs.  Any
// sanitizer report aborts; a wrong answer returns non-zero.  tests/test_beam_search_cpu.py builds and runs it.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ze_host.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                               \
        }                                                             \
    } while (0)

static int beam(const std::vector<int32_t>& seqs, int groups, int B, int R, int max_new, int early, float lp, float pen, int max_seqs, int max_ctx,
                const char* expect = nullptr) {
    const char* why = nullptr;
    const int r = ze_beam_check_impl(seqs.empty() ? nullptr : seqs.data(), groups, B, R, max_new, early, lp, pen, max_seqs, max_ctx, &why);
    if (r != 0) EXPECT(why != nullptr && strlen(why) > 0);
    if (expect) EXPECT(why != nullptr && strstr(why, expect) != nullptr);
    return r;
}

static int reorder(const std::vector<int32_t>& src, const std::vector<int32_t>& dst, int row0, int rows, int max_seqs, int max_ctx) {
    const char* why = nullptr;
    return ze_kv_reorder_check_impl(src.data(), dst.data(), (int)dst.size(), row0, rows, max_seqs, max_ctx, &why);
}

int main() {
    // ---- ze_beam_check_impl: exactly groups * num_beams ids are read, from arrays of exactly that size
    for (int B : {1, 3, 16})
        for (int groups : {1, 3, 5}) {
            std::vector<int32_t> seqs(groups * B);
            for (int i = 0; i < groups * B; ++i) seqs[i] = groups * B - 1 - i;
            EXPECT(beam(seqs, groups, B, B, 12, 2, 1.0f, 1.3f, groups * B, 64) == 0);
            EXPECT(beam(seqs, groups, B, B, 12, 2, 1.0f, 1.3f, groups * B - 1, 64) == -1);   // more rows than slots
            seqs.back() = seqs.front();
            if (groups * B > 1) EXPECT(beam(seqs, groups, B, 1, 12, 0, 1.0f, 1.0f, 80, 64, "named twice") == -1);
            seqs.back() = 80;
            EXPECT(beam(seqs, groups, B, 1, 12, 0, 1.0f, 1.0f, 80, 64, "out of range") == -4);
            seqs.back() = -1;
            EXPECT(beam(seqs, groups, B, 1, 12, 0, 1.0f, 1.0f, 80, 64) == -4);
        }
    std::vector<int32_t> four = {0, 1, 2, 3};
    EXPECT(beam({}, 1, 4, 1, 8, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 0, 4, 1, 8, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, -3, 4, 1, 8, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 0, 1, 8, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 17, 1, 8, 0, 1.f, 1.f, 80, 64) == -1);
    EXPECT(beam(four, 1, 4, 5, 8, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 0, 8, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 0, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 65, 0, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 64, 0, 1.f, 1.f, 8, 64) == 0);
    EXPECT(beam(four, 1, 4, 1, 8, 3, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 8, -1, 1.f, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 8, 0, NAN, 1.f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 8, 0, 1.f, INFINITY, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 8, 0, 1.f, -0.5f, 8, 64) == -1);
    EXPECT(beam(four, 1, 4, 1, 8, 0, -2.f, 0.f, 8, 64) == 0);
    EXPECT(beam(four, 0x7fffffff, 16, 1, 8, 0, 1.f, 1.f, 8, 64) == -1);   // groups * num_beams beyond int: refused, nothing read
    EXPECT(beam(four, 1, 4, 1, 8, 0, 1.f, 1.f, 0, 64) == -1);
    EXPECT(ze_beam_check_impl(four.data(), 1, 4, 1, 8, 0, 1.f, 1.f, 8, 64, nullptr) == 0);   // no message wanted
    // ---- ze_kv_reorder_check_impl
    EXPECT(reorder({0, 1, 1, 1}, {3, 2, 4, 5}, 5, 33, 6, 40) == 0);
    EXPECT(reorder({0, 1}, {1, 2}, 0, 1, 6, 40) == -1);          // a destination that is also a source
    EXPECT(reorder({0, 1}, {2, 2}, 0, 1, 6, 40) == -1);          // a destination named twice
    EXPECT(reorder({0}, {0}, 0, 1, 6, 40) == -1);
    EXPECT(reorder({0, 6}, {1, 2}, 0, 1, 6, 40) == -4);
    EXPECT(reorder({0, 1}, {-1, 2}, 0, 1, 6, 40) == -4);
    EXPECT(reorder({0}, {1}, 8, 33, 6, 40) == -1);
    EXPECT(reorder({0}, {1}, -1, 1, 6, 40) == -1);
    EXPECT(reorder({0}, {1}, 0, -1, 6, 40) == -1);
    EXPECT(reorder({0}, {1}, 0x7fffffff, 0x7fffffff, 6, 40) == -1);   // row0 + rows beyond int
    EXPECT(reorder({0}, {1}, 40, 0, 6, 40) == 0);
    EXPECT(reorder({0, 1, 2, 3, 4, 5, 0}, {1, 2, 3, 4, 5, 0, 1}, 0, 1, 6, 40) == -1);   // more pairs than slots
    const char* why = nullptr;
    EXPECT(ze_kv_reorder_check_impl(nullptr, nullptr, 0, 0, 0, 6, 40, &why) == 0);
    EXPECT(ze_kv_reorder_check_impl(nullptr, nullptr, 2, 0, 1, 6, 40, &why) == -1);
    EXPECT(ze_kv_reorder_check_impl(nullptr, nullptr, -1, 0, 1, 6, 40, nullptr) == -1);
    // ---- the divisor table: Python's n ** length_penalty, rounded to float
    std::vector<float> divs;
    for (float lp : {0.0f, 1.0f, 2.0f, -1.5f}) {
        for (int max_new : {1, 12, 4096}) {
            ze_beam_divs_impl(lp, max_new, divs);
            EXPECT((int)divs.size() == max_new + 1);
            EXPECT(divs[0] == 1.0f && divs[1] == 1.0f);
            EXPECT(divs[max_new] == (float)pow((double)max_new, (double)lp));
        }
    }
    ze_beam_divs_impl(1.0f, 0, divs);
    EXPECT(divs.size() == 1);
    ze_beam_divs_impl(1.0f, -5, divs);
    EXPECT(divs.size() == 1);
    // ---- the live groups of a step
    std::vector<int> still;
    ze_beam_live_impl({0, 1, 2, 3}, {0, 1, 0, 0}, {12, 12, 3, 4}, 3, still);
    EXPECT((still == std::vector<int>{0, 3}));
    ze_beam_live_impl({3, 0}, {0, 0, 0, 0}, {12, 12, 3, 4}, 4, still);
    EXPECT((still == std::vector<int>{0}));
    ze_beam_live_impl({}, {}, {}, 1, still);
    EXPECT(still.empty());
    ze_beam_live_impl({0, 7, -1}, {0}, {5}, 1, still);   // a group outside the tables is dropped, not read
    EXPECT((still == std::vector<int>{0}));
    if (failures) return 1;
    printf("sanitized beam host checks ok\n");
    return 0;
}
