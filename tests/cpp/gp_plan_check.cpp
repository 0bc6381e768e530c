// Host check of optuna_amd/_hip/csrc/gp_plan.h, compiled and run by
// tests/test_gp_plan.py. Prints one line per failed check; exit status 1 if
// any failed.
#include <cstdint>
#include <cstdio>

#include "gp_plan.h"

static int g_failed = 0;

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

// n_chunks chunks of `rows` cover B, and one fewer does not.
static void check_cover(int64_t B, int64_t rows) {
    const int64_t n = gp_n_chunks(B, rows);
    CHECK(n * rows >= B && B > (n - 1) * rows);
}

int main() {
    // The partial buffer holds gp_part_records(rows) records and a chunk of
    // bc <= rows candidates writes bc * splits of them.
    for (int64_t max : {1, 2, 3, 40, 4096}) {
        int bad = 0;
        for (int64_t bc = 1; bc <= 70000; ++bc) {
            const int64_t s = gp_splits(bc, max);
            bad += !(1 <= s && s <= max);
            bad += !(bc * s < GP_TARGET_BLOCKS + bc);
            bad += !((size_t)(bc * s) < gp_part_records(bc));
        }
        CHECK(bad == 0);
    }
    CHECK(gp_splits(1, 4096) == GP_TARGET_BLOCKS);  // the target is reached
    CHECK(gp_splits(100000, 4096) == 1);

    const int64_t N = 257, one = 3 * N * 8;  // one candidate, one set
    for (int sets : {1, 2, 4}) {
        // A budget below one candidate still gives chunks of one.
        for (int64_t budget : {int64_t(1), int64_t(8), one * sets - 1})
            CHECK(gp_chunk_rows(budget, N, sets) == 1);
        CHECK(gp_chunk_rows(one * sets, N, sets) == 1);
        CHECK(gp_chunk_rows(2 * one * sets, N, sets) == 2);
        CHECK(gp_chunk_rows(3 * one * sets - 1, N, sets) == 2);
        // A huge budget stops at the grid's extent.
        CHECK(gp_chunk_rows(GP_GRID_Y_MAX * one * sets, N, sets) == GP_GRID_Y_MAX);
        CHECK(gp_chunk_rows(INT64_MAX, N, sets) == GP_GRID_Y_MAX);
        CHECK(gp_chunk_rows(INT64_MAX, 1, sets) == GP_GRID_Y_MAX);
        // The pinned cases of the GPU tests: 13 candidates in chunks of two,
        // three candidates one at a time.
        CHECK(gp_n_chunks(13, gp_chunk_rows(2 * sets * one, N, sets)) == 7);
        CHECK(gp_n_chunks(3, gp_chunk_rows(8, N, sets)) == 3);
    }
    CHECK(GP_GRID_Y_MAX == 65535);
    CHECK(gp_chunk_rows(GP_SCRATCH_BUDGET_BYTES, 1, 1) == GP_GRID_Y_MAX);

    for (int64_t rows : {int64_t(1), int64_t(2), int64_t(7), GP_GRID_Y_MAX})
        for (int64_t B : {int64_t(1), rows - 1, rows, rows + 1, 13 * rows, 13 * rows + 1,
                          int64_t(70000)})
            if (B >= 1) check_cover(B, rows);
    CHECK(gp_n_chunks(1, GP_GRID_Y_MAX) == 1);
    CHECK(gp_n_chunks(GP_GRID_Y_MAX + 1, GP_GRID_Y_MAX) == 2);

    if (g_failed == 0) std::printf("gp_plan: all checks passed\n");
    return g_failed == 0 ? 0 : 1;
}
