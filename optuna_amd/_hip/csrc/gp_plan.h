// How the GP sessions cut an evaluation into launches: candidates per chunk
// from the scratch budget, and workgroups per candidate towards a target
// total. Plain C++17 with nothing of HIP in it, so tests/cpp/gp_plan_check.cpp
// checks it on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

// A grid's y (and z) extent: k_gp_cross_cov takes one candidate per y.
constexpr int64_t GP_GRID_Y_MAX = 65535;
// A small batch (a local-search step has 10 candidates) spreads the work of
// each candidate over several workgroups, up to about this many in all.
constexpr int GP_TARGET_BLOCKS = 1024;
// Default ceiling on the (rows, N) scratch (the K / MP / V sets) of one
// evaluation; candidates beyond it are evaluated in chunks.
constexpr int64_t GP_SCRATCH_BUDGET_BYTES = int64_t(256) << 20;

// Candidates per chunk: n_sets sets of K / MP / V, (rows, N) doubles each, fit
// the budget. One candidate is the floor, the grid's extent the ceiling.
inline int64_t gp_chunk_rows(int64_t budget_bytes, int64_t N, int n_sets) {
    return std::clamp<int64_t>(budget_bytes / (3 * N * 8 * n_sets), 1, GP_GRID_Y_MAX);
}

inline int64_t gp_n_chunks(int64_t B, int64_t rows) { return (B + rows - 1) / rows; }

// Workgroups per candidate for a chunk of bc >= 1 candidates: towards
// GP_TARGET_BLOCKS in all, at most max_splits >= 1 each.
inline int gp_splits(int64_t bc, int64_t max_splits) {
    return (int)std::clamp<int64_t>((GP_TARGET_BLOCKS + bc - 1) / bc, 1, max_splits);
}

// Partial records that chunks of at most `rows` candidates write:
// bc * gp_splits(bc, max) < GP_TARGET_BLOCKS + bc for every bc and max.
inline size_t gp_part_records(int64_t rows) { return (size_t)(GP_TARGET_BLOCKS + rows); }
