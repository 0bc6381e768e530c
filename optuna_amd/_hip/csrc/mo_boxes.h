// K6e: box decomposition of the non-dominated region for (q)LogEHVI, on the
// device (fp64, gfx950, M = 2..4 objectives, Q draws per launch train).
//
// The host algorithm (_hypervolume/box_decomposition.py, Lacour-Klamroth-
// Fonseca Alg. 2 applied twice) only compares and copies coordinates, so the
// device returns the same set of boxes bit for bit. What the design rests on:
// points are inserted in lexicographic order, a bound u is hit only if the
// point is strictly below it in every coordinate, and u[0] is either ref[0] or
// the objective-0 value of an earlier point. So only bounds with
// u[0] == ref[0] ("active") can ever be hit; a child made in column 0 is
// frozen for the rest of the pass and is streamed out to global memory, a
// child made in a column j >= 1 stays active. The active list is short and
// lives in LDS; one workgroup walks the points of one draw.
//
// Launch train of a batch of draws (a "slot" is a draw's place in the train):
//   k_box_prepare x2   unique + Pareto + lexsort of base|extra rows   -> P1
//   k_box_upper_bounds<M, false>   upper-bound set of P1 under ref    -> U1
//   k_box_prepare x2   the same on -U1                                -> P2
//   k_box_upper_bounds<M, true>    upper-bound set of P2 under +inf   -> U2, D2
//   k_box_emit         boxes of (U2, D2), compacted per slot
//   k_box_pack         the slots' boxes one after another (after the one sync)
//
// Nothing is sorted and no atomics are used: ranks come from all-pairs
// counting, slots of appended entries from in-order prefix sums, so a run is
// reproducible. Every append is bounds-checked; past a capacity the kernels
// keep counting, and the host relaunches those draws once at the counted size.
#pragma once

#include <cmath>
#include <limits>

#include "hip_common.h"

constexpr int BOX_THREADS = 256;
constexpr int BOX_WAVES = BOX_THREADS / 64;
constexpr int BOX_MAX_Q = 65535;
// Static LDS of k_box_upper_bounds next to the dynamic active list.
constexpr size_t BOX_STATIC_LDS = 1024;
// Device bytes one launch train may lay over the workspace; more draws than
// fit go in further trains.
constexpr size_t BOX_TRAIN_BUDGET_BYTES = size_t(1) << 30;

enum BoxStatus : int32_t { BOX_OK = 0, BOX_ACTIVE_OVERFLOW = 1, BOX_OUT_OVERFLOW = 2 };

// Per-slot counters, one int32 array each of `slots` entries.
struct BoxCounters {
    int32_t* status;  // BoxStatus
    int32_t* n_p1;    // points of pass 1
    int32_t* n_u1;    // bounds pass 1 needs (may exceed its capacity)
    int32_t* n_p2;
    int32_t* n_u2;
    int32_t* n_box;
};

// Row i of a slot: the shared base rows first, then the slot's own rows.
template <int M>
__device__ __forceinline__ void box_row(const double* __restrict__ base, int n0,
                                        const double* __restrict__ own, int i,
                                        double sign, double (&r)[M]) {
    const double* src = i < n0 ? base + (int64_t)i * M : own + (int64_t)(i - n0) * M;
#pragma unroll
    for (int j = 0; j < M; ++j) r[j] = sign * src[j];
}

// PHASE 0: flag[i] = row i is below ref, is no copy of an earlier row and is
// not dominated. PHASE 1: the flagged rows written by lexicographic rank.
// Grid (row tiles, slots); thread = row; all rows of the slot stream through
// an LDS tile. `ids` maps a slot to the draw whose rows it takes (nullptr:
// the slot itself), `counts` gives the slot's number of own rows (nullptr:
// n_own for every slot).
template <int M, int PHASE>
__global__ __launch_bounds__(BOX_THREADS)
void k_box_prepare(const double* __restrict__ base, int n0,
                   const double* __restrict__ own, int64_t own_stride, int n_own,
                   const int32_t* __restrict__ ids,
                   const int32_t* __restrict__ counts, double sign,
                   const double* __restrict__ ref,
                   const int32_t* __restrict__ status,
                   int32_t* __restrict__ flag, int64_t flag_stride,
                   double* __restrict__ out, int64_t out_stride,
                   int32_t* __restrict__ n_out) {
    __shared__ double t_row[BOX_THREADS * M];
    __shared__ int32_t t_flag[BOX_THREADS];
    const int slot = blockIdx.y;
    if (status[slot] != BOX_OK) return;
    const int n = n0 + (counts ? counts[slot] : n_own);
    if ((int64_t)blockIdx.x * BOX_THREADS >= n && blockIdx.x > 0) return;
    const double* mine = own + (int64_t)(ids ? ids[slot] : slot) * own_stride;
    int32_t* my_flag = flag + (int64_t)slot * flag_stride;
    const int i = blockIdx.x * BOX_THREADS + threadIdx.x;
    const bool have = i < n;
    double r[M];
    bool ok = have;
    if (have) {
        box_row<M>(base, n0, mine, i, sign, r);
        if (PHASE == 0) {
#pragma unroll
            for (int j = 0; j < M; ++j) ok = ok && r[j] < ref[j];
        } else {
            ok = my_flag[i] != 0;
        }
    } else {
#pragma unroll
        for (int j = 0; j < M; ++j) r[j] = 0.0;
    }
    int rank = 0, total = 0;
    for (int t0 = 0; t0 < n; t0 += BOX_THREADS) {
        const int m = min(BOX_THREADS, n - t0);
        __syncthreads();
        if ((int)threadIdx.x < m) {
            double o[M];
            box_row<M>(base, n0, mine, t0 + threadIdx.x, sign, o);
#pragma unroll
            for (int j = 0; j < M; ++j) t_row[threadIdx.x * M + j] = o[j];
            if (PHASE == 1) t_flag[threadIdx.x] = my_flag[t0 + threadIdx.x];
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            bool all_le = true, all_eq = true, lex_lt = false, decided = false;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const double o = t_row[k * M + j];
                all_le = all_le && o <= r[j];
                all_eq = all_eq && o == r[j];
                if (!decided && o != r[j]) {
                    decided = true;
                    lex_lt = o < r[j];
                }
            }
            if (PHASE == 0) {
                // an equal earlier row, or a row that dominates this one
                if (all_eq ? t0 + k < i : all_le) ok = false;
            } else if (t_flag[k]) {
                total += 1;
                rank += lex_lt ? 1 : 0;
            }
        }
    }
    if (PHASE == 0) {
        if (have) my_flag[i] = ok ? 1 : 0;
    } else {
        if (have && ok) {
            double* dst = out + (int64_t)slot * out_stride + (int64_t)rank * M;
#pragma unroll
            for (int j = 0; j < M; ++j) dst[j] = r[j];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) n_out[slot] = total;
    }
}

// Exclusive prefix of v over the block in thread order, and the block total.
// `wsum` holds BOX_WAVES entries.
__device__ __forceinline__ unsigned long long box_scan(unsigned long long v,
                                                       unsigned long long* wsum,
                                                       unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    __syncthreads();  // the previous user of `wsum` is done
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BOX_WAVES; ++w) {
        const unsigned long long c = wsum[w];
        if (w < wave) before += c;
        total += c;
    }
    return before + inc - v;
}

// Slot of a kept thread among the kept threads of the block, by a wavefront
// ballot and the wavefront counts in order; `total` is the block's count.
__device__ __forceinline__ int box_ballot_slot(bool keep, int* wcnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();  // the previous user of `wcnt` is done
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BOX_WAVES; ++w) {
        const int c = wcnt[w];
        if (w < wave) before += c;
        total += c;
    }
    return before + pre;
}

// The active list in LDS, structure of arrays over `cap` entries: coordinates
// 1..M-1, then the defining-point indices 1..M-1. Coordinate 0 of an active
// entry is ref[0] and its defining point 0 is the dummy, so neither is held.
// A defining point is the index of a point of the pass, or BOX_DUMMY for the
// dummy point of its own row (ref[j] in column j, -inf elsewhere). A hit entry
// that leaves no active child is marked dead: coordinate 1 = -inf, which no
// point is below.
constexpr int32_t BOX_DUMMY = -1;

template <int M>
struct BoxActive {
    double* u;
    int32_t* d;
    int cap;
    __device__ double& coord(int j, int e) const { return u[(j - 1) * cap + e]; }
    __device__ int32_t& defp(int j, int e) const { return d[(j - 1) * cap + e]; }
    __device__ bool dead(int e) const { return u[e] == -INFINITY; }
};

// Stable removal of the dead entries of [0, tail); returns the new tail.
// Round r reads entries [256 r, 256 r + 256) and writes at or below them, after
// a barrier, so no unread entry is overwritten.
template <int M>
__device__ int box_compact(const BoxActive<M>& A, int tail, int* wcnt) {
    int kept = 0;
    for (int r0 = 0; r0 < tail; r0 += BOX_THREADS) {
        const int e = r0 + threadIdx.x;
        const bool live = e < tail && !A.dead(e);
        double u[M];
        int32_t d[M];
        if (live) {
#pragma unroll
            for (int j = 1; j < M; ++j) {
                u[j] = A.coord(j, e);
                d[j] = A.defp(j, e);
            }
        }
        int total;
        const int at = kept + box_ballot_slot(live, wcnt, total);
        if (live) {
#pragma unroll
            for (int j = 1; j < M; ++j) {
                A.coord(j, at) = u[j];
                A.defp(j, at) = d[j];
            }
        }
        kept += total;
    }
    __syncthreads();
    return kept;
}

// Which columns j >= 1 of a hit entry get a child: p[j] >= max over the other
// rows' defining points of their coordinate j (column 0 always passes and is
// not in the mask). Row 0 of an active entry is the dummy.
template <int M>
__device__ __forceinline__ unsigned box_children(const double* __restrict__ pts,
                                                 const double (&p)[M],
                                                 const int32_t (&d)[M]) {
    unsigned mask = 0;
#pragma unroll
    for (int j = 1; j < M; ++j) {
        double thr = -INFINITY;
#pragma unroll
        for (int i = 1; i < M; ++i)
            if (i != j && d[i] != BOX_DUMMY) thr = fmax(thr, pts[(int64_t)d[i] * M + j]);
        if (p[j] >= thr) mask |= 1u << j;
    }
    return mask;
}

// Per-thread tallies of a step, packed for one scan: 21 bits each.
constexpr int BOX_FIELD = 21;
constexpr unsigned long long BOX_FIELD_MASK = (1ull << BOX_FIELD) - 1ull;
constexpr int BOX_MAX_ACTIVE = (1 << BOX_FIELD) / 4;  // 3 * cap < 2^21

// One workgroup per slot: Alg. 2 over the slot's sorted points. Frozen bounds
// (and with EMIT_DEF their defining points) are appended to the slot's region
// of ub_out / def_out in a fixed order; the live active entries follow at the
// end. need[slot] is the number of bounds whether or not they all fitted.
template <int M, bool EMIT_DEF>
__global__ __launch_bounds__(BOX_THREADS)
void k_box_upper_bounds(const double* __restrict__ pts_all, int64_t pts_stride,
                        const int32_t* __restrict__ n_pts,
                        const double* __restrict__ ref, int active_cap,
                        int out_cap, double* __restrict__ ub_all,
                        int32_t* __restrict__ def_all, int32_t* __restrict__ need,
                        int32_t* __restrict__ status) {
    extern __shared__ double box_lds[];
    __shared__ unsigned long long wsum[BOX_WAVES];
    __shared__ int wcnt[BOX_WAVES];
    const int slot = blockIdx.x;
    if (status[slot] != BOX_OK) return;
    const double* pts = pts_all + (int64_t)slot * pts_stride;
    double* ub = ub_all + (int64_t)slot * out_cap * M;
    int32_t* def = EMIT_DEF ? def_all + (int64_t)slot * out_cap * M : nullptr;
    const int n = n_pts[slot];
    const int tid = threadIdx.x;
    BoxActive<M> A{box_lds, reinterpret_cast<int32_t*>(box_lds + (size_t)(M - 1) * active_cap),
                   active_cap};
    double rf[M];
#pragma unroll
    for (int j = 0; j < M; ++j) rf[j] = ref[j];
    if (tid == 0) {
#pragma unroll
        for (int j = 1; j < M; ++j) {
            A.coord(j, 0) = rf[j];
            A.defp(j, 0) = BOX_DUMMY;
        }
    }
    __syncthreads();
    int tail = 1;     // entries in use, dead ones included
    int n_dead = 0;
    int n_frozen = 0;  // bounds streamed out so far (counted past out_cap too)
    bool overflow = false;

    // The point of a step is loaded one step ahead: its latency would
    // otherwise be paid once per step, with nothing to hide it behind.
    double p_next[M];
#pragma unroll
    for (int j = 0; j < M; ++j) p_next[j] = n > 0 ? pts[j] : 0.0;
    for (int s = 0; s < n && !overflow; ++s) {
        double p[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            p[j] = p_next[j];
            if (s + 1 < n) p_next[j] = pts[(int64_t)(s + 1) * M + j];
        }
        if (!(p[0] < rf[0])) continue;  // uniform: no active bound is hit
        if (2 * n_dead > tail && tail > BOX_THREADS) {
            tail = box_compact<M>(A, tail, wcnt);
            n_dead = 0;
        }
        for (int attempt = 0;; ++attempt) {
            // Tally: hits, active children beyond the first of a hit, hits
            // that leave no active child.
            unsigned long long tally = 0;
            for (int e = tid; e < tail; e += BOX_THREADS) {
                bool hit = true;
                int32_t d[M];
#pragma unroll
                for (int j = 1; j < M; ++j) hit = hit && p[j] < A.coord(j, e);
                if (!hit) continue;
#pragma unroll
                for (int j = 1; j < M; ++j) d[j] = A.defp(j, e);
                d[0] = BOX_DUMMY;
                const int c = __popc(box_children<M>(pts, p, d));
                tally += (1ull << BOX_FIELD) + (c > 1 ? (unsigned long long)(c - 1) : 0ull) +
                         (c == 0 ? 1ull << (2 * BOX_FIELD) : 0ull);
            }
            if (!__syncthreads_or(tally != 0)) break;  // no bound hit
            unsigned long long total;
            const unsigned long long before = box_scan(tally, wsum, total);
            const int extra = (int)(total & BOX_FIELD_MASK);
            if (tail + extra > active_cap) {
                if (attempt == 0 && n_dead > 0) {
                    tail = box_compact<M>(A, tail, wcnt);
                    n_dead = 0;
                    continue;  // entries moved: tally again
                }
                overflow = true;
                break;
            }
            int x_at = tail + (int)(before & BOX_FIELD_MASK);
            int f_at = n_frozen + (int)((before >> BOX_FIELD) & BOX_FIELD_MASK);
            for (int e = tid; e < tail; e += BOX_THREADS) {
                bool hit = true;
                double u[M];
                int32_t d[M];
#pragma unroll
                for (int j = 1; j < M; ++j) {
                    u[j] = A.coord(j, e);
                    hit = hit && p[j] < u[j];
                }
                if (!hit) continue;
#pragma unroll
                for (int j = 1; j < M; ++j) d[j] = A.defp(j, e);
                d[0] = BOX_DUMMY;
                const unsigned kids = box_children<M>(pts, p, d);
                // column 0: the frozen child
                if (f_at < out_cap) {
                    ub[(int64_t)f_at * M] = p[0];
#pragma unroll
                    for (int j = 1; j < M; ++j) ub[(int64_t)f_at * M + j] = u[j];
                    if (EMIT_DEF) {
                        def[(int64_t)f_at * M] = s;
#pragma unroll
                        for (int j = 1; j < M; ++j) def[(int64_t)f_at * M + j] = d[j];
                    }
                }
                f_at += 1;
                // columns j >= 1: the first child takes the hit entry's place,
                // the others go to the tail
                bool first = true;
#pragma unroll
                for (int j = 1; j < M; ++j) {
                    if (!((kids >> j) & 1u)) continue;
                    if (first) {
                        first = false;
                        A.coord(j, e) = p[j];
                        A.defp(j, e) = s;
                    } else {
                        // x_at < tail + extra <= active_cap
#pragma unroll
                        for (int k = 1; k < M; ++k) {
                            A.coord(k, x_at) = k == j ? p[k] : u[k];
                            A.defp(k, x_at) = k == j ? s : d[k];
                        }
                        x_at += 1;
                    }
                }
                if (first) A.coord(1, e) = -INFINITY;
            }
            tail += extra;
            n_frozen += (int)((total >> BOX_FIELD) & BOX_FIELD_MASK);
            n_dead += (int)((total >> (2 * BOX_FIELD)) & BOX_FIELD_MASK);
            __syncthreads();
            break;
        }
    }
    if (overflow) {
        if (tid == 0) status[slot] = BOX_ACTIVE_OVERFLOW;
        return;
    }
    tail = box_compact<M>(A, tail, wcnt);
    for (int e = tid; e < tail; e += BOX_THREADS) {
        const int64_t f = (int64_t)n_frozen + e;
        if (f >= out_cap) break;
        ub[f * M] = rf[0];
        if (EMIT_DEF) def[f * M] = BOX_DUMMY;
#pragma unroll
        for (int j = 1; j < M; ++j) {
            ub[f * M + j] = A.coord(j, e);
            if (EMIT_DEF) def[f * M + j] = A.defp(j, e);
        }
    }
    if (tid == 0) {
        need[slot] = n_frozen + tail;
        if (n_frozen + tail > out_cap) status[slot] = BOX_OUT_OVERFLOW;
    }
}

// Boxes of the second pass's bounds, one workgroup per slot. In the negated
// space of that pass the lower corner of a bound's box is the running maximum
// of its defining points, the upper corner the bound itself with +inf in
// column 0; negated twice, these are the max-space corners as they stand.
// Empty boxes are dropped and the rest written in order to the slot's region.
template <int M>
__global__ __launch_bounds__(BOX_THREADS)
void k_box_emit(const double* __restrict__ pts_all, int64_t pts_stride,
                const double* __restrict__ ub_all, const int32_t* __restrict__ def_all,
                int out_cap, const int32_t* __restrict__ n_ub,
                const int32_t* __restrict__ status, double eps,
                double* __restrict__ lo_all, double* __restrict__ iv_all,
                int32_t* __restrict__ n_box) {
    __shared__ int wcnt[BOX_WAVES];
    const int slot = blockIdx.x;
    if (status[slot] != BOX_OK) return;
    const double* pts = pts_all + (int64_t)slot * pts_stride;
    const double* ub = ub_all + (int64_t)slot * out_cap * M;
    const int32_t* def = def_all + (int64_t)slot * out_cap * M;
    double* lo_out = lo_all + (int64_t)slot * out_cap * M;
    double* iv_out = iv_all + (int64_t)slot * out_cap * M;
    const int n = n_ub[slot];  // <= out_cap: the slot's status is BOX_OK
    int kept = 0;
    for (int r0 = 0; r0 < n; r0 += BOX_THREADS) {
        const int e = r0 + threadIdx.x;
        bool keep = e < n;
        double lo[M], iv[M];
        if (keep) {
            int32_t d[M];
#pragma unroll
            for (int j = 0; j < M; ++j) d[j] = def[(int64_t)e * M + j];
            // a dummy in row 0 puts +inf under the +inf upper corner: empty
            keep = d[0] != BOX_DUMMY;
#pragma unroll
            for (int j = 0; j < M && keep; ++j) {
                double lower, upper;
                if (j == 0) {
                    lower = pts[(int64_t)d[0] * M];
                    upper = INFINITY;
                } else {
                    lower = -INFINITY;
#pragma unroll
                    for (int i = 0; i < j; ++i)
                        if (d[i] != BOX_DUMMY) lower = fmax(lower, pts[(int64_t)d[i] * M + j]);
                    upper = ub[(int64_t)e * M + j];
                }
                keep = !(upper <= lower);
                lo[j] = lower;
                iv[j] = fmax(upper - lower, eps);
            }
        }
        int total;
        const int at = kept + box_ballot_slot(keep, wcnt, total);
        if (keep) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                lo_out[(int64_t)at * M + j] = lo[j];
                iv_out[(int64_t)at * M + j] = iv[j];
            }
        }
        kept += total;
    }
    if (threadIdx.x == 0) n_box[slot] = kept;
}

// The finished slots' boxes one after another: slot s goes to row dst[s]
// (dst[s] < 0: the slot is left out). Grid (tiles, slots).
__global__ void k_box_pack(const double* __restrict__ lo_all,
                           const double* __restrict__ iv_all, int64_t slot_stride,
                           const int32_t* __restrict__ n_box,
                           const int64_t* __restrict__ dst, int M,
                           double* __restrict__ lo, double* __restrict__ iv) {
    const int slot = blockIdx.y;
    if (dst[slot] < 0) return;
    const int64_t n = (int64_t)n_box[slot] * M;
    const int64_t from = (int64_t)slot * slot_stride, to = dst[slot] * M;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * blockDim.x) {
        lo[to + k] = lo_all[from + k];
        iv[to + k] = iv_all[from + k];
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

// LDS one workgroup may take, as the device reports it.
static int box_device_lds_bytes() {
    static int bytes = -1;
    if (bytes < 0) {
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        HIP_CHECK(hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    }
    return bytes;
}

static size_t box_active_entry_bytes(int M) { return (size_t)(M - 1) * 12; }

// Bound capacities of the two passes for n points per draw. Exact for two and
// three objectives (n + 1 and 2 n + 1 bounds of n points); an estimate for
// four, which the counted relaunch corrects.
static int64_t box_bound_cap(int M, int64_t n) {
    return M == 2 ? n + 1 : M == 3 ? 2 * n + 1 : 12 * n + 64;
}
static int64_t box_second_cap(int M, int64_t cap1) {
    return M == 4 ? 4 * cap1 : box_bound_cap(M, cap1);
}

struct BoxSlotResult {
    int32_t status = BOX_OK, n_u1 = 0, n_u2 = 0;
    std::vector<double> lo, iv;  // (n_box, M) each, when status == BOX_OK
};

// One launch train over the draws `ids` at the given capacities.
template <int M>
static void box_run_train(const double* base, int n0, const double* extra, int R,
                          int64_t Q, const double* ref, const std::vector<int32_t>& ids,
                          int active_cap, int64_t cap1, int64_t cap2,
                          std::vector<BoxSlotResult>& results) {
    const int64_t S = (int64_t)ids.size();
    const int64_t NP = std::max<int64_t>(n0 + R, 1);
    if (cap1 > INT32_MAX / 8 || cap2 > INT32_MAX / 8 || NP > INT32_MAX / 8)
        throw std::runtime_error("box_decompose: front too large");
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto s_base = L.add<double>((size_t)std::max(n0, 1) * M);
    const auto s_extra = L.add<double>((size_t)std::max<int64_t>(Q * R, 1) * M);
    const auto s_ref = L.add<double>(2 * M);  // ref | +inf
    const auto s_ids = L.add<int32_t>(S);
    const auto s_cnt = L.add<int32_t>(6 * S);
    const auto s_flag = L.add<int32_t>((size_t)S * std::max(NP, cap1));
    const auto s_p1 = L.add<double>((size_t)S * NP * M);
    const auto s_u1 = L.add<double>((size_t)S * cap1 * M);
    const auto s_p2 = L.add<double>((size_t)S * cap1 * M);
    const auto s_u2 = L.add<double>((size_t)S * cap2 * M);
    const auto s_d2 = L.add<int32_t>((size_t)S * cap2 * M);
    const auto s_lo = L.add<double>((size_t)S * cap2 * M);
    const auto s_iv = L.add<double>((size_t)S * cap2 * M);
    const auto s_dst = L.add<int64_t>(S);
    const auto s_plo = L.add<double>((size_t)S * cap2 * M);
    const auto s_piv = L.add<double>((size_t)S * cap2 * M);
    char* ws = g_ws.ensure_bytes(L.bytes());
    double *d_base = s_base.in(ws), *d_extra = s_extra.in(ws), *d_ref = s_ref.in(ws);
    int32_t* d_ids = s_ids.in(ws);
    int32_t* d_cnt = s_cnt.in(ws);
    const BoxCounters c{d_cnt, d_cnt + S, d_cnt + 2 * S, d_cnt + 3 * S, d_cnt + 4 * S,
                        d_cnt + 5 * S};
    int32_t* d_flag = s_flag.in(ws);
    const int64_t flag_stride = std::max(NP, cap1);

    double consts[2 * M];
    for (int j = 0; j < M; ++j) {
        consts[j] = ref[j];
        consts[M + j] = std::numeric_limits<double>::infinity();
    }
    g_ws.begin_uploads();
    g_ws.h2d(d_base, base, (size_t)n0 * M * 8, st);
    g_ws.h2d(d_extra, extra, (size_t)Q * R * M * 8, st);
    g_ws.h2d(d_ref, consts, sizeof(consts), st);
    g_ws.h2d(d_ids, ids.data(), S * 4, st);
    HIP_CHECK(hipMemsetAsync(d_cnt, 0, 6 * S * 4, st));

    const size_t lds = (size_t)active_cap * box_active_entry_bytes(M);
    static bool lds_set = false;  // per instantiation
    if (!lds_set) {
        const int want = box_device_lds_bytes() - (int)BOX_STATIC_LDS;
        HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_box_upper_bounds<M, false>),
            hipFuncAttributeMaxDynamicSharedMemorySize, want));
        HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_box_upper_bounds<M, true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, want));
        lds_set = true;
    }
    const unsigned tiles1 = (unsigned)((NP + BOX_THREADS - 1) / BOX_THREADS);
    const unsigned tiles2 = (unsigned)((cap1 + BOX_THREADS - 1) / BOX_THREADS);
    const dim3 blk(BOX_THREADS);
    // pass 1: base | extra rows of the draw -> P1 -> U1
    hipLaunchKernelGGL((k_box_prepare<M, 0>), dim3(tiles1, (unsigned)S), blk, 0, st, d_base,
                       n0, d_extra, (int64_t)R * M, R, d_ids, (const int32_t*)nullptr, 1.0,
                       d_ref, c.status, d_flag, flag_stride, s_p1.in(ws), NP * M, c.n_p1);
    hipLaunchKernelGGL((k_box_prepare<M, 1>), dim3(tiles1, (unsigned)S), blk, 0, st, d_base,
                       n0, d_extra, (int64_t)R * M, R, d_ids, (const int32_t*)nullptr, 1.0,
                       d_ref, c.status, d_flag, flag_stride, s_p1.in(ws), NP * M, c.n_p1);
    hipLaunchKernelGGL((k_box_upper_bounds<M, false>), dim3((unsigned)S), blk, lds, st,
                       s_p1.in(ws), NP * M, c.n_p1, d_ref, active_cap, (int)cap1,
                       s_u1.in(ws), (int32_t*)nullptr, c.n_u1, c.status);
    // pass 2: -U1 -> P2 -> U2 with defining points, under +inf
    hipLaunchKernelGGL((k_box_prepare<M, 0>), dim3(tiles2, (unsigned)S), blk, 0, st, d_base,
                       0, s_u1.in(ws), cap1 * M, 0, (const int32_t*)nullptr, c.n_u1, -1.0,
                       d_ref + M, c.status, d_flag, flag_stride, s_p2.in(ws), cap1 * M,
                       c.n_p2);
    hipLaunchKernelGGL((k_box_prepare<M, 1>), dim3(tiles2, (unsigned)S), blk, 0, st, d_base,
                       0, s_u1.in(ws), cap1 * M, 0, (const int32_t*)nullptr, c.n_u1, -1.0,
                       d_ref + M, c.status, d_flag, flag_stride, s_p2.in(ws), cap1 * M,
                       c.n_p2);
    hipLaunchKernelGGL((k_box_upper_bounds<M, true>), dim3((unsigned)S), blk, lds, st,
                       s_p2.in(ws), cap1 * M, c.n_p2, d_ref + M, active_cap, (int)cap2,
                       s_u2.in(ws), s_d2.in(ws), c.n_u2, c.status);
    hipLaunchKernelGGL((k_box_emit<M>), dim3((unsigned)S), blk, 0, st, s_p2.in(ws),
                       cap1 * M, s_u2.in(ws), s_d2.in(ws), (int)cap2, c.n_u2, c.status,
                       1e-12, s_lo.in(ws), s_iv.in(ws), c.n_box);
    std::vector<int32_t> cnt(6 * S);
    HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, 6 * S * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());

    std::vector<int64_t> dst(S, -1);
    int64_t rows = 0, widest = 0;
    for (int64_t s = 0; s < S; ++s) {
        BoxSlotResult& r = results[ids[s]];
        r.status = cnt[s];
        r.n_u1 = cnt[2 * S + s];
        r.n_u2 = cnt[4 * S + s];
        if (r.status != BOX_OK) continue;
        dst[s] = rows;
        rows += cnt[5 * S + s];
        widest = std::max<int64_t>(widest, cnt[5 * S + s]);
    }
    if (rows == 0) return;
    std::vector<double> lo((size_t)rows * M), iv((size_t)rows * M);
    g_ws.begin_uploads();
    g_ws.h2d(s_dst.in(ws), dst.data(), S * 8, st);
    const unsigned ptiles =
        (unsigned)std::min<int64_t>((widest * M + BOX_THREADS - 1) / BOX_THREADS, 1024);
    hipLaunchKernelGGL(k_box_pack, dim3(ptiles, (unsigned)S), blk, 0, st, s_lo.in(ws),
                       s_iv.in(ws), cap2 * M, c.n_box, s_dst.in(ws), M, s_plo.in(ws),
                       s_piv.in(ws));
    HIP_CHECK(hipMemcpyAsync(lo.data(), s_plo.in(ws), lo.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(iv.data(), s_piv.in(ws), iv.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    for (int64_t s = 0; s < S; ++s) {
        if (dst[s] < 0) continue;
        BoxSlotResult& r = results[ids[s]];
        const size_t at = (size_t)dst[s] * M, len = (size_t)cnt[5 * S + s] * M;
        r.lo.assign(lo.begin() + at, lo.begin() + at + len);
        r.iv.assign(iv.begin() + at, iv.begin() + at + len);
    }
}

// Workspace bytes of one slot of a train, to split the draws over trains.
static size_t box_slot_bytes(int M, int64_t NP, int64_t cap1, int64_t cap2) {
    return (size_t)M * ((size_t)NP * 8 + (size_t)cap1 * 16 + (size_t)cap2 * 44) +
           (size_t)std::max(NP, cap1) * 4 + 64;
}

template <int M>
static void box_run(const double* base, int n0, const double* extra, int R, int64_t Q,
                    const double* ref, const std::vector<int32_t>& ids, int active_cap,
                    int64_t cap1, int64_t cap2, std::vector<BoxSlotResult>& results) {
    const size_t per_slot = box_slot_bytes(M, std::max<int64_t>(n0 + R, 1), cap1, cap2);
    const size_t chunk = std::max<size_t>(1, BOX_TRAIN_BUDGET_BYTES / per_slot);
    for (size_t at = 0; at < ids.size(); at += chunk) {
        const std::vector<int32_t> part(ids.begin() + at,
                                        ids.begin() + std::min(ids.size(), at + chunk));
        box_run_train<M>(base, n0, extra, R, Q, ref, part, active_cap, cap1, cap2, results);
    }
}

template <int M>
static py::tuple box_decompose_m(const arr_f64& base, const arr_f64& extra,
                                 const arr_f64& ref, int64_t active_cap_arg,
                                 int64_t out_cap_arg) {
    const int n0 = (int)base.shape(0);
    const int64_t Q = extra.shape(0);
    const int R = (int)extra.shape(1);
    const int64_t n = (int64_t)n0 + R;
    const int64_t lds_cap =
        ((int64_t)box_device_lds_bytes() - (int64_t)BOX_STATIC_LDS) /
        (int64_t)box_active_entry_bytes(M);
    int64_t active_cap = std::min<int64_t>(lds_cap, BOX_MAX_ACTIVE);
    if (active_cap_arg > 0) active_cap = std::min(active_cap, active_cap_arg);
    if (active_cap < 1) throw std::runtime_error("box_decompose: no LDS for the active list");

    std::vector<BoxSlotResult> results(Q);
    std::vector<int32_t> all(Q);
    for (int64_t q = 0; q < Q; ++q) all[q] = (int32_t)q;
    const int64_t cap1 = out_cap_arg > 0 ? out_cap_arg : box_bound_cap(M, n);
    const int64_t cap2 = out_cap_arg > 0 ? out_cap_arg : box_second_cap(M, cap1);
    box_run<M>(base.data(), n0, extra.data(), R, Q, ref.data(), all, (int)active_cap, cap1,
               cap2, results);
    // The draws that ran out of room go once more, at the size they counted.
    // A first pass that did not fit leaves the second uncounted: its capacity
    // then comes from the first's exact count.
    std::vector<int32_t> again;
    int64_t need1 = 0, need2 = 0;
    for (int64_t q = 0; q < Q; ++q) {
        const BoxSlotResult& r = results[q];
        if (r.status != BOX_OUT_OVERFLOW) continue;
        again.push_back((int32_t)q);
        need1 = std::max<int64_t>(need1, r.n_u1);
        need2 = std::max<int64_t>(need2, r.n_u1 > cap1 ? box_second_cap(M, r.n_u1) : r.n_u2);
    }
    if (!again.empty())
        box_run<M>(base.data(), n0, extra.data(), R, Q, ref.data(), again, (int)active_cap,
                   std::max(need1, cap1), std::max(need2, cap2), results);

    std::vector<int64_t> host_needed;
    py::array_t<int64_t> offsets(Q + 1);
    int64_t* off = offsets.mutable_data();
    off[0] = 0;
    for (int64_t q = 0; q < Q; ++q) {
        if (results[q].status != BOX_OK) {
            host_needed.push_back(q);
            results[q].lo.clear();
            results[q].iv.clear();
        }
        off[q + 1] = off[q] + (int64_t)results[q].lo.size() / M;
    }
    py::array_t<double> lo({off[Q], (int64_t)M}), iv({off[Q], (int64_t)M});
    for (int64_t q = 0; q < Q; ++q) {
        const size_t len = results[q].lo.size();
        if (len == 0) continue;
        memcpy(lo.mutable_data() + off[q] * M, results[q].lo.data(), len * 8);
        memcpy(iv.mutable_data() + off[q] * M, results[q].iv.data(), len * 8);
    }
    return py::make_tuple(lo, iv, offsets,
                          py::array_t<int64_t>(host_needed.size(), host_needed.data()));
}

// Max-space boxes (lower corner, clamped interval) of the non-dominated region
// of base | extra[q] under ref, for every draw q: (lo, iv, offsets,
// host_needed). A draw in host_needed could not be finished here (its active
// list outgrew the LDS, or a four-objective relaunch still ran out of room);
// it has no rows in lo / iv and is the caller's to decompose.
py::tuple box_decompose(const arr_f64& base, const arr_f64& extra, const arr_f64& ref,
                        int64_t active_cap, int64_t out_cap) {
    const int64_t M = ref.size();
    if (ref.ndim() != 1 || M < 2 || M > 4)
        throw std::runtime_error("box_decompose: 2 to 4 objectives");
    if (base.ndim() != 2 || base.shape(1) != M)
        throw std::runtime_error("box_decompose: base must be (n0, M)");
    if (extra.ndim() != 3 || extra.shape(2) != M)
        throw std::runtime_error("box_decompose: extra must be (Q, R, M)");
    if (extra.shape(0) < 1 || extra.shape(0) > BOX_MAX_Q)
        throw std::runtime_error("box_decompose: 1 to 65535 draws");
    if (active_cap < 0 || out_cap < 0)
        throw std::runtime_error("box_decompose: negative capacity");
    if (!device_available()) throw std::runtime_error("box_decompose: no device");
    if (M == 2) return box_decompose_m<2>(base, extra, ref, active_cap, out_cap);
    if (M == 3) return box_decompose_m<3>(base, extra, ref, active_cap, out_cap);
    return box_decompose_m<4>(base, extra, ref, active_cap, out_cap);
}

// The LDS a workgroup may take as the device reports it, and the active-list
// capacity that follows for M objectives.
py::tuple box_decompose_limits(int64_t M) {
    if (M < 2 || M > 4) throw std::runtime_error("box_decompose_limits: 2 to 4 objectives");
    const int lds = box_device_lds_bytes();
    return py::make_tuple(lds, ((int64_t)lds - (int64_t)BOX_STATIC_LDS) /
                                   (int64_t)box_active_entry_bytes((int)M));
}
