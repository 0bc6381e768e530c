// ---------------------------------------------------------------------------
// Fused suggest: the "above" subset is the ascending-row complement of a short
// sorted exclusion list (below rows + rows invalid for the space), so the
// subset position of a member row is row - lower_bound(excl, row) and no
// position map or compaction pass is needed.
//
// Three launches, split over two native calls so that only the last two sit
// on the path the host waits for:
//   k_fused_fit    above-set coefficients from the resident table and index.
//                  Needs neither candidates nor the below estimator, so
//                  fused_prepare launches it early, into a buffer the history
//                  owns, and the host goes on building those meanwhile.
//   k_fused_score  one block per 64-kernel slice of the above mixture plus one
//                  per (narrower) slice of the below mixture, which fits its
//                  own coefficients into LDS; (m, s) partials per slice.
//   k_fused_merge  log-sum-exp of the above partials -> log g, of the below
//                  partials -> log l; writes [log l - log g | log g | log l].
// ---------------------------------------------------------------------------

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "truncnorm_device.h"

static constexpr int FUSED_MAX_EXCL = 1024;
static constexpr int FUSED_MAX_BELOW = 1024;
static constexpr int FUSED_TILE = 256;

__device__ inline int excl_lower_bound(const int32_t* e, int E, int32_t row) {
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline void write_coeffs(double mu, double sigma, double low,
                                    double high, bool stepped,
                                    double* __restrict__ c1,
                                    double* __restrict__ c2,
                                    double* __restrict__ c3, int64_t idx) {
    const double mass =
        tn::log_gauss_mass((low - mu) / sigma, (high - mu) / sigma);
    if (stepped) {
        c1[idx] = mu;
        c2[idx] = sigma;
        c3[idx] = -mass;
    } else {
        const double inv_var = 1.0 / (sigma * sigma);
        c1[idx] = -0.5 * inv_var;
        c2[idx] = mu * inv_var;
        c3[idx] = -0.5 * mu * mu * inv_var - log(sigma) -
                  0.9189385332046727418 - mass;
    }
}

// Grid (n_tiles, D): each block fits one tile of 256 sorted positions of dim y
// straight from the resident sorted column. It depends on nothing the
// candidates or the below estimator supply, so fused_prepare can launch it
// while the host is still building those.
// domain = alow | ahigh | steps | n_choices (D each). logw == nullptr means
// the caller uploaded custom log-weights; otherwise the dim-0 blocks write the
// default ramp (numpy linspace arithmetic: k*step + start, uncontracted).
__global__ void k_fused_fit(const double* __restrict__ params,
                            const int32_t* __restrict__ sorted,  // (D, s_stride)
                            int64_t s_stride, int64_t Nv,
                            const int32_t* __restrict__ excl, int E,
                            const double* __restrict__ domain, int64_t Na,
                            int64_t D, int consider_endpoints, int magic_clip,
                            double* __restrict__ c1, double* __restrict__ c2,
                            double* __restrict__ c3, double* __restrict__ logw,
                            int64_t w_num, double w_start, double w_step,
                            double log_total, double prior_weight) {
    __shared__ int32_t s_excl[FUSED_MAX_EXCL];
    __shared__ int s_prev[FUSED_TILE];
    __shared__ int s_next[FUSED_TILE];
    __shared__ double s_val[FUSED_TILE];

    const int64_t d = blockIdx.y;
    const double low = domain[d];
    const double high = domain[D + d];
    const bool stepped = domain[2 * D + d] > 0.0;
    const double range = high - low;
    const int i = threadIdx.x;

    for (int e = i; e < E; e += FUSED_TILE) s_excl[e] = excl[e];
    __syncthreads();

    const int64_t K = Na + 1;
    if (blockIdx.x == 0 && i == 0) {
        // Prior kernel: midpoint, full-range width.
        write_coeffs(0.5 * (low + high), range, low, high, stepped, c1, c2, c3,
                     d * K + Na);
        if (d == 0 && logw)
            logw[Na] = (Na == 0) ? 0.0 : log(prior_weight) - log_total;
    }

    const int32_t* col = sorted + d * s_stride;
    const int64_t tile0 = (int64_t)blockIdx.x * FUSED_TILE;
    const int64_t r = tile0 + i;
    int32_t row = -1;
    int lb = 0;
    bool member = false;
    double mu = 0.0;
    if (r < Nv) {
        row = col[r];
        lb = excl_lower_bound(s_excl, E, row);
        member = !(lb < E && s_excl[lb] == row);
        mu = params[(int64_t)row * D + d];
    }
    s_val[i] = mu;
    s_prev[i] = member ? i : -1;
    s_next[i] = member ? i : FUSED_TILE;
    __syncthreads();
    // Inclusive max-scan (last member at or before i) and suffix min-scan
    // (first member at or after i) over the tile's membership flags.
    for (int off = 1; off < FUSED_TILE; off <<= 1) {
        int a = s_prev[i];
        if (i >= off) a = max(a, s_prev[i - off]);
        int b = s_next[i];
        if (i + off < FUSED_TILE) b = min(b, s_next[i + off]);
        __syncthreads();
        s_prev[i] = a;
        s_next[i] = b;
        __syncthreads();
    }
    if (!member) return;
    const int64_t k = (int64_t)row - lb;
    if (k >= Na) return;  // inconsistent inputs: never write out of bounds

    const int pi = (i > 0) ? s_prev[i - 1] : -1;
    const int ni = (i + 1 < FUSED_TILE) ? s_next[i + 1] : FUSED_TILE;
    bool has_prev = pi >= 0, has_next = ni < FUSED_TILE;
    double v_prev = has_prev ? s_val[pi] : low;
    double v_next = has_next ? s_val[ni] : high;
    // No member on that side of the tile: walk the sorted column past
    // excluded rows (at most E steps, in practice one).
    if (!has_prev) {
        for (int64_t j = tile0 - 1; j >= 0; --j) {
            const int32_t rj = col[j];
            const int l = excl_lower_bound(s_excl, E, rj);
            if (!(l < E && s_excl[l] == rj)) {
                v_prev = params[(int64_t)rj * D + d];
                has_prev = true;
                break;
            }
        }
    }
    if (!has_next) {
        for (int64_t j = tile0 + FUSED_TILE; j < Nv; ++j) {
            const int32_t rj = col[j];
            const int l = excl_lower_bound(s_excl, E, rj);
            if (!(l < E && s_excl[l] == rj)) {
                v_next = params[(int64_t)rj * D + d];
                has_next = true;
                break;
            }
        }
    }
    double minsigma = 1e-12;
    if (magic_clip) minsigma = range / fmin(100.0, (double)(Na + 2));
    double sigma = fmax(mu - v_prev, v_next - mu);
    if (!consider_endpoints && Na >= 2) {
        if (!has_prev) {
            sigma = v_next - mu;
        } else if (!has_next) {
            sigma = mu - v_prev;
        }
    }
    sigma = fmin(fmax(sigma, minsigma), range);
    write_coeffs(mu, sigma, low, high, stepped, c1, c2, c3, d * K + k);
    if (d == 0 && logw) {
        double w = 1.0;
        if (k < w_num) {
            w = (w_num > 1 && k == w_num - 1)
                    ? 1.0
                    : __dadd_rn(__dmul_rn((double)k, w_step), w_start);
        }
        logw[k] = log(w) - log_total;
    }
}

// ---------------------------------------------------------------------------
// Fused scoring: the above mixture and the below mixture in one launch.
//
// A block owns a slice of SCORE_SLICE mixture kernels (one per lane) and up to
// SCORE_CAND candidates (SCORE_SG per wavefront), so a coefficient is fetched
// once per block instead of once per candidate. Blocks x < n_above_slices
// score slices of the above mixture from the fitted (D, K) coefficients; the
// trailing blocks are the below mixture: they turn their slice (below_slice
// kernels, at most SCORE_SLICE) of the uploaded (mu, sigma) into coefficients
// in LDS (same formulas as the fit) and score it the same way. Every wavefront reduces its own candidates across its 64
// lanes (maximum first, then one exp per term and a plain sum) and writes one
// (m, s) partial per (slice, candidate); k_fused_merge finishes the job.
// Dims are walked in passes of SCORE_DC so the LDS footprint does not depend
// on D; blockIdx.y walks candidate groups of SCORE_CAND.
// ---------------------------------------------------------------------------

static constexpr int SCORE_SLICE = 64;
static constexpr int SCORE_WAVES = 4;
static constexpr int SCORE_SG = 6;
static constexpr int SCORE_CAND = SCORE_WAVES * SCORE_SG;
static constexpr int SCORE_DC = 24;

__device__ inline double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__device__ inline double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// All-continuous pass: the lane's 3 * SCORE_DC coefficients are loaded back to
// back into registers (rows past dn repeat the last one, so there is no branch
// between the loads), then every candidate of the wavefront takes its two FMAs.
__device__ __forceinline__ void score_pass_cont(const double* q1, const double* q2,
                                                const double* q3, int64_t stride,
                                                int dn, const double* sx,
                                                const double* sx2,
                                                double (&acc)[SCORE_SG]) {
    double r1[SCORE_DC], r2[SCORE_DC], r3[SCORE_DC];
    int64_t o = 0;
#pragma unroll
    for (int d = 0; d < SCORE_DC; ++d) {
        r1[d] = q1[o];
        r2[d] = q2[o];
        r3[d] = q3[o];
        o += (d + 1 < dn) ? stride : 0;
    }
#pragma unroll
    for (int d = 0; d < SCORE_DC; ++d) {
        if (d < dn) {
#pragma unroll
            for (int j = 0; j < SCORE_SG; ++j)
                acc[j] += sx2[j * SCORE_DC + d] * r1[d] + sx[j * SCORE_DC + d] * r2[d] +
                          r3[d];
        }
    }
}

// Pass with stepped dims: those integrate the step cell against (mu, sigma)
// with the cached -logZ; the others keep the quadratic form.
__device__ inline void score_pass_stepped(const double* q1, const double* q2,
                                          const double* q3, int64_t stride, int dn,
                                          const double* __restrict__ steps,  // or null
                                          const double* sx, const double* sx2,
                                          const double* sxl, const double* sxr,
                                          double (&acc)[SCORE_SG]) {
#pragma nounroll
    for (int d = 0; d < dn; ++d) {
        const double a = q1[d * stride];
        const double b = q2[d * stride];
        const double c = q3[d * stride];
        if (steps && steps[d] > 0.0) {
            // One copy of the cell integral's code, not SCORE_SG of them.
            // The loop is kept rolled; acc is rotated through slot 0 so its
            // indices stay static (registers) and SCORE_SG turns restore it.
#pragma nounroll
            for (int j = 0; j < SCORE_SG; ++j) {
                const double t =
                    acc[0] + (tn::log_gauss_mass((sxl[j * SCORE_DC + d] - a) / b,
                                                 (sxr[j * SCORE_DC + d] - a) / b) +
                              c);
#pragma unroll
                for (int i = 0; i + 1 < SCORE_SG; ++i) acc[i] = acc[i + 1];
                acc[SCORE_SG - 1] = t;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SCORE_SG; ++j)
                acc[j] += sx2[j * SCORE_DC + d] * a + sx[j * SCORE_DC + d] * b + c;
        }
    }
}

__global__ __launch_bounds__(SCORE_SLICE * SCORE_WAVES)
void k_fused_score(const double* __restrict__ x,       // (S, D)
                   const double* __restrict__ xedges,  // (S, 2D), read if any_stepped
                   const double* __restrict__ c1,      // (D, K) above coefficients
                   const double* __restrict__ c2,
                   const double* __restrict__ c3,
                   const double* __restrict__ logw,    // (K,)
                   int64_t K, int64_t n_above_slices,
                   const double* __restrict__ bmu,     // (Kb, D)
                   const double* __restrict__ bsig,    // (Kb, D)
                   const double* __restrict__ bw,      // (Kb,)
                   int64_t Kb, int below_slice,
                   const double* __restrict__ domain, int any_stepped,
                   int64_t D, int64_t S,
                   double* __restrict__ part_m,    // (slices, S)
                   double* __restrict__ part_s) {  // (slices, S)
    __shared__ double s_x[SCORE_CAND * SCORE_DC];
    __shared__ double s_x2[SCORE_CAND * SCORE_DC];
    __shared__ double s_xl[SCORE_CAND * SCORE_DC];
    __shared__ double s_xr[SCORE_CAND * SCORE_DC];
    __shared__ double s_bc[3 * SCORE_DC * SCORE_SLICE];  // below blocks only

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t slot = blockIdx.x;
    const bool below = slot >= n_above_slices;
    const int64_t Kmix = below ? Kb : K;
    // Below slices are narrower (see fused_score): building a coefficient
    // costs far more than using it, so they are cut to one per thread.
    const int slice = below ? below_slice : SCORE_SLICE;
    const int64_t k0 = (below ? slot - n_above_slices : slot) * slice;
    const int kn = (int)(Kmix - k0 < slice ? Kmix - k0 : slice);
    const bool active = lane < kn;
    // Idle lanes read their slice's last kernel, so every load is in bounds;
    // their terms are dropped before the reduction.
    const int lc = active ? lane : kn - 1;
    const int64_t s0 = (int64_t)blockIdx.y * SCORE_CAND;
    const int64_t sw = s0 + (int64_t)wave * SCORE_SG;
    const bool wave_busy = sw < S;  // wavefront-uniform

    double acc[SCORE_SG];
    {
        const double lw = below ? log(bw[k0 + lc]) : logw[k0 + lc];
#pragma unroll
        for (int j = 0; j < SCORE_SG; ++j) acc[j] = lw;
    }

    for (int64_t d0 = 0; d0 < D; d0 += SCORE_DC) {
        const int dn = (int)(D - d0 < SCORE_DC ? D - d0 : SCORE_DC);
        if (d0 > 0) __syncthreads();  // the previous pass has read its LDS
        // Candidates past S repeat the last one; nothing is written for them.
        for (int p = threadIdx.x; p < SCORE_CAND * dn; p += blockDim.x) {
            const int c = p / dn;
            const int dl = p - c * dn;
            const int64_t s = s0 + c < S ? s0 + c : S - 1;
            const double v = x[s * D + d0 + dl];
            s_x[c * SCORE_DC + dl] = v;
            s_x2[c * SCORE_DC + dl] = v * v;
            if (any_stepped) {
                s_xl[c * SCORE_DC + dl] = xedges[s * 2 * D + d0 + dl];
                s_xr[c * SCORE_DC + dl] = xedges[s * 2 * D + D + d0 + dl];
            }
        }
        if (below) {
            for (int p = threadIdx.x; p < kn * dn; p += blockDim.x) {
                const int kl = p / dn;
                const int dl = p - kl * dn;
                const int64_t d = d0 + dl;
                write_coeffs(bmu[(k0 + kl) * D + d], bsig[(k0 + kl) * D + d],
                             domain[d], domain[D + d], domain[2 * D + d] > 0.0,
                             s_bc, s_bc + SCORE_DC * SCORE_SLICE,
                             s_bc + 2 * SCORE_DC * SCORE_SLICE,
                             dl * SCORE_SLICE + kl);
            }
        }
        __syncthreads();
        if (!wave_busy) continue;
        const int co = wave * SCORE_SG * SCORE_DC;
        if (below) {
            // Coefficients sit in LDS: the plain per-dim loop has no global
            // latency to hide (s_xl / s_xr are only read for stepped dims).
            const double* q = s_bc + lc;
            score_pass_stepped(q, q + SCORE_DC * SCORE_SLICE,
                               q + 2 * SCORE_DC * SCORE_SLICE, SCORE_SLICE, dn,
                               any_stepped ? domain + 2 * D + d0 : nullptr,
                               s_x + co, s_x2 + co, s_xl + co, s_xr + co, acc);
        } else {
            // k-major (D, K): lanes of a wavefront read consecutive k.
            const int64_t o = d0 * K + k0 + lc;
            if (any_stepped)
                score_pass_stepped(c1 + o, c2 + o, c3 + o, K, dn,
                                   domain + 2 * D + d0, s_x + co, s_x2 + co,
                                   s_xl + co, s_xr + co, acc);
            else
                score_pass_cont(c1 + o, c2 + o, c3 + o, K, dn, s_x + co,
                                s_x2 + co, acc);
        }
    }
    if (!wave_busy) return;

    // A slice whose terms are all -inf (zero weights) yields (-inf, 0), never
    // NaN: exp(-inf - -inf) is not evaluated.
#pragma unroll
    for (int j = 0; j < SCORE_SG; ++j) {
        const double t = active ? acc[j] : -INFINITY;
        const double M = wave_max(t);
        const double e = (M == -INFINITY) ? 0.0 : exp(t - M);
        const double sum = wave_sum(e);
        if (lane == 0 && sw + j < S) {
            part_m[slot * S + sw + j] = M;
            part_s[slot * S + sw + j] = sum;
        }
    }
}

// Log-sum-exp of n (m, s) partials, S apart, by one wavefront.
__device__ inline double wave_lse_partials(const double* __restrict__ pm,
                                           const double* __restrict__ ps,
                                           int64_t n, int64_t S, int lane) {
    double m = -INFINITY;
    for (int64_t c = lane; c < n; c += 64) m = fmax(m, pm[c * S]);
    const double M = wave_max(m);
    if (M == -INFINITY) return -INFINITY;
    double acc = 0.0;
    for (int64_t c = lane; c < n; c += 64) acc += ps[c * S] * exp(pm[c * S] - M);
    return M + log(wave_sum(acc));
}

// Merge stage of the fused suggest, one wavefront per candidate: the above
// partials give log g, the below partials log l;
// out = [log l - log g | log g | log l] (3, S).
__global__ void k_fused_merge(const double* __restrict__ part_m,
                              const double* __restrict__ part_s,
                              int64_t n_above_slices, int64_t n_below_slices,
                              int64_t S, double* __restrict__ out) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const double log_g =
        wave_lse_partials(part_m + s, part_s + s, n_above_slices, S, lane);
    const double log_l = wave_lse_partials(part_m + n_above_slices * S + s,
                                           part_s + n_above_slices * S + s,
                                           n_below_slices, S, lane);
    if (lane == 0) {
        out[s] = log_l - log_g;
        out[S + s] = log_g;
        out[2 * S + s] = log_l;
    }
}
