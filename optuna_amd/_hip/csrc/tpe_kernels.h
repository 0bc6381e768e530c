// MI355X (gfx950/CDNA4) kernels for the TPE hot path: K1 parzen_fit,
// K2 mixture log-pdf / EI scoring, K3 truncnorm device library wrappers.
//
// Replaces the numeric core of reference optuna/samplers/_tpe/
// (parzen_estimator.py:154-221 sigma fit, probability_distributions.py:188-237
// S x K x D log-pdf + logsumexp). Design notes:
//  * The fit consumes the per-dimension sorted order maintained incrementally by
//    the host history mirror (optuna_amd/samplers/_tpe/_history.py), so no device
//    sort is needed; the fit is O(N*D) elementwise work.
//  * The log-pdf kernel uses the quadratic-form expansion (two FMA terms per
//    (sample, kernel, dim)) with the truncation-mass normalization folded into a
//    per-(kernel,dim) constant at fit time — identical math to the host path.
//  * fp64 throughout: TPE history sizes are tiny by GPU standards; correctness
//    and CPU-parity matter more than flops here, and the kernel is
//    latency/launch-bound, not compute-bound.
//  * One workgroup per candidate sample with an online block logsumexp; the
//    c1/c2/c3 coefficient arrays (K x D) are read by all 24 sample blocks and are
//    served from L2/LLC after the first pass.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "truncnorm_device.h"

// ---------------------------------------------------------------------------
// K1: Parzen fit -> per-(kernel, dim) quadratic coefficients.
//
// obs:        (N, D) observations in KDE domain (log already applied on host)
// sorted_pos: (N, D) for each dim d, sorted_pos[r*D? no: r, d] = row index of the
//             r-th smallest observation in dim d (column-wise ranks)
// out c1/c2/c3: (K, D) with K = N + 1 (prior kernel in row N)
// ---------------------------------------------------------------------------

__global__ void k_parzen_fit(const double* __restrict__ obs,
                             const int64_t* __restrict__ sorted_pos,
                             const double* __restrict__ alow,
                             const double* __restrict__ ahigh,
                             const double* __restrict__ steps,
                             const double* __restrict__ n_choices, int64_t N,
                             int64_t D, int consider_endpoints, int magic_clip,
                             double* __restrict__ c1, double* __restrict__ c2,
                             double* __restrict__ c3) {
    const int64_t d = blockIdx.y;
    const double low = alow[d];
    const double high = ahigh[d];
    const double range = high - low;
    double minsigma = 1e-12;
    if (magic_clip) {
        const double denom = fmin(100.0, (double)(N + 2));
        minsigma = range / denom;
    }
    const int64_t K = N + 1;

    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= N;
         r += (int64_t)gridDim.x * blockDim.x) {
        if (n_choices[d] > 0.0) {
            // Categorical: store the kernel's category (-1 ⇒ prior row); the
            // scoring kernel evaluates the smoothed one-hot weight directly.
            const int64_t kc =
                (r == N) ? N : sorted_pos[r * D + d];
            c1[d * K + kc] =
                (r == N) ? -1.0 : obs[sorted_pos[r * D + d] * D + d];
            c2[d * K + kc] = 0.0;
            c3[d * K + kc] = 0.0;
            continue;
        }
        double mu, sigma;
        if (r == N) {
            // Prior kernel: midpoint, full-range width.
            mu = 0.5 * (low + high);
            sigma = range;
        } else {
            const int64_t row = sorted_pos[r * D + d];
            mu = obs[row * D + d];
            const double v_prev = (r == 0) ? low : obs[sorted_pos[(r - 1) * D + d] * D + d];
            const double v_next = (r == N - 1) ? high : obs[sorted_pos[(r + 1) * D + d] * D + d];
            sigma = fmax(mu - v_prev, v_next - mu);
            if (!consider_endpoints && N >= 2) {
                if (r == 0) {
                    const double v1 = obs[sorted_pos[1 * D + d] * D + d];
                    sigma = v1 - mu;
                } else if (r == N - 1) {
                    const double vm2 = obs[sorted_pos[(N - 2) * D + d] * D + d];
                    sigma = mu - vm2;
                }
            }
            sigma = fmin(fmax(sigma, minsigma), range);
        }
        // Truncation-mass normalization; for continuous dims fold everything
        // into the quadratic expansion, for discrete (step>0) dims store
        // (mu, sigma, -logZ) — the scoring kernel integrates the step cell.
        const double mass =
            tn::log_gauss_mass((low - mu) / sigma, (high - mu) / sigma);
        const int64_t k = (r == N) ? N : sorted_pos[r * D + d];
        // k-major (D, K) layout: lane index runs along k, so the scoring
        // kernel's loads (and these writes) are coalesced.
        if (steps[d] > 0.0) {
            c1[d * K + k] = mu;
            c2[d * K + k] = sigma;
            c3[d * K + k] = -mass;
        } else {
            const double inv_var = 1.0 / (sigma * sigma);
            c1[d * K + k] = -0.5 * inv_var;
            c2[d * K + k] = mu * inv_var;
            c3[d * K + k] = -0.5 * mu * mu * inv_var - log(sigma) -
                            0.9189385332046727418 - mass;
        }
    }
}

// ---------------------------------------------------------------------------
// K2: mixture log-pdf: out[s] = logsumexp_k( logw[k] + sum_d x2*c1 + x*c2 + c3 )
// One workgroup per sample; threads stride over kernels with an online
// logsumexp, merged through LDS at the end.
// ---------------------------------------------------------------------------

// Per-(kernel, dim) mixture term: continuous dims use the precomputed
// quadratic form; discrete dims integrate the step cell [xl, xr] against the
// stored (mu, sigma) with the cached -logZ in c3.
__device__ inline double mix_term(const double* __restrict__ c1,
                                  const double* __restrict__ c2,
                                  const double* __restrict__ c3,
                                  const double* __restrict__ steps,
                                  const double* __restrict__ n_choices,
                                  double cat_base,  // prior_weight / K
                                  const double* __restrict__ xs,
                                  const double* __restrict__ x2,
                                  const double* __restrict__ xl,
                                  const double* __restrict__ xr, int64_t K,
                                  int64_t k, int64_t d) {
    const double C = n_choices[d];
    if (C > 0.0) {
        // Categorical: prior-smoothed one-hot weights in closed form —
        // row k of the (K, C) weight matrix is base everywhere plus 1 at the
        // kernel's own category, row-normalized; the prior row is uniform.
        const double v = c1[d * K + k];  // kernel's category (-1 ⇒ prior row)
        if (v < 0.0) return -log(C);
        const double hit = (xs[d] == v) ? 1.0 : 0.0;
        return log(cat_base + hit) - log(C * cat_base + 1.0);
    }
    if (steps[d] > 0.0) {
        const double mu = c1[d * K + k];
        const double sig = c2[d * K + k];
        return tn::log_gauss_mass((xl[d] - mu) / sig, (xr[d] - mu) / sig) +
               c3[d * K + k];
    }
    return x2[d] * c1[d * K + k] + xs[d] * c2[d * K + k] + c3[d * K + k];
}

__global__ void k_mix_logpdf(const double* __restrict__ x,  // (S, D)
                             const double* __restrict__ xedges,  // (S, 2D) lo|hi
                             const double* __restrict__ c1,
                             const double* __restrict__ c2,
                             const double* __restrict__ c3,
                             const double* __restrict__ logw,
                             const double* __restrict__ steps,
                             const double* __restrict__ n_choices,
                             double cat_base, int64_t K,
                             int64_t D, double* __restrict__ out) {
    extern __shared__ double lds[];  // 4 D-vectors + 2*blockDim reduction
    double* xs = lds;
    double* x2 = lds + D;
    double* xl = lds + 2 * D;
    double* xr = lds + 3 * D;
    double* red_m = lds + 4 * D;
    double* red_s = red_m + blockDim.x;

    const int64_t s = blockIdx.x;
    for (int64_t d = threadIdx.x; d < D; d += blockDim.x) {
        const double v = x[s * D + d];
        xs[d] = v;
        x2[d] = v * v;
        xl[d] = xedges[s * 2 * D + d];
        xr[d] = xedges[s * 2 * D + D + d];
    }
    __syncthreads();

    // Online logsumexp per thread. While m is still -inf a term t == -inf
    // (zero mixture weight) adds nothing; exp(t - m) would be exp(NaN).
    double m = -INFINITY, acc = 0.0;
    for (int64_t k = threadIdx.x; k < K; k += blockDim.x) {
        double t = logw[k];
        for (int64_t d = 0; d < D; ++d) {
            // k-major (D, K): lanes of a wavefront read consecutive k.
            t += mix_term(c1, c2, c3, steps, n_choices, cat_base, xs, x2, xl, xr, K, k, d);
        }
        if (t > m) {
            acc = acc * exp(m - t) + 1.0;
            m = t;
        } else if (m != -INFINITY) {
            acc += exp(t - m);
        }
    }
    red_m[threadIdx.x] = m;
    red_s[threadIdx.x] = acc;
    __syncthreads();
    // Tree merge.
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
            double m2 = red_m[threadIdx.x + stride];
            double s2 = red_s[threadIdx.x + stride];
            double m1 = red_m[threadIdx.x];
            double s1 = red_s[threadIdx.x];
            if (m2 > m1) {
                s1 = s1 * exp(m1 - m2) + s2;
                m1 = m2;
            } else if (m1 != -INFINITY) {
                s1 = s1 + s2 * exp(m2 - m1);
            }
            red_m[threadIdx.x] = m1;
            red_s[threadIdx.x] = s1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[s] = (red_m[0] == -INFINITY) ? -INFINITY : red_m[0] + log(red_s[0]);
    }
}

// Two-phase variant for large K. One block per (sample, K-chunk) pair: with
// S≈24 EI candidates a one-block-per-sample launch leaves >90% of the 256 CUs
// idle; S × n_chunks blocks fill the chip. blockIdx.x walks samples fastest so
// the XCD round-robin distributes every chunk's coefficient rows into all 8
// L2s once and the co-resident sample-blocks reuse them.
__global__ void k_mix_logpdf_partial(const double* __restrict__ x,  // (S, D)
                                     const double* __restrict__ xedges,  // (S, 2D)
                                     const double* __restrict__ c1,
                                     const double* __restrict__ c2,
                                     const double* __restrict__ c3,
                                     const double* __restrict__ logw,
                                     const double* __restrict__ steps,
                                     const double* __restrict__ n_choices,
                                     double cat_base, int64_t K,
                                     int64_t D, int64_t chunk,
                                     double* __restrict__ part_m,   // (n_chunks, S)
                                     double* __restrict__ part_s) { // (n_chunks, S)
    extern __shared__ double lds[];
    double* xs = lds;
    double* x2 = lds + D;
    double* xl = lds + 2 * D;
    double* xr = lds + 3 * D;
    double* red_m = lds + 4 * D;
    double* red_s = red_m + blockDim.x;

    const int64_t S = gridDim.x;
    const int64_t s = blockIdx.x;
    const int64_t c = blockIdx.y;
    const int64_t k_lo = c * chunk;
    const int64_t k_hi = k_lo + chunk < K ? k_lo + chunk : K;
    for (int64_t d = threadIdx.x; d < D; d += blockDim.x) {
        const double v = x[s * D + d];
        xs[d] = v;
        x2[d] = v * v;
        xl[d] = xedges[s * 2 * D + d];
        xr[d] = xedges[s * 2 * D + D + d];
    }
    __syncthreads();

    // All-continuous spaces (the common case, incl. the headline bench) take
    // a branch-free two-FMA inner loop; any discrete/categorical dim switches
    // to the general per-dim dispatch.
    bool any_special = false;
    for (int64_t d = 0; d < D; ++d)
        any_special |= (steps[d] > 0.0) || (n_choices[d] > 0.0);

    double m = -INFINITY, acc = 0.0;
    if (!any_special) {
        for (int64_t k = k_lo + threadIdx.x; k < k_hi; k += blockDim.x) {
            double t = logw[k];
            for (int64_t d = 0; d < D; ++d) {
                // k-major (D, K): lanes of a wavefront read consecutive k.
                t += x2[d] * c1[d * K + k] + xs[d] * c2[d * K + k] +
                     c3[d * K + k];
            }
            if (t > m) {
                acc = acc * exp(m - t) + 1.0;
                m = t;
            } else if (m != -INFINITY) {
                acc += exp(t - m);
            }
        }
    } else {
        for (int64_t k = k_lo + threadIdx.x; k < k_hi; k += blockDim.x) {
            double t = logw[k];
            for (int64_t d = 0; d < D; ++d) {
                t += mix_term(c1, c2, c3, steps, n_choices, cat_base, xs, x2,
                              xl, xr, K, k, d);
            }
            if (t > m) {
                acc = acc * exp(m - t) + 1.0;
                m = t;
            } else if (m != -INFINITY) {
                acc += exp(t - m);
            }
        }
    }
    red_m[threadIdx.x] = m;
    red_s[threadIdx.x] = acc;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
            double m2 = red_m[threadIdx.x + stride];
            double s2 = red_s[threadIdx.x + stride];
            double m1 = red_m[threadIdx.x];
            double s1 = red_s[threadIdx.x];
            if (m2 > m1) {
                s1 = s1 * exp(m1 - m2) + s2;
                m1 = m2;
            } else if (m1 != -INFINITY) {
                s1 = s1 + s2 * exp(m2 - m1);
            }
            red_m[threadIdx.x] = m1;
            red_s[threadIdx.x] = s1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part_m[c * S + s] = red_m[0];
        part_s[c * S + s] = red_s[0];
    }
}

__global__ void k_mix_logpdf_merge(const double* __restrict__ part_m,
                                   const double* __restrict__ part_s,
                                   int64_t n_chunks, int64_t S,
                                   double* __restrict__ out) {
    __shared__ double red_m[64];
    __shared__ double red_s[64];
    const int64_t s = blockIdx.x;
    double m = -INFINITY, acc = 0.0;
    for (int64_t c = threadIdx.x; c < n_chunks; c += blockDim.x) {
        const double m2 = part_m[c * S + s];
        const double s2 = part_s[c * S + s];
        if (m2 > m) {
            acc = acc * exp(m - m2) + s2;
            m = m2;
        } else if (m != -INFINITY) {
            acc += s2 * exp(m2 - m);
        }
    }
    red_m[threadIdx.x] = m;
    red_s[threadIdx.x] = acc;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
            double m2 = red_m[threadIdx.x + stride];
            double s2 = red_s[threadIdx.x + stride];
            double m1 = red_m[threadIdx.x];
            double s1 = red_s[threadIdx.x];
            if (m2 > m1) {
                s1 = s1 * exp(m1 - m2) + s2;
                m1 = m2;
            } else if (m1 != -INFINITY) {
                s1 = s1 + s2 * exp(m2 - m1);
            }
            red_m[threadIdx.x] = m1;
            red_s[threadIdx.x] = s1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[s] = (red_m[0] == -INFINITY) ? -INFINITY : red_m[0] + log(red_s[0]);
    }
}

// Per-dim variant for independent-mode TPE (multi-objective default): one
// workgroup per (sample, dim); out[s, d] = logsumexp_k(logw[k] + term(k, d)).
// S·D blocks (24 candidates × D dims) with a thread-strided K loop — fills the
// chip far better than the S-block joint kernel at small S, and one launch
// replaces D independent 1-dim suggest round trips.
__global__ void k_mix_logpdf_perdim(const double* __restrict__ x,  // (S, D)
                                    const double* __restrict__ xedges,  // (S, 2D)
                                    const double* __restrict__ c1,
                                    const double* __restrict__ c2,
                                    const double* __restrict__ c3,
                                    const double* __restrict__ logw,
                                    const double* __restrict__ steps,
                                    const double* __restrict__ n_choices,
                                    double cat_base, int64_t K, int64_t D,
                                    double* __restrict__ out) {  // (S, D)
    __shared__ double red_m[256];
    __shared__ double red_s[256];
    const int64_t s = blockIdx.x;
    const int64_t d = blockIdx.y;
    const double xs = x[s * D + d];
    const double x2v = xs * xs;
    const double xl = xedges[s * 2 * D + d];
    const double xr = xedges[s * 2 * D + D + d];

    double m = -INFINITY, acc = 0.0;
    // Base-offset the per-dim coefficient/descriptor pointers so mix_term's
    // d=0 indexing reads dim d's data against the scalar candidate values.
    const double* c1d = c1 + (size_t)d * K;
    const double* c2d = c2 + (size_t)d * K;
    const double* c3d = c3 + (size_t)d * K;
    for (int64_t k = threadIdx.x; k < K; k += blockDim.x) {
        double t = logw[k] + mix_term(c1d, c2d, c3d, steps + d, n_choices + d,
                                      cat_base, &xs, &x2v, &xl, &xr, K, k, 0);
        if (t > m) {
            acc = acc * exp(m - t) + 1.0;
            m = t;
        } else if (m != -INFINITY) {
            acc += exp(t - m);
        }
    }
    red_m[threadIdx.x] = m;
    red_s[threadIdx.x] = acc;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
            double m2 = red_m[threadIdx.x + stride];
            double s2 = red_s[threadIdx.x + stride];
            double m1 = red_m[threadIdx.x];
            double s1 = red_s[threadIdx.x];
            if (m2 > m1) {
                s1 = s1 * exp(m1 - m2) + s2;
                m1 = m2;
            } else if (m1 != -INFINITY) {
                s1 = s1 + s2 * exp(m2 - m1);
            }
            red_m[threadIdx.x] = m1;
            red_s[threadIdx.x] = s1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[s * D + d] =
            (red_m[0] == -INFINITY) ? -INFINITY : red_m[0] + log(red_s[0]);
    }
}

// Chunk rows so S × n_chunks blocks ≈ 2 per CU; below one chunk the original
// single-phase kernel is cheaper (no scratch round-trip).
static constexpr int64_t MIX_CHUNK = 512;

static inline int64_t mix_n_chunks(int64_t K) { return (K + MIX_CHUNK - 1) / MIX_CHUNK; }

// Order-preserving subset compaction of the per-dim sorted order, three-phase
// so the grid is (n_tiles, D) ≈ 800 blocks instead of one serial block per dim
// (a 20-block launch leaves >90% of the chip idle and was the top kernel in the
// round-4 profile at 71 µs; the tiled scan reads the same bytes chip-wide).

__global__ void k_compact_count(const int32_t* __restrict__ sorted_rows,  // (D, s_stride)
                                const int32_t* __restrict__ pos,          // (n_rows,)
                                int64_t Nv, int64_t s_stride, int64_t D,
                                int32_t* __restrict__ counts) {  // (D, n_tiles)
    const int64_t d = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ int32_t red[256];
    int32_t flag = 0;
    if (r < Nv) flag = (pos[sorted_rows[d * s_stride + r]] >= 0) ? 1 : 0;
    red[threadIdx.x] = flag;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < (unsigned)s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[d * gridDim.x + blockIdx.x] = red[0];
}

__global__ void k_compact_scan(int32_t* __restrict__ counts,  // (D, n_tiles)
                               int64_t n_tiles) {
    // Exclusive scan of ≤ a few hundred tile counts per dim; one lane per dim.
    const int64_t d = blockIdx.x;
    if (threadIdx.x == 0) {
        int32_t* c = counts + d * n_tiles;
        int32_t acc = 0;
        for (int64_t t = 0; t < n_tiles; ++t) {
            const int32_t v = c[t];
            c[t] = acc;
            acc += v;
        }
    }
}

__global__ void k_compact_write(const int32_t* __restrict__ sorted_rows,
                                const int32_t* __restrict__ pos, int64_t Nv,
                                int64_t s_stride, int64_t D,
                                const int32_t* __restrict__ offsets,  // (D, n_tiles)
                                int32_t* __restrict__ sub_rows,  // (D, Nv stride)
                                int32_t* __restrict__ sub_k) {
    const int64_t d = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ int32_t scan[256];
    int32_t row = -1, k = -1, flag = 0;
    if (r < Nv) {
        row = sorted_rows[d * s_stride + r];
        k = pos[row];
        flag = (k >= 0) ? 1 : 0;
    }
    // Hillis-Steele inclusive scan over the tile.
    scan[threadIdx.x] = flag;
    __syncthreads();
    for (int offset = 1; offset < blockDim.x; offset <<= 1) {
        int32_t v = scan[threadIdx.x];
        if (threadIdx.x >= (unsigned)offset) v += scan[threadIdx.x - offset];
        __syncthreads();
        scan[threadIdx.x] = v;
        __syncthreads();
    }
    if (flag) {
        const int32_t out_idx = offsets[d * gridDim.x + blockIdx.x] + scan[threadIdx.x] - 1;
        sub_rows[d * Nv + out_idx] = row;
        sub_k[d * Nv + out_idx] = k;
    }
}

// Row ids < n_table index the resident table; ids >= n_table index the small
// per-suggest "extras" buffer (constant-liar rows from RUNNING trials).
__device__ inline double row_val(const double* __restrict__ params,
                                 const double* __restrict__ extras,
                                 int64_t n_table, int64_t row, int64_t D,
                                 int64_t d) {
    return row < n_table ? params[row * D + d] : extras[(row - n_table) * D + d];
}

// Merge the per-dim sorted liar rows into the compacted subset on device.
// extras_sorted (D, L): per-dim ascending values; extras_sorted_idx (D, L):
// original extra index. Host-stable tie rule: extras sort AFTER equal finished
// values (they sit at the end of the combined observation array), and among
// themselves in original order.
__global__ void k_merge_extras(const int32_t* __restrict__ sub_rows,  // (D, stride)
                               const int32_t* __restrict__ sub_k,
                               int64_t stride, int64_t Na,
                               const double* __restrict__ params,
                               int64_t n_table, int64_t D,
                               const double* __restrict__ extras_sorted,
                               const int32_t* __restrict__ extras_sorted_idx,
                               int64_t L,
                               int32_t* __restrict__ out_rows,  // (D, out_stride)
                               int32_t* __restrict__ out_k,
                               int64_t out_stride) {
    const int64_t d = blockIdx.y;
    const double* ev = extras_sorted + d * L;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < Na + L;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (i < Na) {
            const double v = params[(int64_t)sub_rows[d * stride + i] * D + d];
            // #extras strictly below v (ties go after finished).
            int64_t lo = 0, hi = L;
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                if (ev[mid] < v) lo = mid + 1; else hi = mid;
            }
            out_rows[d * out_stride + i + lo] = sub_rows[d * stride + i];
            out_k[d * out_stride + i + lo] = sub_k[d * stride + i];
        } else {
            const int64_t j = i - Na;  // j-th smallest extra in this dim
            const double v = ev[j];
            // #finished with value <= v (upper bound).
            int64_t lo = 0, hi = Na;
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                const double fv =
                    params[(int64_t)sub_rows[d * stride + mid] * D + d];
                if (fv <= v) lo = mid + 1; else hi = mid;
            }
            const int32_t orig = extras_sorted_idx[d * L + j];
            out_rows[d * out_stride + lo + j] = (int32_t)n_table + orig;
            out_k[d * out_stride + lo + j] = (int32_t)Na + orig;
        }
    }
}

__global__ void k_parzen_fit_table(const double* __restrict__ params,  // (n_rows, D)
                                   const double* __restrict__ extras,  // (L, D) or null
                                   int64_t n_table,
                                   const int32_t* __restrict__ sub_rows,  // (D, stride)
                                   const int32_t* __restrict__ sub_k,
                                   int64_t stride,  // row stride of sub_* (= Nv)
                                   const double* __restrict__ alow,
                                   const double* __restrict__ ahigh,
                                   const double* __restrict__ steps,
                                   const double* __restrict__ n_choices,
                                   int64_t Na,
                                   int64_t D, int consider_endpoints,
                                   int magic_clip, double* __restrict__ c1,
                                   double* __restrict__ c2,
                                   double* __restrict__ c3) {
    const int64_t d = blockIdx.y;
    const double low = alow[d];
    const double high = ahigh[d];
    const double range = high - low;
    double minsigma = 1e-12;
    if (magic_clip) {
        minsigma = range / fmin(100.0, (double)(Na + 2));
    }
    const int32_t* rows_d = sub_rows + d * stride;
    const int32_t* ks_d = sub_k + d * stride;

    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= Na;
         r += (int64_t)gridDim.x * blockDim.x) {
        if (n_choices[d] > 0.0) {
            const int64_t kc = (r == Na) ? Na : (int64_t)ks_d[r];
            c1[d * (Na + 1) + kc] =
                (r == Na) ? -1.0
                          : row_val(params, extras, n_table, rows_d[r], D, d);
            c2[d * (Na + 1) + kc] = 0.0;
            c3[d * (Na + 1) + kc] = 0.0;
            continue;
        }
        double mu, sigma;
        int64_t k;
        if (r == Na) {
            mu = 0.5 * (low + high);
            sigma = range;
            k = Na;
        } else {
            mu = row_val(params, extras, n_table, rows_d[r], D, d);
            const double v_prev =
                (r == 0) ? low
                         : row_val(params, extras, n_table, rows_d[r - 1], D, d);
            const double v_next =
                (r == Na - 1)
                    ? high
                    : row_val(params, extras, n_table, rows_d[r + 1], D, d);
            sigma = fmax(mu - v_prev, v_next - mu);
            if (!consider_endpoints && Na >= 2) {
                if (r == 0) {
                    sigma = row_val(params, extras, n_table, rows_d[1], D, d) - mu;
                } else if (r == Na - 1) {
                    sigma =
                        mu - row_val(params, extras, n_table, rows_d[Na - 2], D, d);
                }
            }
            sigma = fmin(fmax(sigma, minsigma), range);
            k = ks_d[r];
        }
        const double mass =
            tn::log_gauss_mass((low - mu) / sigma, (high - mu) / sigma);
        if (steps[d] > 0.0) {
            c1[d * (Na + 1) + k] = mu;
            c2[d * (Na + 1) + k] = sigma;
            c3[d * (Na + 1) + k] = -mass;
        } else {
            const double inv_var = 1.0 / (sigma * sigma);
            c1[d * (Na + 1) + k] = -0.5 * inv_var;
            c2[d * (Na + 1) + k] = mu * inv_var;
            c3[d * (Na + 1) + k] = -0.5 * mu * mu * inv_var - log(sigma) -
                            0.9189385332046727418 - mass;
        }
    }
}

// Incremental insert into the device-resident per-dim sorted index: one block
// per dim; rows are inserted sequentially. The kernel reads each new row's value
// from the resident table and finds its slot itself with an upper-bound binary
// search through params[col[j]*D+d] (ties go after equal values and rows are
// inserted in row order — the host rule side="right"). The tail shift is a
// block-parallel backward memmove in descending chunks: within a chunk every
// thread reads before any thread writes; a later (lower) chunk only writes
// cells the earlier chunk has already read. Row ids are kernel arguments, so
// nothing is uploaded and the workspace is not touched; stream order alone
// sequences it against later scoring kernels.
__global__ void k_sorted_insert_by_value(int32_t* __restrict__ cols,  // (D, cap)
                                         int64_t cap, int64_t n_sorted,
                                         const double* __restrict__ params,
                                         int64_t D, int64_t first_row,
                                         int64_t n_new) {
    const int64_t d = blockIdx.x;
    int32_t* col = cols + d * cap;
    int64_t n = n_sorted;
    for (int64_t i = 0; i < n_new; ++i) {
        const int64_t row = first_row + i;
        const double v = params[row * D + d];
        // Block-uniform search: every lane walks the same probes.
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (params[(int64_t)col[mid] * D + d] <= v) lo = mid + 1; else hi = mid;
        }
        const int64_t p = lo;
        __syncthreads();  // all probes done before the shift overwrites cells
        for (int64_t top = n; top > p; top -= blockDim.x) {
            const int64_t j = top - 1 - threadIdx.x;
            int32_t t = 0;
            if (j >= p) t = col[j];
            __syncthreads();
            if (j >= p) col[j + 1] = t;
            __syncthreads();
        }
        if (threadIdx.x == 0) col[p] = (int32_t)row;
        __syncthreads();
        ++n;
    }
}
