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
#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <stdexcept>
#include <vector>
#include <algorithm>
#include <cstring>

#include "truncnorm_device.h"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                          \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            throw std::runtime_error(std::string("HIP error: ") +                \
                                     hipGetErrorString(_e) + " at " __FILE__ ":" + \
                                     std::to_string(__LINE__));                  \
        }                                                                        \
    } while (0)

// ---------------------------------------------------------------------------
// Elementwise truncnorm wrappers (golden-tested against scipy on GPU boxes).
// ---------------------------------------------------------------------------

__global__ void k_log_gauss_mass(const double* a, const double* b, double* out,
                                 int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tn::log_gauss_mass(a[i], b[i]);
}

__global__ void k_ppf(const double* q, const double* a, const double* b,
                      double* out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tn::trunc_ppf(q[i], a[i], b[i]);
}

__global__ void k_logpdf(const double* x, const double* a, const double* b,
                         const double* loc, const double* scale, double* out,
                         int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tn::trunc_logpdf(x[i], a[i], b[i], loc[i], scale[i]);
}

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

// d_scratch must hold 2 * mix_n_chunks(K) * S doubles (may alias nothing else).
static void launch_mix_logpdf(hipStream_t st, const double* d_x,
                              const double* d_xedges, const double* d_c1,
                              const double* d_c2, const double* d_c3,
                              const double* d_logw, const double* d_steps,
                              const double* d_nchoices, double cat_base,
                              int64_t K, int64_t D, int64_t S, double* d_out,
                              double* d_scratch) {
    const int block = 256;
    const size_t shmem = (4 * (size_t)D + 2 * block) * sizeof(double);
    const int64_t n_chunks = mix_n_chunks(K);
    if (n_chunks <= 1) {
        hipLaunchKernelGGL(k_mix_logpdf, dim3((unsigned)S), dim3(block), shmem, st,
                           d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                           d_nchoices, cat_base, K, D, d_out);
        return;
    }
    double* d_part_m = d_scratch;
    double* d_part_s = d_scratch + (size_t)n_chunks * S;
    hipLaunchKernelGGL(k_mix_logpdf_partial, dim3((unsigned)S, (unsigned)n_chunks),
                       dim3(block), shmem, st, d_x, d_xedges, d_c1, d_c2, d_c3,
                       d_logw, d_steps, d_nchoices, cat_base, K, D, MIX_CHUNK,
                       d_part_m, d_part_s);
    hipLaunchKernelGGL(k_mix_logpdf_merge, dim3((unsigned)S), dim3(64), 0, st,
                       d_part_m, d_part_s, n_chunks, S, d_out);
}

// ---------------------------------------------------------------------------
// Host-side workspace: grown lazily, reused across calls (no per-suggest
// hipMalloc). One workspace per process; calls are serialized by the GIL.
// ---------------------------------------------------------------------------

struct Workspace {
    double* buf = nullptr;
    size_t capacity = 0;
    hipStream_t stream = nullptr;
    // Pinned host staging: pageable hipMemcpyAsync silently degrades to a slow
    // synchronous staged copy; all H2D goes through this buffer instead.
    char* pinned = nullptr;
    size_t pinned_capacity = 0;
    size_t pinned_cursor = 0;

    double* ensure(size_t n_doubles) {
        if (n_doubles > capacity) {
            if (buf) (void)hipFree(buf);
            capacity = n_doubles + n_doubles / 2;
            HIP_CHECK(hipMalloc(&buf, capacity * sizeof(double)));
        }
        return buf;
    }
    void ensure_pinned(size_t n_bytes) {
        if (n_bytes > pinned_capacity) {
            if (pinned) (void)hipHostFree(pinned);
            pinned_capacity = n_bytes + n_bytes / 2;
            HIP_CHECK(hipHostMalloc(&pinned, pinned_capacity));
        }
    }
    // Event guard: an upload batch that ends without a stream sync (append's
    // fast path) records this event; the next begin_uploads waits on it before
    // reusing the staging buffer.
    hipEvent_t uploads_done = nullptr;
    bool uploads_pending = false;

    void end_uploads_async(hipStream_t st) {
        if (!uploads_done)
            HIP_CHECK(hipEventCreateWithFlags(&uploads_done, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(uploads_done, st));
        uploads_pending = true;
    }
    void begin_uploads() {
        if (uploads_pending) {
            HIP_CHECK(hipEventSynchronize(uploads_done));
            uploads_pending = false;
        }
        pinned_cursor = 0;
    }
    // Reserve a fresh pinned slice (the caller fills it and issues the DMA).
    char* stage(size_t bytes, hipStream_t st) {
        size_t aligned = (bytes + 255) & ~size_t(255);
        if (pinned_cursor + aligned > pinned_capacity) {
            // Grow: must drain in-flight DMAs that read the old buffer first.
            HIP_CHECK(hipStreamSynchronize(st));
            ensure_pinned(pinned_cursor + aligned);
            pinned_cursor = 0;
        }
        char* slot = pinned + pinned_cursor;
        pinned_cursor += aligned;
        return slot;
    }
    // memcpy into a fresh pinned slice, then a true-async DMA on the stream.
    void h2d(void* dst, const void* src, size_t bytes, hipStream_t st) {
        if (bytes == 0) return;
        char* slot = stage(bytes, st);
        memcpy(slot, src, bytes);
        HIP_CHECK(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, st));
    }
    hipStream_t get_stream() {
        if (!stream) HIP_CHECK(hipStreamCreate(&stream));
        return stream;
    }
};

static Workspace g_ws;

static bool g_available_checked = false;
static bool g_available = false;

static bool device_available() {
    if (!g_available_checked) {
        int n = 0;
        g_available = (hipGetDeviceCount(&n) == hipSuccess) && n > 0;
        g_available_checked = true;
    }
    return g_available;
}

template <typename T>
static const T* data_of(const py::array_t<T, py::array::c_style | py::array::forcecast>& a) {
    return a.data();
}

// ---------------------------------------------------------------------------
// Python-facing entry points
// ---------------------------------------------------------------------------

using arr_f64 = py::array_t<double, py::array::c_style | py::array::forcecast>;
using arr_i64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;

static py::array_t<double> elementwise3(const arr_f64& a, const arr_f64& b,
                                        const arr_f64& c, int which) {
    const int64_t n = a.size();
    if (b.size() != n || (which == 1 && c.size() != n))
        throw std::runtime_error("shape mismatch");
    py::array_t<double> out(n);
    hipStream_t st = g_ws.get_stream();
    double* d = g_ws.ensure(4 * (size_t)n);
    double *da = d, *db = d + n, *dc = d + 2 * n, *dout = d + 3 * n;
    g_ws.begin_uploads();
    g_ws.h2d(da, a.data(), n * 8, st);
    g_ws.h2d(db, b.data(), n * 8, st);
    if (which == 1) g_ws.h2d(dc, c.data(), n * 8, st);
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
    if (which == 0)
        hipLaunchKernelGGL(k_log_gauss_mass, dim3(grid), dim3(block), 0, st, da, db,
                           dout, n);
    else
        hipLaunchKernelGGL(k_ppf, dim3(grid), dim3(block), 0, st, dc, da, db, dout,
                           n);  // c = q
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), dout, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return out;
}

py::array_t<double> log_gauss_mass(const arr_f64& a, const arr_f64& b) {
    return elementwise3(a, b, a, 0);
}

py::array_t<double> truncnorm_ppf(const arr_f64& q, const arr_f64& a,
                                  const arr_f64& b) {
    return elementwise3(a, b, q, 1);
}

py::array_t<double> truncnorm_logpdf(const arr_f64& x, const arr_f64& a,
                                     const arr_f64& b, const arr_f64& loc,
                                     const arr_f64& scale) {
    const int64_t n = x.size();
    if (a.size() != n || b.size() != n || loc.size() != n || scale.size() != n)
        throw std::runtime_error("shape mismatch");
    py::array_t<double> out(n);
    hipStream_t st = g_ws.get_stream();
    double* d = g_ws.ensure(6 * (size_t)n);
    double *dx = d, *da = d + n, *db = d + 2 * n, *dl = d + 3 * n,
           *ds = d + 4 * n, *dout = d + 5 * n;
    g_ws.begin_uploads();
    g_ws.h2d(dx, x.data(), n * 8, st);
    g_ws.h2d(da, a.data(), n * 8, st);
    g_ws.h2d(db, b.data(), n * 8, st);
    g_ws.h2d(dl, loc.data(), n * 8, st);
    g_ws.h2d(ds, scale.data(), n * 8, st);
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
    hipLaunchKernelGGL(k_logpdf, dim3(grid), dim3(block), 0, st, dx, da, db, dl,
                       ds, dout, n);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), dout, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return out;
}

// Full fused path: fit one KDE on device and evaluate candidates.
//   obs        (N, D)   observations, KDE domain
//   sorted_pos (N, D)   column-wise ranks (row index of r-th smallest per dim)
//   logw       (N+1,)   log mixture weights (prior last)
//   alow/ahigh (D,)     KDE-domain truncation bounds
//   x          (S, D)   candidates, KDE domain
// returns (S,) log mixture pdf.
py::array_t<double> kde_logpdf(const arr_f64& obs, const arr_i64& sorted_pos,
                               const arr_f64& logw, const arr_f64& alow,
                               const arr_f64& ahigh, const arr_f64& steps,
                               const arr_f64& n_choices, double prior_weight,
                               const arr_f64& x, const arr_f64& xedges,
                               bool consider_endpoints, bool magic_clip) {
    if (obs.ndim() != 2 || x.ndim() != 2) throw std::runtime_error("obs/x must be 2-D");
    const int64_t N = obs.shape(0);
    const int64_t D = obs.shape(1);
    const int64_t S = x.shape(0);
    const int64_t K = N + 1;
    if (x.shape(1) != D || (int64_t)logw.size() != K ||
        (int64_t)alow.size() != D || (int64_t)ahigh.size() != D ||
        (int64_t)steps.size() != D || (int64_t)xedges.size() != 2 * S * D ||
        sorted_pos.shape(0) != N || (N > 0 && sorted_pos.shape(1) != D))
        throw std::runtime_error("shape mismatch in kde_logpdf");

    py::array_t<double> out(S);
    hipStream_t st = g_ws.get_stream();

    const size_t n_obs = (size_t)N * D;
    const size_t n_c = (size_t)K * D;
    // layout: obs | c1 | c2 | c3 | logw | alow | ahigh | steps | x | xedges
    //         | out | lse scratch | sorted(i64 as f64 slots)
    const size_t n_scratch = 2 * (size_t)mix_n_chunks(K) * S;
    size_t total = n_obs + 3 * n_c + K + 4 * D + 3 * (size_t)S * D + S + n_scratch +
                   n_obs + 16;
    double* base = g_ws.ensure(total);
    double* d_obs = base;
    double* d_c1 = d_obs + n_obs;
    double* d_c2 = d_c1 + n_c;
    double* d_c3 = d_c2 + n_c;
    double* d_logw = d_c3 + n_c;
    double* d_alow = d_logw + K;
    double* d_ahigh = d_alow + D;
    double* d_steps = d_ahigh + D;
    double* d_nchoices = d_steps + D;
    double* d_x = d_nchoices + D;
    double* d_xedges = d_x + (size_t)S * D;
    double* d_out = d_xedges + 2 * (size_t)S * D;
    double* d_scratch = d_out + S;
    int64_t* d_sorted = reinterpret_cast<int64_t*>(d_scratch + n_scratch);

    g_ws.begin_uploads();
    if (N > 0) {
        g_ws.h2d(d_obs, obs.data(), n_obs * 8, st);
        g_ws.h2d(d_sorted, sorted_pos.data(), n_obs * 8, st);
    }
    g_ws.h2d(d_logw, logw.data(), K * 8, st);
    g_ws.h2d(d_alow, alow.data(), D * 8, st);
    g_ws.h2d(d_ahigh, ahigh.data(), D * 8, st);
    g_ws.h2d(d_steps, steps.data(), D * 8, st);
    g_ws.h2d(d_nchoices, n_choices.data(), D * 8, st);
    g_ws.h2d(d_x, x.data(), (size_t)S * D * 8, st);
    g_ws.h2d(d_xedges, xedges.data(), 2 * (size_t)S * D * 8, st);

    const double cat_base = prior_weight / (double)K;
    {
        const int block = 256;
        const int gx = (int)((K + block - 1) / block);
        hipLaunchKernelGGL(k_parzen_fit, dim3(gx, (unsigned)D), dim3(block), 0, st,
                           d_obs, d_sorted, d_alow, d_ahigh, d_steps, d_nchoices,
                           N, D, consider_endpoints ? 1 : 0, magic_clip ? 1 : 0,
                           d_c1, d_c2, d_c3);
    }
    launch_mix_logpdf(st, d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                      d_nchoices, cat_base, K, D, S, d_out, d_scratch);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out, S * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}

// ---------------------------------------------------------------------------
// K6: non-domination rank (NSGA-II / MO-TPE). The O(N²M) dominance test is the
// heavy part: pack it into a bitmatrix (bit j of row i ⇔ j dominates i), then
// peel Pareto fronts with two tiny kernels per round against a shrinking
// "unranked" bitmask. The value matrix (N×M fp64 ≤ a few MB) stays L2-resident
// across the whole N²M sweep.
// ---------------------------------------------------------------------------

__global__ void k_dominance_words(const double* __restrict__ vals,  // (N, M)
                                  int64_t N, int64_t M, int64_t W,
                                  uint64_t* __restrict__ words) {  // (N, W)
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = idx / W;
    const int64_t w = idx % W;
    if (i >= N) return;
    const double* vi = vals + i * M;
    uint64_t bits = 0;
    const int64_t j0 = w * 64;
    const int64_t j1 = j0 + 64 < N ? j0 + 64 : N;
    for (int64_t j = j0; j < j1; ++j) {
        if (j == i) continue;
        const double* vj = vals + j * M;
        bool leq = true, lt = false;
        for (int64_t m = 0; m < M; ++m) {
            const double a = vj[m], b = vi[m];
            if (a > b) { leq = false; break; }
            if (a < b) lt = true;
        }
        if (leq && lt) bits |= (uint64_t)1 << (j - j0);
    }
    words[i * W + w] = bits;
}

__global__ void k_front_detect(const uint64_t* __restrict__ words, int64_t N,
                               int64_t W, const uint64_t* __restrict__ mask,
                               int32_t* __restrict__ front) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (!((mask[i / 64] >> (i % 64)) & 1)) { front[i] = 0; return; }
    const uint64_t* row = words + i * W;
    uint64_t any = 0;
    for (int64_t w = 0; w < W; ++w) any |= row[w] & mask[w];
    front[i] = any == 0 ? 1 : 0;
}

__global__ void k_front_apply(const int32_t* __restrict__ front, int64_t N,
                              int32_t rank, int64_t* __restrict__ ranks,
                              uint64_t* __restrict__ mask,
                              int32_t* __restrict__ n_front) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || !front[i]) return;
    ranks[i] = rank;
    atomicAnd(
        reinterpret_cast<unsigned long long*>(mask + i / 64),
        ~((unsigned long long)1 << (i % 64)));
    atomicAdd(n_front, 1);
}

// Rank the (pre-filtered, all-finite) rows; early-stop once n_below rows are
// exactly ranked. Unranked rows return -1 (host lumps them into a bottom
// rank), mirroring _calculate_nondomination_rank in study/_multi_objective.py.
py::array_t<int64_t> nondomination_rank(const arr_f64& vals, int64_t n_below) {
    if (vals.ndim() != 2) throw std::runtime_error("vals must be 2-D");
    const int64_t N = vals.shape(0);
    const int64_t M = vals.shape(1);
    const int64_t W = (N + 63) / 64;
    py::array_t<int64_t> out(N);
    if (N == 0) return out;
    hipStream_t st = g_ws.get_stream();

    const size_t f64_vals = (size_t)N * M;
    // u64 words (N*W) + mask (W) + ranks (N i64) + front (N i32) + counter.
    const size_t u64_slots = (size_t)N * W + W + N + (N + 1) / 2 + 2;
    double* base = g_ws.ensure(f64_vals + u64_slots + 16);
    double* d_vals = base;
    uint64_t* d_words = reinterpret_cast<uint64_t*>(d_vals + f64_vals);
    uint64_t* d_mask = d_words + (size_t)N * W;
    int64_t* d_ranks = reinterpret_cast<int64_t*>(d_mask + W);
    int32_t* d_front = reinterpret_cast<int32_t*>(d_ranks + N);
    int32_t* d_nfront = d_front + N;

    g_ws.begin_uploads();
    g_ws.h2d(d_vals, vals.data(), f64_vals * 8, st);
    std::vector<uint64_t> mask_init(W, 0);
    for (int64_t i = 0; i < N; ++i) mask_init[i / 64] |= (uint64_t)1 << (i % 64);
    g_ws.h2d(d_mask, mask_init.data(), W * 8, st);
    std::vector<int64_t> ranks_init(N, -1);
    g_ws.h2d(d_ranks, ranks_init.data(), N * 8, st);

    {
        const int64_t total = N * W;
        const int block = 256;
        hipLaunchKernelGGL(k_dominance_words,
                           dim3((unsigned)((total + block - 1) / block)),
                           dim3(block), 0, st, d_vals, N, M, W, d_words);
    }
    const int block = 256;
    const unsigned gridN = (unsigned)((N + block - 1) / block);
    int64_t n_assigned = 0;
    int32_t rank = -1;
    int32_t h_nfront = 0;
    while (n_assigned < n_below) {
        ++rank;
        HIP_CHECK(hipMemsetAsync(d_nfront, 0, 4, st));
        hipLaunchKernelGGL(k_front_detect, dim3(gridN), dim3(block), 0, st,
                           d_words, N, W, d_mask, d_front);
        hipLaunchKernelGGL(k_front_apply, dim3(gridN), dim3(block), 0, st,
                           d_front, N, rank, d_ranks, d_mask, d_nfront);
        HIP_CHECK(hipMemcpyAsync(&h_nfront, d_nfront, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (h_nfront == 0) break;
        n_assigned += h_nfront;
    }
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_ranks, (size_t)N * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}

bool available() { return device_available(); }

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------
// Device-resident TPE history (one per (study, search-space) on the Python side).
//
// The parameter table lives in HBM and grows append-only, mirroring the host
// history (_history.py); a suggest uploads only the per-dim global sorted order
// (i32), the subset position map, mixture weights and candidates — the big fp64
// observation matrix never crosses PCIe again after its append.
//
// score() pipeline (all on one stream):
//   1. k_compact_{count,scan,write}: per dim, order-preserving compaction of
//      the global sorted order down to the "above" subset (tiled 3-phase scan).
//   2. k_parzen_fit_table: K1 fit reading mus from the resident table.
//   3. k_mix_logpdf: K2 scoring.
// ---------------------------------------------------------------------------

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
// per dim; rows are inserted sequentially (positions are final indices, i.e.
// already offset by earlier inserts of the same batch). The tail shift is a
// block-parallel backward memmove in descending chunks: within a chunk every
// thread reads before any thread writes; a later (lower) chunk only writes
// cells the earlier chunk has already read.
__global__ void k_sorted_insert(int32_t* __restrict__ cols,  // (D, cap)
                                int64_t cap, int64_t n_sorted,
                                const int32_t* __restrict__ pos,   // (n_new, D)
                                const int32_t* __restrict__ rows,  // (n_new, D)
                                int64_t n_new, int64_t D) {
    const int64_t d = blockIdx.x;
    int32_t* col = cols + d * cap;
    int64_t n = n_sorted;
    for (int64_t i = 0; i < n_new; ++i) {
        const int64_t p = pos[i * D + d];
        for (int64_t hi = n; hi > p; hi -= blockDim.x) {
            const int64_t j = hi - 1 - threadIdx.x;
            int32_t v = 0;
            if (j >= p) v = col[j];
            __syncthreads();
            if (j >= p) col[j + 1] = v;
            __syncthreads();
        }
        if (threadIdx.x == 0) col[p] = rows[i * D + d];
        __syncthreads();
        ++n;
    }
}

// Same insert without staged positions: the kernel reads each new row's value
// from the resident table and finds its slot itself with an upper-bound binary
// search through params[col[j]*D+d] (ties go after equal values and rows are
// inserted in row order — the host rule side="right"). Row ids are kernel
// arguments, so nothing is uploaded and the workspace is not touched; stream
// order alone sequences it against later scoring kernels.
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

using arr_i32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

class TpeDeviceHistory {
  public:
    explicit TpeDeviceHistory(int64_t D) : D_(D) {}

    ~TpeDeviceHistory() {
        if (params_) (void)hipFree(params_);
        if (sorted_) (void)hipFree(sorted_);
        if (domain_) (void)hipFree(domain_);
        if (coef_) (void)hipFree(coef_);
    }

    int64_t n_rows() const { return n_; }

    void append(const arr_f64& block) {
        if (block.ndim() != 2 || block.shape(1) != D_)
            throw std::runtime_error("append: block must be (n_new, D)");
        const int64_t n_new = block.shape(0);
        if (n_new == 0) return;
        prep_.valid = false;
        hipStream_t st = g_ws.get_stream();
        if (n_ + n_new > capacity_) {
            int64_t new_cap = std::max<int64_t>(1024, (n_ + n_new) * 2);
            double* new_params = nullptr;
            HIP_CHECK(hipMalloc(&new_params, (size_t)new_cap * D_ * sizeof(double)));
            if (params_) {
                HIP_CHECK(hipMemcpyAsync(new_params, params_,
                                         (size_t)n_ * D_ * sizeof(double),
                                         hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
                HIP_CHECK(hipFree(params_));
            }
            params_ = new_params;
            capacity_ = new_cap;
        }
        g_ws.begin_uploads();
        g_ws.h2d(params_ + (size_t)n_ * D_, block.data(),
                 (size_t)n_new * D_ * sizeof(double), st);
        // No stream sync: the table write is stream-ordered before any later
        // kernel on this stream; staging reuse is guarded by the upload event.
        g_ws.end_uploads_async(st);
        n_ += n_new;
    }

    py::array_t<double> score(const std::vector<arr_i32>& sorted_cols,  // D × (Nv,)
                              const arr_i32& pos,  // (n_rows,)
                              int64_t n_above,
                              const arr_f64& logw,  // (n_above + L + 1,)
                              const arr_f64& alow, const arr_f64& ahigh,
                              const arr_f64& steps,   // (D,) 0 = continuous
                              const arr_f64& n_choices,  // (D,) 0 = numerical
                              double prior_weight,
                              const arr_f64& x,       // (S, D) KDE domain
                              const arr_f64& xedges,  // (S, 2D) cell lo|hi
                              bool consider_endpoints, bool magic_clip,
                              const arr_f64& extras_raw,         // (L, D) or empty
                              const arr_f64& extras_sorted,      // (D, L)
                              const arr_i32& extras_sorted_idx,  // (D, L)
                              bool per_dim)
    {
        const bool resident_sorted = sorted_cols.empty() && sorted_valid_;
        const int64_t Nv =
            resident_sorted ? n_sorted_
                            : (sorted_cols.empty() ? 0
                                                   : (int64_t)sorted_cols[0].size());
        const int64_t S = x.shape(0);
        const int64_t Na = n_above;
        const int64_t L = extras_raw.ndim() == 2 ? extras_raw.shape(0) : 0;
        const int64_t Nk = Na + L;  // mixture kernels excluding the prior
        const int64_t K = Nk + 1;
        if ((int64_t)pos.size() != n_ || x.shape(1) != D_ ||
            (!resident_sorted && Nv > 0 && (int64_t)sorted_cols.size() != D_) ||
            (int64_t)logw.size() != K)
            throw std::runtime_error("score: shape mismatch");
        if (L > 0 && ((int64_t)extras_sorted.size() != L * D_ ||
                      (int64_t)extras_sorted_idx.size() != L * D_ ||
                      extras_raw.shape(1) != D_))
            throw std::runtime_error("score: extras shape mismatch");
        for (const auto& col : sorted_cols)
            if ((int64_t)col.size() != Nv)
                throw std::runtime_error("score: ragged sorted columns");

        hipStream_t st = g_ws.get_stream();
        const size_t n_c = (size_t)K * D_;
        const int64_t n_tiles = (Nv + 255) / 256;
        const int64_t mstride = Nv + L;  // merged subset stride
        // f64 slots: c1|c2|c3|logw|alow|ahigh|steps|x|xedges|out|lse|extras + i32.
        const size_t n_scratch = 2 * (size_t)mix_n_chunks(K) * S;
        const size_t n_extras_f64 = 2 * (size_t)L * D_;  // raw + per-dim sorted
        const size_t out_elems = (size_t)S * (per_dim ? D_ : 1);
        size_t f64_total = 3 * n_c + K + 4 * D_ + 3 * (size_t)S * D_ + out_elems +
                           n_scratch + n_extras_f64;
        size_t i32_doubles = ((size_t)Nv * D_ /*sorted*/ + n_ /*pos*/ +
                              2 * (size_t)Nv * D_ /*sub*/ +
                              2 * (size_t)mstride * D_ /*merged*/ +
                              (size_t)L * D_ /*extra idx*/ +
                              (size_t)n_tiles * D_ /*tile counts*/) /
                                 2 +
                             8;
        double* base = g_ws.ensure(f64_total + i32_doubles + 16);
        double* d_c1 = base;
        double* d_c2 = d_c1 + n_c;
        double* d_c3 = d_c2 + n_c;
        double* d_logw = d_c3 + n_c;
        double* d_alow = d_logw + K;
        double* d_ahigh = d_alow + D_;
        double* d_steps = d_ahigh + D_;
        double* d_nchoices = d_steps + D_;
        double* d_x = d_nchoices + D_;
        double* d_xedges = d_x + (size_t)S * D_;
        double* d_out = d_xedges + 2 * (size_t)S * D_;
        double* d_scratch = d_out + out_elems;
        double* d_extras_raw = d_scratch + n_scratch;
        double* d_extras_sorted = d_extras_raw + (size_t)L * D_;
        int32_t* d_sorted =
            reinterpret_cast<int32_t*>(d_extras_sorted + (size_t)L * D_);
        int32_t* d_pos = d_sorted + (size_t)Nv * D_;
        int32_t* d_sub_rows = d_pos + n_;
        int32_t* d_sub_k = d_sub_rows + (size_t)Nv * D_;
        int32_t* d_merged_rows = d_sub_k + (size_t)Nv * D_;
        int32_t* d_merged_k = d_merged_rows + (size_t)mstride * D_;
        int32_t* d_extra_idx = d_merged_k + (size_t)mstride * D_;
        int32_t* d_counts = d_extra_idx + (size_t)L * D_;

        g_ws.begin_uploads();
        if (!resident_sorted)
            for (int64_t d = 0; d < (int64_t)sorted_cols.size() && Nv > 0; ++d)
                g_ws.h2d(d_sorted + d * Nv, sorted_cols[d].data(), (size_t)Nv * 4,
                         st);
        if (n_ > 0) g_ws.h2d(d_pos, pos.data(), (size_t)n_ * 4, st);
        g_ws.h2d(d_logw, logw.data(), K * 8, st);
        g_ws.h2d(d_alow, alow.data(), D_ * 8, st);
        g_ws.h2d(d_ahigh, ahigh.data(), D_ * 8, st);
        g_ws.h2d(d_steps, steps.data(), D_ * 8, st);
        g_ws.h2d(d_nchoices, n_choices.data(), D_ * 8, st);
        g_ws.h2d(d_x, x.data(), (size_t)S * D_ * 8, st);
        g_ws.h2d(d_xedges, xedges.data(), 2 * (size_t)S * D_ * 8, st);
        if (L > 0) {
            g_ws.h2d(d_extras_raw, extras_raw.data(), (size_t)L * D_ * 8, st);
            g_ws.h2d(d_extras_sorted, extras_sorted.data(), (size_t)L * D_ * 8, st);
            g_ws.h2d(d_extra_idx, extras_sorted_idx.data(), (size_t)L * D_ * 4, st);
        }

        if (Na > 0) {
            const int32_t* s_src = resident_sorted ? sorted_ : d_sorted;
            const int64_t s_stride = resident_sorted ? sorted_cap_ : Nv;
            const dim3 grid((unsigned)n_tiles, (unsigned)D_);
            hipLaunchKernelGGL(k_compact_count, grid, dim3(256), 0, st, s_src,
                               d_pos, Nv, s_stride, D_, d_counts);
            hipLaunchKernelGGL(k_compact_scan, dim3((unsigned)D_), dim3(64), 0, st,
                               d_counts, n_tiles);
            hipLaunchKernelGGL(k_compact_write, grid, dim3(256), 0, st, s_src,
                               d_pos, Nv, s_stride, D_, d_counts, d_sub_rows,
                               d_sub_k);
        }
        const int32_t* fit_rows = d_sub_rows;
        const int32_t* fit_k = d_sub_k;
        int64_t fit_stride = Nv;
        if (L > 0) {
            const int block = 256;
            const int gx = (int)((Na + L + block - 1) / block);
            hipLaunchKernelGGL(k_merge_extras, dim3(gx, (unsigned)D_), dim3(block),
                               0, st, d_sub_rows, d_sub_k, Nv, Na, params_, n_,
                               D_, d_extras_sorted, d_extra_idx, L,
                               d_merged_rows, d_merged_k, mstride);
            fit_rows = d_merged_rows;
            fit_k = d_merged_k;
            fit_stride = mstride;
        }
        {
            const int block = 256;
            const int gx = (int)((K + block - 1) / block);
            hipLaunchKernelGGL(k_parzen_fit_table, dim3(gx, (unsigned)D_),
                               dim3(block), 0, st, params_,
                               L > 0 ? d_extras_raw : nullptr, n_, fit_rows,
                               fit_k, fit_stride, d_alow, d_ahigh, d_steps,
                               d_nchoices, Nk, D_, consider_endpoints ? 1 : 0,
                               magic_clip ? 1 : 0, d_c1, d_c2, d_c3);
        }
        const double cat_base = prior_weight / (double)K;
        if (per_dim) {
            hipLaunchKernelGGL(k_mix_logpdf_perdim,
                               dim3((unsigned)S, (unsigned)D_), dim3(256), 0, st,
                               d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                               d_nchoices, cat_base, K, D_, d_out);
            py::array_t<double> out({S, D_});
            HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out,
                                     (size_t)S * D_ * 8, hipMemcpyDeviceToHost,
                                     st));
            HIP_CHECK(hipStreamSynchronize(st));
            HIP_CHECK(hipGetLastError());
            return out;
        }
        launch_mix_logpdf(st, d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                          d_nchoices, cat_base, K, D_, S, d_out, d_scratch);
        py::array_t<double> out(S);
        HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out, S * 8,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return out;
    }

    // ---- device-resident per-dim sorted index ------------------------------

    void upload_sorted(const std::vector<arr_i32>& cols) {
        const int64_t Nv = cols.empty() ? 0 : (int64_t)cols[0].size();
        if ((int64_t)cols.size() != D_ && Nv > 0)
            throw std::runtime_error("upload_sorted: wrong number of columns");
        prep_.valid = false;
        hipStream_t st = g_ws.get_stream();
        ensure_sorted_capacity(Nv, st);
        g_ws.begin_uploads();
        for (int64_t d = 0; d < (int64_t)cols.size() && Nv > 0; ++d)
            g_ws.h2d(sorted_ + d * sorted_cap_, cols[d].data(), (size_t)Nv * 4, st);
        g_ws.end_uploads_async(st);
        n_sorted_ = Nv;
        sorted_valid_ = true;
    }

    void insert_sorted(const arr_i32& pos, const arr_i32& rows) {
        // pos (n_new, D): FINAL indices (already offset by earlier rows of the
        // same batch); rows (n_new, D): per-dim row ids in per-dim value order.
        if (!sorted_valid_) throw std::runtime_error("insert_sorted before upload");
        const int64_t n_new = pos.ndim() == 2 ? pos.shape(0) : 0;
        if (n_new == 0) return;
        prep_.valid = false;
        if (pos.shape(1) != D_ || rows.shape(0) != n_new || rows.shape(1) != D_)
            throw std::runtime_error("insert_sorted: shape mismatch");
        hipStream_t st = g_ws.get_stream();
        ensure_sorted_capacity(n_sorted_ + n_new, st);
        // small staging via the workspace device buffer tail is unsafe (ensure
        // may realloc); use a dedicated tiny upload through pinned staging.
        const size_t bytes = (size_t)n_new * D_ * 4;
        double* scratch = g_ws.ensure((2 * bytes) / 8 + 8);
        int32_t* d_pos = reinterpret_cast<int32_t*>(scratch);
        int32_t* d_rows = d_pos + (size_t)n_new * D_;
        g_ws.begin_uploads();
        g_ws.h2d(d_pos, pos.data(), bytes, st);
        g_ws.h2d(d_rows, rows.data(), bytes, st);
        hipLaunchKernelGGL(k_sorted_insert, dim3((unsigned)D_), dim3(256), 0, st,
                           sorted_, sorted_cap_, n_sorted_, d_pos, d_rows, n_new,
                           D_);
        // The insert kernel reads workspace memory that a later ensure() may
        // reallocate; drain before returning (≈ the kernel's own few µs).
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        n_sorted_ += n_new;
    }

    int64_t n_sorted() const { return sorted_valid_ ? n_sorted_ : -1; }

    // Insert table rows [first_row, first_row + n_new) into the resident index
    // by value (see k_sorted_insert_by_value). No upload, no sync.
    void insert_sorted_by_value(int64_t first_row, int64_t n_new) {
        if (!sorted_valid_)
            throw std::runtime_error("insert_sorted_by_value before upload");
        if (n_new <= 0) return;
        prep_.valid = false;
        if (first_row < 0 || first_row + n_new > n_)
            throw std::runtime_error("insert_sorted_by_value: rows not in table");
        hipStream_t st = g_ws.get_stream();
        ensure_sorted_capacity(n_sorted_ + n_new, st);
        hipLaunchKernelGGL(k_sorted_insert_by_value, dim3((unsigned)D_),
                           dim3(256), 0, st, sorted_, sorted_cap_, n_sorted_,
                           params_, D_, first_row, n_new);
        HIP_CHECK(hipGetLastError());
        n_sorted_ += n_new;
    }

    // Debug/test accessor: the resident sorted index as a (D, n_sorted) array.
    py::array_t<int32_t> sorted_index() {
        if (!sorted_valid_) throw std::runtime_error("sorted_index before upload");
        py::array_t<int32_t> out({D_, n_sorted_});
        hipStream_t st = g_ws.get_stream();
        if (n_sorted_ > 0)
            HIP_CHECK(hipMemcpy2DAsync(out.mutable_data(), (size_t)n_sorted_ * 4,
                                       sorted_, (size_t)sorted_cap_ * 4,
                                       (size_t)n_sorted_ * 4, (size_t)D_,
                                       hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return out;
    }

    // Per-space constants (KDE-domain bounds, steps, category counts): they
    // never change for a (study, search-space), so they are uploaded once.
    void set_domain(const arr_f64& alow, const arr_f64& ahigh,
                    const arr_f64& steps, const arr_f64& n_choices) {
        if ((int64_t)alow.size() != D_ || (int64_t)ahigh.size() != D_ ||
            (int64_t)steps.size() != D_ || (int64_t)n_choices.size() != D_)
            throw std::runtime_error("set_domain: shape mismatch");
        prep_.valid = false;
        std::vector<double> host(4 * (size_t)D_);
        std::copy(alow.data(), alow.data() + D_, host.begin());
        std::copy(ahigh.data(), ahigh.data() + D_, host.begin() + D_);
        std::copy(steps.data(), steps.data() + D_, host.begin() + 2 * D_);
        std::copy(n_choices.data(), n_choices.data() + D_, host.begin() + 3 * D_);
        hipStream_t st = g_ws.get_stream();
        if (!domain_) HIP_CHECK(hipMalloc(&domain_, host.size() * sizeof(double)));
        // Earlier launches may still read the old values.
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemcpy(domain_, host.data(), host.size() * sizeof(double),
                            hipMemcpyHostToDevice));
        has_steps_ = false;
        has_categorical_ = false;
        for (int64_t d = 0; d < D_; ++d) {
            has_steps_ |= steps.data()[d] > 0.0;
            has_categorical_ |= n_choices.data()[d] > 0.0;
        }
    }

    // Fused suggest, in two native calls that share one stream:
    //   fused_prepare  uploads the exclusion list (and custom log-weights) and
    //                  launches the above-set fit into this history's own
    //                  coefficient buffer; returns without synchronising.
    //   fused_score    one packed upload (candidates + below estimator),
    //                  k_fused_score, k_fused_merge (which writes the result
    //                  into pinned host memory: no download). It reuses
    //                  the prepared fit when that is still valid for its
    //                  arguments and otherwise runs the fit itself first.
    //   excl     sorted table rows NOT in the above set (below + invalid rows)
    //   n_above  size of the above set (= resident index rows not in excl)
    //   x/xedges candidates (KDE domain); xedges only read for stepped dims
    //   bmu/bsig/bw  below estimator kernels (Kb, D) and mixture weights (Kb,)
    //   logw     custom above log-weights (n_above + 1,), or empty for the
    //            default ramp, which the device writes itself from
    //            (w_num, w_start, w_step, log_total)
    void fused_prepare(const arr_i32& excl, int64_t n_above, const arr_f64& logw,
                       int64_t w_num, double w_start, double w_step,
                       double log_total, double prior_weight,
                       bool consider_endpoints, bool magic_clip) {
        check_fit_args("fused_prepare", excl, n_above, logw);
        g_ws.begin_uploads();
        launch_fit(excl, n_above, logw, w_num, w_start, w_step, log_total,
                   prior_weight, consider_endpoints, magic_clip,
                   /*guard_staging=*/true);
    }

    // Returns (S,) log l - log g, or with return_parts the test/debug form
    // ((3, S) [ei | log g | log l], (K,) above logw).
    py::object fused_score(const arr_i32& excl, int64_t n_above,
                                    const arr_f64& x, const arr_f64& xedges,
                                    const arr_f64& bmu, const arr_f64& bsig,
                                    const arr_f64& bw, const arr_f64& logw,
                                    int64_t w_num, double w_start,
                                    double w_step, double log_total,
                                    double prior_weight,
                                    bool consider_endpoints, bool magic_clip,
                                    bool return_parts) {
        check_fit_args("fused_score", excl, n_above, logw);
        if (x.ndim() != 2 || x.shape(1) != D_ || bmu.ndim() != 2 ||
            bmu.shape(1) != D_ || bsig.ndim() != 2 || bsig.shape(1) != D_)
            throw std::runtime_error("fused_score: shape mismatch");
        const int64_t S = x.shape(0);
        const int64_t Kb = bmu.shape(0);
        const int64_t K = n_above + 1;
        if (S < 1 || Kb < 1 || Kb > FUSED_MAX_BELOW || bsig.shape(0) != Kb ||
            (int64_t)bw.size() != Kb ||
            (has_steps_ && (int64_t)xedges.size() != 2 * S * D_))
            throw std::runtime_error("fused_score: shape mismatch");

        hipStream_t st = g_ws.get_stream();
        g_ws.begin_uploads();
        if (!prepared_matches(excl, n_above, logw, w_num, w_start, w_step,
                              log_total, prior_weight, consider_endpoints,
                              magic_clip))
            launch_fit(excl, n_above, logw, w_num, w_start, w_step, log_total,
                       prior_weight, consider_endpoints, magic_clip,
                       /*guard_staging=*/false);

        // Packed region (one pinned slice, one DMA, same layout on device):
        //   x | bmu | bsig | bw | [xedges]
        const size_t n_x = (size_t)S * D_;
        const size_t n_b = (size_t)Kb * D_;
        const size_t up_doubles = n_x + 2 * n_b + Kb + (has_steps_ ? 2 * n_x : 0);
        const int64_t n_as = (K + SCORE_SLICE - 1) / SCORE_SLICE;
        // Below slices: as many kernels as give each of the block's threads
        // at most one (kernel, dim) coefficient to build per pass over dims.
        const int64_t pass_dims = std::min<int64_t>(D_, SCORE_DC);
        const int below_slice = (int)std::max<int64_t>(
            1, std::min<int64_t>(SCORE_SLICE, SCORE_SLICE * SCORE_WAVES / pass_dims));
        const int64_t n_bs = (Kb + below_slice - 1) / below_slice;
        const size_t n_part = (size_t)(n_as + n_bs) * S;
        double* base = g_ws.ensure(up_doubles + 2 * n_part + 16);
        double* d_x = base;
        double* d_bmu = d_x + n_x;
        double* d_bsig = d_bmu + n_b;
        double* d_bw = d_bsig + n_b;
        double* d_xedges = d_bw + Kb;
        double* d_part_m = base + up_doubles;
        double* d_part_s = d_part_m + n_part;
        {
            double* h = reinterpret_cast<double*>(g_ws.stage(up_doubles * 8, st));
            double* p = h;
            memcpy(p, x.data(), n_x * 8); p += n_x;
            memcpy(p, bmu.data(), n_b * 8); p += n_b;
            memcpy(p, bsig.data(), n_b * 8); p += n_b;
            memcpy(p, bw.data(), (size_t)Kb * 8); p += Kb;
            if (has_steps_) memcpy(p, xedges.data(), 2 * n_x * 8);
            HIP_CHECK(hipMemcpyAsync(base, h, up_doubles * 8,
                                     hipMemcpyHostToDevice, st));
        }

        const size_t n_c = (size_t)K * D_;
        const double* d_logw = coef_ + 3 * n_c;
        const int64_t n_groups = (S + SCORE_CAND - 1) / SCORE_CAND;
        hipLaunchKernelGGL(k_fused_score,
                           dim3((unsigned)(n_as + n_bs), (unsigned)n_groups),
                           dim3(SCORE_SLICE * SCORE_WAVES), 0, st, d_x, d_xedges,
                           coef_, coef_ + n_c, coef_ + 2 * n_c, d_logw, K, n_as,
                           d_bmu, d_bsig, d_bw, Kb, below_slice, domain_,
                           has_steps_ ? 1 : 0,
                           D_, S, d_part_m, d_part_s);
        // The merge writes its (3, S) result straight into a pinned host slot
        // (kernels can address hipHostMalloc memory), which saves the
        // download's own dispatch on the serial chain. The slot belongs to
        // this upload batch and is read after the stream sync below, so it is
        // not reused before the kernel has finished.
        const double* h_out =
            reinterpret_cast<const double*>(g_ws.stage(3 * (size_t)S * 8, st));
        hipLaunchKernelGGL(k_fused_merge, dim3((unsigned)S), dim3(64), 0, st,
                           d_part_m, d_part_s, n_as, n_bs, S,
                           const_cast<double*>(h_out));
        if (return_parts) {
            py::array_t<double> parts({(int64_t)3, S});
            py::array_t<double> lw(K);
            HIP_CHECK(hipMemcpyAsync(lw.mutable_data(), d_logw, (size_t)K * 8,
                                     hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            HIP_CHECK(hipGetLastError());
            memcpy(parts.mutable_data(), h_out, 3 * (size_t)S * 8);
            return py::make_tuple(parts, lw);
        }
        py::array_t<double> out(S);
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        memcpy(out.mutable_data(), h_out, (size_t)S * 8);
        return out;
    }

  private:
    // What the coefficients in coef_ were fitted from. They stay usable only
    // while the table, the index, the domain and every fit argument are the
    // same; every mutator of those clears `valid`.
    struct PreparedFit {
        bool valid = false;
        int64_t n = 0, n_sorted = 0, Na = 0, w_num = 0;
        double w_start = 0.0, w_step = 0.0, log_total = 0.0, prior_weight = 0.0;
        bool consider_endpoints = false, magic_clip = false;
        std::vector<int32_t> excl;
        std::vector<double> logw;  // custom log-weights, empty for the ramp
    };

    void check_fit_args(const char* who, const arr_i32& excl, int64_t Na,
                        const arr_f64& logw) const {
        const std::string w(who);
        if (!sorted_valid_) throw std::runtime_error(w + " before upload_sorted");
        if (!domain_) throw std::runtime_error(w + " before set_domain");
        if (has_categorical_)
            throw std::runtime_error(w + ": categorical dims unsupported");
        const int64_t E = excl.size();
        const int64_t Nv = n_sorted_;
        if (E > FUSED_MAX_EXCL || Na < 0 || Na > Nv || Na + E < Nv ||
            (logw.size() > 0 && (int64_t)logw.size() != Na + 1))
            throw std::runtime_error(w + ": shape mismatch");
        // Strictly ascending in-table rows: keeps row - lower_bound(excl, row)
        // inside [0, n_above) for every member row.
        const int32_t* ex = excl.data();
        for (int64_t e = 0; e < E; ++e)
            if (ex[e] < 0 || ex[e] >= n_ || (e > 0 && ex[e] <= ex[e - 1]))
                throw std::runtime_error(w + ": excl must be sorted table rows");
    }

    // Bit-wise comparisons throughout: equal arguments give the same fit.
    bool prepared_matches(const arr_i32& excl, int64_t Na, const arr_f64& logw,
                          int64_t w_num, double w_start, double w_step,
                          double log_total, double prior_weight,
                          bool consider_endpoints, bool magic_clip) const {
        const PreparedFit& p = prep_;
        const double a[4] = {w_start, w_step, log_total, prior_weight};
        const double b[4] = {p.w_start, p.w_step, p.log_total, p.prior_weight};
        return p.valid && p.n == n_ && p.n_sorted == n_sorted_ && p.Na == Na &&
               p.w_num == w_num && memcmp(a, b, sizeof(a)) == 0 &&
               p.consider_endpoints == consider_endpoints &&
               p.magic_clip == magic_clip &&
               p.excl.size() == (size_t)excl.size() &&
               (p.excl.empty() ||
                memcmp(p.excl.data(), excl.data(), p.excl.size() * 4) == 0) &&
               p.logw.size() == (size_t)logw.size() &&
               (p.logw.empty() ||
                memcmp(p.logw.data(), logw.data(), p.logw.size() * 8) == 0);
    }

    // Upload [logw] | excl into coef_ and launch the fit behind it. The caller
    // has opened the upload batch; with guard_staging the batch is closed with
    // the event guard right behind the DMA (the caller does not synchronise).
    // coef_ = c1 | c2 | c3 (D, K each, k-major) | logw (K) | excl (i32, padded).
    void launch_fit(const arr_i32& excl, int64_t Na, const arr_f64& logw,
                    int64_t w_num, double w_start, double w_step,
                    double log_total, double prior_weight,
                    bool consider_endpoints, bool magic_clip, bool guard_staging) {
        prep_.valid = false;
        hipStream_t st = g_ws.get_stream();
        const int64_t E = excl.size();
        const int64_t K = Na + 1;
        const int64_t Nv = n_sorted_;
        const bool custom_w = logw.size() > 0;
        const size_t n_c = (size_t)K * D_;
        const size_t n_excl = ((size_t)E + 1) / 2;
        const size_t need = 3 * n_c + K + n_excl;
        if (need > coef_cap_) {
            // hipFree waits for the launches that still read the old buffer.
            if (coef_) HIP_CHECK(hipFree(coef_));
            coef_ = nullptr;
            coef_cap_ = 0;
            const size_t new_cap = std::max<size_t>(4096, need * 2);
            HIP_CHECK(hipMalloc(&coef_, new_cap * sizeof(double)));
            coef_cap_ = new_cap;
        }
        double* d_logw = coef_ + 3 * n_c;
        int32_t* d_excl = reinterpret_cast<int32_t*>(d_logw + K);
        const size_t up_doubles = (custom_w ? (size_t)K : 0) + n_excl;
        if (up_doubles) {
            double* h = reinterpret_cast<double*>(g_ws.stage(up_doubles * 8, st));
            double* p = h;
            if (custom_w) { memcpy(p, logw.data(), (size_t)K * 8); p += K; }
            if (n_excl) {
                p[n_excl - 1] = 0.0;  // defined padding for odd E
                memcpy(p, excl.data(), (size_t)E * 4);
            }
            HIP_CHECK(hipMemcpyAsync(custom_w ? d_logw : d_logw + K, h,
                                     up_doubles * 8, hipMemcpyHostToDevice, st));
            if (guard_staging) g_ws.end_uploads_async(st);
        }
        const int64_t n_tiles = std::max<int64_t>(1, (Nv + FUSED_TILE - 1) / FUSED_TILE);
        hipLaunchKernelGGL(k_fused_fit, dim3((unsigned)n_tiles, (unsigned)D_),
                           dim3(FUSED_TILE), 0, st, params_, sorted_, sorted_cap_,
                           Nv, d_excl, (int)E, domain_, Na, D_,
                           consider_endpoints ? 1 : 0, magic_clip ? 1 : 0, coef_,
                           coef_ + n_c, coef_ + 2 * n_c,
                           custom_w ? nullptr : d_logw, w_num, w_start, w_step,
                           log_total, prior_weight);
        HIP_CHECK(hipGetLastError());
        prep_.n = n_;
        prep_.n_sorted = n_sorted_;
        prep_.Na = Na;
        prep_.w_num = w_num;
        prep_.w_start = w_start;
        prep_.w_step = w_step;
        prep_.log_total = log_total;
        prep_.prior_weight = prior_weight;
        prep_.consider_endpoints = consider_endpoints;
        prep_.magic_clip = magic_clip;
        prep_.excl.assign(excl.data(), excl.data() + E);
        prep_.logw.assign(logw.data(), logw.data() + logw.size());
        prep_.valid = true;
    }

    void ensure_sorted_capacity(int64_t need, hipStream_t st) {
        if (need <= sorted_cap_) return;
        const int64_t new_cap = std::max<int64_t>(1024, need * 2);
        int32_t* grown = nullptr;
        HIP_CHECK(hipMalloc(&grown, (size_t)new_cap * D_ * 4));
        if (sorted_ && n_sorted_ > 0) {
            HIP_CHECK(hipMemcpy2DAsync(grown, (size_t)new_cap * 4, sorted_,
                                       (size_t)sorted_cap_ * 4,
                                       (size_t)n_sorted_ * 4, (size_t)D_,
                                       hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        if (sorted_) (void)hipFree(sorted_);
        sorted_ = grown;
        sorted_cap_ = new_cap;
    }

    int64_t D_;
    int64_t n_ = 0;
    int64_t capacity_ = 0;
    double* params_ = nullptr;
    int32_t* sorted_ = nullptr;
    int64_t n_sorted_ = 0;
    int64_t sorted_cap_ = 0;
    bool sorted_valid_ = false;
    double* domain_ = nullptr;  // alow | ahigh | steps | n_choices
    bool has_steps_ = false;
    bool has_categorical_ = false;
    // Above-set coefficients of the fused suggest: owned by the history (the
    // shared workspace is laid over by every other entry point), grown
    // geometrically.
    double* coef_ = nullptr;
    size_t coef_cap_ = 0;
    PreparedFit prep_;
};


// ---------------------------------------------------------------------------
// K6a: exact 3-D hypervolume (minimization, ref-dominated region).
//
// Points sorted ascending by x. HV = sum_t slab_x(t) * A_t where A_t is the
// area in (y, z) dominated by the first t+1 points. A_t is evaluated by a
// y-ascending sweep that maintains the running min z over the points of the
// prefix — one THREAD per prefix t, with the y-sorted stream staged through
// LDS tiles so the O(N^2) scan reads each point once per 256-thread block.
// ---------------------------------------------------------------------------
__global__ void k_hv3d(const double* __restrict__ xs,   // (N) ascending
                       const double* __restrict__ yv,   // (N) y ascending
                       const double* __restrict__ zv,   // (N) z in y-order
                       const int32_t* __restrict__ rk,  // (N) x-rank in y-order
                       int64_t N, double ref_x, double ref_y, double ref_z,
                       double* __restrict__ out) {  // (N) per-prefix volumes
    __shared__ double t_y[256];
    __shared__ double t_z[256];
    __shared__ int32_t t_r[256];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double slab =
        (t < N) ? ((t + 1 < N ? xs[t + 1] : ref_x) - xs[t]) : 0.0;
    double minz = ref_z;
    double area = 0.0;
    for (int64_t base = 0; base < N; base += 256) {
        const int64_t m = min((int64_t)256, N - base);
        __syncthreads();
        if (threadIdx.x < m) {
            t_y[threadIdx.x] = yv[base + threadIdx.x];
            t_z[threadIdx.x] = zv[base + threadIdx.x];
            t_r[threadIdx.x] = rk[base + threadIdx.x];
        }
        // the y-interval right edge needs the NEXT point's y
        __syncthreads();
        for (int64_t q = 0; q < m; ++q) {
            if (t_r[q] <= t) minz = fmin(minz, t_z[q]);
            const int64_t g = base + q;
            const double y_next = (g + 1 < N) ? (q + 1 < m ? t_y[q + 1] : yv[g + 1]) : ref_y;
            area += (y_next - t_y[q]) * (ref_z - minz);
        }
    }
    if (t < N) out[t] = slab * area;
}

// 3-D hypervolume of x-lexsorted points (all strictly inside ref).
double hv3d(const arr_f64& pts, double ref_x, double ref_y, double ref_z) {
    if (pts.ndim() != 2 || pts.shape(1) != 3)
        throw std::runtime_error("hv3d: pts must be (N, 3)");
    const int64_t N = pts.shape(0);
    if (N == 0) return 0.0;
    // Host prep: y-order view (N log N — negligible next to the N^2 sweep).
    std::vector<double> xs(N), yv(N), zv(N);
    std::vector<int32_t> rk(N);
    std::vector<int64_t> order(N);
    const double* P = pts.data();
    for (int64_t i = 0; i < N; ++i) {
        xs[i] = P[i * 3];
        order[i] = i;
    }
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return P[a * 3 + 1] < P[b * 3 + 1];
    });
    for (int64_t i = 0; i < N; ++i) {
        yv[i] = P[order[i] * 3 + 1];
        zv[i] = P[order[i] * 3 + 2];
        rk[i] = (int32_t)order[i];
    }
    hipStream_t st = g_ws.get_stream();
    const size_t need = 4 * (size_t)N + (size_t)(N + 1) / 2 + 8;
    double* base = g_ws.ensure(need);
    double* d_xs = base;
    double* d_yv = d_xs + N;
    double* d_zv = d_yv + N;
    double* d_out = d_zv + N;
    int32_t* d_rk = reinterpret_cast<int32_t*>(d_out + N);
    g_ws.begin_uploads();
    g_ws.h2d(d_xs, xs.data(), N * 8, st);
    g_ws.h2d(d_yv, yv.data(), N * 8, st);
    g_ws.h2d(d_zv, zv.data(), N * 8, st);
    g_ws.h2d(d_rk, rk.data(), N * 4, st);
    const int64_t blocks = (N + 255) / 256;
    hipLaunchKernelGGL(k_hv3d, dim3((unsigned)blocks), dim3(256), 0, st, d_xs,
                       d_yv, d_zv, d_rk, N, ref_x, ref_y, ref_z, d_out);
    std::vector<double> host_out(N);
    HIP_CHECK(hipMemcpyAsync(host_out.data(), d_out, N * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double hv = 0.0;
    for (double v : host_out) hv += v;
    return hv;
}

// ---------------------------------------------------------------------------
// K6b: batched greedy-HSSP contributions, 3 objectives. One workgroup per
// candidate. Key identity: the limited set {max(c, s) : s in S} keeps S's
// sorted orders under the per-coordinate clamp (max(c, .) is monotone), so
// the kernel reads GLOBALLY pre-sorted views of S — x-sorted xs, and the
// y-sorted (y, z, x-rank) triple — clamps them by the candidate, and runs the
// per-prefix staircase sweep directly. No per-candidate sort, no size cap;
// clamp ties produce zero-width slabs the sweep ignores.
// contribution(c | S) = incl(c) - HV3D(limited).
// ---------------------------------------------------------------------------
__global__ void k_hssp3d_contrib(const double* __restrict__ cand,  // (n, 3)
                                 const double* __restrict__ sx,    // (k) x asc
                                 const double* __restrict__ sxz,   // (k) z in x-order
                                 const double* __restrict__ sy,    // (k) y asc
                                 const double* __restrict__ syz,   // (k) z in y-order
                                 const int32_t* __restrict__ syr,  // (k) x-rank in y-order
                                 int64_t n, int64_t k, double ref_x,
                                 double ref_y, double ref_z,
                                 double* __restrict__ out) {  // (n)
    __shared__ double red[128];

    const int64_t c = blockIdx.x;
    const double cx = cand[c * 3], cy = cand[c * 3 + 1], cz = cand[c * 3 + 2];
    const double incl = (ref_x - cx) * (ref_y - cy) * (ref_z - cz);
    if (k == 0) {
        if (threadIdx.x == 0) out[c] = incl;
        return;
    }
    // Lanes stride over prefixes t; the y-stream is staged through LDS tiles
    // shared by the whole block.
    double total = 0.0;
    for (int64_t t = threadIdx.x; t < k; t += blockDim.x) {
        const double lx_t = fmax(cx, sx[t]);
        const double lx_next = (t + 1 < k) ? fmax(cx, sx[t + 1]) : ref_x;
        const double slab = lx_next - lx_t;
        if (slab <= 0.0) continue;
        double minz = ref_z;
        double area = 0.0;
        for (int64_t q = 0; q < k; ++q) {
            if (syr[q] <= t) minz = fmin(minz, fmax(cz, syz[q]));
            const double ly_q = fmax(cy, sy[q]);
            const double ly_next = (q + 1 < k) ? fmax(cy, sy[q + 1]) : ref_y;
            area += (ly_next - ly_q) * (ref_z - minz);
        }
        total += slab * area;
    }
    red[threadIdx.x] = total;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = incl - red[0];
}

// Per-candidate greedy-HSSP contributions against the current selected set,
// passed as pre-sorted views (x-sorted xs/z, y-sorted y/z/x-rank).
py::array_t<double> hssp3d_contrib(const arr_f64& cand, const arr_f64& sx,
                                   const arr_f64& sxz, const arr_f64& sy,
                                   const arr_f64& syz, const arr_i32& syr,
                                   double ref_x, double ref_y, double ref_z) {
    if (cand.ndim() != 2 || cand.shape(1) != 3)
        throw std::runtime_error("hssp3d_contrib: cand must be (n, 3)");
    const int64_t n = cand.shape(0);
    const int64_t k = sx.size();
    if ((int64_t)sy.size() != k || (int64_t)syz.size() != k ||
        (int64_t)syr.size() != k || (int64_t)sxz.size() != k)
        throw std::runtime_error("hssp3d_contrib: ragged sorted views");
    py::array_t<double> out(n);
    if (n == 0) return out;
    hipStream_t st = g_ws.get_stream();
    double* base = g_ws.ensure((size_t)n * 3 + 4 * (size_t)k + n + (size_t)(k + 1) / 2 + 8);
    double* d_cand = base;
    double* d_sx = d_cand + (size_t)n * 3;
    double* d_sxz = d_sx + k;
    double* d_sy = d_sxz + k;
    double* d_syz = d_sy + k;
    double* d_out = d_syz + k;
    int32_t* d_syr = reinterpret_cast<int32_t*>(d_out + n);
    g_ws.begin_uploads();
    g_ws.h2d(d_cand, cand.data(), (size_t)n * 3 * 8, st);
    if (k > 0) {
        g_ws.h2d(d_sx, sx.data(), k * 8, st);
        g_ws.h2d(d_sxz, sxz.data(), k * 8, st);
        g_ws.h2d(d_sy, sy.data(), k * 8, st);
        g_ws.h2d(d_syz, syz.data(), k * 8, st);
        g_ws.h2d(d_syr, syr.data(), k * 4, st);
    }
    hipLaunchKernelGGL(k_hssp3d_contrib, dim3((unsigned)n), dim3(128), 0, st,
                       d_cand, d_sx, d_sxz, d_sy, d_syz, d_syr, n, k, ref_x,
                       ref_y, ref_z, d_out);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}


// Masked argmax over the contributions, one block; the winner is marked taken
// so the next round's kernel skips it — only the 8-byte index crosses the bus
// per greedy round.
__global__ void k_hssp3d_argmax(const double* __restrict__ vals, int64_t n,
                                uint8_t* __restrict__ taken,
                                int64_t* __restrict__ out_idx) {
    __shared__ double red_v[256];
    __shared__ int64_t red_i[256];
    double best = -INFINITY;
    int64_t bi = -1;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        if (!taken[i] && vals[i] > best) {
            best = vals[i];
            bi = i;
        }
    }
    red_v[threadIdx.x] = best;
    red_i[threadIdx.x] = bi;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) {
            if (red_v[threadIdx.x + stride] > red_v[threadIdx.x] ||
                (red_v[threadIdx.x + stride] == red_v[threadIdx.x] &&
                 red_i[threadIdx.x + stride] >= 0 &&
                 (red_i[threadIdx.x] < 0 ||
                  red_i[threadIdx.x + stride] < red_i[threadIdx.x]))) {
                red_v[threadIdx.x] = red_v[threadIdx.x + stride];
                red_i[threadIdx.x] = red_i[threadIdx.x + stride];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_idx[0] = red_i[0];
        if (red_i[0] >= 0) taken[red_i[0]] = 1;
    }
}

// Device-side selected-set insertion: after the argmax picked winner w, put
// cand[w] into the x-sorted (x, z) and y-sorted (y, z, x-rank) views and bump
// the device k counter. One block; the O(k) shifts are a few hundred
// elements. Keeping the views on device lets the whole greedy run as a
// launch train with a single host sync at the end.
__global__ void k_hssp3d_insert(const double* __restrict__ cand,
                                const int64_t* __restrict__ idx,
                                double* __restrict__ sx, double* __restrict__ sxz,
                                double* __restrict__ sy, double* __restrict__ syz,
                                int32_t* __restrict__ syr,
                                int64_t* __restrict__ k_ptr,
                                int64_t* __restrict__ chosen,
                                int64_t* __restrict__ round_ptr) {
    // One block. The O(k) tail shifts run in parallel: every thread stages
    // its strided elements in registers, barriers, then writes them one slot
    // to the right (read-before-write is global across the block).
    __shared__ int64_t s_w, s_px, s_py, s_k;
    if (threadIdx.x == 0) {
        const int64_t w = idx[0];
        s_w = w;
        chosen[round_ptr[0]] = w;
        round_ptr[0] += 1;
        const int64_t k = k_ptr[0];
        s_k = k;
        if (w >= 0) {
            const double x = cand[w * 3], y = cand[w * 3 + 1];
            int64_t px = 0;
            while (px < k && sx[px] <= x) ++px;
            int64_t py = 0;
            while (py < k && sy[py] <= y) ++py;
            s_px = px;
            s_py = py;
            k_ptr[0] = k + 1;
        }
    }
    __syncthreads();
    const int64_t w = s_w;
    if (w < 0) return;
    const int64_t k = s_k, px = s_px, py = s_py;
    const double x = cand[w * 3], y = cand[w * 3 + 1], z = cand[w * 3 + 2];

    constexpr int MAXLOC = 32;  // supports k up to 32 * blockDim
    double rx_v[MAXLOC], rz_v[MAXLOC], ry_v[MAXLOC], ryz_v[MAXLOC];
    int32_t rr_v[MAXLOC];
    int nx = 0, ny = 0;
    for (int64_t i = px + threadIdx.x; i < k; i += blockDim.x) {
        rx_v[nx] = sx[i];
        rz_v[nx] = sxz[i];
        ++nx;
    }
    for (int64_t i = py + threadIdx.x; i < k; i += blockDim.x) {
        ry_v[ny] = sy[i];
        ryz_v[ny] = syz[i];
        // pre-bump the x-ranks shifting right of the x insertion point
        int32_t r = syr[i];
        rr_v[ny] = (r >= (int32_t)px) ? r + 1 : r;
        ++ny;
    }
    // ranks BEFORE py also need the bump; handle them in-place (no shift)
    __syncthreads();
    for (int64_t i = threadIdx.x; i < py; i += blockDim.x) {
        int32_t r = syr[i];
        if (r >= (int32_t)px) syr[i] = r + 1;
    }
    {
        int j = 0;
        for (int64_t i = px + threadIdx.x; i < k; i += blockDim.x, ++j) {
            sx[i + 1] = rx_v[j];
            sxz[i + 1] = rz_v[j];
        }
        j = 0;
        for (int64_t i = py + threadIdx.x; i < k; i += blockDim.x, ++j) {
            sy[i + 1] = ry_v[j];
            syz[i + 1] = ryz_v[j];
            syr[i + 1] = rr_v[j];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sx[px] = x;
        sxz[px] = z;
        sy[py] = y;
        syz[py] = z;
        syr[py] = (int32_t)px;
    }
}

// Contribution kernel variant reading k from device memory (launch-train mode).
__global__ void k_hssp3d_contrib_dk(const double* __restrict__ cand,
                                    const double* __restrict__ sx,
                                    const double* __restrict__ sxz,
                                    const double* __restrict__ sy,
                                    const double* __restrict__ syz,
                                    const int32_t* __restrict__ syr,
                                    int64_t n, const int64_t* __restrict__ k_ptr,
                                    double ref_x, double ref_y, double ref_z,
                                    double* __restrict__ out) {
    __shared__ double red[128];
    const int64_t k = k_ptr[0];
    const int64_t c = blockIdx.x;
    const double cx = cand[c * 3], cy = cand[c * 3 + 1], cz = cand[c * 3 + 2];
    const double incl = (ref_x - cx) * (ref_y - cy) * (ref_z - cz);
    if (k == 0) {
        if (threadIdx.x == 0) out[c] = incl;
        return;
    }
    double total = 0.0;
    for (int64_t t = threadIdx.x; t < k; t += blockDim.x) {
        const double lx_t = fmax(cx, sx[t]);
        const double lx_next = (t + 1 < k) ? fmax(cx, sx[t + 1]) : ref_x;
        const double slab = lx_next - lx_t;
        if (slab <= 0.0) continue;
        double minz = ref_z;
        double area = 0.0;
        for (int64_t q = 0; q < k; ++q) {
            if (syr[q] <= t) minz = fmin(minz, fmax(cz, syz[q]));
            const double ly_q = fmax(cy, sy[q]);
            const double ly_next = (q + 1 < k) ? fmax(cy, sy[q + 1]) : ref_y;
            area += (ly_next - ly_q) * (ref_z - minz);
        }
        total += slab * area;
    }
    red[threadIdx.x] = total;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = incl - red[0];
}

// Greedy-HSSP driver state: candidates and the taken-mask stay resident; each
// round re-uploads only the (small, growing) sorted selected-set views and
// pulls back ONE index.
class Hssp3dSession {
  public:
    Hssp3dSession(const arr_f64& cand, double rx, double ry, double rz)
        : n_(cand.shape(0)), rx_(rx), ry_(ry), rz_(rz) {
        if (cand.ndim() != 2 || cand.shape(1) != 3)
            throw std::runtime_error("Hssp3dSession: cand must be (n, 3)");
        hipStream_t st = g_ws.get_stream();
        HIP_CHECK(hipMalloc(&d_cand_, (size_t)n_ * 3 * 8));
        HIP_CHECK(hipMalloc(&d_out_, (size_t)n_ * 8 + 8 + n_));
        d_idx_ = reinterpret_cast<int64_t*>(d_out_ + n_);
        d_taken_ = reinterpret_cast<uint8_t*>(d_idx_ + 1);
        HIP_CHECK(hipMemcpyAsync(d_cand_, cand.data(), (size_t)n_ * 3 * 8,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_taken_, 0, n_, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    ~Hssp3dSession() {
        if (d_cand_) (void)hipFree(d_cand_);
        if (d_out_) (void)hipFree(d_out_);
    }
    Hssp3dSession(const Hssp3dSession&) = delete;
    Hssp3dSession& operator=(const Hssp3dSession&) = delete;

    // Launch-train greedy: subset_size rounds of contrib→argmax→insert
    // enqueued back-to-back with device-resident views, ONE host sync.
    py::array_t<int64_t> run(int64_t subset_size) {
        if (subset_size > n_) subset_size = n_;
        hipStream_t st = g_ws.get_stream();
        const size_t kcap = (size_t)subset_size + 1;
        double* base = g_ws.ensure(4 * kcap + kcap / 2 + subset_size + 6);
        double* d_sx = base;
        double* d_sxz = d_sx + kcap;
        double* d_sy = d_sxz + kcap;
        double* d_syz = d_sy + kcap;
        int32_t* d_syr = reinterpret_cast<int32_t*>(d_syz + kcap);
        int64_t* d_k = reinterpret_cast<int64_t*>(d_syr + ((kcap + 1) & ~size_t(1)));
        int64_t* d_round = d_k + 1;
        int64_t* d_chosen = d_round + 1;
        HIP_CHECK(hipMemsetAsync(d_k, 0, 16, st));
        // Every round launches the same three kernels with identical args
        // (k and the round index live in device memory), so one captured
        // hipGraph replays the whole train at graph-launch cost.
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        hipLaunchKernelGGL(k_hssp3d_contrib_dk, dim3((unsigned)n_), dim3(128),
                           0, st, d_cand_, d_sx, d_sxz, d_sy, d_syz, d_syr, n_,
                           d_k, rx_, ry_, rz_, d_out_);
        hipLaunchKernelGGL(k_hssp3d_argmax, dim3(1), dim3(256), 0, st, d_out_,
                           n_, d_taken_, d_idx_);
        hipLaunchKernelGGL(k_hssp3d_insert, dim3(1), dim3(64), 0, st, d_cand_,
                           d_idx_, d_sx, d_sxz, d_sy, d_syz, d_syr, d_k,
                           d_chosen, d_round);
        HIP_CHECK(hipStreamEndCapture(st, &graph));
        HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        for (int64_t r = 0; r < subset_size; ++r)
            HIP_CHECK(hipGraphLaunch(exec, st));
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        py::array_t<int64_t> out(subset_size);
        HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_chosen, subset_size * 8,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return out;
    }

    int64_t round(const arr_f64& sx, const arr_f64& sxz, const arr_f64& sy,
                  const arr_f64& syz, const arr_i32& syr) {
        const int64_t k = sx.size();
        hipStream_t st = g_ws.get_stream();
        double* base = g_ws.ensure(4 * (size_t)k + (size_t)(k + 1) / 2 + 8);
        double* d_sx = base;
        double* d_sxz = d_sx + k;
        double* d_sy = d_sxz + k;
        double* d_syz = d_sy + k;
        int32_t* d_syr = reinterpret_cast<int32_t*>(d_syz + k);
        g_ws.begin_uploads();
        if (k > 0) {
            g_ws.h2d(d_sx, sx.data(), k * 8, st);
            g_ws.h2d(d_sxz, sxz.data(), k * 8, st);
            g_ws.h2d(d_sy, sy.data(), k * 8, st);
            g_ws.h2d(d_syz, syz.data(), k * 8, st);
            g_ws.h2d(d_syr, syr.data(), k * 4, st);
        }
        hipLaunchKernelGGL(k_hssp3d_contrib, dim3((unsigned)n_), dim3(128), 0,
                           st, d_cand_, d_sx, d_sxz, d_sy, d_syz, d_syr, n_, k,
                           rx_, ry_, rz_, d_out_);
        hipLaunchKernelGGL(k_hssp3d_argmax, dim3(1), dim3(256), 0, st, d_out_,
                           n_, d_taken_, d_idx_);
        int64_t idx = -1;
        HIP_CHECK(hipMemcpyAsync(&idx, d_idx_, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return idx;
    }

  private:
    int64_t n_;
    double rx_, ry_, rz_;
    double* d_cand_ = nullptr;
    double* d_out_ = nullptr;
    int64_t* d_idx_ = nullptr;
    uint8_t* d_taken_ = nullptr;
};


// ---------------------------------------------------------------------------
// K6c/K6d: 4-objective hypervolume and greedy HSSP. The kernels and the
// algorithm notes live in mo4d_kernels.h; these are the host entry points,
// mirroring the 3-D ones above.
// ---------------------------------------------------------------------------
#include "mo4d_kernels.h"

// 4-D hypervolume of points strictly inside ref, in any order. Host prep
// builds the three stable sorted views (N log N, negligible next to the N^3
// sweep); each block writes one partial and the host sums them in block order.
double hv4d(const arr_f64& pts, double ref_w, double ref_x, double ref_y,
            double ref_z) {
    if (pts.ndim() != 2 || pts.shape(1) != 4)
        throw std::runtime_error("hv4d: pts must be (N, 4)");
    const int64_t N = pts.shape(0);
    if (N == 0) return 0.0;
    if (N > (int64_t)65535 * HV4_TILE)
        throw std::runtime_error("hv4d: too many points");
    const double* P = pts.data();
    std::vector<int64_t> ow(N), ox(N), oy(N);
    for (int64_t i = 0; i < N; ++i) ow[i] = ox[i] = oy[i] = i;
    auto by_col = [&](int col) {
        return [P, col](int64_t a, int64_t b) { return P[a * 4 + col] < P[b * 4 + col]; };
    };
    std::stable_sort(ow.begin(), ow.end(), by_col(0));
    std::stable_sort(ox.begin(), ox.end(), by_col(1));
    std::stable_sort(oy.begin(), oy.end(), by_col(2));
    std::vector<double> ws(N), xs(N), yv(N), zv(N);
    std::vector<int32_t> rank_w(N), rank_x(N), rw(N), rx(N);
    for (int64_t i = 0; i < N; ++i) {
        ws[i] = P[ow[i] * 4];
        xs[i] = P[ox[i] * 4 + 1];
        rank_w[ow[i]] = (int32_t)i;
        rank_x[ox[i]] = (int32_t)i;
    }
    for (int64_t i = 0; i < N; ++i) {
        yv[i] = P[oy[i] * 4 + 2];
        zv[i] = P[oy[i] * 4 + 3];
        rw[i] = rank_w[oy[i]];
        rx[i] = rank_x[oy[i]];
    }
    const int64_t tiles = (N + HV4_TILE - 1) / HV4_TILE;
    const int64_t n_part = tiles * tiles;
    hipStream_t st = g_ws.get_stream();
    double* base = g_ws.ensure(4 * (size_t)N + (size_t)n_part + (size_t)N + 8);
    double* d_ws = base;
    double* d_xs = d_ws + N;
    double* d_yv = d_xs + N;
    double* d_zv = d_yv + N;
    double* d_out = d_zv + N;
    int32_t* d_rw = reinterpret_cast<int32_t*>(d_out + n_part);
    int32_t* d_rx = d_rw + N;
    g_ws.begin_uploads();
    g_ws.h2d(d_ws, ws.data(), N * 8, st);
    g_ws.h2d(d_xs, xs.data(), N * 8, st);
    g_ws.h2d(d_yv, yv.data(), N * 8, st);
    g_ws.h2d(d_zv, zv.data(), N * 8, st);
    g_ws.h2d(d_rw, rw.data(), N * 4, st);
    g_ws.h2d(d_rx, rx.data(), N * 4, st);
    hipLaunchKernelGGL(k_hv4d, dim3((unsigned)tiles, (unsigned)tiles),
                       dim3(HV4_THREADS), 0, st, d_ws, d_xs, d_yv, d_zv, d_rw,
                       d_rx, N, ref_w, ref_x, ref_y, ref_z, d_out);
    std::vector<double> part(n_part);
    HIP_CHECK(hipMemcpyAsync(part.data(), d_out, n_part * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double hv = 0.0;
    for (double v : part) hv += v;
    return hv;
}

static size_t hssp4d_lds_bytes(int64_t kcap) { return (size_t)kcap * 24; }

// Per-candidate greedy-HSSP contributions against a selected set passed as its
// six pre-sorted views. Stateless; the session below is the production path.
py::array_t<double> hssp4d_contrib(const arr_f64& cand, const arr_f64& sw,
                                   const arr_f64& sx, const arr_f64& sy,
                                   const arr_f64& syz, const arr_i32& syrw,
                                   const arr_i32& syrx, double ref_w,
                                   double ref_x, double ref_y, double ref_z) {
    if (cand.ndim() != 2 || cand.shape(1) != 4)
        throw std::runtime_error("hssp4d_contrib: cand must be (n, 4)");
    const int64_t n = cand.shape(0);
    const int64_t k = sw.size();
    if ((int64_t)sx.size() != k || (int64_t)sy.size() != k ||
        (int64_t)syz.size() != k || (int64_t)syrw.size() != k ||
        (int64_t)syrx.size() != k)
        throw std::runtime_error("hssp4d_contrib: ragged sorted views");
    if (k > HSSP4_MAX_K)
        throw std::runtime_error("hssp4d_contrib: selected set exceeds the LDS stream bound");
    py::array_t<double> out(n);
    if (n == 0) return out;
    hipStream_t st = g_ws.get_stream();
    double* base = g_ws.ensure((size_t)n * 4 + 4 * (size_t)k + n + (size_t)k + 8);
    double* d_cand = base;
    double* d_sw = d_cand + (size_t)n * 4;
    double* d_sx = d_sw + k;
    double* d_sy = d_sx + k;
    double* d_syz = d_sy + k;
    double* d_out = d_syz + k;
    int32_t* d_syrw = reinterpret_cast<int32_t*>(d_out + n);
    int32_t* d_syrx = d_syrw + k;
    g_ws.begin_uploads();
    g_ws.h2d(d_cand, cand.data(), (size_t)n * 4 * 8, st);
    if (k > 0) {
        g_ws.h2d(d_sw, sw.data(), k * 8, st);
        g_ws.h2d(d_sx, sx.data(), k * 8, st);
        g_ws.h2d(d_sy, sy.data(), k * 8, st);
        g_ws.h2d(d_syz, syz.data(), k * 8, st);
        g_ws.h2d(d_syrw, syrw.data(), k * 4, st);
        g_ws.h2d(d_syrx, syrx.data(), k * 4, st);
    }
    hipLaunchKernelGGL(k_hssp4d_contrib, dim3((unsigned)n), dim3(HSSP4_THREADS),
                       hssp4d_lds_bytes(k), st, d_cand, d_sw, d_sx, d_sy, d_syz,
                       d_syrw, d_syrx, k, k, ref_w, ref_x, ref_y, ref_z, d_out);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}

// Greedy-HSSP driver, 4 objectives: candidates, the taken-mask, the sorted
// selected-set views and the per-round winner all stay on device.
class Hssp4dSession {
  public:
    Hssp4dSession(const arr_f64& cand, double rw, double rx, double ry, double rz)
        : rw_(rw), rx_(rx), ry_(ry), rz_(rz) {
        if (cand.ndim() != 2 || cand.shape(1) != 4)
            throw std::runtime_error("Hssp4dSession: cand must be (n, 4)");
        n_ = cand.shape(0);
        if (n_ == 0) return;
        hipStream_t st = g_ws.get_stream();
        HIP_CHECK(hipMalloc(&d_cand_, (size_t)n_ * 4 * 8));
        HIP_CHECK(hipMalloc(&d_out_, (size_t)n_ * 8 + 8 + n_));
        d_idx_ = reinterpret_cast<int64_t*>(d_out_ + n_);
        d_taken_ = reinterpret_cast<uint8_t*>(d_idx_ + 1);
        HIP_CHECK(hipMemcpyAsync(d_cand_, cand.data(), (size_t)n_ * 4 * 8,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_taken_, 0, n_, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    ~Hssp4dSession() {
        if (d_cand_) (void)hipFree(d_cand_);
        if (d_out_) (void)hipFree(d_out_);
    }
    Hssp4dSession(const Hssp4dSession&) = delete;
    Hssp4dSession& operator=(const Hssp4dSession&) = delete;

    // Launch-train greedy: the contrib -> argmax -> insert round is captured
    // once as a linear three-kernel hipGraph (k and the round index live in
    // device memory, so every round has identical arguments) and replayed
    // subset_size times; ONE host sync at the end.
    py::array_t<int64_t> run(int64_t subset_size) {
        if (subset_size < 0)
            throw std::runtime_error("Hssp4dSession.run: negative subset_size");
        if (subset_size > n_) subset_size = n_;
        if (subset_size > HSSP4_MAX_K)
            throw std::runtime_error(
                "Hssp4dSession.run: subset_size exceeds the insert staging bound");
        py::array_t<int64_t> out(subset_size);
        if (subset_size == 0) return out;
        hipStream_t st = g_ws.get_stream();
        const size_t kcap = (size_t)subset_size + 1;
        double* base = g_ws.ensure(5 * kcap + subset_size + 6);
        double* d_sw = base;
        double* d_sx = d_sw + kcap;
        double* d_sy = d_sx + kcap;
        double* d_syz = d_sy + kcap;
        int32_t* d_syrw = reinterpret_cast<int32_t*>(d_syz + kcap);
        int32_t* d_syrx = d_syrw + kcap;  // the two rank arrays fill kcap doubles
        int64_t* d_k = reinterpret_cast<int64_t*>(base + 5 * kcap);
        int64_t* d_round = d_k + 1;
        int64_t* d_chosen = d_round + 1;
        HIP_CHECK(hipMemsetAsync(d_k, 0, 16, st));
        HIP_CHECK(hipMemsetAsync(d_taken_, 0, n_, st));
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        hipLaunchKernelGGL(k_hssp4d_contrib_dk, dim3((unsigned)n_),
                           dim3(HSSP4_THREADS), hssp4d_lds_bytes(kcap), st,
                           d_cand_, d_sw, d_sx, d_sy, d_syz, d_syrw, d_syrx, d_k,
                           (int64_t)kcap, rw_, rx_, ry_, rz_, d_out_);
        hipLaunchKernelGGL(k_hssp3d_argmax, dim3(1), dim3(256), 0, st, d_out_,
                           n_, d_taken_, d_idx_);
        hipLaunchKernelGGL(k_hssp4d_insert, dim3(1), dim3(HSSP4_THREADS), 0, st,
                           d_cand_, d_idx_, d_sw, d_sx, d_sy, d_syz, d_syrw,
                           d_syrx, d_k, d_chosen, d_round);
        HIP_CHECK(hipStreamEndCapture(st, &graph));
        HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        hipError_t err = hipSuccess;
        for (int64_t r = 0; r < subset_size && err == hipSuccess; ++r)
            err = hipGraphLaunch(exec, st);
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        HIP_CHECK(err);
        HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_chosen, subset_size * 8,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return out;
    }

  private:
    int64_t n_ = 0;
    double rw_, rx_, ry_, rz_;
    double* d_cand_ = nullptr;
    double* d_out_ = nullptr;
    int64_t* d_idx_ = nullptr;
    uint8_t* d_taken_ = nullptr;
};


// ---------------------------------------------------------------------------
// K5: fused GP log-EI forward + gradient over a device-resident GP.
//
// The torch path spends ~50 launches per batched acquisition evaluation
// (posterior GEMMs, erfc branches, autograd); here one kernel computes the
// cross-covariances, a rocBLAS dgemm applies the explicit covariance inverse
// and one kernel finalizes mean/var, the tail-stable log-EI and its CLOSED
// FORM gradient:  df/dmean = exp(logPhi(z) - logg(z))/s,
// df/dvar = exp(logphi(z) - logg(z))/(2 var),
// dk_i/dx_d = scale * m52'(r2_i) * 2 eta_d (x_d - X_id) — so
// grad_d = 2 eta_d (x_d * sum_i c_i - sum_i c_i X_id) with
// c_i = (w_m alpha_i - 2 w_v V_i) * scale * m52'(r2_i).
// Tensors stay wherever torch put them: the session takes raw device
// pointers (same process, same HIP context).
// ---------------------------------------------------------------------------
#include <rocblas/rocblas.h>

#define ROCBLAS_CHECK(expr)                                                     \
    do {                                                                        \
        rocblas_status s_ = (expr);                                             \
        if (s_ != rocblas_status_success)                                       \
            throw std::runtime_error("rocBLAS error " + std::to_string(s_));    \
    } while (0)

static rocblas_handle g_blas = nullptr;
static rocblas_handle get_blas(hipStream_t st) {
    if (!g_blas) ROCBLAS_CHECK(rocblas_create_handle(&g_blas));
    ROCBLAS_CHECK(rocblas_set_stream(g_blas, st));
    return g_blas;
}

__device__ __forceinline__ double d_log_ndtr(double z) {
    if (z >= 0.0) return log(0.5 * erfc(-z * 0.7071067811865476));
    return -0.5 * z * z + log(0.5 * erfcx(-z * 0.7071067811865476));
}

// log(z*Phi(z) + phi(z)), the same two-branch form as the host standard_logei.
__device__ __forceinline__ double d_standard_logei(double z) {
    constexpr double HALF_LOG_2PI = 0.9189385332046727;
    if (z >= -1.0) {
        const double phi = exp(-0.5 * z * z - HALF_LOG_2PI);
        return log(z * 0.5 * erfc(-z * 0.7071067811865476) + phi);
    }
    const double mills = 1.2533141373155003 * z * erfcx(-z * 0.7071067811865476);
    return (-0.5 * z * z - HALF_LOG_2PI) + log1p(mills);
}

// Phase 1: cross-covariance K[b, i] = scale * m52(r2) and its radial part.
__global__ void k_gp_cross_cov(const double* __restrict__ X,  // (N, D)
                               const double* __restrict__ eta,  // (D)
                               double scale, const double* __restrict__ x,  // (B, D)
                               int64_t N, int64_t D, int64_t B,
                               double* __restrict__ K,    // (B, N)
                               double* __restrict__ MP) {  // (B, N) scale*m52'(r2)
    __shared__ double xs[64];
    __shared__ double et[64];
    const int64_t b = blockIdx.y;
    for (int64_t d = threadIdx.x; d < D; d += blockDim.x) {
        xs[d] = x[b * D + d];
        et[d] = eta[d];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double r2 = 0.0;
    for (int64_t d = 0; d < D; ++d) {
        const double diff = xs[d] - X[i * D + d];
        r2 += et[d] * diff * diff;
    }
    const double u = sqrt(5.0 * r2);
    const double eu = exp(-u);
    K[b * N + i] = scale * (eu * ((5.0 / 3.0) * r2 + u + 1.0));
    MP[b * N + i] = scale * ((-5.0 / 6.0) * (1.0 + u) * eu);
}

// Phase 3: per-candidate mean/var/log-EI (+ gradient when out_grad != null).
__global__ void k_gp_logei_final(const double* __restrict__ K,      // (B, N)
                                 const double* __restrict__ MP,     // (B, N)
                                 const double* __restrict__ V,      // (B, N) = K @ Cinv
                                 const double* __restrict__ alpha,  // (N)
                                 const double* __restrict__ X,      // (N, D)
                                 const double* __restrict__ eta,    // (D)
                                 const double* __restrict__ x,      // (B, D)
                                 double scale, double stab_noise,
                                 double threshold, int64_t N, int64_t D,
                                 double* __restrict__ out_f,     // (B)
                                 double* __restrict__ out_grad) {  // (B, D) or null
    constexpr int MAXD = 64;
    __shared__ double red_a[256];
    __shared__ double red_b[256];
    __shared__ double s_wm, s_wv;
    __shared__ double red_d[MAXD];
    const int64_t b = blockIdx.x;
    const double* Kb = K + b * N;
    const double* Vb = V + b * N;

    double acc_m = 0.0, acc_v = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += blockDim.x) {
        const double k = Kb[i];
        acc_m += k * alpha[i];
        acc_v += k * Vb[i];
    }
    red_a[threadIdx.x] = acc_m;
    red_b[threadIdx.x] = acc_v;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) {
            red_a[threadIdx.x] += red_a[threadIdx.x + stride];
            red_b[threadIdx.x] += red_b[threadIdx.x + stride];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = red_a[0];
        double var = scale - red_b[0];
        var = (var > 0.0 ? var : 0.0) + stab_noise;
        const double sdev = sqrt(var);
        const double z = (mean - threshold) / sdev;
        const double logg = d_standard_logei(z);
        out_f[b] = 0.5 * log(var) + logg;
        if (out_grad) {
            constexpr double HALF_LOG_2PI = 0.9189385332046727;
            // df/dmean and df/dvar in stable log space.
            s_wm = exp(d_log_ndtr(z) - logg) / sdev;
            s_wv = exp(-0.5 * z * z - HALF_LOG_2PI - logg) / (2.0 * var);
        }
    }
    if (!out_grad) return;
    __syncthreads();
    const double wm = s_wm, wv = s_wv;
    double accd[MAXD];
    for (int64_t d = 0; d < D; ++d) accd[d] = 0.0;
    double acc_c = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += blockDim.x) {
        const double c = (wm * alpha[i] - 2.0 * wv * Vb[i]) * MP[b * N + i];
        acc_c += c;
        for (int64_t d = 0; d < D; ++d) accd[d] += c * X[i * D + d];
    }
    red_a[threadIdx.x] = acc_c;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red_a[threadIdx.x] += red_a[threadIdx.x + stride];
        __syncthreads();
    }
    const double sum_c = red_a[0];
    for (int64_t d = 0; d < D; ++d) {
        red_b[threadIdx.x] = accd[d];
        __syncthreads();
        for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
            if ((int)threadIdx.x < stride) red_b[threadIdx.x] += red_b[threadIdx.x + stride];
            __syncthreads();
        }
        if (threadIdx.x == 0) red_d[d] = red_b[0];
        __syncthreads();
    }
    for (int64_t d = threadIdx.x; d < D; d += blockDim.x) {
        out_grad[b * D + d] = 2.0 * eta[d] * (x[b * D + d] * sum_c - red_d[d]);
    }
}

// Session over torch-owned device tensors (raw pointers; same HIP context).
// Built once per fitted GP; evaluations upload only the (B, D) candidates.
class GpLogEiSession {
  public:
    GpLogEiSession(int64_t X_ptr, int64_t alpha_ptr, int64_t cinv_ptr,
                   int64_t eta_ptr, int64_t N, int64_t D, double scale,
                   double stab_noise, double threshold)
        : X_(reinterpret_cast<const double*>(X_ptr)),
          alpha_(reinterpret_cast<const double*>(alpha_ptr)),
          cinv_(reinterpret_cast<const double*>(cinv_ptr)),
          eta_(reinterpret_cast<const double*>(eta_ptr)),
          N_(N), D_(D), scale_(scale), stab_(stab_noise), thr_(threshold) {
        if (D > 64) throw std::runtime_error("GpLogEiSession: D > 64");
    }

    py::tuple eval(const arr_f64& x, bool with_grad) {
        const int64_t B = x.shape(0);
        if (x.shape(1) != D_) throw std::runtime_error("eval: dim mismatch");
        hipStream_t st = g_ws.get_stream();
        const size_t nK = (size_t)B * N_;
        double* base = g_ws.ensure(3 * nK + (size_t)B * D_ + B + (size_t)B * D_ + 8);
        double* d_K = base;
        double* d_MP = d_K + nK;
        double* d_V = d_MP + nK;
        double* d_x = d_V + nK;
        double* d_f = d_x + (size_t)B * D_;
        double* d_g = d_f + B;
        g_ws.begin_uploads();
        g_ws.h2d(d_x, x.data(), (size_t)B * D_ * 8, st);
        {
            const int block = 256;
            const dim3 grid((unsigned)((N_ + block - 1) / block), (unsigned)B);
            hipLaunchKernelGGL(k_gp_cross_cov, grid, dim3(block), 0, st, X_,
                               eta_, scale_, d_x, N_, D_, B, d_K, d_MP);
        }
        {
            // V(B,N) = K(B,N) @ Cinv(N,N): column-major dgemm with the
            // symmetric Cinv — C^T = Cinv^T @ K^T == Cinv @ K^T.
            const double one = 1.0, zero = 0.0;
            ROCBLAS_CHECK(rocblas_dgemm(get_blas(st), rocblas_operation_none,
                                        rocblas_operation_none, (rocblas_int)N_,
                                        (rocblas_int)B, (rocblas_int)N_, &one,
                                        cinv_, (rocblas_int)N_, d_K,
                                        (rocblas_int)N_, &zero, d_V,
                                        (rocblas_int)N_));
        }
        hipLaunchKernelGGL(k_gp_logei_final, dim3((unsigned)B), dim3(256), 0,
                           st, d_K, d_MP, d_V, alpha_, X_, eta_, d_x, scale_,
                           stab_, thr_, N_, D_, d_f,
                           with_grad ? d_g : nullptr);
        py::array_t<double> f(B);
        HIP_CHECK(hipMemcpyAsync(f.mutable_data(), d_f, B * 8,
                                 hipMemcpyDeviceToHost, st));
        py::array_t<double> g;
        if (with_grad) {
            g = py::array_t<double>({B, D_});
            HIP_CHECK(hipMemcpyAsync(g.mutable_data(), d_g, (size_t)B * D_ * 8,
                                     hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return py::make_tuple(f, g);
    }

  private:
    const double *X_, *alpha_, *cinv_, *eta_;
    int64_t N_, D_;
    double scale_, stab_, thr_;
};

PYBIND11_MODULE(_hipcore, m) {
    m.doc() = "optuna_amd MI355X (gfx950) HIP kernels: TPE parzen fit + mixture "
              "log-pdf, truncnorm device library";
    m.def("available", &available);
    m.def("device_count", &device_count);
    m.def("log_gauss_mass", &log_gauss_mass);
    m.def("truncnorm_ppf", &truncnorm_ppf);
    m.def("truncnorm_logpdf", &truncnorm_logpdf);
    m.def("nondomination_rank", &nondomination_rank, py::arg("vals"),
          py::arg("n_below"));
    m.def("hv3d", &hv3d, py::arg("pts"), py::arg("ref_x"), py::arg("ref_y"),
          py::arg("ref_z"));
    py::class_<GpLogEiSession>(m, "GpLogEiSession")
        .def(py::init<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                      double, double, double>(),
             py::arg("X_ptr"), py::arg("alpha_ptr"), py::arg("cinv_ptr"),
             py::arg("eta_ptr"), py::arg("N"), py::arg("D"), py::arg("scale"),
             py::arg("stab_noise"), py::arg("threshold"))
        .def("eval", &GpLogEiSession::eval, py::arg("x"), py::arg("with_grad"));
    py::class_<Hssp3dSession>(m, "Hssp3dSession")
        .def(py::init<const arr_f64&, double, double, double>(), py::arg("cand"),
             py::arg("ref_x"), py::arg("ref_y"), py::arg("ref_z"))
        .def("round", &Hssp3dSession::round, py::arg("sx"), py::arg("sxz"),
             py::arg("sy"), py::arg("syz"), py::arg("syr"))
        .def("run", &Hssp3dSession::run, py::arg("subset_size"));
    m.def("hssp3d_contrib", &hssp3d_contrib, py::arg("cand"), py::arg("sx"),
          py::arg("sxz"), py::arg("sy"), py::arg("syz"), py::arg("syr"),
          py::arg("ref_x"), py::arg("ref_y"), py::arg("ref_z"));
    m.def("hv4d", &hv4d, py::arg("pts"), py::arg("ref_w"), py::arg("ref_x"),
          py::arg("ref_y"), py::arg("ref_z"));
    m.def("hssp4d_contrib", &hssp4d_contrib, py::arg("cand"), py::arg("sw"),
          py::arg("sx"), py::arg("sy"), py::arg("syz"), py::arg("syrw"),
          py::arg("syrx"), py::arg("ref_w"), py::arg("ref_x"), py::arg("ref_y"),
          py::arg("ref_z"));
    py::class_<Hssp4dSession>(m, "Hssp4dSession")
        .def(py::init<const arr_f64&, double, double, double, double>(),
             py::arg("cand"), py::arg("ref_w"), py::arg("ref_x"),
             py::arg("ref_y"), py::arg("ref_z"))
        .def("run", &Hssp4dSession::run, py::arg("subset_size"));
    m.attr("HSSP4D_MAX_SUBSET") = py::int_(HSSP4_MAX_K);
    m.def("kde_logpdf", &kde_logpdf, py::arg("obs"), py::arg("sorted_pos"),
          py::arg("logw"), py::arg("alow"), py::arg("ahigh"), py::arg("steps"),
          py::arg("n_choices"), py::arg("prior_weight"),
          py::arg("x"), py::arg("xedges"),
          py::arg("consider_endpoints") = false, py::arg("magic_clip") = true);
    py::class_<TpeDeviceHistory>(m, "TpeDeviceHistory")
        .def(py::init<int64_t>(), py::arg("dims"))
        .def_property_readonly("n_rows", &TpeDeviceHistory::n_rows)
        .def("append", &TpeDeviceHistory::append, py::arg("block"))
        .def("upload_sorted", &TpeDeviceHistory::upload_sorted, py::arg("cols"))
        .def("insert_sorted", &TpeDeviceHistory::insert_sorted, py::arg("pos"),
             py::arg("rows"))
        .def_property_readonly("n_sorted", &TpeDeviceHistory::n_sorted)
        .def("insert_sorted_by_value", &TpeDeviceHistory::insert_sorted_by_value,
             py::arg("first_row"), py::arg("n_new"))
        .def("sorted_index", &TpeDeviceHistory::sorted_index)
        .def("set_domain", &TpeDeviceHistory::set_domain, py::arg("alow"),
             py::arg("ahigh"), py::arg("steps"), py::arg("n_choices"))
        .def("fused_prepare", &TpeDeviceHistory::fused_prepare, py::arg("excl"),
             py::arg("n_above"), py::arg("logw") = arr_f64(),
             py::arg("w_num") = 0, py::arg("w_start") = 1.0,
             py::arg("w_step") = 0.0, py::arg("log_total") = 0.0,
             py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true)
        .def("fused_score", &TpeDeviceHistory::fused_score, py::arg("excl"),
             py::arg("n_above"), py::arg("x"), py::arg("xedges"),
             py::arg("bmu"), py::arg("bsig"), py::arg("bw"),
             py::arg("logw") = arr_f64(), py::arg("w_num") = 0,
             py::arg("w_start") = 1.0, py::arg("w_step") = 0.0,
             py::arg("log_total") = 0.0, py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true, py::arg("return_parts") = false)
        .def("score", &TpeDeviceHistory::score, py::arg("sorted_rows"),
             py::arg("pos"), py::arg("n_above"), py::arg("logw"), py::arg("alow"),
             py::arg("ahigh"), py::arg("steps"), py::arg("n_choices"),
             py::arg("prior_weight"), py::arg("x"), py::arg("xedges"),
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true,
             py::arg("extras_raw") = arr_f64(),
             py::arg("extras_sorted") = arr_f64(),
             py::arg("extras_sorted_idx") = arr_i32(),
             py::arg("per_dim") = false);
}
