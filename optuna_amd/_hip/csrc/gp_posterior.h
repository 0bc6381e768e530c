// ---------------------------------------------------------------------------
// K5 (shared): one GP posterior over a device-resident GP, and the two ends
// of an evaluation, as all three GP sessions use them.
//
// Per candidate x the posterior needs K = k(x, X), its radial derivative MP
// and V = K @ Cinv against the explicit covariance inverse; every session
// goes on from there with its own kernels (gp_logei.h, gp_ehvi.h,
// gp_feasibility.h). Tensors stay wherever torch put them: a GpRef holds raw
// device pointers (same process, same HIP context).
// ---------------------------------------------------------------------------

#pragma once

#include <rocblas/rocblas.h>

#include "gp_plan.h"
#include "hip_common.h"

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

constexpr int GP_BLOCK = 256;
constexpr int GP_WAVES = GP_BLOCK / 64;

// Sum of the four per-wavefront partials, in wavefront order, seen by every
// thread. `red` holds GP_WAVES doubles.
__device__ __forceinline__ double gp_block_sum(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();  // the previous user of `red` is done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double out = red[0];
    for (int w = 1; w < GP_WAVES; ++w) out += red[w];
    return out;
}

// Cross-covariance K[b, i] = scale * m52(r2) and its radial part. MIXED adds
// the categorical columns of `cat_mask` (bit d = column d): there the term of
// r2 is eta_d * [x_d != X_id], the Hamming indicator, in place of the squared
// difference. MP stays the derivative with respect to r2 either way.
template <bool MIXED>
__global__ void k_gp_cross_cov(const double* __restrict__ X,  // (N, D)
                               const double* __restrict__ eta,  // (D)
                               double scale, const double* __restrict__ x,  // (B, D)
                               int64_t N, int64_t D, int64_t B,
                               double* __restrict__ K,    // (B, N)
                               double* __restrict__ MP,   // (B, N) scale*m52'(r2)
                               uint64_t cat_mask) {
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
        if constexpr (MIXED) {
            if ((cat_mask >> d) & 1) {
                r2 += et[d] * (diff != 0.0 ? 1.0 : 0.0);
                continue;
            }
        }
        r2 += et[d] * diff * diff;
    }
    const double u = sqrt(5.0 * r2);
    const double eu = exp(-u);
    K[b * N + i] = scale * (eu * ((5.0 / 3.0) * r2 + u + 1.0));
    MP[b * N + i] = scale * ((-5.0 / 6.0) * (1.0 + u) * eu);
}

// One fitted GP on the device: X (N, D), alpha = Cinv @ y (N), the explicit
// inverse Cinv (N, N), eta (D), the kernel scale and the categorical columns
// of the search space (bit d = column d; all GPs of a session share it).
struct GpRef {
    const double *X, *alpha, *cinv, *eta;
    double scale;
    uint64_t cat_mask;
};

// Throws, with `who` in front, unless 1 <= D <= 64 and `cat_mask` names
// columns below D only.
static void gp_check_dims(const std::string& who, int64_t D, uint64_t cat_mask) {
    if (D < 1 || D > 64) throw std::runtime_error(who + ": need 1 <= D <= 64");
    if (D < 64 && (cat_mask >> D) != 0)
        throw std::runtime_error(who + ": cat_mask has a bit at or above D");
}

// Whether column d is categorical.
__host__ __device__ __forceinline__ bool gp_is_cat(uint64_t cat_mask, int d) {
    return (cat_mask >> d) & 1;
}

// The GPs behind four pointer vectors and their scales into out[0 .. n), n
// returned. Throws, with `who` in front, unless there is one entry per GP,
// lo <= n <= hi, 1 <= D <= 64, cat_mask within D and N >= 1.
static int gp_make_refs(const std::string& who, const std::vector<int64_t>& X_ptrs,
                        const std::vector<int64_t>& alpha_ptrs,
                        const std::vector<int64_t>& cinv_ptrs,
                        const std::vector<int64_t>& eta_ptrs,
                        const std::vector<double>& scales, int lo, int hi,
                        int64_t N, int64_t D, uint64_t cat_mask, GpRef* out) {
    const size_t n = scales.size();
    if (n < (size_t)lo || n > (size_t)hi)
        throw std::runtime_error(who + ": need " + std::to_string(lo) +
                                 " <= GPs <= " + std::to_string(hi));
    if (X_ptrs.size() != n || alpha_ptrs.size() != n || cinv_ptrs.size() != n ||
        eta_ptrs.size() != n)
        throw std::runtime_error(who + ": one pointer per GP");
    gp_check_dims(who, D, cat_mask);
    if (N < 1) throw std::runtime_error(who + ": N < 1");
    for (size_t i = 0; i < n; ++i)
        out[i] = GpRef{reinterpret_cast<const double*>(X_ptrs[i]),
                       reinterpret_cast<const double*>(alpha_ptrs[i]),
                       reinterpret_cast<const double*>(cinv_ptrs[i]),
                       reinterpret_cast<const double*>(eta_ptrs[i]), scales[i],
                       cat_mask};
    return (int)n;
}

// Enqueue K and MP (bc, N) of the bc <= GP_GRID_Y_MAX candidates x, then
// V(bc, N) = K(bc, N) @ Cinv(N, N): a column-major dgemm with the symmetric
// Cinv — C^T = Cinv^T @ K^T == Cinv @ K^T. An all-continuous space runs the
// unmixed cross-covariance instantiation.
static void gp_enqueue_kv(hipStream_t st, rocblas_handle blas, const GpRef& gp,
                          const double* x, int64_t bc, int64_t N, int64_t D,
                          double* K, double* MP, double* V) {
    const dim3 grid((unsigned)((N + GP_BLOCK - 1) / GP_BLOCK), (unsigned)bc);
    if (gp.cat_mask != 0)
        hipLaunchKernelGGL(k_gp_cross_cov<true>, grid, dim3(GP_BLOCK), 0, st, gp.X,
                           gp.eta, gp.scale, x, N, D, bc, K, MP, gp.cat_mask);
    else
        hipLaunchKernelGGL(k_gp_cross_cov<false>, grid, dim3(GP_BLOCK), 0, st, gp.X,
                           gp.eta, gp.scale, x, N, D, bc, K, MP, gp.cat_mask);
    const double one = 1.0, zero = 0.0;
    ROCBLAS_CHECK(rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none,
                                (rocblas_int)N, (rocblas_int)bc, (rocblas_int)N,
                                &one, gp.cinv, (rocblas_int)N, K, (rocblas_int)N,
                                &zero, V, (rocblas_int)N));
}

// The two ends of an eval(x, with_grad): the check of x (B, D) on
// construction, the upload of the candidates, and the one copy back with the
// one synchronisation. No candidates need no device:
//     GpEvalIo io(x, D_, with_grad);
//     if (io.B == 0) return io.download(nullptr, nullptr);
struct GpEvalIo {
    const arr_f64& x;
    const int64_t B, D;
    const bool with_grad;
    hipStream_t st = nullptr;

    GpEvalIo(const arr_f64& x_, int64_t D_, bool with_grad_)
        : x(x_), B(x_.ndim() == 2 ? x_.shape(0) : 0), D(D_), with_grad(with_grad_) {
        if (x.ndim() != 2 || x.shape(1) != D)
            throw std::runtime_error("eval: dim mismatch");
    }

    // The candidates into d_x (B, D); the stream everything else goes on.
    hipStream_t upload(double* d_x) {
        st = g_ws.get_stream();
        g_ws.begin_uploads();
        g_ws.h2d(d_x, x.data(), (size_t)B * D * 8, st);
        return st;
    }

    // (f (B), g (B, D)) from the device; g is empty without the gradient.
    py::tuple download(const double* d_f, const double* d_g) const {
        py::array_t<double> f(B);
        py::array_t<double> g;
        if (with_grad) g = py::array_t<double>({B, D});
        if (B == 0) return py::make_tuple(f, g);
        HIP_CHECK(hipMemcpyAsync(f.mutable_data(), d_f, B * 8, hipMemcpyDeviceToHost, st));
        if (with_grad)
            HIP_CHECK(hipMemcpyAsync(g.mutable_data(), d_g, (size_t)B * D * 8,
                                     hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return py::make_tuple(f, g);
    }
};
