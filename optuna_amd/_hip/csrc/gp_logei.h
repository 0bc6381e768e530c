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

#pragma once

#include <rocblas/rocblas.h>

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

// The feasibility term of the constrained acquisitions (gp_feasibility.h),
// which the sessions add to their own result on the device when handed a
// constraint set. With no set (nullptr) nothing below does anything.
class GpConstraintSet;
// Throws unless the set was built for the same (N, D).
static void feas_check_shape(const GpConstraintSet* cs, int64_t N, int64_t D);
// Doubles of partial records for chunks of at most `rows` candidates.
static size_t feas_part_doubles(const GpConstraintSet* cs, int64_t rows, bool with_grad);
// Enqueue f += sum_c log Phi(z_c), g += its gradient for the bc candidates xc;
// K / MP / V are (bc, N) scratch the caller is done with.
static void feas_enqueue_add(const GpConstraintSet* cs, hipStream_t st,
                             rocblas_handle blas, const double* xc, int64_t bc,
                             bool with_grad, double* K, double* MP, double* V,
                             double* part, double* f, double* g);

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

    // With a constraint set the feasibility term and its gradient are added
    // on the device, in the (B, N) regions the log-EI kernels are done with,
    // before the one copy back.
    py::tuple eval(const arr_f64& x, bool with_grad,
                   const GpConstraintSet* constraints = nullptr) {
        const int64_t B = x.shape(0);
        if (x.shape(1) != D_) throw std::runtime_error("eval: dim mismatch");
        if (constraints) {
            feas_check_shape(constraints, N_, D_);
            // 65535 is the grid's y extent in k_gp_cross_cov.
            if (B > 65535) throw std::runtime_error("eval: more than 65535 candidates");
        }
        hipStream_t st = g_ws.get_stream();
        const size_t nK = (size_t)B * N_;
        WsLayout L;
        const auto s_K = L.add<double>(nK), s_MP = L.add<double>(nK),
                   s_V = L.add<double>(nK), s_x = L.add<double>((size_t)B * D_),
                   s_f = L.add<double>(B), s_g = L.add<double>((size_t)B * D_),
                   s_part = L.add<double>(
                       constraints ? feas_part_doubles(constraints, B, with_grad) : 0);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_K = s_K.in(base), *d_MP = s_MP.in(base), *d_V = s_V.in(base),
               *d_x = s_x.in(base), *d_f = s_f.in(base), *d_g = s_g.in(base),
               *d_part = s_part.in(base);
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
        if (constraints && B > 0)
            feas_enqueue_add(constraints, st, get_blas(st), d_x, B, with_grad, d_K,
                             d_MP, d_V, d_part, d_f, with_grad ? d_g : nullptr);
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
