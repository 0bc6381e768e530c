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
// c_i = (w_m alpha_i - 2 w_v V_i) * scale * m52'(r2_i). On a categorical
// column (a bit of cat_mask) r2 holds the Hamming indicator, which does not
// move with x: grad_d is exactly 0 there.
// The first two steps are gp_posterior.h's.
// ---------------------------------------------------------------------------

#pragma once

#include "gp_feasibility.h"

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

// Phase 3 (phases 1 and 2 are gp_enqueue_kv): per-candidate mean/var/log-EI (+ gradient when out_grad != null).
__global__ void k_gp_logei_final(const double* __restrict__ K,      // (B, N)
                                 const double* __restrict__ MP,     // (B, N)
                                 const double* __restrict__ V,      // (B, N) = K @ Cinv
                                 const double* __restrict__ alpha,  // (N)
                                 const double* __restrict__ X,      // (N, D)
                                 const double* __restrict__ eta,    // (D)
                                 const double* __restrict__ x,      // (B, D)
                                 double scale, double stab_noise,
                                 double threshold, int64_t N, int64_t D,
                                 uint64_t cat_mask,
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
        if (gp_is_cat(cat_mask, (int)d)) continue;  // block-uniform; red_d[d] unused
        red_b[threadIdx.x] = accd[d];
        __syncthreads();
        for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
            if ((int)threadIdx.x < stride) red_b[threadIdx.x] += red_b[threadIdx.x + stride];
            __syncthreads();
        }
        if (threadIdx.x == 0) red_d[d] = red_b[0];
        __syncthreads();
    }
    // The Hamming term of a categorical column does not move with x.
    for (int64_t d = threadIdx.x; d < D; d += blockDim.x) {
        out_grad[b * D + d] =
            gp_is_cat(cat_mask, (int)d)
                ? 0.0
                : 2.0 * eta[d] * (x[b * D + d] * sum_c - red_d[d]);
    }
}

// Session over torch-owned device tensors (raw pointers; same HIP context).
// Built once per fitted GP; evaluations upload only the (B, D) candidates.
class GpLogEiSession {
  public:
    GpLogEiSession(int64_t X_ptr, int64_t alpha_ptr, int64_t cinv_ptr,
                   int64_t eta_ptr, int64_t N, int64_t D, double scale,
                   double stab_noise, double threshold, uint64_t cat_mask = 0)
        : N_(N), D_(D), stab_(stab_noise), thr_(threshold) {
        gp_make_refs("GpLogEiSession", {X_ptr}, {alpha_ptr}, {cinv_ptr}, {eta_ptr},
                     {scale}, 1, 1, N, D, cat_mask, &gp_);
    }

    // With a constraint set the feasibility term and its gradient are added
    // on the device, in the (B, N) regions the log-EI kernels are done with,
    // before the one copy back.
    py::tuple eval(const arr_f64& x, bool with_grad,
                   const GpConstraintSet* constraints = nullptr) {
        GpEvalIo io(x, D_, with_grad);
        if (constraints) constraints->check_shape(N_, D_, gp_.cat_mask);
        const int64_t B = io.B;
        if (B == 0) return io.download(nullptr, nullptr);
        // The whole batch is one chunk.
        if (B > GP_GRID_Y_MAX) throw std::runtime_error("eval: more than 65535 candidates");
        const size_t nK = (size_t)B * N_;
        WsLayout L;
        const auto s_K = L.add<double>(nK), s_MP = L.add<double>(nK),
                   s_V = L.add<double>(nK), s_x = L.add<double>((size_t)B * D_),
                   s_f = L.add<double>(B), s_g = L.add<double>((size_t)B * D_),
                   s_part = L.add<double>(
                       constraints ? constraints->part_doubles(B, with_grad) : 0);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_K = s_K.in(base), *d_MP = s_MP.in(base), *d_V = s_V.in(base),
               *d_x = s_x.in(base), *d_f = s_f.in(base), *d_g = s_g.in(base),
               *d_part = s_part.in(base);
        hipStream_t st = io.upload(d_x);
        rocblas_handle blas = get_blas(st);
        gp_enqueue_kv(st, blas, gp_, d_x, B, N_, D_, d_K, d_MP, d_V);
        hipLaunchKernelGGL(k_gp_logei_final, dim3((unsigned)B), dim3(256), 0,
                           st, d_K, d_MP, d_V, gp_.alpha, gp_.X, gp_.eta, d_x,
                           gp_.scale, stab_, thr_, N_, D_, gp_.cat_mask, d_f,
                           with_grad ? d_g : nullptr);
        if (constraints)
            constraints->enqueue(st, blas, d_x, B, with_grad, true, d_K, d_MP, d_V,
                                 d_part, d_f, with_grad ? d_g : nullptr);
        return io.download(d_f, d_g);
    }

  private:
    GpRef gp_;
    int64_t N_, D_;
    double stab_, thr_;
};
