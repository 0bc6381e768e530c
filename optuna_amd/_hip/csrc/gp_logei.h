// ---------------------------------------------------------------------------
// K5: fused GP log-EI forward + gradient over a device-resident GP.
//
// The torch path spends ~50 launches per batched acquisition evaluation
// (posterior GEMMs, erfc branches, autograd); here one kernel computes the
// cross-covariances, a rocBLAS dgemm applies the explicit covariance inverse
// and one kernel finalizes mean/var, the tail-stable log-EI and its CLOSED
// FORM gradient:  df/dmean = (Phi(z)/h(z))/s,
// df/dvar = (phi(z)/h(z))/(2 var), 0 where the clamp on the raw variance is
// active (d_logei_weights has the two ratios),
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

// For z < -1 the expectation is h(z) = z Phi(z) + phi(z) = phi(z) (1 + m) with
// m = sqrt(pi/2) z erfcx(-z/sqrt 2) in (-1, 0). 1 + m behaves like 1/z^2, so
// forming it from m loses about z^2 ulps. Below LOGEI_SERIES_Z it comes from
// the asymptotic series
//   1 + m = 1/z^2 - 3/z^4 + 15/z^6 - 105/z^8 + 945/z^10 - ...
// cut after four terms. The two numbers go together
// (mpmath, 80 digits; scripts/gen_gp_logei_golden.py prints both figures):
//   * at z = -256 the four terms differ from 1 + m by 5.1e-17 of it, under
//     2^-53 = 1.1e-16, and by less further out (three terms: 3.7e-13);
//   * just above the cut the direct form is off by about z^2 2^-53 = 7.3e-12,
//     1e5 times under the gradient tolerance 1e-6 where a factor of 100 is
//     asked for, which |z| <= 9490 would still give.
constexpr double LOGEI_SERIES_Z = -256.0;

// 1 + m for z < LOGEI_SERIES_Z: the four terms.
__device__ __forceinline__ double d_logei_series(double z) {
    const double u = 1.0 / (z * z);
    return u * (1.0 - u * (3.0 - u * (15.0 - 105.0 * u)));
}

// log(z*Phi(z) + phi(z)), the same three-branch form as the host standard_logei.
__device__ __forceinline__ double d_standard_logei(double z) {
    constexpr double HALF_LOG_2PI = 0.9189385332046727;
    if (z >= -1.0) {
        const double phi = exp(-0.5 * z * z - HALF_LOG_2PI);
        return log(z * 0.5 * erfc(-z * 0.7071067811865476) + phi);
    }
    if (z < LOGEI_SERIES_Z)
        return (-0.5 * z * z - HALF_LOG_2PI) + log(d_logei_series(z));
    const double mills = 1.2533141373155003 * z * erfcx(-z * 0.7071067811865476);
    return (-0.5 * z * z - HALF_LOG_2PI) + log1p(mills);
}

// r_m = Phi(z)/h(z) = d log h / dz and r_v = phi(z)/h(z), given logg = log h(z).
// For z < -1 both come from erfcx and 1 + m: the log-space form subtracts two
// numbers of size z^2/2 and has lost every digit by z = -1e8.
__device__ __forceinline__ void d_logei_weights(double z, double logg, double* r_m,
                                                double* r_v) {
    constexpr double HALF_LOG_2PI = 0.9189385332046727;
    if (z >= -1.0) {
        *r_m = exp(d_log_ndtr(z) - logg);
        *r_v = exp(-0.5 * z * z - HALF_LOG_2PI - logg);
        return;
    }
    const double e = erfcx(-z * 0.7071067811865476);
    const double s =
        z < LOGEI_SERIES_Z ? d_logei_series(z) : 1.0 + 1.2533141373155003 * z * e;
    *r_m = 1.2533141373155003 * e / s;
    *r_v = 1.0 / s;
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
        const double raw = scale - red_b[0];
        // Like autograd through clamp_min(0), and like k_gp_ehvi_posterior and
        // k_gp_logpi_finish, nothing goes through a clamped variance.
        const bool passes = raw >= 0.0;
        const double var = (passes ? raw : 0.0) + stab_noise;
        const double sdev = sqrt(var);
        const double z = (mean - threshold) / sdev;
        const double logg = d_standard_logei(z);
        out_f[b] = 0.5 * log(var) + logg;
        if (out_grad) {
            double r_m, r_v;
            d_logei_weights(z, logg, &r_m, &r_v);
            s_wm = r_m / sdev;
            s_wv = passes ? r_v / (2.0 * var) : 0.0;
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
