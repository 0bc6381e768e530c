// ---------------------------------------------------------------------------
// K5 (constraints): the feasibility term of the constrained acquisitions,
//   f(x) = sum_c log Phi(z_c(x)),  z_c = (mean_c(x) - t_c) / sd_c(x),
// and its input gradient over C device-resident constraint GPs,
// 1 <= C <= FEAS_MAX_C. Every constraint GP has the structure of an objective
// GP (same X, own eta / alpha / explicit inverse), so the posterior is the one
// of gp_posterior.h: k_gp_cross_cov, a rocBLAS dgemm against the inverse, then
//   mean = K.alpha,  raw = scale - K.V,  sd = sqrt(max(raw, 0) + stab).
//
// CLOSED FORM gradient: with rho = phi(z) / Phi(z),
//   w_m = df/dmean = rho / sd,
//   w_v = df/dvar  = -rho z / (2 sd^2)   (0 where the clamp on raw is active,
//                                         as autograd and k_gp_ehvi_posterior)
// and dK_i/dx_d = MP_i 2 eta_d (x_d - X_id),
//   grad_d = 2 eta_d (w_m A_d - 2 w_v Bv_d),
//   A_d  = sum_i alpha_i MP_i (x_d - X_id),
//   Bv_d = sum_i V_i     MP_i (x_d - X_id).
// A_d and Bv_d do not depend on the weights, so one pass over K / V / MP / X
// yields the posterior sums and the gradient sums together, and that pass can
// be split over S workgroups per candidate (a local-search step has about 10
// candidates). A finish kernel adds the S records in order and adds the result
// to whatever the objective term left in out_f / out_grad. On a categorical
// column (gp_posterior.h's cat_mask) the distance term does not move with x:
// A_d = Bv_d = 0, the walk skips it and the finish writes, or adds, exactly 0.
//
// All reductions run in a fixed order (wavefront shuffles, the wavefronts
// through LDS, the row groups of a dimension in order, the workgroups of a
// candidate in order, the constraints in order) and there are no
// floating-point atomics, so equal inputs in equal batches give equal bits.
// ---------------------------------------------------------------------------

#pragma once

#include "gp_posterior.h"

constexpr int FEAS_MAX_C = 16;

// log Phi(z) and rho = phi(z) / Phi(z) without cancellation in either tail.
// Left: Phi(z) = phi(z) sqrt(pi/2) erfcx(-z/sqrt 2), so rho needs no exp at
// all. Right: log1p of the (tiny) upper tail keeps the value's relative
// accuracy where log(1 - tiny) would round to zero too early.
__device__ __forceinline__ void d_logpi_terms(double z, double* log_phi_cdf,
                                              double* rho) {
    constexpr double INV_SQRT2 = 0.7071067811865476;
    constexpr double INV_SQRT_2PI = 0.3989422804014327;
    constexpr double SQRT_HALF_PI = 1.2533141373155003;
    if (z < 0.0) {
        const double e = erfcx(-z * INV_SQRT2);
        *log_phi_cdf = -0.5 * z * z + log(0.5 * e);
        *rho = 1.0 / (SQRT_HALF_PI * e);
    } else {
        const double upper = 0.5 * erfc(z * INV_SQRT2);
        *log_phi_cdf = log1p(-upper);
        *rho = exp(-0.5 * z * z) * INV_SQRT_2PI / (1.0 - upper);
    }
}

// Words of one partial record: K.alpha, K.V, and with the gradient A_0..A_{D-1}
// then Bv_0..Bv_{D-1}.
static int feas_words(int D, bool grad) { return grad ? 2 + 2 * D : 2; }

// Workgroup (b, s) of a (bc, S) grid walks the observations
// [s * ceil(N / S), (s + 1) * ceil(N / S)) of candidate b once and writes one
// partial record. With GRAD, thread (g, d) = (tid / D, tid % D) owns dimension
// d over the rows g, g + G, ... of the slice (G = 256 / D groups), so X is read
// along its rows and nothing is indexed at run time in registers; the d == 0
// thread of a group also carries the two posterior sums of its rows.
template <bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_logpi_partial(const double* __restrict__ K,      // (bc, N)
                   const double* __restrict__ MP,     // (bc, N)
                   const double* __restrict__ V,      // (bc, N) = K @ Cinv
                   const double* __restrict__ alpha,  // (N)
                   const double* __restrict__ X,      // (N, D)
                   const double* __restrict__ x,      // (bc, D)
                   int64_t N, int D, uint64_t cat_mask,
                   double* __restrict__ part) {  // (bc, S, W)
    __shared__ double red[GP_WAVES];
    __shared__ double part_a[GRAD ? GP_BLOCK : 1];
    __shared__ double part_b[GRAD ? GP_BLOCK : 1];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int S = gridDim.y;
    const int64_t per = (N + S - 1) / S;
    const int64_t i0 = min(N, (int64_t)blockIdx.y * per);
    const int64_t i1 = min(N, i0 + per);
    const int W = GRAD ? 2 + 2 * D : 2;
    const double* Kb = K + b * N;
    const double* Vb = V + b * N;
    double* rec = part + (b * S + blockIdx.y) * W;

    double acc_m = 0.0, acc_v = 0.0;
    if constexpr (!GRAD) {
        for (int64_t i = i0 + tid; i < i1; i += GP_BLOCK) {
            const double k = Kb[i];
            acc_m += k * alpha[i];
            acc_v += k * Vb[i];
        }
    } else {
        const int G = GP_BLOCK / D;
        const int g = tid / D, d = tid % D;
        double acc_a = 0.0, acc_b = 0.0;
        // A categorical column has A_d = Bv_d = 0: its threads sit the walk
        // out, but for the d == 0 one, which carries the posterior sums.
        const bool cat = gp_is_cat(cat_mask, d);
        if (g < G && (!cat || d == 0)) {
            const double* MPb = MP + b * N;
            const double xd = x[b * D + d];
            for (int64_t i = i0 + g; i < i1; i += G) {
                const double al = alpha[i], v = Vb[i];
                const double w = cat ? 0.0 : MPb[i] * (xd - X[i * D + d]);
                acc_a += al * w;
                acc_b += v * w;
                if (d == 0) {
                    const double k = Kb[i];
                    acc_m += k * al;
                    acc_v += k * v;
                }
            }
        }
        part_a[tid] = acc_a;
        part_b[tid] = acc_b;
    }
    // The barriers in here also publish part_a / part_b.
    const double kmean = gp_block_sum(acc_m, red);
    const double kv = gp_block_sum(acc_v, red);
    if (tid == 0) {
        rec[0] = kmean;
        rec[1] = kv;
    }
    if constexpr (GRAD) {
        if (tid < D) {
            const int G = GP_BLOCK / D;
            double a = part_a[tid], bv = part_b[tid];
            for (int k = 1; k < G; ++k) {
                a += part_a[k * D + tid];
                bv += part_b[k * D + tid];
            }
            rec[2 + tid] = a;
            rec[2 + D + tid] = bv;
        }
    }
}

// One thread per candidate (per (candidate, d) with GRAD): the S partial
// records in order, then log Phi(z) into out_f and the closed-form gradient
// into out_grad. `accumulate` = 0 writes the outputs (the first user of the
// buffers), 1 adds to them.
template <bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_logpi_finish(const double* __restrict__ part,  // (B, S, W)
                  const double* __restrict__ eta,   // (D)
                  double scale, double stab_noise, double threshold, int S,
                  int D, int64_t B, int accumulate, uint64_t cat_mask,
                  double* __restrict__ out_f,       // (B)
                  double* __restrict__ out_grad) {  // (B, D), GRAD only
    const int W = GRAD ? 2 + 2 * D : 2;
    const int64_t t = (int64_t)blockIdx.x * GP_BLOCK + threadIdx.x;
    const int64_t b = GRAD ? t / D : t;
    const int d = GRAD ? (int)(t % D) : 0;
    if (b >= B) return;
    const double* rec = part + b * S * W;
    double kmean = rec[0], kv = rec[1];
    for (int s = 1; s < S; ++s) {
        kmean += rec[s * W];
        kv += rec[s * W + 1];
    }
    const double raw = scale - kv;
    const bool passes = raw >= 0.0;  // clamp_min passes the gradient here
    const double sd = sqrt((raw > 0.0 ? raw : 0.0) + stab_noise);
    const double z = (kmean - threshold) / sd;
    double lp, rho;
    d_logpi_terms(z, &lp, &rho);
    if (d == 0) out_f[b] = accumulate ? out_f[b] + lp : lp;
    if constexpr (GRAD) {
        double a = rec[2 + d], bv = rec[2 + D + d];
        for (int s = 1; s < S; ++s) {
            a += rec[s * W + 2 + d];
            bv += rec[s * W + 2 + D + d];
        }
        const double w_m = rho / sd;
        const double w_v = passes ? -rho * z / (2.0 * sd * sd) : 0.0;
        const double gd = gp_is_cat(cat_mask, d)
                              ? 0.0
                              : 2.0 * eta[d] * (w_m * a - 2.0 * w_v * bv);
        out_grad[b * D + d] = accumulate ? out_grad[b * D + d] + gd : gd;
    }
}

// C torch-owned device constraint GPs (raw pointers; same HIP context) and
// their thresholds. Evaluated alone (the "no feasible trial yet" acquisitions)
// or handed to GpLogEiSession / GpLogEhviSession, which add its term to theirs
// on the device before their single copy back.
class GpConstraintSet {
  public:
    GpConstraintSet(const std::vector<int64_t>& X_ptrs,
                    const std::vector<int64_t>& alpha_ptrs,
                    const std::vector<int64_t>& cinv_ptrs,
                    const std::vector<int64_t>& eta_ptrs,
                    const std::vector<double>& scales,
                    const std::vector<double>& thresholds, int64_t N, int64_t D,
                    double stab_noise, int64_t scratch_budget_bytes,
                    uint64_t cat_mask = 0)
        : N_(N), D_(D), stab_(stab_noise), budget_(scratch_budget_bytes),
          cat_mask_(cat_mask) {
        C_ = gp_make_refs("GpConstraintSet", X_ptrs, alpha_ptrs, cinv_ptrs, eta_ptrs,
                          scales, 1, FEAS_MAX_C, N, D, cat_mask, gp_);
        if ((int)thresholds.size() != C_)
            throw std::runtime_error("GpConstraintSet: one threshold per constraint");
        if (N > INT32_MAX) throw std::runtime_error("GpConstraintSet: N out of range");
        if (budget_ < 1) throw std::runtime_error("GpConstraintSet: budget < 1");
        std::copy(thresholds.begin(), thresholds.end(), thr_);
    }

    // Throws unless a session over (N, D) and the categorical columns
    // `cat_mask` can hand its candidates to this set: another mask is another
    // search space.
    void check_shape(int64_t N, int64_t D, uint64_t cat_mask) const {
        if (N_ != N || D_ != D)
            throw std::runtime_error("eval: the constraint set was built for another (N, D)");
        if (cat_mask_ != cat_mask)
            throw std::runtime_error("eval: the constraint set was built for another cat_mask");
    }

    // Candidates per chunk of a stand-alone evaluation: one K / MP / V set,
    // reused constraint by constraint. The gradient needs no further
    // (rows, N) scratch.
    int64_t chunk_rows() const { return gp_chunk_rows(budget_, N_, 1); }
    int64_t n_chunks(int64_t B, bool /*with_grad*/) const {
        return gp_n_chunks(B, chunk_rows());
    }
    // Workgroups per candidate in the partial kernel for a chunk of bc
    // candidates: at least one block's worth of observations each.
    int n_splits(int64_t bc) const {
        return gp_splits(bc, (N_ + GP_BLOCK - 1) / GP_BLOCK);
    }
    // Doubles of partial records for chunks of at most `rows` candidates.
    size_t part_doubles(int64_t rows, bool with_grad) const {
        return gp_part_records(rows) * feas_words((int)D_, with_grad);
    }

    // Enqueue the term for the bc candidates xc: K / MP / V are (bc, N)
    // scratch that the caller no longer needs, f (bc) and g (bc, D) are
    // written by the first constraint when `accumulate` is false and added to
    // otherwise.
    void enqueue(hipStream_t st, rocblas_handle blas, const double* xc, int64_t bc,
                 bool with_grad, bool accumulate, double* K, double* MP, double* V,
                 double* part, double* f, double* g) const {
        const int S = n_splits(bc);
        const int D = (int)D_;
        for (int c = 0; c < C_; ++c) {
            const GpRef& gp = gp_[c];
            gp_enqueue_kv(st, blas, gp, xc, bc, N_, D_, K, MP, V);
            const int acc = (accumulate || c > 0) ? 1 : 0;
            const dim3 pgrid((unsigned)bc, (unsigned)S);
            if (with_grad) {
                hipLaunchKernelGGL(k_gp_logpi_partial<true>, pgrid, dim3(GP_BLOCK),
                                   0, st, K, MP, V, gp.alpha, gp.X, xc, N_, D, cat_mask_,
                                   part);
                hipLaunchKernelGGL(
                    k_gp_logpi_finish<true>,
                    dim3((unsigned)((bc * D + GP_BLOCK - 1) / GP_BLOCK)),
                    dim3(GP_BLOCK), 0, st, part, gp.eta, gp.scale, stab_, thr_[c], S,
                    D, bc, acc, cat_mask_, f, g);
            } else {
                hipLaunchKernelGGL(k_gp_logpi_partial<false>, pgrid, dim3(GP_BLOCK),
                                   0, st, K, MP, V, gp.alpha, gp.X, xc, N_, D, cat_mask_,
                                   part);
                hipLaunchKernelGGL(
                    k_gp_logpi_finish<false>,
                    dim3((unsigned)((bc + GP_BLOCK - 1) / GP_BLOCK)),
                    dim3(GP_BLOCK), 0, st, part, gp.eta, gp.scale, stab_, thr_[c], S,
                    D, bc, acc, cat_mask_, f, g);
            }
        }
    }

    py::tuple eval(const arr_f64& x, bool with_grad) const {
        GpEvalIo io(x, D_, with_grad);
        const int64_t B = io.B;
        if (B == 0) return io.download(nullptr, nullptr);

        const int64_t rows = std::min(chunk_rows(), B);
        const size_t nK = (size_t)rows * N_, nBD = (size_t)B * D_;
        WsLayout L;
        const auto s_x = L.add<double>(nBD), s_f = L.add<double>(B),
                   s_g = L.add<double>(with_grad ? nBD : 0),
                   s_part = L.add<double>(part_doubles(rows, with_grad)),
                   s_K = L.add<double>(nK), s_MP = L.add<double>(nK),
                   s_V = L.add<double>(nK);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_x = s_x.in(base), *d_f = s_f.in(base), *d_g = s_g.in(base),
               *d_part = s_part.in(base), *d_K = s_K.in(base),
               *d_MP = s_MP.in(base), *d_V = s_V.in(base);
        hipStream_t st = io.upload(d_x);
        rocblas_handle blas = get_blas(st);
        for (int64_t b0 = 0; b0 < B; b0 += rows) {
            const int64_t bc = std::min(rows, B - b0);
            enqueue(st, blas, d_x + b0 * D_, bc, with_grad, false, d_K, d_MP, d_V,
                    d_part, d_f + b0, with_grad ? d_g + b0 * D_ : nullptr);
        }
        return io.download(d_f, d_g);
    }

  private:
    GpRef gp_[FEAS_MAX_C];
    double thr_[FEAS_MAX_C];
    int C_;
    int64_t N_, D_;
    double stab_;
    int64_t budget_;
    uint64_t cat_mask_;
};
