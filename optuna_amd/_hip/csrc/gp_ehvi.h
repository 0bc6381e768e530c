// ---------------------------------------------------------------------------
// K5 (multi-objective): fused GP log-EHVI forward + gradient over M
// device-resident GPs, 2 <= M <= 4.
//
// Per candidate x and objective m the posterior is the one of gp_posterior.h
// (k_gp_cross_cov, a rocBLAS dgemm against the explicit inverse, then
// mean_m = K_m.alpha_m, var_m = max(scale_m - K_m.V_m, 0) + stab). With the
// fixed QMC normals eps (Q, M) and the non-dominated boxes lo / iv (J, M):
//   y[q,m]   = mean_m + sd_m * eps[q,m]
//   d[q,j,m] = min(max(y[q,m] - lo[j,m], EPS), iv[j,m])
//   t[q,j]   = sum_m log d[q,j,m]
//   f        = logsumexp_{q,j} t - log Q  =  log sum_{q,j} prod_m d[q,j,m] - log Q
// The box kernel streams the (q, j) pairs of a candidate through LDS: y sits
// there once, the boxes pass through fixed-size tiles, and nothing of size
// Q*J*M ever exists in memory.
//
// The sum is taken over the products themselves, not over their logs: every
// factor is >= EPS = 1e-12, so a product of M <= 4 factors is >= 1e-48 and
// cannot underflow, it is bounded by the spread of the (standardised)
// objectives to the power M, and a plain fp64 sum of such terms loses nothing
// a log-sum-exp would keep (both drop terms below 2^-53 of the total). That
// removes one log and one exp per pair, which measured as nine tenths of the
// kernel (docs/PERF.md).
//
// CLOSED FORM gradient: with S = sum prod and w[q,j] = prod[q,j] / S,
//   df/dy[q,m] = sum_j w[q,j] / d[q,j,m]             over unclamped (j, m)
//              = (1/S) sum_j prod_{m' != m} d[q,j,m']  over unclamped (j, m)
//   wm_m = sum_q df/dy[q,m]
//   wv_m = sum_q eps[q,m] df/dy[q,m] / (2 sd_m)   (0 where var_m was clamped)
// and the input gradient is the LogEI one summed over the objectives:
//   grad_d = sum_m 2 eta_md (x_d sum_i c_mi - sum_i c_mi X_id),
//   c_mi = (wm_m alpha_mi - 2 wv_m V_mi) * MP_mi,
// and exactly 0 on a categorical column (gp_posterior.h's cat_mask).
// All reductions run in a fixed order (wavefront shuffles, the four wavefronts
// through LDS, then the workgroups of a candidate in index order) and there
// are no floating-point atomics, so equal inputs in equal batches give equal
// bits.
// ---------------------------------------------------------------------------

#pragma once

#include "gp_feasibility.h"

constexpr int EHVI_MAX_M = 4;
// Boxes per LDS tile: the LDS footprint is fixed whatever J is.
constexpr int EHVI_BOX_TILE = 128;
// y and eps are staged whole: (2 * Q * M + 2 * M * tile) doubles of LDS stay
// under the 64 KiB a launch gets without opting in to more.
constexpr int EHVI_MAX_Q = 512;
constexpr double EHVI_EPS = 1e-12;  // the host's _EPS

// Posterior of objective m for every candidate of the chunk: the first half
// of k_gp_logei_final. dsd = d sd / d var, zero where the clamp was active.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_ehvi_posterior(const double* __restrict__ K,      // (B, N)
                    const double* __restrict__ V,      // (B, N) = K @ Cinv
                    const double* __restrict__ alpha,  // (N)
                    double scale, double stab_noise, int64_t N, int m, int M,
                    double* __restrict__ mean,    // (B, M)
                    double* __restrict__ sd,      // (B, M)
                    double* __restrict__ dsd) {   // (B, M)
    __shared__ double red[GP_WAVES];
    const int64_t b = blockIdx.x;
    const double* Kb = K + b * N;
    const double* Vb = V + b * N;
    double acc_m = 0.0, acc_v = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += GP_BLOCK) {
        const double k = Kb[i];
        acc_m += k * alpha[i];
        acc_v += k * Vb[i];
    }
    const double kmean = gp_block_sum(acc_m, red);
    const double kv = gp_block_sum(acc_v, red);
    if (threadIdx.x == 0) {
        const double raw = scale - kv;
        const bool passes = raw >= 0.0;  // clamp_min passes the gradient here
        const double s = sqrt((raw > 0.0 ? raw : 0.0) + stab_noise);
        mean[b * M + m] = kmean;
        sd[b * M + m] = s;
        dsd[b * M + m] = passes ? 0.5 / s : 0.0;
    }
}

// Words of one partial record: S = sum prod, and with the gradient
// a_m = sum prod_{m' != m} d (unclamped m only) and e_m = the same times eps.
constexpr int ehvi_words(int M, bool grad) { return grad ? 1 + 2 * M : 1; }

// Doubles of dynamic LDS the box kernel needs.
static size_t ehvi_lds_doubles(int M, int Q, bool grad) {
    return (size_t)Q * M * (grad ? 2 : 1) + 2 * (size_t)M * EHVI_BOX_TILE +
           (size_t)GP_WAVES * ehvi_words(M, grad);
}

// Workgroup (b, s) of a (B, S) grid sums the pairs of candidate b with the box
// tiles s, s + S, ... and writes one partial record. All LDS is one dynamic
// array:
//   ys (Q, M) | [eps (Q, M) with GRAD] | lo tile (M, TILE) | iv tile (M, TILE)
//   | GP_WAVES reduction records.
// The tiles are stored objective-major so that consecutive lanes, which hold
// consecutive boxes, read consecutive doubles.
template <int M, bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_logehvi(const double* __restrict__ mean,  // (B, M)
             const double* __restrict__ sd,    // (B, M)
             const double* __restrict__ eps,   // (Q, M)
             const double* __restrict__ lo,    // (J, M)
             const double* __restrict__ iv,    // (J, M)
             int Q, int J,
             double* __restrict__ part) {  // (B, S, W)
    constexpr int W = ehvi_words(M, GRAD);
    extern __shared__ double ehvi_lds[];
    double* ys = ehvi_lds;
    double* es = ys + (size_t)Q * M;  // used with GRAD only
    double* los = GRAD ? es + (size_t)Q * M : es;
    double* ivs = los + M * EHVI_BOX_TILE;
    double* red = ivs + M * EHVI_BOX_TILE;

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int S = gridDim.y;
    for (int i = tid; i < Q * M; i += GP_BLOCK) {
        const int m = i % M;
        const double ev = eps[i];
        ys[i] = mean[b * M + m] + sd[b * M + m] * ev;
        if constexpr (GRAD) es[i] = ev;
    }

    double acc[W] = {};  // S | a_0..a_{M-1} | e_0..e_{M-1}
    for (int64_t j0 = (int64_t)blockIdx.y * EHVI_BOX_TILE; j0 < J;
         j0 += (int64_t)S * EHVI_BOX_TILE) {
        const int cnt = (int)min((int64_t)EHVI_BOX_TILE, J - j0);
        __syncthreads();  // the previous tile is consumed (first pass: nothing)
        for (int i = tid; i < cnt * M; i += GP_BLOCK) {
            const int jj = i / M, m = i % M;
            los[m * EHVI_BOX_TILE + jj] = lo[j0 * M + i];
            ivs[m * EHVI_BOX_TILE + jj] = iv[j0 * M + i];
        }
        __syncthreads();  // tile (and, first pass, ys / es) visible

        // Pair p = q * cnt + jj, p = tid, tid + 256, ...; (q, jj) advance
        // without a division per pair.
        const int total = Q * cnt;
        const int dq = GP_BLOCK / cnt, dj = GP_BLOCK % cnt;
        int q = tid / cnt, jj = tid % cnt;
        for (int p = tid; p < total; p += GP_BLOCK) {
            double d[M];
            bool open[M];  // neither clamp active
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double diff = ys[q * M + m] - los[m * EHVI_BOX_TILE + jj];
                const double width = ivs[m * EHVI_BOX_TILE + jj];
                d[m] = fmin(fmax(diff, EHVI_EPS), width);
                open[m] = diff > EHVI_EPS && diff < width;
            }
            double prod = d[0];
#pragma unroll
            for (int m = 1; m < M; ++m) prod *= d[m];
            acc[0] += prod;
            if constexpr (GRAD) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    double others = 1.0;  // prod / d[m] without the division
#pragma unroll
                    for (int k = 0; k < M; ++k)
                        if (k != m) others *= d[k];
                    const double ga = open[m] ? others : 0.0;
                    acc[1 + m] += ga;
                    acc[1 + M + m] += ga * es[q * M + m];
                }
            }
            q += dq;
            jj += dj;
            if (jj >= cnt) {
                jj -= cnt;
                ++q;
            }
        }
    }

    // Wavefront tree by shuffles, then the wavefronts in order through LDS.
#pragma unroll
    for (int k = 0; k < W; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) red[(tid >> 6) * W + k] = acc[k];
    }
    __syncthreads();
    if (tid < W) {
        double out = red[tid];
        for (int w = 1; w < GP_WAVES; ++w) out += red[w * W + tid];
        part[(b * S + blockIdx.y) * W + tid] = out;
    }
}

// One thread per candidate: the S partial records in order, then the value
// and the posterior-side weights.
template <int M, bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_logehvi_finish(const double* __restrict__ part,  // (B, S, W)
                    const double* __restrict__ dsd,   // (B, M)
                    int S, int Q, int64_t B,
                    double* __restrict__ out_f,     // (B)
                    double* __restrict__ out_wm,    // (B, M), GRAD only
                    double* __restrict__ out_wv) {  // (B, M), GRAD only
    constexpr int W = ehvi_words(M, GRAD);
    const int64_t b = (int64_t)blockIdx.x * GP_BLOCK + threadIdx.x;
    if (b >= B) return;
    double acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = part[b * S * W + k];
    for (int s = 1; s < S; ++s) {
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += part[(b * S + s) * W + k];
    }
    out_f[b] = log(acc[0]) - log((double)Q);
    if constexpr (GRAD) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            out_wm[b * M + m] = acc[1 + m] / acc[0];
            out_wv[b * M + m] = acc[1 + M + m] / acc[0] * dsd[b * M + m];
        }
    }
}

// What the input-gradient kernel reads per objective.
struct EhviGradArgs {
    const double* X[EHVI_MAX_M];      // (N, D)
    const double* alpha[EHVI_MAX_M];  // (N)
    const double* eta[EHVI_MAX_M];    // (D)
    const double* MP[EHVI_MAX_M];     // (B, N)
    const double* V[EHVI_MAX_M];      // (B, N)
};

// Input gradient, one workgroup per candidate. Thread (g, d) = (tid / D,
// tid % D) owns dimension d over the observations i = g, g + G, ... with
// G = 256 / D groups, so X is read along its rows and nothing is indexed at
// run time in registers. The G partials of a dimension are summed in order.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_ehvi_grad(EhviGradArgs P, int M,
               const double* __restrict__ wm,  // (B, M)
               const double* __restrict__ wv,  // (B, M)
               const double* __restrict__ x,   // (B, D)
               int64_t N, int D, uint64_t cat_mask,
               double* __restrict__ out_grad) {  // (B, D)
    __shared__ double part[GP_BLOCK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int G = GP_BLOCK / D;
    const int g = tid / D, d = tid % D;
    double acc = 0.0;
    // A categorical column keeps acc = 0: its Hamming term does not move with x.
    if (g < G && !gp_is_cat(cat_mask, d)) {
        const double xd = x[b * D + d];
        for (int m = 0; m < M; ++m) {
            const double w_m = wm[b * M + m], w_v = wv[b * M + m];
            const double* alpha = P.alpha[m];
            const double* Xm = P.X[m];
            const double* MPb = P.MP[m] + b * N;
            const double* Vb = P.V[m] + b * N;
            double sum_c = 0.0, sum_cx = 0.0;
            for (int64_t i = g; i < N; i += G) {
                const double c = (w_m * alpha[i] - 2.0 * w_v * Vb[i]) * MPb[i];
                sum_c += c;
                sum_cx += c * Xm[i * D + d];
            }
            acc += 2.0 * P.eta[m][d] * (xd * sum_c - sum_cx);
        }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < D) {
        double out = part[tid];
        for (int k = 1; k < G; ++k) out += part[k * D + tid];
        out_grad[b * D + tid] = out;
    }
}

// Session over M torch-owned device GPs (raw pointers; same HIP context) and
// its own copies of the QMC normals and the boxes. Built once per acquisition
// function; evaluations upload only the (B, D) candidates.
class GpLogEhviSession {
  public:
    GpLogEhviSession(const std::vector<int64_t>& X_ptrs,
                     const std::vector<int64_t>& alpha_ptrs,
                     const std::vector<int64_t>& cinv_ptrs,
                     const std::vector<int64_t>& eta_ptrs,
                     const std::vector<double>& scales, int64_t N, int64_t D,
                     double stab_noise, const arr_f64& eps, const arr_f64& lo,
                     const arr_f64& iv, int64_t scratch_budget_bytes,
                     uint64_t cat_mask = 0)
        : N_(N), D_(D), stab_(stab_noise), budget_(scratch_budget_bytes) {
        M_ = gp_make_refs("GpLogEhviSession", X_ptrs, alpha_ptrs, cinv_ptrs, eta_ptrs,
                          scales, 2, EHVI_MAX_M, N, D, cat_mask, gp_);
        if (budget_ < 1) throw std::runtime_error("GpLogEhviSession: budget < 1");
        if (eps.ndim() != 2 || lo.ndim() != 2 || iv.ndim() != 2 ||
            eps.shape(1) != M_ || lo.shape(1) != M_ || iv.shape(1) != M_ ||
            lo.shape(0) != iv.shape(0))
            throw std::runtime_error("GpLogEhviSession: eps (Q, M), lo / iv (J, M)");
        Q_ = eps.shape(0);
        J_ = lo.shape(0);
        if (Q_ < 1 || Q_ > EHVI_MAX_Q)
            throw std::runtime_error("GpLogEhviSession: need 1 <= Q <= " +
                                     std::to_string(EHVI_MAX_Q));
        if (J_ < 1 || J_ > INT32_MAX / EHVI_MAX_M)
            throw std::runtime_error("GpLogEhviSession: box count out of range");
        const size_t nq = (size_t)Q_ * M_, nj = (size_t)J_ * M_;
        consts_.reserve(nq + 2 * nj);
        HIP_CHECK(hipMemcpy(consts_.ptr, eps.data(), nq * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(consts_.ptr + nq, lo.data(), nj * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(consts_.ptr + nq + nj, iv.data(), nj * 8,
                            hipMemcpyHostToDevice));
    }

    // Candidates per chunk. With the gradient every objective keeps its
    // K / MP / V set; without it one set is reused objective by objective.
    int64_t chunk_rows(bool with_grad) const {
        return gp_chunk_rows(budget_, N_, with_grad ? M_ : 1);
    }
    int64_t n_chunks(int64_t B, bool with_grad) const {
        return gp_n_chunks(B, chunk_rows(with_grad));
    }
    // Workgroups per candidate in the box kernel for a chunk of bc
    // candidates: at least one tile of boxes each.
    int box_splits(int64_t bc) const {
        return gp_splits(bc, (J_ + EHVI_BOX_TILE - 1) / EHVI_BOX_TILE);
    }

    // With a constraint set the feasibility term and its gradient are added
    // on the device, chunk by chunk in the first K / MP / V set once the
    // objectives are done with it, before the one copy back.
    py::tuple eval(const arr_f64& x, bool with_grad,
                   const GpConstraintSet* constraints = nullptr) {
        GpEvalIo io(x, D_, with_grad);
        if (constraints) constraints->check_shape(N_, D_, gp_[0].cat_mask);
        const int64_t B = io.B;
        if (B == 0) return io.download(nullptr, nullptr);

        const int64_t rows = std::min(chunk_rows(with_grad), B);
        const int n_sets = with_grad ? M_ : 1;
        const int W = ehvi_words(M_, with_grad);
        const size_t nK = (size_t)rows * N_, nBM = (size_t)B * M_,
                     nBD = (size_t)B * D_;
        WsLayout L;
        const auto s_x = L.add<double>(nBD), s_mean = L.add<double>(nBM),
                   s_sd = L.add<double>(nBM), s_dsd = L.add<double>(nBM),
                   s_f = L.add<double>(B),
                   s_part = L.add<double>(gp_part_records(rows) * W),
                   s_wm = L.add<double>(with_grad ? nBM : 0),
                   s_wv = L.add<double>(with_grad ? nBM : 0),
                   s_g = L.add<double>(with_grad ? nBD : 0),
                   s_K = L.add<double>(nK * n_sets),
                   s_MP = L.add<double>(nK * n_sets),
                   s_V = L.add<double>(nK * n_sets),
                   s_cpart = L.add<double>(
                       constraints ? constraints->part_doubles(rows, with_grad) : 0);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_x = s_x.in(base), *d_mean = s_mean.in(base),
               *d_sd = s_sd.in(base), *d_dsd = s_dsd.in(base),
               *d_f = s_f.in(base), *d_part = s_part.in(base),
               *d_wm = s_wm.in(base), *d_wv = s_wv.in(base),
               *d_g = s_g.in(base), *d_K = s_K.in(base), *d_MP = s_MP.in(base),
               *d_V = s_V.in(base), *d_cpart = s_cpart.in(base);
        hipStream_t st = io.upload(d_x);

        const size_t lds = ehvi_lds_doubles(M_, (int)Q_, with_grad) * 8;
        rocblas_handle blas = get_blas(st);
        for (int64_t b0 = 0; b0 < B; b0 += rows) {
            const int64_t bc = std::min(rows, B - b0);
            const double* xc = d_x + b0 * D_;
            EhviGradArgs ga{};
            for (int m = 0; m < M_; ++m) {
                const size_t set = with_grad ? (size_t)m * nK : 0;
                double *Km = d_K + set, *MPm = d_MP + set, *Vm = d_V + set;
                const GpRef& gp = gp_[m];
                gp_enqueue_kv(st, blas, gp, xc, bc, N_, D_, Km, MPm, Vm);
                hipLaunchKernelGGL(k_gp_ehvi_posterior, dim3((unsigned)bc),
                                   dim3(GP_BLOCK), 0, st, Km, Vm, gp.alpha,
                                   gp.scale, stab_, N_, m, M_, d_mean + b0 * M_,
                                   d_sd + b0 * M_, d_dsd + b0 * M_);
                ga.X[m] = gp.X;
                ga.alpha[m] = gp.alpha;
                ga.eta[m] = gp.eta;
                ga.MP[m] = MPm;
                ga.V[m] = Vm;
            }
            launch_boxes(with_grad, bc, lds, st, d_mean + b0 * M_, d_sd + b0 * M_,
                         d_dsd + b0 * M_, d_part, d_f + b0,
                         with_grad ? d_wm + b0 * M_ : nullptr,
                         with_grad ? d_wv + b0 * M_ : nullptr);
            if (with_grad)
                hipLaunchKernelGGL(k_gp_ehvi_grad, dim3((unsigned)bc),
                                   dim3(GP_BLOCK), 0, st, ga, M_,
                                   d_wm + b0 * M_, d_wv + b0 * M_, xc, N_,
                                   (int)D_, gp_[0].cat_mask, d_g + b0 * D_);
            if (constraints)
                constraints->enqueue(st, blas, xc, bc, with_grad, true, d_K, d_MP, d_V,
                                     d_cpart, d_f + b0,
                                     with_grad ? d_g + b0 * D_ : nullptr);
        }
        return io.download(d_f, d_g);
    }

  private:
    // The box kernel over a (bc, S) grid, then the per-candidate finish.
    template <int M, bool GRAD>
    void launch_boxes_as(int64_t bc, size_t lds, hipStream_t st,
                         const double* mean, const double* sd, const double* dsd,
                         double* part, double* f, double* wm, double* wv) {
        const double* eps = consts_.ptr;
        const double* lo = eps + (size_t)Q_ * M_;
        const double* iv = lo + (size_t)J_ * M_;
        const int S = box_splits(bc);
        hipLaunchKernelGGL((k_gp_logehvi<M, GRAD>),
                           dim3((unsigned)bc, (unsigned)S), dim3(GP_BLOCK), lds,
                           st, mean, sd, eps, lo, iv, (int)Q_, (int)J_, part);
        hipLaunchKernelGGL((k_gp_logehvi_finish<M, GRAD>),
                           dim3((unsigned)((bc + GP_BLOCK - 1) / GP_BLOCK)),
                           dim3(GP_BLOCK), 0, st, part, dsd, S, (int)Q_, bc, f,
                           wm, wv);
    }
    template <typename... A>
    void launch_boxes(bool grad, A... a) {
        switch (M_ * 2 + (grad ? 1 : 0)) {
            case 4: return launch_boxes_as<2, false>(a...);
            case 5: return launch_boxes_as<2, true>(a...);
            case 6: return launch_boxes_as<3, false>(a...);
            case 7: return launch_boxes_as<3, true>(a...);
            case 8: return launch_boxes_as<4, false>(a...);
            case 9: return launch_boxes_as<4, true>(a...);
        }
    }

    GpRef gp_[EHVI_MAX_M];
    int M_;
    int64_t N_, D_, Q_ = 0, J_ = 0;
    double stab_;
    int64_t budget_;
    DeviceBuffer<double> consts_;  // eps (Q, M) | lo (J, M) | iv (J, M)
};
