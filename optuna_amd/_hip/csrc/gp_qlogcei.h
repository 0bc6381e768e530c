// ---------------------------------------------------------------------------
// K5 (constraints, running trials): fused GP qLogCEI forward + gradient over
// G = [objective] + C device-resident GPs, 0 <= C <= FEAS_MAX_C, G >= 1, each
// conditioned on its own QMC fantasies at the same R running points,
// 1 <= R <= QLOGEI_MAX_R, with 1 <= Q <= QLOGEI_MAX_Q draws. Without an
// objective (no feasible trial yet) the G GPs are the C constraints.
//
// Fixed for the life of the acquisition, per GP g: what gp_qlogehvi.h takes
// per objective (the base GP, Vr_g, L_g, W_g), a threshold t_g, the QMC normals
// z (Q, G) of the candidate column and F (Q), the best utility among the R
// fantasy columns of draw q, which does not move with the candidate.
//
// Per candidate x and GP g, s[q,g] as in gp_qlogehvi.h; then, with the
// objective at g = 0 and v[q,c] = (s[q,c] - t_c) / tau,
//   u_q = log max(s[q,0] - t_0, EPS) + sum_c logsigmoid(v[q,c])
//   f   = logsumexp_q max(F_q, u_q) - log Q
// The sum over the draws is taken in the log domain (block max, then the sum
// of exp): u_q of -1e3 and below is ordinary here, v reaches +-1e4.
//
// CLOSED FORM gradient: with w_q = exp(max(F_q, u_q) - lse) where u_q > F_q and
// 0 elsewhere,
//   a[q,0] = w_q / (s[q,0] - t_0)               (0 where s - t <= EPS)
//   a[q,c] = w_q sigmoid(-v[q,c]) / tau
//   wm_g  = sum_q a[q,g]
//   wv'_g = sum_q a[q,g] z[q,g] / (2 sd_g)      (0 where cv_raw_g <= 0)
//   wv_g  = wv'_g                               (0 where raw_g < 0)
//   u[r,g] = sum_q a[q,g] W_g[r, q] - 2 wv'_g p_g[r]
// and the input gradient is gp_qlogei.h's, summed over the G GPs, times
// 2 eta_gd, exactly 0 on a categorical column.
//
// Every per-GP stage is ONE launch for all G GPs: a grid dimension runs over
// the GP and the kernels read the pointers and scalars of their GP from a
// device table uploaded at construction; the three GEMMs are one
// rocblas_dgemm_batched each. Launches plus rocBLAS calls per chunk of
// candidates, whatever C is:
//   value (7):      k_gp_cross_cov_gps against X, k_gp_cross_cov_gps against
//                   Xr, dgemm_batched K Cinv, dgemm_batched K Vr,
//                   k_gp_kv_partial_gps, k_gp_qcei_cond, k_gp_qlogcei_reduce
//   gradient (+3):  dgemm_batched u Vr^T into the regions K held,
//                   k_gp_qcei_grad_gps, k_gp_qlogcei_grad_finish
// The batched launches need the K / MP / V sets of all G GPs at once, with or
// without the gradient. Every record has one writer, all reductions run in a
// fixed order and there are no floating-point atomics: equal inputs in equal
// batches give equal bits.
// ---------------------------------------------------------------------------

#pragma once

#include <cmath>

#include "gp_qlogehvi.h"

// One GP of the session, as the GP-batched kernels read it.
struct QCeiGp {
    const double *X, *alpha, *cinv, *eta;  // GpRef
    const double *Vr, *L, *W;              // (N, R) column-major, (R, R), (R, Q)
    double scale, thr;
};

// ---- the per-GP stages, GP g = the grid's last dimension -----------------

// Grid (ceil(n / GP_BLOCK), bc, G): k_gp_cross_cov of GP g against its own X
// (Xr == nullptr, n = N) or against the shared running rows (n = R), into set
// g of K / MP.
template <bool MIXED>
__global__ void k_gp_cross_cov_gps(const QCeiGp* __restrict__ gps,
                                   const double* __restrict__ Xr,  // (n, D) or null
                                   const double* __restrict__ x,   // (bc, D)
                                   int64_t n, int64_t D, size_t set_stride,
                                   double* __restrict__ K,    // (G, .): (bc, n)
                                   double* __restrict__ MP,   // (G, .): (bc, n)
                                   uint64_t cat_mask) {
    const QCeiGp& gp = gps[blockIdx.z];
    gp_cross_cov_body<MIXED>(Xr != nullptr ? Xr : gp.X, gp.eta, gp.scale, x, n, D,
                             K + blockIdx.z * set_stride, MP + blockIdx.z * set_stride,
                             cat_mask);
}

// Grid (bc, S, G): the (K.alpha, K.V) records of GP g, set g of part.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_kv_partial_gps(const QCeiGp* __restrict__ gps,
                    const double* __restrict__ K,  // (G, .): (bc, N)
                    const double* __restrict__ V,  // (G, .): (bc, N)
                    const double* __restrict__ x,  // (bc, D)
                    int64_t N, int D, size_t set_stride, size_t part_stride,
                    uint64_t cat_mask,
                    double* __restrict__ part) {  // (G, .): (bc, S, 2)
    const QCeiGp& gp = gps[blockIdx.z];
    const size_t at = blockIdx.z * set_stride;
    gp_logpi_partial_body<false>(K + at, nullptr, V + at, gp.alpha, gp.X, x, N, D,
                                 cat_mask, part + blockIdx.z * part_stride);
}

// Grid (bc, G): the conditioning of candidate b under GP g, s[b, q, g] for
// every draw and, with GRAD, p and post of set g.
template <bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qcei_cond(const QCeiGp* __restrict__ gps,
               const double* __restrict__ part,  // (G, .): (bc, S, 2)
               const double* __restrict__ Kr,    // (G, ld, R)
               const double* __restrict__ KVr,   // (G, ld, R)
               const double* __restrict__ z,     // (Q, G)
               double stab_noise, int S, int R, int Q, int64_t ld,
               size_t part_stride,
               double* __restrict__ out_s,       // (bc, Q, G)
               double* __restrict__ out_p,       // (G, ld, R), GRAD only
               double* __restrict__ out_post) {  // (G, ld, 3), GRAD only
    const int g = blockIdx.y, G = gridDim.y;
    const QCeiGp& gp = gps[g];
    const size_t r_at = (size_t)g * ld * R;
    qehvi_cond_body<GRAD>(part + g * part_stride, Kr + r_at, KVr + r_at, gp.L, gp.W, z,
                          gp.scale, stab_noise, S, R, Q, g, G, out_s,
                          GRAD ? out_p + r_at : nullptr,
                          GRAD ? out_post + (size_t)g * ld * 3 : nullptr);
}

// Grid (bc, S, G): k_gp_qlogei_grad of GP g into record set g.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qcei_grad_gps(const QCeiGp* __restrict__ gps,
                   const double* __restrict__ UV,   // (G, .): (bc, N), where K was
                   const double* __restrict__ MP,   // (G, .): (bc, N)
                   const double* __restrict__ V,    // (G, .): (bc, N)
                   const double* __restrict__ x,    // (bc, D)
                   const double* __restrict__ wm,   // (G, ld)
                   const double* __restrict__ wv,   // (G, ld)
                   const double* __restrict__ u,    // (G, ld, R)
                   const double* __restrict__ MPr,  // (G, ld, R)
                   const double* __restrict__ Xr,   // (R, D)
                   int64_t N, int D, int R, int64_t ld, size_t set_stride,
                   size_t part_stride, uint64_t cat_mask,
                   double* __restrict__ part) {  // (G, .): (bc, S, D)
    const int g = blockIdx.z;
    const QCeiGp& gp = gps[g];
    const size_t at = g * set_stride, r_at = (size_t)g * ld * R;
    qlogei_grad_body(UV + at, MP + at, V + at, gp.alpha, gp.X, x, wm + (size_t)g * ld,
                     wv + (size_t)g * ld, u + r_at, MPr + r_at, Xr, N, D, R, cat_mask,
                     part + g * part_stride);
}

// ---- the reduction over the draws ------------------------------------------

// logsigmoid(v) and sigmoid(-v), its derivative, for |v| up to 1e4 and beyond:
// exp only ever sees a non-positive argument.
__device__ __forceinline__ double qcei_logsigmoid(double v) {
    return v >= 0.0 ? -log1p(exp(-v)) : v - log1p(exp(v));
}
__device__ __forceinline__ double qcei_sigmoid_neg(double v) {
    if (v >= 0.0) {
        const double e = exp(-v);
        return e / (1.0 + e);
    }
    return 1.0 / (1.0 + exp(v));
}

// Max over the block, seen by every thread. `red` holds GP_WAVES doubles.
__device__ __forceinline__ double qcei_block_max(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
    __syncthreads();  // the previous user of `red` is done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double out = red[0];
    for (int w = 1; w < GP_WAVES; ++w) out = fmax(out, red[w]);
    return out;
}

// Bytes of dynamic LDS of k_gp_qlogcei_reduce: GP_WAVES sums | max(F, u), then
// w (Q) | with the gradient a[., g] (Q) | sum_q a W_g[r, .] (R). (bc, Q, G)
// itself never sits in LDS.
static size_t qcei_reduce_lds_bytes(int R, int Q, bool grad) {
    return (GP_WAVES + (size_t)Q + (grad ? (size_t)Q + R : 0)) * 8;
}

// One workgroup per candidate, thread tid owning the draws tid, tid + 256, ...
// from the first line to the last, so its slots of the two (Q) arrays in LDS
// need no barrier until another thread reads them. The G values s[b, q, :] of a
// draw are contiguous. Value: u_q, max(F_q, u_q) into LDS, the block max, the
// in-order block sum of exp. Gradient: w_q over the max in LDS, then one GP at
// a time a[., g] into LDS, wm_g and sum a z by gp_block_sum, and the R sums
// sum_q a[q,g] W_g[r, q] split over the wavefronts, row r = w, w + 4, ..., a
// wavefront reading 64 consecutive q of a row of W_g per step.
template <bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogcei_reduce(const QCeiGp* __restrict__ gps,
                    const double* __restrict__ s,     // (bc, Q, G)
                    const double* __restrict__ z,     // (Q, G)
                    const double* __restrict__ F,     // (Q)
                    const double* __restrict__ p,     // (G, ld, R), GRAD only
                    const double* __restrict__ post,  // (G, ld, 3), GRAD only
                    int G, int n_obj, double tau, int R, int Q, int64_t ld,
                    double* __restrict__ out_f,    // (bc)
                    double* __restrict__ out_wm,   // (G, ld), GRAD only
                    double* __restrict__ out_wv,   // (G, ld), GRAD only
                    double* __restrict__ out_u) {  // (G, ld, R), GRAD only
    extern __shared__ double qcei_lds[];
    double* red = qcei_lds;
    double* ws = red + GP_WAVES;  // (Q)
    double* as = ws + Q;          // (Q), GRAD only
    double* sw = as + Q;          // (R), GRAD only

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* sb = s + b * Q * G;

    double vmax = -INFINITY;
    for (int q = tid; q < Q; q += GP_BLOCK) {
        const double* sq = sb + (size_t)q * G;
        double u = 0.0;
        for (int g = 0; g < G; ++g) {
            const double d = sq[g] - gps[g].thr;
            u += g < n_obj ? log(fmax(d, QLOGEI_EPS)) : qcei_logsigmoid(d / tau);
        }
        const double v = fmax(F[q], u);
        ws[q] = v;
        vmax = fmax(vmax, v);
    }
    vmax = qcei_block_max(vmax, red);
    double acc = 0.0;
    for (int q = tid; q < Q; q += GP_BLOCK) acc += exp(ws[q] - vmax);
    const double lse = vmax + log(gp_block_sum(acc, red));
    if (tid == 0) out_f[b] = lse - log((double)Q);

    if constexpr (GRAD) {
        // The candidate column wins the draw where the max went above F_q.
        for (int q = tid; q < Q; q += GP_BLOCK) {
            const double v = ws[q];
            ws[q] = v > F[q] ? exp(v - lse) : 0.0;
        }
        const int lane = tid & 63;
        for (int g = 0; g < G; ++g) {
            const double thr = gps[g].thr;
            const double* Wg = gps[g].W;
            double acc_a = 0.0, acc_z = 0.0;
            for (int q = tid; q < Q; q += GP_BLOCK) {
                const double d = sb[(size_t)q * G + g] - thr;
                double a;
                if (g < n_obj)
                    a = d > QLOGEI_EPS ? ws[q] / d : 0.0;
                else
                    a = ws[q] * qcei_sigmoid_neg(d / tau) / tau;
                as[q] = a;
                acc_a += a;
                acc_z += a * z[(size_t)q * G + g];
            }
            // The barriers in here also publish `as`.
            const double a_sum = gp_block_sum(acc_a, red);
            const double z_sum = gp_block_sum(acc_z, red);
            const size_t at = (size_t)g * ld + b;
            const double* pm = post + at * 3;  // sd, [cv_raw > 0], [raw >= 0]
            const double wvp = pm[1] != 0.0 ? z_sum / (2.0 * pm[0]) : 0.0;
            if (tid == 0) {
                out_wm[at] = a_sum;
                out_wv[at] = pm[2] != 0.0 ? wvp : 0.0;
            }
            for (int r = tid >> 6; r < R; r += GP_WAVES) {
                const double* Wr = Wg + (size_t)r * Q;
                double a = 0.0;
                for (int q = lane; q < Q; q += 64) a += as[q] * Wr[q];
                for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
                if (lane == 0) sw[r] = a;
            }
            __syncthreads();
            if (tid < R) out_u[at * R + tid] = sw[tid] - 2.0 * wvp * p[at * R + tid];
            __syncthreads();  // `as` and `sw` are free for the next GP
        }
    }
}

// One thread per (candidate, d): the G record sets of k_gp_qcei_grad_gps, GP
// first, then the S records of it in order, each GP times 2 eta_gd; exactly
// 0.0 on a categorical column.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogcei_grad_finish(const QCeiGp* __restrict__ gps,
                         const double* __restrict__ part,  // (G, .): (bc, S, D)
                         size_t part_stride, int G, int S, int D, int64_t B,
                         uint64_t cat_mask,
                         double* __restrict__ out_grad) {  // (bc, D)
    const int64_t t = (int64_t)blockIdx.x * GP_BLOCK + threadIdx.x;
    const int64_t b = t / D;
    const int d = (int)(t % D);
    if (b >= B) return;
    double out = 0.0;
    for (int g = 0; g < G; ++g) {
        const double* r = part + g * part_stride + b * S * D;
        double a = r[d];
        for (int s = 1; s < S; ++s) a += r[s * D + d];
        out += 2.0 * gps[g].eta[d] * a;
    }
    out_grad[b * D + d] = gp_is_cat(cat_mask, d) ? 0.0 : out;
}

// Session over G torch-owned device GPs and the torch-owned tensors of their
// conditioning on the running trials (raw pointers; same HIP context), with its
// own copies of the QMC normals, the fantasies' best utilities and the per-GP
// table. Built once per acquisition function; evaluations upload the (B, D)
// candidates and the 6 G scratch pointers of the batched GEMMs.
class GpQLogCeiSession {
  public:
    static constexpr int MAX_G = FEAS_MAX_C + 1;

    GpQLogCeiSession(const std::vector<int64_t>& X_ptrs,
                     const std::vector<int64_t>& alpha_ptrs,
                     const std::vector<int64_t>& cinv_ptrs,
                     const std::vector<int64_t>& eta_ptrs,
                     const std::vector<double>& scales, int64_t N, int64_t D,
                     double stab_noise, int64_t Xr_ptr,
                     const std::vector<int64_t>& Vr_ptrs,
                     const std::vector<int64_t>& L_ptrs,
                     const std::vector<int64_t>& W_ptrs, int64_t R,
                     const std::vector<double>& thresholds, bool has_objective,
                     const arr_f64& z, const arr_f64& F, double tau,
                     int64_t scratch_budget_bytes, uint64_t cat_mask = 0)
        : n_obj_(has_objective ? 1 : 0), N_(N), D_(D), R_(R), stab_(stab_noise),
          tau_(tau), budget_(scratch_budget_bytes), cat_mask_(cat_mask),
          Xr_(reinterpret_cast<const double*>(Xr_ptr)) {
        const std::string who = "GpQLogCeiSession";
        GpRef refs[MAX_G];
        G_ = gp_make_refs(who, X_ptrs, alpha_ptrs, cinv_ptrs, eta_ptrs, scales, 1,
                          FEAS_MAX_C + n_obj_, N, D, cat_mask, refs);
        const size_t G = (size_t)G_;
        if (Vr_ptrs.size() != G || L_ptrs.size() != G || W_ptrs.size() != G ||
            thresholds.size() != G)
            throw std::runtime_error(who + ": one Vr, L, W pointer and threshold per GP");
        if (N > INT32_MAX) throw std::runtime_error(who + ": N out of range");
        if (budget_ < 1) throw std::runtime_error(who + ": budget < 1");
        if (!(tau > 0.0)) throw std::runtime_error(who + ": tau <= 0");
        if (R < 1 || R > QLOGEI_MAX_R)
            throw std::runtime_error(who + ": need 1 <= R <= " +
                                     std::to_string(QLOGEI_MAX_R));
        if (z.ndim() != 2 || z.shape(1) != G_ || F.ndim() != 1 ||
            F.shape(0) != z.shape(0))
            throw std::runtime_error(who + ": z (Q, G), F (Q)");
        Q_ = z.shape(0);
        if (Q_ < 1 || Q_ > QLOGEI_MAX_Q)
            throw std::runtime_error(who + ": need 1 <= Q <= " +
                                     std::to_string(QLOGEI_MAX_Q));
        for (size_t g = 0; g < G; ++g) {
            host_[g] = QCeiGp{refs[g].X, refs[g].alpha, refs[g].cinv, refs[g].eta,
                              reinterpret_cast<const double*>(Vr_ptrs[g]),
                              reinterpret_cast<const double*>(L_ptrs[g]),
                              reinterpret_cast<const double*>(W_ptrs[g]),
                              refs[g].scale, thresholds[g]};
        }
        table_.reserve(G);
        HIP_CHECK(hipMemcpy(table_.ptr, host_, G * sizeof(QCeiGp),
                            hipMemcpyHostToDevice));
        const size_t nz = (size_t)Q_ * G;
        consts_.reserve(nz + (size_t)Q_);
        HIP_CHECK(hipMemcpy(consts_.ptr, z.data(), nz * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(consts_.ptr + nz, F.data(), Q_ * 8, hipMemcpyHostToDevice));
    }

    // Candidates per chunk: G sets of K / MP / V either way (the batched
    // launches hold all of them at once; K takes u Vr^T once the value pass is
    // done with it), and per candidate of a chunk s (Q, G), per GP Kr, MPr, KVr
    // and the (K.alpha, K.V) record, with the gradient per GP also p, u, post,
    // wm, wv and a record of D words. Left out, as in gp_qlogehvi.h: the 1024
    // records that gp_part_records adds whatever the chunk, and x, f, g of the
    // whole batch.
    int64_t row_doubles(bool with_grad) const {
        const int64_t G = G_;
        return G * (Q_ + 3 * R_ + 2) + (with_grad ? G * (2 * R_ + 5 + D_) : 0);
    }
    int64_t chunk_rows(bool with_grad) const {
        return gp_chunk_rows_with(budget_, N_, G_, row_doubles(with_grad));
    }
    int64_t n_chunks(int64_t B, bool with_grad) const {
        return gp_n_chunks(B, chunk_rows(with_grad));
    }
    // Workgroups per candidate and GP in the two N-walks for a chunk of bc
    // candidates: at least one block's worth of observations each.
    int n_splits(int64_t bc) const {
        return gp_splits(bc, (N_ + GP_BLOCK - 1) / GP_BLOCK);
    }

    py::tuple eval(const arr_f64& x, bool with_grad) {
        GpEvalIo io(x, D_, with_grad);
        const int64_t B = io.B;
        if (B == 0) return io.download(nullptr, nullptr);

        const int64_t rows = std::min(chunk_rows(with_grad), B);
        const int D = (int)D_, R = (int)R_, Q = (int)Q_, G = G_;
        const size_t nK = (size_t)rows * N_, nR = (size_t)rows * R_,
                     nBD = (size_t)B * D_, n_part = gp_part_records(rows) * 2,
                     n_gpart = gp_part_records(rows) * D_;
        const size_t gG = with_grad ? (size_t)G : 0;
        WsLayout lay;
        const auto s_x = lay.add<double>(nBD), s_f = lay.add<double>(B),
                   s_g = lay.add<double>(with_grad ? nBD : 0),
                   s_part = lay.add<double>(G * n_part),
                   s_gpart = lay.add<double>(gG * n_gpart),
                   s_Kr = lay.add<double>(G * nR), s_MPr = lay.add<double>(G * nR),
                   s_KVr = lay.add<double>(G * nR),
                   s_s = lay.add<double>((size_t)rows * Q_ * G),
                   s_p = lay.add<double>(gG * nR), s_u = lay.add<double>(gG * nR),
                   s_post = lay.add<double>(gG * rows * 3),
                   s_wm = lay.add<double>(gG * rows), s_wv = lay.add<double>(gG * rows),
                   s_K = lay.add<double>(G * nK), s_MP = lay.add<double>(G * nK),
                   s_V = lay.add<double>(G * nK);
        const auto s_ptrs = lay.add<double*>(6 * (size_t)G);
        char* base = g_ws.ensure_bytes(lay.bytes());
        double *d_x = s_x.in(base), *d_f = s_f.in(base), *d_g = s_g.in(base),
               *d_part = s_part.in(base), *d_gpart = s_gpart.in(base),
               *d_Kr = s_Kr.in(base), *d_MPr = s_MPr.in(base),
               *d_KVr = s_KVr.in(base), *d_s = s_s.in(base), *d_p = s_p.in(base),
               *d_u = s_u.in(base), *d_post = s_post.in(base), *d_wm = s_wm.in(base),
               *d_wv = s_wv.in(base), *d_K = s_K.in(base), *d_MP = s_MP.in(base),
               *d_V = s_V.in(base);
        double** d_ptrs = s_ptrs.in(base);
        hipStream_t st = io.upload(d_x);
        rocblas_handle blas = get_blas(st);

        // The operand lists of the three batched GEMMs: Cinv | Vr | K | V | KVr
        // | u, G pointers each. The scratch regions keep their place from chunk
        // to chunk, so one upload serves the evaluation.
        const double* ptrs[6 * MAX_G];
        for (int g = 0; g < G; ++g) {
            ptrs[g] = host_[g].cinv;
            ptrs[G + g] = host_[g].Vr;
            ptrs[2 * G + g] = d_K + (size_t)g * nK;
            ptrs[3 * G + g] = d_V + (size_t)g * nK;
            ptrs[4 * G + g] = d_KVr + (size_t)g * nR;
            ptrs[5 * G + g] = d_u + (size_t)g * nR;
        }
        g_ws.h2d(d_ptrs, ptrs, 6 * (size_t)G * sizeof(double*), st);
        const double* const* p_cinv = d_ptrs;
        const double* const* p_Vr = d_ptrs + G;
        double* const* p_K = d_ptrs + 2 * G;
        double* const* p_V = d_ptrs + 3 * G;
        double* const* p_KVr = d_ptrs + 4 * G;
        const double* const* p_u = d_ptrs + 5 * G;

        const QCeiGp* gps = table_.ptr;
        const double* z = consts_.ptr;
        const double* F = z + (size_t)Q_ * G;
        const size_t cond_lds = qehvi_cond_lds_doubles(R) * 8;
        const size_t red_lds = qcei_reduce_lds_bytes(R, Q, with_grad);
        const bool mixed = cat_mask_ != 0;
        const double one = 1.0, zero = 0.0;
        for (int64_t b0 = 0; b0 < B; b0 += rows) {
            const int64_t bc = std::min(rows, B - b0);
            const double* xc = d_x + b0 * D_;
            const int S = n_splits(bc);
            const dim3 block(GP_BLOCK);
            const dim3 pgrid((unsigned)bc, (unsigned)S, (unsigned)G);
            // K, MP (G, bc, N) against each GP's X; Kr, MPr (G, bc, R) against Xr.
            const dim3 kgrid((unsigned)((N_ + GP_BLOCK - 1) / GP_BLOCK), (unsigned)bc,
                             (unsigned)G);
            const dim3 rgrid((unsigned)((R_ + GP_BLOCK - 1) / GP_BLOCK), (unsigned)bc,
                             (unsigned)G);
            if (mixed) {
                hipLaunchKernelGGL(k_gp_cross_cov_gps<true>, kgrid, block, 0, st, gps,
                                   (const double*)nullptr, xc, N_, D_, nK, d_K, d_MP,
                                   cat_mask_);
                hipLaunchKernelGGL(k_gp_cross_cov_gps<true>, rgrid, block, 0, st, gps,
                                   Xr_, xc, R_, D_, nR, d_Kr, d_MPr, cat_mask_);
            } else {
                hipLaunchKernelGGL(k_gp_cross_cov_gps<false>, kgrid, block, 0, st, gps,
                                   (const double*)nullptr, xc, N_, D_, nK, d_K, d_MP,
                                   cat_mask_);
                hipLaunchKernelGGL(k_gp_cross_cov_gps<false>, rgrid, block, 0, st, gps,
                                   Xr_, xc, R_, D_, nR, d_Kr, d_MPr, cat_mask_);
            }
            // V_g (bc, N) = K_g @ Cinv_g as in gp_enqueue_kv, and
            // KVr_g (bc, R) = K_g @ Vr_g: KVr^T (R, bc) = Vr^T @ K^T.
            ROCBLAS_CHECK(rocblas_dgemm_batched(
                blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)N_,
                (rocblas_int)bc, (rocblas_int)N_, &one, p_cinv, (rocblas_int)N_, p_K,
                (rocblas_int)N_, &zero, p_V, (rocblas_int)N_, G));
            ROCBLAS_CHECK(rocblas_dgemm_batched(
                blas, rocblas_operation_transpose, rocblas_operation_none,
                (rocblas_int)R_, (rocblas_int)bc, (rocblas_int)N_, &one, p_Vr,
                (rocblas_int)N_, p_K, (rocblas_int)N_, &zero, p_KVr, (rocblas_int)R_,
                G));
            hipLaunchKernelGGL(k_gp_kv_partial_gps, pgrid, block, 0, st, gps, d_K, d_V,
                               xc, N_, D, nK, n_part, cat_mask_, d_part);
            const dim3 cgrid((unsigned)bc, (unsigned)G);
            if (!with_grad) {
                hipLaunchKernelGGL(k_gp_qcei_cond<false>, cgrid, block, cond_lds, st,
                                   gps, d_part, d_Kr, d_KVr, z, stab_, S, R, Q, rows,
                                   n_part, d_s, (double*)nullptr, (double*)nullptr);
                hipLaunchKernelGGL(k_gp_qlogcei_reduce<false>, dim3((unsigned)bc), block,
                                   red_lds, st, gps, d_s, z, F, (const double*)nullptr,
                                   (const double*)nullptr, G, n_obj_, tau_, R, Q, rows,
                                   d_f + b0, (double*)nullptr, (double*)nullptr,
                                   (double*)nullptr);
                continue;
            }
            hipLaunchKernelGGL(k_gp_qcei_cond<true>, cgrid, block, cond_lds, st, gps,
                               d_part, d_Kr, d_KVr, z, stab_, S, R, Q, rows, n_part, d_s,
                               d_p, d_post);
            hipLaunchKernelGGL(k_gp_qlogcei_reduce<true>, dim3((unsigned)bc), block,
                               red_lds, st, gps, d_s, z, F, d_p, d_post, G, n_obj_, tau_,
                               R, Q, rows, d_f + b0, d_wm, d_wv, d_u);
            // UV_g (bc, N) = u_g (bc, R) @ Vr_g^T, over K_g: UV^T (N, bc) = Vr @ u^T.
            ROCBLAS_CHECK(rocblas_dgemm_batched(
                blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)N_,
                (rocblas_int)bc, (rocblas_int)R_, &one, p_Vr, (rocblas_int)N_, p_u,
                (rocblas_int)R_, &zero, p_K, (rocblas_int)N_, G));
            hipLaunchKernelGGL(k_gp_qcei_grad_gps, pgrid, block, 0, st, gps, d_K, d_MP,
                               d_V, xc, d_wm, d_wv, d_u, d_MPr, Xr_, N_, D, R, rows, nK,
                               n_gpart, cat_mask_, d_gpart);
            hipLaunchKernelGGL(k_gp_qlogcei_grad_finish,
                               dim3((unsigned)((bc * D + GP_BLOCK - 1) / GP_BLOCK)),
                               block, 0, st, gps, d_gpart, n_gpart, G, S, D, bc, cat_mask_,
                               d_g + b0 * D_);
        }
        return io.download(d_f, d_g);
    }

  private:
    int G_ = 0, n_obj_;
    int64_t N_, D_, R_, Q_ = 0;
    double stab_, tau_;
    int64_t budget_;
    uint64_t cat_mask_;
    const double* Xr_;
    QCeiGp host_[MAX_G];             // the table, host side
    DeviceBuffer<QCeiGp> table_;     // (G)
    DeviceBuffer<double> consts_;    // z (Q, G) | F (Q)
};
