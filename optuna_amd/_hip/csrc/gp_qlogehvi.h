// ---------------------------------------------------------------------------
// K5 (multi-objective, running trials): fused GP qLogEHVI forward + gradient
// over M device-resident GPs, 2 <= M <= 4, each conditioned on QMC fantasies at
// the same R running points, 1 <= R <= QLOGEI_MAX_R, with 1 <= Q <= QEHVI_MAX_Q
// draws.
//
// Fixed for the life of the acquisition, per objective m: the base GP, Xr (R, D),
// Vr_m = Cinv_m k_m(X, Xr) (N, R, column-major), the Cholesky factor L_m (R, R),
// W_m = (L_m L_m^T)^-1 delta_m (R, Q) and the QMC normals z (Q, M) of the
// candidate column. The fantasies at the running points move the Pareto front,
// so every draw q has its own n_q non-dominated boxes lo_q, iv_q (n_q, M); they
// are kept packed, (sum n_q, M) with offsets (Q + 1). The host pads every draw
// to Jmax boxes with lo = 0, iv = EPS; a padded box contributes EPS^M to the
// value and nothing to the gradient, which is added here in closed form.
//
// Per candidate x and objective m, as in gp_qlogei.h:
//   c_m = k_m(x, Xr) - K_m Vr_m,  y_m = L_m^-1 c_m,  p_m = L_m^-T y_m
//   cv_raw_m = max(raw_m, 0) + stab - sum y_m^2,  sd_m = sqrt(max(cv_raw_m, 0))
//   s[q,m]   = K_m.alpha_m + c_m.W_m[:, q] + sd_m z[q,m]
// and then, as in gp_ehvi.h but with the boxes of the draw,
//   d[q,j,m] = min(max(s[q,m] - lo[q,j,m], EPS), iv[q,j,m])
//   P_q = sum_{j < n_q} prod_m d[q,j,m] + (Jmax - n_q) EPS^M
//   T = sum_q P_q,  f = log T - log Q
// over the products themselves, not their logs (gp_ehvi.h says why).
//
// CLOSED FORM gradient: with a[q,m] = sum_j prod_{m' != m} d[q,j,m'] over the
// open factors (EPS < s - lo < iv) and g[q,m] = a[q,m] / T,
//   wm_m  = sum_q g[q,m]
//   wv'_m = sum_q g[q,m] z[q,m] / (2 sd_m)       (0 where cv_raw_m <= 0)
//   wv_m  = wv'_m                                (0 where raw_m < 0)
//   u[r,m] = sum_q g[q,m] W_m[r, q] - 2 wv'_m p_m[r]
// and the input gradient is gp_qlogei.h's, summed over the objectives:
//   grad_d = sum_m 2 eta_md (x_d sum coef_m - sum coef_m X_.d)  over N + R rows,
//   coef_mi = (wm_m alpha_mi - 2 wv_m V_mi - sum_r u[r,m] Vr_m[i, r]) MP_mi
//   coef_mr = u[r,m] MPr_mr
// and exactly 0 on a categorical column.
//
// Launches per chunk of candidates: per objective gp_enqueue_kv, k_gp_cross_cov
// against Xr, one dgemm for K Vr, k_gp_logpi_partial<false> and
// k_gp_qehvi_cond, which leaves s (bc, Q, M); then k_gp_qlogehvi_box over
// (tiles of candidates, slices of draws) and k_gp_qlogehvi_finish; with the
// gradient per objective one dgemm u Vr^T into the region K held and
// k_gp_qlogei_grad into its own record set, then k_gp_qlogehvi_grad_finish.
// Every record has one writer, all reductions run in a fixed order and there
// are no floating-point atomics: equal inputs in equal batches give equal bits.
// ---------------------------------------------------------------------------

#pragma once

#include "gp_ehvi.h"
#include "gp_qlogei.h"

// s, the records and the staged a[q,m] of one candidate stay small.
constexpr int QEHVI_MAX_Q = 512;
// Candidates a workgroup of the box kernel applies each box to. Every lane
// keeps QEHVI_TILE * (1 + M) fp64 accumulators in registers beside the 2 M
// doubles of its box (docs/PERF.md has the compiler's figures).
constexpr int QEHVI_TILE = 8;

// Doubles of dynamic LDS of k_gp_qehvi_cond: L (R, ldl) | c (R) | p (R) |
// K.alpha, K.V, quad.
static size_t qehvi_cond_lds_doubles(int R) {
    return (size_t)R * qlogei_ldl(R) + 2 * (size_t)R + 3;
}

// One workgroup per candidate, one launch per objective m: qlogei_condition,
// then all threads write s[b, q, m] for q = tid, tid + 256, ..., reading 64
// consecutive q of a row of W per wavefront. With GRAD also p (R) and
// post = sd, [cv_raw > 0], [raw >= 0] of the candidate.
// The body is a device function so that the GP-batched launch of
// gp_qlogcei.h runs the same code.
template <bool GRAD>
__device__ __forceinline__ void
qehvi_cond_body(const double* __restrict__ part,  // (bc, S, 2): K.alpha, K.V
                const double* __restrict__ Kr,    // (bc, R) = k(x, Xr)
                const double* __restrict__ KVr,   // (bc, R) = K @ Vr
                const double* __restrict__ L,     // (R, R) lower
                const double* __restrict__ W,     // (R, Q)
                const double* __restrict__ z,     // (Q, M)
                double scale, double stab_noise, int S, int R, int Q, int m, int M,
                double* __restrict__ out_s,       // (bc, Q, M)
                double* __restrict__ out_p,       // (bc, R), GRAD only
                double* __restrict__ out_post) {  // (bc, 3), GRAD only
    extern __shared__ double qehvi_cond_lds[];
    double* Ls = qehvi_cond_lds;
    double* cs = Ls + (size_t)R * qlogei_ldl(R);
    double* ps = cs + R;
    double* post = ps + R;  // K.alpha, K.V, quad

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    qlogei_condition<GRAD>(part, Kr, KVr, L, S, R, b, Ls, cs, ps, post);

    const double kmean = post[0];
    const double raw = scale - post[1];
    const double cv_raw = (raw > 0.0 ? raw : 0.0) + stab_noise - post[2];
    const double sd = sqrt(cv_raw > 0.0 ? cv_raw : 0.0);
    for (int q = tid; q < Q; q += GP_BLOCK) {
        double cw = 0.0;
        for (int r = 0; r < R; ++r) cw += cs[r] * W[(size_t)r * Q + q];
        out_s[(b * Q + q) * M + m] = kmean + cw + sd * z[(size_t)q * M + m];
    }
    if constexpr (GRAD) {
        if (tid < R) out_p[b * R + tid] = ps[tid];
        if (tid == 0) {
            out_post[b * 3] = sd;
            out_post[b * 3 + 1] = cv_raw > 0.0 ? 1.0 : 0.0;
            out_post[b * 3 + 2] = raw >= 0.0 ? 1.0 : 0.0;  // clamp_min passes it here
        }
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qehvi_cond(const double* __restrict__ part,  // (bc, S, 2): K.alpha, K.V
                const double* __restrict__ Kr,    // (bc, R) = k(x, Xr)
                const double* __restrict__ KVr,   // (bc, R) = K @ Vr
                const double* __restrict__ L,     // (R, R) lower
                const double* __restrict__ W,     // (R, Q)
                const double* __restrict__ z,     // (Q, M)
                double scale, double stab_noise, int S, int R, int Q, int m, int M,
                double* __restrict__ out_s,       // (bc, Q, M)
                double* __restrict__ out_p,       // (bc, R), GRAD only
                double* __restrict__ out_post) {  // (bc, 3), GRAD only
    qehvi_cond_body<GRAD>(part, Kr, KVr, L, W, z, scale, stab_noise, S, R, Q, m, M,
                          out_s, out_p, out_post);
}

// Words of one (candidate, draw) record: P_q, and with the gradient
// a[q,0] .. a[q,M-1].
constexpr int qehvi_words(int M, bool grad) { return grad ? 1 + M : 1; }

__host__ __device__ __forceinline__ double qehvi_pad_term(int M) {
    double t = EHVI_EPS;
    for (int m = 1; m < M; ++m) t *= EHVI_EPS;
    return t;
}

// Workgroup (t, y) of a (ceil(bc / QEHVI_TILE), Sq) grid takes the candidates
// [t * QEHVI_TILE, ...) and the draws [y * ceil(Q / Sq), (y + 1) * ceil(Q / Sq)).
// The boxes of a draw are the same for every candidate, so each is loaded once
// and applied to the whole tile: a wavefront owns one draw at a time, lane l
// loads the boxes l, l + 64, ... of it into registers (2 M doubles) and applies
// each to the QEHVI_TILE candidates, whose s of that draw sit in LDS and are
// read wavefront-uniformly. After the boxes of the draw the 1 + M sums of every
// candidate are reduced by shuffles and lane 0 writes the record. A draw is
// never split, so a record has one writer and nothing is reduced across
// workgroups. The four wavefronts step through the slice together (four
// consecutive draws per step), which keeps the two barriers of a step uniform
// although the draws differ in their box counts.
template <int M, bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogehvi_box(const double* __restrict__ s,    // (bc, Q, M)
                  const double* __restrict__ lo,   // (sum n_q, M)
                  const double* __restrict__ iv,   // (sum n_q, M)
                  const int* __restrict__ offset,  // (Q + 1)
                  int Q, int Jmax, int64_t bc,
                  double* __restrict__ rec) {  // (bc, Q, W)
    constexpr int W = qehvi_words(M, GRAD);
    __shared__ double ss[GP_WAVES][QEHVI_TILE][M];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t b0 = (int64_t)blockIdx.x * QEHVI_TILE;
    const int nb = (int)min((int64_t)QEHVI_TILE, bc - b0);
    const int per = (Q + (int)gridDim.y - 1) / (int)gridDim.y;
    const int q0 = min(Q, (int)blockIdx.y * per);
    const int q1 = min(Q, q0 + per);

    for (int qb = q0; qb < q1; qb += GP_WAVES) {
        __syncthreads();  // the previous draws are consumed (first step: nothing)
        if (tid < GP_WAVES * QEHVI_TILE * M) {
            const int w = tid / (QEHVI_TILE * M), c = (tid / M) % QEHVI_TILE,
                      m = tid % M;
            // A candidate past the chunk or a draw past the slice stages 0 and
            // writes nothing below.
            ss[w][c][m] = (qb + w < q1 && c < nb)
                              ? s[((b0 + c) * Q + (qb + w)) * M + m]
                              : 0.0;
        }
        __syncthreads();
        const int q = qb + wave;
        if (q >= q1) continue;  // the barriers are at the top: every thread meets them

        const int j0 = offset[q], j1 = offset[q + 1];
        double acc[QEHVI_TILE][W] = {};  // P | a_0..a_{M-1}
        for (int j = j0 + lane; j < j1; j += 64) {
            double bl[M], bw[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                bl[m] = lo[(size_t)j * M + m];
                bw[m] = iv[(size_t)j * M + m];
            }
#pragma unroll
            for (int c = 0; c < QEHVI_TILE; ++c) {
                double d[M];
                bool open[M];  // neither clamp active
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const double diff = ss[wave][c][m] - bl[m];
                    d[m] = fmin(fmax(diff, EHVI_EPS), bw[m]);
                    open[m] = diff > EHVI_EPS && diff < bw[m];
                }
                double prod = d[0];
#pragma unroll
                for (int m = 1; m < M; ++m) prod *= d[m];
                acc[c][0] += prod;
                if constexpr (GRAD) {
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        double others = 1.0;  // prod / d[m] without the division
#pragma unroll
                        for (int k = 0; k < M; ++k)
                            if (k != m) others *= d[k];
                        acc[c][1 + m] += open[m] ? others : 0.0;
                    }
                }
                // One candidate at a time: interleaved, the tile's M compare
                // masks each outgrow the scalar registers and spill.
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int c = 0; c < QEHVI_TILE; ++c)
#pragma unroll
            for (int k = 0; k < W; ++k)
                for (int off = 32; off > 0; off >>= 1)
                    acc[c][k] += __shfl_down(acc[c][k], off);
        if (lane == 0) {
            const double pad = (double)(Jmax - (j1 - j0)) * qehvi_pad_term(M);
#pragma unroll
            for (int c = 0; c < QEHVI_TILE; ++c) {
                if (c < nb) {
                    double* out = rec + ((b0 + c) * Q + q) * W;
                    out[0] = acc[c][0] + pad;
#pragma unroll
                    for (int k = 1; k < W; ++k) out[k] = acc[c][k];
                }
            }
        }
    }
}

// What the two finish kernels read per objective.
struct QEhviArgs {
    const double* W[EHVI_MAX_M];    // (R, Q)
    const double* eta[EHVI_MAX_M];  // (D)
};

// Doubles of dynamic LDS of k_gp_qlogehvi_finish: GP_WAVES sums, and with the
// gradient a (M, Q) | sum_q a W (M, R).
static size_t qehvi_finish_lds_doubles(int M, int R, int Q, bool grad) {
    return GP_WAVES + (grad ? (size_t)M * Q + (size_t)M * R : 0);
}

// One workgroup per candidate: the Q records in draw order, q = tid,
// tid + 256, ... per thread and the threads by in-order block sums; then the
// value and, with GRAD, the posterior-side weights of every objective, set m
// of wm / wv (M, ld) and u / p (M, ld, R). The M R sums sum_q a[q,m] W_m[r, q]
// are split over the wavefronts, pair (m, r) = w, w + 4, ..., each summed by
// its wavefront with 64 consecutive q of a row of W per step.
template <int M, bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogehvi_finish(const double* __restrict__ rec,   // (bc, Q, W)
                     const double* __restrict__ z,     // (Q, M)
                     const double* __restrict__ p,     // (M, ld, R)
                     const double* __restrict__ post,  // (M, ld, 3)
                     QEhviArgs P, int R, int Q, int64_t ld,
                     double* __restrict__ out_f,    // (bc)
                     double* __restrict__ out_wm,   // (M, ld), GRAD only
                     double* __restrict__ out_wv,   // (M, ld), GRAD only
                     double* __restrict__ out_u) {  // (M, ld, R), GRAD only
    constexpr int W = qehvi_words(M, GRAD);
    extern __shared__ double qehvi_fin_lds[];
    double* red = qehvi_fin_lds;
    double* as = red + GP_WAVES;       // (M, Q), GRAD only
    double* sw = as + (size_t)M * Q;   // (M, R), GRAD only

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* rb = rec + b * Q * W;
    double acc_p = 0.0, acc_a[M] = {}, acc_z[M] = {};
    for (int q = tid; q < Q; q += GP_BLOCK) {
        acc_p += rb[(size_t)q * W];
        if constexpr (GRAD) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double a = rb[(size_t)q * W + 1 + m];
                as[m * Q + q] = a;
                acc_a[m] += a;
                acc_z[m] += a * z[(size_t)q * M + m];
            }
        }
    }
    const double total = gp_block_sum(acc_p, red);
    if (tid == 0) out_f[b] = log(total) - log((double)Q);
    if constexpr (GRAD) {
        // The barriers in here also publish `as`.
        double wvp[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double a_sum = gp_block_sum(acc_a[m], red);
            const double z_sum = gp_block_sum(acc_z[m], red);
            const double* pm = post + ((size_t)m * ld + b) * 3;
            wvp[m] = pm[1] != 0.0 ? (z_sum / total) / (2.0 * pm[0]) : 0.0;
            if (tid == 0) {
                out_wm[m * ld + b] = a_sum / total;
                out_wv[m * ld + b] = pm[2] != 0.0 ? wvp[m] : 0.0;
            }
        }
        const int lane = tid & 63;
        for (int pair = tid >> 6; pair < M * R; pair += GP_WAVES) {
            const int m = pair / R, r = pair % R;
            const double* Wr = P.W[m] + (size_t)r * Q;
            double a = 0.0;
            for (int q = lane; q < Q; q += 64) a += as[m * Q + q] * Wr[q];
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
            if (lane == 0) sw[pair] = a;
        }
        __syncthreads();
        for (int pair = tid; pair < M * R; pair += GP_BLOCK) {
            const int m = pair / R, r = pair % R;
            const size_t at = ((size_t)m * ld + b) * R + r;
            double w = wvp[0];
#pragma unroll
            for (int k = 1; k < M; ++k) w = m == k ? wvp[k] : w;
            out_u[at] = sw[pair] / total - 2.0 * w * p[at];
        }
    }
}

// One thread per (candidate, d): the M record sets of k_gp_qlogei_grad, set m
// at part + m * set_stride, objective first, then the S records of it in
// order, each objective times 2 eta_md; exactly 0.0 on a categorical column.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogehvi_grad_finish(const double* __restrict__ part,  // (M, .): (bc, S, D)
                          size_t set_stride, QEhviArgs P, int M, int S, int D,
                          int64_t B, uint64_t cat_mask,
                          double* __restrict__ out_grad) {  // (bc, D)
    const int64_t t = (int64_t)blockIdx.x * GP_BLOCK + threadIdx.x;
    const int64_t b = t / D;
    const int d = (int)(t % D);
    if (b >= B) return;
    double out = 0.0;
    for (int m = 0; m < M; ++m) {
        const double* r = part + m * set_stride + b * S * D;
        double a = r[d];
        for (int s = 1; s < S; ++s) a += r[s * D + d];
        out += 2.0 * P.eta[m][d] * a;
    }
    out_grad[b * D + d] = gp_is_cat(cat_mask, d) ? 0.0 : out;
}

// Session over M torch-owned device GPs and the torch-owned tensors of their
// conditioning on the running trials (raw pointers; same HIP context), with its
// own copies of the QMC normals and the packed per-draw boxes. Built once per
// acquisition function; evaluations upload only the (B, D) candidates.
class GpQLogEhviSession {
  public:
    GpQLogEhviSession(const std::vector<int64_t>& X_ptrs,
                      const std::vector<int64_t>& alpha_ptrs,
                      const std::vector<int64_t>& cinv_ptrs,
                      const std::vector<int64_t>& eta_ptrs,
                      const std::vector<double>& scales, int64_t N, int64_t D,
                      double stab_noise, int64_t Xr_ptr,
                      const std::vector<int64_t>& Vr_ptrs,
                      const std::vector<int64_t>& L_ptrs,
                      const std::vector<int64_t>& W_ptrs, int64_t R,
                      const arr_f64& z, const arr_f64& lo, const arr_f64& iv,
                      const arr_i64& offsets, int64_t Jmax,
                      int64_t scratch_budget_bytes, uint64_t cat_mask = 0)
        : N_(N), D_(D), R_(R), Jmax_(Jmax), stab_(stab_noise),
          budget_(scratch_budget_bytes),
          Xr_(reinterpret_cast<const double*>(Xr_ptr)) {
        const std::string who = "GpQLogEhviSession";
        M_ = gp_make_refs(who, X_ptrs, alpha_ptrs, cinv_ptrs, eta_ptrs, scales, 2,
                          EHVI_MAX_M, N, D, cat_mask, gp_);
        const size_t M = (size_t)M_;
        if (Vr_ptrs.size() != M || L_ptrs.size() != M || W_ptrs.size() != M)
            throw std::runtime_error(who + ": one Vr, L and W pointer per GP");
        if (N > INT32_MAX) throw std::runtime_error(who + ": N out of range");
        if (budget_ < 1) throw std::runtime_error(who + ": budget < 1");
        if (R < 1 || R > QLOGEI_MAX_R)
            throw std::runtime_error(who + ": need 1 <= R <= " +
                                     std::to_string(QLOGEI_MAX_R));
        if (z.ndim() != 2 || z.shape(1) != M_)
            throw std::runtime_error(who + ": z (Q, M)");
        Q_ = z.shape(0);
        if (Q_ < 1 || Q_ > QEHVI_MAX_Q)
            throw std::runtime_error(who + ": need 1 <= Q <= " +
                                     std::to_string(QEHVI_MAX_Q));
        if (lo.ndim() != 2 || iv.ndim() != 2 || lo.shape(1) != M_ ||
            iv.shape(1) != M_ || lo.shape(0) != iv.shape(0) || offsets.ndim() != 1 ||
            offsets.shape(0) != Q_ + 1)
            throw std::runtime_error(who + ": lo / iv (sum J, M), offsets (Q + 1)");
        const int64_t J = lo.shape(0);
        if (J > INT32_MAX / EHVI_MAX_M || Jmax < 1 || Jmax > INT32_MAX)
            throw std::runtime_error(who + ": box count out of range");
        // The kernel walks [offsets[q], offsets[q + 1]): they must stay inside
        // the packed arrays, and no draw may hold more than Jmax boxes.
        std::vector<int> off((size_t)Q_ + 1);
        for (int64_t q = 0; q <= Q_; ++q) {
            const int64_t o = offsets.at(q);
            const int64_t prev = q == 0 ? 0 : offsets.at(q - 1);
            if (o < prev || o - prev > Jmax || o > J || (q == 0 && o != 0) ||
                (q == Q_ && o != J))
                throw std::runtime_error(who + ": offsets must run from 0 to sum J "
                                               "in steps of 0 .. Jmax");
            off[(size_t)q] = (int)o;
        }
        for (size_t m = 0; m < M; ++m) {
            Vr_[m] = reinterpret_cast<const double*>(Vr_ptrs[m]);
            L_[m] = reinterpret_cast<const double*>(L_ptrs[m]);
            args_.W[m] = reinterpret_cast<const double*>(W_ptrs[m]);
            args_.eta[m] = gp_[m].eta;
        }
        const size_t nz = (size_t)Q_ * M, nj = (size_t)J * M;
        consts_.reserve(nz + 2 * nj + 1);
        offsets_.reserve((size_t)Q_ + 1);
        HIP_CHECK(hipMemcpy(consts_.ptr, z.data(), nz * 8, hipMemcpyHostToDevice));
        if (nj > 0) {
            HIP_CHECK(hipMemcpy(consts_.ptr + nz, lo.data(), nj * 8,
                                hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(consts_.ptr + nz + nj, iv.data(), nj * 8,
                                hipMemcpyHostToDevice));
        }
        HIP_CHECK(hipMemcpy(offsets_.ptr, off.data(), off.size() * sizeof(int),
                            hipMemcpyHostToDevice));
        J_ = J;
    }

    // Candidates per chunk. With the gradient every objective keeps its
    // K / MP / V set (K takes u Vr^T once the value pass is done with it);
    // without it one set is reused objective by objective. Everything else
    // eval() lays out per candidate of a chunk counts too, for small N it is
    // the larger part: s and the records, (Q, M) and (Q, W); Kr, KVr and the
    // (K.alpha, K.V) record; MPr per set; with the gradient p, u, post, wm, wv
    // and a record of D words per objective. Left out: the 1024 records that
    // gp_part_records adds whatever the chunk, and x, f, g of the whole batch.
    int64_t row_doubles(bool with_grad) const {
        const int64_t M = M_, sets = with_grad ? M : 1;
        return Q_ * (M + qehvi_words(M_, with_grad)) + 2 * R_ + 2 + sets * R_ +
               (with_grad ? M * (2 * R_ + 5 + D_) : 0);
    }
    int64_t chunk_rows(bool with_grad) const {
        return gp_chunk_rows_with(budget_, N_, with_grad ? M_ : 1,
                                  row_doubles(with_grad));
    }
    int64_t n_chunks(int64_t B, bool with_grad) const {
        return gp_n_chunks(B, chunk_rows(with_grad));
    }
    // Workgroups per candidate in the two N-walks for a chunk of bc
    // candidates: at least one block's worth of observations each.
    int n_splits(int64_t bc) const {
        return gp_splits(bc, (N_ + GP_BLOCK - 1) / GP_BLOCK);
    }
    // Slices of draws in the box kernel for a chunk of bc candidates.
    int draw_splits(int64_t bc) const { return gp_splits(bc, Q_); }

    py::tuple eval(const arr_f64& x, bool with_grad) {
        GpEvalIo io(x, D_, with_grad);
        const int64_t B = io.B;
        if (B == 0) return io.download(nullptr, nullptr);

        const int64_t rows = std::min(chunk_rows(with_grad), B);
        const int D = (int)D_, R = (int)R_, Q = (int)Q_, M = M_;
        const int n_sets = with_grad ? M : 1;
        const int W = qehvi_words(M, with_grad);
        const size_t nK = (size_t)rows * N_, nR = (size_t)rows * R_,
                     nBD = (size_t)B * D_, nQ = (size_t)rows * Q_,
                     n_gpart = gp_part_records(rows) * D_;
        const size_t gM = with_grad ? (size_t)M : 0;
        WsLayout lay;
        const auto s_x = lay.add<double>(nBD), s_f = lay.add<double>(B),
                   s_g = lay.add<double>(with_grad ? nBD : 0),
                   s_part = lay.add<double>(gp_part_records(rows) * 2),
                   s_gpart = lay.add<double>(gM * n_gpart),
                   s_Kr = lay.add<double>(nR), s_KVr = lay.add<double>(nR),
                   s_MPr = lay.add<double>(nR * n_sets),
                   s_s = lay.add<double>(nQ * M), s_rec = lay.add<double>(nQ * W),
                   s_p = lay.add<double>(gM * nR), s_u = lay.add<double>(gM * nR),
                   s_post = lay.add<double>(gM * rows * 3),
                   s_wm = lay.add<double>(gM * rows),
                   s_wv = lay.add<double>(gM * rows),
                   s_K = lay.add<double>(nK * n_sets),
                   s_MP = lay.add<double>(nK * n_sets),
                   s_V = lay.add<double>(nK * n_sets);
        char* base = g_ws.ensure_bytes(lay.bytes());
        double *d_x = s_x.in(base), *d_f = s_f.in(base), *d_g = s_g.in(base),
               *d_part = s_part.in(base), *d_gpart = s_gpart.in(base),
               *d_Kr = s_Kr.in(base), *d_KVr = s_KVr.in(base),
               *d_MPr = s_MPr.in(base), *d_s = s_s.in(base),
               *d_rec = s_rec.in(base), *d_p = s_p.in(base), *d_u = s_u.in(base),
               *d_post = s_post.in(base), *d_wm = s_wm.in(base),
               *d_wv = s_wv.in(base), *d_K = s_K.in(base), *d_MP = s_MP.in(base),
               *d_V = s_V.in(base);
        hipStream_t st = io.upload(d_x);
        rocblas_handle blas = get_blas(st);

        const double* z = consts_.ptr;
        const double* lo = z + (size_t)Q_ * M;
        const double* iv = lo + (size_t)J_ * M;
        const size_t cond_lds = qehvi_cond_lds_doubles(R) * 8;
        const double one = 1.0, zero = 0.0;
        for (int64_t b0 = 0; b0 < B; b0 += rows) {
            const int64_t bc = std::min(rows, B - b0);
            const double* xc = d_x + b0 * D_;
            const int S = n_splits(bc);
            const dim3 pgrid((unsigned)bc, (unsigned)S);
            for (int m = 0; m < M; ++m) {
                const size_t set = with_grad ? (size_t)m : 0;
                double *Km = d_K + set * nK, *MPm = d_MP + set * nK,
                       *Vm = d_V + set * nK, *MPrm = d_MPr + set * nR;
                const GpRef& gp = gp_[m];
                gp_enqueue_kv(st, blas, gp, xc, bc, N_, D_, Km, MPm, Vm);
                // Kr, MPr (bc, R): the same cross-covariance against Xr.
                const dim3 rgrid((unsigned)((R_ + GP_BLOCK - 1) / GP_BLOCK),
                                 (unsigned)bc);
                if (gp.cat_mask != 0)
                    hipLaunchKernelGGL(k_gp_cross_cov<true>, rgrid, dim3(GP_BLOCK), 0,
                                       st, Xr_, gp.eta, gp.scale, xc, R_, D_, bc, d_Kr,
                                       MPrm, gp.cat_mask);
                else
                    hipLaunchKernelGGL(k_gp_cross_cov<false>, rgrid, dim3(GP_BLOCK), 0,
                                       st, Xr_, gp.eta, gp.scale, xc, R_, D_, bc, d_Kr,
                                       MPrm, gp.cat_mask);
                // KVr (bc, R) = K (bc, N) @ Vr (N, R); column-major that is
                // KVr^T (R, bc) = Vr^T @ K^T.
                ROCBLAS_CHECK(rocblas_dgemm(
                    blas, rocblas_operation_transpose, rocblas_operation_none,
                    (rocblas_int)R_, (rocblas_int)bc, (rocblas_int)N_, &one, Vr_[m],
                    (rocblas_int)N_, Km, (rocblas_int)N_, &zero, d_KVr,
                    (rocblas_int)R_));
                hipLaunchKernelGGL(k_gp_logpi_partial<false>, pgrid, dim3(GP_BLOCK), 0,
                                   st, Km, MPm, Vm, gp.alpha, gp.X, xc, N_, D,
                                   gp.cat_mask, d_part);
                if (with_grad)
                    hipLaunchKernelGGL(k_gp_qehvi_cond<true>, dim3((unsigned)bc),
                                       dim3(GP_BLOCK), cond_lds, st, d_part, d_Kr,
                                       d_KVr, L_[m], args_.W[m], z, gp.scale, stab_, S,
                                       R, Q, m, M, d_s, d_p + (size_t)m * nR,
                                       d_post + (size_t)m * rows * 3);
                else
                    hipLaunchKernelGGL(k_gp_qehvi_cond<false>, dim3((unsigned)bc),
                                       dim3(GP_BLOCK), cond_lds, st, d_part, d_Kr,
                                       d_KVr, L_[m], args_.W[m], z, gp.scale, stab_, S,
                                       R, Q, m, M, d_s, nullptr, nullptr);
            }
            launch_boxes(with_grad, bc, rows, st, d_s, z, lo, iv, d_rec, d_p, d_post,
                         d_f + b0, d_wm, d_wv, d_u);
            if (!with_grad) continue;
            for (int m = 0; m < M; ++m) {
                const GpRef& gp = gp_[m];
                double* Km = d_K + (size_t)m * nK;
                const double* um = d_u + (size_t)m * nR;
                // UV (bc, N) = u (bc, R) @ Vr^T, over K: UV^T (N, bc) = Vr @ u^T.
                ROCBLAS_CHECK(rocblas_dgemm(
                    blas, rocblas_operation_none, rocblas_operation_none,
                    (rocblas_int)N_, (rocblas_int)bc, (rocblas_int)R_, &one, Vr_[m],
                    (rocblas_int)N_, um, (rocblas_int)R_, &zero, Km, (rocblas_int)N_));
                hipLaunchKernelGGL(k_gp_qlogei_grad, pgrid, dim3(GP_BLOCK), 0, st, Km,
                                   d_MP + (size_t)m * nK, d_V + (size_t)m * nK, gp.alpha,
                                   gp.X, xc, d_wm + (size_t)m * rows,
                                   d_wv + (size_t)m * rows, um, d_MPr + (size_t)m * nR,
                                   Xr_, N_, D, R, gp.cat_mask,
                                   d_gpart + (size_t)m * n_gpart);
            }
            hipLaunchKernelGGL(k_gp_qlogehvi_grad_finish,
                               dim3((unsigned)((bc * D + GP_BLOCK - 1) / GP_BLOCK)),
                               dim3(GP_BLOCK), 0, st, d_gpart, n_gpart, args_, M, S, D,
                               bc, gp_[0].cat_mask, d_g + b0 * D_);
        }
        return io.download(d_f, d_g);
    }

  private:
    // The box kernel over (tiles of candidates, slices of draws), then the
    // per-candidate finish.
    template <int M, bool GRAD>
    void launch_boxes_as(int64_t bc, int64_t rows, hipStream_t st, const double* s,
                         const double* z, const double* lo, const double* iv,
                         double* rec, const double* p, const double* post, double* f,
                         double* wm, double* wv, double* u) {
        const dim3 grid((unsigned)((bc + QEHVI_TILE - 1) / QEHVI_TILE),
                        (unsigned)draw_splits(bc));
        hipLaunchKernelGGL((k_gp_qlogehvi_box<M, GRAD>), grid, dim3(GP_BLOCK), 0, st, s,
                           lo, iv, offsets_.ptr, (int)Q_, (int)Jmax_, bc, rec);
        hipLaunchKernelGGL((k_gp_qlogehvi_finish<M, GRAD>), dim3((unsigned)bc),
                           dim3(GP_BLOCK),
                           qehvi_finish_lds_doubles(M, (int)R_, (int)Q_, GRAD) * 8, st,
                           rec, z, p, post, args_, (int)R_, (int)Q_, rows, f, wm, wv,
                           u);
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
    int64_t N_, D_, R_, Q_ = 0, J_ = 0, Jmax_;
    double stab_;
    int64_t budget_;
    const double* Xr_;
    const double* Vr_[EHVI_MAX_M];
    const double* L_[EHVI_MAX_M];
    QEhviArgs args_{};                // W and eta per objective
    DeviceBuffer<double> consts_;     // z (Q, M) | lo (sum J, M) | iv (sum J, M)
    DeviceBuffer<int> offsets_;       // (Q + 1)
};
