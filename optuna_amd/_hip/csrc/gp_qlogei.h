// ---------------------------------------------------------------------------
// K5 (running trials): fused GP qLogEI forward + gradient over a
// device-resident GP conditioned on QMC fantasies at R running points,
// 1 <= R <= QLOGEI_MAX_R, with 1 <= Q <= QLOGEI_MAX_Q draws.
//
// Fixed for the life of the acquisition: the running points Xr (R, D),
// Vr = Cinv k(X, Xr) (N, R, column-major), the Cholesky factor L (R, R) of the
// running rows' posterior covariance plus stab, W = (L L^T)^-1 delta (R, Q),
// the QMC normals z (Q) of the candidate column and
// m_q = max_r max(fantasy[q, r] - t, EPS).
//
// Per candidate x, with K = k(x, X), V = K Cinv and raw = scale - K.V from
// gp_posterior.h:
//   c      = k(x, Xr) - K Vr                        (R)
//   y      = L^-1 c,  p = L^-T y,  quad = sum y^2
//   cv_raw = max(raw, 0) + stab - quad,  sd = sqrt(max(cv_raw, 0))
//   s_q    = K.alpha + c.W[:, q] + sd z_q
//   E_q    = max(m_q, s_q - t, EPS)
//   f      = log sum_q E_q - log Q
// quad comes from the triangular solve, never from an explicit (L L^T)^-1, so
// it is a sum of squares and cannot go negative.
//
// CLOSED FORM gradient: with A = {q : s_q - t > max(m_q, EPS)}, S = sum E_q,
//   w_m  = |A| / S
//   w_v' = (sum_A z_q / S) / (2 sd)
//   w_v  = w_v'  (0 where the clamp on raw is active)
//   u_r  = sum_A W[r, q] / S - 2 w_v' p_r
//   grad_d = 2 eta_d (x_d sum coef - sum coef X_.d)  over N + R rows,
//   coef_i = (w_m alpha_i - 2 w_v V_i - sum_r u_r Vr[i, r]) MP_i   (training)
//   coef_r = u_r MPr_r                                              (running)
// and exactly 0 on a categorical column (gp_posterior.h's cat_mask).
// Clamps as in the other sessions: nothing flows through a clamped raw or a
// clamped cv_raw. At cv_raw == 0 exactly, where torch's sqrt backward divides
// by zero and gives NaN, w_v' is 0 here.
//
// Launches per chunk of candidates: k_gp_cross_cov + dgemm (gp_enqueue_kv),
// k_gp_cross_cov against Xr, one dgemm for K Vr, k_gp_logpi_partial<false>
// for the (K.alpha, K.V) records over S workgroups per candidate,
// k_gp_qlogei_sample; with the gradient one dgemm u Vr^T into the region K
// held, k_gp_qlogei_grad over (candidate, S) and k_gp_qlogei_grad_finish.
// All reductions run in a fixed order (wavefront shuffles, the wavefronts
// through LDS, row groups in order, workgroups of a candidate in order) and
// there are no floating-point atomics: equal inputs in equal batches give
// equal bits.
// ---------------------------------------------------------------------------

#pragma once

#include "gp_feasibility.h"

constexpr int QLOGEI_MAX_R = 64;    // one wavefront lane per running row
constexpr int QLOGEI_MAX_Q = 1024;  // one byte of LDS per draw
constexpr double QLOGEI_EPS = 1e-12;  // the host's _EPS

// Row pitch of L in LDS: odd, so that the lanes of a wavefront, which read
// one column of consecutive rows in the forward substitution, hit distinct
// banks.
__host__ __device__ __forceinline__ int qlogei_ldl(int R) { return R | 1; }

// Bytes of dynamic LDS of k_gp_qlogei_sample:
//   L (R, ldl) | c (R) | p (R) | sum_A W (R) | K.alpha, K.V, quad | GP_WAVES sums
//   | flags (Q bytes).
static size_t qlogei_lds_bytes(int R, int Q) {
    return ((size_t)R * qlogei_ldl(R) + 3 * (size_t)R + 3 + GP_WAVES) * 8 +
           (((size_t)Q + 7) & ~size_t(7));
}

// The conditioning of candidate b on the running rows, by a whole workgroup:
// all threads stage L (pitch qlogei_ldl) and c = Kr - KVr in LDS and one adds
// the candidate's S partial records; then the first wavefront does the two
// triangular solves with lane r owning row r (the R steps of each are
// sequential, a step is parallel over the rows and the pivot travels by a
// wavefront shuffle, so they need no block barrier). On return, behind a
// barrier: cs = c (R), post = K.alpha, K.V, quad and, with GRAD, ps = p (R).
template <bool GRAD>
__device__ __forceinline__ void
qlogei_condition(const double* __restrict__ part,  // (bc, S, 2): K.alpha, K.V
                 const double* __restrict__ Kr,    // (bc, R) = k(x, Xr)
                 const double* __restrict__ KVr,   // (bc, R) = K @ Vr
                 const double* __restrict__ L,     // (R, R) lower
                 int S, int R, int64_t b, double* Ls, double* cs, double* ps,
                 double* post) {
    const int tid = threadIdx.x;
    const int ldl = qlogei_ldl(R);
    for (int i = tid; i < R * R; i += GP_BLOCK) Ls[(i / R) * ldl + (i % R)] = L[i];
    if (tid < R) cs[tid] = Kr[b * R + tid] - KVr[b * R + tid];
    if (tid == GP_BLOCK - 1) {
        // The S records of the candidate in order, read once for the workgroup
        // by a thread of the last wavefront, which stages least above.
        const double* rec = part + b * S * 2;
        double km = rec[0], kv = rec[1];
        for (int s = 1; s < S; ++s) {
            km += rec[2 * s];
            kv += rec[2 * s + 1];
        }
        post[0] = km;
        post[1] = kv;
    }
    __syncthreads();

    if (tid < 64) {
        const int r = tid;
        const bool row = r < R;
        // y = L^-1 c, column by column: lane j's value is final at step j.
        double v = row ? cs[r] : 0.0;
        for (int j = 0; j < R; ++j) {
            const double yj = __shfl(v, j) / Ls[j * ldl + j];
            if (r == j)
                v = yj;
            else if (r > j && row)
                v -= Ls[r * ldl + j] * yj;
        }
        double q2 = row ? v * v : 0.0;
        for (int off = 32; off > 0; off >>= 1) q2 += __shfl_down(q2, off);
        if (r == 0) post[2] = q2;
        if constexpr (GRAD) {
            // p = L^-T y, from the last row up; row j of L is read along itself.
            for (int j = R - 1; j >= 0; --j) {
                const double pj = __shfl(v, j) / Ls[j * ldl + j];
                if (r == j)
                    v = pj;
                else if (r < j)
                    v -= Ls[j * ldl + r] * pj;
            }
            if (row) ps[r] = v;
        }
    }
    __syncthreads();
}

// One workgroup per candidate: qlogei_condition, then all threads walk the
// draws, q = tid, tid + 256, ..., reading 64 consecutive q of a row of W per
// wavefront.
template <bool GRAD>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogei_sample(const double* __restrict__ part,  // (bc, S, 2): K.alpha, K.V
                   const double* __restrict__ Kr,    // (bc, R) = k(x, Xr)
                   const double* __restrict__ KVr,   // (bc, R) = K @ Vr
                   const double* __restrict__ L,     // (R, R) lower
                   const double* __restrict__ W,     // (R, Q)
                   const double* __restrict__ z,     // (Q)
                   const double* __restrict__ m,     // (Q)
                   double scale, double stab_noise, double threshold, int S,
                   int R, int Q,
                   double* __restrict__ out_f,    // (bc)
                   double* __restrict__ out_wm,   // (bc), GRAD only
                   double* __restrict__ out_wv,   // (bc), GRAD only
                   double* __restrict__ out_u) {  // (bc, R), GRAD only
    extern __shared__ double qlogei_lds[];
    const int ldl = qlogei_ldl(R);
    double* Ls = qlogei_lds;
    double* cs = Ls + (size_t)R * ldl;
    double* ps = cs + R;
    double* sw = ps + R;
    double* post = sw + R;  // K.alpha, K.V, quad
    double* red = post + 3;
    unsigned char* flag = reinterpret_cast<unsigned char*>(red + GP_WAVES);

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    qlogei_condition<GRAD>(part, Kr, KVr, L, S, R, b, Ls, cs, ps, post);

    const double kmean = post[0];
    const double raw = scale - post[1];
    const double cv_raw = (raw > 0.0 ? raw : 0.0) + stab_noise - post[2];
    const double sd = sqrt(cv_raw > 0.0 ? cv_raw : 0.0);
    double acc_e = 0.0, acc_n = 0.0, acc_z = 0.0;
    for (int q = tid; q < Q; q += GP_BLOCK) {
        double cw = 0.0;
        for (int r = 0; r < R; ++r) cw += cs[r] * W[(size_t)r * Q + q];
        const double zq = z[q];
        const double imp = kmean + cw + sd * zq - threshold;
        const double floor_q = fmax(m[q], QLOGEI_EPS);
        const bool active = imp > floor_q;
        acc_e += active ? imp : floor_q;
        if constexpr (GRAD) {
            flag[q] = active ? 1 : 0;
            if (active) {
                acc_n += 1.0;
                acc_z += zq;
            }
        }
    }
    const double total = gp_block_sum(acc_e, red);
    if (tid == 0) out_f[b] = log(total) - log((double)Q);
    if constexpr (GRAD) {
        // The barriers in here also publish `flag`.
        const double n_act = gp_block_sum(acc_n, red);
        const double z_act = gp_block_sum(acc_z, red);
        // sum_A W[r, .]: wavefront w takes the rows w, w + 4, ...
        const int lane = tid & 63;
        for (int r = tid >> 6; r < R; r += GP_WAVES) {
            double a = 0.0;
            for (int q = lane; q < Q; q += 64)
                if (flag[q]) a += W[(size_t)r * Q + q];
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
            if (lane == 0) sw[r] = a;
        }
        __syncthreads();
        const double wvp = cv_raw > 0.0 ? (z_act / total) / (2.0 * sd) : 0.0;
        if (tid < R) out_u[b * R + tid] = sw[tid] / total - 2.0 * wvp * ps[tid];
        if (tid == 0) {
            out_wm[b] = n_act / total;
            out_wv[b] = raw >= 0.0 ? wvp : 0.0;  // clamp_min passes the gradient here
        }
    }
}

// Workgroup (b, s) of a (bc, S) grid: the coef sums of the observations
// [s * ceil(N / S), (s + 1) * ceil(N / S)) of candidate b, and in workgroup
// s == 0 of the R running rows after them, with thread (g, d) = (tid / D,
// tid % D) as in k_gp_ehvi_grad. One record of D words,
// x_d sum coef - sum coef X_.d, the G groups of a dimension added in order.
// The body is a device function so that the GP-batched launch of
// gp_qlogcei.h runs the same code.
__device__ __forceinline__ void
qlogei_grad_body(const double* __restrict__ UV,     // (bc, N) = u @ Vr^T
                 const double* __restrict__ MP,     // (bc, N)
                 const double* __restrict__ V,      // (bc, N)
                 const double* __restrict__ alpha,  // (N)
                 const double* __restrict__ X,      // (N, D)
                 const double* __restrict__ x,      // (bc, D)
                 const double* __restrict__ wm,     // (bc)
                 const double* __restrict__ wv,     // (bc)
                 const double* __restrict__ u,      // (bc, R)
                 const double* __restrict__ MPr,    // (bc, R)
                 const double* __restrict__ Xr,     // (R, D)
                 int64_t N, int D, int R, uint64_t cat_mask,
                 double* __restrict__ part) {  // (bc, S, D)
    __shared__ double part_s[GP_BLOCK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int S = gridDim.y;
    const int64_t per = (N + S - 1) / S;
    const int64_t i0 = min(N, (int64_t)blockIdx.y * per);
    const int64_t i1 = min(N, i0 + per);
    const int G = GP_BLOCK / D;
    const int g = tid / D, d = tid % D;
    double acc = 0.0;
    // A categorical column keeps acc = 0: its Hamming term does not move with x.
    if (g < G && !gp_is_cat(cat_mask, d)) {
        const double xd = x[b * D + d];
        const double w_m = wm[b], w_v = wv[b];
        const double* MPb = MP + b * N;
        const double* Vb = V + b * N;
        const double* UVb = UV + b * N;
        double sum_c = 0.0, sum_cx = 0.0;
        for (int64_t i = i0 + g; i < i1; i += G) {
            const double c = (w_m * alpha[i] - 2.0 * w_v * Vb[i] - UVb[i]) * MPb[i];
            sum_c += c;
            sum_cx += c * X[i * D + d];
        }
        if (blockIdx.y == 0) {
            for (int r = g; r < R; r += G) {
                const double c = u[b * R + r] * MPr[b * R + r];
                sum_c += c;
                sum_cx += c * Xr[(int64_t)r * D + d];
            }
        }
        acc = xd * sum_c - sum_cx;
    }
    part_s[tid] = acc;
    __syncthreads();
    if (tid < D) {
        double out = part_s[tid];
        for (int k = 1; k < G; ++k) out += part_s[k * D + tid];
        part[(b * S + blockIdx.y) * D + tid] = out;
    }
}

__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogei_grad(const double* __restrict__ UV,     // (bc, N) = u @ Vr^T
                 const double* __restrict__ MP,     // (bc, N)
                 const double* __restrict__ V,      // (bc, N)
                 const double* __restrict__ alpha,  // (N)
                 const double* __restrict__ X,      // (N, D)
                 const double* __restrict__ x,      // (bc, D)
                 const double* __restrict__ wm,     // (bc)
                 const double* __restrict__ wv,     // (bc)
                 const double* __restrict__ u,      // (bc, R)
                 const double* __restrict__ MPr,    // (bc, R)
                 const double* __restrict__ Xr,     // (R, D)
                 int64_t N, int D, int R, uint64_t cat_mask,
                 double* __restrict__ part) {  // (bc, S, D)
    qlogei_grad_body(UV, MP, V, alpha, X, x, wm, wv, u, MPr, Xr, N, D, R, cat_mask,
                     part);
}

// One thread per (candidate, d): the S records in order, times 2 eta_d;
// exactly 0.0 on a categorical column.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_qlogei_grad_finish(const double* __restrict__ part,  // (bc, S, D)
                        const double* __restrict__ eta,   // (D)
                        int S, int D, int64_t B, uint64_t cat_mask,
                        double* __restrict__ out_grad) {  // (bc, D)
    const int64_t t = (int64_t)blockIdx.x * GP_BLOCK + threadIdx.x;
    const int64_t b = t / D;
    const int d = (int)(t % D);
    if (b >= B) return;
    const double* rec = part + b * S * D;
    double a = rec[d];
    for (int s = 1; s < S; ++s) a += rec[s * D + d];
    out_grad[b * D + d] = gp_is_cat(cat_mask, d) ? 0.0 : 2.0 * eta[d] * a;
}

// Session over a torch-owned device GP and the torch-owned tensors of its
// conditioning on the running trials (raw pointers; same HIP context), with
// its own copies of the QMC normals and the fantasies' best improvements.
// Built once per acquisition function; evaluations upload only the (B, D)
// candidates.
class GpQLogEiSession {
  public:
    GpQLogEiSession(int64_t X_ptr, int64_t alpha_ptr, int64_t cinv_ptr,
                    int64_t eta_ptr, int64_t N, int64_t D, double scale,
                    double stab_noise, double threshold, int64_t Xr_ptr,
                    int64_t Vr_ptr, int64_t L_ptr, int64_t W_ptr, int64_t R,
                    const arr_f64& z, const arr_f64& m,
                    int64_t scratch_budget_bytes, uint64_t cat_mask = 0)
        : N_(N), D_(D), R_(R), stab_(stab_noise), thr_(threshold),
          budget_(scratch_budget_bytes),
          Xr_(reinterpret_cast<const double*>(Xr_ptr)),
          Vr_(reinterpret_cast<const double*>(Vr_ptr)),
          L_(reinterpret_cast<const double*>(L_ptr)),
          W_(reinterpret_cast<const double*>(W_ptr)) {
        const std::string who = "GpQLogEiSession";
        gp_make_refs(who, {X_ptr}, {alpha_ptr}, {cinv_ptr}, {eta_ptr}, {scale}, 1, 1,
                     N, D, cat_mask, &gp_);
        if (N > INT32_MAX) throw std::runtime_error(who + ": N out of range");
        if (budget_ < 1) throw std::runtime_error(who + ": budget < 1");
        if (R < 1 || R > QLOGEI_MAX_R)
            throw std::runtime_error(who + ": need 1 <= R <= " +
                                     std::to_string(QLOGEI_MAX_R));
        if (z.ndim() != 1 || m.ndim() != 1 || z.shape(0) != m.shape(0))
            throw std::runtime_error(who + ": z (Q), m (Q)");
        Q_ = z.shape(0);
        if (Q_ < 1 || Q_ > QLOGEI_MAX_Q)
            throw std::runtime_error(who + ": need 1 <= Q <= " +
                                     std::to_string(QLOGEI_MAX_Q));
        consts_.reserve(2 * (size_t)Q_);
        HIP_CHECK(hipMemcpy(consts_.ptr, z.data(), Q_ * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(consts_.ptr + Q_, m.data(), Q_ * 8, hipMemcpyHostToDevice));
    }

    // Candidates per chunk: one K / MP / V set; the region of K takes u Vr^T
    // once the value pass is done with it.
    int64_t chunk_rows() const { return gp_chunk_rows(budget_, N_, 1); }
    int64_t n_chunks(int64_t B) const { return gp_n_chunks(B, chunk_rows()); }
    // Workgroups per candidate in the two N-walks for a chunk of bc
    // candidates: at least one block's worth of observations each.
    int n_splits(int64_t bc) const {
        return gp_splits(bc, (N_ + GP_BLOCK - 1) / GP_BLOCK);
    }

    py::tuple eval(const arr_f64& x, bool with_grad) {
        GpEvalIo io(x, D_, with_grad);
        const int64_t B = io.B;
        if (B == 0) return io.download(nullptr, nullptr);

        const int64_t rows = std::min(chunk_rows(), B);
        const int D = (int)D_, R = (int)R_, Q = (int)Q_;
        const size_t nK = (size_t)rows * N_, nR = (size_t)rows * R_,
                     nBD = (size_t)B * D_;
        const size_t words = with_grad ? std::max<size_t>(2, D_) : 2;
        WsLayout lay;
        const auto s_x = lay.add<double>(nBD), s_f = lay.add<double>(B),
                   s_g = lay.add<double>(with_grad ? nBD : 0),
                   s_part = lay.add<double>(gp_part_records(rows) * words),
                   s_Kr = lay.add<double>(nR), s_MPr = lay.add<double>(nR),
                   s_KVr = lay.add<double>(nR),
                   s_u = lay.add<double>(with_grad ? nR : 0),
                   s_wm = lay.add<double>(with_grad ? rows : 0),
                   s_wv = lay.add<double>(with_grad ? rows : 0),
                   s_K = lay.add<double>(nK), s_MP = lay.add<double>(nK),
                   s_V = lay.add<double>(nK);
        char* base = g_ws.ensure_bytes(lay.bytes());
        double *d_x = s_x.in(base), *d_f = s_f.in(base), *d_g = s_g.in(base),
               *d_part = s_part.in(base), *d_Kr = s_Kr.in(base),
               *d_MPr = s_MPr.in(base), *d_KVr = s_KVr.in(base),
               *d_u = s_u.in(base), *d_wm = s_wm.in(base), *d_wv = s_wv.in(base),
               *d_K = s_K.in(base), *d_MP = s_MP.in(base), *d_V = s_V.in(base);
        hipStream_t st = io.upload(d_x);
        rocblas_handle blas = get_blas(st);

        const double* z = consts_.ptr;
        const double* m = z + Q_;
        const size_t lds = qlogei_lds_bytes(R, Q);
        const double one = 1.0, zero = 0.0;
        for (int64_t b0 = 0; b0 < B; b0 += rows) {
            const int64_t bc = std::min(rows, B - b0);
            const double* xc = d_x + b0 * D_;
            const int S = n_splits(bc);
            gp_enqueue_kv(st, blas, gp_, xc, bc, N_, D_, d_K, d_MP, d_V);
            // Kr, MPr (bc, R): the same cross-covariance against Xr.
            const dim3 rgrid((unsigned)((R_ + GP_BLOCK - 1) / GP_BLOCK), (unsigned)bc);
            if (gp_.cat_mask != 0)
                hipLaunchKernelGGL(k_gp_cross_cov<true>, rgrid, dim3(GP_BLOCK), 0, st,
                                   Xr_, gp_.eta, gp_.scale, xc, R_, D_, bc, d_Kr, d_MPr,
                                   gp_.cat_mask);
            else
                hipLaunchKernelGGL(k_gp_cross_cov<false>, rgrid, dim3(GP_BLOCK), 0, st,
                                   Xr_, gp_.eta, gp_.scale, xc, R_, D_, bc, d_Kr, d_MPr,
                                   gp_.cat_mask);
            // KVr (bc, R) = K (bc, N) @ Vr (N, R); column-major that is
            // KVr^T (R, bc) = Vr^T @ K^T.
            ROCBLAS_CHECK(rocblas_dgemm(
                blas, rocblas_operation_transpose, rocblas_operation_none,
                (rocblas_int)R_, (rocblas_int)bc, (rocblas_int)N_, &one, Vr_,
                (rocblas_int)N_, d_K, (rocblas_int)N_, &zero, d_KVr, (rocblas_int)R_));
            const dim3 pgrid((unsigned)bc, (unsigned)S);
            hipLaunchKernelGGL(k_gp_logpi_partial<false>, pgrid, dim3(GP_BLOCK), 0, st,
                               d_K, d_MP, d_V, gp_.alpha, gp_.X, xc, N_, D, gp_.cat_mask,
                               d_part);
            if (!with_grad) {
                hipLaunchKernelGGL(k_gp_qlogei_sample<false>, dim3((unsigned)bc),
                                   dim3(GP_BLOCK), lds, st, d_part, d_Kr, d_KVr, L_, W_,
                                   z, m, gp_.scale, stab_, thr_, S, R, Q, d_f + b0,
                                   nullptr, nullptr, nullptr);
                continue;
            }
            hipLaunchKernelGGL(k_gp_qlogei_sample<true>, dim3((unsigned)bc),
                               dim3(GP_BLOCK), lds, st, d_part, d_Kr, d_KVr, L_, W_, z,
                               m, gp_.scale, stab_, thr_, S, R, Q, d_f + b0, d_wm, d_wv,
                               d_u);
            // UV (bc, N) = u (bc, R) @ Vr^T, over K: UV^T (N, bc) = Vr @ u^T.
            ROCBLAS_CHECK(rocblas_dgemm(
                blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)N_,
                (rocblas_int)bc, (rocblas_int)R_, &one, Vr_, (rocblas_int)N_, d_u,
                (rocblas_int)R_, &zero, d_K, (rocblas_int)N_));
            hipLaunchKernelGGL(k_gp_qlogei_grad, pgrid, dim3(GP_BLOCK), 0, st, d_K, d_MP,
                               d_V, gp_.alpha, gp_.X, xc, d_wm, d_wv, d_u, d_MPr, Xr_,
                               N_, D, R, gp_.cat_mask, d_part);
            hipLaunchKernelGGL(k_gp_qlogei_grad_finish,
                               dim3((unsigned)((bc * D + GP_BLOCK - 1) / GP_BLOCK)),
                               dim3(GP_BLOCK), 0, st, d_part, gp_.eta, S, D, bc,
                               gp_.cat_mask, d_g + b0 * D_);
        }
        return io.download(d_f, d_g);
    }

  private:
    GpRef gp_;
    int64_t N_, D_, R_, Q_ = 0;
    double stab_, thr_;
    int64_t budget_;
    const double *Xr_, *Vr_, *L_, *W_;
    DeviceBuffer<double> consts_;  // z (Q) | m (Q)
};
