// ---------------------------------------------------------------------------
// K4 (hyperparameter fit): the elementwise and reduction chains of one
// evaluation of the GP fit's loss and gradient, GPRegressor._loss_and_grad_numpy
// with default_log_prior, around torch's factorisation:
//
//   build_cov   C = scale * m52(r2) + noise * I              (N, N), symmetric
//   torch       L = chol(C), alpha = C^-1 y, Cinv = C^-1     rocSOLVER, untouched
//   grad        [loss, d loss / d raw (D + 2)]
//
// with r2_ij = sum_d eta_d (x_id - x_jd)^2 in DIFFERENCE form (eta_d [x_id !=
// x_jd] on a column of cat_mask), u = sqrt(5 r2), m52 = e^-u (5/3 r2 + u + 1),
// m52' = -5/6 (1 + u) e^-u, A = alpha alpha^T - Cinv, W = 1/2 scale A m52' and
//   g_eta_d = sum_ij W_ij (x_id - x_jd)^2,  g_scale = 1/2 sum_ij A_ij m52_ij,
//   g_noise = 1/2 sum_i A_ii.
//
// Both tile kernels run one workgroup of 256 threads per 64 x 64 tile of the
// lower triangle (tile row >= tile column). The two X tiles are staged in LDS
// FIT_CHUNK columns at a time with a row pitch of FIT_CHUNK + 1 doubles, so the
// 16 rows that the lanes of a wavefront read of one column lie in 16 different
// bank pairs. Thread (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 micro-tile
// rows ty + 16 a, columns tx + 16 b: for fixed (a, b) a wavefront touches 4 rows
// of 16 consecutive doubles of C or Cinv.
//
// k_gp_fit_cov writes a tile to C[i, j] and, below the diagonal tiles, the same
// values to C[j, i] through a transpose in LDS (over the X tiles, which are
// done by then), so both writes are row-contiguous. A diagonal tile computes
// all of its 64 x 64 entries; (i, j) and (j, i) run the same operations on
// operands that differ by the sign of the difference only, so C == C^T bit for
// bit either way.
//
// k_gp_fit_grad recomputes r2, m52 and m52' from the staged X tiles (X stays in
// L2); Cinv is the only (N, N) operand it reads. The 16 values W_ij stay in
// registers while the dimensions are walked a second time, FIT_CHUNK at a time,
// with FIT_CHUNK running sums per thread; a chunk is reduced over the wavefront
// by shuffles, over the four wavefronts through LDS in wavefront order, and
// goes into the tile's record: D lengthscale sums | sum A m52 | sum A_ii.
// A tile below the diagonal stands for its mirror image too and counts twice;
// a diagonal tile holds every ordered pair of its rows once and counts once.
// k_gp_fit_grad_finish, one workgroup, adds the records in tile order on two
// levels (runs of consecutive tiles, then the runs), forms y.alpha and
// sum log L_ii by gp_block_sum over strided per-thread sums, and applies the
// prior and the chain rule. Every record has one writer, there are
// no floating-point atomics: equal inputs give equal bits.
//
// Stream order: the kernels run on the workspace stream, torch's on its own.
// build_cov synchronises the workspace stream before it returns, so torch's
// cholesky sees C complete; the caller synchronises torch's current stream
// (torch.cuda.current_stream().synchronize()) before grad, so L, alpha and
// Cinv are complete when the tile kernel reads them. grad ends in the one
// synchronisation of its copy back.
// ---------------------------------------------------------------------------

#pragma once

#include <cmath>

#include "gp_posterior.h"

constexpr int FIT_TILE = 64;
constexpr int FIT_CHUNK = 16;
constexpr int FIT_PITCH = FIT_CHUNK + 1;       // doubles per staged row
constexpr int FIT_X_DOUBLES = 2 * FIT_TILE * FIT_PITCH;
// The transposed tile: with a pitch of 4 mod 32 the 64 lanes of a wavefront
// (16 tx, 4 consecutive ty) write tx * pitch + ty into 32 bank pairs twice each.
constexpr int FIT_T_PITCH = FIT_TILE + 4;

// Tile t of the lower triangle in row-major order: (ti, tj), ti >= tj.
__device__ __forceinline__ void fit_tile_of(unsigned t, int& ti, int& tj) {
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((unsigned)r * (unsigned)(r + 1) / 2 > t) --r;
    while ((unsigned)(r + 1) * (unsigned)(r + 2) / 2 <= t) ++r;
    ti = r;
    tj = (int)(t - (unsigned)r * (unsigned)(r + 1) / 2);
}

// Columns d0 .. d0 + FIT_CHUNK of rows i0 .. i0 + 64 into xi and of rows
// j0 .. j0 + 64 into xj; 0.0 past N and past D.
__device__ __forceinline__ void fit_stage(const double* __restrict__ X, int64_t N, int D,
                                          int64_t i0, int64_t j0, int d0, double* xi,
                                          double* xj) {
    for (int idx = threadIdx.x; idx < 2 * FIT_TILE * FIT_CHUNK; idx += GP_BLOCK) {
        const int which = idx / (FIT_TILE * FIT_CHUNK);
        const int r = (idx / FIT_CHUNK) % FIT_TILE, c = idx % FIT_CHUNK;
        const int64_t row = (which ? j0 : i0) + r;
        const int d = d0 + c;
        const double v = (row < N && d < D) ? X[row * D + d] : 0.0;
        (which ? xj : xi)[r * FIT_PITCH + c] = v;
    }
}

// r2 of the thread's micro-tile over all D columns. Leaves the X tiles free
// (a barrier after the last chunk). `et` holds eta, 0.0 from D to 64.
template <bool MIXED>
__device__ __forceinline__ void fit_r2(const double* __restrict__ X, int64_t N, int D,
                                       int64_t i0, int64_t j0, const double* et,
                                       uint64_t cat_mask, double* xi, double* xj,
                                       double (&r2)[4][4]) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
    for (int d0 = 0; d0 < D; d0 += FIT_CHUNK) {
        fit_stage(X, N, D, i0, j0, d0, xi, xj);
        __syncthreads();
        const int cn = min(FIT_CHUNK, D - d0);
        for (int c = 0; c < cn; ++c) {
            const double e = et[d0 + c];
            double vi[4], vj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                vi[a] = xi[(ty + 16 * a) * FIT_PITCH + c];
                vj[a] = xj[(tx + 16 * a) * FIT_PITCH + c];
            }
            bool cat = false;
            if constexpr (MIXED) cat = gp_is_cat(cat_mask, d0 + c);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double diff = vi[a] - vj[b];
                    if (MIXED && cat)
                        r2[a][b] += diff != 0.0 ? e : 0.0;
                    else
                        r2[a][b] += e * diff * diff;
                }
        }
        __syncthreads();
    }
}

// Grid (T): tile t of the lower triangle of C.
template <bool MIXED>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_fit_cov(const double* __restrict__ X,    // (N, D)
             const double* __restrict__ eta,  // (D)
             double scale, double noise, int64_t N, int D, uint64_t cat_mask,
             double* __restrict__ C) {  // (N, N)
    __shared__ double lds[FIT_TILE * FIT_T_PITCH];
    __shared__ double et[64];
    static_assert(FIT_X_DOUBLES <= FIT_TILE * FIT_T_PITCH, "the X tiles fit the transpose");
    double* xi = lds;
    double* xj = lds + FIT_TILE * FIT_PITCH;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int ti, tj;
    fit_tile_of(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * FIT_TILE, j0 = (int64_t)tj * FIT_TILE;
    if (tid < 64) et[tid] = tid < D ? eta[tid] : 0.0;
    // fit_r2's first barrier publishes et.

    double r2[4][4];
    fit_r2<MIXED>(X, N, D, i0, j0, et, cat_mask, xi, xj, r2);

#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int il = ty + 16 * a, jl = tx + 16 * b;
            const int64_t i = i0 + il, j = j0 + jl;
            const double u = sqrt(5.0 * r2[a][b]);
            double v = scale * (exp(-u) * ((5.0 / 3.0) * r2[a][b] + u + 1.0));
            if (i == j) v += noise;
            if (i < N && j < N) C[i * N + j] = v;
            if (ti != tj) lds[jl * FIT_T_PITCH + il] = v;
        }
    if (ti == tj) return;  // uniform over the workgroup
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int jl = ty + 16 * a, il = tx + 16 * b;
            const int64_t i = i0 + il, j = j0 + jl;
            if (i < N && j < N) C[j * N + i] = lds[jl * FIT_T_PITCH + il];
        }
}

// Grid (T): the record of tile t, part[t * (D + 2) ..]: D lengthscale sums,
// sum A m52, sum A_ii.
template <bool MIXED>
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_fit_grad(const double* __restrict__ X,      // (N, D)
              const double* __restrict__ eta,    // (D)
              const double* __restrict__ alpha,  // (N)
              const double* __restrict__ Cinv,   // (N, N)
              double scale, int64_t N, int D, uint64_t cat_mask,
              double* __restrict__ part) {  // (T, D + 2)
    __shared__ double xs[FIT_X_DOUBLES];
    __shared__ double et[64];
    __shared__ double red[GP_WAVES][FIT_CHUNK];
    __shared__ double red1[GP_WAVES];
    double* xi = xs;
    double* xj = xs + FIT_TILE * FIT_PITCH;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int lane = tid & 63, wave = tid >> 6;
    int ti, tj;
    fit_tile_of(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * FIT_TILE, j0 = (int64_t)tj * FIT_TILE;
    if (tid < 64) et[tid] = tid < D ? eta[tid] : 0.0;

    double W[4][4];
    fit_r2<MIXED>(X, N, D, i0, j0, et, cat_mask, xi, xj, W);  // r2, W from here on

    const double weight = ti != tj ? 2.0 : 1.0;
    double al_i[4], al_j[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * a;
        al_i[a] = i < N ? alpha[i] : 0.0;
        al_j[a] = j < N ? alpha[j] : 0.0;
    }
    double s_am = 0.0, s_tr = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            const double r2 = W[a][b];
            double w = 0.0;
            if (i < N && j < N) {
                const double u = sqrt(5.0 * r2);
                const double eu = exp(-u);
                const double A = al_i[a] * al_j[b] - Cinv[i * N + j];
                s_am += A * (eu * ((5.0 / 3.0) * r2 + u + 1.0));
                if (i == j) s_tr += A;
                w = weight * (0.5 * scale) * (A * ((-5.0 / 6.0) * (1.0 + u) * eu));
            }
            W[a][b] = w;
        }
    s_am *= weight;

    double* rec = part + (size_t)blockIdx.x * (D + 2);
    for (int d0 = 0; d0 < D; d0 += FIT_CHUNK) {
        fit_stage(X, N, D, i0, j0, d0, xi, xj);
        __syncthreads();
        double acc[FIT_CHUNK];
#pragma unroll
        for (int c = 0; c < FIT_CHUNK; ++c) {
            acc[c] = 0.0;
            if (d0 + c < D) {  // uniform
                double vi[4], vj[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    vi[a] = xi[(ty + 16 * a) * FIT_PITCH + c];
                    vj[a] = xj[(tx + 16 * a) * FIT_PITCH + c];
                }
                bool cat = false;
                if constexpr (MIXED) cat = gp_is_cat(cat_mask, d0 + c);
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const double diff = vi[a] - vj[b];
                        if (MIXED && cat)
                            s += diff != 0.0 ? W[a][b] : 0.0;
                        else
                            s += W[a][b] * (diff * diff);
                    }
                acc[c] = s;
            }
        }
#pragma unroll
        for (int c = 0; c < FIT_CHUNK; ++c) {
            double v = acc[c];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
            if (lane == 0) red[wave][c] = v;
        }
        __syncthreads();  // red is complete; the X tiles are free again
        if (tid < FIT_CHUNK && d0 + tid < D) {
            double v = red[0][tid];
            for (int w = 1; w < GP_WAVES; ++w) v += red[w][tid];
            rec[d0 + tid] = v;
        }
        // The next chunk's first barrier (after its staging, which does not
        // touch red) orders these reads before its writes of red.
    }
    const double am = gp_block_sum(s_am, red1);
    const double tr = gp_block_sum(s_tr, red1);
    if (tid == 0) {
        rec[D] = am;
        rec[D + 1] = tr;
    }
}

// One workgroup: out[0] = loss, out[1 .. D + 3) = its gradient in the raw
// (log) parameters eta (D), scale, noise.
__global__ void __launch_bounds__(GP_BLOCK)
k_gp_fit_grad_finish(const double* __restrict__ part,   // (T, D + 2)
                     const double* __restrict__ eta,    // (D)
                     const double* __restrict__ y,      // (N)
                     const double* __restrict__ alpha,  // (N)
                     const double* __restrict__ L,      // (N, N)
                     double scale, double noise, double noise_raw, int deterministic,
                     int64_t N, int D, int64_t T,
                     double* __restrict__ out) {  // (D + 3)
    __shared__ double slice_sums[GP_BLOCK];
    __shared__ double sums[66];
    __shared__ double red[GP_WAVES];
    const int tid = threadIdx.x;
    const int W = D + 2;
    // Two levels, both in tile order: slice s of the GP_BLOCK / W >= 3 slices
    // adds its run of consecutive tiles, then the slices are added in order.
    // The runs depend on T and D alone.
    const int n_slices = GP_BLOCK / W;
    const int slice = tid / W, comp = tid % W;
    if (slice < n_slices) {
        const int64_t per = (T + n_slices - 1) / n_slices;
        const int64_t t1 = min((int64_t)(slice + 1) * per, T);
        double a = 0.0;
        for (int64_t t = slice * per; t < t1; ++t) a += part[t * W + comp];
        slice_sums[tid] = a;
    }
    __syncthreads();
    if (tid < W) {
        double a = slice_sums[tid];
        for (int s = 1; s < n_slices; ++s) a += slice_sums[s * W + tid];
        sums[tid] = a;
    }
    double ya = 0.0, ld = 0.0;
    for (int64_t i = tid; i < N; i += GP_BLOCK) {
        ya += y[i] * alpha[i];
        ld += log(L[i * N + i]);
    }
    const double y_alpha = gp_block_sum(ya, red);
    const double half_logdet = gp_block_sum(ld, red);  // its barriers publish sums
    if (tid < D) {
        const double e = eta[tid];
        out[1 + tid] = -(sums[tid] + (0.1 / (e * e) - 0.1)) * e;
    }
    if (tid == 0) {
        double prior = 0.0;
        for (int d = 0; d < D; ++d) prior -= 0.1 / eta[d] + 0.1 * eta[d];
        prior += (log(scale) - scale) + (0.1 * log(noise) - 30.0 * noise);
        const double mll = -half_logdet - 0.5 * y_alpha;
        out[0] = -mll - prior;
        out[1 + D] = -(0.5 * sums[D] + (1.0 / scale - 1.0)) * scale;
        out[2 + D] = deterministic
                         ? 0.0
                         : -(0.5 * sums[D + 1] + (0.1 / noise - 30.0)) * noise_raw;
    }
}

// Session over the torch-owned X (N, D) and y (N) of one fit (raw pointers;
// same HIP context); the caller keeps the tensors alive. The record buffer,
// eta and the result come from the shared workspace, per call.
class GpFitSession {
  public:
    GpFitSession(int64_t X_ptr, int64_t y_ptr, int64_t N, int64_t D,
                 uint64_t cat_mask = 0)
        : X_(reinterpret_cast<const double*>(X_ptr)),
          y_(reinterpret_cast<const double*>(y_ptr)), N_(N), D_(D), cat_mask_(cat_mask) {
        const std::string who = "GpFitSession";
        gp_check_dims(who, D, cat_mask);
        if (N < 1 || N > INT32_MAX) throw std::runtime_error(who + ": N out of range");
        if (X_ == nullptr || y_ == nullptr) throw std::runtime_error(who + ": null pointer");
        const int64_t nt = (N + FIT_TILE - 1) / FIT_TILE;
        T_ = nt * (nt + 1) / 2;
        if (T_ > INT32_MAX) throw std::runtime_error(who + ": too many tiles");
    }

    void build_cov(const arr_f64& raw_params, double minimum_noise, bool deterministic,
                   int64_t C_ptr) {
        const Params p = params(raw_params, minimum_noise, deterministic);
        double* C = reinterpret_cast<double*>(C_ptr);
        if (C == nullptr) throw std::runtime_error("GpFitSession: null pointer");
        WsLayout lay;
        const auto s_eta = lay.add<double>(D_);
        char* base = g_ws.ensure_bytes(lay.bytes());
        double* d_eta = s_eta.in(base);
        hipStream_t st = g_ws.get_stream();
        g_ws.begin_uploads();
        g_ws.h2d(d_eta, p.eta, D_ * 8, st);
        const dim3 grid((unsigned)T_), block(GP_BLOCK);
        if (cat_mask_ != 0)
            hipLaunchKernelGGL(k_gp_fit_cov<true>, grid, block, 0, st, X_, d_eta, p.scale,
                               p.noise, N_, (int)D_, cat_mask_, C);
        else
            hipLaunchKernelGGL(k_gp_fit_cov<false>, grid, block, 0, st, X_, d_eta, p.scale,
                               p.noise, N_, (int)D_, cat_mask_, C);
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
    }

    // (loss, gradient (D + 2)).
    py::tuple grad(const arr_f64& raw_params, double minimum_noise, bool deterministic,
                   int64_t L_ptr, int64_t alpha_ptr, int64_t Cinv_ptr) {
        const Params p = params(raw_params, minimum_noise, deterministic);
        const double* L = reinterpret_cast<const double*>(L_ptr);
        const double* alpha = reinterpret_cast<const double*>(alpha_ptr);
        const double* Cinv = reinterpret_cast<const double*>(Cinv_ptr);
        if (L == nullptr || alpha == nullptr || Cinv == nullptr)
            throw std::runtime_error("GpFitSession: null pointer");
        const int D = (int)D_;
        WsLayout lay;
        const auto s_eta = lay.add<double>(D_), s_out = lay.add<double>(D_ + 3),
                   s_part = lay.add<double>((size_t)T_ * (D_ + 2));
        char* base = g_ws.ensure_bytes(lay.bytes());
        double *d_eta = s_eta.in(base), *d_out = s_out.in(base), *d_part = s_part.in(base);
        hipStream_t st = g_ws.get_stream();
        g_ws.begin_uploads();
        g_ws.h2d(d_eta, p.eta, D_ * 8, st);
        const dim3 grid((unsigned)T_), block(GP_BLOCK);
        if (cat_mask_ != 0)
            hipLaunchKernelGGL(k_gp_fit_grad<true>, grid, block, 0, st, X_, d_eta, alpha,
                               Cinv, p.scale, N_, D, cat_mask_, d_part);
        else
            hipLaunchKernelGGL(k_gp_fit_grad<false>, grid, block, 0, st, X_, d_eta, alpha,
                               Cinv, p.scale, N_, D, cat_mask_, d_part);
        hipLaunchKernelGGL(k_gp_fit_grad_finish, dim3(1), block, 0, st, d_part, d_eta, y_,
                           alpha, L, p.scale, p.noise, p.noise_raw, deterministic ? 1 : 0,
                           N_, D, T_, d_out);
        double host[67];
        HIP_CHECK(hipMemcpyAsync(host, d_out, (D_ + 3) * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        py::array_t<double> g(D_ + 2);
        std::memcpy(g.mutable_data(), host + 1, (D_ + 2) * 8);
        return py::make_tuple(host[0], g);
    }

  private:
    struct Params {
        double eta[64];
        double scale, noise, noise_raw;
    };

    // The natural parameters of raw (D + 2), as _loss_and_grad_numpy takes them.
    Params params(const arr_f64& raw, double minimum_noise, bool deterministic) const {
        if (raw.ndim() != 1 || raw.shape(0) != D_ + 2)
            throw std::runtime_error("GpFitSession: raw_params must hold D + 2 values");
        Params p;
        const double* r = raw.data();
        for (int64_t d = 0; d < D_; ++d) p.eta[d] = std::exp(r[d]);
        p.scale = std::exp(r[D_]);
        p.noise_raw = std::exp(r[D_ + 1]);
        p.noise = deterministic ? minimum_noise : p.noise_raw + minimum_noise;
        return p;
    }

    const double *X_, *y_;
    int64_t N_, D_, T_ = 0;
    uint64_t cat_mask_;
};
