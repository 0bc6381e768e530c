// K6c/K6d: exact 4-D hypervolume and greedy-HSSP contributions (fp64, gfx950).
//
// The 3-D per-prefix staircase sweep (k_hv3d) nested once more. Axes are
// (w, x, y, z) = columns 0..3. With the points ranked by a stable sort on w
// and, separately, on x:
//
//   HV4 = sum_t sum_u slab_w(t) * slab_x(u) * A(t, u)
//
// slab_w(t) = w[t+1] - w[t] (the last slab runs to ref_w), slab_x likewise,
// and A(t, u) is the (y, z) staircase area of the points with w-rank <= t AND
// x-rank <= u: walk the y-ascending stream, keep the running min of z over the
// points that pass both rank tests, add (y_next - y) * (ref_z - minz). Tied
// coordinates give zero-width slabs; dominated and duplicate points add
// nothing, so no Pareto filter is needed.
//
// No floating-point atomics: every sum has a fixed order, so two runs on the
// same input are bit-identical and the greedy order is reproducible.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

static constexpr int HV4_TILE = 16;                      // pair tile edge
static constexpr int HV4_THREADS = HV4_TILE * HV4_TILE;  // = y-stream tile
static constexpr int HSSP4_THREADS = 256;
// Insert kernel register staging: MAXLOC slots x HSSP4_THREADS lanes bounds
// the selected-set size the session accepts. The contribution kernels stage
// the y-stream in LDS (24 B per entry), which the same bound keeps at 48 KiB.
static constexpr int HSSP4_MAXLOC = 8;
static constexpr int64_t HSSP4_MAX_K = (int64_t)HSSP4_MAXLOC * HSSP4_THREADS;

// Fixed-order block sum over HV4_THREADS / HSSP4_THREADS (= 256) lanes.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
        __syncthreads();
    }
    return red[0];
}

// One thread per (t, u) pair, one 16x16 pair tile per block. The y-stream
// (dy, z, w-rank, x-rank) is staged through 256-entry LDS tiles shared by the
// block; every lane reads the same LDS address (broadcast, no bank conflicts).
// Threads whose slab product is zero (ties, or pairs past N) are masked, never
// returned early: they still reach every barrier of the tile loop.
__global__ __launch_bounds__(HV4_THREADS)
void k_hv4d(const double* __restrict__ ws,    // (N) w ascending
            const double* __restrict__ xs,    // (N) x ascending
            const double* __restrict__ yv,    // (N) y ascending
            const double* __restrict__ zv,    // (N) z in y-order
            const int32_t* __restrict__ rw,   // (N) w-rank in y-order
            const int32_t* __restrict__ rx,   // (N) x-rank in y-order
            int64_t N, double ref_w, double ref_x, double ref_y, double ref_z,
            double* __restrict__ out) {  // (gridDim.y * gridDim.x) partials
    __shared__ double2 t_dh[HV4_THREADS];  // (dy, ref_z - z)
    __shared__ int2 t_r[HV4_THREADS];      // (w-rank, x-rank)
    __shared__ double red[HV4_THREADS];

    const int64_t t = (int64_t)blockIdx.y * HV4_TILE + threadIdx.x / HV4_TILE;
    const int64_t u = (int64_t)blockIdx.x * HV4_TILE + threadIdx.x % HV4_TILE;
    double slab = 0.0;
    if (t < N && u < N) {
        const double sw = (t + 1 < N ? ws[t + 1] : ref_w) - ws[t];
        const double sx = (u + 1 < N ? xs[u + 1] : ref_x) - xs[u];
        slab = sw * sx;
    }
    const bool live = slab > 0.0;
    const int32_t ti = live ? (int32_t)t : -1;  // dead lanes pass no rank test
    const int32_t ui = live ? (int32_t)u : -1;
    // ref_z - min(z) == max(ref_z - z) bit for bit (rounding is monotone), so
    // the sweep keeps the running max of the staged heights
    double h = 0.0;
    double area = 0.0;
    for (int64_t base = 0; base < N; base += HV4_THREADS) {
        const int64_t m = min((int64_t)HV4_THREADS, N - base);
        __syncthreads();
        if ((int64_t)threadIdx.x < m) {
            const int64_t g = base + threadIdx.x;
            const double y_next = (g + 1 < N) ? yv[g + 1] : ref_y;
            t_dh[threadIdx.x] = make_double2(y_next - yv[g], ref_z - zv[g]);
            t_r[threadIdx.x] = make_int2(rw[g], rx[g]);
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < (int)m; ++q) {
            const double2 dh = t_dh[q];
            const int2 r = t_r[q];
            h = fmax(h, (r.x <= ti && r.y <= ui) ? dh.y : 0.0);
            area += dh.x * h;
        }
    }
    const double total = block_sum_256(live ? slab * area : 0.0, red);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// Number of entries <= v in the ascending array s[0..k) (upper bound).
__device__ __forceinline__ int64_t upper_bound_f64(const double* __restrict__ s,
                                                   int64_t k, double v) {
    int64_t lo = 0, hi = k;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (s[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// contribution(c | S) = incl(c) - HV4({max(c, s) : s in S}); one workgroup per
// candidate. The clamp identity documented above k_hssp3d_contrib holds per
// axis, so the selected set's global sorted views (w ascending, x ascending,
// and the y-ascending stream (y, z, w-rank, x-rank)) stay sorted under the
// clamp and no per-candidate sort is needed.
//
// Everything at or below the clamp collapses into one slab: a binary search of
// c.w / c.x in the sorted views restricts the pair range to t >= tlo, u >= ulo
// (about three quarters of a non-dominated candidate's pairs are dead).
// Threads stride over the flattened live pairs and sweep the k-long stream,
// which is staged ONCE per block in LDS, already clamped by the candidate:
// (dy, ref_z - z) as doubles and the two ranks as int32, 24 B per entry (k is
// bounded by HSSP4_MAX_K). The block tree-reduces its partial sums in a fixed
// order.
__device__ __forceinline__ void hssp4d_contrib_body(
    const double* __restrict__ cand,    // (n, 4)
    const double* __restrict__ sw,      // (k) w ascending
    const double* __restrict__ sx,      // (k) x ascending
    const double* __restrict__ sy,      // (k) y ascending
    const double* __restrict__ syz,     // (k) z in y-order
    const int32_t* __restrict__ syrw,   // (k) w-rank in y-order
    const int32_t* __restrict__ syrx,   // (k) x-rank in y-order
    int64_t k, int64_t kcap, double ref_w, double ref_x, double ref_y,
    double ref_z, double* __restrict__ out, double2* smem, double* red) {
    const int64_t c = blockIdx.x;
    const double cw = cand[c * 4], cx = cand[c * 4 + 1];
    const double cy = cand[c * 4 + 2], cz = cand[c * 4 + 3];
    const double incl = (ref_w - cw) * (ref_x - cx) * (ref_y - cy) * (ref_z - cz);
    if (k == 0) {  // uniform across the block: no barrier is skipped
        if (threadIdx.x == 0) out[c] = incl;
        return;
    }
    double2* l_dh = smem;                               // (dy, ref_z - z)
    int2* l_r = reinterpret_cast<int2*>(l_dh + kcap);  // (w-rank, x-rank)
    for (int64_t q = threadIdx.x; q < k; q += blockDim.x) {
        const double y_next = (q + 1 < k) ? fmax(cy, sy[q + 1]) : ref_y;
        l_dh[q] = make_double2(y_next - fmax(cy, sy[q]), ref_z - fmax(cz, syz[q]));
        l_r[q] = make_int2(syrw[q], syrx[q]);
    }
    __syncthreads();

    const int64_t nw_le = upper_bound_f64(sw, k, cw);
    const int64_t nx_le = upper_bound_f64(sx, k, cx);
    const int64_t tlo = nw_le > 0 ? nw_le - 1 : 0;
    const int64_t ulo = nx_le > 0 ? nx_le - 1 : 0;
    // k <= HSSP4_MAX_K keeps the pair count inside int32 (cheap div/mod)
    const int nu = (int)(k - ulo);
    const int n_pairs = (int)(k - tlo) * nu;
    const int kk = (int)k;
    // slab product of flattened pair p, and its (t, u); dead pairs (past the
    // range, or zero width) get ranks no stream entry passes
    auto pair = [&](int p, int32_t& ti, int32_t& ui) -> double {
        ti = ui = -1;
        if (p >= n_pairs) return 0.0;
        const int64_t t = tlo + p / nu;
        const int64_t u = ulo + p % nu;
        const double slab_w =
            (t + 1 < k ? fmax(cw, sw[t + 1]) : ref_w) - fmax(cw, sw[t]);
        const double slab_x =
            (u + 1 < k ? fmax(cx, sx[u + 1]) : ref_x) - fmax(cx, sx[u]);
        const double slab = slab_w * slab_x;
        if (!(slab > 0.0)) return 0.0;
        ti = (int32_t)t;
        ui = (int32_t)u;
        return slab;
    };
    // Two pairs per thread share every LDS read of the stream and give the
    // sweep two independent dependency chains. No barrier inside this loop.
    double total = 0.0;
    for (int p = threadIdx.x; p < n_pairs; p += 2 * HSSP4_THREADS) {
        int32_t ti0, ui0, ti1, ui1;
        const double slab0 = pair(p, ti0, ui0);
        const double slab1 = pair(p + HSSP4_THREADS, ti1, ui1);
        if (ti0 < 0 && ti1 < 0) continue;
        // ref_z - min(z) == max(ref_z - z) bit for bit (rounding is monotone),
        // so the sweep keeps the running max of the staged heights
        double h0 = 0.0, h1 = 0.0, area0 = 0.0, area1 = 0.0;
#pragma unroll 4
        for (int q = 0; q < kk; ++q) {
            const double2 dh = l_dh[q];
            const int2 r = l_r[q];
            h0 = fmax(h0, (r.x <= ti0 && r.y <= ui0) ? dh.y : 0.0);
            h1 = fmax(h1, (r.x <= ti1 && r.y <= ui1) ? dh.y : 0.0);
            area0 += dh.x * h0;
            area1 += dh.x * h1;
        }
        total += slab0 * area0;
        total += slab1 * area1;
    }
    const double sum = block_sum_256(total, red);
    if (threadIdx.x == 0) out[c] = incl - sum;
}

__global__ __launch_bounds__(HSSP4_THREADS)
void k_hssp4d_contrib(const double* __restrict__ cand, const double* __restrict__ sw,
                      const double* __restrict__ sx, const double* __restrict__ sy,
                      const double* __restrict__ syz, const int32_t* __restrict__ syrw,
                      const int32_t* __restrict__ syrx, int64_t k, int64_t kcap,
                      double ref_w, double ref_x, double ref_y, double ref_z,
                      double* __restrict__ out) {
    extern __shared__ double2 hssp4_smem[];
    __shared__ double red[HSSP4_THREADS];
    hssp4d_contrib_body(cand, sw, sx, sy, syz, syrw, syrx, k, kcap, ref_w, ref_x,
                        ref_y, ref_z, out, hssp4_smem, red);
}

// Variant reading k from device memory (launch-train mode).
__global__ __launch_bounds__(HSSP4_THREADS)
void k_hssp4d_contrib_dk(const double* __restrict__ cand, const double* __restrict__ sw,
                         const double* __restrict__ sx, const double* __restrict__ sy,
                         const double* __restrict__ syz, const int32_t* __restrict__ syrw,
                         const int32_t* __restrict__ syrx,
                         const int64_t* __restrict__ k_ptr, int64_t kcap,
                         double ref_w, double ref_x, double ref_y, double ref_z,
                         double* __restrict__ out) {
    extern __shared__ double2 hssp4_smem[];
    __shared__ double red[HSSP4_THREADS];
    hssp4d_contrib_body(cand, sw, sx, sy, syz, syrw, syrx, k_ptr[0], kcap, ref_w,
                        ref_x, ref_y, ref_z, out, hssp4_smem, red);
}

// Device-side selected-set insertion, the analogue of k_hssp3d_insert: after
// the argmax picked winner idx[0], put cand[idx] into the w-sorted and
// x-sorted views and the y-sorted (y, z, w-rank, x-rank) stream, and bump the
// device k counter. One block. Insertion points are the counts of entries
// <= the new value (integer LDS counters); tails are staged in registers,
// then written one slot to the right after a barrier; w-ranks >= pw and
// x-ranks >= px are bumped in every stream entry, moved or not. Holds for
// k <= HSSP4_MAX_K, which the session enforces.
__global__ __launch_bounds__(HSSP4_THREADS)
void k_hssp4d_insert(const double* __restrict__ cand, const int64_t* __restrict__ idx,
                     double* __restrict__ sw, double* __restrict__ sx,
                     double* __restrict__ sy, double* __restrict__ syz,
                     int32_t* __restrict__ syrw, int32_t* __restrict__ syrx,
                     int64_t* __restrict__ k_ptr, int64_t* __restrict__ chosen,
                     int64_t* __restrict__ round_ptr) {
    __shared__ int s_pw, s_px, s_py;
    const int64_t w_idx = idx[0];
    const int64_t k = k_ptr[0];
    if (threadIdx.x == 0) {
        s_pw = 0;
        s_px = 0;
        s_py = 0;
    }
    __syncthreads();  // every thread has read idx/k before thread 0 updates them
    if (threadIdx.x == 0) {
        chosen[round_ptr[0]] = w_idx;
        round_ptr[0] += 1;
        if (w_idx >= 0) k_ptr[0] = k + 1;
    }
    if (w_idx < 0) return;  // uniform across the block
    const double w = cand[w_idx * 4], x = cand[w_idx * 4 + 1];
    const double y = cand[w_idx * 4 + 2], z = cand[w_idx * 4 + 3];
    int cw = 0, cx = 0, cy = 0;
    for (int64_t i = threadIdx.x; i < k; i += blockDim.x) {
        cw += sw[i] <= w;
        cx += sx[i] <= x;
        cy += sy[i] <= y;
    }
    if (cw) atomicAdd(&s_pw, cw);
    if (cx) atomicAdd(&s_px, cx);
    if (cy) atomicAdd(&s_py, cy);
    __syncthreads();
    const int64_t pw = s_pw, px = s_px, py = s_py;

    double r_w[HSSP4_MAXLOC], r_x[HSSP4_MAXLOC], r_y[HSSP4_MAXLOC], r_z[HSSP4_MAXLOC];
    int32_t r_rw[HSSP4_MAXLOC], r_rx[HSSP4_MAXLOC];
#pragma unroll
    for (int j = 0; j < HSSP4_MAXLOC; ++j) {
        const int64_t off = (int64_t)threadIdx.x + (int64_t)j * HSSP4_THREADS;
        if (pw + off < k) r_w[j] = sw[pw + off];
        if (px + off < k) r_x[j] = sx[px + off];
        if (py + off < k) {
            r_y[j] = sy[py + off];
            r_z[j] = syz[py + off];
            const int32_t a = syrw[py + off], b = syrx[py + off];
            r_rw[j] = (a >= (int32_t)pw) ? a + 1 : a;
            r_rx[j] = (b >= (int32_t)px) ? b + 1 : b;
        }
    }
    // stream entries before py do not move but their ranks may bump; the
    // ranges [0, py) and [py, k) are disjoint, so this needs no barrier of
    // its own against the staging reads above
    for (int64_t i = threadIdx.x; i < py; i += blockDim.x) {
        const int32_t a = syrw[i], b = syrx[i];
        if (a >= (int32_t)pw) syrw[i] = a + 1;
        if (b >= (int32_t)px) syrx[i] = b + 1;
    }
    __syncthreads();  // all tails are in registers before any slot is overwritten
#pragma unroll
    for (int j = 0; j < HSSP4_MAXLOC; ++j) {
        const int64_t off = (int64_t)threadIdx.x + (int64_t)j * HSSP4_THREADS;
        if (pw + off < k) sw[pw + off + 1] = r_w[j];
        if (px + off < k) sx[px + off + 1] = r_x[j];
        if (py + off < k) {
            sy[py + off + 1] = r_y[j];
            syz[py + off + 1] = r_z[j];
            syrw[py + off + 1] = r_rw[j];
            syrx[py + off + 1] = r_rx[j];
        }
    }
    if (threadIdx.x == 0) {  // slots pw/px/py: read above, written by nobody else
        sw[pw] = w;
        sx[px] = x;
        sy[py] = y;
        syz[py] = z;
        syrw[py] = (int32_t)pw;
        syrx[py] = (int32_t)px;
    }
}
