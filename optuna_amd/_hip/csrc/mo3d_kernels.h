// K6a/K6b: exact 3-D hypervolume and greedy-HSSP kernels (fp64, gfx950).
// Host entry points: mo_host.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// ---------------------------------------------------------------------------
// K6a: exact 3-D hypervolume (minimization, ref-dominated region).
//
// Points sorted ascending by x. HV = sum_t slab_x(t) * A_t where A_t is the
// area in (y, z) dominated by the first t+1 points. A_t is evaluated by a
// y-ascending sweep that maintains the running min z over the points of the
// prefix — one THREAD per prefix t, with the y-sorted stream staged through
// LDS tiles so the O(N^2) scan reads each point once per 256-thread block.
// ---------------------------------------------------------------------------
__global__ void k_hv3d(const double* __restrict__ xs,   // (N) ascending
                       const double* __restrict__ yv,   // (N) y ascending
                       const double* __restrict__ zv,   // (N) z in y-order
                       const int32_t* __restrict__ rk,  // (N) x-rank in y-order
                       int64_t N, double ref_x, double ref_y, double ref_z,
                       double* __restrict__ out) {  // (N) per-prefix volumes
    __shared__ double t_y[256];
    __shared__ double t_z[256];
    __shared__ int32_t t_r[256];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double slab =
        (t < N) ? ((t + 1 < N ? xs[t + 1] : ref_x) - xs[t]) : 0.0;
    double minz = ref_z;
    double area = 0.0;
    for (int64_t base = 0; base < N; base += 256) {
        const int64_t m = min((int64_t)256, N - base);
        __syncthreads();
        if (threadIdx.x < m) {
            t_y[threadIdx.x] = yv[base + threadIdx.x];
            t_z[threadIdx.x] = zv[base + threadIdx.x];
            t_r[threadIdx.x] = rk[base + threadIdx.x];
        }
        // the y-interval right edge needs the NEXT point's y
        __syncthreads();
        for (int64_t q = 0; q < m; ++q) {
            if (t_r[q] <= t) minz = fmin(minz, t_z[q]);
            const int64_t g = base + q;
            const double y_next = (g + 1 < N) ? (q + 1 < m ? t_y[q + 1] : yv[g + 1]) : ref_y;
            area += (y_next - t_y[q]) * (ref_z - minz);
        }
    }
    if (t < N) out[t] = slab * area;
}

// ---------------------------------------------------------------------------
// K6b: batched greedy-HSSP contributions, 3 objectives. One workgroup per
// candidate. Key identity: the limited set {max(c, s) : s in S} keeps S's
// sorted orders under the per-coordinate clamp (max(c, .) is monotone), so
// the kernel reads GLOBALLY pre-sorted views of S — x-sorted xs, and the
// y-sorted (y, z, x-rank) triple — clamps them by the candidate, and runs the
// per-prefix staircase sweep directly. No per-candidate sort, no size cap;
// clamp ties produce zero-width slabs the sweep ignores.
// contribution(c | S) = incl(c) - HV3D(limited).
// ---------------------------------------------------------------------------
__global__ void k_hssp3d_contrib(const double* __restrict__ cand,  // (n, 3)
                                 const double* __restrict__ sx,    // (k) x asc
                                 const double* __restrict__ sxz,   // (k) z in x-order
                                 const double* __restrict__ sy,    // (k) y asc
                                 const double* __restrict__ syz,   // (k) z in y-order
                                 const int32_t* __restrict__ syr,  // (k) x-rank in y-order
                                 int64_t n, int64_t k, double ref_x,
                                 double ref_y, double ref_z,
                                 double* __restrict__ out) {  // (n)
    __shared__ double red[128];

    const int64_t c = blockIdx.x;
    const double cx = cand[c * 3], cy = cand[c * 3 + 1], cz = cand[c * 3 + 2];
    const double incl = (ref_x - cx) * (ref_y - cy) * (ref_z - cz);
    if (k == 0) {
        if (threadIdx.x == 0) out[c] = incl;
        return;
    }
    // Lanes stride over prefixes t; the y-stream is staged through LDS tiles
    // shared by the whole block.
    double total = 0.0;
    for (int64_t t = threadIdx.x; t < k; t += blockDim.x) {
        const double lx_t = fmax(cx, sx[t]);
        const double lx_next = (t + 1 < k) ? fmax(cx, sx[t + 1]) : ref_x;
        const double slab = lx_next - lx_t;
        if (slab <= 0.0) continue;
        double minz = ref_z;
        double area = 0.0;
        for (int64_t q = 0; q < k; ++q) {
            if (syr[q] <= t) minz = fmin(minz, fmax(cz, syz[q]));
            const double ly_q = fmax(cy, sy[q]);
            const double ly_next = (q + 1 < k) ? fmax(cy, sy[q + 1]) : ref_y;
            area += (ly_next - ly_q) * (ref_z - minz);
        }
        total += slab * area;
    }
    red[threadIdx.x] = total;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = incl - red[0];
}

// Masked argmax over the contributions, one block; the winner is marked taken
// so the next round's kernel skips it — only the 8-byte index crosses the bus
// per greedy round.
__global__ void k_hssp3d_argmax(const double* __restrict__ vals, int64_t n,
                                uint8_t* __restrict__ taken,
                                int64_t* __restrict__ out_idx) {
    __shared__ double red_v[256];
    __shared__ int64_t red_i[256];
    double best = -INFINITY;
    int64_t bi = -1;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        if (!taken[i] && vals[i] > best) {
            best = vals[i];
            bi = i;
        }
    }
    red_v[threadIdx.x] = best;
    red_i[threadIdx.x] = bi;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) {
            if (red_v[threadIdx.x + stride] > red_v[threadIdx.x] ||
                (red_v[threadIdx.x + stride] == red_v[threadIdx.x] &&
                 red_i[threadIdx.x + stride] >= 0 &&
                 (red_i[threadIdx.x] < 0 ||
                  red_i[threadIdx.x + stride] < red_i[threadIdx.x]))) {
                red_v[threadIdx.x] = red_v[threadIdx.x + stride];
                red_i[threadIdx.x] = red_i[threadIdx.x + stride];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_idx[0] = red_i[0];
        if (red_i[0] >= 0) taken[red_i[0]] = 1;
    }
}

// Device-side selected-set insertion: after the argmax picked winner w, put
// cand[w] into the x-sorted (x, z) and y-sorted (y, z, x-rank) views and bump
// the device k counter. One block; the O(k) shifts are a few hundred
// elements. Keeping the views on device lets the whole greedy run as a
// launch train with a single host sync at the end.
__global__ void k_hssp3d_insert(const double* __restrict__ cand,
                                const int64_t* __restrict__ idx,
                                double* __restrict__ sx, double* __restrict__ sxz,
                                double* __restrict__ sy, double* __restrict__ syz,
                                int32_t* __restrict__ syr,
                                int64_t* __restrict__ k_ptr,
                                int64_t* __restrict__ chosen,
                                int64_t* __restrict__ round_ptr) {
    // One block. The O(k) tail shifts run in parallel: every thread stages
    // its strided elements in registers, barriers, then writes them one slot
    // to the right (read-before-write is global across the block).
    __shared__ int64_t s_w, s_px, s_py, s_k;
    if (threadIdx.x == 0) {
        const int64_t w = idx[0];
        s_w = w;
        chosen[round_ptr[0]] = w;
        round_ptr[0] += 1;
        const int64_t k = k_ptr[0];
        s_k = k;
        if (w >= 0) {
            const double x = cand[w * 3], y = cand[w * 3 + 1];
            int64_t px = 0;
            while (px < k && sx[px] <= x) ++px;
            int64_t py = 0;
            while (py < k && sy[py] <= y) ++py;
            s_px = px;
            s_py = py;
            k_ptr[0] = k + 1;
        }
    }
    __syncthreads();
    const int64_t w = s_w;
    if (w < 0) return;
    const int64_t k = s_k, px = s_px, py = s_py;
    const double x = cand[w * 3], y = cand[w * 3 + 1], z = cand[w * 3 + 2];

    constexpr int MAXLOC = 32;  // supports k up to 32 * blockDim
    double rx_v[MAXLOC], rz_v[MAXLOC], ry_v[MAXLOC], ryz_v[MAXLOC];
    int32_t rr_v[MAXLOC];
    int nx = 0, ny = 0;
    for (int64_t i = px + threadIdx.x; i < k; i += blockDim.x) {
        rx_v[nx] = sx[i];
        rz_v[nx] = sxz[i];
        ++nx;
    }
    for (int64_t i = py + threadIdx.x; i < k; i += blockDim.x) {
        ry_v[ny] = sy[i];
        ryz_v[ny] = syz[i];
        // pre-bump the x-ranks shifting right of the x insertion point
        int32_t r = syr[i];
        rr_v[ny] = (r >= (int32_t)px) ? r + 1 : r;
        ++ny;
    }
    // ranks BEFORE py also need the bump; handle them in-place (no shift)
    __syncthreads();
    for (int64_t i = threadIdx.x; i < py; i += blockDim.x) {
        int32_t r = syr[i];
        if (r >= (int32_t)px) syr[i] = r + 1;
    }
    {
        int j = 0;
        for (int64_t i = px + threadIdx.x; i < k; i += blockDim.x, ++j) {
            sx[i + 1] = rx_v[j];
            sxz[i + 1] = rz_v[j];
        }
        j = 0;
        for (int64_t i = py + threadIdx.x; i < k; i += blockDim.x, ++j) {
            sy[i + 1] = ry_v[j];
            syz[i + 1] = ryz_v[j];
            syr[i + 1] = rr_v[j];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sx[px] = x;
        sxz[px] = z;
        sy[py] = y;
        syz[py] = z;
        syr[py] = (int32_t)px;
    }
}

// Contribution kernel variant reading k from device memory (launch-train mode).
__global__ void k_hssp3d_contrib_dk(const double* __restrict__ cand,
                                    const double* __restrict__ sx,
                                    const double* __restrict__ sxz,
                                    const double* __restrict__ sy,
                                    const double* __restrict__ syz,
                                    const int32_t* __restrict__ syr,
                                    int64_t n, const int64_t* __restrict__ k_ptr,
                                    double ref_x, double ref_y, double ref_z,
                                    double* __restrict__ out) {
    __shared__ double red[128];
    const int64_t k = k_ptr[0];
    const int64_t c = blockIdx.x;
    const double cx = cand[c * 3], cy = cand[c * 3 + 1], cz = cand[c * 3 + 2];
    const double incl = (ref_x - cx) * (ref_y - cy) * (ref_z - cz);
    if (k == 0) {
        if (threadIdx.x == 0) out[c] = incl;
        return;
    }
    double total = 0.0;
    for (int64_t t = threadIdx.x; t < k; t += blockDim.x) {
        const double lx_t = fmax(cx, sx[t]);
        const double lx_next = (t + 1 < k) ? fmax(cx, sx[t + 1]) : ref_x;
        const double slab = lx_next - lx_t;
        if (slab <= 0.0) continue;
        double minz = ref_z;
        double area = 0.0;
        for (int64_t q = 0; q < k; ++q) {
            if (syr[q] <= t) minz = fmin(minz, fmax(cz, syz[q]));
            const double ly_q = fmax(cy, sy[q]);
            const double ly_next = (q + 1 < k) ? fmax(cy, sy[q + 1]) : ref_y;
            area += (ly_next - ly_q) * (ref_z - minz);
        }
        total += slab * area;
    }
    red[threadIdx.x] = total;
    __syncthreads();
    for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = incl - red[0];
}
