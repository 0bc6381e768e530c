// K3 entry points: the truncnorm device library (truncnorm_device.h) exposed
// as three elementwise kernels and their numpy wrappers.
#pragma once

#include "hip_common.h"
#include "truncnorm_device.h"

// ---------------------------------------------------------------------------
// Elementwise truncnorm wrappers (golden-tested against scipy on GPU boxes).
// ---------------------------------------------------------------------------

__global__ void k_log_gauss_mass(const double* a, const double* b, double* out,
                                 int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tn::log_gauss_mass(a[i], b[i]);
}

__global__ void k_ppf(const double* q, const double* a, const double* b,
                      double* out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tn::trunc_ppf(q[i], a[i], b[i]);
}

__global__ void k_logpdf(const double* x, const double* a, const double* b,
                         const double* loc, const double* scale, double* out,
                         int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tn::trunc_logpdf(x[i], a[i], b[i], loc[i], scale[i]);
}

static py::array_t<double> elementwise3(const arr_f64& a, const arr_f64& b,
                                        const arr_f64& c, int which) {
    const int64_t n = a.size();
    if (b.size() != n || (which == 1 && c.size() != n))
        throw std::runtime_error("shape mismatch");
    py::array_t<double> out(n);
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto sa = L.add<double>(n), sb = L.add<double>(n), sc = L.add<double>(n),
               so = L.add<double>(n);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *da = sa.in(base), *db = sb.in(base), *dc = sc.in(base),
           *dout = so.in(base);
    g_ws.begin_uploads();
    g_ws.h2d(da, a.data(), n * 8, st);
    g_ws.h2d(db, b.data(), n * 8, st);
    if (which == 1) g_ws.h2d(dc, c.data(), n * 8, st);
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
    if (which == 0)
        hipLaunchKernelGGL(k_log_gauss_mass, dim3(grid), dim3(block), 0, st, da, db,
                           dout, n);
    else
        hipLaunchKernelGGL(k_ppf, dim3(grid), dim3(block), 0, st, dc, da, db, dout,
                           n);  // c = q
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), dout, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return out;
}

py::array_t<double> log_gauss_mass(const arr_f64& a, const arr_f64& b) {
    return elementwise3(a, b, a, 0);
}

py::array_t<double> truncnorm_ppf(const arr_f64& q, const arr_f64& a,
                                  const arr_f64& b) {
    return elementwise3(a, b, q, 1);
}

py::array_t<double> truncnorm_logpdf(const arr_f64& x, const arr_f64& a,
                                     const arr_f64& b, const arr_f64& loc,
                                     const arr_f64& scale) {
    const int64_t n = x.size();
    if (a.size() != n || b.size() != n || loc.size() != n || scale.size() != n)
        throw std::runtime_error("shape mismatch");
    py::array_t<double> out(n);
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto sx = L.add<double>(n), sa = L.add<double>(n), sb = L.add<double>(n),
               sl = L.add<double>(n), ss = L.add<double>(n), so = L.add<double>(n);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *dx = sx.in(base), *da = sa.in(base), *db = sb.in(base),
           *dl = sl.in(base), *ds = ss.in(base), *dout = so.in(base);
    g_ws.begin_uploads();
    g_ws.h2d(dx, x.data(), n * 8, st);
    g_ws.h2d(da, a.data(), n * 8, st);
    g_ws.h2d(db, b.data(), n * 8, st);
    g_ws.h2d(dl, loc.data(), n * 8, st);
    g_ws.h2d(ds, scale.data(), n * 8, st);
    const int block = 256;
    const int grid = (int)((n + block - 1) / block);
    hipLaunchKernelGGL(k_logpdf, dim3(grid), dim3(block), 0, st, dx, da, db, dl,
                       ds, dout, n);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), dout, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return out;
}
