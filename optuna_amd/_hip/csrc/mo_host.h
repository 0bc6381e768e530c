// Host entry points of the 3- and 4-objective hypervolume and greedy HSSP.
// The kernels and the algorithm notes live in mo3d_kernels.h and
// mo4d_kernels.h.
#pragma once

#include "hip_common.h"
#include "mo3d_kernels.h"
#include "mo4d_kernels.h"

// 3-D hypervolume of x-lexsorted points (all strictly inside ref).
double hv3d(const arr_f64& pts, double ref_x, double ref_y, double ref_z) {
    if (pts.ndim() != 2 || pts.shape(1) != 3)
        throw std::runtime_error("hv3d: pts must be (N, 3)");
    const int64_t N = pts.shape(0);
    if (N == 0) return 0.0;
    // Host prep: y-order view (N log N — negligible next to the N^2 sweep).
    std::vector<double> xs(N), yv(N), zv(N);
    std::vector<int32_t> rk(N);
    std::vector<int64_t> order(N);
    const double* P = pts.data();
    for (int64_t i = 0; i < N; ++i) {
        xs[i] = P[i * 3];
        order[i] = i;
    }
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return P[a * 3 + 1] < P[b * 3 + 1];
    });
    for (int64_t i = 0; i < N; ++i) {
        yv[i] = P[order[i] * 3 + 1];
        zv[i] = P[order[i] * 3 + 2];
        rk[i] = (int32_t)order[i];
    }
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto s_xs = L.add<double>(N), s_yv = L.add<double>(N),
               s_zv = L.add<double>(N), s_out = L.add<double>(N);
    const auto s_rk = L.add<int32_t>(N);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *d_xs = s_xs.in(base), *d_yv = s_yv.in(base), *d_zv = s_zv.in(base),
           *d_out = s_out.in(base);
    int32_t* d_rk = s_rk.in(base);
    g_ws.begin_uploads();
    g_ws.h2d(d_xs, xs.data(), N * 8, st);
    g_ws.h2d(d_yv, yv.data(), N * 8, st);
    g_ws.h2d(d_zv, zv.data(), N * 8, st);
    g_ws.h2d(d_rk, rk.data(), N * 4, st);
    const int64_t blocks = (N + 255) / 256;
    hipLaunchKernelGGL(k_hv3d, dim3((unsigned)blocks), dim3(256), 0, st, d_xs,
                       d_yv, d_zv, d_rk, N, ref_x, ref_y, ref_z, d_out);
    std::vector<double> host_out(N);
    HIP_CHECK(hipMemcpyAsync(host_out.data(), d_out, N * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double hv = 0.0;
    for (double v : host_out) hv += v;
    return hv;
}

// The sorted selected-set views of the 3-D greedy, k entries each: x-sorted
// (x, z) and y-sorted (y, z, x-rank).
struct Views3d {
    WsSlot<double> sx, sxz, sy, syz;
    WsSlot<int32_t> syr;
    Views3d(WsLayout& L, size_t k)
        : sx(L.add<double>(k)), sxz(L.add<double>(k)), sy(L.add<double>(k)),
          syz(L.add<double>(k)), syr(L.add<int32_t>(k)) {}

    void upload(char* base, const arr_f64& hsx, const arr_f64& hsxz,
                const arr_f64& hsy, const arr_f64& hsyz, const arr_i32& hsyr,
                hipStream_t st) const {
        const size_t k = hsx.size();
        g_ws.h2d(sx.in(base), hsx.data(), k * 8, st);
        g_ws.h2d(sxz.in(base), hsxz.data(), k * 8, st);
        g_ws.h2d(sy.in(base), hsy.data(), k * 8, st);
        g_ws.h2d(syz.in(base), hsyz.data(), k * 8, st);
        g_ws.h2d(syr.in(base), hsyr.data(), k * 4, st);
    }
};

// Per-candidate greedy-HSSP contributions against the current selected set,
// passed as pre-sorted views (x-sorted xs/z, y-sorted y/z/x-rank).
py::array_t<double> hssp3d_contrib(const arr_f64& cand, const arr_f64& sx,
                                   const arr_f64& sxz, const arr_f64& sy,
                                   const arr_f64& syz, const arr_i32& syr,
                                   double ref_x, double ref_y, double ref_z) {
    if (cand.ndim() != 2 || cand.shape(1) != 3)
        throw std::runtime_error("hssp3d_contrib: cand must be (n, 3)");
    const int64_t n = cand.shape(0);
    const int64_t k = sx.size();
    if ((int64_t)sy.size() != k || (int64_t)syz.size() != k ||
        (int64_t)syr.size() != k || (int64_t)sxz.size() != k)
        throw std::runtime_error("hssp3d_contrib: ragged sorted views");
    py::array_t<double> out(n);
    if (n == 0) return out;
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto s_cand = L.add<double>((size_t)n * 3);
    const Views3d v(L, k);
    const auto s_out = L.add<double>(n);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *d_cand = s_cand.in(base), *d_out = s_out.in(base);
    g_ws.begin_uploads();
    g_ws.h2d(d_cand, cand.data(), (size_t)n * 3 * 8, st);
    v.upload(base, sx, sxz, sy, syz, syr, st);
    hipLaunchKernelGGL(k_hssp3d_contrib, dim3((unsigned)n), dim3(128), 0, st,
                       d_cand, v.sx.in(base), v.sxz.in(base), v.sy.in(base),
                       v.syz.in(base), v.syr.in(base), n, k, ref_x, ref_y, ref_z,
                       d_out);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}

// What the greedy-HSSP sessions share: the candidates, the contributions, the
// round's winner and the taken-mask stay resident (out | idx | taken is one
// allocation), and the selected-set bookkeeping of a launch train sits in the
// workspace as k | round | chosen.
class HsspSession {
  protected:
    HsspSession(const char* who, const arr_f64& cand, int64_t dims) {
        if (cand.ndim() != 2 || cand.shape(1) != dims)
            throw std::runtime_error(std::string(who) + ": cand must be (n, " +
                                     std::to_string(dims) + ")");
        n_ = cand.shape(0);
        hipStream_t st = g_ws.get_stream();
        WsLayout L;
        const auto s_out = L.add<double>(n_);
        const auto s_idx = L.add<int64_t>(1);
        const auto s_taken = L.add<uint8_t>(n_);
        d_cand_.reserve((size_t)n_ * dims);
        state_.reserve(L.bytes());
        d_out_ = s_out.in(state_.ptr);
        d_idx_ = s_idx.in(state_.ptr);
        d_taken_ = s_taken.in(state_.ptr);
        HIP_CHECK(hipMemcpyAsync(d_cand_.ptr, cand.data(), (size_t)n_ * dims * 8,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_taken_, 0, n_, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // k | round (zeroed together at the start of a train) and the winners.
    struct Train {
        WsSlot<int64_t> k_round, chosen;
        Train(WsLayout& L, int64_t rounds)
            : k_round(L.add<int64_t>(2)), chosen(L.add<int64_t>(rounds)) {}
    };

    // Every round of a train launches the same kernels with identical
    // arguments (k and the round index live in device memory), so the round
    // is captured once as a linear hipGraph and replayed `rounds` times at
    // graph-launch cost. Graph and exec are destroyed before an error is
    // reported.
    template <typename F>
    static void replay_captured(hipStream_t st, int64_t rounds, F enqueue_round) {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        enqueue_round();
        HIP_CHECK(hipStreamEndCapture(st, &graph));
        hipError_t err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        for (int64_t r = 0; r < rounds && err == hipSuccess; ++r)
            err = hipGraphLaunch(exec, st);
        if (exec) (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        HIP_CHECK(err);
    }

    // The winners of a finished train; the ONE host sync of a run.
    py::array_t<int64_t> download_chosen(const int64_t* d_chosen, int64_t rounds,
                                         hipStream_t st) {
        py::array_t<int64_t> out(rounds);
        HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_chosen, rounds * 8,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return out;
    }

    int64_t n_ = 0;
    DeviceBuffer<double> d_cand_;
    DeviceBuffer<char> state_;  // out | idx | taken
    double* d_out_ = nullptr;
    int64_t* d_idx_ = nullptr;
    uint8_t* d_taken_ = nullptr;
};

// Greedy-HSSP driver, 3 objectives. run() keeps the selected-set views on the
// device; round() is the stepwise form: each call re-uploads the (small,
// growing) sorted views and pulls back ONE index.
class Hssp3dSession : HsspSession {
  public:
    Hssp3dSession(const arr_f64& cand, double rx, double ry, double rz)
        : HsspSession("Hssp3dSession", cand, 3), rx_(rx), ry_(ry), rz_(rz) {}

    // Launch-train greedy: subset_size rounds of contrib→argmax→insert
    // enqueued back-to-back with device-resident views, ONE host sync.
    py::array_t<int64_t> run(int64_t subset_size) {
        if (subset_size > n_) subset_size = n_;
        hipStream_t st = g_ws.get_stream();
        WsLayout L;
        const Views3d v(L, (size_t)subset_size + 1);
        const Train t(L, subset_size);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_sx = v.sx.in(base), *d_sxz = v.sxz.in(base), *d_sy = v.sy.in(base),
               *d_syz = v.syz.in(base);
        int32_t* d_syr = v.syr.in(base);
        int64_t* d_k = t.k_round.in(base);
        int64_t* d_round = d_k + 1;
        int64_t* d_chosen = t.chosen.in(base);
        HIP_CHECK(hipMemsetAsync(d_k, 0, 16, st));
        replay_captured(st, subset_size, [&] {
            hipLaunchKernelGGL(k_hssp3d_contrib_dk, dim3((unsigned)n_), dim3(128),
                               0, st, d_cand_.ptr, d_sx, d_sxz, d_sy, d_syz, d_syr,
                               n_, d_k, rx_, ry_, rz_, d_out_);
            hipLaunchKernelGGL(k_hssp3d_argmax, dim3(1), dim3(256), 0, st, d_out_,
                               n_, d_taken_, d_idx_);
            hipLaunchKernelGGL(k_hssp3d_insert, dim3(1), dim3(64), 0, st,
                               d_cand_.ptr, d_idx_, d_sx, d_sxz, d_sy, d_syz, d_syr,
                               d_k, d_chosen, d_round);
        });
        return download_chosen(d_chosen, subset_size, st);
    }

    int64_t round(const arr_f64& sx, const arr_f64& sxz, const arr_f64& sy,
                  const arr_f64& syz, const arr_i32& syr) {
        const int64_t k = sx.size();
        hipStream_t st = g_ws.get_stream();
        WsLayout L;
        const Views3d v(L, k);
        char* base = g_ws.ensure_bytes(L.bytes());
        g_ws.begin_uploads();
        v.upload(base, sx, sxz, sy, syz, syr, st);
        hipLaunchKernelGGL(k_hssp3d_contrib, dim3((unsigned)n_), dim3(128), 0,
                           st, d_cand_.ptr, v.sx.in(base), v.sxz.in(base),
                           v.sy.in(base), v.syz.in(base), v.syr.in(base), n_, k,
                           rx_, ry_, rz_, d_out_);
        hipLaunchKernelGGL(k_hssp3d_argmax, dim3(1), dim3(256), 0, st, d_out_,
                           n_, d_taken_, d_idx_);
        int64_t idx = -1;
        HIP_CHECK(hipMemcpyAsync(&idx, d_idx_, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return idx;
    }

  private:
    double rx_, ry_, rz_;
};

// 4-D hypervolume of points strictly inside ref, in any order. Host prep
// builds the three stable sorted views (N log N, negligible next to the N^3
// sweep); each block writes one partial and the host sums them in block order.
double hv4d(const arr_f64& pts, double ref_w, double ref_x, double ref_y,
            double ref_z) {
    if (pts.ndim() != 2 || pts.shape(1) != 4)
        throw std::runtime_error("hv4d: pts must be (N, 4)");
    const int64_t N = pts.shape(0);
    if (N == 0) return 0.0;
    if (N > (int64_t)65535 * HV4_TILE)
        throw std::runtime_error("hv4d: too many points");
    const double* P = pts.data();
    std::vector<int64_t> ow(N), ox(N), oy(N);
    for (int64_t i = 0; i < N; ++i) ow[i] = ox[i] = oy[i] = i;
    auto by_col = [&](int col) {
        return [P, col](int64_t a, int64_t b) { return P[a * 4 + col] < P[b * 4 + col]; };
    };
    std::stable_sort(ow.begin(), ow.end(), by_col(0));
    std::stable_sort(ox.begin(), ox.end(), by_col(1));
    std::stable_sort(oy.begin(), oy.end(), by_col(2));
    std::vector<double> ws(N), xs(N), yv(N), zv(N);
    std::vector<int32_t> rank_w(N), rank_x(N), rw(N), rx(N);
    for (int64_t i = 0; i < N; ++i) {
        ws[i] = P[ow[i] * 4];
        xs[i] = P[ox[i] * 4 + 1];
        rank_w[ow[i]] = (int32_t)i;
        rank_x[ox[i]] = (int32_t)i;
    }
    for (int64_t i = 0; i < N; ++i) {
        yv[i] = P[oy[i] * 4 + 2];
        zv[i] = P[oy[i] * 4 + 3];
        rw[i] = rank_w[oy[i]];
        rx[i] = rank_x[oy[i]];
    }
    const int64_t tiles = (N + HV4_TILE - 1) / HV4_TILE;
    const int64_t n_part = tiles * tiles;
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto s_ws = L.add<double>(N), s_xs = L.add<double>(N),
               s_yv = L.add<double>(N), s_zv = L.add<double>(N);
    const auto s_out = L.add<double>(n_part);
    const auto s_rw = L.add<int32_t>(N), s_rx = L.add<int32_t>(N);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *d_ws = s_ws.in(base), *d_xs = s_xs.in(base), *d_yv = s_yv.in(base),
           *d_zv = s_zv.in(base), *d_out = s_out.in(base);
    int32_t *d_rw = s_rw.in(base), *d_rx = s_rx.in(base);
    g_ws.begin_uploads();
    g_ws.h2d(d_ws, ws.data(), N * 8, st);
    g_ws.h2d(d_xs, xs.data(), N * 8, st);
    g_ws.h2d(d_yv, yv.data(), N * 8, st);
    g_ws.h2d(d_zv, zv.data(), N * 8, st);
    g_ws.h2d(d_rw, rw.data(), N * 4, st);
    g_ws.h2d(d_rx, rx.data(), N * 4, st);
    hipLaunchKernelGGL(k_hv4d, dim3((unsigned)tiles, (unsigned)tiles),
                       dim3(HV4_THREADS), 0, st, d_ws, d_xs, d_yv, d_zv, d_rw,
                       d_rx, N, ref_w, ref_x, ref_y, ref_z, d_out);
    std::vector<double> part(n_part);
    HIP_CHECK(hipMemcpyAsync(part.data(), d_out, n_part * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double hv = 0.0;
    for (double v : part) hv += v;
    return hv;
}

static size_t hssp4d_lds_bytes(int64_t kcap) { return (size_t)kcap * 24; }

// The sorted selected-set views of the 4-D greedy, k entries each: w- and
// x-sorted coordinates and the y-sorted (y, z, w-rank, x-rank) stream.
struct Views4d {
    WsSlot<double> sw, sx, sy, syz;
    WsSlot<int32_t> syrw, syrx;
    Views4d(WsLayout& L, size_t k)
        : sw(L.add<double>(k)), sx(L.add<double>(k)), sy(L.add<double>(k)),
          syz(L.add<double>(k)), syrw(L.add<int32_t>(k)), syrx(L.add<int32_t>(k)) {}
};

// Per-candidate greedy-HSSP contributions against a selected set passed as its
// six pre-sorted views. Stateless; the session below is the production path.
py::array_t<double> hssp4d_contrib(const arr_f64& cand, const arr_f64& sw,
                                   const arr_f64& sx, const arr_f64& sy,
                                   const arr_f64& syz, const arr_i32& syrw,
                                   const arr_i32& syrx, double ref_w,
                                   double ref_x, double ref_y, double ref_z) {
    if (cand.ndim() != 2 || cand.shape(1) != 4)
        throw std::runtime_error("hssp4d_contrib: cand must be (n, 4)");
    const int64_t n = cand.shape(0);
    const int64_t k = sw.size();
    if ((int64_t)sx.size() != k || (int64_t)sy.size() != k ||
        (int64_t)syz.size() != k || (int64_t)syrw.size() != k ||
        (int64_t)syrx.size() != k)
        throw std::runtime_error("hssp4d_contrib: ragged sorted views");
    if (k > HSSP4_MAX_K)
        throw std::runtime_error("hssp4d_contrib: selected set exceeds the LDS stream bound");
    py::array_t<double> out(n);
    if (n == 0) return out;
    hipStream_t st = g_ws.get_stream();
    WsLayout L;
    const auto s_cand = L.add<double>((size_t)n * 4);
    const Views4d v(L, k);
    const auto s_out = L.add<double>(n);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *d_cand = s_cand.in(base), *d_out = s_out.in(base);
    g_ws.begin_uploads();
    g_ws.h2d(d_cand, cand.data(), (size_t)n * 4 * 8, st);
    g_ws.h2d(v.sw.in(base), sw.data(), k * 8, st);
    g_ws.h2d(v.sx.in(base), sx.data(), k * 8, st);
    g_ws.h2d(v.sy.in(base), sy.data(), k * 8, st);
    g_ws.h2d(v.syz.in(base), syz.data(), k * 8, st);
    g_ws.h2d(v.syrw.in(base), syrw.data(), k * 4, st);
    g_ws.h2d(v.syrx.in(base), syrx.data(), k * 4, st);
    hipLaunchKernelGGL(k_hssp4d_contrib, dim3((unsigned)n), dim3(HSSP4_THREADS),
                       hssp4d_lds_bytes(k), st, d_cand, v.sw.in(base),
                       v.sx.in(base), v.sy.in(base), v.syz.in(base),
                       v.syrw.in(base), v.syrx.in(base), k, k, ref_w, ref_x, ref_y,
                       ref_z, d_out);
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_out, n * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}

// Greedy-HSSP driver, 4 objectives: candidates, the taken-mask, the sorted
// selected-set views and the per-round winner all stay on device.
class Hssp4dSession : HsspSession {
  public:
    Hssp4dSession(const arr_f64& cand, double rw, double rx, double ry, double rz)
        : HsspSession("Hssp4dSession", cand, 4), rw_(rw), rx_(rx), ry_(ry), rz_(rz) {}

    // Launch-train greedy: the contrib -> argmax -> insert round replayed
    // subset_size times; ONE host sync at the end. Unlike the 3-D session
    // (whose taken-mask also serves round()), a run starts from a clear mask,
    // and the insert kernel's staging bounds subset_size.
    py::array_t<int64_t> run(int64_t subset_size) {
        if (subset_size < 0)
            throw std::runtime_error("Hssp4dSession.run: negative subset_size");
        if (subset_size > n_) subset_size = n_;
        if (subset_size > HSSP4_MAX_K)
            throw std::runtime_error(
                "Hssp4dSession.run: subset_size exceeds the insert staging bound");
        if (subset_size == 0) return py::array_t<int64_t>(0);
        hipStream_t st = g_ws.get_stream();
        const size_t kcap = (size_t)subset_size + 1;
        WsLayout L;
        const Views4d v(L, kcap);
        const Train t(L, subset_size);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_sw = v.sw.in(base), *d_sx = v.sx.in(base), *d_sy = v.sy.in(base),
               *d_syz = v.syz.in(base);
        int32_t *d_syrw = v.syrw.in(base), *d_syrx = v.syrx.in(base);
        int64_t* d_k = t.k_round.in(base);
        int64_t* d_round = d_k + 1;
        int64_t* d_chosen = t.chosen.in(base);
        HIP_CHECK(hipMemsetAsync(d_k, 0, 16, st));
        HIP_CHECK(hipMemsetAsync(d_taken_, 0, n_, st));
        replay_captured(st, subset_size, [&] {
            hipLaunchKernelGGL(k_hssp4d_contrib_dk, dim3((unsigned)n_),
                               dim3(HSSP4_THREADS), hssp4d_lds_bytes(kcap), st,
                               d_cand_.ptr, d_sw, d_sx, d_sy, d_syz, d_syrw, d_syrx,
                               d_k, (int64_t)kcap, rw_, rx_, ry_, rz_, d_out_);
            hipLaunchKernelGGL(k_hssp3d_argmax, dim3(1), dim3(256), 0, st, d_out_,
                               n_, d_taken_, d_idx_);
            hipLaunchKernelGGL(k_hssp4d_insert, dim3(1), dim3(HSSP4_THREADS), 0,
                               st, d_cand_.ptr, d_idx_, d_sw, d_sx, d_sy, d_syz,
                               d_syrw, d_syrx, d_k, d_chosen, d_round);
        });
        return download_chosen(d_chosen, subset_size, st);
    }

  private:
    double rw_, rx_, ry_, rz_;
};
