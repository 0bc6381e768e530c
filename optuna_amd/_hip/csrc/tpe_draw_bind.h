// Python side of tpe_draw_host.h: binds scipy's scalar special functions
// (capsules of scipy.special.cython_special, looked up in Python) and numpy's
// log / log1p / exp / logaddexp ufunc objects to tpe_draw::Ops, and runs the
// host half of a fused suggest on numpy arrays. pybind11 only, no HIP, so the
// same code builds into the extension and into the host-only module of
// tests/test_tpe_draw_native.py.
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "tpe_below_host.h"
#include "tpe_draw_host.h"

namespace tpe_draw_py {

namespace py = pybind11;

// The signature string cython_special exports the three scalars under.
constexpr const char* SCALAR_SIG = "double (double, int __pyx_skip_dispatch)";

struct Binding {
    tpe_draw::Ops ops;
    py::object log, log1p, exp, logaddexp;  // numpy's ufunc objects
    py::object owner;  // base of the array views over the native buffers
    bool bound = false;
};

// Never destroyed: the ufunc references must not be dropped after the
// interpreter has gone.
inline Binding& binding() {
    static Binding* b = new Binding();
    return *b;
}

inline py::array view(const double* p, size_t n) {
    return py::array(py::dtype::of<double>(), {(py::ssize_t)n},
                     {(py::ssize_t)sizeof(double)}, p, binding().owner);
}

inline void call_unary(const py::object& uf, const double* in, double* out,
                       size_t n) {
    uf(view(in, n), view(out, n));
}

// Takes the three scalars from their capsules and caches the numpy ufuncs.
// False (and nothing bound) when a capsule is not one or carries another
// signature; the caller then keeps the Python quantile.
inline bool bind(const py::object& ndtr, const py::object& log_ndtr,
                 const py::object& ndtri_exp) {
    Binding& B = binding();
    using scalar_fn = double (*)(double, int);
    scalar_fn fns[3] = {nullptr, nullptr, nullptr};
    const py::object* caps[3] = {&ndtr, &log_ndtr, &ndtri_exp};
    for (int i = 0; i < 3; ++i) {
        PyObject* c = caps[i]->ptr();
        const char* name = PyCapsule_CheckExact(c) ? PyCapsule_GetName(c) : nullptr;
        void* p = nullptr;
        if (name != nullptr && std::strcmp(name, SCALAR_SIG) == 0)
            p = PyCapsule_GetPointer(c, name);
        if (p == nullptr) {
            PyErr_Clear();
            B.bound = false;
            return false;
        }
        fns[i] = reinterpret_cast<scalar_fn>(p);
    }
    // Binding the same functions again changes nothing: a suggest running in
    // another thread (inside one of numpy's loops) keeps a valid table.
    if (B.bound && B.ops.ndtr == fns[0] && B.ops.log_ndtr == fns[1] &&
        B.ops.ndtri_exp == fns[2])
        return true;
    B.bound = false;
    py::module_ np = py::module_::import("numpy");
    B.log = np.attr("log");
    B.log1p = np.attr("log1p");
    B.exp = np.attr("exp");
    B.logaddexp = np.attr("logaddexp");
    B.owner = py::none();
    B.ops.ndtr = fns[0];
    B.ops.log_ndtr = fns[1];
    B.ops.ndtri_exp = fns[2];
    B.ops.ctx = &B;
    B.ops.log = [](void* c, const double* in, double* out, size_t n) {
        call_unary(static_cast<Binding*>(c)->log, in, out, n);
    };
    B.ops.log1p = [](void* c, const double* in, double* out, size_t n) {
        call_unary(static_cast<Binding*>(c)->log1p, in, out, n);
    };
    B.ops.exp = [](void* c, const double* in, double* out, size_t n) {
        call_unary(static_cast<Binding*>(c)->exp, in, out, n);
    };
    B.ops.logaddexp = [](void* c, const double* x, const double* y, double* out,
                         size_t n) {
        static_cast<Binding*>(c)->logaddexp(view(x, n), view(y, n), view(out, n));
    };
    B.bound = true;
    return true;
}

inline bool bound() { return binding().bound; }

inline const tpe_draw::Ops& ops() {
    if (!binding().bound) throw std::runtime_error("tpe_draw: not bound");
    return binding().ops;
}

// The arrays are taken as they are: a wrong dtype or a non-contiguous view is
// an error, not a silent copy.
template <typename T>
const T* typed(const py::array& arr, const char* name, py::ssize_t ndim) {
    if (!py::isinstance<py::array_t<T>>(arr) || !(arr.flags() & py::array::c_style) ||
        arr.ndim() != ndim)
        throw std::runtime_error(std::string("tpe_draw: ") + name +
                                 " has the wrong dtype, rank or layout");
    return static_cast<const T*>(arr.data());
}

// Host half of one suggest; the buffers live until the owner's next call.
// Each owner (a device history, a test call) has its own: numpy may release
// the GIL inside a ufunc loop, so two threads can be inside the host half at
// once, and they must not share buffers.
struct HostDraw {
    size_t n = 0, D = 0, S = 0;  // below rows, dims, candidates
    std::vector<double> obs, mus, sigmas, a, b, loc, scale, p, x_raw, x_kde,
        xedges;
    std::vector<int64_t> active;
    tpe_draw::Workspace ws;
    size_t Kb() const { return n + 1; }
};

// Below rows -> observations -> fit -> choice -> quantile -> candidates.
//   table (N, D) f64, valid (N,) bool, below_rows (m,) i64: the below set is
//     the valid ones of below_rows, in that order
//   bw (n + 1,) f64  normalised mixture weights of the below estimator
//   u (S,), q (S, D) f64  uniforms of the choice and of the quantile
//   alow, ahigh, lows, highs, steps (D,) f64, kinds (D,) i8
// with_edges asks for the step-cell edges as well.
inline void draw(HostDraw& H, const py::array& table, const py::array& valid,
                 const py::array& below_rows, const py::array& bw,
                 const py::array& u, const py::array& q, const py::array& alow,
                 const py::array& ahigh, const py::array& kinds,
                 const py::array& lows, const py::array& highs,
                 const py::array& steps, bool consider_endpoints,
                 bool consider_magic_clip, bool with_edges, size_t max_kernels) {
    const tpe_draw::Ops& op = ops();
    const double* p_table = typed<double>(table, "table", 2);
    const bool* p_valid = typed<bool>(valid, "valid", 1);
    const int64_t* p_rows = typed<int64_t>(below_rows, "below_rows", 1);
    const double* p_bw = typed<double>(bw, "bw", 1);
    const double* p_u = typed<double>(u, "u", 1);
    const double* p_q = typed<double>(q, "q", 2);
    const double* p_alow = typed<double>(alow, "alow", 1);
    const double* p_ahigh = typed<double>(ahigh, "ahigh", 1);
    const int8_t* p_kinds = typed<int8_t>(kinds, "kinds", 1);
    const double* p_lows = typed<double>(lows, "lows", 1);
    const double* p_highs = typed<double>(highs, "highs", 1);
    const double* p_steps = typed<double>(steps, "steps", 1);
    const py::ssize_t N = table.shape(0), D = table.shape(1), S = u.shape(0);
    if (D < 1 || S < 1 || valid.shape(0) != N || q.shape(0) != S ||
        q.shape(1) != D || alow.shape(0) != D || ahigh.shape(0) != D ||
        kinds.shape(0) != D || lows.shape(0) != D || highs.shape(0) != D ||
        steps.shape(0) != D)
        throw std::runtime_error("tpe_draw: shape mismatch");
    for (py::ssize_t c = 0; c < D; ++c)
        if (p_kinds[c] < tpe_draw::KIND_CONT || p_kinds[c] > tpe_draw::KIND_LOG_DISC)
            throw std::runtime_error("tpe_draw: numerical dims only");

    const py::ssize_t m = below_rows.shape(0);
    H.D = (size_t)D;
    H.S = (size_t)S;
    H.obs.resize((size_t)m * D);
    size_t n = 0;
    for (py::ssize_t i = 0; i < m; ++i) {
        const int64_t r = p_rows[i];
        if (r < 0 || r >= N) throw std::runtime_error("tpe_draw: below row out of range");
        if (!p_valid[r]) continue;
        std::memcpy(&H.obs[n * D], p_table + (size_t)r * D, (size_t)D * 8);
        ++n;
    }
    H.n = n;
    if (n + 1 > max_kernels) throw std::runtime_error("tpe_draw: too many below kernels");
    if ((size_t)bw.shape(0) != n + 1)
        throw std::runtime_error("tpe_draw: one weight per below kernel expected");
    tpe_draw::log_observations(op, H.obs.data(), n, (size_t)D, p_kinds, H.ws);

    H.active.resize((size_t)S);
    tpe_draw::choose(p_bw, n + 1, p_u, (size_t)S, H.active.data(), H.ws);
    for (py::ssize_t s = 0; s < S; ++s)
        if (H.active[s] < 0 || (size_t)H.active[s] > n)
            throw std::runtime_error("tpe_draw: weights do not form a distribution");

    const size_t n_k = (n + 1) * (size_t)D, n_x = (size_t)S * D;
    H.mus.resize(n_k);
    H.sigmas.resize(n_k);
    for (auto* v : {&H.a, &H.b, &H.loc, &H.scale, &H.p, &H.x_raw, &H.x_kde})
        v->resize(n_x);
    H.xedges.resize(with_edges ? 2 * n_x : 0);
    tpe_below::fit_and_gather(H.obs.data(), n, (size_t)D, p_alow, p_ahigh,
                              consider_endpoints, consider_magic_clip,
                              H.active.data(), (size_t)S, H.mus.data(),
                              H.sigmas.data(), H.a.data(), H.b.data(),
                              H.loc.data(), H.scale.data());
    tpe_draw::ppf(op, p_q, H.a.data(), H.b.data(), n_x, H.p.data(), H.ws);
    tpe_draw::to_candidates(op, H.p.data(), H.loc.data(), H.scale.data(),
                            (size_t)S, (size_t)D, p_kinds, p_lows, p_highs,
                            p_steps, H.x_raw.data(), H.x_kde.data(),
                            with_edges ? H.xedges.data() : nullptr, H.ws);
}

inline py::array_t<double> copy_out(const std::vector<double>& v, size_t rows,
                                    size_t cols) {
    py::array_t<double> out({(py::ssize_t)rows, (py::ssize_t)cols});
    if (rows * cols != 0) std::memcpy(out.mutable_data(), v.data(), rows * cols * 8);
    return out;
}

// Module-level entries. tpe_draw_bind / tpe_draw_bound serve the sampler; the
// others expose the pieces to the tests.
inline void register_functions(py::module_& m, size_t max_kernels) {
    m.def("tpe_draw_bind", &bind, py::arg("ndtr"), py::arg("log_ndtr"),
          py::arg("ndtri_exp"));
    m.def("tpe_draw_bound", &bound);
    m.def("tpe_draw_ppf", [](const py::array& q, const py::array& a,
                             const py::array& b) {
        const double* pq = typed<double>(q, "q", q.ndim());
        const double* pa = typed<double>(a, "a", q.ndim());
        const double* pb = typed<double>(b, "b", q.ndim());
        if (a.size() != q.size() || b.size() != q.size())
            throw std::runtime_error("tpe_draw_ppf: shape mismatch");
        py::array_t<double> out(std::vector<py::ssize_t>(q.shape(), q.shape() + q.ndim()));
        tpe_draw::Workspace ws;
        tpe_draw::ppf(ops(), pq, pa, pb, (size_t)q.size(), out.mutable_data(), ws);
        return out;
    });
    m.def("tpe_draw_choice", [](const py::array& w, const py::array& u) {
        const double* pw = typed<double>(w, "w", 1);
        const double* pu = typed<double>(u, "u", 1);
        py::array_t<int64_t> out(u.shape(0));
        tpe_draw::Workspace ws;
        tpe_draw::choose(pw, (size_t)w.shape(0), pu, (size_t)u.shape(0),
                         out.mutable_data(), ws);
        return out;
    });
    m.def("tpe_draw_argmax", [](const py::array& v) {
        const double* pv = typed<double>(v, "v", 1);
        if (v.shape(0) < 1) throw std::runtime_error("tpe_draw_argmax: empty");
        return tpe_draw::argmax(pv, (size_t)v.shape(0));
    });
    // (x_raw, mus, sigmas, x_kde, xedges) of the host half of a suggest.
    m.def(
        "tpe_draw_candidates",
        [max_kernels](const py::array& table, const py::array& valid,
                      const py::array& below_rows, const py::array& bw,
                      const py::array& u, const py::array& q,
                      const py::array& alow, const py::array& ahigh,
                      const py::array& kinds, const py::array& lows,
                      const py::array& highs, const py::array& steps,
                      bool consider_endpoints, bool consider_magic_clip) {
            HostDraw H;
            draw(H, table, valid, below_rows, bw, u, q, alow, ahigh, kinds, lows,
                 highs, steps, consider_endpoints, consider_magic_clip, true,
                 max_kernels);
            return py::make_tuple(copy_out(H.x_raw, H.S, H.D),
                                  copy_out(H.mus, H.Kb(), H.D),
                                  copy_out(H.sigmas, H.Kb(), H.D),
                                  copy_out(H.x_kde, H.S, H.D),
                                  copy_out(H.xedges, H.S, 2 * H.D));
        },
        py::arg("table"), py::arg("valid"), py::arg("below_rows"), py::arg("bw"),
        py::arg("u"), py::arg("q"), py::arg("alow"), py::arg("ahigh"),
        py::arg("kinds"), py::arg("lows"), py::arg("highs"), py::arg("steps"),
        py::arg("consider_endpoints"), py::arg("consider_magic_clip"));
}

}  // namespace tpe_draw_py
