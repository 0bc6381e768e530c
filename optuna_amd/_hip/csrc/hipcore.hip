// The _hipcore extension: one translation unit, one header per domain.
// This file holds the includes and the Python bindings only.
#include "hip_common.h"

// The GP headers in dependency order: the sessions call the constraint set.
#include "gp_posterior.h"
#include "gp_feasibility.h"
#include "gp_logei.h"
#include "gp_ehvi.h"

#include "mo_host.h"
#include "mo_rank.h"
#include "tpe_host.h"
#include "truncnorm_ops.h"

PYBIND11_MODULE(_hipcore, m) {
    m.doc() = "optuna_amd MI355X (gfx950) HIP kernels: TPE parzen fit + mixture "
              "log-pdf, truncnorm device library";
    m.def("available", &available);
    m.def("device_count", &device_count);
    m.def("log_gauss_mass", &log_gauss_mass);
    m.def("truncnorm_ppf", &truncnorm_ppf);
    m.def("truncnorm_logpdf", &truncnorm_logpdf);
    m.def("nondomination_rank", &nondomination_rank, py::arg("vals"),
          py::arg("n_below"));
    m.def("hv3d", &hv3d, py::arg("pts"), py::arg("ref_x"), py::arg("ref_y"),
          py::arg("ref_z"));
    py::class_<GpConstraintSet>(m, "GpConstraintSet")
        .def(py::init<const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<double>&, const std::vector<double>&,
                      int64_t, int64_t, double, int64_t, uint64_t>(),
             py::arg("X_ptrs"), py::arg("alpha_ptrs"), py::arg("cinv_ptrs"),
             py::arg("eta_ptrs"), py::arg("scales"), py::arg("thresholds"),
             py::arg("N"), py::arg("D"), py::arg("stab_noise"),
             py::arg("scratch_budget_bytes") = GP_SCRATCH_BUDGET_BYTES,
             py::arg("cat_mask") = (uint64_t)0)
        .def("n_chunks", &GpConstraintSet::n_chunks, py::arg("B"),
             py::arg("with_grad"))
        .def("n_splits", &GpConstraintSet::n_splits, py::arg("bc"))
        .def("eval", &GpConstraintSet::eval, py::arg("x"), py::arg("with_grad"));
    m.attr("GP_FEAS_MAX_C") = py::int_(FEAS_MAX_C);
    py::class_<GpLogEiSession>(m, "GpLogEiSession")
        .def(py::init<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                      double, double, double, uint64_t>(),
             py::arg("X_ptr"), py::arg("alpha_ptr"), py::arg("cinv_ptr"),
             py::arg("eta_ptr"), py::arg("N"), py::arg("D"), py::arg("scale"),
             py::arg("stab_noise"), py::arg("threshold"),
             py::arg("cat_mask") = (uint64_t)0)
        .def("eval", &GpLogEiSession::eval, py::arg("x"), py::arg("with_grad"),
             py::arg("constraints") = py::none());
    py::class_<GpLogEhviSession>(m, "GpLogEhviSession")
        .def(py::init<const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<double>&, int64_t, int64_t, double,
                      const arr_f64&, const arr_f64&, const arr_f64&, int64_t,
                      uint64_t>(),
             py::arg("X_ptrs"), py::arg("alpha_ptrs"), py::arg("cinv_ptrs"),
             py::arg("eta_ptrs"), py::arg("scales"), py::arg("N"), py::arg("D"),
             py::arg("stab_noise"), py::arg("eps"), py::arg("lo"), py::arg("iv"),
             py::arg("scratch_budget_bytes") = GP_SCRATCH_BUDGET_BYTES,
             py::arg("cat_mask") = (uint64_t)0)
        .def("n_chunks", &GpLogEhviSession::n_chunks, py::arg("B"),
             py::arg("with_grad"))
        .def("eval", &GpLogEhviSession::eval, py::arg("x"), py::arg("with_grad"),
             py::arg("constraints") = py::none());
    m.attr("GP_EHVI_BOX_TILE") = py::int_(EHVI_BOX_TILE);
    m.attr("GP_EHVI_MAX_Q") = py::int_(EHVI_MAX_Q);
    m.attr("GP_EHVI_SCRATCH_BUDGET_BYTES") = py::int_(GP_SCRATCH_BUDGET_BYTES);
    py::class_<Hssp3dSession>(m, "Hssp3dSession")
        .def(py::init<const arr_f64&, double, double, double>(), py::arg("cand"),
             py::arg("ref_x"), py::arg("ref_y"), py::arg("ref_z"))
        .def("round", &Hssp3dSession::round, py::arg("sx"), py::arg("sxz"),
             py::arg("sy"), py::arg("syz"), py::arg("syr"))
        .def("run", &Hssp3dSession::run, py::arg("subset_size"));
    m.def("hssp3d_contrib", &hssp3d_contrib, py::arg("cand"), py::arg("sx"),
          py::arg("sxz"), py::arg("sy"), py::arg("syz"), py::arg("syr"),
          py::arg("ref_x"), py::arg("ref_y"), py::arg("ref_z"));
    m.def("hv4d", &hv4d, py::arg("pts"), py::arg("ref_w"), py::arg("ref_x"),
          py::arg("ref_y"), py::arg("ref_z"));
    m.def("hssp4d_contrib", &hssp4d_contrib, py::arg("cand"), py::arg("sw"),
          py::arg("sx"), py::arg("sy"), py::arg("syz"), py::arg("syrw"),
          py::arg("syrx"), py::arg("ref_w"), py::arg("ref_x"), py::arg("ref_y"),
          py::arg("ref_z"));
    py::class_<Hssp4dSession>(m, "Hssp4dSession")
        .def(py::init<const arr_f64&, double, double, double, double>(),
             py::arg("cand"), py::arg("ref_w"), py::arg("ref_x"),
             py::arg("ref_y"), py::arg("ref_z"))
        .def("run", &Hssp4dSession::run, py::arg("subset_size"));
    m.attr("HSSP4D_MAX_SUBSET") = py::int_(HSSP4_MAX_K);
    m.def("kde_logpdf", &kde_logpdf, py::arg("obs"), py::arg("sorted_pos"),
          py::arg("logw"), py::arg("alow"), py::arg("ahigh"), py::arg("steps"),
          py::arg("n_choices"), py::arg("prior_weight"),
          py::arg("x"), py::arg("xedges"),
          py::arg("consider_endpoints") = false, py::arg("magic_clip") = true);
    m.def("tpe_below_kernels", &tpe_below_kernels, py::arg("obs"),
          py::arg("alow"), py::arg("ahigh"), py::arg("consider_endpoints"),
          py::arg("consider_magic_clip"), py::arg("active"));
    tpe_draw_py::register_functions(m, (size_t)FUSED_MAX_BELOW);
    py::class_<TpeDeviceHistory>(m, "TpeDeviceHistory")
        .def(py::init<int64_t>(), py::arg("dims"))
        .def_property_readonly("n_rows", &TpeDeviceHistory::n_rows)
        .def("append", &TpeDeviceHistory::append, py::arg("block"))
        .def("upload_sorted", &TpeDeviceHistory::upload_sorted, py::arg("cols"))
        .def_property_readonly("n_sorted", &TpeDeviceHistory::n_sorted)
        .def("insert_sorted_by_value", &TpeDeviceHistory::insert_sorted_by_value,
             py::arg("first_row"), py::arg("n_new"))
        .def("sorted_index", &TpeDeviceHistory::sorted_index)
        .def("set_domain", &TpeDeviceHistory::set_domain, py::arg("alow"),
             py::arg("ahigh"), py::arg("steps"), py::arg("n_choices"))
        .def("fused_prepare", &TpeDeviceHistory::fused_prepare, py::arg("excl"),
             py::arg("n_above"), py::arg("logw") = arr_f64(),
             py::arg("w_num") = 0, py::arg("w_start") = 1.0,
             py::arg("w_step") = 0.0, py::arg("log_total") = 0.0,
             py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true)
        .def("fused_score", &TpeDeviceHistory::fused_score, py::arg("excl"),
             py::arg("n_above"), py::arg("x"), py::arg("xedges"),
             py::arg("bmu"), py::arg("bsig"), py::arg("bw"),
             py::arg("logw") = arr_f64(), py::arg("w_num") = 0,
             py::arg("w_start") = 1.0, py::arg("w_step") = 0.0,
             py::arg("log_total") = 0.0, py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true, py::arg("return_parts") = false)
        .def("fused_draw_score", &TpeDeviceHistory::fused_draw_score,
             py::arg("excl"), py::arg("n_above"), py::arg("table"),
             py::arg("valid"), py::arg("below_rows"), py::arg("bw"),
             py::arg("u"), py::arg("q"), py::arg("alow"), py::arg("ahigh"),
             py::arg("kinds"), py::arg("lows"), py::arg("highs"),
             py::arg("steps"), py::arg("logw") = arr_f64(),
             py::arg("w_num") = 0, py::arg("w_start") = 1.0,
             py::arg("w_step") = 0.0, py::arg("log_total") = 0.0,
             py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true)
        .def("score", &TpeDeviceHistory::score, py::arg("sorted_rows"),
             py::arg("pos"), py::arg("n_above"), py::arg("logw"), py::arg("alow"),
             py::arg("ahigh"), py::arg("steps"), py::arg("n_choices"),
             py::arg("prior_weight"), py::arg("x"), py::arg("xedges"),
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true,
             py::arg("extras_raw") = arr_f64(),
             py::arg("extras_sorted") = arr_f64(),
             py::arg("extras_sorted_idx") = arr_i32(),
             py::arg("per_dim") = false);
}
