// The _hipcore extension: one translation unit, one header per domain.
// This file holds the includes and the Python bindings only.
#include "hip_common.h"

// The GP headers in dependency order: the sessions call the constraint set.
#include "gp_posterior.h"
#include "gp_feasibility.h"
#include "gp_logei.h"
#include "gp_ehvi.h"
#include "gp_qlogei.h"
#include "gp_qlogehvi.h"
#include "gp_qlogcei.h"
#include "gp_fit.h"

#include "mo_boxes.h"
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
    py::class_<GpQLogEiSession>(m, "GpQLogEiSession")
        .def(py::init<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                      double, double, double, int64_t, int64_t, int64_t, int64_t,
                      int64_t, const arr_f64&, const arr_f64&, int64_t, uint64_t>(),
             py::arg("X_ptr"), py::arg("alpha_ptr"), py::arg("cinv_ptr"),
             py::arg("eta_ptr"), py::arg("N"), py::arg("D"), py::arg("scale"),
             py::arg("stab_noise"), py::arg("threshold"), py::arg("Xr_ptr"),
             py::arg("Vr_ptr"), py::arg("L_ptr"), py::arg("W_ptr"), py::arg("R"),
             py::arg("z"), py::arg("m"),
             py::arg("scratch_budget_bytes") = GP_SCRATCH_BUDGET_BYTES,
             py::arg("cat_mask") = (uint64_t)0)
        .def("n_chunks", &GpQLogEiSession::n_chunks, py::arg("B"))
        .def("n_splits", &GpQLogEiSession::n_splits, py::arg("bc"))
        .def("eval", &GpQLogEiSession::eval, py::arg("x"), py::arg("with_grad"));
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
    py::class_<GpQLogEhviSession>(m, "GpQLogEhviSession")
        .def(py::init<const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<double>&, int64_t, int64_t, double, int64_t,
                      const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<int64_t>&, int64_t, const arr_f64&,
                      const arr_f64&, const arr_f64&, const arr_i64&, int64_t,
                      int64_t, uint64_t>(),
             py::arg("X_ptrs"), py::arg("alpha_ptrs"), py::arg("cinv_ptrs"),
             py::arg("eta_ptrs"), py::arg("scales"), py::arg("N"), py::arg("D"),
             py::arg("stab_noise"), py::arg("Xr_ptr"), py::arg("Vr_ptrs"),
             py::arg("L_ptrs"), py::arg("W_ptrs"), py::arg("R"), py::arg("z"),
             py::arg("lo"), py::arg("iv"), py::arg("offsets"), py::arg("Jmax"),
             py::arg("scratch_budget_bytes") = GP_SCRATCH_BUDGET_BYTES,
             py::arg("cat_mask") = (uint64_t)0)
        .def("n_chunks", &GpQLogEhviSession::n_chunks, py::arg("B"),
             py::arg("with_grad"))
        .def("n_splits", &GpQLogEhviSession::n_splits, py::arg("bc"))
        .def("draw_splits", &GpQLogEhviSession::draw_splits, py::arg("bc"))
        .def("eval", &GpQLogEhviSession::eval, py::arg("x"), py::arg("with_grad"));
    m.attr("GP_QEHVI_MAX_Q") = py::int_(QEHVI_MAX_Q);
    m.attr("GP_QEHVI_TILE") = py::int_(QEHVI_TILE);
    py::class_<GpQLogCeiSession>(m, "GpQLogCeiSession")
        .def(py::init<const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<double>&, int64_t, int64_t, double, int64_t,
                      const std::vector<int64_t>&, const std::vector<int64_t>&,
                      const std::vector<int64_t>&, int64_t,
                      const std::vector<double>&, bool, const arr_f64&,
                      const arr_f64&, double, int64_t, uint64_t>(),
             py::arg("X_ptrs"), py::arg("alpha_ptrs"), py::arg("cinv_ptrs"),
             py::arg("eta_ptrs"), py::arg("scales"), py::arg("N"), py::arg("D"),
             py::arg("stab_noise"), py::arg("Xr_ptr"), py::arg("Vr_ptrs"),
             py::arg("L_ptrs"), py::arg("W_ptrs"), py::arg("R"),
             py::arg("thresholds"), py::arg("has_objective"), py::arg("z"),
             py::arg("F"), py::arg("tau"),
             py::arg("scratch_budget_bytes") = GP_SCRATCH_BUDGET_BYTES,
             py::arg("cat_mask") = (uint64_t)0)
        .def("n_chunks", &GpQLogCeiSession::n_chunks, py::arg("B"),
             py::arg("with_grad"))
        .def("n_splits", &GpQLogCeiSession::n_splits, py::arg("bc"))
        .def("eval", &GpQLogCeiSession::eval, py::arg("x"), py::arg("with_grad"));
    py::class_<GpFitSession>(m, "GpFitSession")
        .def(py::init<int64_t, int64_t, int64_t, int64_t, uint64_t>(), py::arg("X_ptr"),
             py::arg("y_ptr"), py::arg("N"), py::arg("D"), py::kw_only(),
             py::arg("cat_mask") = (uint64_t)0)
        .def("build_cov", &GpFitSession::build_cov, py::arg("raw_params"),
             py::arg("minimum_noise"), py::arg("deterministic"), py::arg("C_ptr"))
        .def("grad", &GpFitSession::grad, py::arg("raw_params"),
             py::arg("minimum_noise"), py::arg("deterministic"), py::arg("L_ptr"),
             py::arg("alpha_ptr"), py::arg("Cinv_ptr"));
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
    m.def("box_decompose", &box_decompose, py::arg("base"), py::arg("extra"),
          py::arg("ref"), py::kw_only(), py::arg("active_cap") = 0,
          py::arg("out_cap") = 0);
    m.def("box_decompose_limits", &box_decompose_limits, py::arg("n_objectives"));
    m.def("kde_logpdf", &kde_logpdf, py::arg("obs"), py::arg("sorted_pos"),
          py::arg("logw"), py::arg("alow"), py::arg("ahigh"), py::arg("steps"),
          py::arg("n_choices"), py::arg("prior_weight"),
          py::arg("x"), py::arg("xedges"),
          py::arg("consider_endpoints") = false, py::arg("magic_clip") = true);
    m.def("tpe_below_kernels", &tpe_below_kernels, py::arg("obs"),
          py::arg("alow"), py::arg("ahigh"), py::arg("consider_endpoints"),
          py::arg("consider_magic_clip"), py::arg("active"));
    tpe_draw_py::register_functions(m, (size_t)FUSED_MAX_BELOW);
    tpe_ledger_py::register_functions(m);
    py::class_<TpeDeviceHistory>(m, "TpeDeviceHistory")
        .def(py::init<int64_t>(), py::arg("dims"))
        .def_property_readonly("n_rows", &TpeDeviceHistory::n_rows)
        .def("append", &TpeDeviceHistory::append, py::arg("block"))
        .def("upload_sorted", &TpeDeviceHistory::upload_sorted, py::arg("cols"))
        .def_property_readonly("n_sorted", &TpeDeviceHistory::n_sorted)
        .def("insert_sorted_by_value", &TpeDeviceHistory::insert_sorted_by_value,
             py::arg("first_row"), py::arg("n_new"))
        .def("sorted_index", &TpeDeviceHistory::sorted_index)
        .def("table_rows", &TpeDeviceHistory::table_rows, py::arg("first_row"),
             py::arg("n_rows"))
        .def("set_domain", &TpeDeviceHistory::set_domain, py::arg("alow"),
             py::arg("ahigh"), py::arg("steps"), py::arg("n_choices"))
        .def("fused_prepare", &TpeDeviceHistory::fused_prepare, py::arg("excl"),
             py::arg("n_above"), py::arg("logw") = arr_f64(),
             py::arg("w_num") = 0, py::arg("w_start") = 1.0,
             py::arg("w_step") = 0.0, py::arg("log_total") = 0.0,
             py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true)
        .def("fused_advance", &TpeDeviceHistory::fused_advance, py::arg("ledger"),
             py::arg("n_below"), py::arg("valid"), py::arg("invalid_rows"),
             py::arg("block"), py::arg("first_row"), py::arg("n_valid"),
             py::arg("prior_weight") = 1.0,
             py::arg("consider_endpoints") = false,
             py::arg("magic_clip") = true)
        .def("fused_step", &TpeDeviceHistory::fused_step, py::arg("ledger"),
             py::arg("n_below"), py::arg("valid"), py::arg("invalid_rows"),
             py::arg("block"), py::arg("first_row"), py::arg("n_valid"),
             py::arg("table"), py::arg("bw"), py::arg("u"), py::arg("q"),
             py::arg("alow"), py::arg("ahigh"), py::arg("kinds"),
             py::arg("lows"), py::arg("highs"), py::arg("steps"),
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
