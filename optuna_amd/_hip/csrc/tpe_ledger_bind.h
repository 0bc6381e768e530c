// Python binding of tpe_ledger_host.h: the TpeSplitLedger class that
// _history.py owns, and the two host helpers of fused_advance as functions of
// their own (the tests compare them with the Python they replace). No HIP
// here, so that a host-only module can register it (see
// tests/cpp/tpe_ledger_module.cpp).
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <stdexcept>

#include "tpe_ledger_host.h"

namespace tpe_ledger_py {

namespace py = pybind11;

using i64_in = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using i32_in = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using f64_in = py::array_t<double, py::array::c_style | py::array::forcecast>;

inline py::array_t<int64_t> below(const tpe_ledger::TpeSplitLedger& L, int64_t k) {
    if (k < 0) throw std::invalid_argument("TpeSplitLedger.below: k < 0");
    py::array_t<int64_t> out((py::ssize_t)std::min<size_t>((size_t)k, L.size()));
    L.below((size_t)k, out.mutable_data());
    return out;
}

inline void register_functions(py::module_& m) {
    using tpe_ledger::TpeSplitLedger;
    // module_local: the extension and a host-only test module can both be
    // loaded into one process.
    py::class_<TpeSplitLedger>(m, "TpeSplitLedger", py::module_local())
        .def(py::init<>())
        .def("__len__", &TpeSplitLedger::size)
        .def_property_readonly("capacity", &TpeSplitLedger::capacity)
        .def("insert", &TpeSplitLedger::insert, py::arg("row"), py::arg("key"))
        .def("insert_many",
             [](TpeSplitLedger& L, const i64_in& rows, const f64_in& keys) {
                 if (rows.ndim() != 1 || keys.ndim() != 1 ||
                     rows.shape(0) != keys.shape(0))
                     throw std::invalid_argument(
                         "TpeSplitLedger.insert_many: shape mismatch");
                 L.insert_many(rows.data(), keys.data(), (size_t)rows.shape(0));
             },
             py::arg("rows"), py::arg("keys"))
        .def("below", &below, py::arg("k"))
        .def("export", [](const TpeSplitLedger& L) {
            py::array_t<double> keys((py::ssize_t)L.size());
            py::array_t<int64_t> rows((py::ssize_t)L.size());
            std::copy(L.keys(), L.keys() + L.size(), keys.mutable_data());
            std::copy(L.rows(), L.rows() + L.size(), rows.mutable_data());
            return py::make_tuple(keys, rows);
        });
    m.def("tpe_exclusion_list",
          [](const i64_in& below_rows, const i32_in& invalid) {
              if (below_rows.ndim() != 1 || invalid.ndim() != 1)
                  throw std::invalid_argument("tpe_exclusion_list: 1-D arrays");
              std::vector<int32_t> out((size_t)(below_rows.size() + invalid.size()));
              const size_t E = tpe_ledger::exclusion_list(
                  below_rows.data(), (size_t)below_rows.size(), invalid.data(),
                  (size_t)invalid.size(), out.data());
              py::array_t<int32_t> excl((py::ssize_t)E);
              std::copy(out.begin(), out.begin() + E, excl.mutable_data());
              return excl;
          },
          py::arg("below_rows"), py::arg("invalid_rows"));
    m.def("tpe_default_weight_ramp",
          [](int64_t n, double prior_weight) {
              const auto r = tpe_ledger::default_weight_ramp(n, prior_weight);
              return py::make_tuple(r.num, r.start, r.step, r.log_total);
          },
          py::arg("n"), py::arg("prior_weight"));
}

}  // namespace tpe_ledger_py
