// Host-only pybind11 module over optuna_amd/_hip/csrc/tpe_ledger_bind.h, built
// by tests/test_tpe_ledger_native.py with the host compiler: the split ledger
// of the extension without its device half.
#include "tpe_ledger_bind.h"

PYBIND11_MODULE(_tpe_ledger_host, m) {
    tpe_ledger_py::register_functions(m);
}
