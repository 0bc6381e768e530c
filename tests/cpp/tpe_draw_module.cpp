// Host-only pybind11 module over optuna_amd/_hip/csrc/tpe_draw_bind.h, built
// by tests/test_tpe_draw_native.py with the host compiler: the binding code
// of the extension without its device half.
#include "tpe_draw_bind.h"

PYBIND11_MODULE(_tpe_draw_host, m) {
    tpe_draw_py::register_functions(m, 1024);
}
