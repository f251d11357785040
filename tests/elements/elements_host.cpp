// elements_host.cpp -- TEST INFRASTRUCTURE: the element-space transform of golemflavor_amd/csrc/gf_elements.hpp and gf_elements_exact.hpp compiled for the
// host, so that its arithmetic can be held to the CPU oracle over millions of rows without a device.  Built by
// tests/elements_harness.py with g++ (contraction off); nothing in the product links it.
#include <stdint.h>

#include "../../golemflavor_amd/csrc/gf_elements_exact.hpp"

extern "C" {

int elh_plan_width(const gf_element_plan* plan, int width_in) { return gfel::plan_width(plan, width_in); }

// rows [n][width_in] -> out [n][plan width]; -1: invalid plan
int elh_rows(const gf_element_plan* plan, const double* rows, int64_t n, int width_in, double* out)
{
    const int w = gfel::plan_width(plan, width_in);
    if (w < 0) return -1;
    for (int64_t i = 0; i < n; ++i) gfel::element_row(*plan, rows + i * width_in, out + i * w);
    return 0;
}

}  // extern "C"
