// k_selftest4.hip -- the self-test kernels (k_selftest.hpp) built with the ILP-4 group formulas
// (fe_mul3 / fe_mul4 / fe_sq4), as k_vrf_v4.hip, k_miss4.hip and k_keys4.hip are.
#define PRAOS_ILP4 1
#include "k_selftest.hpp"
