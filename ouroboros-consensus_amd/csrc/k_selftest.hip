// k_selftest.hip -- the self-test kernels (k_selftest.hpp) built with the default two-way
// interleaved group formulas (fe_mul2 / fe_sq2), plus the field-product and field-predicate
// self tests, which do not depend on the build.
#include "k_selftest.hpp"
