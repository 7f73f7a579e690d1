// field32_shim.cpp -- field_test_ops.hpp once more for the host, built with -U__SIZEOF_INT128__ so that g++ takes the
// 32-bit-limb bodies of Mont's add / sub / mul (field.hpp) -- the bodies the device compiler takes -- instead of the
// 64-bit host forms.  Same two entry points as host_shim.cpp; test aid only (tests/test_field_corpora_cpu.py).
#if defined(__SIZEOF_INT128__)
#error "compile with -U__SIZEOF_INT128__: this build is for the 32-bit bodies"
#endif
#include <cstddef>   // (the product's headers leave size_t to whoever includes them)
#include "field_test_ops.hpp"
using namespace ckzg;

extern "C" const char *hs_field_ops() { return fieldtest::desc(); }
extern "C" int hs_field_run(int op, uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                            int n) {
    return fieldtest::run_items(op, out, a, b, c, d, n) ? 0 : 1;
}
