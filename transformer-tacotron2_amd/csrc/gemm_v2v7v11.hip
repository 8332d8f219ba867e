// gemm_v2v7v11.hip -- one translation unit for three kernel families, each in its own file:
// v2 (gemm_v2_impl.h), v7 with the split-K reducers (gemm_v7_impl.h) and v11 (gemm_v11_impl.h).
//
// They are compiled together because of how the shared device helpers are optimised.  The helpers
// (gemm_common.h, gemm_v7.h) have unit-local linkage, and the optimiser narrows such a helper to
// the call sites it sees in its unit (interprocedural constant / range propagation) before it is
// inlined.  A family compiled without the others' call sites therefore gets slightly different
// code for the same source: compiled apart, v2 lost v7's / v11's call of frag2<false>, v11 lost
// v7's calls of the loader helpers, and the grouped reducer lost the plain reducer's call of
// splitk_reduce_body -- 15 kernels changed register allocation, instruction order or compare
// signedness (nothing measured slower or faster; the point is that the split itself changed no
// device code).  v1, skinny, ffn_decode, v8 and v10 compile to the same code on their own.
// The same holds inside v7: the grouped kernels change without the plain ones beside them.
// tools/isa_same.py is the check; a change that edits these kernels anyway is free to split
// the unit and re-measure.
#include "gemm_v2_impl.h"
#include "gemm_v7_impl.h"
#include "gemm_v11_impl.h"
