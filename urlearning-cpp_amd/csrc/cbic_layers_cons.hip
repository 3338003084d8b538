// cbic_layers_cons.hip -- the constrained twins of cbic_layers.hip's kernels
// (score_layer_cons_kernel, score_small_cons_kernel: the same texts compiled
// with ULG_CONS 1), launched while the context holds constraints.  A
// translation unit of their own: the twins are half of the scorer's device
// code, and nothing here but the two lookups below is called from outside.

#include "search_internal.h"
#include "cbic_call.h"

using namespace ulg;

namespace {

#define ULG_CONS 1
#include "cbic_score_layer.inc"
#include "cbic_score_small.inc"
#undef ULG_CONS

}  // namespace

namespace ulg {

TwinFn<true, ScoreArgs> layer_cons_kernel(int L, int phase, int variant, bool narrow) {
    return layer_kernel(L, phase, variant, narrow);
}
TwinFn<true, ScoreArgs, const uint64_t *> small_cons_kernel(int Lf) { return small_kernel(Lf); }

}  // namespace ulg
