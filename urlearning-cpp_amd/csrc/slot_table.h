// slot_table.h -- the steps of a layer scorer that do not depend on the score:
// the slot table of a call (one float and one set mask per parent set, slab
// (i, L) = variable i's sets of L parents in colex order), the prune pass over
// it (disc_prune_kernel) and the compaction of the stored slots into the
// context's lists.  ulg_disc_score (disc.hip) and ulg_bge_score (bge.hip) both
// run them; the kernels and the functions live in disc.hip.
#pragma once

#include <chrono>
#include <vector>

#include "ulg_internal.h"

namespace ulg {

constexpr int kSlotWords = 5;  // the call's words: [error word, dense sets, sparse sets, stored, pruned]

// The host side of a call's table: what the layer, prune and compaction
// kernels read as `toff`, `work` and `vm`.
struct SlotTable {
    std::vector<uint64_t> meta;  // [toff: nv * S + 1][work: S x (nv + 1)]
    std::vector<int> vm;         // [nv][2]: variable, candidate count
    int nv = 0, S = 0;
    uint64_t total_slots = 0;
    int64_t nb = 0;              // compaction blocks

    void build(const ScoreLists &ls);
    // layer L's item prefixes within meta, and their total
    size_t work_at(int L) const { return (size_t)nv * S + 1 + (size_t)L * (nv + 1); }
    uint64_t items(int L) const { return meta[work_at(L) + nv]; }
};

// The table's buffers (d_disc_meta / cand / vm / table / sets / blk / word),
// the uploads, every slot absent and the words zero; synchronises, since the
// sources are pageable.
int slot_table_begin(ulg_ctx *c, const ScoreLists &ls, const SlotTable &st);
// -r (score_calculator.cpp:33-52,78), called after a complete layer that is not
// the last: synchronises the stream and says whether the budget is spent.
int slot_table_time_up(ulg_ctx *c, std::chrono::steady_clock::time_point t_call, bool *up);
// disc_prune_kernel over layers 0 .. done_L; the removed sets are counted in word 4.
int slot_table_prune(ulg_ctx *c, const SlotTable &st, int done_L);
// count / scan / write / offsets into out_sets, out_scores and out_offsets; the
// call's words come back in `word` after the stream has been synchronised.
int slot_table_compact(ulg_ctx *c, const SlotTable &st, unsigned long long (&word)[kSlotWords]);

}  // namespace ulg
