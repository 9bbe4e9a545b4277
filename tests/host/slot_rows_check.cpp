// The rows the slot form's count pass and scan leave for its scatters, and the scatters' LDS, as eorb_slam_amd/csrc/ev_plan.h promises
// them, from a plain C++ caller: one query per input line,
//   NT nchunks chunk waves
// one answer line each:
//   loff_pitch gbase_pitch loff_bytes rows_bytes lds_pre lds_rank lds_ballot scan_waves scan_segments scan_tiles chunk_max
// (tests/test_slot_rows_cpp.py)
#include <stdio.h>
#include "eorb_slam_amd/csrc/ev_plan.h"

using namespace eorb;

int main()
{
    int NT, nchunks, chunk, waves;
    while (scanf("%d %d %d %d", &NT, &nchunks, &chunk, &waves) == 4) {
        const SlotRows r = plan_slot_rows(nchunks, NT);
        printf("%d %d %zu %zu %zu %zu %zu %d %d %d %d\n", r.lp, r.gp, r.loff_bytes, r.bytes, plan_slot_lds_pre(NT, chunk), plan_slot_lds_rank(NT, chunk, waves),
               plan_slot_lds_ballot(NT, chunk), plan_slot_scan_waves(NT), plan_slot_scan_segments(NT), kSlotScanTiles, kSlotChunkMax);
    }
    return 0;
}
