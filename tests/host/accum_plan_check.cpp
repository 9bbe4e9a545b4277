// The accumulation dispatcher's rules (eorb_slam_amd/csrc/ev_plan.h) from a plain C++ caller, no device: one query per input line,
//   W H sigma mode_count B nev raw pol gather_form dedupe_min_events position_dict slot_rank rank_ok dict_valid scatter slots_usable
// (slot_rank: the test hook, -1 = not set; rank_ok: the device check of the rank scatter; dict_valid: a dictionary frozen for this
// W, H, sigma; slots_usable: the positions' slot tables could be built), one answer line each:
//   route pipeline_chunk slot_ok slot_chunk slot_scatter_rank bulk_fits host_events
// (tests/accum_routes.py, tests/test_accum_plan_cpp.py)
#include <stdio.h>
#include "eorb_slam_amd/csrc/ev_plan.h"

using namespace eorb;

int main()
{
    int W, H, mode, B, raw, pol, form, pd, slot_rank, rank_ok, dict_valid, scatter, slots_usable;
    long long nev, dd_min;
    float sigma;
    while (scanf("%d %d %f %d %d %lld %d %d %d %lld %d %d %d %d %d %d", &W, &H, &sigma, &mode, &B, &nev, &raw, &pol, &form, &dd_min, &pd, &slot_rank, &rank_ok,
                 &dict_valid, &scatter, &slots_usable) == 16) {
        const AccumShape S = accum_shape(W, H, sigma, mode, B, nev);
        const AccumRequest Q{raw, pol, mode, B};
        AccumKnobs K;
        K.gather_form = form; K.dd_min = dd_min; K.pd = pd; K.scatter = scatter;
        if (slot_rank >= 0) K.slot_rank = slot_rank != 0;
        const DictState D{dict_valid, W, H, 0, sigma};
        SlotScatterChoice sc{0, 0, false, 0};
        const bool slot_ok = plan_slot_shape(S, B, K, rank_ok != 0, &sc);
        printf("%d %d %d %d %d %d %d\n", plan_first_route(S, Q, K, D, W, H, sigma, rank_ok != 0, slots_usable != 0), plan_pipeline_chunk(S, K), slot_ok ? 1 : 0, slot_ok ? sc.chunk : 0,
               slot_ok && sc.rank ? 1 : 0, plan_bulk_fits(S, K) ? 1 : 0, plan_host_events(S, Q, K) ? 1 : 0);
    }
    return 0;
}
