// The accumulation dispatcher's rules (eorb_slam_amd/csrc/ev_plan.h) from a plain C++ caller, no device: one query per input line,
//   W H sigma mode_count B nev raw pol gather_form dedupe_min_events position_dict slot_rank rank_ok dict_valid scatter slots_usable
//   stride sensor_w sensor_h dict slot_prerank ncu sl_null slot_hot_min nparts
// (slot_rank, slot_prerank: the test hooks, -1 = not set; rank_ok: the device check of the rank scatter; dict_valid: a dictionary
// frozen for this W, H, sigma; slots_usable: the positions' slot tables could be built; stride: the record stride handed to the slot
// form; sensor_w x sensor_h: the positions of the set, 0 0 = the image; dict: 0 none, 1 the count pass writes 4-byte rows, 2 2-byte
// ids; ncu, sl_null: compute units, most slots of a tile; slot_hot_min: the test hook, -1 = by size), one answer line each:
//   route pipeline_chunk slot_ok slot_chunk slot_scatter_rank bulk_fits host_events
//   slot_waves bin_ok count record scatter bin_stride scat_stride lds_count lds_scatter slot_binning
//   g_lds g_wg_per_cu g_nw g_rounds g_tasks g_max_per_tile g_prio_ref g_hot_min g_hot_cap g_hot_waves
// (the binning plan of a shape the slot form declines is all zeros)
// (tests/accum_routes.py, tests/test_accum_plan_cpp.py)
#include <stdio.h>
#include "eorb_slam_amd/csrc/ev_plan.h"

using namespace eorb;

int main()
{
    int W, H, mode, B, raw, pol, form, pd, slot_rank, rank_ok, dict_valid, scatter, slots_usable, stride, sw, sh, dict, prerank, ncu, sl_null, nparts;
    long long nev, dd_min, hot_min;
    float sigma;
    while (scanf("%d %d %f %d %d %lld %d %d %d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %d", &W, &H, &sigma, &mode, &B, &nev, &raw, &pol, &form, &dd_min, &pd, &slot_rank,
                 &rank_ok, &dict_valid, &scatter, &slots_usable, &stride, &sw, &sh, &dict, &prerank, &ncu, &sl_null, &hot_min, &nparts) == 25) {
        const AccumShape S = accum_shape(W, H, sigma, mode, B, nev);
        const AccumRequest Q{raw, pol, mode, B};
        AccumKnobs K;
        K.gather_form = form; K.dd_min = dd_min; K.pd = pd; K.scatter = scatter;
        if (slot_rank >= 0) K.slot_rank = slot_rank != 0;
        if (prerank >= 0) K.slot_prerank = prerank;
        if (hot_min >= 0) K.slot_hot_min = hot_min;
        const DictState D{dict_valid, W, H, 0, sigma};
        SlotScatterChoice sc{0, 0, false, 0};
        const bool slot_ok = plan_slot_shape(S, B, K, rank_ok != 0, &sc);
        printf("%d %d %d %d %d %d %d", plan_first_route(S, Q, K, D, W, H, sigma, rank_ok != 0, slots_usable != 0), plan_pipeline_chunk(S, K), slot_ok ? 1 : 0, slot_ok ? sc.chunk : 0,
               slot_ok && sc.rank ? 1 : 0, plan_bulk_fits(S, K) ? 1 : 0, plan_host_events(S, Q, K) ? 1 : 0);
        SlotBinPlan bp{0, 0, 0, 0, 0, 0, 0};
        const long long nsrc = sw > 0 ? (long long)sw * sh : (long long)W * H;
        const bool bin_ok = slot_ok && plan_slot_binning(S, stride, nsrc, dict, sc, K, &bp);
        printf(" %d %d %d %d %d %d %d %zu %zu %d", slot_ok ? sc.waves : 0, bin_ok ? 1 : 0, bp.count, bp.record, bp.scatter, bp.stride, bp.scat_stride, bp.lds_count, bp.lds_scatter,
               bin_ok ? slot_binning_code(bp) : 0);
        const SlotGatherPlan g = plan_slot_gather(S, B, nev, nparts, sl_null, ncu, K);
        printf(" %zu %d %d %d %d %d %u %u %u %d\n", g.lds, g.wg_per_cu, g.nw, g.rounds, g.Gt, g.max_per_tile, g.prio_ref, g.hot_min, g.hot_cap, g.hot_waves);
    }
    return 0;
}
