// What eorb_bow_transform asks before it touches the arena (eorb_slam_amd/csrc/bow_plan.h: plan_bow_transform), from a plain C++ caller:
// one feature count per input line, one answer line each:
//   P regs lds ok max_features lds_optin
// (tests/test_bow_plan_cpp.py)
#include <stdio.h>
#include "eorb_slam_amd/csrc/bow_plan.h"

using namespace eorb;

int main()
{
    int n;
    while (scanf("%d", &n) == 1) {
        const BowPlan B = plan_bow_transform(n);
        printf("%d %d %zu %d %d %zu\n", B.P, B.regs, B.lds, B.ok, kBowMaxFeatures, kBowLdsOptin);
    }
    return 0;
}
