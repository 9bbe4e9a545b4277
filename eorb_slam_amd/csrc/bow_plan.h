// bow_plan.h -- what a call of eorb_bow_transform costs bow_assemble_kernel (match.hip), from its feature count alone.  Host-only: no
// HIP header, no eorb_ctx, so that a plain C++ compiler can build a caller of the rule (tests/host/bow_plan_check.cpp).
//
// The kernel is one workgroup of 1024 threads that sorts P (word, feature) and then P (node, feature) keys in LDS, P = the power of
// two >= max(n, 64).  Thread t keeps keys t, t + 1024, ... in registers: regs = P / 1024 of them (1 up to P = 1024), the register
// class of block_bitonic_sort_regs.  Per key the kernel holds the 64-bit key, the word's 64-bit value and a 16-bit run index (run
// indices are < P <= 8192), 18 bytes; the largest call, 8192 features, takes 147 456 bytes of the 150 KB the kernel opts into, next to
// its three static words.  eorb_bow_transform asks the rule before it touches the arena or any of the caller's arrays.
#pragma once
#include <stddef.h>
#include "../../include/eorb_fe.h"

namespace eorb {

constexpr int kBowMaxFeatures = EORB_BOW_MAX_FEATURES;
constexpr int kBowSortThreads = 1024;
constexpr size_t kBowLdsPerKey = 8 + 8 + 2;                 // key, value, run index
constexpr size_t kBowLdsOptin = 150 * 1024;

struct BowPlan {
    int P;              // keys sorted: the power of two >= max(n, 64); 0 when the call is refused
    int regs;           // keys a thread keeps in registers: 1, 2, 4 or 8
    size_t lds;         // dynamic LDS of bow_assemble_kernel, bytes
    int ok;             // 0: more than kBowMaxFeatures features (EORB_E_CAPACITY)
};

inline BowPlan plan_bow_transform(int n)
{
    BowPlan B{0, 0, 0, 0};
    if (n < 0 || n > kBowMaxFeatures) return B;
    int P = 64;
    while (P < n) P <<= 1;
    B.P = P;
    B.regs = P <= kBowSortThreads ? 1 : P / kBowSortThreads;
    B.lds = (size_t)P * kBowLdsPerKey;
    B.ok = B.lds <= kBowLdsOptin;
    return B;
}

}  // namespace eorb
