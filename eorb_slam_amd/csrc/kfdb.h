// Device-resident KeyFrameDatabase: pools, launchers and the query's argument block, shared by kfdb.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include "eorb_ctx.h"

namespace eorb {

constexpr int kKfdbMaxSlots = EORB_KFDB_MAX_SLOTS;
constexpr int kKfdbMaxQueryWords = EORB_KFDB_MAX_QUERY_WORDS;      // the query's word ids are staged in LDS: 4 bytes each
constexpr int kKfdbCovis = EORB_KFDB_COVIS;                          // GetBestCovisibilityKeyFrames(10)

// one query (DetectRelocalizationCandidates / DetectNBestCandidates); every pointer is device memory
struct KfdbQuery {
    int n_slots, nq, family, cap, nbest;
    const uint32_t* q_word; const double* q_val;          // the query's BowVector, word ids ascending
    const uint8_t* exclude;                               // spConnectedKF per slot, or NULL
    const int32_t* covis;                                 // n_slots * 10 slot ids (-1: none), or NULL: no accumulation
    int32_t* hdr;                                         // [0] listed, [1] scored, [2] maxCommonWords, [3] bestAccScore (bits); zero on entry
    int32_t* cnt; uint32_t* first; uint8_t* listed; float* si_slot;      // per slot: shared words, smallest common word, in lKFsSharingWords, si
    int lds_cap;                                          // scored entries the finish kernel may sort in LDS (test hook; at most its own limit)
    uint64_t* key; uint32_t* kslot; int npad;             // the scored slots and their (first word, add sequence) keys; npad entries, a power of two >= n_slots
    // results, cap entries each, in lScoreAndMatch order (written only when scored <= cap)
    int32_t* o_slot; float* o_si; int32_t* o_words; float* o_acc; int32_t* o_best; uint8_t* o_keep;
    float* o_sacc; int32_t* o_sbest;                      // NBest: lAccScoreAndMatch after sort(compFirst)
};

int kfdb_reserve(eorb_ctx* c, int new_slots, int64_t new_words);      // room for that many more slots / pool words (grows and compacts on the device)
// K new vectors: d_slot[k] its slot, d_rec[k] its record (pool offset, length, sequence), d_src[k] the offset of its words in d_word / d_val
int kfdb_add_dev(eorb_ctx* c, int K, const int32_t* d_slot, const KfdbSlot* d_rec, const int32_t* d_src, const uint32_t* d_word, const double* d_val);
int kfdb_erase_dev(eorb_ctx* c, int slot);
int kfdb_query_dev(eorb_ctx* c, const KfdbQuery& q);
void kfdb_free(eorb_ctx* c);

}  // namespace eorb
