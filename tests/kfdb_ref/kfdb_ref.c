/* kfdb_ref.c -- literal CPU restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc) for the tests of the device form:
 * a real inverted file (one linked list of keyframes per word, add :39-45 appends, erase :47-66 unlinks), per-keyframe query / words /
 * score members of both query families, L1Scoring::score with its lower_bound jumps (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68),
 * DetectRelocalizationCandidates (:783-895) and DetectNBestCandidates (:612-780) up to the caller-side tail (map test, isBad, the
 * already-added set, nNumCandidates).  The device form has no inverted file and orders by (smallest common word, add sequence): this
 * file is what it is checked against.  A BowVector is a pair of arrays, word ids ascending (the iteration order of the std::map).
 * Keyframes are named by slots, the lowest free slot first, as eorb_kfdb_add names them.  Test infrastructure only. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct node { int kf; struct node* next; } node;
typedef struct { node *head, *tail; } wlist;

typedef struct {
    int live, n;
    uint32_t* word; double* val;                 /* mBowVec */
    long relocQuery, prQuery;                    /* mnRelocQuery, mnPlaceRecognitionQuery */
    int relocWords, prWords;                     /* mnRelocWords, mnPlaceRecognitionWords */
    float relocScore, prScore;                   /* mRelocScore (defined as 0 at add), mPlaceRecognitionScore */
} keyframe;

typedef struct {
    int nwords;                                  /* mpVoc->size() */
    wlist* inv;                                  /* mvInvertedFile */
    keyframe* kf; int n_slots, cap_slots;
    long next_id;                                /* F->mnId / pKF->mnId of the next query */
} kr_db;

kr_db* kr_create(int vocab_words)
{
    kr_db* d = (kr_db*)calloc(1, sizeof(kr_db));
    d->nwords = vocab_words;
    d->inv = (wlist*)calloc((size_t)vocab_words, sizeof(wlist));
    d->next_id = 1;
    return d;
}

static void free_lists(kr_db* d)
{
    for (int w = 0; w < d->nwords; w++) {
        node* p = d->inv[w].head;
        while (p) { node* nx = p->next; free(p); p = nx; }
        d->inv[w].head = d->inv[w].tail = NULL;
    }
}

/* clear :68-72 */
void kr_clear(kr_db* d)
{
    free_lists(d);
    for (int i = 0; i < d->n_slots; i++) { free(d->kf[i].word); free(d->kf[i].val); }
    d->n_slots = 0;
}

void kr_destroy(kr_db* d)
{
    kr_clear(d);
    free(d->inv); free(d->kf); free(d);
}

/* add :39-45 */
int kr_add(kr_db* d, int n, const uint32_t* word, const double* val)
{
    int slot = 0;
    while (slot < d->n_slots && d->kf[slot].live) slot++;
    if (slot == d->n_slots) {
        if (d->n_slots == d->cap_slots) { d->cap_slots = d->cap_slots ? 2 * d->cap_slots : 16; d->kf = (keyframe*)realloc(d->kf, sizeof(keyframe) * (size_t)d->cap_slots); }
        d->n_slots++;
    }
    keyframe* k = &d->kf[slot];
    memset(k, 0, sizeof(*k));
    k->live = 1; k->n = n;
    k->word = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1)); k->val = (double*)malloc(sizeof(double) * (size_t)(n ? n : 1));
    memcpy(k->word, word, sizeof(uint32_t) * (size_t)n); memcpy(k->val, val, sizeof(double) * (size_t)n);
    for (int i = 0; i < n; i++) {                /* mvInvertedFile[vit->first].push_back(pKF) */
        wlist* l = &d->inv[word[i]];
        node* p = (node*)malloc(sizeof(node));
        p->kf = slot; p->next = NULL;
        if (l->tail) l->tail->next = p; else l->head = p;
        l->tail = p;
    }
    return slot;
}

/* erase :47-66 */
int kr_erase(kr_db* d, int slot)
{
    if (slot < 0 || slot >= d->n_slots || !d->kf[slot].live) return -1;
    keyframe* k = &d->kf[slot];
    for (int i = 0; i < k->n; i++) {
        wlist* l = &d->inv[k->word[i]];
        node* prev = NULL;
        for (node* p = l->head; p; prev = p, p = p->next)
            if (p->kf == slot) {
                if (prev) prev->next = p->next; else l->head = p->next;
                if (l->tail == p) l->tail = prev;
                free(p);
                break;
            }
    }
    free(k->word); free(k->val);
    k->word = NULL; k->val = NULL; k->live = 0; k->n = 0;
    return 0;
}

int kr_n_slots(const kr_db* d) { return d->n_slots; }

void kr_get_scores(const kr_db* d, int family, float* out)
{
    for (int i = 0; i < d->n_slots; i++) out[i] = family ? d->kf[i].prScore : d->kf[i].relocScore;
}

/* std::map::lower_bound: index of the first element with key >= w */
static int lower_bound_(const uint32_t* a, int n, uint32_t w)
{
    int lo = 0, hi = n;
    while (lo < hi) { int mid = (lo + hi) / 2; if (a[mid] < w) lo = mid + 1; else hi = mid; }
    return lo;
}

/* L1Scoring::score, ScoringObject.cpp:23-68 */
double kr_l1_score(int n1, const uint32_t* w1, const double* v1, int n2, const uint32_t* w2, const double* v2)
{
    int i1 = 0, i2 = 0;
    double score = 0;
    while (i1 != n1 && i2 != n2) {
        const double vi = v1[i1], wi = v2[i2];
        if (w1[i1] == w2[i2]) {
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++i1; ++i2;
        } else if (w1[i1] < w2[i2]) i1 = lower_bound_(w1, n1, w2[i2]);
        else i2 = lower_bound_(w2, n2, w1[i1]);
    }
    score = -score / 2.0;
    return score;
}

typedef struct { float first; int second; } sm;      /* pair<float, KeyFrame*> */

/* std::list::sort(compFirst): a stable merge sort, compFirst(a, b) = a.first > b.first (:606-609) */
static void sort_comp_first(sm* a, sm* tmp, int n)
{
    if (n < 2) return;
    const int h = n / 2;
    sort_comp_first(a, tmp, h); sort_comp_first(a + h, tmp, n - h);
    int i = 0, j = h, k = 0;
    while (i < h && j < n) { if (a[j].first > a[i].first) tmp[k++] = a[j++]; else tmp[k++] = a[i++]; }
    while (i < h) tmp[k++] = a[i++];
    while (j < n) tmp[k++] = a[j++];
    memcpy(a, tmp, sizeof(sm) * (size_t)n);
}

/* both queries; nbest: the place-recognition family with spConnectedKF = exclude.  Returns 0, or -3 when lScoreAndMatch is longer than
 * cap (the count is in *n_scored; the stored scores are written all the same).  *stale: neighbour scores added that this query did not
 * write (the neighbour is listed but under the threshold) and an earlier query did (not the 0 of add). */
static int detect(kr_db* d, int nbest, int nq, const uint32_t* qword, const double* qval, const uint8_t* exclude, const int32_t* covis, int cap,
                  int32_t* o_slot, float* o_si, int32_t* o_words, float* o_acc, int32_t* o_best, uint8_t* o_keep, float* o_sacc, int32_t* o_sbest,
                  int* n_listed, int* n_scored, int* max_common, float* best_acc, int* stale)
{
    const long id = d->next_id++;
    int* lKFsSharingWords = (int*)malloc(sizeof(int) * (size_t)(d->n_slots + 1));
    int nl = 0;
    *n_listed = *n_scored = *max_common = 0; *best_acc = 0.f;
    if (stale) *stale = 0;
    for (int v = 0; v < nq; v++)
        for (node* lit = d->inv[qword[v]].head; lit; lit = lit->next) {
            keyframe* pKFi = &d->kf[lit->kf];
            if (!nbest) {                                            /* :797-804 */
                if (pKFi->relocQuery != id) { pKFi->relocWords = 0; pKFi->relocQuery = id; lKFsSharingWords[nl++] = lit->kf; }
                pKFi->relocWords++;
            } else {                                                 /* :630-645 */
                if (pKFi->prQuery != id) {
                    pKFi->prWords = 0;
                    if (!(exclude && exclude[lit->kf])) { pKFi->prQuery = id; lKFsSharingWords[nl++] = lit->kf; }
                }
                pKFi->prWords++;
            }
        }
    *n_listed = nl;
    if (!nl) { free(lKFsSharingWords); return 0; }
    int maxCommonWords = 0;
    for (int i = 0; i < nl; i++) {
        const keyframe* k = &d->kf[lKFsSharingWords[i]];
        const int w = nbest ? k->prWords : k->relocWords;
        if (w > maxCommonWords) maxCommonWords = w;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    *max_common = maxCommonWords;
    sm* lScoreAndMatch = (sm*)malloc(sizeof(sm) * (size_t)nl);
    int ns = 0;
    for (int i = 0; i < nl; i++) {
        keyframe* pKFi = &d->kf[lKFsSharingWords[i]];
        if ((nbest ? pKFi->prWords : pKFi->relocWords) > minCommonWords) {
            float si = kr_l1_score(nq, qword, qval, pKFi->n, pKFi->word, pKFi->val);
            if (nbest) pKFi->prScore = si; else pKFi->relocScore = si;
            lScoreAndMatch[ns].first = si; lScoreAndMatch[ns].second = lKFsSharingWords[i]; ns++;
        }
    }
    free(lKFsSharingWords);
    *n_scored = ns;
    if (ns > cap) { free(lScoreAndMatch); return -3; }
    for (int i = 0; i < ns; i++) {
        const keyframe* k = &d->kf[lScoreAndMatch[i].second];
        o_slot[i] = lScoreAndMatch[i].second; o_si[i] = lScoreAndMatch[i].first; o_words[i] = nbest ? k->prWords : k->relocWords;
    }
    if (!covis) { free(lScoreAndMatch); return 0; }
    sm* lAccScoreAndMatch = (sm*)malloc(sizeof(sm) * (size_t)ns * 2);
    float bestAccScore = 0;
    for (int it = 0; it < ns; it++) {                                /* :846-871 / :693-718 */
        const int pKFi = lScoreAndMatch[it].second;
        float bestScore = lScoreAndMatch[it].first;
        float accScore = bestScore;
        int pBestKF = pKFi;
        for (int v = 0; v < 10; v++) {
            const int s2 = covis[(size_t)pKFi * 10 + v];
            if (s2 < 0 || s2 >= d->n_slots || !d->kf[s2].live) continue;       /* not a neighbour in the database */
            const keyframe* pKF2 = &d->kf[s2];
            if ((nbest ? pKF2->prQuery : pKF2->relocQuery) != id) continue;
            const float sc = nbest ? pKF2->prScore : pKF2->relocScore;
            if (stale && sc != 0.f && !((nbest ? pKF2->prWords : pKF2->relocWords) > minCommonWords)) (*stale)++;
            accScore += sc;
            if (sc > bestScore) { pBestKF = s2; bestScore = sc; }
        }
        lAccScoreAndMatch[it].first = accScore; lAccScoreAndMatch[it].second = pBestKF;
        o_acc[it] = accScore; o_best[it] = pBestKF;
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    *best_acc = bestAccScore;
    if (!nbest) {
        float minScoreToRetain = 0.75f * bestAccScore;               /* :874 */
        for (int it = 0; it < ns; it++) o_keep[it] = lAccScoreAndMatch[it].first > minScoreToRetain ? 1 : 0;
    } else {
        sort_comp_first(lAccScoreAndMatch, lAccScoreAndMatch + ns, ns);      /* :722 */
        for (int it = 0; it < ns; it++) { o_sacc[it] = lAccScoreAndMatch[it].first; o_sbest[it] = lAccScoreAndMatch[it].second; }
    }
    free(lScoreAndMatch); free(lAccScoreAndMatch);
    return 0;
}

int kr_detect_reloc(kr_db* d, int nq, const uint32_t* qword, const double* qval, const int32_t* covis, int cap, int32_t* o_slot, float* o_si,
                    int32_t* o_words, float* o_acc, int32_t* o_best, uint8_t* o_keep, int* n_listed, int* n_scored, int* max_common,
                    float* best_acc, int* stale)
{
    return detect(d, 0, nq, qword, qval, NULL, covis, cap, o_slot, o_si, o_words, o_acc, o_best, o_keep, NULL, NULL, n_listed, n_scored, max_common,
                  best_acc, stale);
}

int kr_detect_nbest(kr_db* d, int nq, const uint32_t* qword, const double* qval, const uint8_t* exclude, const int32_t* covis, int cap,
                    int32_t* o_slot, float* o_si, int32_t* o_words, float* o_acc, int32_t* o_best, float* o_sacc, int32_t* o_sbest, int* n_listed,
                    int* n_scored, int* max_common, float* best_acc, int* stale)
{
    return detect(d, 1, nq, qword, qval, exclude, covis, cap, o_slot, o_si, o_words, o_acc, o_best, NULL, o_sacc, o_sbest, n_listed, n_scored,
                  max_common, best_acc, stale);
}
