/*
 * orc_matcher.h -- ORACLE (test infrastructure only): the constants and small helpers of src/ORBmatcher.cc and the Frame grid
 * that the matcher restatements share (orc_match.c, orc_twocam.c).  Internal to oracle/.
 */
#ifndef ORC_MATCHER_H
#define ORC_MATCHER_H

#include "eorb_oracle.h"
#include <math.h>

#define FRAME_GRID_ROWS 48      /* include/Frame.h:45 */
#define FRAME_GRID_COLS 64      /* include/Frame.h:46 */
#define TH_HIGH 100             /* ORBmatcher.cc:36 */
#define TH_LOW 50               /* :37 */
#define HISTO_LENGTH 30         /* :38 */

/* a Frame's keypoints, descriptors and grid (AssignFeaturesToGrid, src/Frame.cc:431-460), made by orc_frame_create */
struct orc_frame {
    int N;
    const orc_keypoint* kps;
    const uint8_t* desc; int desc_stride;
    const uint8_t* is_orb;
    orc_grid_bounds gb;
    int* cell_start;        /* COLS*ROWS+1, cell id = ix*ROWS + iy */
    int* cell_items;        /* insertion order inside each cell */
};

/* the rotation histogram's bin of every matcher (e.g. ORBmatcher.cc:790-796, :1157-1162, :2139-2145) */
static inline int rot_bin(float a1, float a2)
{
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

/* occupancy rule of the projection matchers, getMapPoint(idx) && Observations() > 0 (:91-93, :160-162, :2045-2047, :2128-2130):
 * slot -1 none, k >= 0 query k of this call (observed iff obs[k]), -2 foreign observed, -3 foreign unobserved */
static inline int holds_observed(const int32_t* slot, int idx, const uint8_t* obs)
{
    const int v = slot[idx];
    if (v == -1 || v == -3) return 0;
    if (v == -2) return 1;
    return obs[v] != 0;
}

/* ORBmatcher::RadiusByViewingCos (:221-227) */
static inline float radius_by_viewing_cos(float viewCos) { return viewCos > 0.998 ? 2.5f : 4.0f; }

#endif
