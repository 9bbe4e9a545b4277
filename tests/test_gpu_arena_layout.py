"""The arena layout and the transfers of every host-buffer call are those on record (GPU).

Every case of tests/dirty_cases.py runs once on one clean context; around it the six cumulative counters of eorb_debug_counter are read:
arenas laid out, their bytes, their uploaded prefix, downloads, downloaded bytes and the sum of the downloads' first offsets.  The
differences are compared with tests/golden/arena_layout.json, which was recorded from the commit before the outputs were declared through
Arena::out (that commit with the counters added and nothing else).  The layout is registration order, so a region that moves, grows or
appears changes arena_bytes or arena_download_first; a destination that is fetched although nobody takes it changes arena_download_bytes.

VARIANTS are the same cases with every optional output absent, for the families whose fetched span depends on what the caller takes: the
case runs unchanged, but the named pointer arguments of the named export reach the library as NULL.

FEWER lists the cases where the one rule -- fetch [first wanted offset, end of the last wanted region) -- fetches less than the recorded
commit did.  There the three layout counters still equal the record and the three download counters equal the numbers listed here."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_cases as dc                            # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("arena_calls", "arena_bytes", "arena_in_bytes", "arena_downloads", "arena_download_bytes", "arena_download_first")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arena_layout.json")

# export -> positions of the optional output pointers in its argument list (negative: from the end)
VARIANTS = {
    "eorb_orb_extract": (8, 9, 10),                                 # kps, desc, oob
    "eorb_frame_mono": (8, 9, 10, 11),                              # kps, kps_un, desc, oob
    "eorb_ev_slice_extract": (8, 9, 10, 14),                        # kps, desc, oob, out_u8
    "eorb_ev_slice_track": (-1,),                                   # out_u8
    "eorb_project_frustum": (-2,),                                  # out
    "eorb_search_local_points": (-3,),                              # out
    "eorb_search_local_points_fisheye": (-3,),
    "eorb_search_by_projection_last_pose": (-3, -2),                # valid, uv
    "eorb_search_by_projection_kf_pose": (-4, -3, -2),              # valid, uv, level
    "eorb_project_keyframe_side": (-1,),                            # out
    "eorb_project_keyframe_side_mixed": (-1,),
    "eorb_fuse_pose": (-1,),
    "eorb_fuse_pose_mixed": (-1,),
    "eorb_search_by_projection_kf_scw": (-1,),
    "eorb_search_by_projection_kf_scw_mixed": (-1,),
    "eorb_fuse_keyframes": (-1,),                                   # reason
    "eorb_fuse_keyframes_mixed": (-1,),
    "eorb_search_by_sim3": (-2, -1),                                # vnMatch1, vnMatch2
    "eorb_two_view_ransac": (-4, -3, -2, -1),                       # it_score_h, it_score_f, it_H, it_F
    "eorb_two_view_check_rt": (-1,),                                # cos_all
    "eorb_two_view_reconstruct": (-1,),                             # hyp_poses
    "eorb_sim3_ransac": (-4, -3, -2, -1),                           # it_inliers, it_T12, it_T21, it_scale
    "eorb_mlpnp_ransac": (-3, -2, -1),                              # it_inliers, it_Rt, it_refine_inliers
}

# Why a case fetches less than the record.  The recorded commit ended most spans at the 256-byte boundary behind the last region
# (A.total, a reserve(0) marker), and fetched a family's whole block once any member of it was taken
PAD = "the span ended at the 256-byte boundary behind its last region; it ends with the last byte somebody takes"
ONLY_COUNT = "only n_in_view is taken: its 4 bytes; the record fetched every array of every view"
NOTHING = "nothing is taken: the call only waits for its kernels; the record fetched the whole block"
LAST_ABSENT = "the case does not take the block's last array (uv_r / level): the span ends with the one before; the record fetched the block"

# key -> (downloads, bytes, first offsets) of the record, the same three now, why.  The new numbers follow from the layout: the end of
# the last array taken (its offset in the arena plus its bytes) minus the first offset, which stays.  The test holds them exactly, and no
# entry may exceed its record in downloads or bytes
FEWER = {
    "eorb_create_new_map_points / K = 3, no node in common in the middle": ((1, 3840, 17920), (1, 3596, 17920), PAD),
    "eorb_create_new_map_points_kb8 / K = 3, no node in common in the middle": ((1, 4864, 22016), (1, 4620, 22016), PAD),
    "eorb_frame_fisheye / flat right image": ((1, 28160, 7168), (1, 28032, 7168), PAD),
    "eorb_frame_fisheye / no keypoint in the lapping areas": ((1, 28160, 7168), (1, 28032, 7168), PAD),
    "eorb_frame_fisheye / shifted pair": ((1, 28160, 7168), (1, 28032, 7168), PAD),
    "eorb_frame_stereo / a pair with disparities up to 6": ((1, 27392, 7168), (1, 27200, 7168), PAD),
    "eorb_frame_stereo / no keypoint on either side": ((1, 27392, 7168), (1, 27200, 7168), PAD),
    "eorb_frame_stereo / no stereo match: a flat right image": ((1, 27392, 7168), (1, 27200, 7168), PAD),
    "eorb_fuse_keyframes / K = 3, an empty keyframe in the middle": ((1, 5888, 29184), (1, 5705, 29184), PAD),
    "eorb_fuse_keyframes / K = 3, an empty keyframe in the middle / no optional output": ((1, 5120, 29184), (1, 4900, 29184), PAD),
    "eorb_fuse_keyframes_mixed / K = 3, an empty keyframe in the middle": ((1, 5888, 29440), (1, 5705, 29440), PAD),
    "eorb_fuse_keyframes_mixed / K = 3, an empty keyframe in the middle / no optional output": ((1, 5120, 29440), (1, 4900, 29440), PAD),
    "eorb_fuse_pose / 195 points, 130 keypoints, stereo gate": ((1, 8448, 24320), (1, 8204, 24320), PAD),
    "eorb_fuse_pose / 195 points, 130 keypoints, stereo gate / no optional output": ((1, 2048, 24320), (1, 1804, 24320), PAD),
    "eorb_fuse_pose_mixed / 195 points, 130 keypoints": ((1, 8448, 25344), (1, 8204, 25344), PAD),
    "eorb_fuse_pose_mixed / 195 points, 130 keypoints / no optional output": ((1, 2048, 25344), (1, 1804, 25344), PAD),
    "eorb_kfdb_detect_nbest / a query": ((1, 2048, 1792), (1, 1804, 1792), PAD),
    "eorb_kfdb_detect_nbest / no shared word: an empty candidate list": ((1, 2048, 1024), (1, 1804, 1024), PAD),
    "eorb_kfdb_detect_reloc / a query": ((1, 1792, 1536), (1, 1539, 1536), PAD),
    "eorb_kfdb_detect_reloc / no shared word: an empty candidate list": ((1, 1792, 768), (1, 1539, 768), PAD),
    "eorb_mlpnp_ransac / K = 3, a short problem between two live ones": ((1, 3328, 18688), (1, 3104, 18688), PAD),
    "eorb_mlpnp_ransac / K = 3, a short problem between two live ones / no optional output": ((1, 768, 18688), (1, 648, 18688), PAD),
    "eorb_mlpnp_ransac / N = 7 and a problem of wrong matches": ((1, 1792, 10496), (1, 1600, 10496), PAD),
    "eorb_mlpnp_ransac / N = 7 and a problem of wrong matches / no optional output": ((1, 512, 10496), (1, 328, 10496), PAD),
    "eorb_new_map_points / K = 3, every match of the middle keyframe fails the parallax test": ((1, 4352, 13056), (1, 4108, 13056), PAD),
    "eorb_new_map_points / stereo keyframes": ((1, 4352, 16384), (1, 4108, 16384), PAD),
    "eorb_new_map_points / two-camera keyframes": ((1, 4352, 13312), (1, 4108, 13312), PAD),
    "eorb_project_frustum / 63 points, two cameras": ((1, 4864, 3584), (1, 4671, 3584), PAD),
    "eorb_project_frustum / 63 points, two cameras / no optional output": ((1, 4864, 3584), (1, 4, 3584), ONLY_COUNT),
    "eorb_project_frustum / 65 points": ((1, 4096, 4096), (1, 3905, 4096), PAD),
    "eorb_project_frustum / 65 points / no optional output": ((1, 4096, 4096), (1, 4, 4096), ONLY_COUNT),
    "eorb_project_keyframe_points / 65 points": ((1, 2560, 3328), (1, 2308, 3328), PAD),
    "eorb_project_keyframe_side / 65 points": ((1, 3328, 3840), (1, 3076, 3840), PAD),
    "eorb_project_keyframe_side / 65 points / no optional output": ((1, 3328, 3840), (0, 0, 0), NOTHING),
    "eorb_project_keyframe_side_mixed / 65 points": ((1, 3328, 4864), (1, 3076, 4864), PAD),
    "eorb_project_keyframe_side_mixed / 65 points / no optional output": ((1, 3328, 4864), (0, 0, 0), NOTHING),
    "eorb_project_last_frame / 65 points": ((1, 2816, 4864), (1, 1796, 4864), LAST_ABSENT),
    "eorb_search_by_projection_kf_pose / 195 points, 130 keypoints": ((1, 4096, 26880), (1, 3852, 26880), PAD),
    "eorb_search_by_projection_kf_scw / 195 points, 130 keypoints": ((1, 8704, 23552), (1, 8460, 23552), PAD),
    "eorb_search_by_projection_kf_scw / 195 points, 130 keypoints / no optional output": ((1, 2304, 23552), (1, 2060, 23552), PAD),
    "eorb_search_by_projection_kf_scw_mixed / 195 points, 130 keypoints": ((1, 8704, 24576), (1, 8460, 24576), PAD),
    "eorb_search_by_projection_kf_scw_mixed / 195 points, 130 keypoints / no optional output": ((1, 2304, 24576), (1, 2060, 24576), PAD),
    "eorb_search_by_projection_last_pose / 195 points, 130 keypoints": ((1, 4096, 25344), (1, 2840, 25344), LAST_ABSENT),
    "eorb_search_by_sim3 / 130 slots a keyframe": ((1, 2560, 33024), (1, 2312, 33024), PAD),
    "eorb_search_by_sim3 / 130 slots a keyframe / no optional output": ((1, 1024, 33024), (1, 776, 33024), PAD),
    "eorb_search_local_points / 195 points, 130 keypoints": ((1, 8448, 23552), (1, 8387, 23552), PAD),
    "eorb_search_local_points / every point skipped": ((1, 4352, 11008), (1, 4161, 11008), PAD),
    "eorb_search_local_points_fisheye / 195 points, 65 + 63 keypoints": ((1, 15616, 23808), (1, 15555, 23808), PAD),
    "eorb_sim3_ransac / K = 3, a short problem between two live ones": ((1, 10496, 18176), (1, 10432, 18176), PAD),
    "eorb_sim3_ransac / K = 3, a short problem between two live ones / no optional output": ((1, 768, 18176), (1, 646, 18176), PAD),
    "eorb_sim3_ransac / N = 3 and a problem of wrong matches / no optional output": ((1, 768, 8704), (1, 580, 8704), PAD),
}


class _Nulling:
    """the library with the optional outputs of one export taken away"""

    def __init__(self, L, export, positions):
        self._L, self._export, self._positions = L, export, positions

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if name != self._export:
            return f

        def call(*args):
            a = list(args)
            for p in self._positions:
                a[p] = None
            return f(*a)
        return call


def read(ctx):
    return [ctx.debug_counter(k) for k in COUNTERS]


def measure(fe, ctx, name, case, variant):
    """the counters' differences around one run of the case (variant: without the optional outputs of VARIANTS[name])"""
    L = ctx.L
    before = read(ctx)
    try:
        if variant:
            ctx.L = _Nulling(L, name, VARIANTS[name])
        case.run(fe, ctx)
    finally:
        ctx.L = L
    return [b - a for a, b in zip(before, read(ctx))]


def key(name, case, variant):
    return "%s / %s%s" % (name, case.name, " / no optional output" if variant else "")


RUNS = [(name, case, False) for name, case in dc.all_cases()] + [(name, case, True) for name, case in dc.all_cases() if name in VARIANTS]
IDS = ["%s-%d%s" % (name[5:], i, "-bare" if v else "") for i, (name, _, v) in enumerate(RUNS)]


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,case,variant", RUNS, ids=IDS)
def test_layout_and_transfers_are_the_recorded_ones(fe, ctx, golden, name, case, variant):
    k = key(name, case, variant)
    got, want = measure(fe, ctx, name, case, variant), golden[k]
    print(k, dict(zip(COUNTERS, got)))
    if k in FEWER:
        rec, now, _why = FEWER[k]
        assert list(rec) == want[3:], "%s: the record holds %s, the table of this test %s" % (k, want[3:], list(rec))
        assert now[0] <= rec[0] and now[1] <= rec[1], "%s: the table allows more than the record" % k
        want = want[:3] + list(now)
    assert got == want, "%s: %s, on record %s" % (k, dict(zip(COUNTERS, got)), dict(zip(COUNTERS, want)))


def test_the_record_holds_every_run_and_no_other(golden):
    assert sorted(golden) == sorted(key(*r) for r in RUNS)
    assert set(FEWER) <= set(golden)
