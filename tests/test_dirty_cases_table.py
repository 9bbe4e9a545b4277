"""The table of tests/dirty_cases.py against the ABI (no GPU): every export has an entry, and every export that lays a call out in the
context's arena has a case.  Which exports those are is written down here, from reading csrc/eorb_fe.hip -- the entry points that
construct an Arena themselves, and those that reach one of the shared bodies that do -- and not parsed from the source: a new export
makes the first test fail until someone decides where it belongs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_cases as dc                            # noqa: E402
from eorb_slam_amd import _lib                      # noqa: E402

# the entry points that construct an Arena in their own body
ARENA = """eorb_bow_transform eorb_calc_optical_flow_pyr_lk eorb_distinctive_descriptors eorb_ev_mc_contest eorb_ev_slice_extract eorb_ev_slice_track
eorb_frame_fisheye eorb_frame_mono eorb_frame_stereo eorb_generate_undistort_maps eorb_hamming_bf_knn2 eorb_hamming_window_match
eorb_kb8_triangulate_matches eorb_kfdb_add eorb_measure_image_focus_n eorb_mlpnp_ransac eorb_new_map_points eorb_normalize_minmax_u8 eorb_orb_extract
eorb_parse_events_text eorb_project_frustum eorb_project_keyframe_points eorb_project_last_frame eorb_search_by_projection_last_fisheye
eorb_search_by_projection_map_fisheye eorb_search_by_sim3 eorb_search_for_initialization eorb_search_local_points eorb_search_local_points_fisheye
eorb_sim3_ransac eorb_sort_by_response eorb_two_view_check_rt eorb_two_view_ransac eorb_two_view_reconstruct eorb_undistort_events""".split()

# the shared bodies that construct one, and the exports that reach them
COMMON = {
    "ev_host_common": "eorb_ev2im eorb_ev2im_gauss eorb_ev2im_gauss_raw eorb_ev2im_raw",
    "mci_common": "eorb_ev2mci_se3 eorb_ev2mci_se2 eorb_ev2mci_se3_cam eorb_ev2mci_se2_cam",
    "undistort_common": "eorb_undistort_keypoints eorb_undistort_points",
    "tracked_common": "eorb_orb_tracked_descriptors eorb_orb_assign_level_by_best_desc",
    "proj_last_common": "eorb_search_by_projection_last eorb_search_by_projection_last_stereo eorb_search_by_projection_kf",
    "proj_map_common": "eorb_search_by_projection_map eorb_search_by_projection_map_stereo",
    "proj_pose_common": "eorb_search_by_projection_last_pose eorb_search_by_projection_kf_pose",
    "search_tri_common": "eorb_search_for_triangulation eorb_search_for_triangulation_kb8 eorb_search_for_triangulation_keyframes "
                         "eorb_search_for_triangulation_kb8_keyframes eorb_create_new_map_points eorb_create_new_map_points_kb8",
    "bow_common": "eorb_search_by_bow eorb_search_by_bow_kf eorb_search_by_bow_fisheye eorb_search_by_bow_keyframes eorb_search_by_bow_kf_keyframes",
    "kf_radius_common": "eorb_kf_radius_match eorb_kf_radius_match_stereo eorb_kf_radius_match_mixed",
    "project_kfside_common": "eorb_project_keyframe_side eorb_project_keyframe_side_mixed",
    "fuse_common": "eorb_fuse_pose eorb_fuse_keyframes eorb_fuse_pose_mixed eorb_fuse_keyframes_mixed eorb_search_by_projection_kf_scw "
                   "eorb_search_by_projection_kf_scw_mixed",
    "kfdb_detect": "eorb_kfdb_detect_reloc eorb_kfdb_detect_nbest",
    "eorb_measure_image_focus_n": "eorb_measure_image_focus",
}
NEEDS_A_CASE = sorted(set(ARENA) | {name for names in COMMON.values() for name in names.split()})


def test_the_table_has_every_export_and_nothing_else():
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    missing = sorted(set(_lib.EXPORTS) - set(dc.TABLE)); extra = sorted(set(dc.TABLE) - set(_lib.EXPORTS))
    assert not missing and not extra, "exports without an entry: %s; entries that are no export: %s" % (missing, extra)


def test_every_arena_building_export_has_a_case():
    assert len(ARENA) == 35 and not set(NEEDS_A_CASE) - set(_lib.EXPORTS)
    without = [name for name in NEEDS_A_CASE if not (isinstance(dc.TABLE.get(name), list) and len(dc.TABLE[name]) >= 1)]
    assert not without, "exports that lay a call out in the arena and have no case: %s" % without


def test_every_entry_is_a_case_list_a_walk_or_a_reason():
    for name, v in dc.TABLE.items():
        if isinstance(v, list):
            assert v and all(isinstance(c, dc.Case) and c.name for c in v), name
            assert len({c.name for c in v}) == len(v), "%s: two cases of one name" % name
        elif v == dc.WALK:
            assert name.endswith("_dev"), name
        else:
            assert isinstance(v, str) and len(v) > 10 and name not in NEEDS_A_CASE, name
    assert set(dc.WALKS) == {n for n in _lib.EXPORTS if n.startswith("eorb_fe_run_batch")}
