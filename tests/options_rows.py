"""The switch table of eorb_slam_amd/csrc/eorb_options.h as literals, by hand: what the table must say (tests/test_options_cpp.py,
tests/test_gpu_options.py)."""

# option -> (environment name or None, default)
ROWS = {
    "octree_pool_shrink": (None, 0), "octree_force_global": (None, 0), "octree_list_algorithm": (None, 0), "orb_three_launches": (None, 0),
    "win_list_cap": (None, 0), "win_pool_cap": (None, 0), "win_lds_entries": (None, 0), "gather_form": (None, 0), "slot_hot_cap": (None, 0),
    "kfdb_initial_slots": (None, 0), "kfdb_finish_lds_entries": (None, 0),
    "dedupe_min_events": (None, 1 << 20), "position_dict": (None, 1), "dirty_fill": (None, -1),
    "slot_rank": ("EORB_SLOT_RANK", 1), "slot_hot_min": ("EORB_SLOT_HOT_MIN", -1), "slot_hot_waves": ("EORB_SLOT_HOT_WAVES", 0),
    "slot_prerank": ("EORB_SLOT_PRERANK", 1), "slot_halves": ("EORB_SLOT_HALVES", -1),
    "scatter": ("EORB_SCATTER", 2), "gather_threads": ("EORB_GATHER_THREADS", 0), "gather_nc": ("EORB_GATHER_NC", 0),
    "slot_chunk": ("EORB_SLOT_CHUNK", 0), "slot_waves": ("EORB_SLOT_WAVES", 0), "slot_rounds": ("EORB_SLOT_ROUNDS", 0),
    "win_cand_waves": ("EORB_WIN_CAND_WAVES", 0), "win_qpb": ("EORB_WIN_QPB", 0),
    "upload_kernel_max": ("EORB_UPLOAD_KERNEL_MAX", 1 << 20), "download_kernel_max": ("EORB_DOWNLOAD_KERNEL_MAX", 1 << 20),
    "sync_spin": ("EORB_SYNC_SPIN", 0), "slice_zero_copy": ("EORB_SLICE_ZERO_COPY", 1), "image_zero_copy": ("EORB_IMAGE_ZERO_COPY", 1),
    "contest_direct_max": ("EORB_CONTEST_DIRECT_MAX", 49152),
    "octree_budget_kb": ("EORB_OCT_BUDGET_KB", 156), "octree_direct": ("EORB_OCT_DIRECT", 1), "octree_dynamic": ("EORB_OCT_DYNAMIC", 1),
    "orb_describe": ("EORB_ORB_DESCRIBE", 1),
}
DEFAULTS = {k: v[1] for k, v in ROWS.items()}

# every environment name at a legal value of its own, none at its default (a flag is on for any non-zero value)
SEED = {
    "EORB_SLOT_RANK": 27, "EORB_SLOT_HOT_MIN": 5000, "EORB_SLOT_HOT_WAVES": 96, "EORB_SLOT_PRERANK": 26, "EORB_SLOT_HALVES": 3,
    "EORB_SCATTER": 1, "EORB_GATHER_THREADS": 384, "EORB_GATHER_NC": 4, "EORB_SLOT_CHUNK": 1024, "EORB_SLOT_WAVES": 8, "EORB_SLOT_ROUNDS": 6,
    "EORB_WIN_CAND_WAVES": 16, "EORB_WIN_QPB": 32, "EORB_UPLOAD_KERNEL_MAX": 65536, "EORB_DOWNLOAD_KERNEL_MAX": 131072, "EORB_SYNC_SPIN": 11,
    "EORB_SLICE_ZERO_COPY": 21, "EORB_IMAGE_ZERO_COPY": 22, "EORB_CONTEST_DIRECT_MAX": 20000, "EORB_OCT_BUDGET_KB": 120, "EORB_OCT_DIRECT": 23,
    "EORB_OCT_DYNAMIC": 24, "EORB_ORB_DESCRIBE": 25,
}
SEEDED = dict(DEFAULTS, **{opt: SEED[env] for opt, (env, _) in ROWS.items() if env})

# the rows with a "not set" range: row -> a value inside it (< 0; slot_hot_waves: <= 0)
NOT_SET = {"slot_rank": -1, "slot_hot_min": -1, "slot_hot_waves": 0, "slot_prerank": -1, "slot_halves": -1}
