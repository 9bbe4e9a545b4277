"""Every host-buffer entry point on device memory that is not zero (GPU).  The table of tests/dirty_cases.py is run in three states, each
on one context of its own that the whole module shares:

  clean         a context without the hook: pins a case to its reference.  A failure here is a broken case, not a finding;
  filled        eorb_debug_option("dirty_fill", 0xFF) right after eorb_create: every allocation, the whole arena before every call, the
                staging slot and the landing buffer hold 0xFF.  A failure here alone is a read of memory that nothing wrote;
  after larger  no hook; right before the case the same entry point runs a scene three times as large (results thrown away), so every
                region of the small call lies in memory that holds values which look like results.  A second pass runs the cases in
                reversed order, without the larger call: each inherits an unrelated call's arena.  A failure here alone is a stale
                value taken for a result.

The workspaces that persist across calls are not reached by a per-call fill: four shape walks on one filled context each (the batch
step, the window matchers' pair counters, the LK pyramids, the KeyFrameDatabase pools) compare every step with the CPU side.

The references come from the oracle and the restatements only (dirty_cases.Case.want, computed once per case); nothing is compared with
another run of the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_cases as dc                            # noqa: E402
from eorb_slam_amd import _lib, synth               # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xFF
CASES = dc.all_cases()
IDS = ["%s-%d" % (name[5:], i) for i, (name, _) in enumerate(CASES)]
REVERSED = list(reversed(CASES))
REVERSED_IDS = list(reversed(IDS))


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


def _context(fe, fill):
    c = fe.Context()
    if fill:
        c.debug_option("dirty_fill", FILL)
    return c


@pytest.fixture(scope="module")
def clean(fe):
    c = _context(fe, False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def filled(fe):
    c = _context(fe, True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def after(fe):
    c = _context(fe, False)
    yield c
    c.close()


def _check(fe, ctx, name, case, state):
    dc.same(case.run(fe, ctx), case.want(), "%s [%s], state '%s'" % (name, case.name, state), case.canon)


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_clean(fe, clean, name, case):
    _check(fe, clean, name, case, "clean")


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_filled(fe, filled, name, case):
    _check(fe, filled, name, case, "filled")


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_after_a_larger_call(fe, after, name, case):
    case.run_big(fe, after)
    _check(fe, after, name, case, "after larger")


@pytest.mark.parametrize("name,case", REVERSED, ids=REVERSED_IDS)
def test_after_an_unrelated_call(fe, after, name, case):
    _check(fe, after, name, case, "after larger (reversed order)")


def test_the_hook_takes_a_byte_or_minus_one(fe):
    c = fe.Context()
    try:
        for v in (0, 255, -1):
            c.debug_option("dirty_fill", v)
        for v in (-2, 256):
            with pytest.raises(fe.EorbError) as e:
                c.debug_option("dirty_fill", v)
            assert e.value.code == _lib.EORB_E_ARG
    finally:
        c.close()


# ---- the walks -------------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.nbytes == b.nbytes and a.tobytes() == b.tobytes()


def _first(a, b):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8); b = np.ascontiguousarray(b).reshape(-1).view(np.uint8)
    bad = np.flatnonzero(a != b) if a.size == b.size else np.array([-1])
    return "%d bytes differ, first at %d" % (len(bad), int(bad[0]))


BATCH_ORB = (200, 1.2, 1, 10, 0, 9)
BATCH_STEPS = [(64, 48, 3, 6000), (70, 50, 5, 20000), (64, 48, 2, 700), (64, 48, 3, 6000)]


def _batch_maps(W, H):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (xx + 1.5 * np.sin(yy / 19.0) - 0.5).astype(np.float32), (yy + 1.0 * np.cos(xx / 29.0) + 0.5).astype(np.float32)


def _batch_events(W, H, B, n, seed):
    """B slices of n raw events: most of them on a dozen small blobs that move a pixel from slice to slice (corners for the extractor
    that the next slice finds again), the rest anywhere"""
    rng = np.random.default_rng(seed)
    cx, cy = rng.integers(12, W - 12, 12), rng.integers(12, H - 12, 12)
    out = []
    for b in range(B):
        raw = synth.random_raw_events(n, W, H, seed=seed * 10 + b)
        k = (9 * n) // 10
        r2 = np.random.default_rng(seed * 100)                              # (the same blobs in every slice)
        pick = r2.integers(0, 12, k)
        dx, dy = r2.integers(-2, 3, k), r2.integers(-2, 3, k)
        raw["x"][:k] = np.clip(cx[pick] + dx + b % 2, 0, W - 1); raw["y"][:k] = np.clip(cy[pick] + dy, 0, H - 1)
        raw["t"] = np.arange(n) * 1e-6
        out.append(raw)
    return out


class _Out:
    """the caller's output buffers of a batch call, every byte 0xFF before the call"""

    def __init__(self, c, B, cap, W, H, images=True):
        self.c, self.B, self.cap, self.W, self.H = c, B, cap, W, H
        sizes = dict(img=B * W * H if images else 0, kp=B * cap * 28, desc=B * cap * 32, n=B * 4, m=B * cap * 4, nm=B * 4)
        self.d = {}
        for k, nb in sizes.items():
            if nb:
                self.d[k] = c.dev_alloc(nb)
                c.upload(self.d[k], np.full(nb, FILL, np.uint8))

    def get(self):
        c, B, cap = self.c, self.B, self.cap
        o = dict(n=np.zeros(B, np.int32), kp=np.zeros((B, cap), synth.KP_DTYPE), desc=np.zeros((B, cap, 32), np.uint8), m=np.zeros((B, cap), np.int32),
                 nm=np.zeros(B, np.int32))
        if "img" in self.d:
            o["img"] = np.zeros((B, self.H, self.W), np.uint8)
        for k, a in o.items():
            c.download(a, self.d[k])
        return o

    def free(self):
        for p in self.d.values():
            self.c.dev_free(p)


def _batch_want(orc, u8s, W, H, prev=None):
    """the oracle's extraction of every image and SearchForInitialization of image b against image b - 1 (prev: the carried one)"""
    oe = orc.OrbExtractor(*BATCH_ORB[:5], edgeTh=BATCH_ORB[5], imWidth=W)
    out = []
    for u8 in u8s:
        _, kp, desc, _ = oe.extract(u8)
        row = dict(kp=kp, desc=desc)
        if prev is not None:
            pm = np.stack([prev["kp"]["x"], prev["kp"]["y"]], axis=1)
            n, m, _ = orc.search_for_initialization(orc.Frame(prev["kp"], prev["desc"], W, H), orc.Frame(kp, desc, W, H), pm, 100, 0.9, True)
            row.update(nm=n, m=m)
        out.append(row)
        prev = row
    return out


def _batch_compare(what, got, want, u8s=None, first_pair=True):
    for b, w in enumerate(want):
        n = len(w["kp"])
        assert got["n"][b] == n, "%s, slice %d: %d keypoints, the oracle %d" % (what, b, got["n"][b], n)
        assert _bits(got["kp"][b, :n], w["kp"]), "%s, slice %d: keypoints: %s" % (what, b, _first(got["kp"][b, :n], w["kp"]))
        assert _bits(got["desc"][b, :n], w["desc"]), "%s, slice %d: descriptors: %s" % (what, b, _first(got["desc"][b, :n], w["desc"]))
        if u8s is not None:
            assert _bits(got["img"][b], u8s[b]), "%s, slice %d: image: %s" % (what, b, _first(got["img"][b], u8s[b]))
        if "nm" in w:
            k = len(w["m"])
            assert got["nm"][b] == w["nm"] and _bits(got["m"][b, :k], np.asarray(w["m"], np.int32)), "%s, slice %d: matches %d, the oracle %d: %s" % (
                what, b, got["nm"][b], w["nm"], _first(got["m"][b, :k], np.asarray(w["m"], np.int32)))
        elif first_pair:
            assert got["nm"][b] == 0 and (got["m"][b] == -1).all(), "%s, slice %d has no partner: nmatches %d" % (what, b, got["nm"][b])


@pytest.mark.parametrize("form", [1, 4], ids=["lds-gather", "slot-lists"])
def test_batch_step_walk(fe, form):
    """eorb_fe_run_batch_raw_dev, _raw4_dev, _raw2_dev, _dev and _images_dev over batches that grow, shrink and grow again on one filled
    context, the caller's output buffers filled with 0xFF: images, keypoints, descriptors, counts and matches against the oracle"""
    orc = dc.orc()
    c = _context(fe, True)
    try:
        c.debug_option("gather_form", form)
        c.debug_option("dedupe_min_events", 1 << 20)
        for step, (W, H, B, n) in enumerate(BATCH_STEPS):
            mx, my = _batch_maps(W, H)
            raws = _batch_events(W, H, B, n, 11 + step)
            evs = [orc.undistort_events(r, mx, my, W, H, True, 1.0) for r in raws]
            u8s = [orc.ev2im_gauss(e, W, H, 1.0, False, True)[1] for e in evs]
            want = _batch_want(orc, u8s, W, H)
            off = np.arange(B + 1, dtype=np.int64) * n
            blobs = {True: np.concatenate(raws), 4: np.concatenate([fe.pack_raw_events4(r) for r in raws]),
                     2: np.concatenate([fe.pack_raw_events2(r, W) for r in raws]), False: None}
            for fmt in (True, 4, 2, False, "images"):
                what = "step %d (%dx%d, B %d, %d events), form %d, entry %s" % (step, W, H, B, n, form, {True: "raw", 4: "raw4", 2: "raw2", False: "float"}.get(fmt, fmt))
                fb = fe.FrontEndBatch(W, H, 1.0, False, *BATCH_ORB, max_batch=B, max_events=n, ctx=c)
                fe.EvImConverter.set_undistort_maps(mx, my, True, ctx=c)
                out = _Out(c, B, fb.cap, W, H, images=fmt != "images")
                if fmt == "images":
                    blob = np.concatenate([u.ravel() for u in u8s])
                    d_in = c.dev_alloc(blob.nbytes); c.upload(d_in, blob)
                    fb.run_images_dev(d_in, B, out.d["kp"], out.d["desc"], out.d["n"], out.d["m"], out.d["nm"])
                else:
                    if fmt is False:                                        # the float events of the slices, which are not all n long
                        blob = np.concatenate([fe.pack_events(e) for e in evs])
                        foff = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.int64)
                    else:
                        blob, foff = blobs[fmt], off
                    d_in = c.dev_alloc(max(blob.nbytes, 16)); c.upload(d_in, blob)
                    fb.run_dev(d_in, foff, out.d["img"], out.d["kp"], out.d["desc"], out.d["n"], out.d["m"], out.d["nm"], raw=fmt)
                c.sync()
                _batch_compare(what, out.get(), want, None if fmt == "images" else u8s)
                out.free(); c.dev_free(d_in)
    finally:
        c.close()


def _frames(W, H, n, seed):
    base = synth.texture_image(W, H, seed=seed)
    return [np.ascontiguousarray(np.roll(base, (i % 3, -(2 * i % 5)), axis=(0, 1))) for i in range(n)]


def test_window_matcher_pair_counter_walk(fe):
    """5 pairs, then 2 with the list and pool capacities shrunk so that the lists overflow into the full scan, then a call refused for
    its batch size, then 5 again: every call's matches against the oracle, and the pairs' entry counters (win_total) at zero after
    each of them"""
    orc = dc.orc()
    W, H = dc.W, dc.H
    c = _context(fe, True)
    try:
        fb = fe.FrontEndBatch(W, H, 1.0, False, *BATCH_ORB, max_batch=6, max_events=1, ctx=c)
        frames = _frames(W, H, 13, 77)
        want = _batch_want(orc, frames, W, H)
        assert all(len(w["kp"]) > 20 for w in want) and sum(w["nm"] for w in want[1:]) > 50
        at = 0
        for call, (B, caps) in enumerate(((6, (0, 0)), (2, (2, 40)), (0, None), (5, (0, 0)))):
            if caps is None:                                                # refused before anything is launched
                with pytest.raises(fe.EorbError) as e:
                    fb.run_images_dev(0, 7)
                assert e.value.code == _lib.EORB_E_ARG
                assert c.debug_counter("win_total_nonzero") == 0, "call %d: a pair counter is not zero after the refused call" % call
                continue
            c.debug_option("win_list_cap", caps[0]); c.debug_option("win_pool_cap", caps[1])
            blob = np.concatenate([f.ravel() for f in frames[at:at + B]])
            d_in = c.dev_alloc(blob.nbytes); c.upload(d_in, blob)
            out = _Out(c, B, fb.cap, W, H, images=False)
            fb.run_images_dev(d_in, B, out.d["kp"], out.d["desc"], out.d["n"], out.d["m"], out.d["nm"])
            c.sync()
            _batch_compare("call %d (%d frames, caps %s)" % (call, B, caps), out.get(), want[at:at + B], first_pair=at == 0)
            assert c.debug_counter("win_total_nonzero") == 0, "call %d: a pair counter is not zero after the call" % call
            out.free(); c.dev_free(d_in)
            at += B
        c.debug_option("win_list_cap", 0); c.debug_option("win_pool_cap", 0)
        # a lone pair through the host-buffer entry point shares the counters
        a, b = want[0], want[1]
        pm = np.stack([a["kp"]["x"], a["kp"]["y"]], axis=1)
        n, m, _ = fe.ORBmatcher(0.9, True, c).SearchForInitialization(fe.FrameView(a["kp"], a["desc"], W, H), fe.FrameView(b["kp"], b["desc"], W, H), pm, 100)
        assert n == b["nm"] and _bits(m, np.asarray(b["m"], np.int32))
        assert c.debug_counter("win_total_nonzero") == 0
    finally:
        c.close()


def _lk_pair(W, H, seed):
    img1 = synth.texture_image(W, H, seed=seed)
    rng = np.random.default_rng(seed)
    img2 = np.clip(np.roll(img1, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-3, 4, (H, W)), 0, 255).astype(np.uint8)
    pts = np.stack([rng.uniform(2, W - 2, 65), rng.uniform(2, H - 2, 65)], axis=1).astype(np.float32)
    return img1, img2, pts


def test_lk_pyramid_walk(fe):
    """calcOpticalFlowPyrLK on a 70 x 50 pair, a 64 x 48 pair and the first pair again; then the L1 chain's reference frame (its pyramid
    kept under a key) with a call of another size between two tracked chunks: the key must not match the buffer the other call wrote"""
    orc = dc.orc()
    c = _context(fe, True)
    try:
        trk = fe.ELK_Tracker(9, 1, 10, 0.03, ctx=c)
        pairs = [_lk_pair(70, 50, 21), _lk_pair(64, 48, 22)]
        for step, k in enumerate((0, 1, 0)):
            img1, img2, pts = pairs[k]
            gn, gs, ge = trk.calcOpticalFlowPyrLK(img1, img2, pts, None, 0)
            on, os_, oe = orc.calc_optical_flow_pyr_lk(img1, img2, pts, None, 9, 1, 10, 0.03, 0)
            assert _bits(gn, on) and _bits(gs, os_) and _bits(ge, oe), "step %d (%dx%d): next %s, status %s, err %s" % (
                step, img1.shape[1], img1.shape[0], _first(gn, on), _first(gs, os_), _first(ge, oe))
        W, H = dc.W, dc.H
        evs = [dc._slice_events(2003, 30 + k, 0.4 + 0.3 * k) for k in range(3)]
        u8 = [orc.ev2im_gauss(e, W, H, 1.0, False, True)[1] for e in evs]
        kps, img = dc._sl_extract(fe, c, evs[0])
        assert _bits(img, u8[0])
        ref = np.stack([kps["x"], kps["y"]], axis=1).astype(np.float32)
        assert len(ref) > 10
        flow = ref
        for k in (1, 2):
            pts, st, er, cur = dc._sl_track(fe, c, evs[k], flow)
            op, os_, oe = orc.calc_optical_flow_pyr_lk(u8[0], u8[k], ref, flow, 23, 1, 10, 0.03, 4)
            assert _bits(cur, u8[k]) and _bits(pts, op) and _bits(st, os_) and _bits(er, oe), "chunk %d: points %s, status %s" % (k, _first(pts, op), _first(st, os_))
            flow = pts
            if k == 1:                                                      # another size, and a window of 23 as the chain's: the same buffers
                img1, img2, p = pairs[1]
                gn, gs, ge = fe.ELK_Tracker(23, 1, 10, 0.03, ctx=c).calcOpticalFlowPyrLK(img1, img2, p, None, 0)
                on, os_, oe = orc.calc_optical_flow_pyr_lk(img1, img2, p, None, 23, 1, 10, 0.03, 0)
                assert _bits(gn, on) and _bits(gs, os_) and _bits(ge, oe)
    finally:
        c.close()


def test_keyframe_database_pool_walk(fe):
    """add, detect, erase, detect with first pools of 2 slots and 128 words: the pools regrow several times with the fill in them"""
    import kfdb_ref
    c = _context(fe, True)
    try:
        c.debug_option("kfdb_initial_slots", 2)
        d = synth.bow_database(13, 9, vocab_words=700, words_per_kf=64, nplaces=3, nqueries=2, kf_words=[64, 40, 65, 63, 1, 64, 0, 65, 64], query_words=[65, 64])
        dev, ref = fe.KeyFrameDatabase(c), kfdb_ref.KeyFrameDatabase(d["vocab_words"])
        dev.clear()

        def query(step):
            covis = np.full((ref.n_slots, 10), -1, np.int32)
            for s in range(ref.n_slots):
                covis[s, :2] = [(s + 1) % ref.n_slots, (s + ref.n_slots - 1) % ref.n_slots]
            for i, q in enumerate(d["queries"]):
                for nbest in (0, 1):
                    if nbest:
                        want = ref.detect_nbest_candidates(q["word"], q["val"], covis=covis)
                        got = dev.detect_nbest_candidates(q["word"], q["val"], covis=covis)
                    else:
                        want = ref.detect_relocalization_candidates(q["word"], q["val"], covis=covis)
                        got = dev.detect_relocalization_candidates(q["word"], q["val"], covis=covis)
                    want.pop("stale")
                    what = "%s, query %d, nbest %d" % (step, i, nbest)
                    assert sorted(got) == sorted(want), what
                    for k, w in want.items():
                        g = got[k]
                        if isinstance(w, np.ndarray):
                            assert g.dtype == w.dtype and _bits(g, w), "%s: %s: %s" % (what, k, _first(g, w))
                        else:
                            assert np.float32(g).tobytes() == np.float32(w).tobytes(), (what, k, g, w)
                    for fam in (0, 1):
                        assert _bits(dev.scores(fam), ref.scores(fam)), "%s: stored scores of family %d" % (what, fam)
        caps = set()
        for k, (w, v) in enumerate(d["kfs"]):
            assert dev.add(w, v) == ref.add(w, v)
            caps.add((c.debug_counter("kfdb_slot_cap"), c.debug_counter("kfdb_word_cap")))
            query("after add %d" % k)
        assert len({s for s, _ in caps}) >= 3, caps
        for slot in (1, 4):
            dev.erase(slot); ref.erase(slot)
        query("after erase")
        assert dev.add(*d["kfs"][1]) == ref.add(*d["kfs"][1]) == 1
        query("after the slot is taken again")
    finally:
        c.close()
