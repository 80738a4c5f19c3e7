"""GPU: map-point creation for all older keyframes in one device call
(sfm_matcher_pair_points_first) against a loop of sfm_matcher_pair_points over
the same pairs -- integers exactly, points by bits -- and the live loop with
batch_pairs=True against the pair-by-pair device_mapping=True run."""
import ctypes

import numpy as np
import pytest

from map_points_composed import composed
from sfm_amd._ffi import SfmError, lib, ptr
from sfm_amd.live import MAX_REPR_ERR, KeypointStream, LiveSfM
from sfm_amd.mapping import _rodrigues
from sfm_amd.matcher import FeatureMatcher

pytestmark = pytest.mark.gpu

OLD = (0, 10, 20, 30, 40, 50)   # stream frames stored in slots 0-5
NEW, NEW_SLOT = 55, 6           # the new keyframe


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class _Keyframes:
    """KeypointStream(n_landmarks=N) frames 0, 10, ..., 50 as keyframe slots
    0-5 and frame 55 as slot 6, with the stream's true poses.  The camera
    moves about 2 px a frame and the match window is 40 px, so slots 4 and 5
    give points and slots 0-2 none (asserted from the pair-by-pair loop in
    test_position_of_the_first_productive_pair)."""

    def __init__(self, n_landmarks, desc_bytes=64):
        st = KeypointStream(n_landmarks=n_landmarks, desc_bytes=desc_bytes)
        self.K = st.K
        self.m = FeatureMatcher(desc_bytes)
        self.n, self.R, self.t, self.pts = [], [], [], []
        for slot, k in enumerate(OLD + (NEW,)):
            pts, desc, _ = st.frame(k)
            r, t = st.pose(k)
            self.m.store_keyframe(slot, pts, desc)
            self.pts.append(pts)
            self.n.append(len(pts))
            self.R.append(_rodrigues(r))
            self.t.append(np.asarray(t, np.float64))
        self.all1 = np.arange(self.n[NEW_SLOT], dtype=np.int32)
        self._single = {}

    def rows(self, slot):
        return np.arange(self.n[slot], dtype=np.int32)

    def item(self, slot, idx0=None, pose=None):
        """(slot, rows, R, t): pose = the slot whose pose the item is given."""
        p = slot if pose is None else pose
        return slot, (self.rows(slot) if idx0 is None else np.asarray(idx0, np.int32)), self.R[p], self.t[p]

    def single(self, it, idx1):
        """pair_points of one item, computed once per distinct item."""
        key = (it[0], it[1].tobytes(), it[2].tobytes(), it[3].tobytes(), idx1.tobytes())
        if key not in self._single:
            self._single[key] = self.m.pair_points(it[0], it[1], NEW_SLOT, idx1, self.K, it[2], it[3], self.K,
                                                   self.R[NEW_SLOT], self.t[NEW_SLOT], MAX_REPR_ERR)
        return self._single[key]

    def batched(self, items, idx1, **kw):
        return self.m.pair_points_first([it[0] for it in items], [it[1] for it in items], NEW_SLOT, idx1, self.K,
                                        np.array([it[2] for it in items]).reshape(-1, 3, 3),
                                        np.array([it[3] for it in items]).reshape(-1, 3), self.K, self.R[NEW_SLOT],
                                        self.t[NEW_SLOT], MAX_REPR_ERR, **kw)

    def check(self, items, idx1=None, label=""):
        """One batched call against the loop of single calls; -> (first, kept, matched)."""
        idx1 = self.all1 if idx1 is None else np.asarray(idx1, np.int32)
        ref = [self.single(it, idx1) for it in items]
        kept = [len(r[0]) for r in ref]
        matched = [r[3] for r in ref]
        want = next((b for b, k in enumerate(kept) if k > 0), -1)
        first, m0, m1, X, n_kept, n_matched = self.batched(items, idx1)
        print(f"{label}: {len(items)} items, rows {[len(it[1]) for it in items][:12]} x {len(idx1)}, "
              f"first {first} (want {want}), kept {kept[:12]}, matched {matched[:12]}")
        assert first == want
        assert n_kept.tolist() == kept and n_matched.tolist() == matched
        if want >= 0:
            assert np.array_equal(m0, ref[want][0]) and np.array_equal(m1, ref[want][1])
            assert _bits(X, ref[want][2])
        else:
            assert len(m0) == len(m1) == len(X) == 0
        return first, kept, matched


@pytest.fixture(scope="module")
def kfs():
    made = {}

    def get(n, desc_bytes=64):
        if (n, desc_bytes) not in made:
            made[(n, desc_bytes)] = _Keyframes(n, desc_bytes)
        return made[(n, desc_bytes)]
    yield get
    for f in made.values():
        f.m.close()


def test_single_call_equals_match_triangulate_filter(kfs):
    """The reference of check(), _Keyframes.single, runs the batch's own host
    path and kernels with one pair, so here it is pinned itself -- on the
    kinds of item the cases below use -- against the calls it fuses
    (map_points_composed: match_keyframes, sfm_triangulate_points and the CPU
    restatement of the filter), which share none of that code."""
    f, f32 = kfs(1200), kfs(1200, 32)

    def pinned(g, it, label):
        m0, m1, X, n_matched = g.single(it, g.all1)
        pi, ci, Xa, keep = composed(g.m, it[0], g.pts[it[0]], it[1], NEW_SLOT, g.pts[NEW_SLOT], g.all1, g.K, it[2],
                                    it[3], g.R[NEW_SLOT], g.t[NEW_SLOT], MAX_REPR_ERR)
        print(f"{label}: rows {len(it[1])} x {len(g.all1)}, matched {n_matched}, kept {len(m0)}")
        assert n_matched == len(pi)
        assert np.array_equal(m0, pi[keep]) and np.array_equal(m1, ci[keep])
        assert _bits(X, Xa[keep])
        return n_matched, len(m0)

    assert pinned(f, f.item(0), "slot 0")[1] == 0
    assert pinned(f, f.item(4), "slot 4")[1] >= 1
    nm5, nk5 = pinned(f, f.item(5), "slot 5")
    assert nk5 >= 1
    assert pinned(f, f.item(5, pose=NEW_SLOT), "slot 5, F = 0") == (nm5, 0) and nm5 > 0
    good = f.rows(5)[f.single(f.item(5), f.all1)[0]]          # rows that give a point go first, as in the cases below
    rows = np.concatenate([good, np.setdiff1d(f.rows(5), good)]).astype(np.int32)
    for n in (1, 63, 65):
        pinned(f, f.item(5, rows[:n]), f"slot 5, {n} rows")
    assert pinned(f, f.item(5, f.rows(5)[::-1].copy()), "slot 5, reversed")[1] >= 1
    assert pinned(f32, f32.item(5), "slot 5, desc_bytes = 32")[1] >= 1


@pytest.mark.parametrize("n_landmarks", [1200, 8000])
def test_position_of_the_first_productive_pair(kfs, n_landmarks):
    f = kfs(n_landmarks)
    first, kept, _ = f.check([f.item(s) for s in range(6)], label=f"N = {n_landmarks}, slots 0..5")
    # the pattern the other cases rely on, from the pair-by-pair loop itself
    assert kept[0] == kept[1] == kept[2] == 0 and kept[4] > 0 and kept[5] > 0
    assert first == next(b for b in range(6) if kept[b] > 0) and 3 <= first <= 4      # in the middle
    assert f.check([f.item(s) for s in (5, 4, 3, 2, 1, 0)], label="slots 5..0")[0] == 0
    assert f.check([f.item(s) for s in (0, 1, 2)], label="slots 0, 1, 2")[0] == -1


@pytest.mark.parametrize("n_landmarks", [1200, 8000])
def test_an_item_that_matches_but_keeps_nothing_is_skipped(kfs, n_landmarks):
    """Slot 5 given the new keyframe's own pose: F = 0, every distance is NaN."""
    f = kfs(n_landmarks)
    first, kept, matched = f.check([f.item(0), f.item(5, pose=NEW_SLOT), f.item(5)], label="F = 0 ahead")
    assert first == 2 and kept[1] == 0 and matched[1] > 0 and matched[1] == matched[2]


@pytest.mark.parametrize("n_landmarks", [1200, 8000])
def test_item_sizes_inside_one_call(kfs, n_landmarks):
    """1, 63, 65 and all rows, an empty item, a reversed subset, one slot twice
    with different subsets; every rotation of the list, so that each item is
    seen at each position and the sized items come first in turn."""
    f = kfs(n_landmarks)
    good = f.rows(5)[f.single(f.item(5), f.all1)[0]]          # rows of slot 5 that give a point: they go first
    rows = np.concatenate([good, np.setdiff1d(f.rows(5), good)]).astype(np.int32)
    assert len(good) >= 1 and len(rows) == f.n[5] > 65
    items = [f.item(5, []), f.item(1), f.item(5, rows[:1]), f.item(5, rows[:63]), f.item(5, rows[:65]),
             f.item(5, f.rows(5)[::-1].copy()), f.item(4), f.item(5, f.rows(5)[f.n[5] // 2:]), f.item(5)]
    firsts = set()
    for r in range(len(items)):
        rot = items[r:] + items[:r]
        firsts.add(len(rot[f.check(rot, label=f"rotation {r}")[0]][1]))
    assert {1, 63, 65, f.n[5], f.n[4]} <= firsts


def test_one_train_row_and_no_items(kfs):
    f = kfs(1200)
    items = [f.item(s) for s in (4, 5)]
    first, kept, matched = f.check(items, idx1=[3], label="n1 = 1")
    assert first == -1 and not any(kept) and not any(matched)
    first, m0, m1, X, n_kept, n_matched = f.batched([], f.all1)
    assert first == -1 and len(m0) == len(X) == len(n_kept) == len(n_matched) == 0
    assert f.check([f.item(4, []), f.item(5, [])], label="two empty items")[0] == -1
    assert f.check(items, idx1=f.all1[:2], label="n1 = 2")[0] in (-1, 0, 1)


def test_seventy_items_cross_one_wave_in_the_pick(kfs):
    f = kfs(1200)
    good = f.rows(5)[f.single(f.item(5), f.all1)[0]]
    items = [f.item(b % 3, f.rows(b % 3)[8 * (b // 3 % 10):8 * (b // 3 % 10) + 8]) for b in range(70)]
    items[66] = f.item(5, good[:8])
    assert all(len(it[1]) == 8 for it in items)
    first, kept, _ = f.check(items, label="B = 70")
    assert first == 66 and sum(k > 0 for k in kept) == 1


def test_descriptors_of_32_bytes(kfs):
    f = kfs(1200, 32)
    first, kept, _ = f.check([f.item(s) for s in range(6)], label="desc_bytes = 32")
    assert first >= 3 and kept[5] > 0


def test_the_same_call_twice_gives_the_same_bits(kfs):
    f = kfs(8000)
    items = [f.item(s) for s in range(6)]
    a, b = f.batched(items, f.all1), f.batched(items, f.all1)
    assert a[0] == b[0] >= 0 and len(a[1]) > 0
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and _bits(a[3], b[3])


def test_errors_leave_the_handle_usable(kfs):
    f = kfs(1200)
    items = [f.item(s) for s in (0, 4, 5)]
    good = f.batched(items, f.all1)
    nk = int(good[4][good[0]])
    assert good[0] == 1 and nk > 1

    def refused(items, idx1, **kw):
        with pytest.raises(SfmError) as e:
            f.batched(items, idx1, **kw)
        assert e.value.code == -22 and len(str(e.value).split(": ", 1)[1]) > 3, str(e.value)
        return e.value

    def same_as_good():
        again = f.batched(items, f.all1)
        assert again[0] == good[0] and all(np.array_equal(x, y) for x, y in zip(good[1:], again[1:]))
        assert _bits(good[3], again[3])

    refused([f.item(0), (9, f.rows(0), f.R[0], f.t[0])], f.all1)                    # unstored slot
    refused([f.item(0), (NEW_SLOT, f.rows(0), f.R[0], f.t[0])], f.all1)             # slot0 == slot1
    same_as_good()
    refused([f.item(4), f.item(5, [0, f.n[5]])], f.all1)                            # row out of range
    refused(items, [0, -1])
    refused([f.item(4), (5, f.rows(5), f.R[5] * np.nan, f.t[5])], f.all1)           # compose_pair fails
    same_as_good()
    e = refused(items, f.all1, capacity=nk - 1)                                     # capacity too small
    assert e.first == good[0] and e.n_kept.tolist() == good[4].tolist() and e.n_matched.tolist() == good[5].tolist()
    same_as_good()
    # non-monotone offsets and NULL outputs, straight at the C ABI
    s0 = np.array([4, 5], np.int32)
    i0 = np.concatenate([f.rows(4), f.rows(5)])
    off = np.array([0, f.n[4], f.n[4] + f.n[5]], np.int32)
    K9 = np.ascontiguousarray(np.tile(f.K.reshape(1, 9), (2, 1)))
    R9 = np.ascontiguousarray(np.stack([f.R[4], f.R[5]]).reshape(2, 9))
    t3 = np.ascontiguousarray(np.stack([f.t[4], f.t[5]]))
    K1, R1, t1 = (np.ascontiguousarray(x, np.float64).reshape(-1) for x in (f.K, f.R[NEW_SLOT], f.t[NEW_SLOT]))
    cap = max(f.n[4], f.n[5])
    o0, o1, X = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 3))
    nk2, nm2, first = np.zeros(2, np.int32), np.zeros(2, np.int32), ctypes.c_int32(7)

    def call(off_, outs):
        return lib().sfm_matcher_pair_points_first(f.m._h, 2, ptr(s0), ptr(i0), ptr(off_), NEW_SLOT, ptr(f.all1),
                                                   len(f.all1), 0.8, 1.5, 40.0, ptr(K9), ptr(R9), ptr(t3), ptr(K1),
                                                   ptr(R1), ptr(t1), 7.0, cap, *outs)

    ok = (ctypes.byref(first), ptr(o0), ptr(o1), ptr(X), ptr(nk2), ptr(nm2))
    for bad in (np.array([0, f.n[4] + 1, f.n[4]], np.int32), np.array([1, f.n[4], f.n[4] + f.n[5]], np.int32)):
        assert call(bad, ok) == -22 and lib().sfm_last_error()
    for k in range(6):
        assert call(off, ok[:k] + (None,) + ok[k + 1:]) == -22 and lib().sfm_last_error()
    assert call(off, ok) == 0 and first.value == 0 and nk2[0] > 0 and nk2[1] > 0     # the good call, same arrays
    want = f.single(f.item(4), f.all1)
    assert np.array_equal(o0[:nk2[0]], want[0]) and np.array_equal(o1[:nk2[0]], want[1])
    assert _bits(X[:nk2[0]], want[2]) and nm2[0] == want[3]
    same_as_good()


# ---- the live loop -------------------------------------------------------------

@pytest.fixture(scope="module")
def runs():
    a = LiveSfM(KeypointStream(), device_mapping=True)
    b = LiveSfM(KeypointStream(), device_mapping=True, batch_pairs=True)
    a.run(60)
    b.run(60)
    yield a, b
    a.close()
    b.close()


def test_loop_batched_equals_pair_by_pair(runs):
    a, b = runs
    print("pair by pair:", [f.no for f in a.kfs], a.stats, len(a.map_log), "matcher calls")
    print("batched     :", [f.no for f in b.kfs], b.stats, len(b.map_log), "matcher calls")
    assert a.lost == 0 and b.lost == 0
    assert [f.no for f in a.kfs] == [f.no for f in b.kfs] and len(b.kfs) >= 5
    for fa, fb in zip(a.kfs, b.kfs):
        assert np.array_equal(fa.pt3d, fb.pt3d)
    assert a.map.size() == b.map.size() and a.stats == b.stats
    frames = [f.no for f in a.kfs]
    for (a3, a2), (b3, b2) in zip(a.map.getPointsInFrameMulti(frames), b.map.getPointsInFrameMulti(frames)):
        assert np.array_equal(a3, b3) and np.array_equal(a2, b2)
    ids = np.arange(a.map.size()[0], dtype=np.int32)
    assert _bits(a.map.getPointsAtIdx(ids), b.map.getPointsAtIdx(ids))
    assert len(a.ba_log) == len(b.ba_log) == len(a.kfs) - 1
    for ra, rb in zip(a.ba_log, b.ba_log):
        for k in ("cam_idx", "pt_idx"):
            assert np.array_equal(ra[k], rb[k]), k
        for k in ("uv", "K", "rot", "t", "X", "rot_out", "t_out", "X_out"):
            assert _bits(ra[k], rb[k]), k
        sa, sb = ra["summary"].as_dict(), rb["summary"].as_dict()
        for k in sa:
            if not k.endswith("_time_s"):
                assert sa[k] == sb[k], k
        assert ra["trace"] == rb["trace"]
    # strictly fewer matcher calls than the pair-by-pair run made
    assert 0 < len(b.map_log) < len(a.map_log)


def test_loop_batched_calls_replay_through_pair_points(runs):
    _, s = runs
    kept = 0
    for e in s.map_log:
        want_first = -1
        for b, (slot0, idx0) in enumerate(zip(e["slots0"], e["idx0"])):
            m0, m1, X, nm = s.matcher.pair_points(slot0, idx0, e["slot1"], e["idx1"], e["K"], e["R0s"][b], e["t0s"][b],
                                                  e["K"], e["R1"], e["t1"], MAX_REPR_ERR)
            assert e["n_kept"][b] == len(m0) and e["n_matched"][b] == nm
            if len(m0) and want_first < 0:
                want_first = b
                assert np.array_equal(e["m0"], m0) and np.array_equal(e["m1"], m1) and _bits(e["X"], X)
        assert e["first"] == want_first
        kept += len(e["m0"])
    assert kept == s.stats["new_points"] - len(s.ba_log[0]["X"])   # all but the initial pair's
