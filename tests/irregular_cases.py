"""Seeded scenes with the visibility a tracker produces, at the camera counts
whose kernels the regular scenes alone reach (more than 64 cameras: the step
preparation folded into the evaluation; from 128 on: k_schur_pairs_rot_pw and
k_backsub_pm): points of every degree from 0 to nearly C, cameras without
observations (the last block row of S among them), (camera, point) keys
observed twice, observations in shuffled caller order.

Shared by tests/golden/make_irregular.py (which records the oracle's
trajectories, the scenes' structural counts and, for the rejecting scenes, the
oracle's disagreement with the dense numpy restatement of the loop:
tests/golden/irregular.json), tests/test_irregular_oracle.py (CPU: the scenes
are what they claim to be, inside the solver's bounds, with decisive
trajectories) and tests/test_gpu_irregular.py (GPU: the HIP solver against
the oracle).
"""
from __future__ import annotations

import numpy as np

from sfm_amd import scene

import lm_cases as L

SEED = L.SEED

# restated from sfm_amd/csrc/ba_host_layout.h (the constants ba_plan.h's plans are made from)
K_HOST_CHECK_MAX_OBS = 65536
K_STAGE_MAX_BYTES = 1 << 20
K_SMALL_SETUP_MAX_C = 256
K_SMALL_SETUP_MAX_CHUNKS = 2048
K_SMALL_SETUP_MAX_PT_OBS = 64
K_SMALL_SETUP_MAX_OBS = 64 * 1024
K_SCHUR_XCD_MIN_BLOCKS = 8192
K_CAM_PM_MAX = 512  # ba_device.h


def _rotate(rot, X):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(rot)).apply(X)


def irregular(s, seed=5, hubs=(), empty=(), dups=40, shuffle=True, maxdeg=10):
    """Makes the regular scene `s` irregular, in this order:
    1. point p keeps the first 1 + p % maxdeg of its observations (generator order);
    2. the cameras in `empty` lose every observation (points seen only by them
       stay in the problem, unobserved);
    3. each point in `hubs` gets one more observation from every non-empty
       camera that does not see it yet: its true position through the true
       pose and the camera's K, plus N(0, 0.5) px, kept where depth > 0.5 and
       |u|, |v| < 4000;
    4. `dups` observations (drawn without replacement) are appended again with
       the same camera and point and uv shifted by N(0, 0.3);
    5. all observations are shuffled."""
    rng = np.random.default_rng(seed)
    uv, cam, pt = s.uv, s.cam_idx, s.pt_idx
    # 1. (the generator emits each point's observations together, in camera order)
    first = np.searchsorted(pt, pt, side="left")
    keep = np.arange(len(pt)) - first < 1 + pt % maxdeg
    # 2.
    keep &= ~np.isin(cam, np.asarray(empty, dtype=cam.dtype))
    uv, cam, pt = uv[keep], cam[keep], pt[keep]
    # 3.
    live = np.setdiff1d(np.arange(s.n_cams), np.asarray(empty, dtype=np.int64))
    for h in hubs:
        cs = np.setdiff1d(live, cam[pt == h])
        pc = _rotate(s.rot_true[cs], s.X_true[h]) + s.t_true[cs]
        x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        K = s.K[cs]
        p = np.stack([K[:, 0] * x + K[:, 1] * y + K[:, 2], K[:, 4] * y + K[:, 5]], axis=1)
        p = p + rng.normal(0, 0.5, p.shape)
        ok = (pc[:, 2] > 0.5) & (np.abs(p[:, 0]) < 4000) & (np.abs(p[:, 1]) < 4000)
        uv = np.vstack([uv, p[ok]])
        cam = np.concatenate([cam, cs[ok].astype(cam.dtype)])
        pt = np.concatenate([pt, np.full(int(ok.sum()), h, pt.dtype)])
    # 4.
    if dups:
        d = rng.choice(len(pt), dups, replace=False)
        uv = np.vstack([uv, uv[d] + rng.normal(0, 0.3, (dups, 2))])
        cam = np.concatenate([cam, cam[d]])
        pt = np.concatenate([pt, pt[d]])
    # 5.
    if shuffle:
        perm = rng.permutation(len(pt))
        uv, cam, pt = uv[perm], cam[perm], pt[perm]
    s.uv = np.ascontiguousarray(uv, dtype=np.float64)
    s.cam_idx = np.ascontiguousarray(cam, dtype=np.int32)
    s.pt_idx = np.ascontiguousarray(pt, dtype=np.int32)
    return s


HUBS = (0, 1, 2, 3)
_REJ = dict(views=10, pt_sigma=1.0, rot_sigma=0.3, t_sigma=2.0)

# name -> (cameras, points, generate() keywords, hubs); every scene drops
# camera 7 and its last camera, doubles 40 observations and is shuffled
SCENES = {
    "irr_136": (136, 3000, dict(views=10, seed=11), HUBS),
    "irr_136_big": (136, 14000, dict(views=10, seed=11), HUBS),
    "irr_100_hub": (100, 3000, dict(views=10, seed=11), HUBS),
    "irr_100": (100, 3000, dict(views=10, seed=11), ()),
    "rej_130_irr": (130, 400, dict(seed=SEED + 219, **_REJ), HUBS),
    "rej_100_irr": (100, 400, dict(seed=SEED + 219, **_REJ), ()),
}
PLAIN = ("irr_136", "irr_136_big", "irr_100_hub", "irr_100")
REJECTING = ("rej_130_irr", "rej_100_irr")


def empty_cameras(name):
    return (7, SCENES[name][0] - 1)


def build(name):
    C, P, kw, hubs = SCENES[name]
    return irregular(scene.generate(C, P, **kw), seed=5, hubs=hubs, empty=empty_cameras(name), dups=40, shuffle=True,
                     maxdeg=10)


def pair_count_rule(cam, pt, P):
    """k_pair_count's rule (ba_setup.hip): for each observation, the other
    observations of its point with camera >= its own.  -> (total, per-block
    counts as a dict (c1, c2) -> pairs)."""
    order = np.lexsort((cam, pt))
    c, p = cam[order].astype(np.int64), pt[order]
    off = np.searchsorted(p, np.arange(P + 1))
    blocks = {}
    total = 0
    for q in range(P):
        cs = c[off[q]:off[q + 1]]
        n = len(cs)
        if n < 2:
            continue
        ge = cs[None, :] >= cs[:, None]
        np.fill_diagonal(ge, False)
        i1, i2 = np.nonzero(ge)
        total += len(i1)
        for a, b in zip(cs[i1].tolist(), cs[i2].tolist()):
            blocks[(a, b)] = blocks.get((a, b), 0) + 1
    return total, blocks


def structure(s, hubs=()):
    """Structural counts of a scene (all from the index arrays).  A block is
    a camera block (c1 <= c2) of the reduced system; it is empty when its pair
    list is (a diagonal block's list holds same-camera duplicates only)."""
    C, P = s.n_cams, s.n_pts
    cam, pt = s.cam_idx, s.pt_idx
    deg = np.bincount(pt, minlength=P)
    cdeg = np.bincount(cam, minlength=C)
    keys, cnt = np.unique(cam.astype(np.int64) * P + pt, return_counts=True)
    dup_pts = keys[cnt > 1] % P
    total, blocks = pair_count_rule(cam, pt, P)
    sizes = np.array(list(blocks.values()), np.int64)
    n_blk = C * (C + 1) // 2
    # every hub adds one pair to every block of two live cameras, so the
    # blocks of one pair are counted among the other points: unordered pairs
    # (a same-camera pair is emitted twice into its diagonal block)
    rest = ~np.isin(pt, np.asarray(hubs, pt.dtype))
    _, rb = pair_count_rule(cam[rest], pt[rest], P)
    one = sum(1 for (a, b), v in rb.items() if (v // 2 if a == b else v) == 1)
    return dict(
        n_obs=int(len(pt)), n_cams=int(C), n_pts=int(P), n_pairs=int(total), n_blk=int(n_blk),
        pairs_est=int(np.sum(deg.astype(np.int64) * (deg - 1) // 2)),
        min_degree=int(deg.min()), max_degree=int(deg.max()),
        single_view_points=int(np.sum(deg == 1)), unobserved_points=int(np.sum(deg == 0)),
        empty_cameras=int(np.sum(cdeg == 0)), duplicate_keys=int(np.sum(cnt == 2)),
        keys_seen_more_than_twice=int(np.sum(cnt > 2)),
        duplicates_on_hubs=int(np.sum(np.isin(dup_pts, np.asarray(hubs, np.int64)))),
        nonempty_blocks=int(len(sizes)), empty_blocks=int(n_blk - len(sizes)),
        one_pair_blocks=int(one), min_pairs_in_block=int(sizes.min()), max_pairs_in_block=int(sizes.max()),
        diagonal_pairs=int(sum(v for (a, b), v in blocks.items() if a == b)),
        camera_chunks=int(np.sum((cdeg + 63) // 64)))


def small_setup_sizes_fit(st, C):
    """small_setup_fits's size conditions (ba_host_layout.h) from structure()."""
    return (0 < st["n_obs"] <= K_SMALL_SETUP_MAX_OBS and 0 < C <= K_SMALL_SETUP_MAX_C
            and C * (C + 1) // 2 <= K_SCHUR_XCD_MIN_BLOCKS and st["camera_chunks"] <= K_SMALL_SETUP_MAX_CHUNKS
            and st["max_degree"] <= K_SMALL_SETUP_MAX_PT_OBS)


def host_counts(st):
    """plan_setup's host_counts: at most 65536 observations and an input blob
    (uv | cam | pt | point counts, 256-B aligned pieces) within the 1-MB stage."""
    al = lambda n: (n + 255) & ~255
    N, P = st["n_obs"], st["n_pts"]
    return N <= K_HOST_CHECK_MAX_OBS and al(16 * N) + 2 * al(4 * N) + al(4 * (P + 1)) <= K_STAGE_MAX_BYTES


def seq_of(trace):
    return "".join("I" if not it["step_is_valid"] else ("A" if it["step_is_successful"] else "R") for it in trace[1:])
