"""The point creation of one keyframe pair through the calls that
sfm_matcher_pair_points fuses: sfm_matcher_match_keyframes, then
sfm_triangulate_points, then the CPU restatement map_points_ref.filter_matches.
The reference of the GPU tests of sfm_matcher_pair_points and
sfm_matcher_pair_points_first; it shares no host path and no kernel tail with
them."""
import numpy as np

import map_points_ref as ref
from sfm_amd.mapping import triangulate_points


def composed(matcher, slot0, pts0, idx0, slot1, pts1, idx1, K, R0, t0, R1, t1, max_err):
    """-> (pi, ci, X, keep): the matches of rows idx0 of slot0 (positions
    pts0, all rows) with rows idx1 of slot1, subset-local; their points; the
    filter's flags."""
    idx0, idx1 = np.asarray(idx0, np.int32), np.asarray(idx1, np.int32)
    pi, ci = matcher.match_keyframes(slot0, idx0, slot1, idx1)
    uv0, uv1 = pts0[idx0[pi]], pts1[idx1[ci]]
    P = np.stack([ref.compose_P(K, R0, t0), ref.compose_P(K, R1, t1)])
    X = triangulate_points(np.zeros(len(pi), np.int32), np.ones(len(pi), np.int32), uv0, uv1, P)
    keep = ref.filter_matches(uv0, uv1, X, K, R0, t0, K, R1, t1, max_err)
    return pi, ci, X, keep
