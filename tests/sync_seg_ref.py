"""The frame synchronizer's average over frames, c_f = al c_(f-1) + om m_f per position with the arg max of every frame, three times over (NumPy only, no oracle,
no GPU): in float64 (the truth), as the single walk in float32 scalars in the reference's order (the yardstick: what the reference's own arithmetic is off by), and as
the segmented form of k_sync.hip does it in float32 -- {A, B} per sub-segment of 64 frames, a segment's start value the carried average folded through the sub-segments
in front of it, only the last segment's end carried on -- with a `mistake` argument that plants one wrong step at a time (tests/test_sync_seg_ref.py shows the bars of
tests/test_sync_seg_gpu.py reject every one of them).

Positions >= end_vec are not averaged (al = 0, om = 1: c = m).  alpha is the float32 the device holds; om = 1 - alpha is exact in float32 for alpha in [0.5, 1).

The input builder makes the result observable through the only things that leave the device, each frame's maximum and its index: cor_SOF = 0 and cor_PLSC = (v, 0)
give m = max(|p + s|, |s - p|) = |v|, and every v has at most 12 significant bits (background 1 + k / 2048, the bump a power of two), so v^2 and its root are exact."""
import numpy as np

SUB = 64                  # frames per sub-segment (SYNC_SUB)
CHUNK = 96                # frames between two barriers of the thirteen-wave kernel
BUMP = {0.9: 128.0, 0.99: 2048.0, 0.999: 32768.0}      # per alpha: large enough that the float64 winner of every frame is unambiguous
MISTAKES = ("a63", "no_cv", "skip_sub", "swap_sub", "seam_twice", "seam_dropped", "tail_averaged", "cv_writer", "keys_offset")


def coefficients(n, alpha, end_vec, dtype):
    """(al, om) per position: (alpha, 1 - alpha) in front of end_vec, (0, 1) from there on"""
    a = np.float32(alpha)
    avg = np.arange(n) < end_vec
    return np.where(avg, a, np.float32(0)).astype(dtype), np.where(avg, np.float32(1) - a, np.float32(1)).astype(dtype)


def average_fp64(m, cv, alpha, end_vec):
    """-> (max[F], first index of it[F], (max - second largest) / max [F], the final average[n]), all in float64"""
    F, n = m.shape
    al, om = coefficients(n, alpha, end_vec, np.float64)
    c = np.asarray(cv, np.float64).copy()
    mx, idx, margin = np.empty(F), np.empty(F, np.int64), np.empty(F)
    for f in range(F):
        c = al * c + om * m[f]
        top = np.partition(c, n - 2)[n - 2:]
        mx[f], idx[f], margin[f] = top[1], int(np.argmax(c)), (top[1] - top[0]) / top[1]
    return mx, idx, margin, c


def average_walk_fp32(m, cv, alpha, end_vec):
    """the single walk: each product and the sum rounded once to float32, frame after frame -> (max[F] float32, first index[F], the final average[n] float32)"""
    F, n = m.shape
    al, om = coefficients(n, alpha, end_vec, np.float32)
    c = np.asarray(cv, np.float32).copy()
    mx, idx = np.empty(F, np.float32), np.empty(F, np.int64)
    for f in range(F):
        c = al * c + om * m[f]
        idx[f] = int(np.argmax(c))
        mx[f] = c[idx[f]]
    return mx, idx, c


def average_segments_fp32(m, cv, alpha, end_vec, nseg, seg_F, mistake=None):
    """the segmented form as sync_seg_partial_kernel and sync_metric_argmax_kernel<96> compute it -> (max[F] float32, first index[F], the carried average[n] float32).
    mistake: None, or one of MISTAKES --
      a63            A of a sub-segment with 63 factors instead of 64
      no_cv          a segment behind the first starts its fold from 0 instead of the carried average
      skip_sub       the fold leaves out the last sub-segment in front of the segment
      swap_sub       the fold takes the last two sub-segments in the wrong order
      seam_twice     a segment behind the first reads its frames one frame early: the frame in front of the seam is counted twice
      seam_dropped   ... one frame late: the first frame behind the seam is dropped
      tail_averaged  positions >= end_vec averaged like the rest
      cv_writer      the first segment's end, not the last one's, becomes the carried average
      keys_offset    a segment behind the first writes its frames' results one chunk of 96 frames early (the call's last chunk is never written: 0, index 0)"""
    assert mistake is None or mistake in MISTAKES
    F, n = m.shape
    al, om = coefficients(n, alpha, n if mistake == "tail_averaged" else end_vec, np.float32)
    cv = np.asarray(cv, np.float32)
    if nseg == 1:
        seg_F = F
    assert nseg == 1 or (seg_F % SUB == 0 and seg_F % CHUNK == 0 and (nseg - 1) * seg_F < F <= nseg * seg_F)
    per = seg_F // SUB
    A, B = [], []
    for k in range((nseg - 1) * per):
        a, b = np.ones(n, np.float32), np.zeros(n, np.float32)
        for f in range(k * SUB, (k + 1) * SUB):
            b = al * b + om * m[f]
            if not (mistake == "a63" and f == k * SUB):
                a = a * al
        A.append(a); B.append(b)
    mx, idx = np.zeros(F, np.float32), np.zeros(F, np.int64)
    carried = None
    for s in range(nseg):
        f_base = s * seg_F
        c = np.zeros(n, np.float32) if (mistake == "no_cv" and s > 0) else cv.copy()
        order = list(range(s * per))
        if s > 0 and mistake == "skip_sub":
            order = order[:-1]
        if s > 0 and mistake == "swap_sub":
            order[-2:] = order[-2:][::-1]
        for j in order:
            c = A[j] * c + B[j]
        shift = {"seam_twice": -1, "seam_dropped": 1}.get(mistake, 0) if s > 0 else 0
        out = f_base - (CHUNK if (mistake == "keys_offset" and s > 0) else 0)
        for t in range(min(seg_F, F - f_base)):
            c = al * c + om * m[min(f_base + t + shift, F - 1)]
            i = int(np.argmax(c))
            mx[out + t], idx[out + t] = c[i], i
        if s == (0 if mistake == "cv_writer" else nseg - 1):
            carried = c
    return mx, idx, carried


def special_positions(n, end_vec):
    """where the bump of the eight frames behind a seam sits: the first and last lane of the first workgroup, the first of the second, the last averaged position, the
    first that is not averaged, the last position, the first position of the last (partial) workgroup of 64, one in mid-frame"""
    return [0, 63, 64, end_vec - 1, end_vec, n - 1, (n - 1) // 64 * 64, n // 2 + 7]


def build_metric(n, F, end_vec, alpha, seams, call, seed=2024):
    """-> (v[F, n] float32, position of every frame's bump[F], the bump): |v| is the metric m of call number `call` (0, 1, ..) of F frames.  Background 1 + k / 2048 with
    a random sign, one bump per frame on a position that walks over the frame (stride 977 mod n, running on from call to call); the eight frames from each frame in
    `seams` on get the bump at special_positions(n, end_vec)."""
    rng = np.random.default_rng(seed + 7919 * call)
    v = (1.0 + rng.integers(0, 2048, size=(F, n)) / 2048.0).astype(np.float32)
    v *= rng.choice(np.float32([-1.0, 1.0]), size=(F, n))
    pos = (977 * (call * F + np.arange(F, dtype=np.int64))) % n
    for s in seams:
        for q, p in enumerate(special_positions(n, end_vec)):
            if 0 <= s + q < F:
                pos[s + q] = p
    bump = np.float32(BUMP[round(float(alpha), 6)])
    v[np.arange(F), pos] = bump
    return v, pos, bump


def correlations(v):
    """-> (cor_SOF, cor_PLSC) float32 [F, 2 n], interleaved re / im: cor_SOF = 0, cor_PLSC = (v, 0)"""
    F, n = v.shape
    cp = np.zeros((F, 2 * n), np.float32)
    cp[:, 0::2] = v
    return np.zeros((F, 2 * n), np.float32), cp


def rel_err(mx, mx64):
    """largest |mx - mx64| / mx64 over the frames"""
    return float(np.max(np.abs(np.asarray(mx, np.float64) - mx64) / mx64))
