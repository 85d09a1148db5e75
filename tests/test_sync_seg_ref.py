"""The bars that tests/test_sync_seg_gpu.py holds the segmented average over frames to, tried on the CPU: the float32 model of the segmented form as the kernels do it
(tests/sync_seg_ref.py) passes them, and the same model with one wrong step planted -- each of the mistakes the segmented form invites -- misses at least one of them
at one alpha at least.  32APSK-S (n = 3402 positions, vec_width 8: 3400 averaged), a call of F = 1632 frames = a segment of 960 and one of 672 (6 whole chunks of 96 and
96 frames more), two calls with the carried average, alpha 0.9, 0.99 and 0.999.

The bars, per frame: the index of the maximum is the float64 one; the maximum is within 4 x the single float32 walk's own largest error of the float64 one; where the
bump sits on a position that is not averaged the maximum IS the bump; against the single walk, bit for bit equal over the first segment of the first call and within
2 x that bar behind the first seam."""
import functools

import numpy as np
import pytest

import sync_seg_ref as R

N, VEC, F, NSEG, SEG_F, CALLS = 3402, 8, 1632, 2, 960, 2
END_VEC = N // VEC * VEC
ALPHAS = (0.9, 0.99, 0.999)
SEAMS = [k * SEG_F for k in range(NSEG)]


def run(form, alpha, ms, **kw):
    """the CALLS calls through one form with the average carried -> per call (max, index), the average at the end"""
    cv, out = np.zeros(N, np.float32 if form is not R.average_fp64 else np.float64), []
    for m in ms:
        r = form(m, cv, alpha, END_VEC, **kw)
        out.append(r[:-1])
        cv = r[-1]
    return out, cv


@functools.lru_cache(maxsize=None)
def world_of(alpha):
    built = [R.build_metric(N, F, END_VEC, alpha, SEAMS, call) for call in range(CALLS)]
    ms = [np.abs(b[0]) for b in built]
    w = dict(alpha=alpha, ms=ms, pos=[b[1] for b in built], bump=built[0][2])
    w["f64"], _ = run(R.average_fp64, alpha, ms)
    w["walk"], w["walk_cv"] = run(R.average_walk_fp32, alpha, ms)
    w["E"] = max(R.rel_err(w["walk"][c][0], w["f64"][c][0]) for c in range(CALLS))
    for a, b in zip(w["walk"], w["f64"]):
        assert np.array_equal(a[1], b[1])                       # the yardstick itself finds every float64 winner
    return w


@pytest.fixture(params=ALPHAS)
def world(request):
    return world_of(request.param)


def misses(w, got):
    """the bars a form's per-call (max, index) misses -> {bar: by how much}"""
    bad = {}
    for c in range(CALLS):
        mx, idx = got[c]
        mx64, idx64, _ = w["f64"][c]
        wrong = int(np.sum(idx != idx64))
        if wrong:
            bad["index c%d" % c] = "%d frames" % wrong
        e = R.rel_err(mx, mx64)
        if e > 4 * w["E"]:
            bad["fp64 c%d" % c] = "%.3g = %.1f x the walk's %.3g" % (e, e / w["E"], w["E"])
        tail = w["pos"][c] >= END_VEC
        if not np.array_equal(mx[tail], np.full(int(tail.sum()), w["bump"], np.float32)):
            bad["tail c%d" % c] = "not the bump"
        wmx = w["walk"][c][0]
        if c == 0 and not np.array_equal(mx[:SEG_F].view(np.uint32), wmx[:SEG_F].view(np.uint32)):
            bad["first segment"] = "not the walk's bits"
        d = float(np.max(np.abs(mx.astype(np.float64) - wmx) / mx64))
        if d > 2 * 4 * w["E"]:
            bad["walk c%d" % c] = "%.3g = %.1f x the walk's %.3g" % (d, d / w["E"], w["E"])
    return bad


def test_the_inputs_are_exact_and_their_winners_unambiguous(world):
    """|v| has at most 12 significant bits (so v^2 is exact in float32 and its root is |v|), every frame's float64 winner is clear of the runner-up by far more than
    the float32 walk is off, and the frames behind each seam put the bump on the edge positions"""
    w = world
    for c in range(CALLS):
        m = w["ms"][c]
        assert np.array_equal(np.round(m.astype(np.float64) * 2048) / 2048, m) and m.max() == w["bump"] and m.min() >= 1.0
        assert np.array_equal(np.sqrt(m * m), m)
        margin = w["f64"][c][2]
        print("inputs alpha %g call %d: smallest margin %.3g, walk error %.3g" % (w["alpha"], c, margin.min(), w["E"]))
        assert margin.min() > 50 * w["E"]
        for s in SEAMS:
            assert list(w["pos"][c][s:s + 8]) == R.special_positions(N, END_VEC)
    assert R.special_positions(N, END_VEC)[3:7] == [3399, 3400, 3401, 3392]


def test_one_segment_is_the_walk(world):
    w = world
    got, cv = run(R.average_segments_fp32, w["alpha"], w["ms"], nseg=1, seg_F=F)
    for a, b in zip(got, w["walk"]):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert np.array_equal(cv, w["walk_cv"])


def test_the_segment_model_passes_every_bar(world):
    w = world
    got, cv = run(R.average_segments_fp32, w["alpha"], w["ms"], nseg=NSEG, seg_F=SEG_F)
    e = max(R.rel_err(got[c][0], w["f64"][c][0]) for c in range(CALLS))
    d = max(float(np.max(np.abs(got[c][0].astype(np.float64) - w["walk"][c][0]) / w["f64"][c][0])) for c in range(CALLS))
    print("model alpha %g: error %.3g = %.2f x the walk's %.3g; against the walk %.3g = %.2f x" % (w["alpha"], e, e / w["E"], w["E"], d, d / w["E"]))
    assert misses(w, got) == {}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_mistake_misses_a_bar(mistake):
    caught = 0
    for alpha in ALPHAS:
        w = world_of(alpha)
        got, _ = run(R.average_segments_fp32, alpha, w["ms"], nseg=NSEG, seg_F=SEG_F, mistake=mistake)
        bad = misses(w, got)
        print("mistake %-13s alpha %-5g: %s" % (mistake, alpha, "; ".join("%s %s" % kv for kv in sorted(bad.items())) or "passes every bar"))
        caught += bool(bad)
    assert caught >= 1, mistake
