"""The frame synchronizer's average over frames IN SEGMENTS (k_sync.hip: sync_seg_partial_kernel + sync_metric_argmax_kernel<96> with more than one grid row, what every
short-frame call of 1536 frames or more runs) held to float64, to the oracle and to the single walk.

(a) a synthetic metric through the two-task form (tests/sync_seg_ref.py: cor_SOF = 0, cor_PLSC = (v, 0), so m = |v| exactly; one bump per frame that walks over the
    positions, on the edge positions in the frames behind every seam), two calls on one handle: DEL / FLG / Y equal to the oracle's, the delay the one of the float64 first
    maximum, TRI within 4 x the float32 single walk's own largest error of the float64 maximum (the margin tests/test_fine_sync_fp64_gpu.py gives a reordered fp32 sum over
    the reference's own error), TRI the bump itself where the bump sits on a position that is not averaged;
(b) the same calls on a fresh handle with DVBS2HIP_SYNC_SEGMENTS=1 (the single walk; the switch is read at each call): DEL / FLG / Y equal, TRI bit for bit equal
    over the first segment of the first call, within 2 x the bar of (a) anywhere else (each side is entitled to that bar against float64);
(c) the one-task form on a real stream, one call of 1632 frames against calls of 1536 + 96, the oracle and the single walk;
(d) the located form against the delayed copy on that stream.
Every case asks `plan_probe sync` (the library's sync_choose, dvbs2_amd/csrc/rx_dispatch.h, under this process's knobs) which arg-max form its call takes and what it is
cut into, and requires the thirteen-wave form in two segments at least; the single walk's calls have to come back as one segment.  tests/test_sync_seg_ref.py shows
on the CPU that these bars reject each mistake the segmented form invites.  Measured figures: results/sync_segments/README.md."""
import hashlib
import os

import numpy as np
import pytest

import sync_seg_ref as R

pytestmark = pytest.mark.gpu
TOL = 2e-4                # the metric's bar against the oracle on a real stream (tests/test_sync_gpu.py)
CALLS = 2
# (MODCOD, frames per call, alpha, vec_width)
CASES = [("32APSK-S_3/4", 1536, 0.9, 8),         # 2 whole segments of 8 chunks
         ("32APSK-S_3/4", 1632, 0.9, 8),         # 2, the last one partial: 6 chunks + 96 frames
         ("32APSK-S_3/4", 1632, 0.99, 8),
         ("32APSK-S_3/4", 1632, 0.999, 8),
         ("32APSK-S_3/4", 3072, 0.99, 16),       # 4 segments, 36 folds in front of the last
         ("16APSK-S_8/9", 2400, 0.9, 8),         # 3: 960 + 960 + 480
         ("8PSK-S_3/5", 1537, 0.9, 8)]           # 2, the last one 577 frames: 6 chunks + 1 frame
STREAM = ("32APSK-S_3/4", 1632, 1501)            # (c), (d): MODCOD, frames, offset of the stream


def digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).view(np.uint8), digest_size=16).hexdigest()


def metric_of(n, F, alpha, vec_width, seg_F, call):
    """-> (v, position of each frame's bump, the bump) of one call: tests/sync_seg_ref.py build_metric with a seam every seg_F frames"""
    return R.build_metric(n, F, n // vec_width * vec_width, alpha, range(0, F, seg_F), call)


def x_of(n, F, call):
    """the samples the delay line moves: any will do, the metric does not come from them in the two-task form"""
    return np.random.default_rng(100 + call).standard_normal((F, 2 * n), dtype=np.float32)


def trigger_of(alpha):
    return R.BUMP[alpha] / 2        # far from every TRI: above what an averaged position reaches ((1 - alpha) bump + 2), below the bump itself


def device_synthetic(case, seg_F):
    """the CALLS calls of a case on one handle (the two-task form) -> per call {DEL, FLG, TRI, Y, its digest, metric, flag, and the inputs' v, pos, bump}"""
    from dvbs2_amd.receiver import Dvbs2Hip
    modcod, F, alpha, vec_width = case
    rx = Dvbs2Hip(modcod, max_frames=F)
    rx.sync_frame_set_params(alpha, trigger_of(alpha), vec_width)
    out = []
    for call in range(CALLS):
        v, pos, bump = metric_of(rx.pl_frame, F, alpha, vec_width, seg_F, call)
        cs, cp = R.correlations(v)
        DEL, FLG, TRI, Y = rx.sync_frame_synchronize2(x_of(rx.pl_frame, F, call), cs, cp, with_flags=True)
        m, flag = rx.sync_frame_metric()
        out.append(dict(DEL=DEL, FLG=FLG, TRI=TRI, Y=Y, Yd=digest(Y), metric=np.float32(m), flag=bool(flag), v=v, pos=pos, bump=bump))
    rx.close()
    return out


def device_stream(modcod, x, cuts):
    """the one-task form over the stream x cut into calls -> DEL, FLG, TRI, Y of the whole stream"""
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip(modcod, max_frames=x.shape[0])
    parts = [rx.sync_frame_synchronize(x[a:b], with_flags=True) for a, b in cuts]
    rx.close()
    return [np.concatenate([p[k] for p in parts]) for k in range(4)]


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """(n, F) -> (nseg, seg_F) of a one-stream call as the library's sync_choose cuts it under the knobs this process has at that moment; the form is the thirteen-wave one"""
    from test_plan_digest import build_probe
    from test_rx_dispatch import SYNC, ask
    assert "DVBS2HIP_SYNC_SEGMENTS" not in os.environ and "DVBS2HIP_SYNC_ARGMAX4" not in os.environ, "this process has to run the default form"
    exe = str(tmp_path_factory.mktemp("sync_seg_gpu") / "plan_probe")
    build_probe(exe)

    def plan(n, F):
        m = SYNC.match(ask(exe, "sync", [(n, F, 1, 16, 1, 1, 1, 0)], inherit=True)[0])
        assert m[5] == "sync_metric_argmax_kernel<96>", m[0]
        return int(m[7]), int(m[8])
    return plan


@pytest.fixture(scope="module", params=range(len(CASES)), ids=["%s-F%d-a%g-v%d" % c for c in CASES])
def case(request, plan_of, P):
    """one case, run once on the device for (a) and (b): what the device gave for the CALLS calls, and over the same metric the float64 average and the float32 single
    walk (per call max64, index64, margin, the walk's max) with E = the walk's largest relative error"""
    k = request.param
    modcod, F, alpha, vec_width = CASES[k]
    n = P.get_modcod(modcod).pl_frame
    nseg, seg_F = plan_of(n, F)
    assert nseg >= 2, (CASES[k], nseg, seg_F)
    got = device_synthetic(CASES[k], seg_F)
    end_vec = n // vec_width * vec_width
    c64, c32, ref = np.zeros(n), np.zeros(n, np.float32), []
    for call in range(CALLS):
        m = np.abs(got[call]["v"])
        mx64, idx64, margin, c64 = R.average_fp64(m, c64, alpha, end_vec)
        mx32, idx32, c32 = R.average_walk_fp32(m, c32, alpha, end_vec)
        assert np.array_equal(idx32, idx64)
        ref.append((mx64, idx64, margin, mx32))
    return dict(k=k, n=n, nseg=nseg, seg_F=seg_F, end_vec=end_vec, got=got, ref=ref, E=max(R.rel_err(r[3], r[0]) for r in ref))


def test_synthetic_metric_in_segments_against_fp64_and_the_oracle(O, case):
    modcod, F, alpha, vec_width = CASES[case["k"]]
    n, nseg, seg_F, got, ref, E, end_vec = (case[q] for q in ("n", "nseg", "seg_F", "got", "ref", "E", "end_vec"))
    sf = O.SyncFrame(n, alpha=alpha, trigger=trigger_of(alpha), vec_width=vec_width)
    for call in range(CALLS):
        g = got[call]
        X, (cs, cp), pos, bump = x_of(n, F, call), R.correlations(g["v"]), g["pos"], g["bump"]
        mx64, idx64, margin, mx32 = ref[call]
        e = R.rel_err(g["TRI"], mx64)
        print("sync_seg (a) %s F %d alpha %g vec %d nseg %d seg_F %d call %d: walk error %.3g device error %.3g ratio %.2f smallest margin %.3g"
              % (modcod, F, alpha, vec_width, nseg, seg_F, call, E, e, e / E, margin.min()))
        assert margin.min() > 50 * E and np.min(np.abs(mx64 - trigger_of(alpha))) > 0.25 * trigger_of(alpha)        # the inputs decide every index and flag
        assert np.array_equal(g["DEL"], (n + idx64 - 25 - 64) % n)
        for f in range(F):
            do, Yo = sf.synchronize2(X[f], cs[f], cp[f])
            assert g["DEL"][f] == do and bool(g["FLG"][f]) == sf.packet_flag, (call, f, g["DEL"][f], do)
            assert np.array_equal(g["Y"][f], Yo), (call, f)
        moves = int(np.sum(idx64[1:] != idx64[:-1]))
        print("sync_seg (a) ... the delay moves in %d of %d frames, %d flags up" % (moves, F, int(g["FLG"].sum())))
        assert moves > 100 and 0 < g["FLG"].sum() < F                   # the delay line's transitional branches run over and over (at alpha = 0.999 an old bump often stays the winner); both flags occur
        assert e <= 4 * E, (call, e, E)
        tail = pos >= end_vec
        assert tail.sum() >= nseg and np.array_equal(g["TRI"][tail].view(np.uint32), np.full(int(tail.sum()), bump, np.float32).view(np.uint32)), call
        assert g["metric"].view(np.uint32) == g["TRI"][-1].view(np.uint32) and g["flag"] == bool(g["FLG"][-1])


def test_synthetic_metric_in_segments_against_the_single_walk(case, plan_of, monkeypatch):
    k, n, seg_F, got, ref, E = (case[q] for q in ("k", "n", "seg_F", "got", "ref", "E"))
    monkeypatch.setenv("DVBS2HIP_SYNC_SEGMENTS", "1")
    assert plan_of(n, CASES[k][1]) == (1, CASES[k][1])
    walk = device_synthetic(CASES[k], seg_F)                        # a fresh handle, the same inputs
    monkeypatch.delenv("DVBS2HIP_SYNC_SEGMENTS")
    for call in range(CALLS):
        g, o, mx64 = got[call], walk[call], ref[call][0]
        assert np.array_equal(o["DEL"], g["DEL"]) and np.array_equal(o["FLG"], g["FLG"]) and o["Yd"] == g["Yd"] and np.array_equal(o["Y"], g["Y"]), call
        a, b = g["TRI"], o["TRI"]
        if call == 0:
            assert np.array_equal(a[:seg_F].view(np.uint32), b[:seg_F].view(np.uint32))
        d = float(np.max(np.abs(a.astype(np.float64) - b) / mx64))
        ulp = int(np.max(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32))))
        print("sync_seg (b) %s F %d alpha %g call %d: against the single walk %.3g = %.2f x the walk's error %.3g, at most %d ulp, %d of %d frames differ"
              % (CASES[k][0], CASES[k][1], CASES[k][2], call, d, d / E, E, ulp, int(np.sum(a.view(np.uint32) != b.view(np.uint32))), len(a)))
        assert d <= 2 * 4 * E, (call, d, E)


@pytest.fixture(scope="module")
def stream(O, plan_of):
    """(c), (d): 7 PL frames tiled from offset 1501 on (as test_average_and_arg_max_over_many_short_frames of tests/test_sync_gpu.py builds it), how the library cuts
    its calls, and what the one-task form gave for the stream as one call"""
    from helpers import make_pl_frames
    modcod, F, off = STREAM
    _, pl, _, _ = make_pl_frames(O, modcod, 7, 9.0, seed=31)
    n = pl.shape[1] // 2
    x = np.concatenate([np.zeros(2 * off, np.float32), np.tile(pl.reshape(-1), F // 7 + 2)])[:F * 2 * n].reshape(F, 2 * n)
    nseg, seg_F = plan_of(n, F)
    assert nseg >= 2 and plan_of(n, 1536)[0] >= 2 and plan_of(n, 96)[0] == 1
    return dict(x=x, n=n, seg_F=seg_F, seg_F_cut=plan_of(n, 1536)[1], one=device_stream(modcod, x, [(0, F)]))


def stream_twin(O, x, n):
    """the oracle over the stream -> (delay, flag, metric, Y) per frame and, from its two correlations, (max64, the walk's largest relative error) of the average"""
    F = x.shape[0]
    sf = O.SyncFrame(n, alpha=0.9, trigger=30.0, vec_width=8)
    d, flg, met, Ys, m = np.empty(F, np.int32), np.empty(F, bool), np.empty(F, np.float32), [], np.empty((F, n), np.float32)
    held = np.zeros(64, complex)                                    # cor_SOF meets cor_PLSC 64 samples late
    for f in range(F):
        cs, cp = sf.synchronize1(x[f])
        d[f], Y = sf.synchronize2(x[f], cs, cp)
        flg[f], met[f] = sf.packet_flag, sf.metric
        Ys.append(Y)
        s = np.concatenate([held, cs[0::2].astype(np.float64) + 1j * cs[1::2]])
        held, s, p = s[n:], s[:n], cp[0::2].astype(np.float64) + 1j * cp[1::2]
        m[f] = np.maximum(np.abs(p + s), np.abs(s - p))
    end_vec = n // 8 * 8
    mx64 = R.average_fp64(m, np.zeros(n), 0.9, end_vec)[0]
    mx32 = R.average_walk_fp32(m, np.zeros(n, np.float32), 0.9, end_vec)[0]
    return d, flg, met, Ys, mx64, R.rel_err(mx32, mx64)


def test_one_task_form_on_a_real_stream_in_segments(O, stream, plan_of, monkeypatch):
    modcod, F, off = STREAM
    x, n, seg_F = stream["x"], stream["n"], stream["seg_F"]
    DEL, FLG, TRI, Y = stream["one"]
    d, flg, met, Ys, mx64, E = stream_twin(O, x, n)
    for f in range(F):
        assert DEL[f] == d[f] and np.array_equal(Y[f], Ys[f]), f
        assert abs(TRI[f] - met[f]) <= TOL * max(1.0, met[f]) and bool(FLG[f]) == flg[f], f
    assert DEL[-1] == off and FLG[-1] == 1
    # the same stream as calls of 1536 + 96 frames: segments of 768 + 768, then a single walk from the carried average
    cut = stream["seg_F_cut"]
    DEL2, FLG2, TRI2, Y2 = device_stream(modcod, x, [(0, 1536), (1536, F)])
    assert np.array_equal(DEL2, DEL) and np.array_equal(Y2, Y) and np.array_equal(FLG2, FLG)
    same = min(cut, seg_F)                                          # both cuts walk from the reset average up to their first seam
    assert np.array_equal(TRI2[:same].view(np.uint32), TRI[:same].view(np.uint32))
    d2 = float(np.max(np.abs(TRI2.astype(np.float64) - TRI) / mx64))
    # the single walk on a fresh handle
    monkeypatch.setenv("DVBS2HIP_SYNC_SEGMENTS", "1")
    assert plan_of(n, F) == (1, F)
    o = dict(zip(("DEL", "FLG", "TRI", "Y"), device_stream(modcod, x, [(0, F)])))
    monkeypatch.delenv("DVBS2HIP_SYNC_SEGMENTS")
    assert np.array_equal(o["DEL"], DEL) and np.array_equal(o["FLG"], FLG) and np.array_equal(o["Y"], Y)
    assert np.array_equal(o["TRI"][:seg_F].view(np.uint32), TRI[:seg_F].view(np.uint32))
    d1 = float(np.max(np.abs(o["TRI"].astype(np.float64) - TRI) / mx64))
    print("sync_seg (c) %s F %d: walk error %.3g; one call against 1536 + 96: %.3g = %.2f x; against the single walk %.3g = %.2f x; device against the oracle's metric %.3g"
          % (modcod, F, E, d2, d2 / E, d1, d1 / E, float(np.max(np.abs(TRI - met) / np.maximum(1.0, met)))))
    assert d2 <= 2 * 4 * E and d1 <= 2 * 4 * E, (d2, d1, E)


def test_located_form_in_segments_equals_the_delayed_copy(stream):
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    modcod, F, _ = STREAM
    dev = torch.device("cuda")
    xd = torch.from_numpy(stream["x"]).to(dev)
    out = {}
    for form in ("copy", "located"):
        rx = Dvbs2Hip(modcod, max_frames=F)
        DEL = torch.empty(F, dtype=torch.int32, device=dev); FLG = torch.empty_like(DEL); TRI = torch.empty(F, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if form == "copy":
            Yd = torch.empty_like(xd)
            rx.sync_frame_synchronize_dev(xd.data_ptr(), DEL.data_ptr(), FLG.data_ptr(), TRI.data_ptr(), Yd.data_ptr(), F)
        else:
            SRC = torch.zeros(F, dtype=torch.int64, device=dev)
            rx.sync_frame_locate_dev(xd.data_ptr(), DEL.data_ptr(), FLG.data_ptr(), TRI.data_ptr(), SRC.data_ptr(), F)
        rx.synchronize()
        out[form] = (DEL.cpu().numpy(), FLG.cpu().numpy(), TRI.cpu().numpy())
        rx.close()
    for a, b in zip(out["copy"], out["located"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(out["copy"], stream["one"][:3]):                # and both are what the host form gave
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
