"""The receiver's waiting and learning phases (the reference's src/mains/RX/main_sched.cpp:407-635) above the C ABI: one function that drives a `Dvbs2Hip`
handle -- or anything with the same methods -- over a sample source until the coarse frequency, the symbol timing and the frame start are acquired.

  waiting     PLL coefficients (1, damping, nbw_wait); front gain stage -> step_mf (coarse rotation + matched filter + Gardner step + PLL, one fused task) -> extract ->
              gain stage -> frame synchronizer, the synchronizer's delay fed back to step_mf's DEL by one call (the reference's Feedbacker), until the frame
              synchronizer raises its packet flag (main_sched.cpp:472-494); then step_mf, the frame synchronizer and the timing synchronizer are reset (:500-502)
  learning 1  the same sequence for `learn1` frames at nbw1                                                                       (:527-560)
  learning 2  `learn2` more at nbw2
  learning 3  the PLL frozen: front gain stage -> coarse frequency SHIFT -> matched filter -> timing synchronize -> extract -> gain stage -> frame synchronizer ->
              PL descrambler -> L&R -> pilot-aided fine synchronizer, for `learn3` frames                                            (:562-630)

The handle is left where the transmission phase starts: every task's state carries on.  Defaults are the reference's: 150 / 150 / 200 frames, 1e-4 / 1e-4 / 5e-5."""
from __future__ import annotations

import numpy as np

from .iqfile import ProcessingAborted
from .rx_sequence import RxSequence


def acquire(rx, receive, n_frames=1, osf=2, learn1=150, learn2=150, learn3=200, nbw_wait=1e-4, nbw1=1e-4, nbw2=5e-5, damping=0.5 ** 0.5, wait_max=2000, agc=True,
            on_frames=None, smf_kernel=None):
    """rx: the handle; receive(): the next n_frames frames of pl_frame * osf complex samples (float32, interleaved), raising ProcessingAborted at the end of the source.
    on_frames(phase, n): called after every call of a phase with the frames it took (progress).
    smf_kernel: "LANE" or "WAVE", the form of the coarse-frequency loop (rx.sync_step_mf_set_kernel: the same results, WAVE the faster with one stream); None leaves the
    handle as it is and calls nothing.
    -> dict(acquired: the packet flag came within wait_max frames, and the source lasted through the learning phases; flag: the packet flag came;
            frames: {"waiting", "learning1", "learning2", "learning3"} frames spent; freq: estimated_freq per stream; nu: the floored frequency in use per stream)"""
    F = n_frames
    spent = dict(waiting=0, learning1=0, learning2=0, learning3=0)
    res = dict(acquired=False, flag=False, frames=spent, freq=None, nu=None)
    if smf_kernel is not None:
        rx.sync_step_mf_set_kernel(smf_kernel)
    fed_back = np.zeros(F, np.int32)                                  # Feedbacker: what memorize took at the last call, produce gives at this one (zeros at first)

    # the gain stages and the frame synchronizer of every phase, and learning phase 3, are the transmission phase's (rx_sequence.py)
    seq = RxSequence(rx, F, osf, agc=agc, coarse=True, timing="FAST", fine=True, lr=True)

    def wl12_call():
        """one run of the waiting / learning 1-2 sequence -> the packet flag after it (None: the sequence was cut short by an underflow)"""
        nonlocal fed_back
        x = seq.front(receive())
        _, _, _, y, b = rx.sync_step_mf_synchronize(fed_back, x)
        y2, _, rdy = rx.sync_timing_extract(y, b)
        if not rdy[0]:
            return None                                               # (the reference's sequence aborts here; the Feedbacker keeps what it had)
        delay, flags, _, _ = seq.align(y2)
        fed_back = np.array(delay, np.int32)
        return bool(flags[-1])

    try:
        # ---------------------------------------------------------- waiting
        rx.sync_coarse_set_pll(1, damping, nbw_wait)
        while not res["flag"]:
            if spent["waiting"] >= wait_max:
                return _finish(rx, res)
            flag = wl12_call()
            spent["waiting"] += F
            if on_frames:
                on_frames("waiting", F)
            res["flag"] = bool(flag)
        rx.sync_step_mf_reset()
        rx.sync_frame_reset()
        rx.sync_timing_reset()
        # ---------------------------------------------------------- learning 1 and 2
        rx.sync_coarse_set_pll(1, damping, nbw1)
        m, limit, second = 0, learn1, False
        while m < limit:
            wl12_call()
            m += F
            spent["learning2" if second else "learning1"] += F
            if on_frames:
                on_frames("learning2" if second else "learning1", F)
            if not second and m >= learn1:
                second, limit = True, m + learn2
                rx.sync_coarse_set_pll(1, damping, nbw2)
        # ---------------------------------------------------------- learning 3
        m = 0
        while m < learn3:
            sym = seq.symbols(seq.front(receive()))
            m += F
            spent["learning3"] += F
            if on_frames:
                on_frames("learning3", F)
            if sym is not None:
                seq.fine_sync(seq.align(sym)[3])
        res["acquired"] = True
    except ProcessingAborted:
        pass
    return _finish(rx, res)


def _finish(rx, res):
    est, nu = rx.sync_coarse_get_freq()
    res["freq"], res["nu"] = [float(v) for v in est], [float(v) for v in nu]
    return res
