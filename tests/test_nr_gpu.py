"""kg_post's noise-reduction stage (rx/rx_sound.cpp:933-949: NR_WDSP -> rx/wdsp/ANR.cpp, NR_ORIG -> rx/kiwi/lms.cpp) on the GPU:
every unit scenario of tests/golden/nr_ref.npz (the reference's own commands and stage, tools/make_ref_nr_golden.py) BIT-EXACT
through kg_post_set_nr_* and kg_post_nr_process_dev, with the end states through kg_post_nr_state; the fused pass of
kg_post_process_dev equal to the same audio without NR followed by the standalone filters; mixed batches and changing channel
lists equal to each channel alone; NR-off channels byte-identical to a run that never touched NR; the state semantics of algo
switches, kg_post_reset and mode changes; argument errors."""
import os

import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post
from flydog_sdr_gps_amd._lib import KiwiGpuError
from tests import script_common

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS = 12000.0


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "nr_ref.npz"))


def digest(a):
    """as tests/golden/nr_ref.npz keeps the weight vectors: SHA-256 prefix with every NaN as 0x7FC00000"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).copy()
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return script_common.digest(u.tobytes())


def run_unit(P, ch, g, name):
    """Replays a unit scenario's script on channel ch of P through the standalone call site; asserts every block and end state."""
    x, want = g[name + "_in"], g[name + "_out"]
    algo, en, pos = 0, [0, 0], 0
    for line in (str(l) for l in g[name + "_script"]):
        f = line.split()
        if f[0] == "A":
            algo = int(f[1]); en = [0, 0]
            P.set_nr_algo(ch, algo)
        elif f[0] == "E":
            en[int(f[1])] = int(f[2])
            P.set_nr_enable(ch, int(f[1]), int(f[2]))
        elif f[0] == "P":
            P.set_nr_param(ch, int(f[1]), int(f[2]), np.float32(f[3]))
        elif f[0] == "C":
            algo, en = 0, [0, 0]
            P.reset(ch)
        elif f[0] == "B":
            n, stereo = int(f[1]), int(f[2])
            y = x[pos:pos + n][None, :].copy()
            if not stereo and algo in (post.NR_WDSP, post.NR_ORIG):
                for t in (post.NR_AUTONOTCH, post.NR_DENOISE):            # rx_sound.cpp:936-942: auto-notch first
                    if en[t]:
                        y = P.nr_process([ch], t, y)
            bad = np.flatnonzero(y[0] != want[pos:pos + n])
            assert bad.size == 0, (name, pos, bad.size, bad[:4])
            pos += n
        elif f[0] == "S":
            for t in range(2):
                st = P.nr_state([ch], t, weights=True)
                si, sf = g[name + "_state_i"][t], g[name + "_state_f"][t]
                assert list(st["anr_i"][0]) == list(si[:3]), (name, t)
                assert list(st["lms_i"][0]) == list(si[3:6]), (name, t)
                assert np.array_equal(st["anr_f"][0].view(np.uint32), sf.view(np.uint32)), (name, t)
                assert digest(st["anr_w"][0]) == bytes(g[name + "_w_sha"][t]), (name, t, "w[]")
                assert digest(st["lms_coef"][0]) == bytes(g[name + "_coef_sha"][t]), (name, t, "m_lmscoef[]")
    assert pos == x.size


def test_unit_scenarios_bit_exact(gpu_ctx, golden):
    for name in (str(n) for n in golden["names"]):
        P = Post(gpu_ctx, nchan=3)                         # fresh, zeroed filters (the reference's statics), on channel 2
        try:
            run_unit(P, 2, golden, name)
        finally:
            P.close()


def ssb_input(n, seed, amp=0.3):
    r = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = amp * (np.exp(2j * np.pi * 1000.0 * t) + 0.6 * np.exp(2j * np.pi * (300.0 + 50 * seed) * t)) + 0.08 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return x.astype(np.complex64)


def configure(P, ch, mode):
    P.set_agc(ch, True, False, -100, 50, 6, 1000, FS)
    P.set_smeter(ch, FS)
    P.set_am_passband(ch, -2700.0, 2700.0, FS)
    P.set_mode(ch, mode)
    P.reset(ch)
    P.squelch_setup(ch, FS)
    P.squelch_set(ch, 0, 0)


# channel -> (mode, algo, {type: params}, enables (denoise, auto-notch))
PLAN = {
    0: (post.MODE_SSB, post.NR_WDSP, {1: [64, 16, 1e-4, 0.1], 0: [64, 16, 1e-4, 0.1]}, (1, 1)),
    1: (post.MODE_AM, post.NR_ORIG, {1: [0, 0, 0], 0: [0, 0, 0]}, (1, 1)),
    2: (post.MODE_SSB, post.NR_OFF, {}, (0, 0)),
    3: (post.MODE_IQ, post.NR_WDSP, {0: [64, 16, 1e-4, 0.1]}, (1, 0)),        # stereo: NR is skipped
    4: (post.MODE_NBFM, post.NR_WDSP, {1: [128, 2, 2.048e-4, 0.2]}, (0, 1)),
    5: (post.MODE_SAM, post.NR_ORIG, {0: [20, 0.01, 0.97]}, (1, 0)),
    6: (post.MODE_SSB, post.NR_WDSP, {0: [128, 64, 1e-4, 0.1]}, (0, 0)),      # params, nothing enabled
    7: (post.MODE_SAS, post.NR_ORIG, {1: [0, 0, 0]}, (0, 1)),                 # stereo: NR is skipped
}


def set_nr(P, ch, algo, params, enables):
    P.set_nr_algo(ch, algo)
    for t, vals in params.items():
        for k, v in enumerate(vals):
            P.set_nr_param(ch, t, k, v)
    for t in (0, 1):
        if enables[t]:
            P.set_nr_enable(ch, t, enables[t])


def test_fused_pass_equals_post_then_standalone_filters(gpu_ctx):
    """kg_post_process_dev with NR on == the same channel without NR, then kg_post_nr_process_dev auto-notch, then denoise"""
    n = 512
    A, B = Post(gpu_ctx, nchan=8), Post(gpu_ctx, nchan=8)
    try:
        for ch, (mode, algo, params, en) in PLAN.items():
            for P in (A, B):
                configure(P, ch, mode)
                set_nr(P, ch, algo, params, en)
            B.set_nr_enable(ch, 0, 0); B.set_nr_enable(ch, 1, 0)         # B: the same filters, run by hand
        chans = list(PLAN)
        for blk in range(4):
            x = np.stack([ssb_input(n, 10 * blk + ch) for ch in chans])
            ya, _, agc_a = A.process(chans, x)
            yb, _, agc_b = B.process(chans, x)
            for i, ch in enumerate(chans):
                mode, algo, params, en = PLAN[ch]
                assert np.array_equal(agc_a[i].view(np.uint32), agc_b[i].view(np.uint32)), ch
                if mode in post.STEREO_MODES or algo == post.NR_OFF:
                    assert np.array_equal(ya[i], yb[i]), ch
                    continue
                want = yb[i][None, :]
                for t in (post.NR_AUTONOTCH, post.NR_DENOISE):
                    if en[t]:
                        want = B.nr_process([ch], t, want)
                assert np.array_equal(ya[i], want[0]), (ch, blk)
                if en[0] or en[1]:
                    assert not np.array_equal(ya[i], yb[i]), (ch, "NR changed nothing")
    finally:
        A.close(); B.close()


def test_mixed_batches_equal_each_channel_alone(gpu_ctx):
    n = 512
    chans = list(PLAN)
    M = Post(gpu_ctx, nchan=8)
    alone = {ch: Post(gpu_ctx, nchan=1) for ch in chans}
    try:
        for ch, (mode, algo, params, en) in PLAN.items():
            configure(M, ch, mode); set_nr(M, ch, algo, params, en)
            configure(alone[ch], 0, mode); set_nr(alone[ch], 0, algo, params, en)
        lists = [chans, [5, 0, 3], chans[::-1], [1, 4, 7, 2], chans]
        fed = {ch: 0 for ch in chans}
        for blk, lst in enumerate(lists):
            x = np.stack([ssb_input(n, 100 * blk + ch) for ch in lst])
            y, _, agc = M.process(lst, x)
            for i, ch in enumerate(lst):
                ya, _, agca = alone[ch].process([0], x[i][None, :])
                assert np.array_equal(y[i], ya[0]), (blk, ch)
                assert np.array_equal(agc[i].view(np.uint32), agca[0].view(np.uint32)), (blk, ch)
                fed[ch] += 1
        for ch, (mode, algo, params, en) in PLAN.items():
            if algo in (post.NR_WDSP, post.NR_ORIG):
                for t in (0, 1):
                    a = M.nr_state([ch], t, weights=True)
                    b = alone[ch].nr_state([0], t, weights=True)
                    for k in a:
                        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ch, t, k)
    finally:
        M.close()
        for P in alone.values():
            P.close()


def test_nr_off_channels_byte_identical_to_never_touched(gpu_ctx):
    n = 512
    chans = list(PLAN)
    A, B = Post(gpu_ctx, nchan=8), Post(gpu_ctx, nchan=8)        # A: NR as PLAN; B: no NR call at all
    try:
        for ch, (mode, algo, params, en) in PLAN.items():
            configure(A, ch, mode); configure(B, ch, mode)
            set_nr(A, ch, algo, params, en)
        for blk in range(3):
            x = np.stack([ssb_input(n, 7 * blk + ch) for ch in chans])
            ya, da, ga = A.process(chans, x)
            yb, db, gb = B.process(chans, x)
            for i, ch in enumerate(chans):
                mode, algo, params, en = PLAN[ch]
                if mode in post.STEREO_MODES or not (en[0] or en[1]) or algo == post.NR_OFF:
                    assert np.array_equal(ya[i], yb[i]), ch
                assert np.array_equal(da[i].view(np.uint32), db[i].view(np.uint32)), ch
                assert np.array_equal(ga[i].view(np.uint32), gb[i].view(np.uint32)), ch
    finally:
        A.close(); B.close()


def test_state_semantics(gpu_ctx):
    n = 512
    P = Post(gpu_ctx, nchan=2)
    try:
        configure(P, 0, post.MODE_SSB)
        set_nr(P, 0, post.NR_WDSP, {1: [64, 16, 1e-4, 0.1]}, (0, 1))
        x = ssb_input(n, 3)[None, :]
        P.process([0], x)
        s0 = P.nr_state([0], 1, weights=True)
        assert s0["anr_i"][0, 1] == 64 and s0["anr_i"][0, 0] == (0 - n) & 511
        # a mode change leaves NR alone
        P.set_mode(0, post.MODE_AM)
        s1 = P.nr_state([0], 1, weights=True)
        assert all(np.array_equal(s0[k], s1[k]) for k in s0)
        P.set_mode(0, post.MODE_SSB)
        # an algo switch keeps the WDSP state and clears the enables: the next block is NR-free and nothing advances
        P.set_nr_algo(0, post.NR_ORIG)
        y_orig, _, _ = P.process([0], x)
        assert all(np.array_equal(s0[k], P.nr_state([0], 1, weights=True)[k]) for k in s0)
        Q = Post(gpu_ctx, nchan=1)
        try:
            configure(Q, 0, post.MODE_SSB)
            Q.process([0], x)
            y_plain, _, _ = Q.process([0], x)
        finally:
            Q.close()
        assert np.array_equal(y_orig, y_plain)
        P.set_nr_algo(0, post.NR_WDSP)
        P.set_nr_enable(0, 1, 1)
        P.process([0], x)
        s2 = P.nr_state([0], 1)
        assert s2["anr_i"][0, 0] == (0 - 2 * n) & 511                   # resumed where it stood
        # kg_post_reset: a new connection -- algo off, enables and params cleared, filter state kept
        P.reset(0)
        P.process([0], x)
        s3 = P.nr_state([0], 1)
        assert s3["anr_i"][0, 0] == s2["anr_i"][0, 0]
        P.set_nr_algo(0, post.NR_WDSP)
        P.set_nr_param(0, 1, post.NR_GAIN, 1e-4)                         # re-init from the CLEARED vector: taps 0, delay 0
        s4 = P.nr_state([0], 1)
        assert list(s4["anr_i"][0]) == [0, 0, 0] and s4["anr_f"][0, 0] == 120.0
    finally:
        P.close()


def test_argument_errors(gpu_ctx):
    P = Post(gpu_ctx, nchan=2)
    try:
        def bad(f, *a):
            with pytest.raises(KiwiGpuError):
                f(*a)
        bad(P.set_nr_algo, 0, post.NR_SPECTRAL)
        bad(P.set_nr_algo, 2, post.NR_WDSP)
        bad(P.set_nr_enable, 0, 2, 1)
        bad(P.set_nr_enable, 0, -1, 1)
        bad(P.set_nr_param, 0, 2, 0, 1.0)
        bad(P.set_nr_param, 0, 0, 8, 1.0)
        bad(P.set_nr_param, 0, 0, -1, 1.0)
        P.set_nr_param(0, 0, post.NR_TAPS, float("nan"))                 # NR_OFF: stored, nothing converts it
        P.set_nr_param(0, 0, post.NR_TAPS, 64)
        P.set_nr_algo(0, post.NR_WDSP)
        for v in (float("nan"), float("inf"), -float("inf"), 3e9, 513):
            bad(P.set_nr_param, 0, 0, post.NR_TAPS, v)
        bad(P.set_nr_param, 0, 0, post.NR_DLY, 2147483520.0)
        P.set_nr_param(0, 0, post.NR_TAPS, 512)
        P.set_nr_param(0, 0, post.NR_DLY, -5)
        P.set_nr_algo(0, post.NR_ORIG)
        bad(P.set_nr_param, 0, 1, post.NR_DELAY, float("nan"))
        P.set_nr_param(0, 1, post.NR_DELAY, float("inf"))                # clamped to 300 before its conversion
        assert P.nr_state([0], 1)["lms_i"][0, 1] == 300
        # the standalone call site needs WDSP or ORIG
        P.set_nr_algo(1, post.NR_OFF)
        bad(P.nr_process, [1], 0, np.zeros((1, 16), np.int16))
        bad(P.nr_process, [0], 2, np.zeros((1, 16), np.int16))
        # a batch with NR on needs d_s16
        configure(P, 0, post.MODE_SSB)
        P.set_nr_algo(0, post.NR_ORIG)
        P.set_nr_enable(0, 0, 1)
        ctx = P.ctx
        d = ctx.alloc(8 * 512)
        try:
            with pytest.raises(KiwiGpuError):
                P.process_dev([0], d, 512, 512, 0, 0, d, 512)
        finally:
            ctx.sync()
            ctx.free(d)
    finally:
        P.close()
