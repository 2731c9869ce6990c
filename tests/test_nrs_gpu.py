"""kg_post's spectral noise reduction (NR_SPECTRAL: rx/rx_sound.cpp:945-947 -> rx/Teensy/NR_spectral.cpp) on the GPU: every scenario
of tests/golden/nrs_ref.npz (the reference's own commands and stage, tools/make_ref_nrs_golden.py) BIT-EXACT -- every int16 output
sample, every state value -- through kg_post_nrs_select / kg_post_set_nr_param / kg_post_nrs_passband and kg_post_nrs_process_dev:
all scenarios of a rate side by side in one batch (channels at different phases, out of place), each alone in place in calls of one,
two and three blocks; the fused pass of kg_post_process_dev equal to the same audio without NR followed by the standalone call;
a batch mixing NR_WDSP, NR_ORIG, spectral and NR-off channels with the non-spectral rows byte-identical to a run without any
spectral call; the state semantics; the refusals, which leave the state untouched.  On a digest mismatch the failing block is named
and diffed against the host driver (which tests/test_nrs_cpu.py holds to the same digests)."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post
from flydog_sdr_gps_amd._lib import KiwiGpuError

from . import nrs_common as nc

pytestmark = pytest.mark.gpu
FS = 12000.0


@pytest.fixture(scope="module")
def golden():
    return nc.load()


def explain(g, name, y, tmp_path):
    """the first block of y that differs from the host driver's output, for the assertion message"""
    exe = nc.build_driver(tmp_path)
    want, _, _, rc = nc.run_driver(exe, int(g[name + "_rate"]), nc.script(g, name), nc.scenario_input(g, name), tmp_path)
    assert rc == 0
    bad = np.flatnonzero(y != want)
    return "first difference at block %d sample %d: got %d, host driver %d; %d samples differ" % (
        bad[0] // nc.BLK, bad[0] % nc.BLK, y[bad[0]], want[bad[0]], bad.size) if bad.size else "equal to the host driver"


def check(g, name, y, states, what, tmp_path):
    try:
        nc.check_blocks(name, y, g, what)
    except AssertionError as e:
        raise AssertionError("%s -- %s" % (e, explain(g, name, y, tmp_path)))
    nc.check_states(name, states, g, what)


def test_all_scenarios_side_by_side_bit_exact(gpu_ctx, golden, tmp_path):
    """one kg_post per rate, one channel per scenario, one batch per round over the channels whose next block runs the stage: the
    channels are at different phases (start-up, phase 3, never initialised) and leave and re-enter the list; out of place"""
    names = nc.names(golden)
    assert len(names) >= 20
    for rate in (12000, 20250):
        mine = [n for n in names if int(golden[n + "_rate"]) == rate]
        assert len(mine) >= 3
        P = Post(gpu_ctx, nchan=len(mine) + 1)
        try:
            P.nrs_setup(rate)
            reps = [nc.Replay(P, ch + 1, nc.script(golden, n), nc.scenario_input(golden, n)) for ch, n in enumerate(mine)]
            live = list(reps)
            while live:
                batch = []
                for r in list(live):
                    nxt = r.step()
                    if nxt is None:
                        live.remove(r)
                    elif nxt[1]:
                        batch.append((r, nxt[0]))
                    else:
                        r.done(nxt[0])                  # stereo, or another algo without enables: the stage leaves the block alone
                if batch:
                    y = P.nrs_process([r.ch for r, _ in batch], np.stack([b for _, b in batch]), in_place=False)
                    for (r, _), row in zip(batch, y):
                        r.done(row)
            for n, r in zip(mine, reps):
                check(golden, n, r.output(), r.states, "side by side", tmp_path)
        finally:
            P.close()


@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_each_scenario_alone_in_place(gpu_ctx, golden, tmp_path, blocks):
    """each scenario on a fresh kg_post, in place, in calls of up to `blocks` blocks (1024- and 1536-sample calls equal 512-sample
    calls: a call is nr_spectral_process once per 512 samples)"""
    for n in nc.names(golden):
        P = Post(gpu_ctx, nchan=3)
        try:
            P.nrs_setup(int(golden[n + "_rate"]))
            r = nc.Replay(P, 2, nc.script(golden, n), nc.scenario_input(golden, n))
            while True:
                nxt = r.step()
                if nxt is None:
                    break
                if not nxt[1]:
                    r.done(nxt[0])
                    continue
                run = [nxt[0]]
                while len(run) < blocks and r.peek_is_block():
                    run.append(r.step()[0])
                r.done(P.nrs_process([2], np.concatenate(run)[None, :])[0])
            check(golden, n, r.output(), r.states, "alone, %d blocks a call" % blocks, tmp_path)
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


SPEC = "spectral"
# channel -> (mode, algo, {type: params}, enables (denoise, auto-notch), passband)
PLAN = {
    0: (post.MODE_SSB, SPEC, {0: [1, 0.95, 1000]}, (0, 0), (300.0, 2700.0)),
    1: (post.MODE_AM, SPEC, {1: [2, 0.9, 100]}, (0, 0), (-4900.0, 4900.0)),
    2: (post.MODE_SSB, post.NR_OFF, {}, (0, 0), None),
    3: (post.MODE_IQ, SPEC, {0: [1, 0.95, 1000]}, (0, 0), (-5000.0, 5000.0)),              # stereo: the stage is skipped
    4: (post.MODE_NBFM, SPEC, {0: [1, 0.95, 1000]}, (0, 0), (-5999.0, 5999.0)),
    5: (post.MODE_SAM, SPEC, {0: [0.5, 0.99, 30]}, (0, 0), (-4900.0, 4900.0)),
    6: (post.MODE_SSB, post.NR_WDSP, {1: [64, 16, 1e-4, 0.1], 0: [64, 16, 1e-4, 0.1]}, (1, 1), None),
    7: (post.MODE_SAS, SPEC, {0: [1, 0.95, 1000]}, (0, 0), (-4900.0, 4900.0)),             # stereo: skipped
    8: (post.MODE_AM, post.NR_ORIG, {1: [0, 0, 0], 0: [0, 0, 0]}, (1, 1), None),
    9: (post.MODE_SSB, SPEC, {}, (0, 0), (-2700.0, -300.0)),                               # selected, never initialised: silence
}


def set_nr(P, ch, plan, spectral=True):
    mode, algo, params, en, pb = plan
    if algo == SPEC:
        if not spectral:
            return
        P.nrs_passband(ch, *pb)
        P.nrs_select(ch)
    else:
        P.set_nr_algo(ch, algo)
    for t, vals in params.items():
        for k, v in enumerate(vals):
            P.set_nr_param(ch, t, k, v)
    for t in (0, 1):
        if en[t]:
            P.set_nr_enable(ch, t, en[t])


def test_fused_pass_equals_post_then_standalone(gpu_ctx):
    """A: kg_post_process_dev with the stage on.  B: the same channels, spectral ones in NR_OFF during the pass and the standalone
    call by hand on their rows.  C: no spectral call at all -- its non-spectral rows equal A's byte for byte."""
    n = 512
    A, B, Cc = Post(gpu_ctx, nchan=10), Post(gpu_ctx, nchan=10), Post(gpu_ctx, nchan=10)
    try:
        for ch, plan in PLAN.items():
            for P in (A, B, Cc):
                configure(P, ch, plan[0])
            set_nr(A, ch, plan)
            set_nr(B, ch, plan)
            set_nr(Cc, ch, plan, spectral=False)
        chans = list(PLAN)
        spectral_ran = {ch: False for ch in chans}
        for blk in range(14):
            x = np.stack([ssb_input(n, 10 * blk + ch) for ch in chans])
            ya, da, ga = A.process(chans, x)
            for ch, plan in PLAN.items():                   # B: the pass without the stage, then the stage by hand
                if plan[1] == SPEC:
                    B.set_nr_algo(ch, post.NR_OFF)
            yb, db, gb = B.process(chans, x)
            yc, dc, gc = Cc.process(chans, x)
            for i, ch in enumerate(chans):
                mode, algo = PLAN[ch][0], PLAN[ch][1]
                assert np.array_equal(ga[i].view(np.uint32), gb[i].view(np.uint32)), ch
                assert np.array_equal(ga[i].view(np.uint32), gc[i].view(np.uint32)), ch
                assert np.array_equal(da[i].view(np.uint32), dc[i].view(np.uint32)), ch
                if algo == SPEC:
                    B.nrs_select(ch)
                if algo != SPEC or mode in post.STEREO_MODES:
                    assert np.array_equal(ya[i], yb[i]) and np.array_equal(ya[i], yc[i]), (ch, blk)
                    continue
                want = B.nrs_process([ch], yb[i][None, :])[0]
                assert np.array_equal(ya[i], want), (ch, blk)
                assert np.array_equal(yb[i], yc[i]), (ch, blk)
                spectral_ran[ch] |= not np.array_equal(ya[i], yb[i])
        for ch, plan in PLAN.items():
            if plan[1] == SPEC:
                sa, sb = A.nrs_state([ch]), B.nrs_state([ch])
                for k in sa:
                    assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), (ch, k)
                if plan[0] not in post.STEREO_MODES:
                    assert spectral_ran[ch], (ch, "the stage changed nothing")
                    if plan[2]:
                        assert sa["ints"][0, 0] == 3, (ch, "phase 3 was not reached")
                else:
                    assert sa["ints"][0, 0] == 1 and sa["ints"][0, 1] == 0, (ch, "a stereo channel's state advanced")
    finally:
        A.close(); B.close(); Cc.close()


def test_fused_batch_of_1024_samples_and_changing_lists(gpu_ctx):
    """a 1024-sample pass is two blocks; channels entering and leaving the list keep their own state"""
    M, alone = Post(gpu_ctx, nchan=3), [Post(gpu_ctx, nchan=1) for _ in range(3)]
    try:
        for ch in range(3):
            for P, c in ((M, ch), (alone[ch], 0)):
                configure(P, c, post.MODE_SSB)
                P.nrs_passband(c, 300.0, 2700.0 + 100 * ch)
                P.nrs_select(c)
                for k, v in enumerate([1, 0.95, 1000]):
                    P.set_nr_param(c, 0, k, v)
        for blk, (lst, n) in enumerate([([0, 1, 2], 512), ([2, 0], 1024), ([1], 512), ([0, 1, 2], 1024), ([2, 1, 0], 512)] * 3):
            x = np.stack([ssb_input(n, 100 * blk + ch) for ch in lst])
            y, _, _ = M.process(lst, x)
            for i, ch in enumerate(lst):
                ya = np.concatenate([alone[ch].process([0], x[i][None, k:k + 512])[0][0] for k in range(0, n, 512)])
                assert np.array_equal(y[i], ya), (blk, ch)
        for ch in range(3):
            a, b = M.nrs_state([ch]), alone[ch].nrs_state([0])
            for k in a:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ch, k)
            assert a["ints"][0, 0] == 3
    finally:
        M.close()
        for P in alone:
            P.close()


def test_state_semantics(gpu_ctx):
    P = Post(gpu_ctx, nchan=2)
    try:
        configure(P, 0, post.MODE_SSB)
        P.nrs_passband(0, 300.0, 2700.0)
        P.nrs_select(0)
        P.set_nr_param(0, 1, post.NR_ALPHA, 0.95)               # the first init: first_time = 1, through type index 1
        s = P.nrs_state([0])
        assert list(s["ints"][0]) == [1, 0, 12, 116] and s["scalars"][0, 1] == np.float32(0.95) and s["scalars"][0, 0] == 0
        assert (s["arrays"][0, 0] == np.float32(0.1)).all() and (s["arrays"][0, 5] == 2.0).all() and (s["arrays"][0, 6] == 1.0).all()
        x = ssb_input(512, 3)[None, :]
        for _ in range(3):
            P.process([0], x)
        s1 = P.nrs_state([0])
        assert list(s1["ints"][0, :2]) == [2, 6]
        P.set_mode(0, post.MODE_AM); P.set_mode(0, post.MODE_SSB)       # a mode change leaves the state alone
        P.set_nr_algo(0, post.NR_WDSP)                                  # leaving: nothing advances, nothing is re-armed
        P.process([0], x)
        s2 = P.nrs_state([0])
        assert all(np.array_equal(s1[k].view(np.uint32), s2[k].view(np.uint32)) for k in s1)
        P.set_nr_param(0, 0, post.NR_S_GAIN, 5.0)                       # under NR_WDSP: wdsp's init, not nr_spectral_init
        assert P.nrs_state([0])["scalars"][0, 0] == 0
        P.nrs_select(0)
        P.process([0], x)
        assert list(P.nrs_state([0])["ints"][0, :2]) == [2, 8]          # resumed where it stood
        P.reset(0)                                                      # a new connection: NR off, passband zeroed, state kept
        P.process([0], x)
        s3 = P.nrs_state([0])
        assert list(s3["ints"][0]) == [2, 8, 1, 2] and list(s3["scalars"][0, 6:8]) == [0, 0]
        with pytest.raises(KiwiGpuError):
            P.nrs_select(0)                                             # the zeroed passband is bins 1..2
        P.nrs_passband(0, -2700.0, -300.0)
        P.nrs_select(0)
        P.set_nr_param(0, 0, post.NR_S_GAIN, 2.0)                       # re-parameterised from the CLEARED vector; first_time not re-armed
        s4 = P.nrs_state([0])
        assert list(s4["ints"][0]) == [2, 8, 12, 116] and list(s4["scalars"][0, :3]) == [2.0, 0.0, 0.0]
        P.nrs_setup(20250)                                              # the bins follow the rate
        assert list(P.nrs_state([0])["ints"][0, 2:]) == [7, 69]
    finally:
        P.close()


def test_refusals_leave_the_state_untouched(gpu_ctx):
    P = Post(gpu_ctx, nchan=2)
    ctx = P.ctx
    try:
        def bad(f, *a):
            with pytest.raises(KiwiGpuError):
                f(*a)
        configure(P, 0, post.MODE_SSB)
        bad(P.nrs_select, 0)                                            # no passband yet: bins 1..2
        bad(P.nrs_select, 2)
        bad(P.nrs_passband, -1, 300.0, 2700.0)
        bad(P.set_nr_algo, 0, post.NR_SPECTRAL)                         # that entry point keeps its refusal
        P.nrs_passband(0, 0.0, 300.0)                                   # NR off: any passband is stored
        bad(P.nrs_select, 0)                                            # VAD_high = 13 < 17
        P.nrs_passband(0, 300.0, 2700.0)
        bad(P.nrs_process, [0], np.zeros((1, 512), np.int16))           # the standalone call needs the algo
        P.nrs_select(0)
        for k, v in enumerate([1, 0.95, 1000]):
            P.set_nr_param(0, 0, k, v)
        x = ssb_input(512, 5)[None, :]
        for _ in range(12):
            P.process([0], x)
        before = P.nrs_state([0])
        assert before["ints"][0, 0] == 3
        bad(P.nrs_passband, 0, 0.0, 370.0)                              # VAD 1..16 under spectral NR: refused, previous kept
        bad(P.nrs_passband, 0, 5800.0, 5999.0)                          # VAD_low = 247 > 244
        bad(P.nrs_setup, 96000)                                         # 300..2700 Hz at 96 kHz is bins 1..15
        bad(P.nrs_process, [0], np.zeros((1, 256), np.int16))           # nsamps % 512
        bad(P.nrs_process, [0], np.zeros((1, 768), np.int16))
        bad(P.nrs_process, [0], np.zeros((1, 512 * 9), np.int16))       # more than KG_NRS_MAX_SAMPLES
        bad(P.nrs_process, [0, 0], np.zeros((2, 512), np.int16))        # listed twice
        bad(P.nrs_process, [5], np.zeros((1, 512), np.int16))           # a bad channel
        d = ctx.alloc(8 * 1024)
        o = ctx.alloc(2 * 1024)
        try:
            bad(P.process_dev, [0], d, 512, 512, 0, 0, d, 512)          # the fused pass needs d_s16 ...
            bad(P.process_dev, [0], d, 256, 256, o, 0, 0, 256)          # ... and whole blocks
            bad(P.process_dev, [0], d, 768, 768, o, 0, 0, 768)
        finally:
            ctx.sync()
            ctx.free(d); ctx.free(o)
        after = P.nrs_state([0])
        for k in before:
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        assert list(after["ints"][0, 2:]) == [12, 116] and list(after["scalars"][0, 6:8]) == [300.0, 2700.0]
        P.process([0], x)                                               # and the channel goes on
        assert not np.array_equal(P.nrs_state([0])["arrays"].view(np.uint32), before["arrays"].view(np.uint32))
    finally:
        P.close()
