"""GPU parity of the standard noise blanker (NB_STD): every scenario of tests/golden/nb_ref.npz -- the reference's own CNoiseProc
(tools/make_ref_nb_golden.py) -- through kg_nb_process_dev (audio) and kg_wf_nb_frames_dev (waterfall), bit for bit, end states
included; blanked frames through kg_wf_frames_dev against the oracle's compute_frame fed the reference's blanked frames (under
tests/test_wf_gpu.py's bar); plain rows unchanged beside blanked ones; the refusals."""
import os

import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, NoiseBlanker, Waterfall, WfParams, synth, wf
from tests import nb_signals
from tests.test_nb_cpu import digest
from tests.test_wf_gpu import check_row, db_bound, RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "nb_ref.npz"))
AUDIO = [str(n) for n in G["audio_names"]]
WFN = [str(n) for n in G["wf_names"]]
MAX_IN = 1 << 14
ERR_INVALID, ERR_STATE = -2, -5


def script(name):
    return [str(l) for l in G[name + "_script"]]


def audio_input(name):
    sig = G[name + "_sig"]
    n = sum(int(l.split()[1]) for l in script(name) if l[0] == "B")
    return nb_signals.audio(str(sig[0]), n, int(sig[1]))


def setup_args(line):
    a = line.split()[1:]
    return np.float32(a[0]), [np.float32(a[1]), np.float32(a[2])]


@pytest.fixture(scope="module")
def nb(gpu_ctx):
    b = NoiseBlanker(gpu_ctx, nchan=32, max_in=MAX_IN)
    yield b
    b.close()


@pytest.fixture(scope="module")
def dbuf(gpu_ctx):
    n = 32 * MAX_IN * 8
    d_in, d_out = gpu_ctx.alloc(n), gpu_ctx.alloc(n)
    yield d_in, d_out
    gpu_ctx.free(d_in)
    gpu_ctx.free(d_out)


def replay_audio(ctx, nb, d_in, d_out, ch, name, in_place):
    """the scenario's script on channel ch through kg_nb_process_dev: per block the output, per S the state"""
    x = audio_input(name)
    p, outs, states = 0, [], []
    for l in script(name):
        if l[0] == "U":
            rate, prm = setup_args(l)
            nb.setup(ch, rate, prm)
        elif l[0] == "B":
            n = int(l.split()[1])
            blk = np.ascontiguousarray(x[p:p + n]); p += n
            if n:
                ctx.upload(d_in, blk)
            dst = d_in if in_place else d_out
            nb.process_dev([ch], d_in, MAX_IN, [n], dst, MAX_IN)
            y = np.empty((n, 2), np.float32)
            if n:
                ctx.sync()
                ctx.download(dst, y)
            outs.append(y)
        elif l[0] == "S":
            states.append(nb.state(ch))
    return outs, states


def check_audio(name, outs, states):
    want = G[name + "_sha"]
    assert len(outs) == len(want)
    for k, o in enumerate(outs):
        assert np.array_equal(digest(o.tobytes()), want[k]), (name, "block", k)
    si = np.array([s[0][0] for s in states], np.int32)
    sf = np.array([s[1][0] for s in states], np.float32)
    assert np.array_equal(si, G[name + "_state_i"]), (name, si, G[name + "_state_i"])
    assert np.array_equal(sf.view(np.uint32), G[name + "_state_f"].view(np.uint32)), (name, sf, G[name + "_state_f"])


@pytest.mark.parametrize("name", AUDIO)
@pytest.mark.parametrize("in_place", [True, False])
def test_audio_scenarios_bit_exact(gpu_ctx, nb, dbuf, name, in_place):
    outs, states = replay_audio(gpu_ctx, nb, dbuf[0], dbuf[1], 3, name, in_place)
    check_audio(name, outs, states)


def test_audio_host_call(nb):
    name = "snd_chunked"
    x = audio_input(name)
    p, outs = 0, []
    for l in script(name):
        if l[0] == "U":
            rate, prm = setup_args(l)
            nb.setup(5, rate, prm)
        elif l[0] == "B":
            n = int(l.split()[1])
            outs.append(nb.process(5, x[p:p + n])); p += n
    for k, o in enumerate(outs):
        assert np.array_equal(digest(o.tobytes()), G[name + "_sha"][k]), k


def test_mixed_batch_equals_single_channels(gpu_ctx, nb, dbuf):
    """scenarios with one setup, run side by side: block r of each in ONE call (different rates, params, block sizes, zero counts)"""
    names = [n for n in AUDIO if sum(l[0] == "U" for l in script(n)) == 1 and script(n)[-1] == "S"]
    assert len(names) >= 8
    d_in = dbuf[0]
    chans = np.arange(len(names), dtype=np.int32) * 2 + 1          # rows i, channels 1, 3, 5 ...
    xs, blocks, pos = [], [], []
    for i, name in enumerate(names):
        rate, prm = setup_args(script(name)[0])
        nb.setup(int(chans[i]), rate, prm)
        xs.append(audio_input(name))
        blocks.append([int(l.split()[1]) for l in script(name) if l[0] == "B"])
        pos.append(0)
    outs = [[] for _ in names]
    for r in range(max(len(b) for b in blocks)):
        cnt = np.array([b[r] if r < len(b) else 0 for b in blocks], np.int32)
        buf = np.zeros((len(names), MAX_IN, 2), np.float32)
        for i in range(len(names)):
            buf[i, :cnt[i]] = xs[i][pos[i]:pos[i] + cnt[i]]
        gpu_ctx.upload(d_in, buf)
        nb.process_dev(chans, d_in, MAX_IN, cnt, d_in, MAX_IN)      # in place
        gpu_ctx.sync()
        gpu_ctx.download(d_in, buf)
        for i in range(len(names)):
            if r < len(blocks[i]):
                outs[i].append(buf[i, :cnt[i]].copy())
                pos[i] += cnt[i]
    ints, flts = nb.state(chans)
    for i, name in enumerate(names):
        check_audio(name, outs[i], [(ints[i:i + 1], flts[i:i + 1])])


# ---- waterfall ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    return wf.window_functions(), wf.cic_comp_table()


def wf_engine(ctx, tables, nchan=8):
    w = Waterfall(ctx, nchan=nchan)
    w.set_tables(*tables)
    return w


def wf_input(name):
    sig = G[name + "_sig"]
    return nb_signals.wf_frames(str(sig[0]), int(sig[2]), int(sig[1])), int(sig[3])


@pytest.mark.parametrize("name", WFN)
@pytest.mark.parametrize("per_call", [1, 0])
def test_wf_scenarios_bit_exact(gpu_ctx, tables, name, per_call):
    """every W / F / T line through kg_wf_nb_setup / kg_wf_nb_frames_dev / kg_wf_nb_state; per_call 1: a call per frame, 0: every
    run of F lines in one call (the state carries from frame to frame inside the pre-pass)"""
    frames, wfn = wf_input(name)
    w = wf_engine(gpu_ctx, tables)
    ch = 6
    w.set_channel(ch, WfParams.for_zoom(0, 0.0), window_func=wfn)
    d_iq = gpu_ctx.alloc(frames.nbytes)
    d_out = gpu_ctx.alloc(frames.shape[0] * 8192 * 8)
    gpu_ctx.upload(d_iq, frames)
    outs, states, f, run = [], [], 0, []

    def flush():
        if run:
            w.nb_frames([ch] * len(run), d_iq, d_out, np.array(run, np.uint64) * 8192, frames.shape[0] * 8192)
            y = np.empty((len(run), 8192, 2), np.float32)
            gpu_ctx.sync()
            gpu_ctx.download(d_out, y)
            outs.extend(list(y))
            run.clear()
    try:
        for l in script(name):
            if l[0] == "W":
                flush()
                a = l.split()[1:]
                w.nb_setup(ch, [np.float32(a[0]), np.float32(a[1])])
            elif l[0] == "F":
                run.append(f); f += 1
                if per_call:
                    flush()
            elif l[0] == "T":
                flush()
                states.append(w.nb_state(ch))
        flush()
    finally:
        gpu_ctx.free(d_iq)
        gpu_ctx.free(d_out)
        w.close()
    want = G[name + "_sha"]
    assert len(outs) == len(want)
    for k, o in enumerate(outs):
        assert np.array_equal(digest(np.ascontiguousarray(o).tobytes()), want[k]), (name, "frame", k)
    for k, fr in zip(G[name + "_keep"], G[name + "_frames"]):
        assert np.array_equal(outs[k].view(np.uint32), fr.view(np.uint32)), (name, k)
    si = np.array([s[0][0] for s in states], np.int32)
    sf = np.array([s[1][0] for s in states], np.float32)
    assert np.array_equal(si, G[name + "_state_i"]) and np.array_equal(sf.view(np.uint32), G[name + "_state_f"].view(np.uint32))


def test_blanked_rows_match_oracle_and_plain_rows_unchanged(gpu_ctx, oracle, tables):
    """kg_wf_frames_dev with the blanker on for one channel: its rows against the oracle's compute_frame fed the reference's
    blanked frames (the kept frames of wf_seq), under tests/test_wf_gpu.py's bar; the plain channels' rows byte-identical to a call
    without any blanked channel."""
    name = "wf_seq"
    frames, wfn = wf_input(name)
    keep = [int(k) for k in G[name + "_keep"]]
    nf = max(keep) + 1
    w = wf_engine(gpu_ctx, tables)
    p = WfParams.for_zoom(0, 0.0)
    pz = WfParams.for_zoom(4, 3.0e6)
    w.set_channel(0, p, window_func=wfn)
    w.set_channel(1, pz, interp=wf.WF_MAX, window_func=wf.WINF_BLACKMAN_HARRIS)
    w.set_channel(2, p, interp=wf.WF_CMA, window_func=wf.WINF_HAMMING)
    plain = np.stack([synth.wf_iq_frame(seed=500 + k) for k in range(2 * nf)])
    # the list: blanked frames of channel 0 interleaved with plain frames of channels 1 and 2
    chan_of, iq = [], []
    for k in range(nf):
        chan_of += [1, 0, 2]
        iq += [plain[2 * k], frames[k], plain[2 * k + 1]]
    chan_of = np.array(chan_of, np.int32)
    iq = np.stack(iq)
    try:
        base = w.frames(chan_of, iq)                 # no blanker anywhere
        a = np.array(G[name + "_script"][0].split()[1:], np.float32)
        w.nb_setup(0, a)
        w.set_nb(0, True)
        rows = w.frames(chan_of, iq)
        w.set_nb(0, False)
        again = w.frames(chan_of, iq)
    finally:
        w.close()
    plain_rows = chan_of != 0
    assert np.array_equal(rows[plain_rows], base[plain_rows])
    assert np.array_equal(again, base)
    windows, cic = tables
    m, d = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped)
    sc = np.full(1024, p.fft_scale, np.float32)
    blanked_rows = rows[chan_of == 0]
    assert not np.array_equal(blanked_rows, base[chan_of == 0])
    for k, fr in zip(keep, G[name + "_frames"]):
        samps = np.ascontiguousarray(fr).view(np.complex64).reshape(-1)
        w_out, w_pwr, w_pwr_out, w_dB = oracle.wf_compute_frame(samps, p.zoom, wfn, wf.WF_CMA, True, False, p.fft_used, p.plot_width,
                                                                 p.plot_width_clamped, m, d, sc, (sc / np.float32(2)).astype(np.float32),
                                                                 p.fft_offset, cic)
        check_row(blanked_rows[k], w_out, w_dB, db_bound(w_pwr_out))


def test_two_blanked_channels_interleaved(gpu_ctx, tables):
    """two blanked channels (different gates and windows) interleaved with a plain one in ONE kg_wf_frames call: each blanked
    channel's rows equal that channel alone, frame by frame (fresh setups); the plain rows equal a call without the blanker"""
    fa, _ = wf_input("wf_seq")
    fb, _ = wf_input("wf_wide_flush")
    nf = 6
    plain = np.stack([synth.wf_iq_frame(seed=900 + k) for k in range(nf)])
    w = wf_engine(gpu_ctx, tables)
    p0, p4 = WfParams.for_zoom(0, 0.0), WfParams.for_zoom(4, 2.0e6)
    try:
        w.set_channel(3, p0, window_func=wf.WINF_HANNING)
        w.set_channel(5, p4, interp=wf.WF_MAX, window_func=wf.WINF_BLACKMAN_HARRIS)
        w.set_channel(1, p0, window_func=wf.WINF_HAMMING)
        chan_of, iq = [], []
        for k in range(nf):
            chan_of += [5, 1, 3] if k % 2 else [3, 5, 1]
            iq += [fb[k], plain[k], fa[k]] if k % 2 else [fa[k], fb[k], plain[k]]
        chan_of = np.array(chan_of, np.int32)
        iq = np.stack(iq)
        base = w.frames(chan_of, iq)
        w.nb_setup(3, [100.0, 50.0]); w.nb_setup(5, [100000.0, 30.0])
        w.set_nb(3, True); w.set_nb(5, True)
        rows = w.frames(chan_of, iq)
        for ch, src in ((3, fa), (5, fb)):
            w.nb_setup(ch, [100.0, 50.0] if ch == 3 else [100000.0, 30.0])
            alone = np.stack([w.frames([ch], src[k][None])[0] for k in range(nf)])
            assert np.array_equal(rows[chan_of == ch], alone), ch
            assert not np.array_equal(rows[chan_of == ch], base[chan_of == ch]), ch
        assert np.array_equal(rows[chan_of == 1], base[chan_of == 1])
    finally:
        w.close()


def test_debug_frame_applies_the_blanker(gpu_ctx, tables):
    frames, wfn = wf_input("wf_seq")
    w = wf_engine(gpu_ctx, tables)
    try:
        w.set_channel(0, WfParams.for_zoom(0, 0.0), window_func=wfn)
        w.nb_setup(0, [100.0, 50.0])
        w.set_nb(0, True)
        out, _, _, _ = w.debug_frame(0, frames[0])
        w.nb_setup(0, [100.0, 50.0])                 # the same state again: a one-frame call gives the same row
        assert np.array_equal(w.frames([0], frames[:1])[0], out)
    finally:
        w.close()


def test_refusals(gpu_ctx, tables, nb, dbuf):
    def status(fn, *a):
        with pytest.raises(KiwiGpuError) as e:
            fn(*a)
        return e.value.status
    fresh = NoiseBlanker(gpu_ctx, nchan=4, max_in=1024)
    try:
        assert status(fresh.process_dev, [0], dbuf[0], 1024, [16], dbuf[0], 1024) == ERR_STATE      # never set up
        assert status(fresh.process, 1, np.zeros((8, 2), np.float32)) == ERR_STATE
        assert status(fresh.setup, 2, 0.0, [100.0, 50.0]) == ERR_STATE                                # rate 0 before any setup
        assert status(fresh.state, [3]) == ERR_STATE
        assert status(fresh.setup, 0, 12000.0, [1e30, 50.0]) == ERR_INVALID                          # gate outside int
        assert status(fresh.setup, 0, 12000.0, [float("nan"), 50.0]) == ERR_INVALID
        assert status(fresh.setup, 0, 205000.0, [100.0, 50.0]) == ERR_INVALID                        # beyond KG_NB_MAG_CAP
        assert status(fresh.setup, 0, float("nan"), [100.0, 50.0]) == ERR_INVALID
        fresh.setup(0, 12000.0, [100.0, 50.0])
        assert status(fresh.process_dev, [0], dbuf[0], 1024, [1025], dbuf[0], 1024) == ERR_INVALID   # above max_in
        assert status(fresh.process_dev, [0, 0], dbuf[0], 1024, [8, 8], dbuf[0], 1024) == ERR_INVALID
        assert status(fresh.process_dev, [4], dbuf[0], 1024, [8], dbuf[0], 1024) == ERR_INVALID
        assert status(fresh.process_dev, [0], dbuf[0], 1024, [-1], dbuf[0], 1024) == ERR_INVALID
        fresh.process_dev([0], dbuf[0], 1024, [0], dbuf[0], 1024)                                     # all counts 0: nothing
        assert fresh.state(0)[0][0, 0] == 0
    finally:
        fresh.close()
    w = wf_engine(gpu_ctx, tables, nchan=2)
    d = gpu_ctx.alloc(8192 * 8)
    try:
        w.set_channel(0, WfParams.for_zoom(0, 0.0))
        assert status(w.set_nb, 0, True) == ERR_STATE
        w.set_nb(0, False)
        assert status(w.nb_frames, [0], d, d, [0], 8192) == ERR_STATE
        assert status(w.nb_state, [0]) == ERR_STATE
        assert status(w.nb_setup, 0, [1e30, 50.0]) == ERR_INVALID
        assert status(w.set_nb, 2, True) == ERR_INVALID
        w.nb_setup(0, [100.0, 50.0])
        assert status(w.nb_frames, [0], d, d, [8], 8192) == ERR_INVALID                              # runs past iq_len
        assert status(w.nb_frames, [1], d, d, [0], 8192) == ERR_STATE                                # channel 1 never configured
    finally:
        gpu_ctx.free(d)
        w.close()
