"""kg_post -- the whole audio post path -- against c2s_sound()'s own statements from `s_samps_c = fir_samps_c` to the end of the NR
switch (rx/rx_sound.cpp:676-949) run as one program with every stage linked (tests/golden/post_rand_ref.npz, made by
tools/make_ref_post_golden.py --random from tools/ref/ref_post_main.cpp), driven by the 40 seeded random scripts and the 11
AGC-window shapes of tests/post_random.py.  BIT-EXACT, digest for digest:

  * every script alone, nchan = 1, blocks as recorded: out_samps_s2 behind the NR switch, agc_samps_c, sMeterAvg_dB and its two
    taps, wdsp_SAM_carrier, isChanNull, s->squelched, and at the end the ANR / CLMS, Wild and spectral states;
  * the same sample stream under two other partitions into calls -- merged (blocks with no command between them joined up to 1024
    samples) and, for the ragged scripts, split (pieces of 1, 7, 64, 170): streams and end states equal the record.  NBFM blocks
    stay as recorded there: the reference's squelch decides once per call (post_random.per_call);
  * each group of four seeds as one batch of a five-channel object whose fifth channel is configured and never listed, the list
    order rotating every call: every channel equals its own record whoever shares its launch, and the fifth is left as it was.

On a mismatch the failure names the first stream that differs in the order agc_samps_c -> out_samps_s2 ahead of the Wild stage (from
a second object with the stages off) -> out_samps_s2."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post
from tests import post_random as C
from tests.script_common import digest

pytestmark = pytest.mark.gpu

GOLDEN = C.load()
SCRIPTS = C.all_scripts()
NAMES = list(SCRIPTS)
SEEDS = [n for n in NAMES if n[0] == "r"]
RAGGED_SEEDS = [n for n in SEEDS if C.group_of(int(n[1:]))[1]]
_inputs = {}


def record(name):
    return C.Record(C.unjoin(GOLDEN, name), name, SCRIPTS[name])


def stream(name):
    if not _inputs:
        _inputs["pool"] = C.pool()
    if name not in _inputs:
        _inputs[name] = C.as_complex(C.script_input(SCRIPTS[name], _inputs["pool"]))
    return _inputs[name]


def bits(v):
    return np.float32(v).view(np.uint32)


def nominal(name):
    return name[0] != "w"


def pre_of(ctx, name, k):
    """out_samps_s2 of recorded block k ahead of rx_sound.cpp:922: the script on a second object with the stages off"""
    lines, x = SCRIPTS[name], stream(name)
    P = Post(ctx, nchan=1)
    try:
        ch = C.Channel(P, 0, lines, stages=False, nominal=nominal(name))
        pos = 0
        for s in C.steps_of(lines):
            if s[0] == "cmd":
                ch.cmd(s[1])
                continue
            s16 = P.process([0], x[pos:pos + s[1]][None, :])[0][0]
            pos += s[1]
            if s[2][0] == k:
                return s16
    finally:
        P.close()


def first_difference(ctx, name, rec, k, s16, agc):
    """which stream of recorded block k differs first: agc_samps_c, out_samps_s2 ahead of the Wild stage, or behind the NR switch"""
    b = rec.blocks[k]
    if b["agc"] is not None and digest(np.ascontiguousarray(agc, np.complex64).tobytes()) != b["agc"]:
        return "agc_samps_c"
    if b["s16"] is None or digest(np.ascontiguousarray(s16, np.int16).tobytes()) == b["s16"]:
        return None
    if digest(pre_of(ctx, name, k).tobytes()) != b["pre"]:
        return "out_samps_s2 ahead of the Wild stage (s16_pre)"
    return "out_samps_s2 behind the NR switch (s16), stages %s" % "/".join(b["stages"])


class Checker:
    """the outputs of a channel's calls, cut back into the recorded blocks and held against the record"""

    def __init__(self, ctx, name, rec, partition):
        self.ctx, self.name, self.rec, self.partition = ctx, name, rec, partition
        self.s16, self.agc, self.blocks = [], [], 0

    def call(self, P, ch, step, s16, agc):
        """after a call that ran step on channel ch of P with these output rows"""
        rec = self.rec
        self.s16.append(np.asarray(s16, np.int16)); self.agc.append(np.asarray(agc, np.complex64))
        ids, lens = step[2], step[3]
        if not ids:
            return
        s16, agc = np.concatenate(self.s16), np.concatenate(self.agc)
        self.s16, self.agc = [], []
        assert len(s16) == sum(lens), (self.name, self.partition, ids)
        at = 0
        for k, n in zip(ids, lens):
            b = rec.blocks[k]
            assert b["n"] == n
            bad = first_difference(self.ctx, self.name, rec, k, s16[at:at + n], agc[at:at + n])
            assert bad is None, (self.name, self.partition, "block", k, C.MODE_NAMES[b["mode"]], n, "first stream that differs:", bad)
            if self.name in C.FULL and b["s16"] is not None:
                done = sum(c["n"] for c in rec.blocks[:k] if c["s16"] is not None)
                assert np.array_equal(s16[at:at + n], rec.full["s16"][done:done + n]), (self.name, k)
            at += n
            self.blocks += 1
        k = ids[-1]
        where = (self.name, self.partition, "behind block", k, C.MODE_NAMES[rec.blocks[k]["mode"]])
        avg, taps = P.smeter([ch])
        car, null, _ = P.sam_state([ch])
        assert bits(avg[0]) == bits(rec.smeter[k, 0]), (where, "sMeterAvg_dB", avg[0], rec.smeter[k, 0])
        assert int(null[0]) == rec.chan_null(k), (where, "isChanNull")
        if rec.blocks[k]["mode"] == C.M_NBFM:
            assert int(P.squelch_state([ch])[1][0]) == rec.squelched(k), (where, "s->squelched")
        if self.partition in ("recorded", "batch"):      # per call: the taps (j = 0, j = n / 2), the carrier's averager (SAM_demod.cpp:341-344)
            assert bits(car[0]) == bits(rec.carrier[k]), (where, "wdsp_SAM_carrier", car[0], rec.carrier[k])
            assert np.float32(taps[0, 0]) + C.S_METER_CAL == rec.smeter[k, 1], (where, "S-meter tap j = 0")
            assert lens[-1] < 2 or np.float32(taps[0, 1]) + C.S_METER_CAL == rec.smeter[k, 2], (where, "S-meter tap j = n / 2")

    def end(self, chan):
        rec = self.rec
        assert self.blocks == len(rec.blocks) and not self.s16, (self.name, self.partition)
        ints, sha = chan.end_state()
        want = C.state_ints(rec)
        assert np.array_equal(ints, want), (self.name, self.partition, "end state integers", ints, want)
        for i, what in enumerate(C.STATE_NAMES):
            assert sha[i] == bytes(rec.state_sha[i]), (self.name, self.partition, "end state", what)


def run_alone(ctx, name, partition):
    lines, x, rec = SCRIPTS[name], stream(name), record(name)
    steps = C.steps_of(lines)
    if partition == "merged":
        steps = C.merged(steps, C.per_call(rec))
    elif partition == "split":
        steps = C.split(steps, int(name[1:]), C.per_call(rec))
    assert sum(s[1] for s in steps if s[0] == "blk") == len(x)
    P = Post(ctx, nchan=1)
    try:
        P.nrs_setup(C.snd_rate_of(float(lines[0].split()[1])))
        ch = C.Channel(P, 0, lines, nominal=nominal(name))
        chk = Checker(ctx, name, rec, partition)
        pos = 0
        for s in steps:
            if s[0] == "cmd":
                ch.cmd(s[1])
                continue
            s16, _, agc = P.process([0], x[pos:pos + s[1]][None, :])
            pos += s[1]
            chk.call(P, 0, s, s16[0], agc[0])
        chk.end(ch)
        if name[0] == "w":
            assert P.agc_delay(0) == int(rec.wd[1]) == C.shape_wd(name)[2], (name, "GetDelaySamples()")
    finally:
        P.close()
    return len(steps)


@pytest.mark.parametrize("name", NAMES)
def test_every_script_alone(gpu_ctx, name):
    run_alone(gpu_ctx, name, "recorded")


@pytest.mark.parametrize("name", NAMES)
def test_merged_calls_equal_the_record(gpu_ctx, name):
    calls = run_alone(gpu_ctx, name, "merged")
    assert name[0] != "w" or calls < len(C.steps_of(SCRIPTS[name])), (name, "nothing was merged")


@pytest.mark.parametrize("name", RAGGED_SEEDS)
def test_split_calls_equal_the_record(gpu_ctx, name):
    run_alone(gpu_ctx, name, "split")


# ---- each group of four as one batch ------------------------------------------------------------------------------------------
def configure_bystander(P, ch, rate):
    """channel 4: every stage on, a SAM mode, and never listed"""
    bystander = [C.r_line(rate)] + C.passband_lines(300, 2700, rate) + [
        "A 1 1 -90 50 4 500", "E 1 1", "N 12", "M %d" % C.M_SAU, "nbA 2", "nbP 0 0 3", "nbP 0 1 10", "nbP 0 2 7", "nbE 0 1",
        "nrA 1", "nrP 0 0 64", "nrP 0 1 16", "nrP 0 2 1e-4", "nrP 0 3 0.1", "nrP 1 0 32", "nrP 1 1 3", "nrP 1 2 1e-4", "nrP 1 3 0.1", "nrE 0 1", "nrE 1 1"]
    c = C.Channel(P, ch, bystander)
    for l in bystander[1:]:
        c.cmd(l)
    return c


def bystander_state(P, c, ch):
    ints, sha = c.end_state()
    avg, taps = P.smeter([ch])
    car, null, phz = P.sam_state([ch])
    return (ints.tolist(), sha, bits(avg[0]), taps.tobytes(), bits(car[0]), int(null[0]), bits(phz[0]), [np.asarray(v).tobytes() for v in P.squelch_state([ch])],
            P.agc_delay(ch))


def run_batch(ctx, names, rate, lens, want_sam_mix):
    """the scripts of names, which share rate and block list, as channels 0 .. of one five-channel object; channel 4 a bystander"""
    nn = len(names)
    recs = [record(n) for n in names]
    xs = [stream(n) for n in names]
    steps = [C.steps_of(SCRIPTS[n]) for n in names]
    F = Post(ctx, nchan=5)                               # the fresh object the bystander is held against
    try:
        F.nrs_setup(C.snd_rate_of(rate))
        want4 = bystander_state(F, configure_bystander(F, 4, rate), 4)
    finally:
        F.close()
    P = Post(ctx, nchan=5)
    try:
        P.nrs_setup(C.snd_rate_of(rate))
        chans = [C.Channel(P, k, SCRIPTS[n]) for k, n in enumerate(names)]
        by = configure_bystander(P, 4, rate)
        chk = [Checker(ctx, n, r, "batch") for n, r in zip(names, recs)]
        ip, pos, sam_mix = [0] * nn, 0, 0
        for call, n in enumerate(lens):
            blk = []
            for k in range(nn):                          # every channel's commands up to its next block
                while steps[k][ip[k]][0] == "cmd":
                    chans[k].cmd(steps[k][ip[k]][1])
                    ip[k] += 1
                blk.append(steps[k][ip[k]])
                ip[k] += 1
                assert blk[-1][1] == n
            order = [(call + k) % nn for k in range(nn)]
            fam = [chans[k].w.sam for k in order]
            sam_mix += any(fam) and not all(fam)
            s16, _, agc = P.process(order, np.stack([xs[k][pos:pos + n] for k in order]))
            pos += n
            for row, k in enumerate(order):
                chk[k].call(P, k, blk[k], s16[row], agc[row])
        for k in range(nn):
            assert all(s[0] == "cmd" for s in steps[k][ip[k]:])
            chk[k].end(chans[k])
        assert bystander_state(P, by, 4) == want4, (names, "the channel that was never listed changed")
        assert sam_mix >= want_sam_mix, (names, "calls that mixed SAM-family and other channels", sam_mix)
    finally:
        P.close()


@pytest.mark.parametrize("group", range(C.NSEED // C.GROUP))
def test_group_of_four_as_one_batch(gpu_ctx, group):
    rate, ragged, lens = C.group_of(group * C.GROUP)
    run_batch(gpu_ctx, ["r%02d" % (group * C.GROUP + k) for k in range(C.GROUP)], rate, lens, 1)


def test_stereo_channel_beside_one_that_runs_wild_and_spectral(gpu_ctx):
    """pb has Wild and spectral NR on and spends four blocks in SAS while pa, in the same launches, runs both: the kernels are
    launched for the batch and must leave the stereo channel's states alone"""
    lens = C.blocks_of(SCRIPTS["pa"])
    assert lens == C.blocks_of(SCRIPTS["pb"]) and record("pb").blocks[6]["mode"] == C.M_SAS and record("pa").blocks[6]["stages"] == ("wild", "spectral")
    run_batch(gpu_ctx, list(C.PAIR), C.PAIR_RATE, lens, 4)
