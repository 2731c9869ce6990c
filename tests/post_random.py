"""Seeded random command scripts for the whole audio post path kg_post (tests/test_post_rand_{cpu,gpu}.py,
tools/make_ref_post_golden.py --random): S-meter and CAgc, the AM / NBFM / SSB / IQ detectors, the five synchronous-AM modes, the
CFir tails, the squelch and de-emphasis, the Wild noise blanker and the NR switch (ANR, CLMS, spectral), as c2s_sound() runs them
one behind the other (rx/rx_sound.cpp:676-949).  Each stage has its own golden and its own hand-written scenarios; these scripts draw
the combinations nobody wrote down -- a mode change with ANR left on across a stereo stretch, `SET nr algo=` WDSP -> spectral -> WDSP,
Wild re-initialised between two blocks, de-emphasis toggled under a SAM mode, the AGC switched off and on -- and a fixed list of
named scripts (SHAPES) walks the AGC window maximum, which is the kernel's own algorithm, over the window widths where a doubling
prefix maximum can go wrong.

post_script(seed) is a pure function of the seed and answers a script in tools/ref/ref_post_main.cpp's language (ref_sam_main.cpp's
lines, `nbA / nbE / nbP`, `nrA / nrE / nrP / nrM`, and two comment lines the harness skips and script_input() reads: `#I off`, the
next blocks' samples start at pool offset off and wrap inside that segment; `#K d`, the sample d before the next block's last one
is an isolated full-scale peak).  It draws from the domain on which the harness exits 0 and the library refuses nothing.  Seeds come
in groups of four that share the rate and the list of block lengths and draw their own commands, so a group can run as one batch.
What the reference wrote is kept in tests/golden/post_rand_ref.npz: integers in full, sample streams by digest (pack / RECORD).
features() walks a script beside its record and names what it reached (CONDITIONS)."""
import os

import numpy as np

from .script_common import digest, digest_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GOLDEN = "post_rand_ref.npz"
NSEED = 40
GROUP = 4
BASE = 0x504F0800                                # the first base whose 40 seeds reach every condition (profiles/post_random.txt)
PARTITION = 0x50415254                           # added to the base for the generator of a script's split into calls
BLK = 512
RATES = (12000, 20250)
RAGGED = (1, 2, 7, 63, 64, 65, 170, 301, 511, 512)
SPLIT = (1, 7, 64, 170)
MAX_CALL = 1024                                  # KG_POST_MAX_SAMPLES

# rx/mode.h:69-70
M_AM, M_USB, M_NBFM, M_IQ, M_SAM, M_SAU, M_SAL, M_SAS, M_QAM = 0, 2, 6, 7, 11, 12, 13, 14, 15
MODES = (M_AM, M_USB, M_NBFM, M_IQ, M_SAM, M_SAU, M_SAL, M_SAS, M_QAM)
MODE_NAMES = {M_AM: "AM", M_USB: "SSB", M_NBFM: "NBFM", M_IQ: "IQ", M_SAM: "SAM", M_SAU: "SAU", M_SAL: "SAL", M_SAS: "SAS", M_QAM: "QAM"}
SAM_FAMILY = (M_SAM, M_SAU, M_SAL, M_SAS, M_QAM)
STEREO = (M_IQ, M_SAS, M_QAM)                    # IS_STEREO (rx/mode.h:45-55)
NR_WDSP, NR_ORIG, NR_SPECTRAL = 1, 2, 3
NB_WILD = 2
S_METER_CAL = np.float32(-13)


# --------------------------------------------------------------------------------------------------------------------- the pool
SEGMENTS = ("am", "nbfm", "tone", "burst", "clicks", "silence", "full")
SEG = 16 * BLK
AT = {s: i * SEG for i, s in enumerate(SEGMENTS)}
POOL_SEED = 0x504F5301
POOL_RATE = 12000.0
PEAK = 32767


def _i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def pool():
    """int16 [7 * SEG, 2]: whole-number I/Q pairs, a valid CFastFIR output.  One generator, drawn in a fixed order; the golden file
    holds the pool's digest."""
    rng = np.random.Generator(np.random.PCG64(POOL_SEED))
    t = np.arange(SEG) / POOL_RATE
    noise = lambda a: a * (rng.standard_normal(SEG) + 1j * rng.standard_normal(SEG))
    out = {}
    # an AM station: the carrier 31 Hz off tune and drifting, other audio on the lower than on the upper sideband, fading
    car = 2 * np.pi * (31.0 * t + 0.5 * 2.5 * t * t) + 0.7
    fade_c = 1.0 - 0.25 * (1 + np.sin(2 * np.pi * 0.8 * t))
    fade_s = 1.0 - 0.25 * (1 + np.cos(2 * np.pi * 1.3 * t))
    side = 0.35 * np.exp(2j * np.pi * 700.0 * t) + 0.2 * np.exp(2j * np.pi * 1900.0 * t) + 0.3 * np.exp(-2j * np.pi * 1250.0 * t)
    out["am"] = 6000.0 * np.exp(1j * car) * (fade_c + fade_s * side) + noise(25.0)
    # NBFM: 2.5 kHz deviation by a 700 Hz tone, with gaps in which only noise is left
    ph = 2 * np.pi * np.cumsum(2500.0 * np.sin(2 * np.pi * 700.0 * t)) / POOL_RATE
    on = np.ones(SEG)
    for b in (3, 4, 5, 9, 10, 13):
        on[b * BLK:(b + 1) * BLK] = 0.0
    out["nbfm"] = 5000.0 * on * np.exp(1j * ph) + noise(60.0)
    # tones in noise
    out["tone"] = 3000.0 * np.exp(2j * np.pi * 1000.0 * t) + 2500.0 * np.exp(1j * (2 * np.pi * 500.0 * t + 0.3)) + noise(400.0)
    # speech-like bursts in noise: a gated harmonic series with a moving pitch
    f0 = 140.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)
    hp = 2 * np.pi * np.cumsum(f0) / POOL_RATE
    gate = 0.5 * (1 + np.sin(2 * np.pi * 3.1 * t)) ** 2
    out["burst"] = gate * (3000.0 * np.exp(1j * hp) + 1800.0 * np.exp(1j * (3 * hp + 0.4)) + 900.0 * np.exp(1j * (5 * hp + 1.1))) + noise(400.0)
    # tones on a low floor with clicks of one to three samples
    x = 2500.0 * np.exp(2j * np.pi * 500.0 * t) + 2000.0 * np.exp(1j * (2 * np.pi * 1000.0 * t + 0.3)) + noise(60.0)
    for b in range(SEG // BLK):
        if rng.random() < 0.6:
            for _ in range(int(rng.integers(1, 4))):
                p = b * BLK + int(rng.integers(0, BLK - 3))
                w = int(rng.integers(1, 4))
                x[p:p + w] += rng.choice([-1.0, 1.0]) * rng.uniform(9000, 16000) * (1 + 0.5j)
    out["clicks"] = x
    out["silence"] = np.zeros(SEG, complex)
    sq = lambda v: np.where(v >= 0, 1.0, -1.0)
    out["full"] = PEAK * (sq(np.sin(2 * np.pi * 450.0 * t)) + 1j * sq(np.cos(2 * np.pi * 450.0 * t)))
    return np.concatenate([np.stack([_i16(out[s].real), _i16(out[s].imag)], axis=1) for s in SEGMENTS])


def blocks_of(lines):
    """the block lengths of a script, in order"""
    return [int(v) for l in lines if l[0] == "P" for v in l.split()[1:]]


def script_input(lines, samples):
    """-> int16 [n, 2]: what the script's `#I` / `#K` lines and blocks take from the pool"""
    out, peaks, pos, base, at = [], [], None, 0, 0
    pend = []
    for l in lines:
        f = l.split()
        if f[0] == "#I":
            base = int(f[1]) // SEG * SEG
            pos = int(f[1]) - base
        elif f[0] == "#K":
            pend.append(int(f[1]))
        elif f[0] == "P":
            for n in (int(v) for v in f[1:]):
                assert pos is not None, "a block ahead of the first #I"
                out.append(samples[base + (pos + np.arange(n)) % SEG])
                pos = (pos + n) % SEG
                at += n
                peaks += [at - 1 - d for d in pend]
                pend = []
    x = np.concatenate(out).copy()
    for p in peaks:
        assert 0 <= p < len(x), "a peak ahead of the stream"
        x[p] = (PEAK, -PEAK)
    return x


def as_complex(x):
    return np.ascontiguousarray(x, np.int16).astype(np.float32).view(np.complex64).reshape(-1)


# --------------------------------------------------------------------------------------------------------------- the generators
def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def r_line(rate):
    fw_sel, nrx, adc = (2, 226, 66.6666e6) if abs(rate - 20250.0) < 1 else (0, 170, 66.6666e6)
    return "R %r %d %d %d %r" % (float(rate), fw_sel, nrx, int(round(adc / rate)), adc)


PASSBANDS = ((300, 2700), (-2700, -300), (-4900, 4900), (-3000, 3000), (50, 3500), (-4000, 1200))     # inside every rate, NR_SPECTRAL's bins in range


def passband_lines(lo, hi, rate):
    """`SET mod= low_cut= high_cut=`: the m_AM_FIR design as kg_post_set_am_passband computes it (rx_sound_cmd.cpp:268-282) and the
    normalised passband (:252-266)"""
    hbw = np.float32(max(abs(hi), abs(lo)))
    stop = np.float32(float(hbw) * 1.8)
    if stop > rate / 2:
        stop = np.float32(rate / 2)
    return ["L %.9g %.9g" % (hbw, stop), "nrM %d %d" % (lo, hi)]


AGC_DECAYS = (20, 100, 500, 1000, 5000)
MPARAMS = (0, 4, 8, 12, 1, 2, 9, 14, 13, 10)
SQ_VALUES = (0, 10, 30, 50, 70, 90)
SQ_MAX = (0, 0, 3000, 8192, 20000)
WDSP_TAPS, WDSP_DLY = (16, 32, 64, 128), (1, 2, 3, 16, 64, 128)
WDSP_GAIN, WDSP_LEAK = ("1e-4", "2.048e-4", "1.28e-5", "8.192e-2", "1e-3", "4.096e-2"), ("0.1", "0.2", "8", "1e-3", "0.4")
NR_TOUR = (NR_WDSP, NR_SPECTRAL, NR_WDSP, NR_ORIG)
ORIG_DELAY, ORIG_BETA, ORIG_DECAY = ("0", "1", "17", "300", "1000", "0.5"), ("0", "0.1", "0.01", "0.05"), ("0", "0.999", "0.97")


def _agc(rng, on=None):
    on = int(rng.random() < 0.75) if on is None else on
    return "A %d %d %d %d %d %d" % (on, int(rng.integers(2)), int(rng.integers(-130, -19)), int(rng.integers(0, 91)), int(rng.integers(0, 11)),
                                    _pick(rng, AGC_DECAYS))


def _nr_value(rng, algo, k):
    if algo == NR_WDSP:
        return [str(_pick(rng, WDSP_TAPS)), str(_pick(rng, WDSP_DLY)), _pick(rng, WDSP_GAIN), _pick(rng, WDSP_LEAK)][k]
    if algo == NR_ORIG:
        return [_pick(rng, ORIG_DELAY), _pick(rng, ORIG_BETA), _pick(rng, ORIG_DECAY)][k]
    return ["%.9g" % 10 ** (rng.uniform(-30, 30) / 20), "%.9g" % rng.uniform(0.9, 0.99), "%.9g" % 10 ** (rng.uniform(2, 30) / 10)][k]


def _nb_value(rng, k):
    return ["%.9g" % 10 ** rng.uniform(-0.3, 0.8), "%d" % rng.integers(1, 41), "%d" % rng.integers(2, 42)][k]


class _Draw:
    """the command state a generator keeps to stay inside the domain (what the server's snd_t holds)"""

    def __init__(self, rng, rate, ragged):
        self.rng, self.rate, self.ragged = rng, rate, ragged
        self.mode = M_USB
        self.nb_algo, self.nb_on, self.nb_sent = 0, 0, False
        self.nr_algo, self.nr_owner = 0, [0, 0]          # whose parameters each type's vector holds
        self.tour = 0

    def nr_params(self, t):
        n = 4 if self.nr_algo == NR_WDSP else 3
        self.nr_owner[t] = self.nr_algo
        return ["nrP %d %d %s" % (t, k, _nr_value(self.rng, self.nr_algo, k)) for k in range(n)]

    def nb_three(self):
        self.nb_sent = True
        return ["nbP 0 %d %s" % (k, _nb_value(self.rng, k)) for k in range(3)]

    def command(self):
        rng = self.rng
        r = rng.random()
        if r < 0.22:
            self.mode = _pick(rng, MODES)
            l = ["M %d" % self.mode]
            if self.mode == M_NBFM and rng.random() < 0.6:       # a squelch that can close, and a signal with gaps to close it on
                l += ["Q %d %d" % (_pick(rng, SQ_VALUES[1:]), _pick(rng, SQ_MAX)), "#I %d" % (AT["nbfm"] + int(rng.integers(SEG)))]
            return l
        if r < 0.32:
            return [_agc(rng)]
        if r < 0.40:
            return ["N %d" % _pick(rng, MPARAMS)]
        if r < 0.45:
            return ["G %d" % _pick(rng, (-1, 0, 1, 2))]
        if r < 0.55:
            return ["E %d %d" % (int(rng.integers(3)), int(rng.integers(3)))]
        if r < 0.62:
            return ["Q %d %d" % (_pick(rng, SQ_VALUES), _pick(rng, SQ_MAX))]
        if r < 0.67:
            return passband_lines(*_pick(rng, PASSBANDS), self.rate)
        if r < 0.80 and not self.ragged:
            return self.nb_command()
        return self.nr_command()

    def nb_command(self):
        rng = self.rng
        r = rng.random()
        if r < 0.35 or self.nb_algo != NB_WILD:
            self.nb_algo = NB_WILD if rng.random() < 0.8 else int(rng.integers(2))
            self.nb_on = 0
            l = ["nbA %d" % self.nb_algo]
            if self.nb_algo == NB_WILD:
                if not self.nb_sent or rng.random() < 0.5:
                    l += self.nb_three()
                l.append("nbE 0 1")
                self.nb_on = 1
            return l
        if r < 0.75:                                     # one message: nb_Wild_init from the whole stored vector, in mid-stream
            l = [] if self.nb_sent else self.nb_three()
            k = int(rng.integers(3))
            return l + ["nbP 0 %d %s" % (k, _nb_value(rng, k))]
        self.nb_on ^= 1
        return ([] if self.nb_sent or not self.nb_on else self.nb_three()) + ["nbE 0 %d" % self.nb_on]

    def nr_command(self):
        rng = self.rng
        r = rng.random()
        if r < 0.45 or self.nr_algo == 0:
            algos = (0, NR_WDSP, NR_WDSP, NR_ORIG) if self.ragged else (0, NR_WDSP, NR_WDSP, NR_ORIG, NR_SPECTRAL, NR_SPECTRAL)
            if not self.ragged and rng.random() < 0.5:           # the tour WDSP -> spectral -> WDSP -> CLMS, from wherever it stands
                self.nr_algo = NR_TOUR[self.tour % len(NR_TOUR)]
                self.tour += 1
            else:
                self.nr_algo = _pick(rng, algos)
            l = ["nrA %d" % self.nr_algo]
            if self.nr_algo == NR_SPECTRAL:
                if self.nr_owner[0] != NR_SPECTRAL or rng.random() < 0.4:
                    l += self.nr_params(0)
            elif self.nr_algo:
                for t in (0, 1):
                    if self.nr_owner[t] != self.nr_algo or rng.random() < 0.4:
                        l += self.nr_params(t)
                en = _pick(rng, ((1, 0), (0, 1), (1, 1), (1, 0), (0, 1)))
                l += ["nrE %d 1" % t for t in (0, 1) if en[t]]
            return l
        t = 0 if self.nr_algo == NR_SPECTRAL else int(rng.integers(2))
        if r < 0.75:
            if self.nr_owner[t] != self.nr_algo:
                return self.nr_params(t)
            k = int(rng.integers(4 if self.nr_algo == NR_WDSP else 3))
            return ["nrP %d %d %s" % (t, k, _nr_value(rng, self.nr_algo, k))]
        return ["nrE %d %d" % (int(rng.integers(2)), int(rng.integers(2)))]

    def source(self):
        rng = self.rng
        if rng.random() < 0.6:
            seg = "am" if self.mode in SAM_FAMILY or self.mode == M_AM else "nbfm" if self.mode == M_NBFM else _pick(rng, ("tone", "burst", "clicks"))
        else:
            seg = _pick(rng, SEGMENTS)
        return "#I %d" % (AT[seg] + int(rng.integers(SEG)))


def group_of(seed):
    """-> (rate, ragged?, block lengths): what the four seeds of a group share"""
    g = seed // GROUP
    rng = np.random.default_rng(BASE + 0x10000 + g)
    ragged = bool(g & 1)
    rate = RATES[(g >> 1) & 1]
    if ragged:
        lens = [int(_pick(rng, RAGGED)) for _ in range(int(rng.integers(12, 25)))]
    else:
        lens = [BLK] * int(rng.integers(12, 23))
    return rate, ragged, lens


def post_script(seed):
    rate, ragged, lens = group_of(seed)
    rng = np.random.default_rng(BASE + seed)
    d = _Draw(rng, rate, ragged)
    lines = [r_line(rate)] + passband_lines(*_pick(rng, PASSBANDS), rate) + [_agc(rng, 1)]
    d.mode = _pick(rng, MODES)
    lines.append("M %d" % d.mode)
    for _ in range(int(rng.integers(0, 4))):
        lines += d.command()
    lines.append(d.source())
    for n in lens:
        for _ in range(int(rng.integers(3))):
            lines += d.command()
        if rng.random() < 0.2:
            lines.append(d.source())
        lines.append("P %d" % n)
    return lines


# ---- the AGC window edges ----
AGC_WINDOW, AGC_DELAY = .018, .015               # WINDOW_TIMECONST, DELAY_TIMECONST (rx/CuteSDR/agc.cpp)
# (W = 1 at 105 Hz, not at 100: CAgc's constructor sets m_SampleRate = 100.0, so a first SetParameters at exactly 100 Hz never sets the
# buffers and averagers (agc.cpp:85, :117) and the reference runs on members it never wrote)
SHAPE_RATES = {1: 105.0, 2: 120.0, 3: 170.0, 4: 230.0, 255: 14200.0, 256: 14250.0, 257: 14300.0, 511: 28400.0, 512: 28450.0, 513: 28520.0,
               2047: 113750.0}
POST_CIRC = 4096


SHAPES = tuple("w%d" % w for w in sorted(SHAPE_RATES))    # the fixed, named list behind the seeds; they count towards no condition


def shape_names():
    return list(SHAPES)


def shape_wd(name):
    """-> (rate, W, D) as the arithmetic gives them; the tests assert them through the harness's echo and agc_delay()"""
    w = int(name[1:])
    rate = SHAPE_RATES[w]
    return rate, int(np.float32(rate) * AGC_WINDOW), int(np.float32(rate) * AGC_DELAY)


def shape_script(name):
    """SSB with the hang timer off, then IQ with it on: blocks of W-1, W, W+1, D, D+1 and 1 (clipped to 1..512), then 512s until the
    window and the delay ring have wrapped twice (for W = 2047, until the sample count has passed the kernel's history ring twice),
    the last three of them with an isolated peak W-1, W and W+1 samples ahead of their end"""
    rate, W, D = shape_wd(name)
    edge = [min(max(v, 1), BLK) for v in (W - 1, W, W + 1, D, D + 1, 1)]
    need = 2 * POST_CIRC + 1 if W == 2047 else 2 * max(W, D) + W + 2
    full = max(3, -(-max(need - sum(edge), 0) // BLK))
    lines = [r_line(rate)]
    for k, (mode, hang) in enumerate(((M_USB, 0), (M_IQ, 1))):
        lines += ["A 1 %d -100 50 6 %d" % (hang, 500 if hang else 1000), "M %d" % mode, "#I %d" % (AT["burst"] + 700 + 4000 * k)]
        lines += ["P %d" % n for n in edge]
        for i in range(full):
            if i >= full - 3:
                lines.append("#K %d" % (W - 1 + i - (full - 3)))
            lines.append("P %d" % BLK)
    return lines


# ---- a stereo channel beside a channel that runs the stages ----
PAIR = ("pa", "pb")                              # one batch: both have Wild and spectral NR on; pb goes mono -> SAS -> mono meanwhile
PAIR_RATE, PAIR_BLOCKS = 12000, 14


def pair_script(name):
    """The Wild and spectral kernels are launched for a whole batch when one channel runs them, and a stereo channel that has them
    switched on must return at once: alone it never meets them (no launch), and no group of seeds puts a stereo channel with spectral
    NR selected beside one that runs it.  pa runs both stages on every block; pb has both on and spends blocks 5..8 in SAS."""
    lines = [r_line(PAIR_RATE)] + passband_lines(300, 2700, PAIR_RATE) + [
        "A 1 0 -100 50 6 1000", "M %d" % M_USB, "nbA 2", "nbP 0 0 3", "nbP 0 1 10", "nbP 0 2 7", "nbE 0 1",
        "nrA 3", "nrP 0 0 1", "nrP 0 1 0.95", "nrP 0 2 1000", "#I %d" % (AT["clicks"] + (0 if name == "pa" else 3 * BLK))]
    for k in range(PAIR_BLOCKS):
        if name == "pb" and k in (5, 9):
            lines.append("M %d" % (M_SAS if k == 5 else M_USB))
        lines.append("P %d" % BLK)
    return lines


def all_scripts():
    """name -> script: the seeds (r00 ..), the shapes (w1 ..) and the pair (pa, pb)"""
    out = {"r%02d" % s: post_script(s) for s in range(NSEED)}
    out.update({n: shape_script(n) for n in shape_names()})
    out.update({n: pair_script(n) for n in PAIR})
    return out


FULL = ("w1", "w2")                              # the short scripts whose streams the golden keeps in full


# ------------------------------------------------------------------------------------------------ walking a script: what runs where
class Walk:
    """The command state of snd_t beside a script: feed it every line; at a block it knows the mode and which stages run."""

    def __init__(self):
        self.mode, self.agc_on, self.de, self.de_nfm = M_USB, 1, 0, 0
        self.nb_algo, self.nb_en = 0, 0
        self.nr_algo, self.nr_en = 0, [0, 0]

    def line(self, l):
        f = l.split()
        if f[0] == "M":
            self.mode = int(f[1])
        elif f[0] == "A":
            self.agc_on = int(f[1])
        elif f[0] == "E":
            self.de, self.de_nfm = int(f[1]), int(f[2])
        elif f[0] == "nbA":
            self.nb_algo, self.nb_en = int(f[1]), 0
        elif f[0] == "nbE" and int(f[1]) == 0:
            self.nb_en = int(f[2])
        elif f[0] == "nrA":
            self.nr_algo, self.nr_en = int(f[1]), [0, 0]
        elif f[0] == "nrE":
            self.nr_en[int(f[1])] = int(f[2])

    @property
    def stereo(self):
        return self.mode in STEREO

    @property
    def sam(self):
        return self.mode in SAM_FAMILY

    def stages(self):
        """the stages of rx_sound.cpp:922-949 that run on a block now"""
        if self.stereo:
            return ()
        out = ["wild"] if self.nb_en and self.nb_algo == NB_WILD else []
        if self.nr_algo == NR_WDSP:
            out += [n for t, n in ((1, "anr_an"), (0, "anr_dn")) if self.nr_en[t]]
        elif self.nr_algo == NR_ORIG:
            out += ["clms"] if self.nr_en[0] or self.nr_en[1] else []
        elif self.nr_algo == NR_SPECTRAL:
            out.append("spectral")
        return tuple(out)


def steps_of(lines):
    """a script as steps: ("cmd", line) and ("blk", n, [recorded block numbers], [their lengths])"""
    steps, k = [], 0
    for l in lines[1:]:
        if l[0] == "#":
            continue
        if l[0] == "P":
            for n in (int(v) for v in l.split()[1:]):
                steps.append(("blk", n, [k], [n]))
                k += 1
        else:
            steps.append(("cmd", l))
    return steps


def per_call(rec):
    """the blocks whose bytes the REFERENCE makes depend on where a call ends: NBFM, whose squelch compares its average and gates the
    samples once per call (rx/CuteSDR/squelch.cpp:172-218).  The other partitions leave them as recorded.  (wdsp_SAM_carrier and the
    S-meter taps are per call as well -- SAM_demod.cpp:341-344, rx_sound.cpp:693 -- and no stream depends on them.)"""
    return {k for k, b in enumerate(rec.blocks) if b["mode"] == M_NBFM}


def merged(steps, fixed=()):
    """consecutive blocks with no command between them joined while the sum stays inside one call"""
    out = []
    for s in steps:
        if (s[0] == "blk" and out and out[-1][0] == "blk" and out[-1][1] + s[1] <= MAX_CALL and s[2][0] not in fixed
                and out[-1][2][-1] not in fixed):
            out[-1] = ("blk", out[-1][1] + s[1], out[-1][2] + s[2], out[-1][3] + s[3])
        else:
            out.append(s)
    return out


def split(steps, seed, fixed=()):
    """every block cut into pieces drawn from SPLIT: a block's number and length stand on its last piece, ("blk", piece, [k], [n]);
    the pieces ahead of it are ("blk", piece, [], [])"""
    rng = np.random.default_rng(BASE + PARTITION + seed)
    out = []
    for s in steps:
        if s[0] != "blk" or s[2][0] in fixed:
            out.append(s)
            continue
        left = s[1]
        while left:
            n = min(left, int(_pick(rng, SPLIT)))
            left -= n
            out.append(("blk", n, s[2], s[3]) if not left else ("blk", n, [], []))
    return out


# ------------------------------------------------------------------------------------------------------------------ the record
def fdigest(a):
    """SHA-256 prefix of a float32 vector with every NaN as 0x7FC00000 (x86's default NaN is the negative quiet one, the GPU's the
    positive one)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).copy().reshape(-1)
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return digest(u.tobytes())


NR_REC = 6 * 4 + 2 * 4 + 512 * 4 + 121 * 4
NBW_REC = 4 * 4 + 4 + 120 * 4
NRS_REC = 2 * 4 + 12 * 4 + 9 * 256 * 4
ST_SIZE = 3 * 4 + 2 * NR_REC + NBW_REC + NRS_REC


def nr_digest(anr_f, anr_w, lms_coef):
    return fdigest(np.concatenate([np.ravel(anr_f), np.ravel(anr_w), np.ravel(lms_coef)]))


def nbw_digest(thresh, hist):
    return fdigest(np.concatenate([[np.float32(thresh)], np.ravel(hist)]))


def nrs_digest(first_time, scalars5, rate5, norm2, arrays):
    """final_gain, alpha, asnr, xih1r, pfac; tinc .. ap (the reference computes them at the first init: zeroed here before it);
    norm_locut, norm_hicut; the nine arrays"""
    rate5 = np.asarray(rate5, np.float32) if first_time else np.zeros(5, np.float32)
    return fdigest(np.concatenate([np.ravel(scalars5), rate5, np.ravel(norm2), np.ravel(arrays)]))


def pack(lines, out_bin, st_bin, full=False):
    """the harness's two files -> the arrays the golden keeps for one script"""
    w = Walk()
    raw, pos = bytes(out_bin), 0
    rec, hits, chg, pre_sha, s16_sha, agc_sha, pre_full, s16_full, agc_full = [], [], [], [], [], [], [], [], []
    for l in lines[1:]:
        if l[0] != "P":
            w.line(l)
            continue
        for n in (int(v) for v in l.split()[1:]):
            rec.append(np.frombuffer(raw[pos:pos + 28], np.float32)); pos += 28
            hits.append(int(np.frombuffer(raw[pos:pos + 4], np.int32)[0])); pos += 4
            if not w.stereo:
                pre = np.frombuffer(raw[pos:pos + 2 * n], np.int16); pos += 2 * n
                s16 = np.frombuffer(raw[pos:pos + 2 * n], np.int16); pos += 2 * n
                pre_sha.append(digest_u8(pre.tobytes()))
                chg.append(int(not np.array_equal(pre, s16)))
                if chg[-1]:
                    s16_sha.append(digest_u8(s16.tobytes()))
                pre_full.append(pre); s16_full.append(s16)
            if w.stereo or w.sam:
                agc = np.frombuffer(raw[pos:pos + 8 * n], np.float32); pos += 8 * n
                agc_sha.append(digest_u8(agc.tobytes()))
                agc_full.append(agc)
    assert pos == len(raw), (pos, len(raw))
    rec = np.array(rec, np.float32).reshape(-1, 7)
    assert np.array_equal(rec[:, 1], rec[:, 0] + S_METER_CAL)
    st = bytes(st_bin)
    assert len(st) == ST_SIZE, len(st)
    echo = np.frombuffer(st[:12], np.int32)
    o = {"smeter": rec[:, [0, 2, 3]].copy(), "carrier": rec[:, 5].copy(), "flags": (rec[:, 4].astype(np.int8) | (rec[:, 6].astype(np.int8) << 1)),
         "hits": np.array(hits, np.int16), "chg": np.array(chg, np.int8),
         "pre_sha": np.array(pre_sha, np.uint8).reshape(-1, 16), "s16_sha": np.array(s16_sha, np.uint8).reshape(-1, 16),
         "agc_sha": np.array(agc_sha, np.uint8).reshape(-1, 16), "wd": echo[:2].copy()}
    assert echo[2] == 0, "the reference indexed outside its arrays %d times" % echo[2]
    p = 12
    nr_i, sha = [], []
    for t in range(2):
        r = st[p:p + NR_REC]; p += NR_REC
        nr_i.append(np.frombuffer(r[:24], np.int32))
        sha.append(nr_digest(np.frombuffer(r[24:32], np.float32), np.frombuffer(r[32:32 + 2048], np.float32), np.frombuffer(r[32 + 2048:], np.float32)))
    r = st[p:p + NBW_REC]; p += NBW_REC
    nbw_i = np.frombuffer(r[:16], np.int32)
    sha.append(nbw_digest(np.frombuffer(r[16:20], np.float32)[0], np.frombuffer(r[20:], np.float32)))
    r = st[p:p + NRS_REC]
    nrs_i = np.frombuffer(r[:8], np.int32)
    fv = np.frombuffer(r[8:56], np.float32)
    sha.append(nrs_digest(int(nrs_i[0]), fv[:5], fv[5:10], fv[10:12], np.frombuffer(r[56:], np.float32)))
    o["state_i"] = np.concatenate([nr_i[0], nr_i[1], nbw_i, nrs_i]).astype(np.int32)
    o["state_sha"] = np.array([np.frombuffer(s, np.uint8) for s in sha], np.uint8)
    o["script_sha"] = digest_u8("\n".join(lines).encode())
    if full:                                             # (out_samps_s2 ahead of :922 only where a stage changed it)
        o["s16"] = np.concatenate(s16_full + [np.zeros(0, np.int16)])
        o["agc"] = np.concatenate(agc_full + [np.zeros(0, np.float32)])
        if any(chg):
            o["pre"] = np.concatenate(pre_full + [np.zeros(0, np.int16)])
    return o


def load():
    return np.load(os.path.join(GOLD, GOLDEN))


VAR_KEYS = ("smeter", "carrier", "flags", "hits", "chg", "pre_sha", "s16_sha", "agc_sha")      # one row per block (or per block that has it)
FIX_KEYS = ("script_sha", "wd", "state_i", "state_sha")                                          # one row per script
FULL_KEYS = ("pre", "s16", "agc")


def join(names, packed):
    """the arrays of pack() of every script -> the golden's: each key once, the scripts one behind the other, `<key>_n` rows each"""
    out = {"names": np.array(names)}
    for k in VAR_KEYS:
        out[k] = np.concatenate([packed[n][k] for n in names])
        out[k + "_n"] = np.array([len(packed[n][k]) for n in names], np.int32)
    for k in FIX_KEYS:
        out[k] = np.stack([packed[n][k] for n in names])
    for n in names:
        for k in FULL_KEYS:
            if k in packed[n]:
                out["full_%s_%s" % (n, k)] = packed[n][k]
    return out


def unjoin(g, name):
    """-> the arrays of pack() of one script"""
    names = [str(n) for n in g["names"]]
    i = names.index(name)
    o = {}
    for k in VAR_KEYS:
        at = int(g[k + "_n"][:i].sum())
        o[k] = g[k][at:at + int(g[k + "_n"][i])]
    for k in FIX_KEYS:
        o[k] = g[k][i]
    for k in FULL_KEYS:
        if "full_%s_%s" % (name, k) in g.files:
            o[k] = g["full_%s_%s" % (name, k)]
    return o


class Record:
    """one script's record (the arrays of pack()), block by block"""

    def __init__(self, o, name, lines):
        self.name, self.lines = name, lines
        self.smeter, self.carrier, self.flags, self.hits = o["smeter"], o["carrier"], o["flags"], o["hits"]
        self.wd, self.state_i, self.state_sha = o["wd"], o["state_i"], o["state_sha"]
        self.full = {v: o[v] for v in FULL_KEYS if v in o}
        chg, pre_sha, s16_sha, agc_sha = o["chg"], o["pre_sha"], o["s16_sha"], o["agc_sha"]
        w = Walk()
        self.blocks = []                                 # per block: dict n, mode, stages, agc_on, pre, s16, agc (digests or None), chg
        im = ic = ia = 0
        for l in lines[1:]:
            if l[0] != "P":
                w.line(l)
                continue
            for n in (int(v) for v in l.split()[1:]):
                b = dict(n=n, mode=w.mode, stages=w.stages(), agc_on=w.agc_on, de=w.de, de_nfm=w.de_nfm, pre=None, s16=None, agc=None, chg=0)
                if not w.stereo:
                    b["pre"] = bytes(pre_sha[im]); b["chg"] = int(chg[im]); im += 1
                    b["s16"] = b["pre"]
                    if b["chg"]:
                        b["s16"] = bytes(s16_sha[ic]); ic += 1
                if w.stereo or w.sam:
                    b["agc"] = bytes(agc_sha[ia]); ia += 1
                self.blocks.append(b)
        assert (im, ic, ia) == (len(pre_sha), len(s16_sha), len(agc_sha)) and len(self.blocks) == len(self.smeter), name

    def squelched(self, k):
        return int(self.flags[k]) & 1

    def chan_null(self, k):
        return (int(self.flags[k]) >> 1) & 1


# ------------------------------------------------------------------------------------------------------------------- FEATURES
CONDITIONS = (["mode_" + MODE_NAMES[m] for m in MODES]
              + ["sam_return", "nr_over_stereo", "wdsp_spectral_wdsp", "wild_hit", "wild_reinit", "spectral6", "agc_off_on", "deemp_under_sam",
                 "squelch_both", "null_both", "one_behind_mode", "chg_wild", "chg_anr_dn", "chg_anr_an", "chg_clms", "chg_spectral"])


def features(lines, rec):
    """what a script reached, from its lines and its record (the names of CONDITIONS)"""
    got = set()
    w = Walk()
    k = 0
    sam_phase = nr_phase = wsw = spectral_run = 0
    agc_was_off = wild_ran = reinit_pending = False
    mode_changed = de_changed_in = False
    sq_seen, last_null, null_up, null_down = set(), None, False, False
    sam_mono_before_de = False
    for l in lines[1:]:
        f = l.split()
        if l[0] == "#":
            continue
        if f[0] != "P":
            if f[0] == "M" and int(f[1]) != w.mode:
                mode_changed = True
            if f[0] == "E" and w.mode in (M_SAM, M_SAU, M_SAL) and int(f[1]) != w.de and sam_mono_before_de:
                de_changed_in = True
            if f[0] == "nbP" and int(f[1]) == 0 and w.nb_algo == NB_WILD and wild_ran:
                reinit_pending = True
            if f[0] in ("nrP", "nrA", "nrE"):
                nr_phase = 0                             # a re-init or another switch inside the stretch: not the state carried across
            w.line(l)
            continue
        for n in (int(v) for v in f[1:]):
            b = rec.blocks[k]
            st = b["stages"]
            got.add("mode_" + MODE_NAMES[w.mode])
            # SAM-family -> non-SAM -> SAM-family
            if w.sam:
                if sam_phase == 2:
                    got.add("sam_return")
                sam_phase = 1
            elif sam_phase:
                sam_phase = 2
            # mono -> stereo -> mono with ANR or CLMS enabled throughout
            lms_on = w.nr_algo in (NR_WDSP, NR_ORIG) and (w.nr_en[0] or w.nr_en[1])
            if not lms_on:
                nr_phase = 0
            elif not w.stereo:
                if nr_phase == 2:
                    got.add("nr_over_stereo")
                nr_phase = 1
            elif nr_phase:
                nr_phase = 2
            # WDSP -> spectral -> WDSP
            if "anr_an" in st or "anr_dn" in st:
                if wsw == 2:
                    got.add("wdsp_spectral_wdsp")
                wsw = 1
            elif "spectral" in st and wsw:
                wsw = 2
            spectral_run = spectral_run + 1 if "spectral" in st else 0
            if spectral_run >= 6:
                got.add("spectral6")
            if "wild" in st:
                if rec.hits[k] > 0:
                    got.add("wild_hit")
                if reinit_pending:
                    got.add("wild_reinit")
                wild_ran, reinit_pending = True, False
            if not w.agc_on:
                agc_was_off = True
            elif agc_was_off:
                got.add("agc_off_on")
            if w.mode in (M_SAM, M_SAU, M_SAL):
                if de_changed_in:
                    got.add("deemp_under_sam")
                sam_mono_before_de = True
            else:
                sam_mono_before_de = False
            de_changed_in = False
            if w.mode == M_NBFM:
                sq_seen.add(rec.squelched(k))
                if sq_seen == {0, 1}:
                    got.add("squelch_both")
            if w.sam:
                cn = rec.chan_null(k)
                if last_null is not None and cn != last_null:
                    null_up |= cn == 1
                    null_down |= cn == 0
                last_null = cn
                if null_up and null_down:
                    got.add("null_both")
            else:
                last_null = None
            if mode_changed and n == 1:
                got.add("one_behind_mode")
            mode_changed = False
            if b["chg"] and len(st) == 1:
                got.add("chg_" + st[0])
            k += 1
    return got


def check_conditions(feats):
    """feats: the feature sets of the NSEED seeds -> the conditions reached by fewer than two seeds"""
    count = {c: sum(c in f for f in feats) for c in CONDITIONS}
    return count, [c for c in CONDITIONS if count[c] < 2]


# ------------------------------------------------------------------------------------- a script on a kg_post channel (GPU tests)
# rx/mode.h -> KG_POST_*
def kg_mode(post, mode):
    return {M_AM: post.MODE_AM, M_USB: post.MODE_SSB, M_NBFM: post.MODE_NBFM, M_IQ: post.MODE_IQ, M_SAM: post.MODE_SAM, M_SAU: post.MODE_SAU,
            M_SAL: post.MODE_SAL, M_SAS: post.MODE_SAS, M_QAM: post.MODE_QAM}[mode]


def snd_rate_of(rate):
    return 12000 if abs(rate - 12000.0) < abs(rate - 20250.0) else 20250


class Channel:
    """One script's commands on channel ch of P, with the command state of snd_t kept here as kg_rxbank keeps it (kg_post holds the
    stages' vectors and switches only).  stages=False leaves every `nb` / `nr` line out: the object whose s16 is out_samps_s2 ahead
    of rx_sound.cpp:922."""

    def __init__(self, P, ch, lines, stages=True, nominal=True):
        from flydog_sdr_gps_amd import post
        self.post, self.P, self.ch, self.stages = post, P, ch, stages
        self.w = Walk()
        self.rate = float(lines[0].split()[1])
        self.nb_param = np.zeros((4, 8), np.float32)
        P.sam_setup(ch, snd_rate_of(self.rate))          # wdsp_SAM_demod_init() at the server's snd_rate
        P.set_smeter(ch, self.rate); P.set_mode(ch, post.MODE_SSB); P.reset(ch)
        if nominal:                                      # (no CFir design at the shapes' rates; SSB and IQ need none)
            P.squelch_setup(ch, self.rate); P.squelch_set(ch, 0, 0)

    def cmd(self, l):
        P, ch, post, w = self.P, self.ch, self.post, self.w
        f = l.split()
        op = f[0]
        if op[:2] in ("nb", "nr") and not self.stages:
            return
        if op == "A":
            P.set_agc(ch, *[int(v) for v in f[1:7]], self.rate)
        elif op == "L":
            P.cfir_init_lp(ch, post.CFIR_AM, 0, 1.0, 50.0, float(f[1]), float(f[2]), self.rate)
        elif op == "Q":
            P.squelch_set(ch, int(f[1]), int(f[2]))
        elif op == "E":
            r12k = snd_rate_of(self.rate) == 12000
            P.set_de_emp(ch, int(f[1]), 0, snd_rate_12k=r12k, frate=self.rate)
            P.set_de_emp(ch, int(f[2]), 1, snd_rate_12k=r12k, frate=self.rate)
        elif op == "M":
            P.set_mode(ch, kg_mode(post, int(f[1])))
        elif op == "G":
            P.sam_pll(ch, int(f[1]))
        elif op == "N":
            P.set_sam_mparam(ch, int(f[1]))
        elif op == "nbA":
            P.set_nbw(ch, 0)
        elif op == "nbE":
            if int(f[1]) == 0 and w.nb_algo == NB_WILD:
                P.set_nbw(ch, int(f[2]))
        elif op == "nbP":
            t, p = int(f[1]), int(f[2])
            v = self.nb_param[t].copy()
            v[p] = np.float32(f[3])
            if t == 0 and w.nb_algo == NB_WILD:
                P.nbw_init(ch, v)
            self.nb_param[t] = v
        elif op == "nrA":
            if int(f[1]) == NR_SPECTRAL:
                P.nrs_select(ch)
            else:
                P.set_nr_algo(ch, int(f[1]))
        elif op == "nrE":
            P.set_nr_enable(ch, int(f[1]), int(f[2]))
        elif op == "nrP":
            P.set_nr_param(ch, int(f[1]), int(f[2]), np.float32(f[3]))
        elif op == "nrM":
            P.nrs_passband(ch, float(f[1]), float(f[2]))
        else:
            raise AssertionError(l)
        w.line(l)

    def end_state(self):
        """-> (int32[22], four digests) as pack() keeps them"""
        P, ch = self.P, self.ch
        ints, sha = [], []
        for t in range(2):
            st = P.nr_state([ch], t, weights=True)
            ints += [st["anr_i"][0], st["lms_i"][0]]
            sha.append(nr_digest(st["anr_f"][0], st["anr_w"][0], st["lms_coef"][0]))
        st = P.nbw_state([ch])
        ints.append(st["ints"][0, :2])
        sha.append(nbw_digest(st["thresh"][0], st["hist"][0]))
        st = P.nrs_state([ch])
        ints.append(st["ints"][0, :2])
        sc = st["scalars"][0]
        sha.append(nrs_digest(int(st["ints"][0, 0]), [sc[0], sc[1], sc[2], sc[4], sc[5]], st["rate"][:5], sc[6:8], st["arrays"][0]))
        return np.concatenate(ints).astype(np.int32), sha


STATE_NAMES = ("ANR / CLMS denoise", "ANR / CLMS autonotch", "Wild", "spectral")


def state_ints(rec):
    """the golden's 22 end-state integers as Channel.end_state orders them: per NR type in_idx, taps, delay, dlp, dlen, nr_type; Wild's
    taps, impulse_samples; spectral's first_time, init_counter"""
    i = rec.state_i
    return np.concatenate([i[0:6], i[6:12], i[12:14], i[16:18]]).astype(np.int32)
