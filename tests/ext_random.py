"""Seeded random command scripts for the five extension modules kg_iqd, kg_lorc, kg_fftext, kg_fax and kg_cw
(tests/test_{iqd,lorc,fftext,fax,cw}_{cpu,gpu}.py, tools/make_ref_{iqd,lorc,fftext,fax,cw}_golden.py --random): the hand-written scripts
of the five *_common.py pin one case each; these draw the combinations nobody wrote down -- a command of one kind behind one of another
in mid-lap, points changed while both instances alternate, a GRI behind a stop / start, a function change behind a rate change behind
a clear, a fax line of 1024 or 10 samples at half the nominal rate, 300 sound blocks of Morse in one push.

A generator is a pure function of an integer seed and answers a script in its module's own script language over the module's own
seeded pool; it draws from the domain on which the reference harness and the host model take every script (exit status 0).  What the
reference wrote for seeds 0 .. NSEED-1 is kept in tests/golden/{iqd,lorc,fftext,fax,cw}_rand_ref.npz: integers in full, bytes by
digest (RECORD / pack / unpack).  FEATURES walks a script beside its record and names what it reached: the conditions of
test_random_fixture_meets_its_conditions.  fax and cw keep, behind the 40 seeds, the records of a short fixed list of named shape
scripts (SHAPES): the kernel-shape edges held whatever the seeds draw; they count towards no condition.  tests/ext_random_dev.py runs
the scripts on the device."""
import os
import shutil

import numpy as np

from . import cw_common as cwc
from . import fax_common as fxc
from . import fftext_common as fc
from . import iqd_common as ic
from . import lorc_common as lc

NSEED = 40
BASE = {"iqd": 0x49510400, "lorc": 0x4C4F0400, "fftext": 0x46580000, "fax": 0x46410700, "cw": 0x43570000}      # the first bases whose 40 seeds reach every condition (check_conditions)
PARTITION = 0x50415254                           # added to the base for the generator of a script's partition into calls
NS = (1, 7, 170, 511, 512)


def _rng(mod, seed, partition=False):
    return np.random.default_rng(BASE[mod] + seed + (PARTITION if partition else 0))


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _nblk(rng, ns):
    return int(rng.integers(1, 61 if ns <= 7 else 13))


# ---------------------------------------------------------------------------------------------------------------- the generators
IQD_RATES = (8000, 12000, 20250)
IQD_GAINS = (0, 38, 50, 52, 91, 100, -10)
IQD_POINTS = (1, 5, 100, 300, 511, 512, 513, 700, 1024, 4096, 16384)
IQD_EXPONENTS = (0, 1, 2, 3, 4, 5, 7, 8)         # none above 8: |s|^8 is where the power still fits (include/kiwigpu.h)
IQD_BAUDS = (50, 100, 200, -50)
IQD_BANDWIDTHS = ("0.5", "1", "5", "15", "20", "30", "100")


def _iqd_command(rng):
    k = int(rng.integers(8))
    if k == 0:
        return "G %d" % _pick(rng, IQD_GAINS)
    if k == 1:
        return "P %d" % _pick(rng, IQD_POINTS)
    if k == 2:
        m = int(rng.integers(4))
        return "M %d %d" % (m, _pick(rng, IQD_BAUDS) if m == 2 else _pick(rng, IQD_EXPONENTS))
    if k == 3:
        return "W %s" % _pick(rng, IQD_BANDWIDTHS)
    if k == 4:
        return "D %d" % int(rng.integers(3))
    if k == 5:
        return "Y %d" % int(rng.integers(2))
    if k == 6:
        return "C"
    return "R %d %d" % (int(rng.integers(2)), _pick(rng, IQD_RATES))


def iqd_script(seed):
    rng = _rng("iqd", seed)
    lines = ["N", "R 1 %d" % _pick(rng, IQD_RATES)]
    for _ in range(int(rng.integers(3, 9))):
        lines += [_iqd_command(rng) for _ in range(int(rng.integers(3)))]
        ns, seg = _pick(rng, NS), _pick(rng, ic.SEGMENTS)
        n = _nblk(rng, ns)
        room = (ic.MSK_BLOCKS * 512 if seg == "msk" else ic.SEG) // ns
        first = int(rng.integers(room - n + 1))
        both, one = rng.random() < 0.25, int(rng.random() < 0.125)
        lines += ["B %d %d %d" % ((k & 1) if both else one, ns, ic.AT[seg] + ns * (first + k)) for k in range(n)]
    return lines


LORC_RATES = ((12000, 600), (12000, 12000), (20250, 900), (12001.3, 700), (11998.7, 350))
LORC_PARAMS = {lc.CMA: (1, 1.5, 2, 2.5, 3, -2, 1000), lc.EMA: (0.5, 1, 1.49, 4, 8, 16.5), lc.IIR: (0, 1e-4, 5e-4, 3e-3, 0.05)}
LORC_OFFSETS = (-2000000000, -500, 37, 700, 2000000000)


def _lorc_gri(rng, srate):
    if rng.random() < 0.1:
        return int(rng.integers(8, 200))
    return int(rng.integers(3000, (9999 if srate == 20250 else 9980) + 1))


def _lorc_rule(rng, ch, algo):
    return ["A %d %d" % (ch, algo), "P %d %r" % (ch, float(_pick(rng, LORC_PARAMS[algo])))]


def _lorc_blocks(seg, first, n, ns=512):
    return ["B %d %d" % (ns, lc.AT[seg] + ns * (first + k)) for k in range(n)]


def _lorc_setup(rng, algo):
    """`N` and what both chains need ahead of a block; algo[ch] is left at the rule drawn"""
    srate, i_srate = _pick(rng, LORC_RATES)
    l = ["N %r %d" % (float(srate), i_srate)]
    for ch in range(2):
        algo[ch] = int(rng.integers(3))
        l += ["I %d %d" % (ch, _lorc_gri(rng, srate))] + _lorc_rule(rng, ch, algo[ch])
        if rng.random() < 0.5:
            l.append("G %d %d" % (ch, int(rng.integers(-40, 41))))
        if rng.random() < 0.5:
            l.append("O %d %d" % (ch, int(rng.integers(-3000, 3001))))
    return l, srate


def lorc_script(seed):
    rng = _rng("lorc", seed)
    algo = [0, 0]
    lines, srate = _lorc_setup(rng, algo)
    lines.append("S")
    nseg = int(rng.integers(3, 8))
    again = int(rng.integers(1, nseg)) if rng.random() < 0.3 else -1       # the gap that holds a second `N`
    for s in range(nseg):
        if s == again:
            l, srate = _lorc_setup(rng, algo)                              # no `S`: the registration outlives the memset
            lines += l
        elif s:
            k, ch = int(rng.integers(6)), int(rng.integers(2))
            if k == 0:
                lines.append("I %d %d" % (ch, _lorc_gri(rng, srate)))
            elif k == 1:
                lines.append("G %d %d" % (ch, int(rng.integers(-40, 41))))
            elif k == 2:
                algo[ch] = int(rng.integers(3))
                lines += _lorc_rule(rng, ch, algo[ch])
            elif k == 3:
                lines.append(_lorc_rule(rng, ch, algo[ch])[1])
            elif k == 4:
                lines.append("O %d %d" % (ch, _pick(rng, LORC_OFFSETS)))
            else:
                lines += ["T"] + _lorc_blocks("noise", int(rng.integers(40)), 2) + ["S"]
        ns = _pick(rng, NS)
        seg, blocks = lc.SEGMENTS[int(rng.integers(len(lc.SEGMENTS)))]
        n = _nblk(rng, ns)
        first = int(rng.integers(512 * blocks // ns - n + 1))
        lines += _lorc_blocks(seg, first, n, ns=ns)
    return lines


FFTEXT_RATES = (12000, 20250)
FFTEXT_ITIMES = ("0.01", "0.05", "0.13", "0.2", "0.5", "3.0", "8.768")
FFTEXT_MODES = (fc.USB, fc.SAM, fc.QAM)


def _fftext_run(rng):
    mode = _pick(rng, FFTEXT_MODES)
    return "S %d %d %d" % (int(rng.integers(-1, 3)), int(mode != fc.USB), mode)


def fftext_script(seed):
    """One script in five holds, in place of one of its segments, a long integration: `I 8.768` or `I 3.0`, `S 2` and 201 to 260
    passband blocks with no command between them.  At 8.768 s the period has 205 bins (346 at 20.25 kHz) and the blocks past bin 199
    are dropped; at 3.0 s it has 70 (118) and the walk wraps or fills more than a hundred bins of the sums."""
    rng = _rng("fftext", seed)
    lines = ["R %d" % _pick(rng, FFTEXT_RATES), "I %s" % _pick(rng, FFTEXT_ITIMES), _fftext_run(rng)]
    nseg = int(rng.integers(3, 9))
    long_at = int(rng.integers(1, nseg)) if rng.random() < 0.2 else -1
    for s in range(nseg):
        if s == long_at:
            lines += ["I %s" % _pick(rng, ("8.768", "3.0")), "S %d 0 %d" % (fc.INTEG, fc.USB)]
            lines += ["B %d %d" % (fc.PASSBAND, int(rng.integers(fc.NPOOL))) for _ in range(int(rng.integers(201, 261)))]
            continue
        if s:
            k = int(rng.integers(5))
            lines += [["C"], ["I %s" % _pick(rng, FFTEXT_ITIMES)], [_fftext_run(rng)], ["R %d" % _pick(rng, FFTEXT_RATES)], ["C", _fftext_run(rng)]][k]
        lines += ["B %d %d" % (_pick(rng, (fc.PASSBAND, fc.CHAN_NULL)), int(rng.integers(fc.NPOOL))) for _ in range(int(rng.integers(1, 40)))]
    return lines


# ---- kg_fax.  C lpm imagewidth carrier deviation bandwidth headers phasing autostop debug nom srate | R srate | H shift | T | B off
MOST_BLOCKS = 400                                # a fax or cw script has no more blocks
LONG = (257, 400)                                # one script in five holds a stretch of so many blocks with no other line between them
FAX_LINES = 255                                  # the reference harness ends a run whose configuration outgrows 256 lines (exit 9)
FAX_WIDTHS = (1, 7, 255, 256, 257, 333, 640, 1024, 1809, 1900)         # and spl
FAX_TUNINGS = ((1900, 400), (1800, 450), (1900, -400))
FAX_SPLS = (10, 16, 17, 100, 255, 256, 257, 1023, 1024, 1025, 1030, 1039, 1040, 2048, 2049, 2999, 3000, 3001, 4096, 20250, 24575, 24576)
FAX_SHIFTS = ("0.0", "0.0245", "0.37", "0.9", "1.0")
FAX_NATIVE = tuple(s for s in fxc.SEGMENTS if s[0] != "zeros")
FAX_DENSE = ((1039, 257), (1039, 258), (1040, 257), (1040, 258), (2048, 400))     # (spl, blocks) at half the nominal rate: 200 lines or more, under 256
FAX_NPOOL = fxc.POOL // fxc.BLK


def fax_rates(nom):
    """half the nominal rate exactly and just above, the nominal and just above, twice the nominal just below and exactly"""
    return (nom / 2, nom / 2 * 1.002, float(nom), nom * 1.0001, 2 * nom * 0.998, 2.0 * nom)


class _Fax:
    """a fax script under way: its lines, the blocks it may still hold and the bound on the lines since the last C, computed from the
    script alone -- a block gives at most 512 / ratio + 1 picks, under the least ratio a line since the C can have begun with"""

    def __init__(self):
        self.lines, self.left, self.on = [], MOST_BLOCKS, False
        self.spl = self.nom = self.picks = 0
        self.rmin = 1.0

    def config(self, lpm, w, tuning, bw, hdr, ph, stop, dbg, nom, srate):
        self.lines.append(fxc._C(lpm, w, tuning[0], tuning[1], bw, hdr, ph, stop, dbg, nom, srate))
        self.spl, self.nom, self.rmin, self.picks, self.on = int(nom * 60.0 / lpm), nom, srate / nom, 0.0, True

    def rate(self, srate):
        self.lines.append("R %r" % float(srate))
        self.rmin = min(self.rmin, srate / self.nom)

    def room(self):
        if not self.on:
            return self.left
        return max(0, min(self.left, int((FAX_LINES * self.spl - self.picks) // (fxc.BLK / self.rmin + 1))))

    def blocks(self, first, n):
        """n pool blocks from block `first` on, around the pool's end; as many of them as fit -> how many"""
        n = min(n, self.room())
        self.lines += ["B %d" % (fxc.BLK * ((first + k) % FAX_NPOOL)) for k in range(n)]
        self.left -= n
        if self.on:
            self.picks += n * (fxc.BLK / self.rmin + 1)
        return n

    def stop(self, rng):
        """T with blocks behind it"""
        self.lines.append("T")
        self.on = False
        self.blocks(int(rng.integers(FAX_NPOOL)), int(rng.integers(1, 5)))


def _fax_flags(rng):
    """headers, phasing, autostop, debug"""
    return int(rng.random() < 0.7), int(rng.random() < 0.6), int(rng.random() < 0.6), int(rng.random() < 0.2)


def _fax_native(g, rng, seg, story):
    """a pool segment at its own lpm and nominal rate, the sample rate within 2 Hz of it -> what gives the next stretch's first block"""
    name, fs, lpm, _, plan = seg
    spl = fs * 60 // lpm
    hdr, ph, stop, dbg = (int(rng.random() < 0.5), 1, int(rng.integers(2)), 0) if story else _fax_flags(rng)
    g.config(lpm, _pick(rng, FAX_WIDTHS + (spl,)), _pick(rng, FAX_TUNINGS[:2] if story else FAX_TUNINGS), int(rng.integers(3)), hdr, ph, stop, dbg, fs,
             round(fs + float(rng.uniform(-2, 2)), 2))
    starts = np.cumsum([0] + [n for _, n in plan])[:-1] * spl // fxc.BLK          # the first block of every part of the segment
    kinds = [k for k, _ in plan]
    # under autostop, two times in five: the stop tone first, then the start tone behind it
    order = [starts[kinds.index("stop")], starts[kinds.index("start")]] if stop and "stop" in kinds and rng.random() < 0.4 else []

    def first():
        at = order.pop(0) if order else _pick(rng, starts)
        return fxc.AT[name] // fxc.BLK + int(np.clip(at + rng.integers(-3, 4), 0, fxc.NBLK[name] - 1))
    return first


def _fax_foreign(g, rng, spl=None, srate=None):
    """60 lpm at a nominal rate equal to the wanted line length, over any blocks of the pool"""
    spl = _pick(rng, FAX_SPLS) if spl is None else spl
    g.config(60, min(_pick(rng, FAX_WIDTHS + (spl,)), spl), _pick(rng, FAX_TUNINGS), int(rng.integers(3)), *_fax_flags(rng), spl,
             _pick(rng, fax_rates(spl)) if srate is None else srate)
    return lambda: int(rng.integers(FAX_NPOOL))


def fax_script(seed):
    """Two to five configurations, native or foreign, each with one to four stretches of blocks (60 to 140 of a native segment or of a line above 20000 samples, 3 to 80 otherwise) and
    between two stretches sometimes a command: R (either end of the accepted range, or anywhere in it), H, a second C in mid-line, or T with blocks behind it and a C.  One
    script in four is the 240 lpm segment from its start tone through its phasing lines, 372 blocks or more: phased, or -- with a shift in
    the middle of the phasing lines -- rejected.  One in five holds a stretch of 257 to 400 blocks with no other line between them; half
    of the foreign ones are FAX_DENSE, where the stretch completes 200 lines or more and stays under the 256."""
    rng = _rng("fax", seed)
    g = _Fax()
    if rng.random() < 0.25:
        first = _fax_native(g, rng, fxc.SEGMENTS[2], True)
        at, n = fxc.AT["a240"] // fxc.BLK + int(rng.integers(10, 30)), int(rng.integers(372, 391))
        if rng.random() < 0.5:
            k = int(rng.integers(200, 300))                                # the phasing lines are blocks 146 to 404 of the segment
            g.blocks(at, k)
            g.lines.append("H %s" % _pick(rng, FAX_SHIFTS[2:4]))
            g.blocks(at + k, n - k)
        else:
            g.blocks(at, n)
        g.blocks(first(), int(rng.integers(1, 11)))
        return g.lines
    nlong = int(rng.integers(LONG[0], LONG[1] + 1)) if rng.random() < 0.2 else 0
    nconf = int(rng.integers(2, 6))
    long_at = int(rng.integers(nconf)) if nlong else -1
    g.left -= nlong                                                        # kept for the long stretch
    for c in range(nconf):
        if c and rng.random() < 0.3:
            g.stop(rng)
        if c == long_at:
            g.left += nlong
            if rng.random() < 0.4:
                seg = _pick(rng, [s for s in FAX_NATIVE if fxc.NBLK[s[0]] >= nlong])
                _fax_native(g, rng, seg, False)
                g.blocks(fxc.AT[seg[0]] // fxc.BLK + int(rng.integers(fxc.NBLK[seg[0]] - nlong + 1)), nlong)
            elif rng.random() < 0.5:
                spl, n = _pick(rng, [d for d in FAX_DENSE if d[1] <= g.left] or FAX_DENSE[:1])
                first = _fax_foreign(g, rng, spl, fax_rates(spl)[0])
                g.blocks(first(), n)
            else:
                fits = [(s, r) for s in FAX_SPLS for r in fax_rates(s) if nlong * (fxc.BLK / (r / s) + 1) <= FAX_LINES * s]
                first = _fax_foreign(g, rng, *_pick(rng, fits))
                g.blocks(first(), nlong)
            continue
        native = rng.random() < 0.35
        seg = _pick(rng, FAX_NATIVE)
        again = (lambda: _fax_native(g, rng, seg, False)) if native else (lambda: _fax_foreign(g, rng))
        first = again()
        for s in range(int(rng.integers(1, 5))):
            if s:
                k = int(rng.integers(6))
                if k == 0:
                    g.rate(_pick(rng, (g.nom / 2, 2.0 * g.nom, round(float(rng.uniform(g.nom / 2, 2 * g.nom)), 3))))
                elif k == 1:
                    g.lines.append("H %s" % _pick(rng, FAX_SHIFTS))
                elif k == 2:
                    first = again()
                elif k == 3:
                    g.stop(rng)
                    first = again()
            g.blocks(first(), int(rng.integers(60, 141)) if native or g.spl >= 20000 else int(rng.integers(3, 81)))
    return g.lines


def fax_shapes():
    """the kernel-shape edges of csrc/kg_fax.hip, one script each: the pick walk's bound (1024 picks at half the rate), the demodulator's
    chunk of 1024 (a line of exactly one, two and 24 chunks, a last chunk shorter than the 16 carried products, a line shorter than
    them, than the workgroup), the detector's cap of 3000 from either side, the phasing search at its smallest stride (w == spl) and at
    one candidate (w == 1).  60 lpm at a nominal rate of 10 or 100 calls every line with a mean brightness above 5 a start line (300 Hz
    is a whole number of turns a sample): blocks of signal arm the phasing and blocks of silence, image lines, run it."""
    C, B, Z = fxc._C, fxc._B, fxc._B("zeros", 0, 18)
    s = {
        "ratio_half": [C(120, srate=6000.0)] + B("a120", 40, 60),
        "ratio_just_above_half": [C(120, srate=6000.0 * 1.002)] + B("a120", 40, 60),
        "ratio_twice": [C(120, srate=24000.0)] + B("a120", 40, 100),
        "spl_10": [C(60, w=7, nom=10)] + B("a120", 50, 1) + Z[:3],
        "spl_100": [C(60, w=100, nom=100, bw=2)] + B("a120", 50, 20) + Z[:10],
        "spl_255_w255": [C(60, w=255, nom=255)] + B("a240", 20, 50),
        "spl_1024_w1024": [C(60, w=1024, nom=1024, bw=0)] + B("a120", 40, 60),
        "spl_1030": [C(60, w=640, nom=1030)] + B("a120", 40, 60),
        "spl_4096": [C(60, w=1809, nom=4096, dev=-400)] + B("a60", 20, 80),
        "spl_24576": [C(60, w=1024, nom=24576)] + B("a60_20250", 30, 100),
        "spl_2999": [C(60, w=333, nom=2999)] + B("a240", 10, 60),
        "spl_3001": [C(60, w=333, nom=3001)] + B("a240", 10, 60),
        "w_equals_spl": [C(240, w=3000, stop=0)] + B("a240", 17, 60) + [C(60, w=100, nom=100)] + B("a120", 50, 2) + Z,
        "w_1": [C(120, w=1)] + B("a120", 40, 40) + [C(60, w=1, nom=100)] + B("a120", 50, 2) + Z,
        "rate_walk": [C(120, w=640)] + B("a120", 40, 20) + ["R 6000.0"] + B("a120", 60, 25) + ["R 24000.0"] + B("a120", 85, 30) + ["H 1.0"] + B("a120", 115, 25),
    }
    return s


# ---- kg_cw.  S training_interval nom srate | W wpm training_interval | P pboff | C wsc | A on | H threshold | T | N now | B off
CW_INTERVALS = (1, 2, 30, 40, 100, 255)
CW_NOMS = (12000, 12000, 12000, 12000, 12000, 12000, 20250, 20250, 20250, 88, 1000)
CW_RATIOS = (0.5, 1.0, 1.0, 1.0 + 1e-4, 1.0 - 1e-4, 2.0)
CW_WPMS = (0, 5, 25, 30, 60)
CW_THRESHOLDS = (-5, 0, 3000, 15000, 20000)
CW_PER_SEC = (6, 23, 40)
CW_BIN = {12000: 6, 20250: 4}                    # the pool's tone (cw_common.TONE)


def cw_pboff_a(srate, pboff):
    """g->a of kg_cw.h (pboff_a): the command is taken where it is within 0 .. 44"""
    return int(0.5 + float(np.float32(np.float32(pboff) * np.float32(88) / np.float32(srate))))


def cw_pboffs(srate, tone_bin):
    """0, the offset of the pool's tone bin, an offset of an empty bin, the largest accepted"""
    most = int(44.5 * srate / 88) + 2
    while cw_pboff_a(srate, most) > 44:
        most -= 1
    out = (0, int(round(tone_bin * srate / 88)), int(round(11 * srate / 88)), most)
    assert all(0 <= cw_pboff_a(srate, p) <= 44 for p in out) and cw_pboff_a(srate, out[1]) == tone_bin and cw_pboff_a(srate, most + 1) > 44, (srate, out)
    return out


class _Cw:
    """a cw script under way: its lines, the blocks it may still hold, the clock of the N lines and the rate in force"""

    def __init__(self, now):
        cwc.pool()
        self.lines, self.left, self.now, self.srate, self.bin = [], MOST_BLOCKS, now, 0.0, 6

    def start(self, ti, nom, ratio, seg):
        self.srate, self.bin = nom * ratio, CW_BIN[cwc.FS[seg]]
        self.lines.append("S %d %d %r" % (ti, nom, float(self.srate)))

    def tone(self):
        self.lines.append("P %d" % cw_pboffs(self.srate, self.bin)[1])

    def clock(self, step=1):
        self.now = (self.now + step) % (1 << 32)
        self.lines.append("N %d" % self.now)

    def blocks(self, seg, first, n, per_sec):
        """n blocks of the segment (around its end), the clock moving every per_sec blocks; per_sec 0: no line between them"""
        n = min(n, self.left)
        for k in range(n):
            if per_sec and k % per_sec == 0:
                self.clock()
            self.lines.append("B %d" % (cwc.AT[seg] + cwc.BLK * ((first + k) % cwc.NBLK[seg])))
        self.left -= n


def _cw_command(g, rng):
    k = int(rng.integers(8))
    if k == 0:
        return ["P %d" % _pick(rng, cw_pboffs(g.srate, g.bin))]
    if k == 1:
        return ["C %d" % int(rng.integers(2))]
    if k == 2:
        return ["A %d" % int(rng.integers(2))]
    if k == 3:
        return ["H %d" % _pick(rng, CW_THRESHOLDS)]
    if k == 4:                                   # CwDecode_Init: samples wait for the next pboff
        return ["W %d %d" % (_pick(rng, CW_WPMS), _pick(rng, CW_INTERVALS))] + (["P %d" % cw_pboffs(g.srate, g.bin)[1], "H 20000"] if rng.random() < 0.8 else [])
    if k == 5:
        g.clock(-int(rng.integers(1, 50)))       # the clock jumps backwards
        return []
    if k == 6:
        g.clock(int(rng.integers(2, 30)))
        return []
    return []


def cw_script(seed):
    """Half the scripts are a listening: one segment of the pool from its first block at its own rate (within 1e-4), the tone's bin, a
    training interval of 30 or 40, a fixed or the automatic threshold, tracked or (at 30 wpm) fixed speed -- so that the text, its
    word spaces, prosigns, [err], the retraining and the error time-out are reached -- with a command or two thrown in late.  The other
    half is commands at large: any interval, nominal rate (88 and 1000 too) and ratio, S in mid-stream, T then blocks then S, every
    command between stretches of 5 to 120 blocks.  The clock begins anywhere, a few seconds short of 2^32 in one script in six, moves
    every 6, 23 or 40 blocks and sometimes jumps backwards.  One script in five holds a stretch of 257 to 400 blocks with no N or other
    line between them."""
    rng = _rng("cw", seed)
    g = _Cw(int(_pick(rng, (100, 100, 5, 0x7ffffff0, 0xfffffff4, 0xfffffffa))))
    nlong = int(rng.integers(LONG[0], LONG[1] + 1)) if rng.random() < 0.2 else 0
    segs = sorted(cwc.NBLK)
    if rng.random() < 0.5:
        seg = _pick(rng, segs)
        g.start(_pick(rng, (30, 40)), cwc.FS[seg], _pick(rng, (1.0, 1.0, 1.0 + 1e-4, 1.0 - 1e-4)), seg)
        if rng.random() < 0.25:
            g.lines.append("W %d 40" % _pick(rng, (30, 25)))
        g.tone()
        g.lines.append("A 1" if rng.random() < 0.25 else "H %d" % _pick(rng, (15000, 20000)))
        per_sec = _pick(rng, CW_PER_SEC)
        n = min(cwc.NBLK[seg], MOST_BLOCKS - 10)
        if nlong:
            g.clock()
            g.blocks(seg, 0, nlong, 0)
            g.blocks(seg, nlong, max(n - nlong, 0), per_sec)
        else:
            cut = int(rng.integers(150, n))
            g.blocks(seg, 0, cut, per_sec)
            g.lines += _cw_command(g, rng) if rng.random() < 0.5 else []
            g.blocks(seg, cut, n - cut, per_sec)
        return g.lines
    nstretch = int(rng.integers(3, 9))
    long_at = int(rng.integers(nstretch)) if nlong else -1
    g.left -= nlong
    seg = _pick(rng, segs)
    for s in range(nstretch):
        if s == 0 or rng.random() < 0.3:
            if s and rng.random() < 0.4:
                g.lines.append("T")
                g.blocks(seg, int(rng.integers(cwc.NBLK[seg])), int(rng.integers(1, 5)), 0)
            seg = _pick(rng, segs)
            nom = _pick(rng, CW_NOMS)
            g.start(_pick(rng, CW_INTERVALS), nom, _pick(rng, CW_RATIOS), seg)
            if rng.random() < 0.85:
                g.tone()
            if rng.random() < 0.7:
                g.lines.append("H %d" % _pick(rng, CW_THRESHOLDS))
        else:
            for _ in range(int(rng.integers(1, 4))):
                g.lines += _cw_command(g, rng)
        first = 0 if rng.random() < 0.4 else int(rng.integers(cwc.NBLK[seg]))
        if s == long_at:
            g.left += nlong
            g.blocks(seg, first, nlong, 0)
        else:
            g.blocks(seg, first, int(rng.integers(5, 121)), _pick(rng, CW_PER_SEC))
    return g.lines


def cw_shapes():
    """the kernel-shape edges of csrc/kg_cw.hip, one script each: a push of 256 sound blocks (1489 or 1490 Goertzel blocks: six turns
    of phase A's loop, the whole of its magnitudes) and then one of 1; the ends of what the commands accept"""
    B = cwc._B
    head = lambda ti=40, nom=12000, srate=None, p=cwc.PBOFF, h=20000: [cwc._S(ti, nom, srate), "P %d" % p, "H %d" % h]
    plain = lambda seg, n: ["B %d" % (cwc.AT[seg] + cwc.BLK * k) for k in range(n)]
    cwc.pool()
    return {
        "one_push_256": head() + ["N 100"] + plain("clean", 256) + ["N 111"] + plain("clean", 257)[256:],
        "ti_1": head(ti=1) + B("clean", 0, 100),
        "ti_255": head(ti=255) + B("jitter", 0, 100),
        "threshold_0": head(h=0) + B("clean", 0, 40) + ["H 20000"] + B("clean", 40, 40),
        "ratio_half": head(srate=6000.0, p=409) + B("clean", 0, 100),
        "ratio_twice": head(srate=24000.0, p=1636) + B("clean", 0, 100),
        "nom_88": head(nom=88, p=6) + B("clean", 0, 100),
        "clock_backwards": head() + B("errtime", 0, 50, now=4294967280, per_sec=6) + ["N 3"] + B("errtime", 50, 30, now=1000, per_sec=6) + B("errtime", 80, 20, now=500, per_sec=6),
    }


SCRIPT = {"iqd": iqd_script, "lorc": lorc_script, "fftext": fftext_script, "fax": fax_script, "cw": cw_script}
COMMON = {"iqd": ic, "lorc": lc, "fftext": fc, "fax": fxc, "cw": cwc}
SHAPES = {"fax": fax_shapes, "cw": cw_shapes}


def shape_names(mod):
    return list(SHAPES[mod]())


def script_digest(lines):
    return np.frombuffer(ic.digest(("\n".join(lines) + "\n").encode()), np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the fixture
def _sha(b):
    return np.frombuffer(ic.digest(b), np.uint8)


def _status_bytes(status):
    """the four numbers of the text message, field by field (the record's last word is reserved)"""
    return b"".join(np.ascontiguousarray(status[f]).tobytes() for f in ("cmaI", "cmaQ", "df", "phase"))


def iqd_record(lines, got):
    return {"script_sha": script_digest(lines), "nrows": got["nrows"], "cmd": got["cmd"], "len": got["len"], "sent": got["sent"], "ints": got["ints"],
            "floats": got["floats"], "pll": got["pll"].reshape(-1), "stream_sha": _sha(ic.stream(got)), "status_sha": _sha(_status_bytes(got["status"])),
            "iq_sha": _sha(np.ascontiguousarray(got["iq"]).tobytes()), "plot_sha": _sha(np.ascontiguousarray(got["plot"]).tobytes()),
            "map_sha": _sha(np.ascontiguousarray(got["map"]).tobytes())}


def lorc_record(lines, got):
    return {"script_sha": script_digest(lines), "nrows": got["nrows"], "samp": got["samp"], "ch": got["ch"], "cmd": got["cmd"], "len": got["len"],
            "scalars": np.frombuffer(got["scalars"].tobytes(), np.uint8), "rows_sha": _sha(lc.all_bytes(got).tobytes()),
            "avg_sha": _sha(np.ascontiguousarray(got["avg"], np.float32).tobytes())}


def fftext_record(lines, got):
    return {"script_sha": script_digest(lines), "sent": got["sent"], "bins": got["bins"],
            "state": np.array([got["run"], got["instance"], got["nbins"], got["reset"]], np.int32),
            "scales": np.array([got["fft_scale"], got["spectrum_scale"]], np.float32), "times": np.array([got["fi"], got["fft_sec"], got["time"]], np.float64),
            "ncma": np.asarray(got["ncma"], np.int32), "rows_sha": _sha(np.ascontiguousarray(got["rows"], np.uint8).tobytes()),
            "pwr_sha": _sha(np.ascontiguousarray(got["pwr"], np.float32).tobytes())}


def _one_nan(rec):
    """a copy of a record with every NaN as one bit pattern (the device's is the positive quiet one, x86's the negative) and `pad` zeroed"""
    out = np.array(rec).reshape(1).copy()
    for name in out.dtype.names:
        if out.dtype[name].base.kind == "f":
            v = out[name]
            v[np.isnan(v)] = np.nan
        elif name == "pad":
            out[name] = 0
    return out


def fax_record(lines, got):
    """in full what places a failure: the lines of every block, and per line its type, flags and the pick at which it completed"""
    r = got["recs"]
    rest = r.copy()
    for f in ("blk", "off", "type", "flags"):
        rest[f] = 0
    return {"script_sha": script_digest(lines), "nlines": got["nlines"].astype(np.int16), "type": r["type"].astype(np.uint8), "flags": r["flags"].astype(np.uint8),
            "off": r["off"].astype(np.int16), "recs_sha": _sha(rest.tobytes()), "rows_sha": _sha(fxc.all_bytes(got).tobytes()),
            "info_sha": _sha(_one_nan(got["info"]).tobytes()), "samples_sha": _sha(np.ascontiguousarray(got["samples"], np.int16).tobytes()),
            "demod_sha": _sha(np.ascontiguousarray(got["demod"], np.uint8).tobytes()), "prev_sha": _sha(np.ascontiguousarray(got["prev"], np.uint8).tobytes()),
            "out_sha": _sha(np.ascontiguousarray(got["out"], np.uint8).tobytes())}


def cw_record(lines, got):
    """in full what places a failure: the events of every block and the text; of the other kinds their number and, for the walk of
    cw_features, every TRAIN event below 1 that does not repeat the TRAIN before it, as (block, value)"""
    e = got["evs"]
    tr = e[e["kind"] == cwc.TRAIN]
    new = np.ones(tr.size, bool)
    new[1:] = tr["a"][1:] != tr["a"][:-1]
    marks = tr[new & (tr["a"] <= 0)]
    return {"script_sha": script_digest(lines), "nev": got["nev"].astype(np.int16), "text": e[e["kind"] == cwc.CHARS]["a"].astype(np.uint8),
            "kinds": np.array([(e["kind"] == k).sum() for k in range(4)], np.int32),
            "marks": np.stack([marks["blk"], marks["a"]], axis=1).astype(np.int32).reshape(-1),
            "evs_sha": _sha(np.ascontiguousarray(e).tobytes()), "info_sha": _sha(np.array(got["info"]).tobytes())}


RECORD = {"iqd": iqd_record, "lorc": lorc_record, "fftext": fftext_record, "fax": fax_record, "cw": cw_record}


def pack(records, nseed=None):
    """per-seed records -> the arrays of the file: every field end to end over the seeds, and how many elements each seed has; where
    the records of shape scripts stand behind those of the nseed seeds, "nseed" counts the seeds alone"""
    out = {"nseed": np.array([len(records) if nseed is None else nseed], np.int32)}
    for key in records[0]:
        parts = [np.ascontiguousarray(r[key]).reshape(-1) for r in records]
        assert len({p.dtype for p in parts}) == 1, key
        out[key] = np.concatenate(parts)
        out["n_" + key] = np.array([p.size for p in parts], np.int32)
    return out


def unpack(g, seed):
    out = {}
    for key in g.files:
        if "n_" + key in g.files:
            n = g["n_" + key]
            at = int(n[:seed].sum())
            out[key] = g[key][at:at + int(n[seed])]
    return out


def fixture_path(mod):
    return os.path.join(ic.GOLD, "%s_rand_ref.npz" % mod)


def load(mod):
    return np.load(fixture_path(mod))


def _first_difference(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    if a.size != b.size:
        return "sizes %d and %d" % (a.size, b.size)
    if a.dtype != b.dtype:
        return "types %s and %s" % (a.dtype, b.dtype)
    w = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize)
    bad = np.flatnonzero(a.view(w) != b.view(w)) if w and a.dtype.names is None else np.array([0] if a.tobytes() != b.tobytes() else [], np.int64)
    return None if bad.size == 0 else "first at element %d: %r and %r (%d differ)" % (int(bad[0]), a[bad[0]], b[bad[0]], int(bad.size))


def same(a, b, *what):
    """bit for bit; a failure names the first differing element"""
    d = _first_difference(a, b)
    assert d is None, what + (d,)


def check_record(mod, seed, lines, got, want):
    """got (the keys of the module's parse()) against the fixture's record of the seed, field by field"""
    have = RECORD[mod](lines, got)
    assert sorted(have) == sorted(want), (mod, seed)
    for key in have:
        same(have[key], want[key], mod, "seed %d" % seed, key)


# ---------------------------------------------------------------------------------------------------------------- what a script reached
def iqd_features(lines, rec):
    """the schedule of kg_iqd.h (fresh, the commands, block_sched) walked beside the reference's record of the script"""
    f = set()
    points = draw = dmode = exponent = msk = gain = 0
    ring, on, fed, last_inst = [0, 0], False, 0, None
    after_clear = after_stop = False
    stretch = [0, 0]                             # samples of the blocks since the last command or change of ns, and their ns

    def close_stretch():
        if stretch[0] and draw in (0, 1) and points > stretch[0]:
            f.add("lap longer than a call")
        stretch[0] = 0

    for l in lines:
        a = l.split()
        if a[0] != "B":
            close_stretch()
            last_inst = None
        if a[0] == "N":
            points, draw, dmode, exponent, msk, gain, ring, on = 1024, 0, 0, 1, 0, 0, [0, 0], False
        elif a[0] == "R":
            on = int(a[1]) != 0
            after_stop = not on and fed > 0
        elif a[0] == "G":
            gain = int(a[1])
        elif a[0] == "P":
            points = int(a[1])
        elif a[0] == "M":
            if int(a[1]) <= 1:
                exponent, msk = int(a[2]), 0
            elif int(a[1]) == 2:
                exponent, msk = 2, 1
        elif a[0] == "D":
            draw = int(a[1])
        elif a[0] == "Y":
            dmode = int(a[1])
        elif a[0] == "C":
            after_clear = fed > 0
        elif a[0] == "B":
            inst, ns = int(a[1]), int(a[2])
            if not on:
                if after_stop:
                    f.add("R 0 with blocks behind it")
                continue
            if stretch[0] and stretch[1] != ns:
                close_stretch()
            stretch[0], stretch[1] = stretch[0] + ns, ns
            fed += 1
            f.add("ns %d" % ns)
            f.add("draw 2" if draw == 2 else "drawn")
            f.add("msk" if msk else "pll off" if exponent == 0 else "exponent %d" % exponent if exponent in (1, 2, 4, 8) else "odd exponent")
            f.add("fixed gain" if gain else "auto gain")
            if dmode == 1 and exponent:
                f.add("display_mode 1")
            if after_clear:
                f.add("C with blocks behind it")
                after_clear = False
            if last_inst is not None and last_inst != inst:
                f.add("both instances alternating")
            last_inst = inst
            if draw in (0, 1):
                if points < ns:
                    f.add("lap shorter than a block")
                if ring[inst] >= points:
                    f.add("points below the ring position")
                first = max(points - ring[inst], 1)
                ring[inst] = ring[inst] + ns if ns < first else (ns - first) % points
    close_stretch()
    cmd = rec["cmd"]
    if ((cmd == 0) | (cmd == 1)).any():
        f.add("points rows")
    if ((cmd == 2) | (cmd == 3)).any():
        f.add("density rows")
    return f


IQD_CONDITIONS = (["ns %d" % n for n in NS] + ["points rows", "density rows", "pll off", "exponent 1", "exponent 2", "exponent 4", "exponent 8", "odd exponent",
                                                "msk", "display_mode 1", "lap shorter than a block", "lap longer than a call", "points below the ring position",
                                                "both instances alternating", "C with blocks behind it", "R 0 with blocks behind it", "auto gain", "fixed gain",
                                                "draw 2"])
IQD_MIN_ROWS = 5000


def _lorc_nbucket(srate, gri):
    """cmd_gri of kg_lorc.h -> (nbucket, halved)"""
    nb = int(np.floor(srate * (gri / 1e5))) + 1
    return (nb // 2, True) if nb > lc.MAX_BUCKET else (nb, False)


def lorc_features(lines, rec):
    """the commands of kg_lorc.h walked beside the reference's record of the script.  SCOPE_RESET is sent behind `SET gri` and `SET
    start` alone (loran_c.cpp:119-121), which the walk asserts of every row; what no command causes is the CMA's reset by time-out (:126).
    It sends no row, so it is named twice: "CMA reset by time-out" from the script alone, by a sufficient bound on the samples fed since a
    restart was asked for -- not an observation --, and "CMA time-out in the end state" from what the reference wrote: avg_samps counts
    from the last reset, the restart's comes within a GRI of its command, and a count more than that short of the samples fed since
    says that a later reset, which only the time-out makes, zeroed it"""
    f = set()
    srate, i_srate, started, ninit, fed = 0.0, 0, False, 0, 0
    algo, nbucket, halved, offset, param, quiet = [0, 0], [0, 0], [False, False], [0, 0], [0, 0], [0, 0]      # quiet: samples since a restart was asked for
    fresh = after_start = False                  # no block since `N`; a stop and a start with no block of the run since
    armed = False                                # a command has asked for the SCOPE_RESET of the next row
    nrows, cmd, samp, ch = rec["nrows"], rec["cmd"], rec["samp"], rec["ch"]
    blk = row = 0
    for l in lines:
        a = l.split()
        if a[0] == "N":
            srate, i_srate, ninit, fresh = float(a[1]), int(a[2]), ninit + 1, True
            algo, nbucket, halved, offset, param, quiet, armed = [0, 0], [0, 0], [False, False], [0, 0], [0, 0], [0, 0], False
        elif a[0] == "I":
            c = int(a[1])
            (nbucket[c], halved[c]), armed, quiet[c] = _lorc_nbucket(srate, int(a[2])), True, 0
        elif a[0] == "O":
            c = int(a[1])
            offset[c], quiet[c] = ((offset[c] + int(a[2])) % (1 << 32)) % nbucket[c], 0
        elif a[0] == "G":
            quiet[int(a[1])] = 0
        elif a[0] == "A":
            algo[int(a[1])], quiet[int(a[1])] = int(a[2]), 0
        elif a[0] == "P":
            v = float(a[2])
            param[int(a[1])], quiet[int(a[1])] = int(np.copysign(np.floor(abs(v) + 0.5), v)), 0       # lround
        elif a[0] == "S":
            after_start, started, armed, quiet = fed > 0 and not started, True, True, [0, 0]
        elif a[0] == "T":
            started = False
        elif a[0] == "B":
            n = int(nrows[blk])
            blk += 1
            if not started:
                assert n == 0
                continue
            fed += 1
            for c in range(2):
                f.add("rule %d on chain %d" % (algo[c], c))
                if halved[c] and srate == 20250:
                    f.add("halved GRI")
                if nbucket[c] <= 24:
                    f.add("nbucket <= 24")
                if fresh and offset[c] > 0:
                    f.add("samp below the offset")      # samp is 0 behind the memset
                # the restart is taken at the first bucket 0, the time-out at the first one behind i_srate * avg_param_i further samples
                quiet[c] += int(a[1])
                if algo[c] == lc.CMA and param[c] >= 1 and quiet[c] > i_srate * param[c] + 2 * (nbucket[c] + 1):
                    f.add("CMA reset by time-out")
            if after_start:
                f.add("stop / start")
            if ninit > 1:
                f.add("a second N")
            fresh = after_start = False
            if n and armed:
                f.add("SCOPE_RESET rows")
            for r in range(row, row + n):
                assert (cmd[r] == 1) == armed, "SCOPE_RESET is the first row behind `SET gri` or `SET start`, and no other"
                armed = False
                if r > row and samp[r] == samp[r - 1] and (ch[r - 1], ch[r]) == (0, 1):
                    f.add("two chains on one sample")
            row += n
    end = np.frombuffer(rec["scalars"].tobytes(), lc.scalars_dtype)[0]["ch"]
    for c in range(2):
        assert (int(end[c]["avg_algo"]), int(end[c]["nbucket"]), int(end[c]["avg_param_i"])) == (algo[c], nbucket[c], param[c]), "the walk's commands"
        if algo[c] == lc.CMA and end[c]["restart"] == 0 and quiet[c] - int(end[c]["avg_samps"]) > nbucket[c] + 1:
            f.add("CMA time-out in the end state")
    return f


LORC_CONDITIONS = (["rule %d on chain %d" % (a, c) for a in range(3) for c in range(2)]
                   + ["halved GRI", "nbucket <= 24", "CMA reset by time-out", "CMA time-out in the end state", "SCOPE_RESET rows", "two chains on one sample", "samp below the offset", "stop / start",
                      "a second N"])
LORC_MIN_ROWS = 300


def fftext_features(lines, rec):
    """the head of fft_data as kg_fftext.h has it (block()), walked beside the reference's record; the walk's own answer of which blocks
    are sent is held to the record's"""
    f = set()
    rate, run, instance, mode, reset, time = 0.0, fc.OFF, fc.PASSBAND, fc.USB, False, 0.0
    at_rate, bins, fi, fft_sec = None, 0, 0.0, 0.0
    taken, changed, rate_waits, off_waits = 0, False, False, False
    sent, blk = rec["sent"], 0
    for l in lines:
        a = l.split()
        if a[0] == "R":
            rate = float(a[1])
            rate_waits = at_rate is not None and rate != at_rate
        elif a[0] == "I":
            time, reset, changed = float(a[1]), True, False
        elif a[0] == "C":
            reset, changed = True, False
        elif a[0] == "S":
            new = int(a[1])
            if new == fc.OFF:
                off_waits = True
            else:
                changed = changed or (run != fc.OFF and new != run and taken > 0 and not reset)
                mode = int(a[3])
                instance = fc.CHAN_NULL if new == fc.SPEC and int(a[2]) else fc.PASSBAND
            run = new
        elif a[0] == "B":
            s, blk = int(sent[blk]), blk + 1
            if run == fc.OFF:
                if off_waits:
                    f.add("S -1 with blocks behind it")
                assert s == 0
                continue
            if int(a[1]) != instance:
                assert s == 0
                continue
            if reset:
                if rate_waits and rate != at_rate and taken:
                    f.add("rate change taken up at a reset")
                at_rate, fft_sec, fi, reset, rate_waits = rate, 1.0 / (rate * 2 / fc.W), 0.0, False, False
                bins = int(np.trunc(time / fft_sec))
            b = 0
            if run == fc.INTEG:
                f.add("integ period of 0 bins" if bins == 0 else "integ period above 200 bins" if bins > fc.MAX_BINS else "integ")
                b = int(np.trunc(np.fmod(fi, time) / time * bins))
                fi += fft_sec
            assert s == int(b < fc.MAX_BINS), (blk, s, b)
            if run == fc.INTEG and not s:
                f.add("block dropped past bin 199")                    # the reference sent nothing for it, and fi went on
            if run == fc.INTEG and b >= 100:
                f.add("bin 100 or above filled")
            if run == fc.INTEG and bins > 0 and fi - fft_sec >= time:
                f.add("integ walk wrapped")
            taken += 1
            if changed:
                f.add("function change without C")
                changed = False
            if s:
                f.add("rows of function %d" % run)
                if instance == fc.CHAN_NULL:
                    f.add("SAM on the second instance" if mode == fc.SAM else "QAM on the second instance")
    return f


FFTEXT_CONDITIONS = (["rows of function %d" % k for k in (fc.WF, fc.SPEC, fc.INTEG)]
                     + ["SAM on the second instance", "QAM on the second instance", "integ period of 0 bins", "integ period above 200 bins", "block dropped past bin 199",
                        "bin 100 or above filled", "integ walk wrapped",
                        "function change without C", "rate change taken up at a reset", "S -1 with blocks behind it"])

def fax_features(lines, rec):
    """the commands of kg_fax.h and the head of ProcessSamples (block_head) walked beside the reference's record of the script.  The
    ratio a line is demodulated with is that of the block it completes in (line_begin).  `skip` is a bound, from the script and the
    flags alone, on the samples still to come off the front of the next blocks (a shift, the phasing result; a restart keeps it): a
    block with nothing to skip that completes no line leaves the line begun, which is what "a C in mid-line" is told by"""
    f = set()
    nl, typ, flg = rec["nlines"], rec["type"], rec["flags"]
    on = mid = after_stop = False
    spl = w = bw = dev = dbg = skip = stretch = stretch_lines = 0
    nom = srate = shift = 0.0
    r_end, h1 = None, False
    blk = line = 0

    def close_stretch():
        if stretch >= LONG[0]:
            f.add("a stretch of 257 blocks or more")
            if stretch_lines >= 200:
                f.add("a stretch that completes 200 lines or more")

    for l in lines:
        a = l.split()
        if a[0] != "B":
            close_stretch()
            stretch = stretch_lines = 0
        if a[0] == "C":
            if mid:
                f.add("a C in mid-line")
            lpm, w, dev, bw, dbg, nom, srate = int(a[1]), int(a[2]), int(a[4]), int(a[5]), int(a[9]), float(a[10]), float(a[11])
            spl, on, mid, r_end, h1 = int(nom * 60.0 / lpm), True, False, None, False
        elif a[0] == "R":
            srate = float(a[1])
            r_end = "half" if srate == nom / 2 else "twice" if srate == nom * 2 else None
        elif a[0] == "H":
            shift = float(a[1])
        elif a[0] == "T":
            on, shift, after_stop = False, 0.0, True
        elif a[0] == "B":
            n = int(nl[blk])
            blk += 1
            if not on:
                assert n == 0
                if after_stop:
                    f.add("T with blocks behind it")
                continue
            if shift:
                if shift == 1.0 and spl > fxc.BLK:
                    h1 = True
                skip, shift = spl, 0.0
            if h1:
                f.add("H 1.0: a skip larger than a block")
                h1 = False
            mid = (skip < fxc.BLK and n == 0) or (mid and skip >= fxc.BLK)
            skip = max(skip - fxc.BLK, 0)
            stretch, stretch_lines = stretch + 1, stretch_lines + n
            if n >= 2:
                f.add("a block that completes 2 lines or more")
            for k in range(line, line + n):
                f.add("line type %d" % typ[k])
                f |= {"flag %d" % b for b in (1, 2, 4, 8, 16, 32, 64) if flg[k] & b}
                if flg[k] & fxc.F_PHASED:
                    skip = spl                                             # phased is sent with a non-zero skip, and only then
                if dbg and flg[k] & fxc.F_ROW_SENT:
                    f.add("debug rows")
            line += n
            if n:
                mid = False
                ratio = srate / nom
                f |= {"lines at ratio <= 0.501"} if ratio <= 0.501 else {"lines at ratio >= 1.996"} if ratio >= 1.996 else set()
                if r_end:
                    f.add("R to %s the nominal rate with lines behind it" % r_end)
                f.add("bandwidth %d" % bw)
                if dev < 0:
                    f.add("negative deviation")
                f |= {"spl a multiple of 1024"} if spl % 1024 == 0 else set()
                f |= {"spl in 1025..1039"} if 1025 <= spl <= 1039 else set()
                f |= {"spl below 256"} if spl < 256 else set()
                f |= {"spl below 17"} if spl < 17 else set()
                f |= {"spl %d" % spl} if spl in (2999, 3000, 3001, 24576) else set()
                f |= {"w == spl"} if w == spl else set()
                f |= {"w == 1"} if w == 1 else set()
                f |= {"w in 255..257"} if w in (255, 256, 257) else set()
    close_stretch()
    assert blk == nl.size and line == typ.size
    return f


FAX_CONDITIONS = (["lines at ratio <= 0.501", "lines at ratio >= 1.996", "spl a multiple of 1024", "spl in 1025..1039", "spl below 256", "spl below 17", "spl 2999", "spl 3000",
                   "spl 3001", "spl 24576", "w == spl", "w == 1", "w in 255..257", "bandwidth 0", "bandwidth 1", "bandwidth 2", "negative deviation", "debug rows"]
                  + ["line type %d" % t for t in range(3)] + ["flag %d" % b for b in (1, 2, 4, 8, 16, 32, 64)]      # 8: phased, with a non-zero skip; 32: rejected
                  + ["R to half the nominal rate with lines behind it", "R to twice the nominal rate with lines behind it", "H 1.0: a skip larger than a block",
                     "a C in mid-line", "T with blocks behind it", "a block that completes 2 lines or more", "a stretch of 257 blocks or more",
                     "a stretch that completes 200 lines or more"])


def cw_features(lines, rec):
    """the commands of kg_cw.h walked beside the reference's record of the script.  A TRAIN of -4 is the fourth error, which restarts
    the training; a TRAIN of 0 behind one of -1 .. -3 with no S or W between their blocks is the error time-out's (cw_train sends its
    own only while the decoder is not initialised, which an error count above 0 rules out)"""
    f = set()
    nev, text, kinds, marks = rec["nev"], rec["text"], rec["kinds"], rec["marks"].reshape(-1, 2)
    f |= {"event kind %d" % k for k in range(4) if kinds[k]}
    f |= {"a word space"} if (text == ord(" ")).any() else set()
    f |= {"a prosign"} if (text < 12).any() else set()
    f |= {"[err]"} if (text == 0xff).any() else set()
    on = taking = auto_waits = after_stop = False
    nom = ratio = 0.0
    ti = wpm = fed = stretch = 0
    threshold, now, back, wrapped = 0, None, False, False
    inits, blk = [], 0                                                     # the blocks ahead of which an S or W came
    for l in lines:
        a = l.split()
        if a[0] != "B":
            if stretch >= LONG[0]:
                f.add("a stretch of 257 blocks or more")
            stretch = 0
        if a[0] == "S":
            if fed and on:
                f.add("S in mid-stream")
            if after_stop:
                f.add("T then S")
            ti, nom, ratio, wpm = int(a[1]), float(a[2]), float(a[3]) / float(a[2]), 0
            on, taking, threshold, after_stop, fed, auto_waits = True, False, 0, False, 0, False
            inits.append(blk)
        elif a[0] == "W":
            wpm, ti, taking, threshold, fed, auto_waits = int(a[1]), int(a[2]), False, 0, 0, False
            inits.append(blk)
        elif a[0] == "P":
            if taking and (fxc.BLK * fed) % cwc.GBLK:
                f.add("a P in mid Goertzel block")
            taking = True
        elif a[0] == "A":
            auto_waits = int(a[1]) == 1
        elif a[0] == "H":
            threshold = int(a[1])
        elif a[0] == "T":
            on, after_stop = False, True
        elif a[0] == "N":
            v = int(a[1])
            if now is not None and v < now:
                wrapped, back = (True, back) if now >= (1 << 32) - 64 and v < 64 else (wrapped, True)
            now = v
        elif a[0] == "B":
            n, blk = int(nev[blk]), blk + 1
            if not (on and taking):
                assert n == 0
                continue
            fed, stretch = fed + 1, stretch + 1
            f.add("fixed speed" if wpm else "tracked speed")
            f.add("nominal %d" % nom if nom in (12000, 20250) else "nominal 88 or 1000")
            f |= {"ratio 0.5"} if ratio == 0.5 else {"ratio 2"} if ratio == 2 else set()
            f |= {"training interval %d" % ti} if not wpm and ti in (1, 255) else set()
            f |= {"threshold <= 0"} if threshold <= 0 else set()
            f |= {"a sound block with 8 events or more"} if n >= 8 else set()
            if auto_waits:
                f.add("automatic threshold switched on with blocks behind it")
                auto_waits = False
            if back:
                f.add("the clock going backwards")
            if wrapped:
                f.add("the clock crossing 2^32")
            back = wrapped = False
    if stretch >= LONG[0]:
        f.add("a stretch of 257 blocks or more")
    if (marks[:, 1] == -4).any():
        f.add("a retraining")
    for (b0, a0), (b1, a1) in zip(marks[:-1], marks[1:]):
        if -3 <= a0 <= -1 and a1 == 0 and not any(b0 < i <= b1 for i in inits):
            f.add("err_timeout taken")
    return f


CW_CONDITIONS = (["event kind %d" % k for k in range(4)]
                 + ["a word space", "a prosign", "[err]", "a retraining", "fixed speed", "tracked speed", "automatic threshold switched on with blocks behind it",
                    "a P in mid Goertzel block", "S in mid-stream", "T then S", "nominal 12000", "nominal 20250", "nominal 88 or 1000", "ratio 0.5", "ratio 2",
                    "training interval 1", "training interval 255", "threshold <= 0", "a sound block with 8 events or more", "the clock going backwards",
                    "the clock crossing 2^32", "err_timeout taken", "a stretch of 257 blocks or more"])

FEATURES = {"iqd": iqd_features, "lorc": lorc_features, "fftext": fftext_features, "fax": fax_features, "cw": cw_features}
CONDITIONS = {"iqd": IQD_CONDITIONS, "lorc": LORC_CONDITIONS, "fftext": FFTEXT_CONDITIONS, "fax": FAX_CONDITIONS, "cw": CW_CONDITIONS}


def reached(mod, g):
    """-> ({condition: seeds that reach it}, rows in total, blocks in total) over the seeds of the fixture g"""
    by = {c: [] for c in CONDITIONS[mod]}
    rows = blocks = 0
    for seed in range(int(g["nseed"][0])):
        lines, rec = SCRIPT[mod](seed), unpack(g, seed)
        same(script_digest(lines), rec["script_sha"], mod, "seed %d" % seed, "the script")
        for c in FEATURES[mod](lines, rec):
            if c in by:
                by[c].append(seed)
        blocks += COMMON[mod].nblocks(lines)
        rows += int(rec[{"fftext": "sent", "fax": "nlines", "cw": "nev"}.get(mod, "nrows")].sum())
    return by, rows, blocks


def check_conditions(mod, g):
    by, rows, blocks = reached(mod, g)
    missed = [c for c, seeds in by.items() if not seeds]
    assert not missed, (mod, "no seed reaches", missed)
    assert int(g["nseed"][0]) == NSEED
    assert rows >= {"iqd": IQD_MIN_ROWS, "lorc": LORC_MIN_ROWS}.get(mod, 1), (mod, rows)
    return by, rows, blocks


def write_fixture(mod, exe, samples, tmp):
    """tools/make_ref_*_golden.py --random: seeds 0 .. NSEED-1 and then the module's shape scripts, in the order of SHAPES, through
    the reference harness `exe`; none may be refused"""
    C, recs = COMMON[mod], []
    for lines in [SCRIPT[mod](seed) for seed in range(NSEED)] + list(SHAPES[mod]().values() if mod in SHAPES else ()):
        got = C.run_script_exe(exe, lines, samples, tmp)                   # asserts exit status 0
        recs.append(RECORD[mod](lines, got))
    path = os.path.join(str(tmp), "rand.npz")
    np.savez_compressed(path, **pack(recs, NSEED))
    by, rows, blocks = reached(mod, np.load(path))
    for c, seeds in by.items():
        print("   %-36s %2d seeds" % (c, len(seeds)))
    print("%d seeds, %d blocks, %d rows, %d bytes" % (NSEED, blocks, rows, os.path.getsize(path)))
    check_conditions(mod, np.load(path))                                   # the file is kept only if it meets them
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    shutil.copyfile(path, fixture_path(mod))
    print("wrote %s" % fixture_path(mod))
