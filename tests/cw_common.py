"""What the CW decoder tests share (tests/test_cw_cpu.py, test_cw_gpu.py, tools/make_ref_cw_golden.py): the seeded pool of 16-bit audio
that tests/golden/cw_ref.npz was made from (the file holds the pool's digest, not the samples), the Morse keyer, the command / block
scripts, the parser of what the reference harness and the host driver write, the host driver tools/cw_host_driver.cpp (csrc/kg_cw.h
compiled for the host with the reference's flags) and the runner of a script on the device object.

A signal here is a tone at TONE Hz (the centre of the Goertzel bin that pboff 818 selects at 12 kHz) keyed by a list of (key down,
length in dots): raised edges (a 4 ms Hann window over the keying), Gaussian noise, Gaussian jitter of every length."""
import os

import numpy as np

from flydog_sdr_gps_amd.cw import ev_dtype, info_dtype

from . import script_common
from .script_common import digest, script_steps  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 0x43572121
BLK = 512
GBLK = 88                                       # CW_DECODER_BLOCKSIZE_DEFAULT
PBOFF = 818
CHARS, WPM, TRAIN, PLOT = 0, 1, 2, 3
PROSIGNS = ("<aa>", "<ar>", "<as>", "<bk>", "<bt>", "<cl>", "<ct>", "<hh>", "<kn>", "<nj>", "<sk>", "<sn>")
MORSE = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---", "K": "-.-", "L": ".-..",
         "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-", "U": "..-", "V": "...-", "W": ".--", "X": "-..-",
         "Y": "-.--", "Z": "--..", "0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...",
         "8": "---..", "9": "----.", "/": "-..-.", "?": "..--..", "=": "-...-", ".": ".-.-.-", ",": "--..--",
         "<ar>": ".-.-.", "<kn>": "-.--.", "<sk>": "...-.-", "<bt>": "-...-"}

assert ev_dtype.itemsize == 24 and len(info_dtype.names) == 56 + 3 and info_dtype.itemsize == 1760


def max_events(nblk):
    """kg_cw_max_events: 7 events a Goertzel block (csrc/kg_cw.h derives it), (512 nblk + 87) / 88 Goertzel blocks a push"""
    return 7 * ((BLK * nblk + GBLK - 1) // GBLK)


# ---- the keyer
def elements(text, char_gap=3.0, word_gap=7.0):
    """a text (prosigns as <xx>) -> [(key down, dots)], ending with a character gap"""
    out, i = [], 0
    while i < len(text):
        if text[i] == " ":
            out[-1] = (0, word_gap)
            i += 1
            continue
        tok = text[i:text.index(">", i) + 1] if text[i] == "<" else text[i]
        i += len(tok)
        for e in MORSE[tok]:
            out += [(1, 1.0 if e == "." else 3.0), (0, 1.0)]
        out[-1] = (0, char_gap)
    return out


def raw(pattern, gap=3.0):
    """one character from a string of . and -"""
    out = []
    for e in pattern:
        out += [(1, 1.0 if e == "." else 3.0), (0, 1.0)]
    out[-1] = (0, gap)
    return out


def key(rng, fs, wpm, plan, amp=8000.0, sigma=150.0, jitter=0.0, tone=None):
    """[(key down, dots)] -> int16 samples, padded with silence to whole sound blocks"""
    dot = fs * 1.2 / wpm
    n = [max(1, int(round(d * dot * (1.0 + (jitter * rng.standard_normal() if jitter else 0.0))))) for _, d in plan]
    env = np.concatenate([np.full(k, float(on)) for k, (on, _) in zip(n, plan)])
    env = np.concatenate([env, np.zeros((-env.size) % BLK)])
    w = np.hanning(int(0.004 * fs) | 1)
    env = np.convolve(env, w / w.sum(), mode="same")
    f = (tone if tone is not None else TONE[fs])
    x = amp * env * np.sin(2 * np.pi * f * np.arange(env.size) / fs) + sigma * rng.standard_normal(env.size)
    return np.round(x).astype(np.int16)


TONE = {12000: 6 * 12000.0 / GBLK, 20250: 4 * 20250.0 / GBLK}          # bin 6 at 12 kHz (818.18 Hz), bin 4 at 20.25 kHz (920.45 Hz)
MSG = "CQ DE K1ABC PSE <kn>"
PRE = "NINE NINE NINE NINE SEE SEE "           # what the training swallows.  It begins with a dash, which the first average needs, and its characters
                                               # end in dots: only the gap behind a dot moves cwspace_avg (:895)
SIL = [(0, 40.0)]


def _plans():
    """name -> (fs, wpm, sigma, jitter, [(key down, dots)])"""
    E = elements
    return (
        ("clean", 12000, 30, 150.0, 0.0, E(PRE + MSG, char_gap=2.6, word_gap=7.5) + SIL),
        ("jitter", 12000, 25, 300.0, 0.06, E(PRE + "THE QUICK FOX <ar>") + SIL),
        ("wsc", 12000, 30, 150.0, 0.0, E(PRE + "TEST ", 2.6, 7.5) + E("YOU ", 2.6, 4.3) + E("ARE HERE", 2.6, 7.5) + SIL),
        ("silence", 12000, 30, 0.0, 0.0, [(0, 200.0)]),
        ("gaps", 12000, 30, 150.0, 0.0, E(PRE + "K") + [(0, 88.0)] + E("NOW") + [(1, 60.0), (0, 7.0)] + E("END") + SIL),
        # a glitch of 0.3 dots inside a character: - . - glitch . is no character.  The first corrective branch drops the glitch, and its
        # shift (:1137-1147) stops one short of the character's first element, which the second then stands in for: . . - . is F
        ("glitch1", 12000, 25, 100.0, 0.0, E(PRE + "TEST ") + raw("-.-", gap=1.0) + [(1, 0.3), (0, 1.0)] + raw(".", gap=7.0) + E("TEST") + SIL),
        # two characters run together by a gap of 1.6 dots: Q Q as one is no character
        ("runon", 12000, 25, 100.0, 0.0, E(PRE + "TEST ") + raw("--.-", gap=1.2) + raw("--.-", gap=7.0) + E("TEST") + SIL),
        ("garble", 12000, 30, 150.0, 0.0, E(PRE + "TEST ") + raw(".........", 7.0) + raw(".......", 7.0) + raw("---------", 7.0) + raw(".-.-.-.-.", 7.0)
         + E("NINE NINE") + SIL),
        ("errtime", 12000, 25, 150.0, 0.0, E(PRE + "TEST ") + raw(".........", 7.0) + E("TEST TEST OK") + SIL),
        ("toolong", 12000, 35, 150.0, 0.0, E(PRE + "TEST ") + raw("." * 44, 7.0) + E("TEST OK") + SIL),
        ("clean20250", 20250, 35, 250.0, 0.0, E(PRE + "CQ K") + [(0, 20.0)]),
    )


AT, NBLK, FS, POOL = {}, {}, {}, 0
_pool = None


def pool():
    """-> int16 [POOL].  One generator, drawn in a fixed order; built once a process."""
    global _pool, POOL
    if _pool is not None:
        return _pool
    rng = np.random.Generator(np.random.PCG64(SEED))
    parts, at = [], 0
    for name, fs, wpm, sigma, jitter, plan in _plans():
        x = key(rng, fs, wpm, plan, sigma=sigma, jitter=jitter)
        AT[name], NBLK[name], FS[name] = at, x.size // BLK, fs
        parts.append(x)
        at += x.size
    out = np.concatenate(parts)
    out.setflags(write=False)
    POOL = out.size
    _pool = out
    return out


def load():
    return np.load(os.path.join(GOLD, "cw_ref.npz"))


# ---- the scripts.  S training_interval nom srate | W wpm training_interval | P pboff | C wsc | A on | H threshold | T | N now | B off
def _B(seg, first=0, n=None, now=100, per_sec=23):
    """blocks of a segment, with the clock of timer_sec() moving every per_sec blocks (23.4 sound blocks a second at 12 kHz)"""
    pool()
    n = NBLK[seg] - first if n is None else n
    assert first + n <= NBLK[seg], (seg, first, n)
    out = []
    for k in range(first, first + n):
        if k == first or k % per_sec == 0:
            out.append("N %d" % (now + k // per_sec))
        out.append("B %d" % (AT[seg] + BLK * k))
    return out


def _S(ti=40, nom=12000, srate=None):
    return "S %d %d %r" % (ti, nom, float(nom if srate is None else srate))


HEAD = [_S(), "P %d" % PBOFF, "H 20000"]


def scripts():
    pool()
    s = {
        # clean text, fixed threshold, tracking: training, the message with its word spaces, a prosign
        "clean_fixed": HEAD + _B("clean"),
        # fixed WPM: no training, no tracking
        "fixed_wpm": [_S(), "W 30 40", "P %d" % PBOFF, "H 20000"] + _B("clean"),
        # the automatic threshold (it lowers threshold_linear to 15849 and sets the weights)
        "auto_threshold": [_S(), "P %d" % PBOFF, "A 1"] + _B("clean"),
        "jitter_25": HEAD + _B("jitter"),
        # YOU before a word gap of 5.6 dots: the correction swallows the space; without it the space is printed
        "wsc_on": HEAD + _B("wsc"),
        "wsc_off": HEAD + ["C 0"] + _B("wsc"),
        # pboff moves to an empty bin and back, between sound blocks: in mid Goertzel block (512 is no multiple of 88)
        "pboff_mid": HEAD + _B("clean", 0, 150) + ["P 1500"] + _B("clean", 150, 40) + ["P %d" % PBOFF] + _B("clean", 190),
        # cw_train in mid stream: CwDecode_Init clears everything, the threshold too, and samples wait for the next pboff
        "restart_mid": HEAD + _B("clean", 0, 170) + [_S(30)] + _B("clean", 170, 3) + ["P %d" % PBOFF, "H 15000"] + _B("clean", 173),
        "silence_then_signal": HEAD + _B("silence", 0, 30) + _B("clean", 0, 250, now=200),
        # 3.5 s of key up (the time-out character, the clamp at 3 s), then 2.4 s of key down (a stuck key)
        "gaps": HEAD + _B("gaps"),
        "glitch_dropped": HEAD + _B("glitch1"),
        "run_on_split": HEAD + _B("runon"),
        # four characters that are none: the fourth error restarts the training
        "garble_retrain": HEAD + _B("garble"),
        # one error, then more than 8 s of good text by the clock of the N lines (time is an input): err_timeout clears the count
        "err_timeout": HEAD + _B("errtime", per_sec=6),
        # 44 dots in one character
        "too_long": HEAD + _B("toolong"),
        "rate_20250": [_S(40, 20250), "P 920", "H 20000"] + _B("clean20250", per_sec=40),
        "rate_off_nominal": [_S(40, 12000, 12001.37), "P %d" % PBOFF, "H 20000"] + _B("clean", 0, 300) + ["T"] + _B("clean", 300, 5),
    }
    return s


def nblocks(lines):
    return sum(1 for l in lines if l[0] == "B")


def parse(rawb, lines):
    """out.bin of the reference harness or the host driver -> dict: nev int32 [blocks], evs (ev_dtype, blk the script's block),
    info (one record of info_dtype), stats int32 [8] (the harness's; zeros from the driver)"""
    at, nev, evs = 0, [], []
    for b in range(nblocks(lines)):
        n = int(np.frombuffer(rawb[at:at + 4], np.int32)[0])
        at += 4
        e = np.frombuffer(rawb[at:at + 24 * n], ev_dtype).copy()
        at += 24 * n
        e["blk"] = b
        nev.append(n)
        evs.append(e)
    info = np.frombuffer(rawb[at:at + info_dtype.itemsize], info_dtype)[0].copy()
    at += info_dtype.itemsize
    assert len(rawb) - at == 32, (len(rawb), at)
    return {"nev": np.array(nev, np.int32), "evs": np.concatenate(evs) if evs else np.zeros(0, ev_dtype), "info": info,
            "stats": np.frombuffer(rawb[at:], np.int32).copy()}


def golden_of(got):
    return {"nev": got["nev"], "evs": np.frombuffer(got["evs"].tobytes(), np.int32).reshape(-1, 6), "info": np.frombuffer(got["info"].tobytes(), np.uint8),
            "stats": got["stats"]}


def text_of(evs):
    """the CHARS events as the client's text"""
    out = []
    for e in evs[evs["kind"] == CHARS]:
        a = int(e["a"])
        out.append("[err]" if a == 0xff else PROSIGNS[a] if a < 12 else chr(a))
    return "".join(out)


def check_against_golden(g, name, got):
    """equality on everything: the events of every block, every event's fields, the end state bit for bit"""
    k = "s_%s_" % name
    assert np.array_equal(got["nev"], g[k + "nev"]), (name, "events per block", np.flatnonzero(got["nev"] != g[k + "nev"])[:8])
    want = np.frombuffer(np.ascontiguousarray(g[k + "evs"]).tobytes(), ev_dtype)
    have = got["evs"]
    assert have.size == want.size, (name, have.size, want.size)
    for f in ev_dtype.names:
        bad = np.flatnonzero(have[f] != want[f])
        assert bad.size == 0, (name, "event field", f, "first differing event", int(bad[0]), have[bad[0]], want[bad[0]], int(bad.size))
    winfo = np.frombuffer(g[k + "info"].tobytes(), info_dtype)[0]
    for f in info_dtype.names:
        a, b = np.asarray(got["info"][f]), np.asarray(winfo[f])
        assert a.tobytes() == b.tobytes(), (name, "state", f, a, b)


# ---- the host driver
def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "cw_host_driver")


def run_script_exe(exe, lines, samples, tmpdir, expect=0, keep_on=False):
    out = script_common.run_script(exe, ["-k"] if keep_on else [], lines, samples, np.int16, tmpdir, expect)
    return parse(out, lines) if expect == 0 else None


# ---- a script on the device object
def apply_command(q, conn, l, now):
    """-> the clock behind the command"""
    a = l.split()
    if a[0] == "S":
        q.start(conn, int(a[1]), float(a[2]), float(a[3]))
    elif a[0] == "W":
        q.set_wpm(conn, int(a[1]), int(a[2]))
    elif a[0] == "P":
        q.set_pboff(conn, int(a[1]))
    elif a[0] == "C":
        q.set_wsc(conn, int(a[1]))
    elif a[0] == "A":
        q.set_auto_threshold(conn, int(a[1]))
    elif a[0] == "H":
        q.set_threshold(conn, int(a[1]))
    elif a[0] == "T":
        q.stop(conn)
    elif a[0] == "N":
        return int(a[1])
    else:
        raise ValueError(l)
    return now


class Recorder:
    """what a script leaves, in the keys of parse(): events are added push by push"""

    def __init__(self, nblk):
        self.nev = np.zeros(nblk, np.int32)
        self.evs = []

    def add(self, blocks, evs):
        """blocks: the script's block number of each block of the push; evs: ONE connection's, in order"""
        e = evs.copy()
        e["blk"] = np.asarray(blocks, np.int32)[evs["blk"]] if evs.size else e["blk"]
        np.add.at(self.nev, e["blk"], 1)
        self.evs.append(e)

    def result(self, info):
        return {"nev": self.nev, "evs": np.concatenate(self.evs) if self.evs else np.zeros(0, ev_dtype), "info": info}


def _items(lines):
    out, seen = [], 0
    for l in lines:
        if l[0] == "B":
            out.append(("blk", int(l.split()[1]), seen))
            seen += 1
        else:
            out.append(("cmd", l))
    return out


def run_side_by_side(q, scripts, samples, rng, most=24):
    """scripts[c] on connection c of q (a CwDecoder), in lockstep: every round each script takes its commands up to its next block,
    then ONE push feeds every connection with blocks left, 1 to `most` consecutive blocks each (drawn from rng, a numpy Generator) under
    its own now_sec, listed out of connection order.  Nothing of the schedule depends on what the device answers: with q None only the
    schedule is walked.  -> (per script the keys of parse() -- None without q --, pushes, pushes that carried more than one connection)"""
    items = [_items(s) for s in scripts]
    at, now = [0] * len(items), [0] * len(items)
    rec = [Recorder(nblocks(s)) for s in scripts]
    shared = calls = 0
    while any(a < len(it) for a, it in zip(at, items)):
        for c, it in enumerate(items):
            while at[c] < len(it) and it[at[c]][0] == "cmd":
                if q is not None:
                    now[c] = apply_command(q, c, it[at[c]][1], now[c])
                at[c] += 1
        take = {}
        for c, it in enumerate(items):
            n = 0
            lim = int(rng.integers(1, most + 1))
            while n < lim and at[c] + n < len(it) and it[at[c] + n][0] == "blk":
                n += 1
            if n:
                take[c] = it[at[c]:at[c] + n]
        if not take:
            break
        conns = sorted(take, key=lambda c: -c)
        if q is not None:
            x = np.zeros((len(conns), max(len(v) for v in take.values()), BLK), np.int16)
            for e, c in enumerate(conns):
                for b, (_, off, _) in enumerate(take[c]):
                    x[e, b] = samples[off:off + BLK]
            evs = q.push(conns, x, [now[c] for c in conns], nblk=[len(take[c]) for c in conns])
        for e, c in enumerate(conns):
            if q is not None:
                rec[c].add([b for _, _, b in take[c]], evs[e])
            at[c] += len(take[c])
        shared += len(conns) > 1
        calls += 1
    return [rec[c].result(q.state(c)) if q is not None else None for c in range(len(scripts))], calls, shared


def run_script_dev(q, lines, samples, conn=0, cuts=lambda: 64):
    """Runs a script on connection conn of q (a CwDecoder): every push one call.  -> the keys of parse(), "calls" and "gblocks"."""
    rec, calls, now, gblocks = Recorder(nblocks(lines)), 0, 0, []
    for st in script_steps(lines, cuts):
        if st[0] == "cmd":
            now = apply_command(q, conn, st[1], now)
            continue
        _, offs, blocks = st
        x = np.stack([samples[o:o + BLK] for o in offs])[None]
        evs = q.push([conn], x, [now])
        rec.add(blocks, evs[0])
        gblocks.append((len(offs), int(q.last_counts[0, 1])))
        calls += 1
    out = rec.result(q.state(conn))
    out["calls"], out["gblocks"] = calls, gblocks                          # per push: its sound blocks, the Goertzel blocks the device counted
    return out
