"""Seeded random command scripts for the three extension modules kg_iqd, kg_lorc and kg_fftext (tests/test_{iqd,lorc,fftext}_{cpu,gpu}.py,
tools/make_ref_{iqd,lorc,fftext}_golden.py --random): the hand-written scripts of the three *_common.py pin one case each; these draw
the combinations nobody wrote down -- a command of one kind behind one of another in mid-lap, points changed while both instances
alternate, a GRI behind a stop / start, a function change behind a rate change behind a clear.

A generator is a pure function of an integer seed and answers a script in its module's own script language over the module's own
seeded pool; it draws from the domain on which the reference harness and the host model take every script (exit status 0).  What the
reference wrote for seeds 0 .. NSEED-1 is kept in tests/golden/{iqd,lorc,fftext}_rand_ref.npz: integers in full, bytes by digest
(RECORD / pack / unpack).  FEATURES walks a script beside its record and names what it reached: the conditions of
test_random_fixture_meets_its_conditions.  tests/ext_random_dev.py runs the scripts on the device."""
import os
import shutil

import numpy as np

from . import fftext_common as fc
from . import iqd_common as ic
from . import lorc_common as lc

NSEED = 40
BASE = {"iqd": 0x49510400, "lorc": 0x4C4F0400, "fftext": 0x46580000}      # the first bases whose 40 seeds reach every condition (check_conditions)
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


SCRIPT = {"iqd": iqd_script, "lorc": lorc_script, "fftext": fftext_script}
COMMON = {"iqd": ic, "lorc": lc, "fftext": fc}


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


RECORD = {"iqd": iqd_record, "lorc": lorc_record, "fftext": fftext_record}


def pack(records):
    """per-seed records -> the arrays of the file: every field end to end over the seeds, and how many elements each seed has"""
    out = {"nseed": np.array([len(records)], np.int32)}
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

FEATURES = {"iqd": iqd_features, "lorc": lorc_features, "fftext": fftext_features}
CONDITIONS = {"iqd": IQD_CONDITIONS, "lorc": LORC_CONDITIONS, "fftext": FFTEXT_CONDITIONS}


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
        rows += int(rec["sent"].sum()) if mod == "fftext" else int(rec["nrows"].sum())
    return by, rows, blocks


def check_conditions(mod, g):
    by, rows, blocks = reached(mod, g)
    missed = [c for c, seeds in by.items() if not seeds]
    assert not missed, (mod, "no seed reaches", missed)
    assert int(g["nseed"][0]) == NSEED
    assert rows >= {"iqd": IQD_MIN_ROWS, "lorc": LORC_MIN_ROWS, "fftext": 1}[mod], (mod, rows)
    return by, rows, blocks


def write_fixture(mod, exe, samples, tmp):
    """tools/make_ref_*_golden.py --random: seeds 0 .. NSEED-1 through the reference harness `exe`; none may be refused"""
    C, recs = COMMON[mod], []
    for seed in range(NSEED):
        lines = SCRIPT[mod](seed)
        got = C.run_script_exe(exe, lines, samples, tmp)                   # asserts exit status 0
        recs.append(RECORD[mod](lines, got))
    path = os.path.join(str(tmp), "rand.npz")
    np.savez_compressed(path, **pack(recs))
    by, rows, blocks = reached(mod, np.load(path))
    for c, seeds in by.items():
        print("   %-36s %2d seeds" % (c, len(seeds)))
    print("%d seeds, %d blocks, %d rows, %d bytes" % (NSEED, blocks, rows, os.path.getsize(path)))
    check_conditions(mod, np.load(path))                                   # the file is kept only if it meets them
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    shutil.copyfile(path, fixture_path(mod))
    print("wrote %s" % fixture_path(mod))
