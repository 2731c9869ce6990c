"""Shared by the tracking tests (plain helper, imported like tests/fixtures.py): the scenarios, and three ways to run one --

    run_tool(model_exe, sc)     tools/trk_model.cpp, the LITERAL clock-by-clock model (the reference)
    run_tool(host_exe, sc)      tools/trk_host_driver.cpp: kg_trk.h, the closed form, on the host as one lane
    run_gpu(ctx, sc)            the library through flydog_sdr_gps_amd.trk.Tracker

all three give the same structure: one entry per 'X' step ([records per channel], a record = the 11 integers of a kg_trk_epoch
without its reserved word) and per 'D' step ([78-byte GPS_CHAN hex per channel], clocks consumed, [replica word per channel]).

A scenario is a list of steps in the script format of tools/trk_model.cpp: ("S", ch, word) CmdSetSat, ("C", ch, block) E1B code,
("L" / "G", ch, rate), ("l" / "g", ch, ki, kp - ki), ("P", ch, pol), ("M", mask), ("R",) sampler reset, ("U", ch, count) pause,
("O", ch, on) set_loop, ("X", nclocks), ("D",).  The literal model also restates, here in Python, the C/A generator of cacode.v
(ca_chips_literal) for the comparison with prn.py.

The signal tests (tests/test_trk_signal_cpu.py, tests/test_trk_signal_gpu.py) take from the end of this file scene() (several satellites
and gaps in one stream), start_at_bin() / start_acquired() (how a channel is started), signal_report() (what a run says about the
signal it was given) and signal_cases() (the table of cases).
"""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOM = 1 << 28                       # 16 clocks per chip
LO_NOM = 1 << 30                    # FC / FS
CA_EPOCH, E1B_EPOCH = 16368, 65472  # clocks at the nominal rate
RATE_MIN, RATE_MAX = 1 << 27, (1 << 29) - 1


class Scenario:
    def __init__(self, name, nchan, steps, bits=None, seed=1, lo_delay=216, cg_delay=577, codes=()):
        self.name, self.nchan, self.steps, self.lo_delay, self.cg_delay = name, nchan, list(steps), lo_delay, cg_delay
        self.nclocks = sum(s[1] for s in self.steps if s[0] == "X")
        if bits is None:
            bits = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (self.nclocks + 7) // 8 + 1, dtype=np.uint8)
        self.bits = np.ascontiguousarray(bits, np.uint8)
        assert self.bits.size * 8 >= self.nclocks
        self.codes = [np.ascontiguousarray(c, np.uint8) for c in codes]

    def script(self):
        return "".join(" ".join(str(int(v) if not isinstance(v, str) else v) for v in s) + "\n"
                       for s in [("N", self.nchan, self.lo_delay, self.cg_delay)] + self.steps)


def e1b_code(seed):
    """a stand-in memory code: 4092 seeded chips (the channel treats any column of the code memory alike)"""
    return np.random.Generator(np.random.PCG64(0xE1B0 + seed)).integers(0, 2, 4092, dtype=np.uint8)


def build(tmpdir, name):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/%s.cpp" % name
    exe = os.path.join(str(tmpdir), name)
    subprocess.run([gxx, "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", name + ".cpp")], check=True)
    return exe


def run_tool(exe, sc, tmpdir):
    """-> {"records": [records per channel, over all X steps], "dumps": [(GPS_CHAN hex per channel, clock, replicas) per D step],
    "refused": [indices into sc.steps of the commands the closed form's command layer refused with nothing changed]}"""
    tmp = str(tmpdir)
    bpath, cpath = os.path.join(tmp, sc.name + ".bits"), os.path.join(tmp, sc.name + ".codes")
    sc.bits.tofile(bpath)
    (np.concatenate(sc.codes) if sc.codes else np.zeros(0, np.uint8)).tofile(cpath)
    p = subprocess.run([exe, bpath, cpath], input=sc.script().encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (sc.name, p.returncode, p.stderr.decode()[-400:])
    recs = [[] for _ in range(sc.nchan)]
    dumps = []
    pend = []
    refused = []
    for line in p.stdout.decode().splitlines():
        f = line.split()
        if f[0] == "!":
            refused.append(int(f[1]))
        elif f[0] == "E":
            recs[int(f[1])].append(tuple(int(v) for v in f[2:]))
        elif f[0] == "C":
            pend.append(f[2])
        elif f[0] == "K":
            dumps.append((pend, int(f[1]), [int(v) for v in f[2:]]))
            pend = []
    return {"records": recs, "dumps": dumps, "refused": refused}


def without(sc, refused):
    """the scenario without the steps of those indices: what the literal model is given once the library has refused them"""
    return Scenario(sc.name + "_less", sc.nchan, [s for i, s in enumerate(sc.steps) if i not in set(refused)], bits=sc.bits,
                    lo_delay=sc.lo_delay, cg_delay=sc.cg_delay, codes=sc.codes)


def run_lines(exe, lines, tmpdir):
    """script lines that need no stream (Q, T) -> the output lines, split"""
    empty = os.path.join(str(tmpdir), "empty.bin")
    open(empty, "wb").close()
    p = subprocess.run([exe, empty, empty], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    return [l.split() for l in p.stdout.decode().splitlines()]


def run_gpu(ctx, sc, tracker_cls=None):
    """the same through the library: one Tracker.process per X step, from the byte that holds the next bit"""
    from flydog_sdr_gps_amd import KiwiGpuError, trk
    t = (tracker_cls or trk.Tracker)(ctx, sc.nchan, sc.lo_delay, sc.cg_delay)
    recs = [[] for _ in range(sc.nchan)]
    dumps = []
    refused = []
    clock = 0
    try:
        for i, s in enumerate(sc.steps):
            op = s[0]
            if op in "GRU":                             # the three commands that may answer KG_ERR_STATE and change nothing
                try:
                    {"G": t.set_rate_cg, "R": t.sampler_reset, "U": t.pause}[op](*s[1:])
                except KiwiGpuError as e:
                    assert e.status == -5, e
                    refused.append(i)
            elif op == "S":
                t.set_sat(s[1], s[2])
            elif op == "C":
                t.set_e1b_code(s[1], sc.codes[s[2]])
            elif op == "L":
                t.set_rate_lo(s[1], s[2])
            elif op == "l":
                t.set_gain_lo(s[1], s[2], s[3])
            elif op == "g":
                t.set_gain_cg(s[1], s[2], s[3])
            elif op == "P":
                t.set_polarity(s[1], s[2])
            elif op == "M":
                t.set_mask(s[1])
            elif op == "O":
                t.set_loop(s[1], s[2])
            elif op == "X":
                n = s[1]
                piece = sc.bits[clock // 8:(clock % 8 + n + 7) // 8 + clock // 8]
                for ch, ep in enumerate(t.process(piece, n)):
                    recs[ch] += [record_tuple(e) for e in ep]
                assert not t.stopped, t.stopped
                clock += n
            elif op == "D":
                ck, rep = t.get_clocks()
                dumps.append(([t.get_chan(ch).tobytes().hex() for ch in range(sc.nchan)], ck, [int(r) for r in rep]))
    finally:
        t.close()
    return {"records": recs, "dumps": dumps, "refused": refused}


def record_tuple(e):
    assert int(e["reserved"]) == 0
    return tuple(int(e[k]) for k in ("clock", "ip", "qp", "ie", "qe", "il", "ql", "lo_rate", "cg_rate", "flags"))


def assert_equal(got, want, what):
    """every epoch record, every GPS_CHAN byte, every replica word"""
    assert len(got["records"]) == len(want["records"]), what
    for ch, (g, w) in enumerate(zip(got["records"], want["records"])):
        assert len(g) == len(w), (what, "channel %d: %d records against %d" % (ch, len(g), len(w)), g[:2], w[:2])
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, (what, "channel %d record %d" % (ch, i), a, b)
    assert len(got["dumps"]) == len(want["dumps"]), what
    for i, (g, w) in enumerate(zip(got["dumps"], want["dumps"])):
        assert g[1] == w[1] and g[2] == w[2], (what, "dump %d: clock / replicas" % i, g[1:], w[1:])
        for ch, (a, b) in enumerate(zip(g[0], w[0])):
            assert a == b, (what, "dump %d GPS_CHAN of channel %d" % (i, ch), a, b)


def ca_chips_literal(word, n=1023):
    """cacode.v restated: reg [10:1] g1, g2; rst seeds them; rd shifts; chip from the taps or, under g2_init, g1[10] ^ g2[10]"""
    g2_init, init = (word >> 10) & 1, word & 0x3FF
    T0, T1 = (init >> 4) & 15, init & 15
    g1 = [None] + [1] * 10
    g2 = [None] + [((init >> (i - 1)) & 1) if g2_init else 1 for i in range(1, 11)]
    out = np.empty(n, np.uint8)
    for k in range(n):
        out[k] = (g1[10] ^ g2[10]) if g2_init else (g1[10] ^ g2[T0] ^ g2[T1])
        n1 = g1[3] ^ g1[10]
        n2 = g2[2] ^ g2[3] ^ g2[6] ^ g2[8] ^ g2[9] ^ g2[10]
        g1 = [None, n1] + g1[1:10]
        g2 = [None, n2] + g2[1:10]
    return out


# ---- the scenarios (tests/test_trk_cpu.py: host closed form; tests/test_trk_gpu.py: the kernel)
CA1, CA7 = (2 << 4) + 6, (1 << 4) + 8           # Navstar PRN 1, PRN 7
QZ = 0x400 | 0o1607                             # QZSS 194
E1 = 0x800 | 10


def _setup(ch, word, cg=NOM, lo=LO_NOM, gl=(20, 7), gc=(11, 12), code=None):
    s = [("S", ch, word)]
    if code is not None:
        s.append(("C", ch, code))
    return s + [("G", ch, cg), ("L", ch, lo), ("l", ch) + gl, ("g", ch) + gc]


def _pieces(total, pieces):
    """X steps of the given sizes in turn until `total` clocks are consumed"""
    out, left, i = [], total, 0
    while left:
        n = min(pieces[i % len(pieces)], left)
        out.append(("X", n))
        left -= n
        i += 1
    return out


def scenarios():
    S = {}
    D = ("D",)
    S["ca_taps"] = Scenario("ca_taps", 1, _setup(0, CA1) + [("R",), ("X", 40 * CA_EPOCH + 100), D])
    S["qzss"] = Scenario("qzss", 1, _setup(0, QZ) + [("R",), ("X", 40 * CA_EPOCH + 100), D], seed=2)
    for pol in (0, 1, 2):
        S["e1b_pol%d" % pol] = Scenario("e1b_pol%d" % pol, 1, _setup(0, E1, gl=(17, 7), code=0) + [("P", 0, pol), ("R",), ("X", 12 * E1B_EPOCH + 50), D],
                                        seed=3 + pol, codes=[e1b_code(pol)])
    # both ends of the accepted code rate.  At 2^27 the loop is off: its first negative error would write 2^27 - 1, which the library
    # stops on (the closed form's bound); one above it the loop runs with the smallest gains
    S["rate_ends"] = Scenario("rate_ends", 3, _setup(0, CA1, cg=RATE_MIN) + [("O", 0, 0)] + _setup(1, CA7, cg=RATE_MAX, gc=(0, 0)) +
                              _setup(2, CA1, cg=RATE_MIN + 64, gc=(0, 0)) + [("R",), ("X", 3 * 32736 + 17), D], seed=6)
    S["neg_lo"] = Scenario("neg_lo", 1, _setup(0, CA1, lo=(1 << 32) - LO_NOM - 12345) + [("R",), ("X", 6 * CA_EPOCH), D], seed=7)
    # pauses of 0, 1 and 16367 right after the reset (as CHANNEL::Start does), one more in mid-run, and one that a second channel's
    # pause moves (one counter for the bank)
    S["pauses"] = Scenario("pauses", 3, _setup(0, CA1) + _setup(1, CA7) + _setup(2, QZ) +
                           [("R",), ("X", 5000), ("U", 0, 0), ("X", 3), ("U", 1, 1), ("X", 40000), ("U", 2, 16367), ("X", 20000), D,
                            ("U", 0, 30000), ("X", 100), ("U", 1, 7), ("X", 5 * CA_EPOCH), D], seed=8)
    S["reset_masked"] = Scenario("reset_masked", 4, sum((_setup(c, w) for c, w in enumerate((CA1, CA7, QZ, CA1))), []) +
                                 [("R",), ("X", 3 * CA_EPOCH + 77), D, ("M", 0b0101), ("R",), ("X", 3 * CA_EPOCH), D], seed=9)
    S["all_ones"] = Scenario("all_ones", 2, _setup(0, CA1) + _setup(1, E1, code=0) + [("R",), ("X", 8 * CA_EPOCH), D],
                             bits=np.full(8 * CA_EPOCH // 8 + 1, 0xFF, np.uint8), codes=[e1b_code(5)])
    S["all_zeros"] = Scenario("all_zeros", 2, _setup(0, CA1) + _setup(1, E1, code=0) + [("R",), ("X", 8 * CA_EPOCH), D],
                              bits=np.zeros(8 * CA_EPOCH // 8 + 1, np.uint8), codes=[e1b_code(5)])
    # the integrators' extremes: the stream IS the early replica (then its complement), the LO stands at phase 0 and the loops are off,
    # so ie counts +8184 (every d 0) and then -8184 (every d 1) per epoch
    k = np.arange(8 * CA_EPOCH)
    rep = ca_chips_literal(CA1)[(k // 16) % 1023]
    rep[4 * CA_EPOCH:] ^= 1
    S["replica"] = Scenario("replica", 1, _setup(0, CA1, lo=0) + [("O", 0, 0), ("R",), ("X", 8 * CA_EPOCH), D],
                            bits=np.packbits(rep, bitorder="little"))
    words = [CA1, CA7, QZ, E1, (3 << 4) + 7, (4 << 4) + 8, 0x400 | 0o1747, 0x800 | 3, (5 << 4) + 9, (2 << 4) + 10, (1 << 4) + 9, 0x800 | 1]
    st = []
    for c, w in enumerate(words):
        st += _setup(c, w, cg=NOM + 40000 * (c - 6), lo=LO_NOM + 900000 * (c - 5), gl=(20 - c % 3, 7), gc=(11 + c % 2, 12),
                     code=(c % 3 if w & 0x800 else None))
        if w & 0x800:
            st.append(("P", c, c % 3))
    S["twelve"] = Scenario("twelve", 12, st + [("O", 5, 0), ("R",), ("X", 30000), ("U", 2, 777), ("X", 2 * E1B_EPOCH + 5), D], seed=10,
                           codes=[e1b_code(0), e1b_code(1), e1b_code(2)])
    S["delays2"] = Scenario("delays2", 2, _setup(0, CA1) + _setup(1, E1, code=0) + [("R",), ("X", 6 * CA_EPOCH), D], seed=11, lo_delay=2, cg_delay=8183,
                            codes=[e1b_code(7)])
    S["delays_equal"] = Scenario("delays_equal", 1, _setup(0, CA1) + [("R",), ("X", 4 * CA_EPOCH), D], seed=12, lo_delay=2, cg_delay=2)
    S["loop_off"] = Scenario("loop_off", 1, _setup(0, CA1) + [("O", 0, 0), ("R",), ("X", 5 * CA_EPOCH), D, ("O", 0, 1), ("X", 3 * CA_EPOCH), D], seed=13)
    # the same stream in one call and in pieces: inside a byte (1, 7), at an ms0 (the first ms0 of a reset channel is set by edge 7,
    # so a piece of 8 ends on it), between ms0 and each delay (7 + 100 and 7 + 300 with delays 216 / 577), and long ones
    total = 2 * 100001 + 8191 + 30000
    base = _setup(0, CA1) + _setup(1, E1, code=0) + [("R",)]
    S["one_call"] = Scenario("one_call", 2, base + [("X", total), D], seed=14, codes=[e1b_code(8)])
    S["pieces"] = Scenario("pieces", 2, base + [("X", 8), D, ("X", 99), D, ("X", 200), D, ("X", 1), ("X", 7), D] +
                           _pieces(total - 315, (1, 7, 8191, 100001)) + [D], seed=14, codes=[e1b_code(8)])
    # The three commands that would make a paused channel hold ms0 set, each refused with nothing changed while the bank runs on:
    # step 13 a code rate that turns channel 0's held phase (7 clocks of 2^28 - 40000 after the reset, just below a half chip with
    # nchip 0) into a held half chip; step 15 a pause 10 clocks after the reset (ms0 was set by edge 7, nchip is still 0, the service is
    # due); step 19 a reset that would take the paused channel 1, whose service is due (its ms0 fell near clock 16375), back to nchip 0.
    # The pauses of steps 12 and 17 and the masked reset of step 21 are accepted.
    S["refused_cmds"] = Scenario("refused_cmds", 2, _setup(0, CA1, cg=NOM - 40000) + _setup(1, CA7) +
                                 [("R",), ("X", 7), ("U", 0, 100), ("G", 0, NOM + 300000), ("X", 3), ("U", 1, 50), ("X", 16390), ("U", 1, 30000),
                                  ("X", 10), ("R",), ("M", 2), ("R",), ("X", 40000), D, ("X", 2 * CA_EPOCH), D], seed=16)
    S["e1b_nav130"] = Scenario("e1b_nav130", 1, _setup(0, E1, cg=RATE_MAX, gc=(0, 0), gl=(17, 7), code=0) + [("R",), ("X", 131 * 32737), D], seed=15,
                               codes=[e1b_code(9)])
    return S


def random_scenario(seed):
    """a seeded script of commands and process calls of every size class, for the soak of the closed form against the literal model"""
    r = np.random.default_rng(seed)
    nch = int(r.integers(1, 5))
    st, codes = [], [e1b_code(seed % 7), e1b_code(seed % 5 + 10)]
    words = [CA1, CA7, QZ, E1, 0x800 | 5]
    for c in range(nch):
        w = words[int(r.integers(0, len(words)))]
        cg = int(r.integers(RATE_MIN + 5000, RATE_MAX - 5000)) if r.random() < 0.5 else NOM + int(r.integers(-100000, 100000))
        st += _setup(c, w, cg=cg, lo=int(r.integers(0, 1 << 32)), gl=(int(r.integers(0, 22)), int(r.integers(0, 9))),
                     gc=(int(r.integers(0, 8)), int(r.integers(0, 8))), code=(int(r.integers(0, 2)) if w & 0x800 else None))
        if w & 0x800:
            st.append(("P", c, int(r.integers(0, 3))))
    st.append(("R",))
    for _ in range(int(r.integers(3, 14))):
        u, c = r.random(), int(r.integers(0, nch))
        if u < 0.35:
            st.append(("U", c, int(r.choice([0, 1, 5, 100, 9000, 16367, 65535, int(r.integers(0, 65536))]))))
        elif u < 0.45:
            st.append(("G", c, NOM + int(r.integers(-200000, 200000))))
        elif u < 0.5:
            st.append(("L", c, int(r.integers(0, 1 << 32))))
        elif u < 0.55:
            st += [("M", int(r.integers(0, 16))), ("R",)]
        elif u < 0.6:
            st.append(("O", c, int(r.integers(0, 2))))
        st.append(("X", int(r.choice([1, 2, 3, 7, 8, 9, 15, 16, 17, 64, 100, 217, 578, 5000, 16368, 40000, int(r.integers(1, 90000))]))))
        if r.random() < 0.3:
            st.append(("D",))
    st.append(("D",))
    return Scenario("soak%d" % seed, nch, st, seed=seed, lo_delay=int(r.choice([2, 3, 216, 100])), cg_delay=int(r.choice([216, 577, 8183])), codes=codes)


# ---- the lock check's scene: one PRN with Doppler, a code offset and 50 bps data, acquired by the oracle and started through the
# kg_acq_chan_start arithmetic after LOCK_T0 clocks (the reset falls on clock 0, where the acquisition's samples begin)
LOCK_SAT, LOCK_DOPPLER, LOCK_TAU, LOCK_CN0, LOCK_MS, LOCK_T0, LOCK_SEED = 0, 1500.0, 300.5, 55.0, 400, 65536, 77
LOCK_DATA = np.random.default_rng(5).integers(0, 2, 64).astype(np.uint8)


def lock_bits():
    from flydog_sdr_gps_amd import prn, sats, trk
    _, t1, t2, _ = sats.SATS[LOCK_SAT]
    chips = prn.cacode(t1, t2)
    return chips, trk.scene_bits(chips, LOCK_MS * CA_EPOCH, LOCK_TAU, LOCK_DOPPLER, LOCK_CN0, LOCK_DATA, seed=LOCK_SEED)


def lock_scenario(bits, start):
    """start: a handoff.ChanStart (or anything with lo_rate, ca_rate, ca_pause)"""
    from flydog_sdr_gps_amd import trk
    return start_acquired("lock", bits, trk.codegen_init(LOCK_SAT), False, start, LOCK_T0, LOCK_MS * CA_EPOCH)


def fault_scenario():
    """channel 0 starts at the lowest accepted code rate with the loop closed at the smallest gains: the first time its summed error
    is negative the loop writes 2^27 - 1, outside the closed form's range; channel 1 is an ordinary channel beside it"""
    steps = _setup(0, CA1, cg=RATE_MIN, gc=(0, 0)) + _setup(1, CA7) + [("R",), ("X", 12 * 32736), ("D",)]
    return Scenario("fault", 2, steps, seed=17)


# ---- signals (tests/test_trk_signal_cpu.py: the model against what a tracking channel must do; tests/test_trk_signal_gpu.py: the
# kernel against the model on the same scenes).  Everything a bar is compared with comes from the scene, nothing from the code under test.
BIN_HZ = 249.755859375              # gps.h: the acquisition's Doppler bin
L1_HZ = 1575.42e6
E1B_MODE = 0x800
NAV_K = {False: 10, True: 30}       # nav bits compared: C/A (one per 20 epochs), E1B (one per epoch)


def sat_data(k):
    """64 seeded data bits of satellite k of a scene (k = 0: the lock check's)"""
    return np.random.default_rng(5 + k).integers(0, 2, 64).astype(np.uint8)


def sat_chips(row):
    from flydog_sdr_gps_amd import prn, sats
    _, t1, t2, kind = sats.SATS[row]
    assert kind != sats.E1B
    return prn.cacode(t1, t2)


def sv(chips, code_phase, doppler_hz, cn0_dbhz, data_bits, boc=False, bit_epochs=20, theta=0.7):
    """one satellite of scene(): the arguments of trk.scene_bits that describe it"""
    return dict(chips=np.asarray(chips, np.uint8), code_phase=float(code_phase), doppler_hz=float(doppler_hz), cn0_dbhz=float(cn0_dbhz),
                data_bits=np.asarray(data_bits, np.int64), boc=bool(boc), bit_epochs=int(bit_epochs), theta=float(theta))


def scene(svs, n, seed, gaps=()):
    """trk.scene_bits generalised: a packed 1-bit IF stream of n clocks holding every satellite of svs.  One noise draw per block comes
    first and the satellites are added to it, in order, before the sign is taken; gaps: (first clock, end clock) ranges in which no
    satellite is present.  With one satellite and no gap the bytes are trk.scene_bits' (the CPU test asserts it)."""
    from flydog_sdr_gps_amd import trk
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n + 7) // 8, np.uint8)
    block = 1 << 20
    for s in range(0, n, block):
        m = min(block, n - s)
        t = np.arange(s, s + m, dtype=np.float64)
        x = rng.standard_normal(m)
        present = None
        for g0, g1 in gaps:
            if g0 < s + m and g1 > s:
                present = np.ones(m) if present is None else present
                present[(t >= g0) & (t < g1)] = 0.0
        for v in svs:
            chips = v["chips"]
            a = np.sqrt(4.0 * 10.0 ** (v["cn0_dbhz"] / 10.0) / trk.FS)
            rate = trk.CPS * (1.0 + v["doppler_hz"] / L1_HZ) / trk.FS
            pos = t * rate + v["code_phase"]
            idx = np.floor(pos).astype(np.int64)
            code = 1.0 - 2.0 * chips[idx % chips.size]
            if v["boc"]:
                code = code * np.where(pos - idx >= 0.5, -1.0, 1.0)
            nbit = (idx // chips.size) // v["bit_epochs"]
            d = 1.0 - 2.0 * v["data_bits"][nbit % v["data_bits"].size]
            term = a * d * code * np.cos(2 * np.pi * ((trk.FC + v["doppler_hz"]) / trk.FS) * t + v["theta"])
            x = x + (term if present is None else term * present)
        b = (x < 0).astype(np.uint8)
        if m % 8:
            b = np.concatenate([b, np.zeros(8 - m % 8, np.uint8)])
        out[s // 8:s // 8 + b.size // 8] = np.packbits(b, bitorder="little")
    return out


def bits_sent(v, n):
    """how many data bits of satellite v a scene of n clocks holds, counted as the lock check counts them: its length in bit times"""
    return n // (16 * v["chips"].size * v["bit_epochs"])


def start_at_bin(ch, word, bin, e1b, code=None, gains=None, pol=None):
    """the command steps (without the reset) of a channel whose NCOs start at the centre of acquisition bin `bin`, with the rates of
    CHANNEL::Start (the kg_acq_chan_start arithmetic) and the gains CHANNEL::Reset sends (gains: another pair of pairs)"""
    from flydog_sdr_gps_amd import handoff, trk
    st = handoff.chan_start(int(e1b), bin, 0, 0.0)
    lo, cg = gains if gains is not None else trk.gains(bool(e1b))
    return ([("S", ch, word)] + ([("C", ch, code)] if code is not None else []) + [("G", ch, NOM), ("l", ch) + lo, ("g", ch) + cg] +
            ([("P", ch, pol)] if pol is not None else []) + [("L", ch, st.lo_rate), ("G", ch, st.ca_rate)])


def start_acquired(name, bits, word, e1b, start, t0, nclocks, codes=()):
    """one channel reset on clock 0 at the nominal code rate and started t0 clocks later, as CHANNEL::Start does, from a
    handoff.ChanStart (or anything with lo_rate, ca_rate, ca_pause): the two rates, then the pause that lines the code up"""
    from flydog_sdr_gps_amd import trk
    lo, cg = trk.gains(bool(e1b))
    steps = [("S", 0, word)] + ([("C", 0, 0)] if e1b else []) + [("G", 0, NOM), ("l", 0) + lo, ("g", 0) + cg, ("R",), ("X", t0),
             ("L", 0, start.lo_rate), ("G", 0, start.ca_rate)] + ([("U", 0, start.ca_pause - 1)] if start.ca_pause else []) + \
            [("X", nclocks - t0), ("D",)]
    return Scenario(name, 1, steps, bits=bits, codes=codes)


def acquire(oracle, chips, bits, e1b):
    """the oracle's Sample() and Correlate() on the first 8192 bytes -> its result dict"""
    from flydog_sdr_gps_amd import sats
    return oracle.correlate(oracle.code_fft(chips, boc=bool(e1b)), oracle.sample_bits(bits[:8192]),
                            limit=sats.E1B_LIMIT if e1b else sats.L1_LIMIT)[0]


def lo_hz(records):
    from flydog_sdr_gps_amd import trk
    return np.array([r[7] for r in records], np.float64) / 2.0 ** 32 * trk.FS - trk.FC


def unlocked_of(records, part):
    """(epochs with ca_unlocked set, epochs) over records[part]"""
    from flydog_sdr_gps_amd import trk
    f = np.array([r[9] for r in records[part]], np.int64)
    return int((f & trk.UNLOCKED).sum()), int(f.size)


def signal_report(records, chan, truth):
    """What one channel's run says about the signal it was given.  records: its epoch records; chan: its GPS_CHAN hex of the last
    dump; truth: dict(doppler_hz, e1b, data_bits (None: not compared), nsent (bits_sent), tail (a slice of the records; None: the
    last quarter), t0 (records before that clock, before an acquired channel's start, are left out)).  ->
      lo_err     the mean LO error in Hz over each eighth of the run
      lo_tail    the mean LO error over the tail
      unlocked   (epochs with ca_unlocked set, epochs) over the tail
      margins    (min (pp - pe) / pp, min (pp - pl) / pp) over the tail
      match      the number of sent bits at which the last K saved nav bits (trk.nav_bits_of, K = 10 for C/A and 30 for E1B) end when
                 they equal the sent ones up to one global sign -- only the scene's last or second-to-last bit is accepted -- else None
    """
    from flydog_sdr_gps_amd import trk
    records = [r for r in records if r[0] >= truth.get("t0", 0)]
    r = np.array(records, np.int64).reshape(len(records), 10)
    n = len(r)
    tail = truth.get("tail") or slice(n - n // 4, n)
    err = lo_hz(records) - truth["doppler_hz"]
    p = r[tail, 1:7].astype(np.float64) ** 2
    pp, pe, pl = p[:, 0] + p[:, 1], p[:, 2] + p[:, 3], p[:, 4] + p[:, 5]
    rep = {"lo_err": [float(e.mean()) for e in np.array_split(err, 8)], "lo_tail": float(err[tail].mean()),
           "unlocked": unlocked_of(records, tail), "margins": (float(((pp - pe) / pp).min()), float(((pp - pl) / pp).min())), "match": None}
    if truth.get("data_bits") is not None:
        K = NAV_K[bool(truth["e1b"])]
        ch = np.frombuffer(bytes.fromhex(chan), trk.chan_dtype)[0]
        got = trk.nav_bits_of(ch, K)
        data = np.asarray(truth["data_bits"], np.uint8)
        for e in (truth["nsent"], truth["nsent"] - 1):
            if e >= K:
                sent = data[np.arange(e - K, e) % data.size]
                if np.array_equal(got, sent) or np.array_equal(got, 1 - sent):
                    rep["match"] = e
                    break
    return rep


def report_line(name, ch, rep):
    return "trk_signal %-18s ch %d  lo_err by eighth %s  tail %+.2f Hz  unlocked %d/%d  margins %.2f/%.2f  nav match %s" % (
        name, ch, " ".join("%+.1f" % e for e in rep["lo_err"]), rep["lo_tail"], rep["unlocked"][0], rep["unlocked"][1],
        rep["margins"][0], rep["margins"][1], rep["match"])


PRN4 = (5 << 4) + 9
QZ_ROW = 32                         # the first QZSS row of sats.SATS
# where the prompt replica of a channel reset on clock 0 stands: half a chip (C/A) or a quarter chip (E1B) behind the early one, so
# a scene whose code is that far before its epoch's start at clock 0 is lined up; the cases start 0.1 chip beside it
CA_TAU0, E1B_TAU0 = 1023 - 0.5 + 0.1, 4092 - 0.25 + 0.05


def _ca_sv(row, k, bin, off, cn0, tau=CA_TAU0):
    return sv(sat_chips(row), tau, bin * BIN_HZ + off, cn0, sat_data(k))


def _e1b_sv(k, bin, off, cn0, tau=E1B_TAU0):
    return sv(e1b_code(1), tau, bin * BIN_HZ + off, cn0, sat_data(k), boc=True, bit_epochs=1)


def _chan(word, bin, sat, e1b=False, gains=None, pol=None):
    """sat: the index into the case's svs of the satellite this channel is on, None: not in the scene"""
    return dict(word=word, bin=bin, sat=sat, e1b=e1b, gains=gains, pol=pol)


def signal_cases():
    """name -> case.  kind "bin": channels started at a bin's centre by start_at_bin; "acquired": one channel acquired by the oracle and
    started by start_acquired t0 clocks after its reset.  epochs: the CPU length, gpu: the GPU length (None: CPU only), both in epochs
    (epoch_clocks) of the case's own code (epochs None: GPU only).  gaps / gpu_gaps: in epochs.  tail: the epochs the bars are taken over (None: the last quarter)."""
    from flydog_sdr_gps_amd import trk
    C = {}

    def add(name, svs, chans, epochs, gpu=None, e1b=False, kind="bin", seed=101, **kw):
        C[name] = dict(name=name, svs=svs, chans=chans, epochs=epochs, gpu=gpu, epoch_clocks=E1B_EPOCH if e1b else CA_EPOCH, kind=kind,
                       seed=seed + len(C), gaps=(), tail=None, pieces=None, max_unlocked=0.0, **kw)

    ca1 = lambda: [_chan(CA1, 6, 0)]
    # 1. C/A carrier pull-in from inside the acquisition bin
    add("ca_pull_p100", [_ca_sv(0, 0, 6, 100.0, 55.0)], ca1(), 1500, gpu=800)
    add("ca_pull_m120", [_ca_sv(0, 0, 6, -120.0, 55.0)], ca1(), 3000)
    add("ca_pull_p60_48", [_ca_sv(0, 0, 6, 60.0, 48.0)], ca1(), 4000)
    C["ca_pull_p60_48"]["max_unlocked"] = 0.01
    C["ca_pull_p100"]["pieces"] = 100001            # the GPU run's X steps
    # 2. E1B: BOC(1,1), quarter-chip latches, the latched memory code, 4 ms epochs, a nav bit per epoch
    e1 = lambda pol=0: [_chan(E1B_MODE | 0, -9, 0, e1b=True, pol=pol)]
    add("e1b_p0", [_e1b_sv(0, -9, 0.0, 50.0)], e1(), 600, e1b=True)
    add("e1b_p30", [_e1b_sv(0, -9, 30.0, 50.0)], e1(), 600, gpu=200, e1b=True)
    # 4. QZSS g2_init, negative Doppler
    add("qzss_m1000", [_ca_sv(QZ_ROW, 0, -4, 25.0, 55.0)], [_chan(trk.codegen_init(QZ_ROW), -4, 0)], 600)
    # 5. the handoff's edges
    add("edge_ca_tau0", [_ca_sv(0, 0, 6, 20.0, 55.0, tau=0.1)], [_chan(CA1, None, 0)], 600, kind="acquired")
    add("edge_ca_tau_end", [_ca_sv(0, 0, -13, -25.0, 55.0, tau=1022.7)], [_chan(CA1, None, 0)], 600, kind="acquired")
    add("edge_e1b_tau0", [_e1b_sv(0, 4, -15.0, 50.0, tau=0.1)], [_chan(E1B_MODE | 0, None, 0, e1b=True)], 200, e1b=True, kind="acquired")
    add("edge_e1b_tau1777", [_e1b_sv(0, -9, 20.0, 50.0, tau=1777.25)], [_chan(E1B_MODE | 0, None, 0, e1b=True)], 200, gpu=150, e1b=True,
        kind="acquired")
    # 6. loss of signal: 500 epochs of PRN 1, then noise
    add("loss", [_ca_sv(0, 0, 6, 0.0, 55.0)], ca1(), 900)
    C["loss"]["tail"] = slice(300, 500)
    C["loss"]["gaps"] = ((500, 900),)
    C["loss"].update(gpu=500, gpu_gaps=((300, 500),))
    # 7. a channel on PRN 1, a scene holding PRN 7 only
    add("wrong_prn", [_ca_sv(6, 1, 6, 0.0, 55.0)], [_chan(CA1, 6, None)], 400)
    C["wrong_prn"]["tail"] = slice(200, None)
    # 8. a bank on one stream: four satellites, six channels (PRN 4 is absent; PRN 1 twice, once with the LO gain lowered by one)
    def bank(offs, cn0):
        svs = [_ca_sv(0, 0, 6, offs[0], cn0[0]), _ca_sv(6, 1, -13, offs[1], cn0[1]), _ca_sv(QZ_ROW, 2, 2, offs[2], cn0[2]),
               _e1b_sv(3, -9, offs[3], cn0[3])]
        chans = [_chan(CA1, 6, 0), _chan(CA7, -13, 1), _chan(trk.codegen_init(QZ_ROW), 2, 2), _chan(E1B_MODE | 0, -9, 3, e1b=True, pol=0),
                 _chan(PRN4, 6, None), _chan(CA1, 6, 0, gains=trk.gains(False, adj_lo=-1))]
        return svs, chans
    add("bank", *bank((40.0, -55.0, 80.0, 20.0), (52.0, 50.0, 52.0, 50.0)), 1500)
    add("bank_gpu", *bank((25.0, -25.0, 28.0, 20.0), (55.0,) * 4), None, gpu=600)
    return C



def case_scenario(case, gpu=False, oracle=None, epochs=None):
    """the case at its CPU length (gpu: at its GPU length; epochs: at another one) -> (Scenario, truth per channel (None: its satellite is not in the scene), acquisition (kind "acquired": (the oracle's result,
    the ChanStart)))"""
    from flydog_sdr_gps_amd import handoff, trk
    n = (epochs or case["gpu" if gpu else "epochs"]) * case["epoch_clocks"]
    gaps = tuple((a * case["epoch_clocks"], b * case["epoch_clocks"]) for a, b in (case.get("gpu_gaps", case["gaps"]) if gpu else case["gaps"]))
    bits = scene(case["svs"], n, case["seed"], gaps)
    codes = [e1b_code(1)] if any(c["e1b"] for c in case["chans"]) else []
    truths = []
    for c in case["chans"]:
        v = None if c["sat"] is None else case["svs"][c["sat"]]
        truths.append(None if v is None else dict(doppler_hz=v["doppler_hz"], e1b=c["e1b"], data_bits=None if gaps else v["data_bits"],
                                                  nsent=bits_sent(v, n), tail=case["tail"],
                                                  t0=LOCK_T0 if case["kind"] == "acquired" else 0))
    if case["kind"] == "acquired":
        c, v = case["chans"][0], case["svs"][0]
        acq = acquire(oracle, v["chips"], bits, c["e1b"])
        start = handoff.chan_start(int(c["e1b"]), acq["dop"], acq["idx"] * handoff.DECIM, LOCK_T0 / trk.FS)
        return start_acquired(case["name"], bits, c["word"], c["e1b"], start, LOCK_T0, n, codes=codes), truths, (acq, start)
    steps = []
    for ch, c in enumerate(case["chans"]):
        steps += start_at_bin(ch, c["word"], c["bin"], c["e1b"], code=0 if c["e1b"] else None, gains=c["gains"], pol=c["pol"])
    steps += [("R",)] + (_pieces(n, (case["pieces"],)) if case["pieces"] else [("X", n)]) + [("D",)]
    return Scenario(case["name"], len(case["chans"]), steps, bits=bits, codes=codes), truths, None
