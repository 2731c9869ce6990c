"""What the IQ-display tests share (tests/test_iqd_cpu.py, test_iqd_gpu.py, test_containment_iqd_gpu.py, tools/make_ref_iqd_golden.py):
the seeded pool of complex samples that tests/golden/iqd_ref.npz was made from (the file holds the pool's digest, not the samples), the
command / block scripts, the parser of what the reference harness and the host driver write, the host driver
tools/iqd_host_driver.cpp (csrc/kg_iqd.h compiled for the host with the reference's flags) and the runner of a script on the device
object.

Amplitudes stay below 3e4 and no sample is NaN or infinite: overflow inside the power and NaN input are outside the contract."""
import os

import numpy as np

from . import script_common
from .script_common import digest  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 0x49514450
FS = 12000.0
OFFSET_HZ = 37.0                                 # the carrier of the PSK segments
MSK_OFFSET_HZ = 3.0                              # and of the MSK segment
RING, MAX_NS = 16384, 512
SEG = 40 * 512                                   # samples a pool segment
MSK_BLOCKS = 400                                 # the MSK segment is longer: its narrow loops take seconds to settle
SEGMENTS = ("cw", "bpsk", "qpsk", "psk8", "noise", "silence_noise", "msk")
AT = {n: i * SEG for i, n in enumerate(SEGMENTS)}
POOL = AT["msk"] + MSK_BLOCKS * 512
STATE_BYTES = 44 + 24 + 84 + 2 * RING * 8 + 2 * RING * 4 + RING * 2


def pool():
    """-> complex64 [POOL].  One generator, drawn in a fixed order."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    t = np.arange(SEG) / FS
    car = 2 * np.pi * OFFSET_HZ * t + 0.4
    out = {}

    def noise(sigma):
        return sigma * (rng.standard_normal(SEG) + 1j * rng.standard_normal(SEG))

    def psk(m, baud):
        sym = rng.integers(0, m, SEG // int(FS / baud) + 1)
        return 2 * np.pi * sym[(np.arange(SEG) // int(FS / baud))] / m

    out["cw"] = 9000.0 * np.exp(1j * car) + noise(150.0)
    out["bpsk"] = 8000.0 * np.exp(1j * (car + psk(2, 100))) + noise(200.0)
    out["qpsk"] = 12000.0 * np.exp(1j * (car + psk(4, 100))) + noise(150.0)
    out["psk8"] = 20000.0 * np.exp(1j * (car + psk(8, 50))) + noise(100.0)
    per, nm = int(FS / 200), MSK_BLOCKS * 512    # MSK at 200 baud: the phase ramps +-pi/2 a symbol
    bits = rng.integers(0, 2, nm // per + 1) * 2 - 1
    ramp = np.cumsum(bits[np.arange(nm) // per] * (np.pi / 2) / per)
    out["msk"] = (10000.0 * np.exp(1j * (2 * np.pi * MSK_OFFSET_HZ * np.arange(nm) / FS + 0.4 + ramp))
                  + 100.0 * (rng.standard_normal(nm) + 1j * rng.standard_normal(nm)))
    out["noise"] = noise(3000.0)
    s = noise(2500.0)
    s[:1300] = 0                                 # leading silence, ending inside a block
    out["silence_noise"] = s
    p = np.concatenate([out[n] for n in SEGMENTS]).astype(np.complex64)
    assert np.isfinite(p.view(np.float32)).all() and np.abs(p).max() <= 3e4
    return p


def load():
    return np.load(os.path.join(GOLD, "iqd_ref.npz"))


# ---- the scripts.  N | R run rate | G gain | P points | M pll_mode arg | W bandwidth | D draw | Y display_mode | C | B inst ns off
def _B(seg, first, n, ns=512, inst=0):
    return ["B %d %d %d" % (inst, ns, AT[seg] + ns * (first + k)) for k in range(n)]


HEAD = ["N", "R 1 12000"]
MSK_SETTLED = 30                                 # so many of the MSK script's last text messages are held to the offset, not one


def pll_offset(ints):
    """the offset a script's final df is held to, from its END STATE (parse()'s "ints"): None with the PLL off.  Every script that ends
    with a PLL on is a PLL script; none is listed by hand."""
    exponent, msk_mode = int(ints[2]), int(ints[3])
    return MSK_OFFSET_HZ if msk_mode else (OFFSET_HZ if exponent else None)


FULL = ("pll_off", "exp1_cw", "points_change", "both_instances", "silence_auto", "silence_auto_density")                                       # rows kept in full


def scripts():
    s = {
        "pll_off": HEAD + ["M 0 0"] + _B("noise", 0, 8),
        "exp1_cw": HEAD + ["M 1 1", "P 300", "G 52"] + _B("cw", 0, 16),
        "exp2_bpsk_density": HEAD + ["M 1 2", "P 512", "D 1"] + _B("bpsk", 0, 20),
        "exp4_qpsk": HEAD + ["M 1 4", "W 20", "G 50"] + _B("qpsk", 0, 30),
        "exp8_psk8_carrier": HEAD + ["M 1 8", "W 30", "P 5", "Y 1", "G 91"] + _B("psk8", 0, 30),
        # each of the two PLLs sees its tone half of the time and the other tone, a turn a symbol away, the rest: df carries b[0] * ud of
        # that sawtooth, about +-0.78 Hz per Hz of bandwidth.  At 1 Hz the loops take some 190 blocks to pull in; the messages behind that
        # all stay within 1 Hz of the offset
        "msk": HEAD + ["M 2 200", "W 1"] + _B("msk", 0, MSK_BLOCKS),
        # leading silence under auto gain: ama == 0, the scale is inf, 0 * inf is NaN, the byte 255; draw switched mid-lap
        "silence_auto": HEAD + ["M 0 0", "P 300"] + _B("silence_noise", 0, 4) + ["D 1"] + _B("silence_noise", 4, 4),
        "silence_auto_density": HEAD + ["M 0 0", "P 300", "D 1"] + _B("silence_noise", 0, 8),
        "points_1": HEAD + ["M 0 0", "P 1"] + _B("noise", 0, 10, ns=170) + ["D 1"] + _B("noise", 10, 10, ns=170),
        "points_16384": HEAD + ["M 0 0", "P 16384", "G 50"] + _B("noise", 0, 33) + ["D 1"] + _B("cw", 0, 35),
        # points lowered below the ring position, raised mid-lap (stale entries of the longer lap are sent again), draw = 2: nothing
        # is processed, nsamp goes on
        "points_change": HEAD + ["M 0 0", "P 300", "G 48"] + _B("noise", 0, 1) + ["P 100"] + _B("noise", 1, 1) + ["P 700"] + _B("noise", 2, 2)
                         + ["P 5"] + _B("noise", 4, 1, ns=170) + ["D 2"] + _B("noise", 5, 2) + ["D 0", "P 1024"] + _B("noise", 7, 3),
        "clear_run_mid": HEAD + ["M 1 2", "P 512"] + _B("bpsk", 0, 6) + ["C"] + _B("bpsk", 6, 5) + ["R 1 12000"] + _B("bpsk", 11, 3) + ["R 0 12000"]
                         + _B("bpsk", 14, 2) + ["R 1 12000"] + _B("bpsk", 16, 20),
        # both instances share the one PLL (and, in density mode, the map): consecutive blocks of the carrier alternate between them
        "both_instances": HEAD + ["M 1 1", "P 512", "G 38"] + [l for k in range(8) for l in (_B("cw", 2 * k, 1) + _B("cw", 2 * k + 1, 1, inst=1))] + ["D 1"]
                          + [l for k in range(8, 14) for l in (_B("cw", 2 * k, 1) + _B("cw", 2 * k + 1, 1, inst=1))],
        "density_5_1024": HEAD + ["M 0 0", "D 1", "P 5"] + _B("noise", 0, 2, ns=170) + ["P 1024"] + _B("noise", 1, 8),
        "exp3_and_mode3": HEAD + ["M 1 3", "M 3 7", "W 15", "G 52"] + _B("cw", 0, 12) + ["M 1 0"] + _B("cw", 12, 2) + ["M 1 3"] + _B("cw", 14, 16),
        "ns7": HEAD + ["M 1 1", "W 20", "P 5", "G 52"] + _B("cw", 0, 870, ns=7),
        "rate_20250": ["N", "R 1 20250", "M 0 0", "P 1024"] + _B("noise", 0, 11),
    }
    return s


def nblocks(lines):
    return sum(1 for l in lines if l[0] == "B")


def parse(raw, nblk):
    """out.bin of the reference harness or the host driver -> dict: nrows int32 [blocks], cmd / len int32 [rows], rows (list of uint8
    arrays), sent int32 [blocks], status (records of the sent blocks), and the final state"""
    from flydog_sdr_gps_amd.iqd import status_dtype
    at, nrows, cmd, ln, rows, sent, status = 0, [], [], [], [], [], []
    for _ in range(nblk):
        n = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        at += 4
        nrows.append(n)
        for _ in range(n):
            c, l = (int(v) for v in np.frombuffer(raw[at:at + 8], np.int32))
            cmd.append(c)
            ln.append(l)
            rows.append(np.frombuffer(raw[at + 8:at + 8 + l], np.uint8))
            at += 8 + l
        s = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        at += 4
        sent.append(s)
        if s:
            status.append(np.frombuffer(raw[at:at + 24], status_dtype)[0])
            at += 24
    assert len(raw) - at == STATE_BYTES, (len(raw), at)
    out = {"nrows": np.array(nrows, np.int32), "cmd": np.array(cmd, np.int32), "len": np.array(ln, np.int32), "rows": rows,
           "sent": np.array(sent, np.int32), "status": np.array(status, status_dtype)}
    out["ints"] = np.frombuffer(raw[at:at + 44], np.int32).copy()
    out["floats"] = np.frombuffer(raw[at + 44:at + 68], np.float32).copy()
    out["pll"] = np.frombuffer(raw[at + 68:at + 152], np.float32).reshape(3, 7).copy()
    at += 152
    out["iq"] = np.frombuffer(raw[at:at + 2 * RING * 8], np.uint8).copy()
    out["plot"] = np.frombuffer(raw[at + 2 * RING * 8:at + 2 * RING * 12], np.uint8).copy()
    out["map"] = np.frombuffer(raw[at + 2 * RING * 12:], np.uint8).copy()
    return out


def stream(got):
    """the rows as one byte string: per row cmd, len and the bytes"""
    parts = []
    for c, l, r in zip(got["cmd"], got["len"], got["rows"]):
        parts += [np.array([c, l], np.int32).tobytes(), np.asarray(r, np.uint8).tobytes()]
    return b"".join(parts)


def golden_of(got, full):
    """what the golden file keeps of a reference run"""
    out = {"nrows": got["nrows"], "sent": got["sent"], "status": got["status"].view(np.uint8), "ints": got["ints"], "floats": got["floats"],
           "pll": got["pll"], "stream_sha": np.frombuffer(digest(stream(got)), np.uint8), "cmd": got["cmd"], "len": got["len"],
           "iq_sha": np.frombuffer(digest(got["iq"]), np.uint8), "plot_sha": np.frombuffer(digest(got["plot"]), np.uint8),
           "map_sha": np.frombuffer(digest(got["map"]), np.uint8)}
    allb = np.concatenate([np.asarray(r, np.uint8) for r in got["rows"]]) if got["rows"] else np.zeros(0, np.uint8)
    out["edge_bytes"] = np.array([int(((allb == 0) | (allb == 255)).sum()), allb.size], np.int64)
    if full:
        out["rows"] = allb
    return out


def check_against_golden(g, name, got):
    """equality on everything the golden keeps: rows (bytes, cmd, length, the block they went out behind), the status records and
    which were sent, the end state bit for bit, the rings by digest"""
    from flydog_sdr_gps_amd.iqd import status_dtype
    k = "s_%s_" % name
    assert np.array_equal(got["nrows"], g[k + "nrows"]), (name, "rows per block")
    assert np.array_equal(got["cmd"], g[k + "cmd"]) and np.array_equal(got["len"], g[k + "len"]), (name, "cmd / len")
    assert np.array_equal(got["sent"], g[k + "sent"]), (name, "sent", got["sent"], g[k + "sent"])
    want = g[k + "status"].view(status_dtype)
    assert got["status"].size == want.size, name
    for f in ("cmaI", "cmaQ", "df", "phase"):
        a, b = np.ascontiguousarray(got["status"][f]), np.ascontiguousarray(want[f])
        assert a.tobytes() == b.tobytes(), (name, "status", f, a[:4], b[:4])
    if k + "rows" in g.files:
        allb = np.concatenate([np.asarray(r, np.uint8) for r in got["rows"]]) if got["rows"] else np.zeros(0, np.uint8)
        bad = np.flatnonzero(allb != g[k + "rows"])
        assert bad.size == 0, (name, "first differing row byte", int(bad[0]), int(allb[bad[0]]), int(g[k + "rows"][bad[0]]), int(bad.size))
    assert digest(stream(got)) == bytes(g[k + "stream_sha"]), (name, "rows")
    assert np.array_equal(got["ints"], g[k + "ints"]), (name, "state", got["ints"], g[k + "ints"])
    assert got["floats"].tobytes() == g[k + "floats"].tobytes(), (name, "gain, fs, bandwidth, cma, ama", got["floats"], g[k + "floats"])
    assert got["pll"].tobytes() == g[k + "pll"].tobytes(), (name, "PLLs", got["pll"], g[k + "pll"])
    for a in ("iq", "plot", "map"):
        assert digest(got[a]) == bytes(g[k + a + "_sha"]), (name, a)


# ---- the host driver
def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "iqd_host_driver")


def run_script_exe(exe, lines, samples, tmpdir, expect=0):
    out = script_common.run_script(exe, [], lines, samples, np.complex64, tmpdir, expect)
    return parse(out, nblocks(lines)) if expect == 0 else None


# ---- a script on the device object
def apply_command(q, ch, l):
    """-> whether the receiver is registered after it (None: unchanged)"""
    op, a = l[0], l[2:].split()
    if op == "N":
        q.init(ch)
        return False
    if op == "R":
        q.set_run(ch, int(a[0]), float(a[1]))
        return int(a[0]) != 0
    if op == "G":
        q.set_gain(ch, int(a[0]))
    elif op == "P":
        q.set_points(ch, int(a[0]))
    elif op == "M":
        q.set_pll_mode(ch, int(a[0]), int(a[1]))
    elif op == "W":
        q.set_pll_bandwidth(ch, float(np.float32(a[0])))
    elif op == "D":
        q.set_draw(ch, int(a[0]))
    elif op == "Y":
        q.set_display_mode(ch, int(a[0]))
    elif op == "C":
        q.clear(ch)
    return None


def state_of(q, ch):
    info, iq, plot, mp = q.state(ch, arrays=True)
    ints = np.array([info[f] for f in ("points", "nsamp", "exponent", "msk_mode", "msk_baud", "draw", "display_mode", "maN", "maNsend")]
                    + [info["ring"][0], info["ring"][1]], np.int32)
    floats = np.array([info[f] for f in ("gain", "fs", "pll_bandwidth", "cmaI", "cmaQ", "ama")], np.float32)
    return {"ints": ints, "floats": floats, "pll": info["pll"].copy(), "iq": iq.view(np.uint8).reshape(-1), "plot": plot.reshape(-1), "map": mp.reshape(-1)}


def run_script_dev(q, ctx, lines, samples, ch=0, cuts=None, merge=False):
    """Runs a script on channel ch of q (an IqDisplay): consecutive B lines of one ns are ONE kg_iqd_process_dev call -- one entry per
    line, or with `merge` one entry per run of lines of one instance -- cut where a command stands between them and behind the block
    counts in `cuts` (block numbers of the script).  -> the keys of parse(), plus "calls" and "samp" (per row)."""
    from flydog_sdr_gps_amd.iqd import status_dtype
    nb = nblocks(lines)
    nrows, sent, status = np.zeros(nb, np.int32), np.zeros(nb, np.int32), np.zeros(nb, status_dtype)
    cmd, ln, samp, rows = [], [], [], []
    pend, seen, calls, registered = [], 0, 0, False
    cuts = set(cuts or ())

    def flush():
        nonlocal calls
        if not pend:
            return
        ns = pend[0][1]
        ents = []                                    # [instance, [block numbers], [pool offsets]]
        for inst, _, off, blk in pend:
            if merge and ents and ents[-1][0] == inst:
                ents[-1][1].append(blk)
                ents[-1][2].append(off)
            else:
                ents.append([inst, [blk], [off]])
        stride = ns * max(len(e[1]) for e in ents)
        host = np.zeros((len(ents), stride), np.complex64)
        for i, e in enumerate(ents):
            host[i, :ns * len(e[1])] = np.concatenate([samples[o:o + ns] for o in e[2]])
        cap = (ns * len(pend) + 2 * RING) * 4       # a row's samples, and a first row of each instance behind a change of points
        d_iq, d_rows, d_st = ctx.alloc(host.nbytes), ctx.alloc(cap), ctx.alloc(24 * len(pend))
        try:
            ctx.upload(d_iq, host)
            m, snt = q.process_dev([ch] * len(ents), [len(e[1]) for e in ents], [e[0] for e in ents], ns, d_iq, stride, d_rows, cap, d_st, len(pend),
                                   ns * len(pend))
            ctx.sync()
            used = int(m["off"][-1] + m["len"][-1]) if m.size else 0
            hrows, hst = np.zeros(max(used, 1), np.uint8), np.zeros(len(pend), status_dtype)
            ctx.download(d_rows, hrows)
            ctx.download(d_st, hst)
        finally:
            for p in (d_iq, d_rows, d_st):
                ctx.free(p)
        at = 0
        for r in m:
            assert r["ch"] == ch and r["off"] == at, ("rows are packed back to back", r, at)
            blk = ents[r["ent"]][1][r["blk"]]
            nrows[blk] += 1
            cmd.append(int(r["cmd"])); ln.append(int(r["len"])); samp.append(int(r["samp"]))
            rows.append(hrows[at:at + r["len"]].copy())
            at += int(r["len"])
        k = 0
        for e in ents:
            for blk in e[1]:
                sent[blk], status[blk] = snt[k], hst[k]
                k += 1
        calls += 1
        pend.clear()

    for l in lines:
        if l[0] == "B":
            _, inst, ns, off = l.split()
            if registered:
                if pend and pend[0][1] != int(ns):
                    flush()
                pend.append((int(inst), int(ns), int(off), seen))
            seen += 1
            if seen in cuts:
                flush()
            continue
        flush()
        r = apply_command(q, ch, l)
        if r is not None:
            registered = r
    flush()
    out = {"nrows": nrows, "cmd": np.array(cmd, np.int32), "len": np.array(ln, np.int32), "rows": rows, "sent": sent, "status": status[sent != 0],
           "status_all": status, "samp": np.array(samp, np.int32), "calls": calls}
    out.update(state_of(q, ch))
    return out
