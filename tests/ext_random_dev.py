"""Seeded random command scripts (tests/ext_random.py) on the device, for tests/test_{iqd,lorc,fftext,fax,cw}_gpu.py: the comparison of
a device result with the host driver's in full, the random partition of one script into calls, and three scripts side by side on
three channels of one object (iqd, fftext: fed from host arrays call by call or from one device-resident buffer; lorc, fax and cw have
their lock-step runners in tests/test_lorc_gpu.py, tests/fax_common.py and tests/cw_common.py).  The schedule of the calls is decided
ahead of the run, so what it reaches is checked without a GPU."""
import numpy as np

from . import cw_common as cwc
from . import fax_common as fxc
from . import fftext_common as fc
from . import iqd_common as ic
from . import lorc_common as lc
from .ext_random import BASE, COMMON, NSEED, PARTITION, SCRIPT, SHAPES, _pick, _rng, same

# A device result (the keys of the module's parse(), from run_script_dev or from run_plan below) against the host driver's, in full: a
# failure names the first differing row or element.
def iqd_same(dev, host, *what):
    for k in ("nrows", "cmd", "len", "sent"):
        same(dev[k], host[k], *what + (k,))
    assert len(dev["rows"]) == len(host["rows"]), what
    for i, (a, b) in enumerate(zip(dev["rows"], host["rows"])):
        same(a, b, *what + ("row %d" % i,))
    for f in ("cmaI", "cmaQ", "df", "phase"):
        same(dev["status"][f], host["status"][f], *what + ("status", f))
    for k in ("ints", "floats", "pll", "iq", "plot", "map"):
        same(dev[k], host[k], *what + ("end state", k))


def lorc_same(dev, host, *what):
    for k in ("nrows", "samp", "ch", "cmd", "len"):
        same(dev[k], host[k], *what + (k,))
    for i, (a, b) in enumerate(zip(dev["rows"], host["rows"])):
        same(a, b, *what + ("row %d" % i,))
    for f in ("i_srate", "redraw_legend", "srate"):
        same(dev["scalars"][f], host["scalars"][f], *what + ("end state", f))
    for c in range(2):
        for f in lc.chan_dtype.names:
            same(dev["scalars"]["ch"][c][f], host["scalars"]["ch"][c][f], *what + ("end state, chain %d" % c, f))
    same(np.asarray(dev["avg"], np.float32), np.asarray(host["avg"], np.float32), *what + ("avg",))


def fftext_same(dev, host, *what):
    for k in ("sent", "bins"):
        same(dev[k], host[k], *what + (k,))
    assert dev["rows"].shape == host["rows"].shape, what
    bad = np.argwhere(dev["rows"] != host["rows"])
    assert bad.size == 0, what + ("first differing byte (row, column)", bad[0].tolist(), int(dev["rows"][tuple(bad[0])]), int(host["rows"][tuple(bad[0])]))
    for k in ("run", "instance", "nbins", "reset"):
        assert int(dev[k]) == int(host[k]), what + (k, dev[k], host[k])
    for k, t in (("fft_scale", np.float32), ("spectrum_scale", np.float32), ("fi", np.float64), ("fft_sec", np.float64), ("time", np.float64)):
        same(np.array([dev[k]], t), np.array([host[k]], t), *what + ("end state", k))
    same(np.asarray(dev["ncma"], np.int32), host["ncma"], *what + ("ncma",))
    same(np.asarray(dev["pwr"], np.float32), host["pwr"], *what + ("sums",))


def fax_same(dev, host, *what):
    same(dev["nlines"], host["nlines"], *what + ("lines per block",))
    for f in fxc.rec_dtype.names:
        if f != "blk":                                                     # the block of the push; nlines places a line in the script
            same(dev["recs"][f], host["recs"][f], *what + ("line", f))
    assert len(dev["rows"]) == len(host["rows"]), what + ("rows", len(dev["rows"]), len(host["rows"]))
    for i, (a, b) in enumerate(zip(dev["rows"], host["rows"])):
        same(a, b, *what + ("row %d" % i,))
    for f in fxc.info_dtype.names:
        if f != "pad":
            a, b = np.asarray(dev["info"][f]), np.asarray(host["info"][f])
            assert fxc._same_float(a, b) if a.dtype.kind == "f" else np.array_equal(a, b), what + ("end state", f, a, b)
    for k in ("samples", "demod", "prev", "out"):
        same(dev[k], host[k], *what + ("end state", k))


def cw_same(dev, host, *what):
    same(dev["nev"], host["nev"], *what + ("events per block",))
    for f in cwc.ev_dtype.names:
        same(dev["evs"][f], host["evs"][f], *what + ("event", f))
    for f in cwc.info_dtype.names:
        same(dev["info"][f], host["info"][f], *what + ("end state", f))


SAME = {"iqd": iqd_same, "lorc": lorc_same, "fftext": fftext_same, "fax": fax_same, "cw": cw_same}
PUSHES = (1, 2, 7, 64, 256)                      # blocks a push of a fax or cw partition: 256 is the most kg_fax_push and kg_cw_push take


def partition(mod, seed, nb):
    """how the seed's script is cut into calls, from a generator of its own: (cuts behind block numbers, merge); for lorc max_blocks;
    for fax and cw the `cuts` of script_steps, which draws the blocks of the next push from PUSHES"""
    rng = _rng(mod, seed, partition=True)
    if mod == "lorc":
        return _pick(rng, (1, 2, 5, 48))
    if mod in ("fax", "cw"):
        return lambda: _pick(rng, PUSHES)
    p = _pick(rng, (0.02, 0.1, 0.3))
    return {b for b in range(1, nb) if rng.random() < p}, bool(rng.integers(2))


# ---- three scripts side by side on three channels of one object (iqd, fftext; lorc has its lock-step runner in tests/test_lorc_gpu.py)
def _items(mod, lines):
    """("cmd", line) / ("blk", instance, ..., block number): iqd (instance, ns, pool offset), fftext (instance, pool row)"""
    out, seen = [], 0
    for l in lines:
        if l[0] == "B":
            out.append(("blk",) + tuple(int(v) for v in l.split()[1:]) + (seen,))
            seen += 1
        else:
            out.append(("cmd", l))
    return out


def plan_side_by_side(mod, scripts, rng, most=4):
    """The calls of scripts[c] run in lock step, decided ahead of the run (nothing of it depends on what the device answers).  Every
    round each script takes its commands up to its next block, then ONE call carries every script whose next blocks share the round's
    key -- iqd: ns; fftext: the sample rate, which is the object's and is taken up at a channel's reset.  The round's key is the one
    most scripts wait with; each takes a random number of consecutive blocks, up to `most`.  A script alone in its call takes all its
    blocks up to its next command: the calls are spent where scripts share them, and the cutting of one script's run of blocks into
    calls is left to the partition tests.  A script's blocks become entries of one block, or (drawn per script and call) of a run of
    blocks of one instance; the entries of the scripts are shuffled into each other and stand between entries of no block, so that an
    entry's samples are not at the row of its position among the entries that have some.
    -> steps ("cmd", c, line) / ("call", key, [(c, instance, [block items]) ...])"""
    items = [_items(mod, s) for s in scripts]
    at, on, rate, steps = [0] * len(items), [False] * len(items), [None] * len(items), []
    while True:
        for c, it in enumerate(items):
            while at[c] < len(it):
                if it[at[c]][0] == "cmd":
                    l = it[at[c]][1]
                    steps.append(("cmd", c, l))
                    if mod == "iqd" and l[0] in "NR":
                        on[c] = l[0] == "R" and int(l.split()[1]) != 0
                    if mod == "fftext" and l[0] == "R":
                        rate[c] = float(l[2:])
                elif mod == "iqd" and not on[c]:
                    pass                                                   # not registered: the block is not handed over
                else:
                    break
                at[c] += 1
        ready = [c for c, it in enumerate(items) if at[c] < len(it)]
        if not ready:
            return steps
        key_of = (lambda c: items[c][at[c]][2]) if mod == "iqd" else (lambda c: rate[c])
        keys = [key_of(c) for c in ready]
        key = _pick(rng, [k for k in keys if keys.count(k) == max(keys.count(v) for v in keys)])       # the one most scripts wait with
        queues = []
        for c in ready:
            if key_of(c) != key:
                continue
            # a script alone in its call takes all the blocks up to its next command: the calls are spent where scripts share them
            it, n, lim = items[c], 0, int(rng.integers(1, most + 1)) if keys.count(key) > 1 else len(items[c])
            while n < lim and at[c] + n < len(it) and it[at[c] + n][0] == "blk" and (mod != "iqd" or it[at[c] + n][2] == key):
                n += 1
            q, merge = [], bool(rng.integers(2))
            for b in it[at[c]:at[c] + n]:
                if merge and q and q[-1][1] == b[1]:
                    q[-1][2].append(b)
                else:
                    q.append((c, b[1], [b]))
            queues.append(q)
            at[c] += n
        ents = []
        while any(queues):
            q = _pick(rng, [q for q in queues if q])
            if rng.random() < 0.2:
                ents.append((q[0][0], 0, []))
            ents.append(q.pop(0))
        steps.append(("call", key, ents))


def _layout(steps, width, rng):
    """where every call's samples stand in ONE buffer: (first element, stride) per call -- a stride larger than the longest entry --
    and the elements in all"""
    where, at = [], int(rng.integers(1, 9))
    for s in steps:
        if s[0] == "call":
            stride = width(s) * max(len(e[2]) for e in s[2]) + int(rng.integers(1, 64))
            where.append((at, stride))
            at += stride * len(s[2])
    return where, at


def iqd_run_plan(q, ctx, steps, chans, scripts, samples, resident=False, rng=None):
    """steps (plan_side_by_side) on channels chans[c] of q.  resident: every call's samples are uploaded ONCE, ahead of the first
    call, into one device buffer filled with NaN (a sample read from outside an entry's blocks would show), and no copy, to or from the
    device, stands between two calls: rows and status records of all calls go to one buffer each and are read behind the last call.
    -> (per script the keys of iqd_common.run_script_dev, calls, calls that carried more than one script)"""
    from flydog_sdr_gps_amd.iqd import status_dtype
    n = len(scripts)
    nb = [ic.nblocks(s) for s in scripts]
    nrows, sent, stat_at = [np.zeros(b, np.int32) for b in nb], [np.zeros(b, np.int32) for b in nb], [np.zeros(b, np.int64) for b in nb]
    heads = [[] for _ in range(n)]                                         # cmd, len, samp, where the row's bytes are
    calls = [s for s in steps if s[0] == "call"]
    nblocks = sum(len(e[2]) for s in calls for e in s[2])
    # a row of `len` bytes needs len / 4 (density: len / 2) samples of its instance, but for the first one behind a command: 4 bytes a
    # sample and two full rings a command bound what a script can send
    cap = sum(4 * sum(int(l.split()[2]) for l in s if l[0] == "B") + 8 * ic.RING * (1 + sum(l[0] != "B" for l in s)) for s in scripts) + 16 * len(calls)
    d_rows, d_st, d_iq = ctx.alloc(cap), ctx.alloc(24 * max(nblocks, 1)), None
    at_rows = at_st = shared = k = 0
    try:
        if resident:
            where, total = _layout(steps, lambda s: s[1], rng)
            host = np.full(total, np.nan + 1j * np.nan, np.complex64)
            for (base, stride), s in zip(where, calls):
                for i, e in enumerate(s[2]):
                    for j, b in enumerate(e[2]):
                        host[base + i * stride + j * s[1]:][:s[1]] = samples[b[3]:b[3] + s[1]]
            d_iq = ctx.alloc(host.nbytes)
            ctx.upload(d_iq, host)
        for s in steps:
            if s[0] == "cmd":
                ic.apply_command(q, chans[s[1]], s[2])
                continue
            _, ns, ents = s
            nblk = [len(e[2]) for e in ents]
            if resident:
                base, stride = where[k]
                d_in = d_iq + 8 * base
            else:
                stride = ns * max(nblk)
                host = np.zeros((len(ents), stride), np.complex64)
                for i, e in enumerate(ents):
                    for j, b in enumerate(e[2]):
                        host[i, j * ns:(j + 1) * ns] = samples[b[3]:b[3] + ns]
                d_in = ctx.alloc(host.nbytes)
                ctx.upload(d_in, host)
            try:
                m, snt = q.process_dev([chans[e[0]] for e in ents], nblk, [e[1] for e in ents], ns, d_in, stride, d_rows + at_rows, cap - at_rows,
                                       d_st + 24 * at_st, sum(nblk), ns * sum(nblk))
            finally:
                if not resident:
                    ctx.sync()
                    ctx.free(d_in)
            for r in m:
                c, e = chans.index(int(r["ch"])), ents[r["ent"]]
                assert e[0] == c
                nrows[c][e[2][r["blk"]][4]] += 1
                heads[c].append((int(r["cmd"]), int(r["len"]), int(r["samp"]), at_rows + int(r["off"])))
            j = 0
            for e in ents:
                for b in e[2]:
                    sent[e[0]][b[4]], stat_at[e[0]][b[4]] = snt[j], at_st + j
                    j += 1
            at_rows = (at_rows + (int(m["off"][-1] + m["len"][-1]) if m.size else 0) + 15) & ~15
            at_st += j
            shared += len({e[0] for e in ents if e[2]}) > 1
            k += 1
        ctx.sync()
        hrows, hst = np.zeros(max(at_rows, 1), np.uint8), np.zeros(max(at_st, 1), status_dtype)
        ctx.download(d_rows, hrows)
        ctx.download(d_st, hst)
    finally:
        for p in (d_rows, d_st, d_iq):
            if p:
                ctx.free(p)
    out = []
    for c in range(n):
        h = np.array(heads[c], np.int64).reshape(-1, 4)
        got = {"nrows": nrows[c], "cmd": h[:, 0].astype(np.int32), "len": h[:, 1].astype(np.int32), "samp": h[:, 2].astype(np.int32),
               "rows": [hrows[o:o + l].copy() for _, l, _, o in heads[c]], "sent": sent[c], "status": hst[stat_at[c][sent[c] != 0]]}
        got.update(ic.state_of(q, chans[c]))
        out.append(got)
    return out, len(calls), shared


def fftext_run_plan(fx, ctx, steps, chans, scripts, spec, resident=False, rng=None, row_stride=fc.W + 64, fill=0xAA):
    """the same for kg_fftext: the object's sample rate is set to the round's ahead of a call that needs another.  resident: the
    spectra of all calls are uploaded once into one NaN-filled device buffer.  Rows go to one buffer, read behind the last call;
    every byte of it outside the rows keeps `fill`.  -> (per script the keys of fftext_common.run_script_dev, calls, shared calls)"""
    n = len(scripts)
    nb = [fc.nblocks(s) for s in scripts]
    sent, bins, row_at = [np.zeros(b, np.int32) for b in nb], [[] for _ in range(n)], [[] for _ in range(n)]
    calls = [s for s in steps if s[0] == "call"]
    nblocks = max(sum(len(e[2]) for s in calls for e in s[2]), 1)
    hrows = np.full((nblocks, row_stride), fill, np.uint8)
    d_rows, d_spec = ctx.alloc(hrows.nbytes), None
    at = shared = k = 0
    now = None
    try:
        ctx.upload(d_rows, hrows)
        if resident:
            where, total = _layout(steps, lambda s: fc.W, rng)
            host = np.full(total, np.nan + 1j * np.nan, np.complex64)
            for (base, stride), s in zip(where, calls):
                for i, e in enumerate(s[2]):
                    for j, b in enumerate(e[2]):
                        host[base + i * stride + j * fc.W:][:fc.W] = spec[b[2]]
            d_spec = ctx.alloc(host.nbytes)
            ctx.upload(d_spec, host)
        for s in steps:
            if s[0] == "cmd":
                ch, l = chans[s[1]], s[2]
                if l[0] == "S":
                    run, sam, mode = (int(v) for v in l[2:].split())
                    fx.set_run(ch, run, sam != 0, mode == fc.QAM)
                elif l[0] == "I":
                    fx.set_itime(ch, float(l[2:]))
                elif l[0] == "C":
                    fx.clear(ch)
                continue                                                   # `R`: with the call
            _, rate, ents = s
            if rate != now:
                fx.set_rate(rate)
                now = rate
            nblk = [len(e[2]) for e in ents]
            if resident:
                base, stride = where[k]
                d_in = d_spec + 8 * base
            else:
                stride = fc.W * max(nblk)
                host = np.zeros((len(ents), stride), np.complex64)
                for i, e in enumerate(ents):
                    for j, b in enumerate(e[2]):
                        host[i, j * fc.W:(j + 1) * fc.W] = spec[b[2]]
                d_in = ctx.alloc(host.nbytes)
                ctx.upload(d_in, host)
            try:
                m = fx.process_dev([chans[e[0]] for e in ents], nblk, [e[1] for e in ents], d_in, stride, d_rows + at * row_stride, row_stride, sum(nblk))
            finally:
                if not resident:
                    ctx.sync()
                    ctx.free(d_in)
            for i, (ch, ent, blk, b) in enumerate(m.tolist()):
                c, e = chans.index(ch), ents[ent]
                assert e[0] == c
                sent[c][e[2][blk][3]] = 1
                bins[c].append(b)
                row_at[c].append(at + i)
            at += m.shape[0]
            shared += len({e[0] for e in ents if e[2]}) > 1
            k += 1
        ctx.sync()
        ctx.download(d_rows, hrows)
    finally:
        for p in (d_rows, d_spec):
            if p:
                ctx.free(p)
    assert (hrows[:at, fc.W:] == fill).all() and (hrows[at:] == fill).all(), "bytes outside the rows were written"
    out = []
    for c in range(n):
        info, ncma, pwr = fx.state(chans[c], sums=True)
        out.append({"sent": sent[c], "bins": np.array(bins[c], np.int32), "rows": hrows[row_at[c], :fc.W].reshape(-1, fc.W).copy(), "run": int(info["run"]),
                    "instance": int(info["instance"]), "nbins": int(info["bins"]), "reset": int(info["reset"]), "fft_scale": np.float32(info["fft_scale"]),
                    "spectrum_scale": np.float32(info["spectrum_scale"]), "fi": float(info["fi"]), "fft_sec": float(info["fft_sec"]),
                    "time": float(info["time"]), "ncma": ncma, "pwr": pwr})
    return out, len(calls), shared


_ORDER = [(7 * i + 5) % NSEED for i in range(NSEED + 2)]                 # 7 and 40 have no common factor: every seed once, then two again
TRIPLES = [_ORDER[i:i + 3] for i in range(0, NSEED, 3)]


def triples():
    """the 40 seeds three at a time, out of order; every seed is in one at least"""
    assert sorted({s for t in TRIPLES for s in t}) == list(range(NSEED)) and all(len(set(t)) == 3 for t in TRIPLES)
    return TRIPLES


def plan_rng(mod, group, resident=False):
    return np.random.default_rng(BASE[mod] + PARTITION + 1000 * (1 + resident) + group)


def planned(mod, group, resident=False):
    """-> (the seeds of the group, their scripts, the steps, the generator behind them)"""
    seeds = triples()[group]
    scripts = [SCRIPT[mod](s) for s in seeds]
    rng = plan_rng(mod, group, resident)
    return seeds, scripts, plan_side_by_side(mod, scripts, rng), rng


def calls_of(steps):
    """-> (calls, calls that carry more than one script, blocks)"""
    calls = [s for s in steps if s[0] == "call"]
    return len(calls), sum(len({e[0] for e in s[2] if e[2]}) > 1 for s in calls), sum(len(e[2]) for s in calls for e in s[2])


def pushes(mod, lines, cuts):
    """fax, cw: the blocks of every push of run_script_dev(.., cuts=cuts), decided ahead of the run"""
    return [len(st[1]) for st in COMMON[mod].script_steps(lines, cuts) if st[0] == "push"]


def planned_pushes(mod):
    """fax, cw: the blocks of every push of test_random_scripts_under_a_random_partition and test_shape_scripts"""
    out = []
    for seed in range(NSEED):
        lines = SCRIPT[mod](seed)
        out += pushes(mod, lines, partition(mod, seed, COMMON[mod].nblocks(lines))) + pushes(mod, lines, lambda: 1)
    for lines in SHAPES[mod]().values():
        out += pushes(mod, lines, lambda: 256) + pushes(mod, lines, lambda: 1)
    return out


def side_by_side(mod, q, pool, group):
    """fax, cw: the group's three seeds on connections 0 .. 2 of q in lock step (q None: the schedule alone)
    -> (the seeds, per seed the device's result, pushes, pushes that carried more than one connection)"""
    seeds = triples()[group]
    return (seeds,) + COMMON[mod].run_side_by_side(q, [SCRIPT[mod](s) for s in seeds], pool, plan_rng(mod, group))


def shared_in_all(mod, resident=False):
    """over all the groups: (calls, calls that carry more than one script)"""
    if mod in ("fax", "cw"):
        n = [side_by_side(mod, None, None, g)[2:] for g in range(len(TRIPLES))]
        return sum(v[0] for v in n), sum(v[1] for v in n)
    n = [calls_of(planned(mod, g, resident)[2]) for g in range(len(TRIPLES))]
    return sum(v[0] for v in n), sum(v[1] for v in n)
