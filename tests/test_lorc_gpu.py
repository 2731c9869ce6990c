"""kg_lorc on the device against tests/golden/lorc_ref.npz (the reference's own statements, tools/make_ref_lorc_golden.py): every row --
bytes, command, length, channel, block, sample, order -- and the end state bit for bit.  Three connections with different parameters
run their scripts side by side in one object, several blocks and connections a call; 48 blocks in one call equal 48 calls of one
block; a refused call leaves the state and a canary-filled rows array as they were.  Every comparison is an equality."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, lorc

from . import lorc_common as lc

pytestmark = pytest.mark.gpu

NAMES = sorted(lc.scripts())
TRIPLES = [[NAMES[(3 * g + k) % len(NAMES)] for k in range(3)] for g in range((len(NAMES) + 2) // 3)]


@pytest.fixture(scope="module")
def golden():
    return lc.load()


@pytest.fixture(scope="module")
def pool():
    return lc.pool()


def _items(lines):
    """a script as commands and blocks: ("cmd", line) / ("blk", ns, pool offset, block number)"""
    out, seen = [], 0
    for l in lines:
        if l[0] == "B":
            ns, off = (int(v) for v in l.split()[1:])
            out.append(("blk", ns, off, seen))
            seen += 1
        else:
            out.append(("cmd", l))
    return out


def run_side_by_side(q, scripts, samples, most=8, rng=None):
    """scripts[c] on connection c of q, in lockstep: every round each connection takes its commands up to its next block, then ONE call
    feeds every connection whose next blocks have the round's ns -- up to `most` consecutive blocks each, so the entries differ in
    length.  With rng (a numpy Generator) the round's ns is the one most connections wait with, each takes a random number of blocks up
    to `most`, and a connection alone in its call all its consecutive blocks (256 at most): the calls are spent where they are shared.
    -> per connection the keys of lorc_common.parse(), the number of calls with more than one connection, and with rng the calls"""
    items = [_items(s) for s in scripts]
    at = [0] * len(items)
    rec = [lc.Recorder(lc.nblocks(s)) for s in scripts]
    shared = calls = 0
    while any(a < len(it) for a, it in zip(at, items)):
        for c, it in enumerate(items):
            while at[c] < len(it) and it[at[c]][0] == "cmd":
                lc.apply_command(q, c, it[at[c]][1])
                at[c] += 1
        ready = [c for c, it in enumerate(items) if at[c] < len(it)]
        if not ready:
            break
        waits = [items[c][at[c]][1] for c in ready]
        ns = waits[0] if rng is None else max(sorted(set(waits)), key=waits.count)
        take = {}
        for c in ready:
            it, k = items[c], at[c]
            if it[k][1] != ns:
                continue
            n, lim = 1, most if rng is None else int(rng.integers(1, most + 1)) if waits.count(ns) > 1 else 256
            while n < lim and k + n < len(it) and it[k + n][0] == "blk" and it[k + n][1] == ns and it[k + n][2] == it[k + n - 1][2] + ns:
                n += 1
            take[c] = it[k:k + n]
        conns = sorted(take, key=lambda c: -c)                            # not in connection order: the list's order is the caller's
        nb = max(len(v) for v in take.values())
        x = np.zeros((len(conns), nb, ns), np.complex64)
        for i, c in enumerate(conns):
            x[i, :len(take[c])] = samples[take[c][0][2]:take[c][0][2] + ns * len(take[c])].reshape(-1, ns)
        rows, m = q.process(conns, x, nblk=[len(take[c]) for c in conns])
        assert np.array_equal(m["conn"], np.array(sorted(m["conn"], key=conns.index), np.int32)), "rows go connection by connection, in list order"
        assert (m["off"] % 16 == 0).all() and (np.diff(m["off"]) >= m["len"][:-1]).all()
        for c in conns:
            rec[c].add([b[3] for b in take[c]], m[m["conn"] == c], rows)
            at[c] += len(take[c])
        shared += len(conns) > 1
        calls += 1
    got = [r.result(lc.state_of(q, c)) for c, r in enumerate(rec)]
    return (got, shared) if rng is None else (got, shared, calls)


@pytest.mark.parametrize("group", range(len(TRIPLES)))
def test_three_connections_side_by_side_equal_the_golden(gpu_ctx, golden, pool, group):
    names = TRIPLES[group]
    sc = lc.scripts()
    q = lorc.LoranC(gpu_ctx, nconn=3)
    try:
        got, shared = run_side_by_side(q, [sc[n] for n in names], pool)
        assert shared >= 2              # a call takes 8 blocks of a script at most, and two scripts of every group have 16 or more
        for n, g in zip(names, got):
            lc.check_against_golden(golden, n, g)
    finally:
        q.close()


@pytest.mark.parametrize("name", ["noise_cma_long", "iir_auto", "same_sample", "nbucket_1_2"])
def test_many_blocks_in_one_call_equal_a_call_a_block(gpu_ctx, golden, pool, name):
    """48 blocks in one call (24 and 4 for the shorter scripts) against as many calls of one block: rows and state, byte for byte, and
    both equal to the reference"""
    lines = lc.scripts()[name]
    q = lorc.LoranC(gpu_ctx, nconn=2)
    try:
        one = lc.run_script_dev(q, lines, pool, conn=0, max_blocks=48)
        each = lc.run_script_dev(q, lines, pool, conn=1, max_blocks=1)
        assert one["calls"] == 1 and each["calls"] == lc.nblocks(lines) and (name != "noise_cma_long" or each["calls"] == 48)
        for k in ("nrows", "samp", "ch", "cmd", "len"):
            assert np.array_equal(one[k], each[k]), k
        assert lc.all_bytes(one).tobytes() == lc.all_bytes(each).tobytes()
        assert one["scalars"].tobytes() == each["scalars"].tobytes() and one["avg"].tobytes() == each["avg"].tobytes()
        lc.check_against_golden(golden, name, one)
    finally:
        q.close()


def test_a_refused_call_or_command_changes_nothing(gpu_ctx, golden, pool):
    """refused commands and refused calls strewn through a script: the state read back is the one ahead of them, a rows array full of
    0xA5 stays full of it, and the script still ends where the reference ends"""
    name = "same_sample"
    lines = lc.scripts()[name]
    q = lorc.LoranC(gpu_ctx, nconn=2)
    canary = np.full(8192, 0xA5, np.uint8)

    def snapshot():
        s = lc.state_of(q, 0)
        return s["scalars"].tobytes() + s["avg"].tobytes()

    def refused(fn):
        before = snapshot()
        with pytest.raises(KiwiGpuError):
            fn()
        assert snapshot() == before and (canary == 0xA5).all()

    try:
        with pytest.raises(KiwiGpuError):
            q.set_gri(0, 0, 7980)                                          # ahead of kg_lorc_init
        rec, pushes = lc.Recorder(lc.nblocks(lines)), 0
        for st in lc.script_calls(lines, 4):
            if st[0] == "cmd":
                lc.apply_command(q, 0, st[1])
                if st[1][0] == "N":
                    refused(lambda: q.set_offset(0, 0, 5))                   # ahead of a GRI
                continue
            _, ns, offs, blocks = st
            x = pool[offs[0]:offs[0] + ns * len(offs)].reshape(1, len(offs), ns)
            for bad in (lambda: q.set_gri(0, 0, 9990), lambda: q.set_gri(0, 1, 0), lambda: q.set_gri(0, 2, 7980), lambda: q.set_avg_algo(0, 0, 3),
                        lambda: q.set_gain(0, -1, 3), lambda: q.set_avg_param(0, 2, 1.0), lambda: q.init(0, 0.0, 600)):
                refused(bad)
            refused(lambda: q.process([0], x, rows=canary, max_rows=0) if pushes % 3 == 1 else q.process([0], x, rows=canary[:1], max_rows=64))
            refused(lambda: q.process([0, 0], np.concatenate([x, x]), rows=canary))                      # listed twice
            refused(lambda: q.process([2], x, rows=canary))                                              # no such connection
            refused(lambda: q.process([0], np.zeros((1, 1, 513), np.complex64), rows=canary))            # ns
            refused(lambda: q.process([0, 1], np.concatenate([x, x]), rows=canary))                      # connection 1 was never initialised
            before = snapshot()
            runs, nrows, nbytes = q.plan([0], [len(offs)], ns)                # the schedule alone, on copies
            assert snapshot() == before
            rows, m = q.process([0], x)
            assert nrows == m.size and nbytes == int(m["off"][-1] + m["len"][-1]) and runs >= 2 * (ns * len(offs) // 958)
            rec.add(blocks, m, rows)
            pushes += 1
        got = rec.result(lc.state_of(q, 0))
        assert got["nrows"].sum() >= 20 and pushes >= 6          # the rows_cap and max_rows refusals met calls that had rows to send
        lc.check_against_golden(golden, name, got)
        # the pushes kg_lorc.h refuses, on a started connection: EMA below 1, IIR negative, a channel without a GRI
        x = pool[:512].reshape(1, 1, 512)
        q.set_avg_algo(0, 1, lorc.EMA); q.set_avg_param(0, 1, 0.3)
        refused(lambda: q.process([0], x, rows=canary))
        q.set_avg_algo(0, 1, lorc.IIR); q.set_avg_param(0, 1, -1e-9)
        refused(lambda: q.process([0], x, rows=canary))
        q.set_avg_param(0, 1, float("inf"))
        refused(lambda: q.process([0], x, rows=canary))
        q.init(0, 12000.0, 600)                                  # still started: the registration outlives the memset
        q.set_gri(0, 0, 7980)
        refused(lambda: q.process([0], x, rows=canary))
        q.set_gri(0, 1, 7980)
        q.set_avg_param(0, 0, 1); q.set_avg_param(0, 1, 1)
        rows, m = q.process([0], x, rows=canary)
        info, avg = q.state(0)
        assert m.size == 0 and int(info["ch"][0]["samp"]) == 512 and (avg[0][:511] != 0).all() and (canary == 0xA5).all()
    finally:
        q.close()


def test_a_stopped_connection_takes_nothing(gpu_ctx, pool):
    q = lorc.LoranC(gpu_ctx, nconn=1)
    try:
        q.init(0, 12000.0, 600)
        rows, m = q.process([0], pool[:1024].reshape(1, 2, 512))           # not started, no GRI: the callback is not registered
        info, avg = q.state(0)
        assert m.size == 0 and int(info["ch"][0]["samp"]) == 0 and not avg.any() and not rows.any()
    finally:
        q.close()


# ---- seeded random scripts (tests/ext_random.py) under random call partitions: the device against the host model, in full
PARTS = 4                                                                  # the 40 seeds, ten a test


@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er, ext_random_dev as ed
    return er.load("lorc")


@pytest.fixture(scope="module")
def random_host(pool, tmp_path_factory):
    """the host driver's result of every seed, sample by sample: made once, shared, left unchanged"""
    from . import ext_random as er, ext_random_dev as ed
    tmp = tmp_path_factory.mktemp("lorc_random")
    driver = lc.build_driver(tmp)
    return [lc.run_script_exe(driver, er.lorc_script(seed), pool, tmp) for seed in range(er.NSEED)]


@pytest.mark.parametrize("part", range(PARTS))
def test_random_scripts_under_a_random_partition(gpu_ctx, random_ref, random_host, pool, part):
    """every seed's script with at most max_blocks (drawn from 1, 2, 5, 48 by a generator of its own) blocks a call, and again a call a
    block: both equal the host model in every row byte and map field and the whole end state with avg[2][1199], hence each other, and
    the fixture's digests"""
    from . import ext_random as er, ext_random_dev as ed
    q = lorc.LoranC(gpu_ctx, nconn=2)
    try:
        for seed in range(part * er.NSEED // PARTS, (part + 1) * er.NSEED // PARTS):
            lines = er.lorc_script(seed)
            most = ed.partition("lorc", seed, lc.nblocks(lines))
            got = lc.run_script_dev(q, lines, pool, conn=0, max_blocks=most)
            each = lc.run_script_dev(q, lines, pool, conn=1, max_blocks=1)
            ed.lorc_same(got, random_host[seed], "seed %d" % seed, "max_blocks %d" % most)
            ed.lorc_same(each, random_host[seed], "seed %d" % seed, "a call a block")
            assert lc.all_bytes(got).tobytes() == lc.all_bytes(each).tobytes() and each["calls"] >= got["calls"]
            er.check_record("lorc", seed, lines, got, er.unpack(random_ref, seed))
    finally:
        q.close()


class _Planned:
    """stands in for a LoranC where only the schedule of run_side_by_side is wanted: takes every command and call, answers no row"""

    def __getattr__(self, name):
        return lambda *a, **k: None

    def process(self, conns, x, nblk=None):
        return np.zeros(0, np.uint8), np.zeros(0, lorc.row_dtype)

    def state(self, conn):
        return np.zeros(1, lorc.info_dtype)[0], np.zeros((2, lc.MAX_BUCKET), np.float32)


def _random_group(q, pool, group):
    from . import ext_random as er, ext_random_dev as ed
    seeds = ed.triples()[group]
    return seeds, run_side_by_side(q, [er.lorc_script(s) for s in seeds], pool, most=4, rng=ed.plan_rng("lorc", group))


@pytest.mark.parametrize("group", range(14))
def test_random_scripts_side_by_side(gpu_ctx, random_ref, random_host, pool, group):
    """the seeds three at a time on three connections of one object, listed out of order: every call carries every connection whose next
    blocks share the round's ns, a random number of blocks each; the commands go between the calls.  Each connection equals the host
    model of its own script in full, and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    q = lorc.LoranC(gpu_ctx, nconn=3)
    try:
        seeds, (got, shared, calls) = _random_group(q, pool, group)
    finally:
        q.close()
    for seed, g in zip(seeds, got):
        ed.lorc_same(g, random_host[seed], "seed %d of %s" % (seed, seeds))
        er.check_record("lorc", seed, er.lorc_script(seed), g, er.unpack(random_ref, seed))
    assert shared >= 1 and calls >= shared


def test_random_side_by_side_calls_are_shared(pool):
    """at least half of the calls of all the groups carry more than one connection: the schedule alone, which no row decides"""
    every = [_random_group(_Planned(), pool, k)[1][1:] for k in range(14)]
    assert 2 * sum(s for s, _ in every) >= sum(c for _, c in every), every
