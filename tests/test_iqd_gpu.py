"""The IQ display extension on the device (extensions/IQ_display/iq_display.cpp with rx/kiwi/pll.h; kg_iqd): kg_iqd_process_dev against
every row byte, row map entry, status record, status map entry and end state of the reference's scripts (tests/golden/iqd_ref.npz),
the same bytes whatever the split of a script into calls, two channels in one call, refusals that change nothing, the host-array
twin, rows behind a real kg_fir_process_dev against the host model (csrc/kg_iqd.h through tools/iqd_host_driver.cpp) of the samples
that call stored, and the device's hypotf / fmodf against the host's.  Every comparison is an equality."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, iqd, snd

from . import iqd_common as ic

pytestmark = pytest.mark.gpu
KG_ERR_INVALID, KG_ERR_STATE = -2, -5


@pytest.fixture(scope="module")
def golden():
    return ic.load()


@pytest.fixture(scope="module")
def pool():
    return ic.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return ic.build_driver(tmp_path_factory.mktemp("iqd"))


def samp_of_rows(lines):
    """the sample behind which every row goes out, walked as display_data walks (:74-96)"""
    points, draw, ring, on, out = 1024, 0, [0, 0], False, []
    for l in lines:
        a = l.split()
        if a[0] == "N":
            points, draw, ring, on = 1024, 0, [0, 0], False
        elif a[0] == "R":
            on = int(a[1]) != 0
        elif a[0] == "P":
            points = int(a[1])
        elif a[0] == "D":
            draw = int(a[1])
        elif a[0] == "B" and on and draw in (0, 1):
            ch = int(a[1])
            for i in range(int(a[2])):
                ring[ch] += 1
                if ring[ch] >= points:
                    out.append(i)
                    ring[ch] = 0
    return np.array(out, np.int32)


@pytest.mark.parametrize("name", sorted(ic.scripts()))
def test_scripts_equal_the_reference(gpu_ctx, golden, pool, name):
    """rows, cmd, length, the block and the sample a row went out behind, the sent status records and which blocks sent one, and the
    end state -- every scalar, _iq, _plot and _map --, with the blocks between two commands in ONE call"""
    lines = ic.scripts()[name]
    q = iqd.IqDisplay(gpu_ctx, nchan=1)
    try:
        got = ic.run_script_dev(q, gpu_ctx, lines, pool)
    finally:
        q.close()
    ic.check_against_golden(golden, name, got)
    assert np.array_equal(got["samp"], samp_of_rows(lines)), "the row map's sample index"
    assert got["calls"] <= sum(1 for l in lines if l[0] != "B") + 3          # + a change of ns


@pytest.mark.parametrize("name", ["exp2_bpsk_density", "points_change", "both_instances", "msk", "silence_auto"])
def test_any_split_into_calls_gives_the_same_bytes(gpu_ctx, golden, pool, name):
    """cut at a few places, one block a call, and several blocks an entry: LDS or memory, the state is the same"""
    lines = ic.scripts()[name]
    nb = ic.nblocks(lines)
    q = iqd.IqDisplay(gpu_ctx, nchan=1)
    try:
        for cuts, merge in (({1}, False), ({nb // 2, nb // 2 + 1}, True), (set(range(1, nb, 3)), True), (set(range(1, nb)), False), (set(), True)):
            got = ic.run_script_dev(q, gpu_ctx, lines, pool, cuts=cuts, merge=merge)
            ic.check_against_golden(golden, name, got)
    finally:
        q.close()


def test_two_channels_in_one_call_do_not_mix(gpu_ctx, golden, pool):
    """three scripts whose commands all stand ahead of their blocks, on three channels of one object (listed out of order), their
    blocks interleaved entry by entry in ONE call"""
    ctx = gpu_ctx
    names, chan = ("exp1_cw", "exp2_bpsk_density", "pll_off"), (2, 0, 1)
    q = iqd.IqDisplay(ctx, nchan=3)
    blocks = []
    for name, ch in zip(names, chan):
        lines = ic.scripts()[name]
        assert all(l[0] != "B" for l in lines[:lines.index(next(l for l in lines if l[0] == "B"))]) and lines[-1][0] == "B"
        for l in lines:
            if l[0] != "B":
                ic.apply_command(q, ch, l)
        blocks.append([int(l.split()[3]) for l in lines if l[0] == "B"])
    ents = [(k, b) for b in range(max(len(x) for x in blocks)) for k in range(3) if b < len(blocks[k])]
    host = np.stack([pool[blocks[k][b]:blocks[k][b] + 512] for k, b in ents])
    cap = (512 * len(ents) + 3 * ic.RING) * 4
    d_iq, d_rows, d_st = ctx.alloc(host.nbytes), ctx.alloc(cap), ctx.alloc(24 * len(ents))
    try:
        ctx.upload(d_iq, host)
        m, sent = q.process_dev([chan[k] for k, _ in ents], [1] * len(ents), [0] * len(ents), 512, d_iq, 512, d_rows, cap, d_st, len(ents), len(ents) * 512)
        ctx.sync()
        hrows, hst = np.zeros(cap, np.uint8), np.zeros(len(ents), iqd.status_dtype)
        ctx.download(d_rows, hrows)
        ctx.download(d_st, hst)
        for k, (name, ch) in enumerate(zip(names, chan)):
            mine = m[m["ch"] == ch]
            idx = [i for i, e in enumerate(ents) if e[0] == k]
            got = {"nrows": np.array([int((mine["ent"] == i).sum()) for i in idx], np.int32), "cmd": mine["cmd"].copy(), "len": mine["len"].copy(),
                   "rows": [hrows[r["off"]:r["off"] + r["len"]] for r in mine], "sent": sent[idx]}
            got["status"] = hst[idx][got["sent"] != 0]
            got.update(ic.state_of(q, ch))
            ic.check_against_golden(golden, name, got)
    finally:
        for p in (d_iq, d_rows, d_st):
            ctx.free(p)
        q.close()


def test_a_refused_call_changes_nothing(gpu_ctx, pool):
    ctx = gpu_ctx
    q = iqd.IqDisplay(ctx, nchan=3)
    for l in ic.HEAD + ["M 1 2", "P 300"]:
        ic.apply_command(q, 0, l)
    ic.apply_command(q, 1, "N")                                            # channel 1: no rate; channel 2: no init
    host = np.ascontiguousarray(pool[ic.AT["bpsk"]:ic.AT["bpsk"] + 4 * 512]).reshape(4, 512)
    cap = 4 * 512 * 4
    d_iq, d_rows, d_st = ctx.alloc(host.nbytes), ctx.alloc(cap), ctx.alloc(24 * 4)
    fill_r, fill_s = np.full(cap, 0x5A, np.uint8), np.full(24 * 4, 0xA5, np.uint8)
    try:
        ctx.upload(d_iq, host)
        q.process_dev([0], [2], [0], 512, d_iq, 1024, d_rows, cap, d_st, 4, 64)          # two blocks taken: ring 124, three rows
        ctx.sync()
        before = ic.state_of(q, 0)
        assert before["ints"][9] == 1024 % 300
        ctx.upload(d_rows, fill_r)
        ctx.upload(d_st, fill_s)
        call = lambda **kw: q.process_dev(kw.get("chans", [0]), kw.get("nblk", [2]), kw.get("inst", [0]), kw.get("ns", 512), d_iq, 1024, d_rows,
                                          kw.get("cap", cap), d_st, kw.get("scap", 4), kw.get("max_rows", 64))
        refused = [({"cap": 3 * 1200 - 1}, KG_ERR_INVALID),                  # ring 124: rows behind samples 175, 475 and 263 of the next blocks
                   ({"ns": 0}, KG_ERR_INVALID), ({"ns": 513}, KG_ERR_INVALID), ({"inst": [2]}, KG_ERR_INVALID), ({"inst": [-1]}, KG_ERR_INVALID),
                   ({"scap": 1}, KG_ERR_INVALID), ({"max_rows": 2}, KG_ERR_INVALID), ({"chans": [3]}, KG_ERR_INVALID),
                   ({"chans": [0, 1], "nblk": [1, 1], "inst": [0, 0]}, KG_ERR_STATE), ({"chans": [0, 2], "nblk": [1, 1], "inst": [0, 0]}, KG_ERR_STATE)]
        for kw, status in refused:
            with pytest.raises(KiwiGpuError) as e:
                call(**kw)
            assert e.value.status == status, (kw, e.value.status)
        for bad in (lambda: q.set_points(0, 0), lambda: q.set_points(0, 16385), lambda: q.set_pll_mode(0, 1, -1), lambda: q.set_pll_mode(0, 0, -2),
                    lambda: q.set_run(0, 1, 0.0), lambda: q.set_gain(2, 10)):
            with pytest.raises(KiwiGpuError):
                bad()
        ctx.sync()
        after = ic.state_of(q, 0)
        for k in before:
            assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
        got_r, got_s = np.zeros(cap, np.uint8), np.zeros(24 * 4, np.uint8)
        ctx.download(d_rows, got_r)
        ctx.download(d_st, got_s)
        assert np.array_equal(got_r, fill_r) and np.array_equal(got_s, fill_s)
        # the neighbours are taken: exactly the capacity, points at both ends, exponent 0, pll_mode 2 with a negative baud
        m, _ = call(cap=3 * 1200)
        assert m["len"].tolist() == [1200] * 3 and m["samp"].tolist() == [175, 475, 263] and m["blk"].tolist() == [0, 0, 1]
        q.set_points(0, 1); q.set_points(0, 16384); q.set_pll_mode(0, 1, 0); q.set_pll_mode(0, 2, -5); q.set_pll_mode(0, 7, -5)
    finally:
        for p in (d_iq, d_rows, d_st):
            ctx.free(p)
        q.close()


def test_host_array_twin_equals_the_device_path(gpu_ctx, golden, pool):
    lines = ic.scripts()["exp1_cw"]
    q = iqd.IqDisplay(gpu_ctx, nchan=2)
    try:
        for l in lines:
            if l[0] != "B":
                ic.apply_command(q, 1, l)
        offs = [int(l.split()[3]) for l in lines if l[0] == "B"]
        x = np.stack([pool[o:o + 512] for o in offs])[None]              # one entry, all the blocks
        rows, m, status, sent = q.process([1], x, [0])
        got = {"nrows": np.array([int((m["blk"] == b).sum()) for b in range(len(offs))], np.int32), "cmd": m["cmd"].copy(), "len": m["len"].copy(),
               "rows": [rows[r["off"]:r["off"] + r["len"]] for r in m], "sent": sent, "status": status[sent != 0]}
        got.update(ic.state_of(q, 1))
        ic.check_against_golden(golden, "exp1_cw", got)
    finally:
        q.close()


def test_behind_the_fir_the_tap_is_its_output(gpu_ctx, driver, tmp_path):
    """three channels through kg_fir_process_dev, two calls; kg_iqd reads the filter's d_out in place: each channel's rows, status and
    end state equal the host model of the samples the filter stored"""
    ctx = gpu_ctx
    NCH, N = 3, 1536
    setup = [["M 1 1", "P 300", "G 60"], ["M 2 200", "D 1", "P 700"], ["M 0 0", "P 100"]]
    rng = np.random.default_rng(77)
    F = snd.FastFir(ctx, nchan=NCH, max_in=2048)
    q = iqd.IqDisplay(ctx, nchan=NCH)
    out_stride = 2048
    cap = (out_stride * NCH + NCH * ic.RING) * 4
    d_in, d_out, d_rows, d_st = ctx.alloc(NCH * N * 8), ctx.alloc(NCH * out_stride * 8), ctx.alloc(cap), ctx.alloc(24 * 4 * NCH)
    try:
        for ch in range(NCH):
            F.setup(ch, -2500.0 + 300 * ch, 2500.0, 0.0, 12000.0)
            for l in ic.HEAD + setup[ch]:
                ic.apply_command(q, ch, l)
        scripts = [ic.HEAD + setup[ch] for ch in range(NCH)]
        taps, got = [np.zeros(0, np.complex64) for _ in range(NCH)], [dict(rows=[], sent=[], status=[]) for _ in range(NCH)]
        t = np.arange(N) / 12000.0
        for call in range(2):
            x = np.stack([(3000.0 * np.exp(2j * np.pi * (200.0 + 40 * ch) * (t + call * N / 12000.0)) + 300.0 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)))
                          for ch in range(NCH)]).astype(np.complex64)
            ctx.upload(d_in, x)
            nout = F.process_dev(np.arange(NCH), d_in, N, N, d_out, out_stride)
            assert (nout % 512 == 0).all() and nout.sum() > 0
            nblk = (nout // 512).astype(np.int32)
            m, sent = q.process_dev(np.arange(NCH), nblk, [0] * NCH, 512, d_out, out_stride, d_rows, cap, d_st, 4 * NCH, 4096)
            ctx.sync()
            hout, hrows, hst = np.zeros((NCH, out_stride), np.complex64), np.zeros(cap, np.uint8), np.zeros(4 * NCH, iqd.status_dtype)
            ctx.download(d_out, hout)
            ctx.download(d_rows, hrows)
            ctx.download(d_st, hst)
            k = 0
            for ch in range(NCH):
                scripts[ch] += ["B 0 512 %d" % (taps[ch].size + 512 * b) for b in range(nblk[ch])]
                taps[ch] = np.concatenate([taps[ch], hout[ch, :nout[ch]]])
                got[ch]["rows"] += [hrows[r["off"]:r["off"] + r["len"]].copy() for r in m[m["ch"] == ch]]
                got[ch]["sent"] += sent[k:k + nblk[ch]].tolist()
                got[ch]["status"] += [hst[k + b] for b in range(nblk[ch]) if sent[k + b]]
                k += nblk[ch]
        assert sum(len(g["rows"]) for g in got) > 6 and sum(sum(g["sent"]) for g in got) >= 1
        for ch in range(NCH):
            d = tmp_path / ("ch%d" % ch)
            d.mkdir()
            want = ic.run_script_exe(driver, scripts[ch], taps[ch], d)
            assert len(want["rows"]) == len(got[ch]["rows"]) and want["sent"].tolist() == got[ch]["sent"], ch
            for a, b in zip(want["rows"], got[ch]["rows"]):
                assert np.array_equal(a, b), ch
            assert want["status"].tobytes() == np.array(got[ch]["status"], iqd.status_dtype).tobytes(), ch
            st = ic.state_of(q, ch)
            for key in ("ints", "floats", "pll", "iq", "plot", "map"):
                assert np.asarray(st[key]).tobytes() == np.asarray(want[key]).tobytes(), (ch, key)
    finally:
        for p in (d_in, d_out, d_rows, d_st):
            ctx.free(p)
        q.close()
        F.close()


def math_arguments(fn):
    """2^20 pairs: random bit patterns, subnormals, zeros, equal operands, what the PLL and the means feed in"""
    rng = np.random.default_rng(0x4D415448 + fn)
    n = 1 << 20
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    q = n // 8
    a[q:2 * q] = (rng.uniform(-60, 60, q)).astype(np.float32)                          # the phase ahead of its wrap
    b[q:2 * q] = np.float32(16 * np.pi) if fn == iqd.FMODF else rng.uniform(-3e4, 3e4, q).astype(np.float32)
    b[q:q + q // 2] = np.float32(2 * np.pi) if fn == iqd.FMODF else b[q:q + q // 2]
    a[2 * q:3 * q] = rng.integers(0, 1 << 23, q).astype(np.uint32).view(np.float32)     # subnormals (and +0)
    b[2 * q:2 * q + q // 2] = rng.integers(1, 1 << 23, q // 2).astype(np.uint32).view(np.float32)
    a[3 * q:4 * q] = b[3 * q:4 * q]                                                   # equal operands
    a[4 * q:4 * q + 1024] = np.array([0.0, -0.0, np.inf, -np.inf], np.float32).repeat(256)
    b[4 * q + 1024:4 * q + 2048] = np.array([0.0, -0.0, np.inf, -np.inf], np.float32).repeat(256)
    with np.errstate(all="ignore"):
        a[4 * q + 2048:5 * q] = (b[4 * q + 2048:5 * q].astype(np.float64) * rng.integers(1, 40, q - 2048)).astype(np.float32)      # near multiples
    lo = rng.integers(0, 1 << 32, q, dtype=np.uint64).astype(np.uint32)
    a[5 * q:6 * q] = ((lo & np.uint32(0x807FFFFF)) | (rng.integers(100, 160, q).astype(np.uint32) << 23)).view(np.float32)   # exponents close together
    b[5 * q:6 * q] = ((lo[::-1] & np.uint32(0x807FFFFF)) | (rng.integers(100, 160, q).astype(np.uint32) << 23)).view(np.float32)
    return a, b


@pytest.mark.parametrize("fn", [iqd.HYPOTF, iqd.FMODF])
def test_device_hypotf_and_fmodf_equal_the_hosts(gpu_ctx, fn):
    ctx = gpu_ctx
    a, b = math_arguments(fn)
    with np.errstate(all="ignore"):
        want = (np.hypot(a, b) if fn == iqd.HYPOTF else np.fmod(a, b)).astype(np.float32)
    assert want.dtype == np.float32
    d_a, d_b, d_o = ctx.alloc(a.nbytes), ctx.alloc(b.nbytes), ctx.alloc(a.nbytes)
    try:
        ctx.upload(d_a, a)
        ctx.upload(d_b, b)
        iqd.math_dev(ctx, fn, d_a, d_b, a.size, d_o)
        ctx.sync()
        got = np.zeros_like(a)
        ctx.download(d_o, got)
    finally:
        for p in (d_a, d_b, d_o):
            ctx.free(p)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)                              # a NaN compares as a NaN: its sign and payload are the unit's
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, (bad.size, a[bad[:4]], b[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert nan.sum() > 1000 and (np.abs(want[~nan]) < 1.2e-38).sum() > 1000                  # NaN results and subnormal ones were reached
    assert fn == iqd.HYPOTF or (want[~nan] == 0).sum() > 100000                                 # equal operands: a signed zero


# ---- seeded random scripts (tests/ext_random.py) under random call partitions: the device against the host model, in full
PARTS = 4                                                                  # the 40 seeds, ten a test


@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er, ext_random_dev as ed
    return er.load("iqd")


@pytest.fixture(scope="module")
def random_host(driver, pool, tmp_path_factory):
    """the host driver's result of every seed: made once, shared, left unchanged"""
    from . import ext_random as er, ext_random_dev as ed
    tmp = tmp_path_factory.mktemp("iqd_random")
    return [ic.run_script_exe(driver, er.iqd_script(seed), pool, tmp) for seed in range(er.NSEED)]


@pytest.mark.parametrize("part", range(PARTS))
def test_random_scripts_under_a_random_partition(gpu_ctx, random_ref, random_host, pool, part):
    """every seed's script cut into calls by a generator of its own (cuts, entries merged or not), and again a call a block: both equal
    the host model in every row byte, map and status field and the whole end state, hence each other, and the fixture's digests"""
    from . import ext_random as er, ext_random_dev as ed
    q = iqd.IqDisplay(gpu_ctx, nchan=1)
    try:
        for seed in range(part * er.NSEED // PARTS, (part + 1) * er.NSEED // PARTS):
            lines = er.iqd_script(seed)
            nb = ic.nblocks(lines)
            cuts, merge = ed.partition("iqd", seed, nb)
            got = ic.run_script_dev(q, gpu_ctx, lines, pool, cuts=cuts, merge=merge)
            each = ic.run_script_dev(q, gpu_ctx, lines, pool, cuts=set(range(1, nb)))
            ed.iqd_same(got, random_host[seed], "seed %d" % seed, "cuts %s, merge %s" % (sorted(cuts), merge))
            ed.iqd_same(each, random_host[seed], "seed %d" % seed, "a call a block")
            assert np.array_equal(got["samp"], samp_of_rows(lines)) and np.array_equal(each["samp"], got["samp"]), (seed, "the row map's sample index")
            assert ic.stream(got) == ic.stream(each) and each["calls"] >= got["calls"]
            er.check_record("iqd", seed, lines, got, er.unpack(random_ref, seed))
    finally:
        q.close()


def _side_by_side(gpu_ctx, random_ref, random_host, pool, group, resident):
    from . import ext_random as er, ext_random_dev as ed
    seeds, scripts, steps, rng = ed.planned("iqd", group, resident)
    chans = [2, 0, 1]                                                      # not in channel order
    q = iqd.IqDisplay(gpu_ctx, nchan=3)
    try:
        got, calls, shared = ed.iqd_run_plan(q, gpu_ctx, steps, chans, scripts, pool, resident=resident, rng=rng)
    finally:
        q.close()
    for seed, lines, g in zip(seeds, scripts, got):
        ed.iqd_same(g, random_host[seed], "seed %d of %s" % (seed, seeds), "channel %d" % chans[seeds.index(seed)])
        assert np.array_equal(g["samp"], samp_of_rows(lines)), (seed, "the row map's sample index")
        er.check_record("iqd", seed, lines, g, er.unpack(random_ref, seed))
    # the calls were the plan's: tests/test_iqd_cpu.py::test_random_side_by_side_plans_share_their_calls holds the plans to their share
    assert (calls, shared) == ed.calls_of(steps)[:2]


@pytest.mark.parametrize("group", range(14))
def test_random_scripts_side_by_side(gpu_ctx, random_ref, random_host, pool, group):
    """the seeds three at a time on three channels of one object, out of order: every call carries every channel whose next blocks
    share the round's ns, a random number of blocks each, their entries shuffled into each other; the commands go between the calls.
    Each channel equals the host model of its own script in full, and the fixture"""
    _side_by_side(gpu_ctx, random_ref, random_host, pool, group, False)


@pytest.mark.parametrize("group", range(14))
def test_random_scripts_from_device_resident_input(gpu_ctx, random_ref, random_host, pool, group):
    """the same from ONE device buffer that holds every call's samples, uploaded ahead of the first call: an entry's samples stand at a
    stride larger than its blocks and -- entries of no block between them -- not at the row of its position among the entries that
    have some; the buffer is NaN outside the blocks; no copy to or from the device stands between two calls.  A gap: the row list
    itself (iq_row of kg_iqd_process_rows_) is the bank's, not part of the ABI, so here every entry still reads row i of its list, and
    the iq_row[i] branch of the host walk stays with tests/test_iqd_bank_gpu.py"""
    _side_by_side(gpu_ctx, random_ref, random_host, pool, group, True)
