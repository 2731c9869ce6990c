"""The seeded random scripts and the AGC-window shapes of the audio post path (tests/post_random.py) on the CPU: the fixture
tests/golden/post_rand_ref.npz (tools/make_ref_post_golden.py --random, from tools/ref/ref_post_main.cpp: the reference's own
statements of rx/rx_sound.cpp:676-949 with every stage linked) holds what the generators draw now; the 40 seeds reach every condition
the fixture was made for; and the oracle (oracle/kiwi_oracle_post.c, kiwi_oracle_cfir.c: S-meter, CAgc, AM / NBFM detectors, CFir,
CSquelch) equals the reference's bytes on every block whose mode it models -- SSB, AM, NBFM, IQ -- which pins it at AGC window widths
(1, 2, 3, 4, 2^k and 2^k +- 1, 2047) it was never held to.  Every comparison is equality."""
import numpy as np
import pytest

from tests import post_random as C
from tests.script_common import digest


@pytest.fixture(scope="module")
def golden():
    return C.load()


@pytest.fixture(scope="module")
def scripts():
    return C.all_scripts()


@pytest.fixture(scope="module")
def samples():
    return C.pool()


def test_fixture_holds_what_the_generators_draw(golden, scripts, samples):
    assert digest(samples.tobytes()) == bytes(golden["pool_sha"]), "the pool changed: regenerate the fixture"
    assert samples.dtype == np.int16 and samples.shape == (len(C.SEGMENTS) * C.SEG, 2)
    assert not samples[C.AT["silence"]:C.AT["silence"] + C.SEG].any() and np.abs(samples[C.AT["full"]:C.AT["full"] + C.SEG]).min() == C.PEAK
    assert [str(n) for n in golden["names"]] == list(scripts), "a script was dropped or added"
    for name, lines in scripts.items():
        rec = C.unjoin(golden, name)
        assert digest("\n".join(lines).encode()) == bytes(rec["script_sha"]), (name, "the generator draws another script now")
    assert C.post_script(7) == C.post_script(7)


def test_seeds_come_in_batches_and_stay_inside_the_domain(scripts):
    for s in range(0, C.NSEED, C.GROUP):
        rate, ragged, lens = C.group_of(s)
        for k in range(C.GROUP):
            lines = scripts["r%02d" % (s + k)]
            assert float(lines[0].split()[1]) == rate and C.blocks_of(lines) == lens, (s, k)
            assert len(lens) <= 40
            if ragged:
                assert set(lens) <= set(C.RAGGED)
                assert not any(l.split()[0] in ("nbA", "nbE", "nbP") or l == "nrA %d" % C.NR_SPECTRAL for l in lines), (s, k, "Wild / spectral asserts 512")
            else:
                assert set(lens) == {C.BLK}
    kinds = {(C.group_of(s)[0], C.group_of(s)[1]) for s in range(0, C.NSEED, C.GROUP)}
    assert kinds == {(r, k) for r in C.RATES for k in (False, True)}


def test_random_fixture_meets_its_conditions(golden, scripts):
    feats = []
    for s in range(C.NSEED):
        name = "r%02d" % s
        feats.append(C.features(scripts[name], C.Record(C.unjoin(golden, name), name, scripts[name])))
    count, missing = C.check_conditions(feats)
    assert not missing, ("conditions reached by fewer than two of the %d seeds" % C.NSEED, {m: count[m] for m in missing})


def test_shapes_cover_the_window_edges(golden, scripts):
    """W and D as the reference's CAgc echoed them, not as the arithmetic says"""
    seen = {}
    for name in C.shape_names():
        lines = scripts[name]
        rec = C.Record(C.unjoin(golden, name), name, lines)
        rate, W, D = C.shape_wd(name)
        assert (int(rec.wd[0]), int(rec.wd[1])) == (W, D) and W == int(name[1:]), (name, rec.wd, W, D)
        seen[W] = D
        lens = C.blocks_of(lines)
        assert {b["mode"] for b in rec.blocks} == {C.M_USB, C.M_IQ} and all(b["agc_on"] for b in rec.blocks)
        assert {min(max(v, 1), C.BLK) for v in (W - 1, W, W + 1, D, D + 1, 1)} <= set(lens)
        half = sum(lens) // 2
        assert half >= 2 * max(W, D) and (W != 2047 or half > 2 * C.POST_CIRC), (name, half)
        assert [int(l.split()[1]) for l in lines if l.startswith("#K")] == [W - 1, W, W + 1] * 2
        assert len(lens) <= 40 or W == 2047
    assert sorted(seen) == [1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 2047]
    assert seen[2047] == 1706 > C.MAX_CALL           # every delayed sample of a call comes from the ring
    for name in C.FULL:
        assert "s16" in C.unjoin(golden, name) and "agc" in C.unjoin(golden, name)


# ---- the oracle beside the record --------------------------------------------------------------------------------------------
def bits(v):
    return np.float32(v).view(np.uint32)


def oracle_walk(ko, lines, x, rec):
    """Runs the oracle over a script; asserts equality with the record on every block of a mode it models.  -> blocks compared.
    A SAM-family block only advances what the oracle has of it (S-meter, CAgc).  m_am_ssb_deemp_FIR runs over the SAM demodulator's
    output in SAM / SAU / SAL, which the oracle does not have: from such a block on, blocks with that filter on are left out until the
    filter is set again (InitConstFir clears its samples)."""
    from flydog_sdr_gps_amd import deemp
    rate = float(lines[0].split()[1])
    r12k = C.snd_rate_of(rate) == 12000
    nominal = rate in (12000.0, 20250.0)
    agc, am_fir, de_fir, de_nfm_fir, sq = ko.Agc(), ko.CFir(), ko.CFir(), ko.CFir(), ko.Squelch()
    if nominal:
        sq.setup(rate); sq.set_squelch(0, 0)
    alpha = ko.smeter_alpha(rate)
    w = C.Walk()
    avg, z1, last, squelched, tainted = 0.0, 0.0, (0.0, 0.0), 0, False
    pos = k = compared = 0
    for l in lines[1:]:
        f = l.split()
        if l[0] == "#":
            continue
        if f[0] == "A":
            agc.set_parameters(*[int(v) for v in f[1:7]], rate)
        elif f[0] == "L":
            am_fir.init_lp(0, 1.0, 50.0, float(f[1]), float(f[2]), rate)
        elif f[0] == "Q":
            sq.set_squelch(int(f[1]), int(f[2]))
        elif f[0] == "E":
            if int(f[1]):
                de_fir.init_const(deemp.table(0, r12k)[int(f[1]) - 1], rate)
                tainted = False
            if int(f[2]):
                de_nfm_fir.init_const(deemp.table(1, r12k)[int(f[2]) - 1], rate)
        if f[0] != "P":
            w.line(l)
            continue
        for n in (int(v) for v in f[1:]):
            xs = x[pos:pos + n]
            pos += n
            b = rec.blocks[k]
            where = (rec.name, k, C.MODE_NAMES[w.mode], n)
            avg, taps = ko.smeter_process(avg, alpha, xs)
            assert bits(avg) == bits(rec.smeter[k, 0]), (where, "sMeterAvg_dB", avg, rec.smeter[k, 0])
            assert np.float32(taps[0]) + C.S_METER_CAL == rec.smeter[k, 1], (where, "S-meter tap j = 0")
            assert n < 2 or np.float32(taps[1]) + C.S_METER_CAL == rec.smeter[k, 2], (where, "S-meter tap j = n / 2")
            s16 = None
            if w.sam:
                agc.process_cpx(xs)
                tainted |= bool(w.de) and not w.stereo
            elif w.mode == C.M_IQ:
                got = agc.process_cpx(xs)
                assert digest(np.ascontiguousarray(got, np.complex64).tobytes()) == b["agc"], (where, "agc_samps_c")
                compared += 1
            elif w.mode == C.M_USB:
                s16 = agc.process_s16(xs)
            elif w.mode == C.M_AM:
                d, z1 = ko.am_detect(z1, agc.process_cpx(xs))
                s16 = am_fir.process_rm(d)
            else:
                assert w.mode == C.M_NBFM
                d, last = ko.nbfm_detect(last, agc.process_cpx(xs))
                s16, rc = sq.perform_fm(d)
                if rc:
                    squelched = int(rc == 1)
                assert squelched == rec.squelched(k), (where, "s->squelched")
            if s16 is not None:
                if w.mode == C.M_NBFM:
                    if w.de_nfm:
                        s16 = de_nfm_fir.process_mm(s16)
                elif w.de:
                    s16 = None if tainted else de_fir.process_mm(s16)
            if s16 is not None:
                assert digest(np.ascontiguousarray(s16, np.int16).tobytes()) == b["pre"], (where, "out_samps_s2 ahead of the Wild stage")
                if rec.name in C.FULL:
                    at = sum(c["n"] for c in rec.blocks[:k] if c["pre"] is not None)
                    assert np.array_equal(s16, rec.full["s16"][at:at + n]), where
                compared += 1
            k += 1
    assert k == len(rec.blocks) and pos == len(x)
    return compared


def test_oracle_equals_the_reference_on_every_block_it_models(oracle, golden, scripts, samples):
    total = 0
    for name, lines in scripts.items():
        rec = C.Record(C.unjoin(golden, name), name, lines)
        x = C.as_complex(C.script_input(lines, samples))
        n = oracle_walk(oracle, lines, x, rec)
        assert name[0] != "w" or n == len(rec.blocks), (name, "every block of a shape is SSB or IQ")
        total += n
    assert total >= 400, total
