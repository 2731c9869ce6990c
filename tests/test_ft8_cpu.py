"""kg_ft8.h, stage 1 of the FT8 / FT4 extension (extensions/FT8/ft8_lib: decode_ft8.c:503-620, common/monitor.c:55-203,
ft8/decode.c:63-328, :393-485) as the host twin runs it, compiled with g++ -O2 -ffp-contract=off in tools/ft8_host_driver.cpp, against
tests/golden/ft8_ref.npz (made by tools/make_ref_ft8_golden.py from the reference's own statements).  The twin's transform here is the
double-precision DFT of tools/ref/ft8_harness.h, so it must equal the golden's build B in every record: schedule, events, waterfall
bytes, max_mag, candidates in the heap's order, log174 by its bits (NaN included), the end state and last_frame.  (With the reference's
kiss_fftr the twin wrote build A's records byte for byte when the golden was made: profiles/ft8_golden.txt.)  Also: the golden's own
conditions, the scenes rebuilt from their seeds, the refusals, two mutations the golden must notice, the prototypes."""
import os
import re

import numpy as np
import pytest

from . import ft8_common as F

ROOT = F.ROOT
FT8_SYMBOLS = {
    "kg_ft8_create": ("int kg_ft8_create(kg_ctx *ctx, int nconn, kg_ft8 **out);", 3),
    "kg_ft8_destroy": ("void kg_ft8_destroy(kg_ft8 *q);", 1),
    "kg_ft8_set_snr_adj": ("int kg_ft8_set_snr_adj(kg_ft8 *q, float snr_adj);", 2),
    "kg_ft8_init": ("int kg_ft8_init(kg_ft8 *q, int conn, int protocol, double snd_rate);", 4),
    "kg_ft8_push": ("int kg_ft8_push(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, int ns, const int16_t *samples, size_t sample_stride, const double *times,", 15),
    "kg_ft8_plan": ("int kg_ft8_plan(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, int ns, const double *times, size_t time_stride, int32_t *nblocks,", 10),
    "kg_ft8_state": ("int kg_ft8_state(kg_ft8 *q, int conn, kg_ft8_info *info, float *last_frame, uint8_t *mag, int previous);", 6),
    "kg_ft8_load_wf": ("int kg_ft8_load_wf(kg_ft8 *q, int conn, int protocol, int num_blocks, const uint8_t *mag, int num_candidates, int min_score, kg_ft8_slot *slot);", 8),
    "kg_rxbank_ft8_init": ("int kg_rxbank_ft8_init(struct kg_rxbank *bank, int rx, int protocol, double snd_rate);", 4),
    "kg_rxbank_ft8_start": ("int kg_rxbank_ft8_start(struct kg_rxbank *bank, int rx);", 2),
    "kg_rxbank_ft8_stop": ("int kg_rxbank_ft8_stop(struct kg_rxbank *bank, int rx);", 2),
    "kg_rxbank_ft8_set_now": ("int kg_rxbank_ft8_set_now(struct kg_rxbank *bank, double now);", 2),
    "kg_rxbank_ft8": ("kg_ft8 *kg_rxbank_ft8(struct kg_rxbank *bank);", 1),
    "kg_rxbank_ft8_out": ("int kg_rxbank_ft8_out(struct kg_rxbank *bank, kg_ft8_slot **d_slots, kg_ft8_ev *evs, int max_events, int32_t *nevents, int32_t *rx_of_slot, int max_slots);", 7),
}


@pytest.fixture(scope="module")
def golden():
    return F.load()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return F.build_driver(tmp_path_factory.mktemp("ft8"))


def test_golden_file_meets_its_conditions(golden):
    F.golden_conditions(golden, os.path.getsize(os.path.join(F.GOLD, "ft8_ref.npz")))


def test_scenes_rebuild(golden):
    """the seeded waterfalls and streams are the ones the reference binary was fed"""
    for name in F.LOADS:
        assert F.digest(F.scene_bytes(name)) == bytes(golden["l_%s_sha" % name]), name
    for name in F.STREAMS:
        assert F.digest(F.scene_bytes(name)) == bytes(golden["s_%s_sha" % name]), name


@pytest.mark.parametrize("name", sorted(F.LOADS))
def test_twin_equals_the_golden_on_a_waterfall(golden, driver, tmp_path, name):
    got = F.run_exe(driver, F.scene_bytes(name), tmp_path)
    assert len(got["slots"]) == 1 and not got["events"] and got["end"] is None
    F.same_slot(got["slots"][0], golden, "l_%s_" % name, F.LDPC_N if name == F.FULL_LOG else F.KEEP, name)
    p = F.LOADS[name][0]
    sz = golden["sizes_" + F.pname(p)]
    assert [got["sizes"][f] for f in ("block", "nfft", "num_bins", "min_bin", "max_blocks", "num_samples", "block_stride", "subblock")] == [int(v) for v in sz[:8]]
    assert F.bits(got["window"]).tobytes() == F.bits(golden["window_" + F.pname(p)]).tobytes()        # sinf of the host libm, as the reference's


@pytest.mark.parametrize("name", sorted(F.STREAMS))
def test_twin_equals_the_golden_on_a_stream(golden, driver, tmp_path, name):
    got = F.run_exe(driver, F.scene_bytes(name), tmp_path)
    k = "s_%s_" % name
    assert np.array_equal(np.array(got["events"], np.int64).reshape(-1, 5), golden[k + "events"]), (name, "events")
    assert np.array_equal(got["end"]["state"], golden[k + "state"]), (name, "tsync, in_pos, frame_pos, num_blocks, slot, decode_time")
    assert F.digest(got["end"]["last_frame"].tobytes()) == bytes(golden[k + "last_frame_sha"]), (name, "last_frame")
    want = golden[k + "end_mag"].copy()
    want[golden[k + "end_ab_idx"]] = golden[k + "end_ab_val"]              # build B's bytes: build A's, and where the two differ
    assert np.array_equal(got["end"]["mag"], want), (name, "the waterfall bytes of the slot under way")
    mm = np.array([s["max_mag"] for s in got["slots"]] + [got["end"]["max_mag"]], np.float32)
    assert F.bits(mm).tobytes() == F.bits(golden[k + "max_mag_b"]).tobytes(), (name, "max_mag")
    assert len(got["slots"]) == (1 if k + "b_head" in golden else 0)
    for sl in got["slots"]:
        F.same_slot(sl, golden, k + "b_", F.KEEP, name)
        assert F.digest(sl["mag"].tobytes()) == bytes(golden[k + "slot_mag_sha_b"]), (name, "the slot's waterfall bytes")
        ev = [e for e in got["events"] if e[1] == 1][0]
        assert ev[2] == F.SIZES[F.STREAMS[name][0]]["slot_blocks"] == sl["num_blocks"]
    if name.startswith("silence"):
        assert not got["end"]["mag"].any() and got["end"]["max_mag"] == np.float32(-120.0)


def test_schedule_edges(driver, tmp_path):
    """a callback just inside the first quarter of a slot syncs (the comparison of decode_ft8.c:515 is >), one beyond does not; slot_start and
    decode_time are the clock's; a protocol change begins again: slot 0, not synced"""
    p = F.FT8
    x = np.zeros((3, F.NS), np.int16)
    for t, synced in ((15.0 * 7 + 0.8125 + 3.75 - 1.0 / 64, 1), (15.0 * 7 + 0.8125 + 3.75, 0)):
        got = F.run_exe(driver, F.stream_bytes(p, x, [t, t, t]), tmp_path)
        assert int(got["end"]["state"][0]) == synced and len(got["events"]) == synced
    t0 = 15.0 * 9 + 0.8125
    got = F.run_exe(driver, F.stream_bytes(p, x, F.clock(t0, 3)), tmp_path)
    assert got["events"] == [(0, 0, 1, int(np.floor(t0)), 135)] and [int(v) for v in got["end"]["state"]] == [1, 3 * F.NS, 0, 0, 1, int(np.floor(t0))]
    got = F.run_exe(driver, F.stream_bytes(p, x, F.clock(t0, 3), reinit_at=2, reinit_protocol=F.FT4), tmp_path)
    assert got["events"] == [(0, 0, 1, 135, 135), (2, 0, 1, 135, 135)] and [int(v) for v in got["end"]["state"][:5]] == [1, F.NS, 0, 0, 1] and got["end"]["nfft"] == 1152


REFUSALS = {"ns_2049": (F.stream_bytes(F.FT8, np.zeros((1, 2049), np.int16), [100.0]), 6), "time_nan": (F.stream_bytes(F.FT8, np.zeros((1, 64), np.int16), [np.nan]), 13),
            "time_negative": (F.stream_bytes(F.FT8, np.zeros((1, 64), np.int16), [-1.0]), 13), "time_inf": (F.stream_bytes(F.FT4, np.zeros((1, 64), np.int16), [np.inf]), 13),
            "candidates_0": (F.load_bytes(F.FT8, np.zeros((2, 2, 2, 481), np.uint8), 0, 10), 5), "candidates_141": (F.load_bytes(F.FT4, np.zeros((2, 2, 2, 145), np.uint8), 141, 10), 5),
            "blocks_94": (F.load_bytes(F.FT8, np.zeros((94, 2, 2, 481), np.uint8)), 4), "protocol_2": (F.load_bytes(2, np.zeros((2, 2, 2, 481), np.uint8)), 11)}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(driver, tmp_path, name):
    scene, status = REFUSALS[name]
    F.run_exe(driver, scene, tmp_path, expect=status)


def test_neighbours_of_the_refusals_are_taken(driver, tmp_path):
    got = F.run_exe(driver, F.stream_bytes(F.FT8, np.zeros((1, 2048), np.int16), [0.0]), tmp_path)
    assert int(got["end"]["state"][0]) == 1 and int(got["end"]["state"][3]) == 1          # time 0 syncs (fmod of a negative is negative), 2048 samples: one block
    got = F.run_exe(driver, F.load_bytes(F.FT8, np.zeros((93, 2, 2, 481), np.uint8), 1, 0), tmp_path)
    assert got["slots"][0]["ncand"] == 1


# the scene that must notice each mutation
MUTATIONS = {"KG_FT8_MUT_EVICT": "load_c_ft8", "KG_FT8_MUT_TAIL": "boundary_ft4"}


@pytest.mark.parametrize("define", sorted(MUTATIONS))
def test_the_golden_notices_a_mutated_twin(golden, tmp_path, define):
    name = MUTATIONS[define]
    got = F.run_exe(F.build_driver(tmp_path, defines=(define,)), F.scene_bytes(name), tmp_path)
    if name in F.LOADS:
        assert got["slots"][0]["cand"].tobytes() != np.ascontiguousarray(golden["l_%s_cand" % name]).tobytes()
    else:
        k = "s_%s_" % name
        want = golden[k + "end_mag"].copy()
        want[golden[k + "end_ab_idx"]] = golden[k + "end_ab_val"]
        assert not np.array_equal(got["end"]["mag"], want)


def test_ft8_symbols_declared_bound_and_exported():
    """the prototypes rule of tests/test_wspr_cpu.py, on include/kiwigpu_ft8.h"""
    from flydog_sdr_gps_amd import _lib, ft8
    import flydog_sdr_gps_amd
    assert flydog_sdr_gps_amd.Ft8 is ft8.Ft8
    header = open(os.path.join(ROOT, "include", "kiwigpu_ft8.h")).read()
    assert '#include "kiwigpu_ft8.h"' in open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load_library()
    for s, (proto, nargs) in FT8_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.FT8_SYMBOLS and len(_lib.FT8_SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
    protos = re.findall(r"\b(kg_\w*)\s*\(([^;{}()]*)\)\s*;", bare)
    assert sorted(n for n, _ in protos) == sorted(FT8_SYMBOLS)
    for n, a in protos:
        assert not re.search(r"\bvoid\s*\*", a), (n, "every pointer is typed")
        assert not re.search(r"(?<!\*)\*\s*d_\w+", a), (n, "no parameter is a single pointer named d_...")
        assert len(a.split(",")) == FT8_SYMBOLS[n][1], n
    for s in FT8_SYMBOLS:                                                     # every prototype cites the reference lines it replaces
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void|kg_ft8 \*)\s*%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    d = {k: int(v) for k, v in re.findall(r"#define KG_FT8_(\w+)\s+(\d+)", header)}
    assert (d["MAX_CAND"], d["MIN_SCORE"], d["LDPC_N"], d["MAX_NS"], d["MAX_NFFT"], d["MAX_WF"]) == (ft8.MAX_CAND, ft8.MIN_SCORE, ft8.LDPC_N, ft8.MAX_NS, ft8.MAX_NFFT, ft8.MAX_WF)
    assert (ft8.MAX_CAND, ft8.MIN_SCORE, ft8.LDPC_N) == (F.MAX_CAND, F.MIN_SCORE, F.LDPC_N) and ft8.cand_dtype == F.cand_dtype
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_ft8.h")).read()
    assert "{3, 1, 4, 0, 6, 5, 2}" in src and "{0, 1, 3, 2, 5, 6, 4, 7}" in src and tuple(F.COSTAS8) == (3, 1, 4, 0, 6, 5, 2)
