"""What the five extension objects (kg_fftext, kg_iqd, kg_lorc, kg_fax, kg_cw) answer to a bad count, a bad index and a bad
connection list: the status and the text of kg_last_error, word for word.  The texts are literals taken from the sources as they
stood before the objects' host plumbing moved into csrc/kg_ext.h, so the test passes against a library of either side of that
change.  Every call here is refused on the host before anything is enqueued; objects have 2 connections, lists at most 2 entries
of 1 block."""
import ctypes as C

import numpy as np
import pytest

from flydog_sdr_gps_amd._lib import ptr

pytestmark = pytest.mark.gpu

INVALID = -2                                    # KG_ERR_INVALID
NS = 4                                          # samples of a sound block where the caller says (kg_iqd, kg_lorc)


def i32(*v):
    return np.array(v, np.int32)


def refused(lib, status, text):
    assert status == INVALID
    assert lib.kg_last_error().decode() == text


@pytest.fixture(scope="module")
def ext(gpu_ctx):
    """name -> handle of an object with 2 connections"""
    lib, made = gpu_ctx.lib, {}
    for name in ("fftext", "iqd", "lorc", "fax", "cw"):
        h = C.c_void_p()
        assert getattr(lib, "kg_%s_create" % name)(gpu_ctx.h, 2, C.byref(h)) == 0
        made[name] = h
    for c in (0, 1):                            # a list entry of these two is looked at only once its connection is initialised
        assert lib.kg_lorc_init(made["lorc"], c, 12000.0, 12000) == 0
        assert lib.kg_iqd_init(made["iqd"], c) == 0
        assert lib.kg_iqd_set_run(made["iqd"], c, 0, 12000.0) == 0
    yield made
    for name, h in made.items():
        getattr(lib, "kg_%s_destroy" % name)(h)


@pytest.mark.parametrize("name,noun,most", [("fftext", "nchan", 1024), ("iqd", "nchan", 1024), ("lorc", "nconn", 1024), ("fax", "nconn", 256),
                                            ("cw", "nconn", 256)])
def test_create_count(gpu_ctx, name, noun, most):
    lib = gpu_ctx.lib
    for count in (0, most + 1):
        h = C.c_void_p(1)
        refused(lib, getattr(lib, "kg_%s_create" % name)(gpu_ctx.h, count, C.byref(h)), "kg_%s_create: %s %d (1..%d)" % (name, noun, count, most))
        assert h.value is None                  # *out is cleared ahead of the count's check


def test_command_index(gpu_ctx, ext):
    lib = gpu_ctx.lib
    refused(lib, lib.kg_fftext_clear(ext["fftext"], 2), "kg_fftext_clear: channel 2 of 2")
    refused(lib, lib.kg_iqd_init(ext["iqd"], 2), "kg_iqd_init: channel 2 of 2")
    refused(lib, lib.kg_iqd_set_gain(ext["iqd"], 2, 0), "kg_iqd_set_gain: channel 2 of 2")
    refused(lib, lib.kg_lorc_init(ext["lorc"], 2, 12000.0, 12000), "kg_lorc_init: connection 2 of 2")
    refused(lib, lib.kg_lorc_start(ext["lorc"], 2), "kg_lorc_start: connection 2 of 2")
    refused(lib, lib.kg_fax_stop(ext["fax"], 2), "kg_fax_stop: connection 2 of 2")
    refused(lib, lib.kg_cw_stop(ext["cw"], 2), "kg_cw_stop: connection 2 of 2")
    refused(lib, lib.kg_cw_state(ext["cw"], 2, None), "kg_cw_state: connection 2 of 2")


# a list per case: (conns, entries, nblk, stride in samples) and the text behind "<entry point>: "
def list_cases(most_blk, unit, stride_name, head, index_text):
    return [((0, 0), 0, (1, 1), unit, head),
            ((2, 0), 1, (0, 0), unit, index_text),
            ((0, 1), 1, (most_blk + 1, 0), unit, "nblk[0] = %d (0..%d)" % (most_blk + 1, most_blk)),
            ((0, 1), 2, (1, 1), unit - 1, "%s %d below the 1 blocks of entry 0" % (stride_name, unit - 1))]


TWICE = ((1, 1), 2, (1, 1), None, "connection 1 is listed twice")


@pytest.mark.parametrize("case", list_cases(4096, 1024, "spec_stride", "nch 0 (1..65536), max_rows 1", None))
def test_fftext_list(gpu_ctx, ext, case):
    lib = gpu_ctx.lib
    conns, n, nblk, stride, text = case
    spec, rows, inst = np.zeros((2, 1024, 2), np.float32), np.zeros(1024, np.uint8), i32(0, 0)
    st = lib.kg_fftext_process(ext["fftext"], ptr(i32(*conns)), n, ptr(i32(*nblk)), ptr(inst), ptr(spec), stride, ptr(rows), 1024, 1, None, None, None, None)
    # the index is the one check the host-array call leaves to kg_fftext_process_dev, which it calls
    refused(lib, st, "kg_fftext_process: " + text if text else "kg_fftext_process_dev: chans[0] = 2 of 2")


@pytest.mark.parametrize("case", list_cases(4096, NS, "iq_stride", "nch 0 (1..4096), ns %d (1..512)" % NS, "chans[0] = 2 of 2"))
def test_iqd_list(gpu_ctx, ext, case):
    lib = gpu_ctx.lib
    conns, n, nblk, stride, text = case
    iq, rows, inst = np.zeros((2, NS, 2), np.float32), np.zeros(65536, np.uint8), i32(0, 0)
    status, row_map, sent = np.zeros(4 * 64, np.uint8), np.zeros(64 * 64, np.uint8), i32(0, 0)
    st = lib.kg_iqd_process(ext["iqd"], ptr(i32(*conns)), n, ptr(i32(*nblk)), ptr(inst), NS, ptr(iq), stride, ptr(rows), rows.size, ptr(status), 2, ptr(row_map), 64,
                            ptr(sent))
    refused(lib, st, "kg_iqd_process: " + text)


@pytest.mark.parametrize("case", list_cases(256, NS, "iq_stride", "nconn 0 (1..2)", "conns[0] = 2 of 2") + [TWICE])
def test_lorc_list(gpu_ctx, ext, case):
    lib = gpu_ctx.lib
    conns, n, nblk, stride, text = case
    iq, rows, row_map, nrows = np.zeros((2, NS, 2), np.float32), np.zeros(65536, np.uint8), np.zeros(64 * 64, np.uint8), i32(0)
    st = lib.kg_lorc_process(ext["lorc"], ptr(i32(*conns)), n, ptr(i32(*nblk)), NS, ptr(iq), NS if stride is None else stride, ptr(rows), rows.size, ptr(row_map), 64,
                             ptr(nrows))
    refused(lib, st, "kg_lorc_process: " + text)


@pytest.mark.parametrize("case", list_cases(256, 512, "stride", "nconn 0 (1..2)", "conns[0] = 2 of 2") + [TWICE])
def test_fax_list(gpu_ctx, ext, case):
    lib = gpu_ctx.lib
    conns, n, nblk, stride, text = case
    s16, srate, rows, recs, counts = np.zeros((2, 512), np.int16), np.full(2, 12000.0), np.zeros(4096, np.uint8), np.zeros(2 * 48, np.uint8), i32(*[0] * 8)
    st = lib.kg_fax_push(ext["fax"], ptr(i32(*conns)), n, ptr(i32(*nblk)), ptr(s16), 512 if stride is None else stride, ptr(srate), ptr(rows), 2048, ptr(recs), 1,
                         ptr(counts))
    refused(lib, st, "kg_fax_push: " + text)


@pytest.mark.parametrize("case", list_cases(256, 512, "stride", "nconn 0 (1..2)", "conns[0] = 2 of 2") + [TWICE])
def test_cw_list(gpu_ctx, ext, case):
    lib = gpu_ctx.lib
    conns, n, nblk, stride, text = case
    s16, now, evs, counts = np.zeros((2, 512), np.int16), np.zeros(2, np.uint32), np.zeros(2 * 64 * 24, np.uint8), i32(*[0] * 8)
    st = lib.kg_cw_push(ext["cw"], ptr(i32(*conns)), n, ptr(i32(*nblk)), ptr(s16), 512 if stride is None else stride, ptr(now), ptr(evs), 64, ptr(counts))
    refused(lib, st, "kg_cw_push: " + text)
