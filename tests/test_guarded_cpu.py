"""The guard-band helper itself (tests/guarded.py) against a fake context whose device memory is a bytearray: every planted
violation is reported with its region, row and offset, and a clean run reports nothing -- the net has no holes."""
import numpy as np
import pytest

from tests.guarded import Guarded, MIN_GUARD


class FakeCtx:
    """alloc / upload / download / free over one bytearray; addresses are offsets into it plus a base"""
    BASE = 0x10000

    def __init__(self):
        self.mem = bytearray()
        self.allocs = {}

    def alloc(self, nbytes):
        at = self.BASE + len(self.mem)
        self.mem += bytes(int(nbytes))
        self.allocs[at] = int(nbytes)
        return at

    def free(self, dptr):
        del self.allocs[dptr]

    def _span(self, dptr, n):
        for at, size in self.allocs.items():
            if at <= dptr and dptr + n <= at + size:
                return dptr - self.BASE
        raise AssertionError("access outside every allocation")

    def upload(self, dptr, host):
        b = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
        o = self._span(dptr, b.size)
        self.mem[o:o + b.size] = b.tobytes()

    def download(self, dptr, host):
        o = self._span(dptr, host.nbytes)
        host.reshape(-1).view(np.uint8)[:] = np.frombuffer(bytes(self.mem[o:o + host.nbytes]), np.uint8)

    def poke(self, dptr, data):
        """what a stray kernel store would do"""
        self.upload(dptr, np.frombuffer(bytes(data), np.uint8))


USED, STRIDE, NROWS = [40, 24, 0], 56, 3


@pytest.fixture
def g():
    ctx = FakeCtx()
    g = Guarded(ctx, NROWS, USED, STRIDE, offset_bytes=8, fill=0xA5)
    g.upload_rows([np.arange(u, dtype=np.uint8) for u in USED])
    return g


def test_layout(g):
    assert g.ptr == g.base + MIN_GUARD + 8
    assert g.nbytes == MIN_GUARD + 8 + NROWS * STRIDE + MIN_GUARD
    assert g.row_ptr(2) == g.ptr + 2 * STRIDE
    # upload_rows wrote the used parts and nothing else
    img = g.download_all()
    assert np.array_equal(img, g.image) and g.changed() == []
    assert np.count_nonzero(img != 0xA5) == sum(np.count_nonzero(np.arange(u, dtype=np.uint8) != 0xA5) for u in USED)
    rows = g.download_rows(USED)
    assert [r.size for r in rows] == USED and np.array_equal(rows[0], np.arange(40, dtype=np.uint8))


def test_clean_run_reports_nothing(g):
    assert g.violations(USED) == []
    # a legitimate write inside a used part, fill-valued or not, is no violation
    g.ctx.poke(g.row_ptr(1) + 23, b"\x00")
    assert g.violations(USED) == []
    assert g.changed() == [(MIN_GUARD + 8 + STRIDE + 23, 1)]


def test_one_byte_behind_the_used_part_of_row_1(g):
    g.ctx.poke(g.row_ptr(1) + 24, b"\x00")
    assert g.violations(USED) == [("gap", 1, 24, 1)]


def test_sixteen_bytes_straddling_the_end_of_the_last_row(g):
    g.ctx.poke(g.row_ptr(2) + STRIDE - 6, bytes(16))
    assert g.violations(USED) == [("gap", 2, STRIDE - 6, 6), ("tail", None, 0, 10)]


def test_write_into_the_head(g):
    g.ctx.poke(g.ptr - 3, b"\x01\x02")                      # inside the offset bytes in front of row 0
    g.ctx.poke(g.base + 100, b"\x07")
    assert g.violations(USED) == [("head", None, 100, 1), ("head", None, MIN_GUARD + 8 - 3, 2)]


def test_row_with_nothing_used_is_checked_over_its_whole_stride(g):
    g.ctx.poke(g.row_ptr(2), b"\x00")
    g.ctx.poke(g.row_ptr(2) + STRIDE - 1, b"\x00")
    assert g.violations(USED) == [("gap", 2, 0, 1), ("gap", 2, STRIDE - 1, 1)]
    # a count of 0 given as a range is the same thing
    assert g.violations([40, 24, (6, 6)]) == [("gap", 2, 0, 1), ("gap", 2, STRIDE - 1, 1)]


def test_bytes_in_front_of_a_range_are_guard_too(g):
    g.ctx.poke(g.row_ptr(0) + 3, b"\x00")
    # row 0 holds 0, 1, 2, .. from upload_rows: bytes 0..7 are all non-fill once they count as guard
    assert g.violations([(8, 40), 24, 0]) == [("gap", 0, 0, 8)]
    g.refill(0xA5)
    g.ctx.poke(g.row_ptr(0) + 3, b"\x00")
    g.ctx.poke(g.row_ptr(0) + 40, b"\x00")
    assert g.violations([(8, 40), 24, 0]) == [("gap", 0, 3, 1), ("gap", 0, 40, 1)]


def test_a_fill_valued_stray_write_needs_the_other_fill(g):
    """a stray store of the fill value itself is invisible to one run: the tests run every case with 0x00 AND 0xFF"""
    g.ctx.poke(g.row_ptr(0) + 41, b"\xa5")
    assert g.violations(USED) == []
    g.refill(0x00)
    g.ctx.poke(g.row_ptr(0) + 41, b"\xa5")
    assert g.violations(USED) == [("gap", 0, 41, 1)]


def test_refusals():
    ctx = FakeCtx()
    with pytest.raises(ValueError):
        Guarded(ctx, 2, 8, 16, head=64)                     # guards are never below 4096 bytes
    with pytest.raises(ValueError):
        Guarded(ctx, 2, 8, 16, tail=0)                      # never flush against the end of the allocation
    with pytest.raises(ValueError):
        Guarded(ctx, 2, 24, 16)                             # used part beyond the stride
    g = Guarded(ctx, 2, 8, 16)
    with pytest.raises(ValueError):
        g.violations([8, 17])
    with pytest.raises(ValueError):
        g.upload_rows([np.zeros(17, np.uint8), np.zeros(1, np.uint8)])
