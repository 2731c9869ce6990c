"""Guard bands around a caller-visible device buffer (plain helper, imported like tests/fixtures.py).

A `Guarded` is ONE device allocation

    [ head | offset | row 0 | row 1 | ... | row nrows-1 | tail ]

whose rows are `stride_bytes` apart and of which a call may touch only the first `used` bytes of each row (or a byte range
of it).  Everything else is filled with one byte value, so that a stray write shows as a byte that is no longer the fill
(`violations`) and a stray read as a result that changes with the fill (run twice, 0x00 and 0xFF).  The bands lie inside
the test's own allocation: the point is to SEE a stray access, never to make one leave our memory -- head and tail are at
least 4096 bytes, and the rows never end flush with the allocation.

`ctx` is anything with alloc(nbytes) -> int, upload(dptr, host_array), download(dptr, host_array), free(dptr): a
flydog_sdr_gps_amd.Context, or the bytearray fake of tests/test_guarded_cpu.py.
"""
import numpy as np

MIN_GUARD = 4096


def _runs(bad, base=0):
    """bad: bool array -> [(first_offset, count)] of its runs of True"""
    if not bad.any():
        return []
    idx = np.flatnonzero(bad)
    cuts = np.flatnonzero(np.diff(idx) > 1)
    starts = np.concatenate(([idx[0]], idx[cuts + 1]))
    ends = np.concatenate((idx[cuts], [idx[-1]]))
    return [(int(s) + base, int(e - s + 1)) for s, e in zip(starts, ends)]


class Guarded:
    def __init__(self, ctx, nrows, row_bytes_used, stride_bytes, *, head=MIN_GUARD, tail=MIN_GUARD, offset_bytes=0, fill=0xA5):
        nrows, stride_bytes, offset_bytes = int(nrows), int(stride_bytes), int(offset_bytes)
        if head < MIN_GUARD or tail < MIN_GUARD:
            raise ValueError("guard bands are never below %d bytes" % MIN_GUARD)
        if nrows < 1 or offset_bytes < 0 or not 0 <= int(fill) <= 255:
            raise ValueError("bad layout")
        self.used = self._per_row(row_bytes_used, nrows)
        if max(self.used) > stride_bytes:
            raise ValueError("a row's used part (%d bytes) exceeds the stride (%d)" % (max(self.used), stride_bytes))
        self.ctx, self.nrows, self.stride = ctx, nrows, stride_bytes
        self.head, self.tail, self.offset, self.fill = int(head), int(tail), offset_bytes, int(fill)
        self.row0 = self.head + self.offset                       # offset of row 0 in the allocation
        self.nbytes = self.row0 + nrows * stride_bytes + self.tail
        self.base = ctx.alloc(self.nbytes)
        self.ptr = self.base + self.row0
        self.image = np.full(self.nbytes, self.fill, np.uint8)    # what the host last put there
        ctx.upload(self.base, self.image)

    @staticmethod
    def _per_row(v, nrows):
        if np.isscalar(v):
            return [int(v)] * nrows
        v = [int(x) for x in v]
        if len(v) != nrows:
            raise ValueError("one used size per row")
        return v

    def free(self):
        if self.base:
            self.ctx.free(self.base)
            self.base = 0

    def row_ptr(self, i):
        return self.ptr + i * self.stride

    def refill(self, fill):
        """the whole allocation, rows included, to one byte value"""
        self.fill = int(fill)
        self.image[:] = self.fill
        self.ctx.upload(self.base, self.image)

    def upload_rows(self, host_rows):
        """host_rows[i]: the bytes (any dtype) of row i's used part, at most the stride; nothing else is written"""
        if len(host_rows) != self.nrows:
            raise ValueError("one host row per row")
        for i, r in enumerate(host_rows):
            b = np.ascontiguousarray(r).reshape(-1).view(np.uint8)
            if b.size > self.stride:
                raise ValueError("row %d: %d bytes exceed the stride" % (i, b.size))
            if b.size:
                at = self.row0 + i * self.stride
                self.image[at:at + b.size] = b
                self.ctx.upload(self.base + at, b)

    def download_all(self):
        got = np.empty(self.nbytes, np.uint8)
        self.ctx.download(self.base, got)
        return got

    def _ranges(self, used):
        """used: one int for all rows, or per row an int (bytes [0, used)) or a (start, end) byte range"""
        if np.isscalar(used):
            used = [used] * self.nrows
        if len(used) != self.nrows:
            raise ValueError("one used extent per row")
        out = []
        for u in used:
            lo, hi = (0, int(u)) if np.isscalar(u) else (int(u[0]), int(u[1]))
            if hi <= lo:
                lo = hi = 0                                       # an empty row is guard over its whole stride
            if lo < 0 or hi > self.stride:
                raise ValueError("the allowed extent [%d, %d) leaves the row (stride %d)" % (lo, hi, self.stride))
            out.append((lo, hi))
        return out

    def download_rows(self, used_bytes_per_row):
        got = self.download_all()
        return [got[self.row0 + i * self.stride + lo:self.row0 + i * self.stride + hi].copy()
                for i, (lo, hi) in enumerate(self._ranges(used_bytes_per_row))]

    def violations(self, used_bytes_per_row, got=None):
        """-> [(region, row, first_offset, count)]: every run of bytes that no longer hold the fill in the head ("head", None,
        offset from the allocation's start), in the gaps of each row ("gap", row, offset from the row's start) and in the tail
        ("tail", None, offset from the end of the last row)."""
        if got is None:
            got = self.download_all()
        bad = got != self.fill
        out = [("head", None, o, c) for o, c in _runs(bad[:self.row0])]
        for i, (lo, hi) in enumerate(self._ranges(used_bytes_per_row)):
            at = self.row0 + i * self.stride
            out += [("gap", i, o, c) for o, c in _runs(bad[at:at + lo])]
            out += [("gap", i, o, c) for o, c in _runs(bad[at + hi:at + self.stride], hi)]
        end = self.row0 + self.nrows * self.stride
        out += [("tail", None, o, c) for o, c in _runs(bad[end:])]
        return out

    def changed(self):
        """for a buffer a call may only read: the runs of the allocation that differ from what the host put there"""
        return _runs(self.download_all() != self.image)


def freeze(v):
    """a result tree (arrays, numbers, tuples, lists, dicts) as plain comparable values: arrays by their BYTES, so that NaN == NaN
    and -0.0 != 0.0"""
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, dict):
        return tuple((k, freeze(v[k])) for k in sorted(v))
    if isinstance(v, (list, tuple)):
        return tuple(freeze(x) for x in v)
    if isinstance(v, (np.integer, np.floating)):
        return freeze(np.asarray(v))
    return v


def first_difference(a, b, path="result"):
    """where two frozen trees differ, as text (None: equal)"""
    if type(a) is not type(b):
        return "%s: %r against %r" % (path, type(a), type(b))
    if isinstance(a, tuple):
        if len(a) == 3 and isinstance(a[2], bytes) and isinstance(a[0], str):
            if a == b:
                return None
            if a[:2] != b[:2]:
                return "%s: %r against %r" % (path, a[:2], b[:2])
            x, y = np.frombuffer(a[2], np.uint8), np.frombuffer(b[2], np.uint8)
            at = int(np.flatnonzero(x != y)[0])
            return "%s: %s%s differs from byte %d on (%d bytes in all)" % (path, a[0], a[1], at, int((x != y).sum()))
        if len(a) != len(b):
            return "%s: %d against %d entries" % (path, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, "%s[%s]" % (path, x[0] if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], str) else i))
            if d:
                return d
        return None
    return None if a == b else "%s: %r against %r" % (path, a, b)


class Layout:
    """The buffers of ONE run of a containment case.  Guarded runs (tight=False): every stride is the used size plus an odd number
    of elements (rounded up only as far as `stride_mult` demands), row 0 sits at the smallest alignment the entry point accepts
    (`align` bytes and not 2 * align), and every byte outside the stated extents -- guard bands, row gaps, and the output rows
    themselves before the call -- holds `fill` in the buffers a call reads and the COMPLEMENT of it in the buffers it writes: a
    kernel that copies a gap byte of its input to the same place of its output would otherwise store the fill over the fill,
    unseen.  The tight run: stride = the used size, row 0 at 4096 bytes, zero-filled: the layout the parity tests use.  finish()
    asserts write containment for every buffer made."""

    def __init__(self, ctx, fill, tight=False):
        self.ctx, self.fill, self.tight = ctx, int(fill), bool(tight)
        self.fill_out = self.fill if tight else self.fill ^ 0xFF
        self.inputs, self.outputs, self.all = [], [], []

    def stride(self, used_elems, pad=3, mult=1):
        s = max(int(used_elems), 1) + (0 if self.tight else int(pad))
        return -(-s // mult) * mult

    def _make(self, nrows, used_bytes, stride_bytes, align, fill):
        g = Guarded(self.ctx, nrows, used_bytes, stride_bytes, offset_bytes=0 if self.tight else align, fill=fill)
        assert self.tight or (g.ptr % align == 0 and g.ptr % (2 * align) != 0)
        self.all.append(g)
        return g

    def inp(self, rows, align, pad=3, mult=1, stride=None, inplace=False, elem=None):
        """rows: one array per row (its used part; an element is one item of its dtype, or `elem` bytes) -> (Guarded, stride in
        elements)"""
        rows = [np.ascontiguousarray(r).reshape(-1) for r in rows]
        elem = rows[0].dtype.itemsize if elem is None else int(elem)
        st = self.stride(max(r.nbytes // elem for r in rows), pad, mult) if stride is None else int(stride)
        g = self._make(len(rows), [r.nbytes for r in rows], st * elem, align, self.fill)
        g.upload_rows(rows)
        (self.outputs if inplace else self.inputs).append(g)
        g.taken = not inplace
        return g, st

    def out(self, nrows, max_used_elems, elem_bytes, align, pad=3, mult=1, stride=None):
        """an output buffer, every byte prefilled -> (Guarded, stride in elements)"""
        st = self.stride(max_used_elems, pad, mult) if stride is None else int(stride)
        g = self._make(nrows, 0, st * elem_bytes, align, self.fill_out)
        self.outputs.append(g)
        g.taken = False
        return g, st

    def take(self, g, used_bytes_per_row):
        """after the call and a sync: W for this output, -> the used part of every row (uint8 arrays)"""
        got = g.download_all()
        bad = g.violations(used_bytes_per_row, got)
        assert bad == [], "stray writes (region, row, first offset, count): %s" % bad[:8]
        g.taken = True
        return [got[g.row0 + i * g.stride + lo:g.row0 + i * g.stride + hi].copy()
                for i, (lo, hi) in enumerate(g._ranges(used_bytes_per_row))]

    def finish(self):
        for g in self.outputs:
            assert g.taken, "an output buffer of the case was never checked"
        for g in self.inputs:
            ch = g.changed()
            assert ch == [], "an input buffer was written (first offset, count): %s" % ch[:8]

    def free(self):
        for g in self.all:
            g.free()


def contain(ctx, case):
    """W, R, P and E for one case: case(layout) makes its object from scratch, its buffers through the layout, calls the entry point,
    syncs and returns everything the contract promises (used parts through layout.take, counts, the state getters).  Run with
    fill 0x00 around the inputs (and 0xFF in the outputs), with 0xFF around the inputs (0x00 in the outputs) and on the tight layout:
    the three results are equal bit for bit."""
    res = []
    for fill, tight in ((0x00, False), (0xFF, False), (0x00, True)):
        lay = Layout(ctx, fill, tight)
        try:
            res.append(freeze(case(lay)))
            lay.finish()
        finally:
            lay.free()
    d = first_difference(res[0], res[1])
    assert d is None, "the result depends on bytes outside the stated input extents or on what the outputs held before (0x00 / 0xFF): " + d
    d = first_difference(res[0], res[2])
    assert d is None, "the guarded layout differs from the tight one: " + d
    return res[0]
